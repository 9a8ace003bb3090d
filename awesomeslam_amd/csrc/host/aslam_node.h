// aslam_node.h -- host-side mirror of the reference's filter nodes, ROS-free.
//
// aslam::EKFSlam / aslam::UKFSlam keep the reference's class and member names
// (awesome_slam/src/ekf/ekf.h:71-131, awesome_slam/src/ukf/ukf.h:84-143): the callbacks, the data
// association and the landmark bookkeeping (ekf.cpp:74-290, ukf.cpp:70-257) run on the host exactly as
// in the reference, while `param.P`, `param.X` and slam() live on the MI355X behind the C ABI of
// include/aslam_core.h (per-callback seam: aslam_grow + aslam_ekf_step / aslam_ukf_step).
// Messages are plain structs with the fields the nodes read; ros/ekf_node.cpp and ros/ukf_node.cpp
// (compile-gated on catkin) wrap them into the real ROS callbacks.
//
// This is product code: it never touches oracle/.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/aslam_core.h"

namespace aslam
{
/// the fields of nav_msgs/Odometry the nodes read (ekf.cpp:139-142,94)
struct Odometry
{
        double px, py;         // pose.pose.position.{x,y}
        double qw, qx, qy, qz; // pose.pose.orientation
        double vx, wz;         // twist.twist.linear.x, twist.twist.angular.z
};

/// awesome_slam_msgs/Landmarks (msg/Landmarks.msg:1-2)
struct Landmarks
{
        std::vector<double> x, y;
};

/// structures.h:85-112
struct LaserData
{
        float range;
        float bearing;
};

/// tools.h:44-50 / 62-66 (binary32)
float normalizeAngle(float theta);
float quat2euler(float w, float x, float y, float z);

class FilterNode
{
      public:
        /// `now_init` stands for the ros::Time::now().toSec() of initialize() (ekf.cpp:54 / ukf.cpp:54): it seeds the binary32 last_time
        FilterNode(int filter, int max_landmark_count, int device, double now_init = 0.0);
        virtual ~FilterNode();
        FilterNode(const FilterNode &) = delete;
        FilterNode &operator=(const FilterNode &) = delete;

        /// ekf.cpp:102-114 / ukf.cpp:98-110
        void cbSensorLandmark(const Landmarks &msg);
        /// ekf.cpp:74-99 / ukf.cpp:70-95; `now` stands for ros::Time::now().toSec().  Returns false when the
        /// callback returned early (no sensor message yet).  Throws std::runtime_error if the core fails.
        bool cbOdom(const Odometry &msg, double now);
        /// same with delta_time given instead of derived from the clock
        bool cbOdomDt(const Odometry &msg, float delta_time);
        /// convertToLandmarkMsg(N, param.X), common.h:93-108: what the node publishes on out/landmarks/kalman
        Landmarks landmarks() const;

        uint32_t dim() const
        {
                return N;
        }
        const std::vector<double> &X() const
        {
                return param_X;
        }
        const std::vector<double> &Z() const
        {
                return param_Z;
        }
        double A00() const
        {
                return a00;
        }
        double A10() const
        {
                return a10;
        }
        const std::vector<std::pair<LaserData, uint32_t>> &waitList() const
        {
                return new_landmark_wait;
        }
        aslam_ctx *core() const
        {
                return ctx;
        }
        bool growthRefused() const
        {
                return growth_refused;
        }
        /// the innovation statistics of the last odometry callback (aslam_innovation_enable / aslam_get_innovation of the core): y^T S^-1 y and
        /// ln |det S| of its slam(), NaN when the callback returned before slam().  Off by default; innovation() throws while it is off.
        /// A deliberate trade-off: aslam_node.cpp binds these two entry points of the core WEAKLY, so that the mirror still links against a
        /// stand-in core without them (the oracle-backed one of tests/sanitize/); the price is that a core library lacking them is refused
        /// here, at run time ("this core has no innovation record"), not by the linker.
        void enableInnovation(bool on);
        void innovation(double &nis, double &logdet) const;
        /// The sighted-only update (aslam_sighted_update_enable, aslam_core.h; EKF): slam() then uses the rows of the landmarks this callback's own
        /// association sighted -- the mask updateZ records next to hits() -- through aslam_ekf_step_sighted.  Bound weakly, as the record above.
        void setSightedOnly(bool on);
        const std::vector<uint8_t> &sighted() const
        {
                return lm_sighted;
        }
        /// The noise and association parameters (aslam_params, aslam_core.h; the reference's config.h constants by default).  The mirror's own
        /// association and wait-list use assoc_dist and promote_count; everything else lives in the core's record of this filter.  Meant to be
        /// called before the first callback: the core is then initialised again so that p0_pose applies; later calls change R, Q, var_a,
        /// assoc_dist and p0_landmark from the next callback on and leave P alone.  Throws on a refused field (the message names it) and, with
        /// a core that lacks aslam_set_params (bound weakly, like the innovation record; aslam_reset with it), on anything but the defaults -- such
        /// a core validates nothing: the record is only compared, byte for byte, with the default table.
        void setParams(const aslam_params &p);
        const aslam_params &params() const
        {
                return prm;
        }
        /// Forget the landmarks with these indices (0-based, as landmarks() lists them): aslam_remove_landmarks on the core, and the host copies
        /// of X and Z compacted the same way -- survivors keep their order.  Between two callbacks.  The wait-list and the stored sensor message
        /// stay: a later sighting of a removed landmark is an unassociated observation like any other (see aslam_core.h).  Throws on an index
        /// out of range (nothing is removed then) and with a core that lacks the entry point (bound weakly, like the innovation record).
        void removeLandmarks(const std::vector<int> &indices);
        /// The sighting record of aslam_core.h (aslam_get_sightings), kept here because this mirror does the association itself: the clock counts the
        /// callbacks in which updateZ ran, lastSeen()[i] is the clock of the last one that associated an observation with landmark i (of its promotion
        /// before the first), hits()[i] counts them.  removeLandmarks moves the records with their landmarks and keeps the clock.
        uint32_t clock() const
        {
                return sight_clock;
        }
        const std::vector<uint32_t> &lastSeen() const
        {
                return lm_seen;
        }
        const std::vector<uint32_t> &hits() const
        {
                return lm_hits;
        }
        /// removeLandmarks of every landmark whose age, clock() - lastSeen()[i] in unsigned 32-bit arithmetic, exceeds max_age; returns how many went
        int removeStale(uint32_t max_age);
        /// Fuse duplicate landmarks (aslam_merge_landmarks of aslam_core.h): each pair (i, j), i < j, applies "i and j are the same point" (with
        /// noise_var on the constraint's diagonal) to X and P on the core and drops j; the mirror's lastSeen / hits fuse by the core's rule (hits
        /// add up, the younger last_seen stays), its X is read back and its Z compacted.  Returns the pairs fused; throws where the core refuses
        /// (nothing has changed then).  Between two callbacks.
        int mergeLandmarks(const std::vector<std::pair<int, int>> &pairs, double noise_var = 0.0);
        /// aslam_select_duplicates' rule, evaluated here on the state read back from the core (one filter; the arithmetic of aslam_core.h operation
        /// by operation, so the selection is the device selector's), then mergeLandmarks; passes until one merges nothing, 4 at the most.
        /// Returns the landmarks merged.
        int mergeDuplicates(double gate, double max_dist, double noise_var = 0.0);
        /// Join a foreign map (aslam_join_maps of aslam_snapshot.h): the landmarks of record `record` of the HOST snapshot blob, with their
        /// covariance block, go behind this filter's state as an independent map.  frame12 (may be null: identity, zero covariance) holds
        /// tx, ty, phi and the row-major 3 x 3 covariance of the transform source frame -> this filter's frame; select (may be null: every
        /// landmark) holds select_len entries, one per landmark of the record.  The mirror's X and Z are read back, the new landmarks enter
        /// lastSeen / hits as promoted ones do.  Returns the landmarks joined; throws where the core refuses (nothing has changed then: before
        /// the first callback, no room below max_landmark_count, a malformed blob or frame).  Between two callbacks.
        int joinMap(const void *blob, int64_t bytes, int record = 0, const double *frame12 = nullptr, const uint8_t *select = nullptr, int select_len = 0);
        /// Mahalanobis-gated association (aslam_gate_observations of aslam_core.h).  gate = 0, the default: off, updateZ associates by the
        /// reference's Euclidean rule alone.  gate > 0 (9.21: the 99 % point of chi-square with 2 degrees of freedom), once a landmark is mapped:
        /// updateZ asks the core for the gated landmark of every observation of the stored message in ONE call and copies the indices back (4
        /// bytes per observation; P stays on the device).  An observation the gate accepts goes to that landmark; one it refuses although the
        /// Euclidean rule (best_d < assoc_dist) would have associated it is DROPPED -- neither a match nor evidence for a new landmark, which
        /// is what keeps drift from promoting duplicates -- and counted in assocRejected(); every other one goes to the wait-list as before
        /// (the wait-list stays Euclidean: its entries have no covariance).  The gate is evaluated at the state the last callback left on
        /// the device: the motion of one odometry period is not added.  Throws on a negative or NaN gate, and at the first gated callback with
        /// a core that lacks the entry point or without the HIP runtime in the process (both bound weakly, like the innovation record).
        void setAssocGate(double gate);
        double assocGate() const
        {
                return assoc_gate;
        }
        uint64_t assocRejected() const
        {
                return assoc_rejected;
        }
        /// Joint compatibility behind the gate (aslam_joint_compat of aslam_core.h).  prob = 0, the default: off.  prob in (0, 1), while the
        /// gate above is > 0: the pairings the gate accepted for a message are tested as a set, in message order, in place on the same device
        /// array (aslam_gate_observations -> aslam_joint_compat, one copy back), against the chi-square points of probability `prob` for 2, 4,
        /// ... degrees of freedom (aslam_chi2_point; the table is rebuilt by this call, not per callback).  A pairing the joint test refuses
        /// is handled like one the gate refuses within assoc_dist: DROPPED, neither a match nor wait-list evidence, and counted in
        /// jointRejected().  The decisions depend on the order of the message.  Messages of more than ASLAM_JC_MAX_OBS observations are
        /// refused by the core (the callback throws).  With the joint test off the mirror computes bit for bit what it did without it.
        /// Throws on a prob outside [0, 1) or NaN, and with a core that lacks the entry points (bound weakly, like the gate's).
        void setJointProb(double prob);
        double jointProb() const
        {
                return joint_prob;
        }
        uint64_t jointRejected() const
        {
                return joint_rejected;
        }

      private:
        void compactHost(const std::vector<uint8_t> &mask);
        void associateGated(uint32_t mapped, std::vector<uint8_t> &sighted);
        double assoc_gate = 0.0;
        uint64_t assoc_rejected = 0;
        double joint_prob = 0.0;
        uint64_t joint_rejected = 0;
        std::vector<double> joint_tab; // [ASLAM_JC_MAX_OBS + 1] chi-square points of joint_prob, entry m for m pairings
        void *gate_dev = nullptr; // device [gate_cap] i32: the indices of one gated message
        size_t gate_cap = 0;
        int filter;
        int MAX_LANDMARK_COUNT;
        aslam_ctx *ctx;

        uint32_t N;
        bool init_z;
        bool init_x;
        float last_time;
        bool growth_refused;
        bool slam_ran; // in the last odometry callback
        aslam_params prm;
        std::vector<LaserData> sensor_landmark;
        std::vector<std::pair<LaserData, uint32_t>> new_landmark_wait;
        std::vector<double> param_X, param_Z; // host copies; P and the authoritative X are device-resident
        double a00, a10;                      // param.A(0,0), param.A(1,0) (EKF)
        uint32_t sight_clock;
        std::vector<uint32_t> lm_seen, lm_hits; // one entry per mapped landmark
        std::vector<uint8_t> lm_sighted;        // the mask of the last callback's association, one entry per mapped landmark
        bool sighted_only = false;

        void updateZ(const Odometry &msg, float delta_time);
        void updateNewLandmarkWait(const LaserData &data);
        void updateNewLandmark(const std::vector<LaserData> &new_landmark);
        void slam(float vx, float az, float delta_time);
};

class EKFSlam : public FilterNode
{
      public:
        explicit EKFSlam(int max_landmark_count = 30, int device = 0, double now_init = 0.0) : FilterNode(ASLAM_EKF, max_landmark_count, device, now_init)
        {
        }
};

class UKFSlam : public FilterNode
{
      public:
        explicit UKFSlam(int max_landmark_count = 30, int device = 0, double now_init = 0.0) : FilterNode(ASLAM_UKF, max_landmark_count, device, now_init)
        {
        }
};
} // namespace aslam

// ---- C shim (ctypes / other FFI) ------------------------------------------------------------------------
extern "C" {
typedef struct aslam_node aslam_node;
/* filter: ASLAM_EKF | ASLAM_UKF.  NULL on failure (aslam_node_error()). */
aslam_node *aslam_node_create(int filter, int max_landmark_count, int device);
/* the same with the construction time of the node (seconds): initialize() stores ros::Time::now().toSec() in the binary32 last_time
 * (ekf.cpp:54), which the first delta_time of aslam_node_odom_now() is measured from.  aslam_node_create = ..._at(..., 0.0). */
aslam_node *aslam_node_create_at(int filter, int max_landmark_count, int device, double now_init);
void aslam_node_destroy(aslam_node *n);
const char *aslam_node_error(void);
int aslam_node_sensor(aslam_node *n, int count, const double *x, const double *y);
/* returns 1 if slam() ran, 0 if the callback returned early, negative on error */
int aslam_node_odom(aslam_node *n, const double msg[8], float delta_time);
int aslam_node_odom_now(aslam_node *n, const double msg[8], double now);
int aslam_node_dim(const aslam_node *n);
int aslam_node_get(const aslam_node *n, double *X, double *Z, double *a00, double *a10);
int aslam_node_wait(const aslam_node *n, float *range, float *bearing, uint32_t *count, int cap);
aslam_ctx *aslam_node_core(const aslam_node *n);
/* Switch the record of the last callback's innovation statistics on or off (off by default); 0, or -1 with aslam_node_error(). */
int aslam_node_enable_innovation(aslam_node *n, int on);
/* FilterNode::setSightedOnly (EKF nodes; off by default); 0, or -1 with aslam_node_error(). */
int aslam_node_set_sighted_only(aslam_node *n, int on);
/* y^T S^-1 y and ln |det S| of the last odometry callback's slam() (NaN when that callback returned early, or before the first one);
 * -1 with aslam_node_error() while the record is off. */
int aslam_node_innovation(const aslam_node *n, double *nis, double *logdet);
/* FilterNode::setParams / params(): 0, or -1 with aslam_node_error() (a refused field, or a core without run-time parameters). */
int aslam_node_set_params(aslam_node *n, const aslam_params *params);
int aslam_node_get_params(const aslam_node *n, aslam_params *params);
/* FilterNode::removeLandmarks: 0, or -1 with aslam_node_error() (an index out of range, a core that cannot remove landmarks). */
int aslam_node_remove_landmarks(aslam_node *n, const int32_t *indices, int count);
/* FilterNode::lastSeen / hits / clock: up to `cap` entries into last_seen and hits (either may be NULL), the clock into *clock (may be NULL);
 * returns the number of landmarks. */
int aslam_node_get_sightings(const aslam_node *n, uint32_t *last_seen, uint32_t *hits, int cap, uint32_t *clock);
/* FilterNode::removeStale: the number of landmarks removed, or -1 with aslam_node_error(). */
int aslam_node_remove_stale(aslam_node *n, uint32_t max_age);
/* FilterNode::mergeLandmarks: pairs [count][2] = (i, j); the number of pairs fused, or -1 with aslam_node_error(). */
int aslam_node_merge_landmarks(aslam_node *n, const int32_t *pairs, int count, double noise_var);
/* FilterNode::mergeDuplicates: the number of landmarks merged, or -1 with aslam_node_error(). */
int aslam_node_merge_duplicates(aslam_node *n, double gate, double max_dist, double noise_var);
/* FilterNode::joinMap: a host blob, frame12 = tx, ty, phi, cov[9] or NULL, select [select_len] or NULL; the number of landmarks joined, or -1
 * with aslam_node_error(). */
int aslam_node_join_map(aslam_node *n, const void *blob, int64_t bytes, int record, const double *frame12, const uint8_t *select, int select_len);
/* FilterNode::setAssocGate (0 = off, the default): 0, or -1 with aslam_node_error() (a negative or NaN gate). */
int aslam_node_set_assoc_gate(aslam_node *n, double gate);
/* FilterNode::assocRejected: observations the gate dropped although the Euclidean rule would have associated them. */
uint64_t aslam_node_assoc_rejected(const aslam_node *n);
/* FilterNode::setJointProb (0 = off, the default): 0, or -1 with aslam_node_error() (a value outside [0, 1), a core without the entry points). */
int aslam_node_set_joint_prob(aslam_node *n, double prob);
/* FilterNode::jointRejected: pairings the gate accepted and the joint test refused. */
uint64_t aslam_node_joint_rejected(const aslam_node *n);
/* Narrow `count` recorded odometry messages ([count][8]: px,py,qw,qx,qy,qz,vx,wz) the way cbOdom/updateZandA do
 * (ekf.cpp:139-142): pose[count][2], yaw[count] = quat2euler(...) as binary32, twist[count][2]. */
void aslam_host_narrow_odom(int64_t count, const double *odom, double *pose, float *yaw, double *twist);
}

// aslam_node.cpp -- host mirror of aslam::EKFSlam / aslam::UKFSlam (see aslam_node.h).
//
// Build: g++ -O2 -ffp-contract=off (the binary32 rounding points of the reference must not be fused),
// linked against libaslam_core.so.
#include "aslam_node.h"
#include "../../../include/aslam_snapshot.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace aslam
{
namespace
{
// include/awesome_slam/config.h:39 (MIN_DIST_THRESH and MIN_LANDMARK_OCC, config.h:43-44, are FilterNode::params(): assoc_dist, promote_count)
const float PI = 3.141592654;

struct WorldPoint
{
        float x, y; // structures.h:44-47: a Point built from two floats
};

/// LaserData::toPoint (structures.h:104-111) from the odometry pose held in Z(0..2)
WorldPoint project(const LaserData &d, const std::vector<double> &Z)
{
        const double heading = Z[2] + d.bearing;
        WorldPoint p;
        p.x = Z[0] + d.range * std::cos(heading);
        p.y = Z[1] + d.range * std::sin(heading);
        return p;
}

/// Point::distance -> eulerDistance (structures.h:69-73, tools.h:53-59)
float separation(const WorldPoint &a, const WorldPoint &b)
{
        const float dx = (double)a.x - (double)b.x;
        const float dy = (double)a.y - (double)b.y;
        return std::sqrt(dx * dx + dy * dy);
}

void check(int rc, const char *what)
{
        if (rc != ASLAM_OK)
                throw std::runtime_error(std::string(what) + ": " + aslam_last_error());
}
} // namespace

float normalizeAngle(float theta)
{
        float wrapped = std::fmod(theta, 2 * PI);
        if (wrapped > PI)
                wrapped = wrapped - 2 * PI;
        if (wrapped < -PI)
                wrapped = wrapped + 2 * PI;
        return wrapped;
}

float quat2euler(float w, float x, float y, float z)
{
        return std::atan2(2 * (w * z + x * y), 1 - 2 * (z * z + y * y));
}

FilterNode::FilterNode(int filter_, int max_landmark_count, int device, double now_init)
    : filter(filter_), MAX_LANDMARK_COUNT(max_landmark_count), ctx(nullptr), N(3), init_z(true), init_x(true),
      last_time((float)now_init), // ekf.cpp:54: last_time = ros::Time::now().toSec(), a float member (ekf.h:98)
      growth_refused(false), slam_ran(false), prm ASLAM_PARAMS_DEFAULT_INIT, param_X(3, 0.0), param_Z(3, 0.0), a00(1.0), a10(0.0), sight_clock(0)
{
        aslam_config cfg = {};
        cfg.filter = filter;
        cfg.dtype = ASLAM_F64;
        cfg.max_landmark_count = max_landmark_count;
        cfg.batch = 1;
        cfg.max_obs = 1; // the stored sensor message and the wait-list stay on the host at this seam
        cfg.max_wait = 1;
        cfg.device = device;
        check(aslam_create(&cfg, &ctx), "aslam_create");
}

extern "C" int hipFree(void *) __attribute__((weak)); // (associateGated's array: see there)

FilterNode::~FilterNode()
{
        if (gate_dev && hipFree)
                (void)hipFree(gate_dev);
        aslam_destroy(ctx);
}

void FilterNode::cbSensorLandmark(const Landmarks &msg)
{
        init_z = false;
        sensor_landmark.resize(msg.x.size());
        for (size_t i = 0; i < msg.x.size(); ++i)
        {
                sensor_landmark[i].range = msg.x[i]; // double -> float, LaserData::assign(const float &, const float &)
                sensor_landmark[i].bearing = msg.y[i];
        }
}

bool FilterNode::cbOdom(const Odometry &msg, double now)
{
        slam_ran = false;
        if (init_z)
                return false;
        // ekf.cpp:80-81: last_time is a float member
        float delta_time = std::min(now - last_time, 1.0);
        last_time = now;
        return cbOdomDt(msg, delta_time);
}

bool FilterNode::cbOdomDt(const Odometry &msg, float delta_time)
{
        slam_ran = false;
        if (init_z)
                return false;
        updateZ(msg, delta_time);
        if (init_x)
        {
                init_x = false;
                param_X = param_Z;
                check(aslam_set_state(ctx, 0, (int)N, param_X.data(), nullptr, nullptr), "aslam_set_state");
        }
        slam(msg.vx, msg.wz, delta_time);
        slam_ran = true;
        return true;
}

// The innovation record is the one part of the core's ABI this file binds weakly: a stand-in core without it (the oracle-backed one of
// tests/sanitize/) still links, and the record is then refused like any other call sequence error.
extern "C" {
int aslam_innovation_enable(aslam_ctx *, int) __attribute__((weak));
int aslam_get_innovation(aslam_ctx *, int, double *, double *) __attribute__((weak));
}

void FilterNode::enableInnovation(bool on)
{
        if (!aslam_innovation_enable || !aslam_get_innovation)
                throw std::runtime_error("this core has no innovation record");
        check(aslam_innovation_enable(ctx, on ? 1 : 0), "aslam_innovation_enable");
}

void FilterNode::innovation(double &nis, double &logdet) const
{
        if (!aslam_get_innovation)
                throw std::runtime_error("this core has no innovation record");
        check(aslam_get_innovation(ctx, 0, &nis, &logdet), "aslam_get_innovation"); // (fails while the record is off)
        if (!slam_ran)
                nis = logdet = std::nan(""); // the core still holds the callback before
}

// The sighted-only update is bound weakly like the innovation record: a core without it refuses the mode, at run time.
extern "C" {
int aslam_sighted_update_enable(aslam_ctx *, int) __attribute__((weak));
int aslam_ekf_step_sighted(aslam_ctx *, int, float, float, float, const double *, const uint8_t *, double, double, double *, void *) __attribute__((weak));
}

void FilterNode::setSightedOnly(bool on)
{
        if (!aslam_sighted_update_enable || !aslam_ekf_step_sighted)
                throw std::runtime_error("this core has no sighted-only update");
        check(aslam_sighted_update_enable(ctx, on ? 1 : 0), "aslam_sighted_update_enable"); // (refused for the UKF)
        sighted_only = on;
}

// The parameter entry points are bound weakly for the same reason (and aslam_reset, which only setParams calls): with a core that lacks them
// the mirror runs on the reference's constants, and anything else is refused.
extern "C" {
int aslam_set_params(aslam_ctx *, int, const aslam_params *) __attribute__((weak));
int aslam_reset(aslam_ctx *) __attribute__((weak));
}

void FilterNode::setParams(const aslam_params &p)
{
        if (aslam_set_params && aslam_reset)
        {
                check(aslam_set_params(ctx, 0, &p), "aslam_set_params");
                // p0_pose applies at initialize(): a node that has not run a callback yet is initialised again, a running one keeps its P
                if (init_x)
                        check(aslam_reset(ctx), "aslam_reset");
        }
        else
        {
                const aslam_params def = ASLAM_PARAMS_DEFAULT_INIT;
                if (std::memcmp(&p, &def, sizeof(def)) != 0)
                        throw std::runtime_error("this core has no run-time parameters: only the defaults can be set");
        }
        prm = p;
}

// aslam_remove_landmarks is bound weakly like the entry points above: a core without it refuses the call, at run time.
extern "C" {
int aslam_remove_landmarks(aslam_ctx *, const uint8_t *, int, int, void *) __attribute__((weak));
}

void FilterNode::removeLandmarks(const std::vector<int> &indices)
{
        if (!aslam_remove_landmarks)
                throw std::runtime_error("this core cannot remove landmarks");
        const int mapped = (int)(N - 3) / 2;
        std::vector<uint8_t> mask((size_t)std::max(mapped, (MAX_LANDMARK_COUNT - 2) / 2), 0);
        for (int i : indices)
        {
                if (i < 0 || i >= mapped)
                        throw std::runtime_error("removeLandmarks: landmark index " + std::to_string(i) + " out of range");
                mask[i] = 1;
        }
        if (indices.empty())
                return;
        check(aslam_remove_landmarks(ctx, mask.data(), (int)mask.size(), 0, nullptr), "aslam_remove_landmarks");
        compactHost(mask);
}

/// the host copies of X and Z and the sighting record, compacted the way the core compacts its own (the wait-list and the stored message stay)
void FilterNode::compactHost(const std::vector<uint8_t> &mask)
{
        const int mapped = (int)(N - 3) / 2;
        uint32_t kept = 3;
        for (int i = 0; i < mapped; ++i)
        {
                if (mask[i])
                        continue;
                lm_seen[(kept - 3) / 2] = lm_seen[i];
                lm_hits[(kept - 3) / 2] = lm_hits[i];
                for (int k = 0; k < 2; ++k, ++kept)
                {
                        param_X[kept] = param_X[3 + 2 * i + k];
                        param_Z[kept] = param_Z[3 + 2 * i + k];
                }
        }
        N = kept;
        param_X.resize(N);
        param_Z.resize(N);
        lm_seen.resize((N - 3) / 2);
        lm_hits.resize((N - 3) / 2);
        lm_sighted.assign((N - 3) / 2, 0); // (the mask of the last callback indexed the old landmarks)
}

// aslam_merge_landmarks is bound weakly like aslam_remove_landmarks: a core without it refuses the call, at run time.
extern "C" {
int aslam_merge_landmarks(aslam_ctx *, const int32_t *, int, int, double, int32_t *, void *) __attribute__((weak));
}

int FilterNode::mergeLandmarks(const std::vector<std::pair<int, int>> &pairs, double noise_var)
{
        if (!aslam_merge_landmarks)
                throw std::runtime_error("this core cannot merge landmarks");
        const int mapped = (int)(N - 3) / 2;
        std::vector<int32_t> into((size_t)std::max(mapped, (MAX_LANDMARK_COUNT - 2) / 2), -1);
        for (const auto &p : pairs)
        {
                if (p.second < 0 || p.second >= mapped || into[p.second] != -1)
                        throw std::runtime_error("mergeLandmarks: landmark index " + std::to_string(p.second) + " out of range or named twice");
                into[p.second] = p.first; // (the core checks 0 <= i < j and the chains, and changes nothing when it refuses)
        }
        if (pairs.empty())
                return 0;
        int32_t merged = 0;
        check(aslam_merge_landmarks(ctx, into.data(), (int)into.size(), 0, noise_var, &merged, nullptr), "aslam_merge_landmarks");
        // the core takes the pairs in ascending j and stops, if at all, at a round: the first `merged` of them are fused and gone
        std::vector<uint8_t> mask(into.size(), 0);
        int done = 0;
        for (int j = 0; j < mapped && done < merged; ++j)
        {
                const int i = into[j];
                if (i < 0)
                        continue;
                lm_hits[i] += lm_hits[j];
                if (sight_clock - lm_seen[j] < sight_clock - lm_seen[i])
                        lm_seen[i] = lm_seen[j];
                mask[j] = 1;
                ++done;
        }
        if (done)
        {
                compactHost(mask);
                check(aslam_get_state(ctx, 0, param_X.data(), nullptr, nullptr), "aslam_get_state"); // (the constraint moved every entry of X)
        }
        return done;
}

// aslam_join_maps (aslam_snapshot.h) is bound weakly like aslam_merge_landmarks: a core without it refuses the call, at run time.
extern "C" {
int aslam_join_maps(aslam_ctx *, const int32_t *, const int32_t *, int, const void *, int64_t, int, const aslam_frame *, const uint8_t *, int, int32_t *,
                    void *) __attribute__((weak));
}

int FilterNode::joinMap(const void *blob, int64_t bytes, int record, const double *frame12, const uint8_t *select, int select_len)
{
        if (!aslam_join_maps)
                throw std::runtime_error("this core cannot join maps");
        if (!blob)
                throw std::runtime_error("joinMap: null blob");
        aslam_frame f = {};
        if (frame12)
        {
                f.tx = frame12[0], f.ty = frame12[1], f.phi = frame12[2];
                std::copy(frame12 + 3, frame12 + 12, f.cov);
        }
        const int32_t rec = record, slot = 0;
        int32_t joined = 0;
        check(aslam_join_maps(ctx, &rec, &slot, 1, blob, bytes, 0, frame12 ? &f : nullptr, select, select ? select_len : 0, &joined, nullptr),
              "aslam_join_maps"); // (the core checks everything and changes nothing when it refuses)
        if (joined == 0)
                return 0;
        N += 2 * (uint32_t)joined;
        param_X.resize(N);
        param_Z.resize(N);
        check(aslam_get_state(ctx, 0, param_X.data(), param_Z.data(), nullptr), "aslam_get_state"); // (the new X and the Z seeded from the pose)
        lm_seen.resize((N - 3) / 2, sight_clock); // as updateNewLandmark enters a promoted landmark
        lm_hits.resize((N - 3) / 2, 0);
        lm_sighted.assign((N - 3) / 2, 0);
        return joined;
}

int FilterNode::mergeDuplicates(double gate, double max_dist, double noise_var)
{
        if (!(gate > 0.0) || !std::isfinite(max_dist) || max_dist <= 0.0)
                throw std::runtime_error("mergeDuplicates: gate must be positive, max_dist finite and positive");
        const double maxd2 = max_dist * max_dist;
        int total = 0;
        for (int pass = 0; pass < 4; ++pass)
        {
                const int n = (int)N, L = (n - 3) / 2;
                if (L < 2)
                        break;
                std::vector<double> X((size_t)n), P((size_t)n * n);
                check(aslam_get_state(ctx, 0, X.data(), nullptr, P.data()), "aslam_get_state");
                // aslam_select_duplicates' arithmetic (aslam_core.h), operation by operation; this file is compiled without FMA contraction
                std::vector<int> partner((size_t)L, -1);
                auto p = [&](int r, int c) { return P[(size_t)r * n + c]; };
                for (int j = 1; j < L; ++j)
                {
                        double best = 0.0;
                        for (int i = 0; i < j; ++i)
                        {
                                const int a0 = 3 + 2 * i, a1 = a0 + 1, c0 = 3 + 2 * j, c1 = c0 + 1;
                                const double dx = X[a0] - X[c0], dy = X[a1] - X[c1];
                                const double r2 = dx * dx + dy * dy;
                                if (!(r2 <= maxd2))
                                        continue;
                                const double s00 = ((p(a0, a0) + p(c0, c0)) - p(c0, a0)) - p(c0, a0);
                                const double s11 = ((p(a1, a1) + p(c1, c1)) - p(c1, a1)) - p(c1, a1);
                                const double s10 = ((p(a1, a0) + p(c1, c0)) - p(c1, a0)) - p(c0, a1);
                                const double det = s00 * s11 - s10 * s10;
                                if (!(s00 > 0.0) || !(det > 0.0))
                                        continue;
                                const double t1 = (s10 * dx) * dy;
                                const double num = (((s11 * dx) * dx) - (t1 + t1)) + ((s00 * dy) * dy);
                                const double m = num / det;
                                if (m < gate && (partner[j] < 0 || m < best))
                                        best = m, partner[j] = i;
                        }
                }
                std::vector<std::pair<int, int>> pairs;
                for (int j = 1; j < L; ++j)
                        if (partner[j] >= 0 && partner[partner[j]] == -1)
                                pairs.emplace_back(partner[j], j);
                const int k = pairs.empty() ? 0 : mergeLandmarks(pairs, noise_var);
                total += k;
                if (k == 0)
                        break;
        }
        return total;
}

// aslam_gate_observations is bound weakly like the entry points above.  Its output is a device array, and this file is plain C++: the three
// calls of the HIP runtime it needs for that array (the copy libaslam_core.so itself is linked against) are declared here with their C ABI
// -- hipError_t and hipMemcpyKind are int-sized enums -- and bound weakly too, so that the mirror still links where no HIP runtime is.
extern "C" {
int aslam_gate_observations(aslam_ctx *, const float *, int, int, const int32_t *, const double *, int32_t *, double *, void *) __attribute__((weak));
int aslam_joint_compat(aslam_ctx *, const float *, int, int, const int32_t *, const int32_t *, const double *, int32_t *, double *, double *, int32_t *,
                       void *) __attribute__((weak));
int aslam_chi2_point(double, int, double *) __attribute__((weak));
int hipMalloc(void **, size_t) __attribute__((weak));
int hipFree(void *) __attribute__((weak));
int hipMemcpy(void *, const void *, size_t, int) __attribute__((weak));
}

void FilterNode::setAssocGate(double gate)
{
        if (!(gate >= 0.0))
                throw std::runtime_error("setAssocGate: the gate must be positive, or 0 for off");
        assoc_gate = gate;
}

void FilterNode::setJointProb(double prob)
{
        if (!(prob >= 0.0 && prob < 1.0))
                throw std::runtime_error("setJointProb: the probability must lie inside (0, 1), or be 0 for off");
        std::vector<double> tab;
        if (prob > 0.0)
        {
                if (!aslam_joint_compat || !aslam_chi2_point)
                        throw std::runtime_error("this core has no joint-compatibility test");
                tab.assign(ASLAM_JC_MAX_OBS + 1, 0.0);
                for (int m = 1; m <= ASLAM_JC_MAX_OBS; ++m)
                        check(aslam_chi2_point(prob, 2 * m, &tab[m]), "aslam_chi2_point");
        }
        joint_prob = prob;
        joint_tab.swap(tab);
}

/// updateZ's association with the gate on and `mapped` > 0 landmarks: one aslam_gate_observations call for the stored message, then the
/// observations in message order (see setAssocGate in aslam_node.h)
void FilterNode::associateGated(uint32_t mapped, std::vector<uint8_t> &sighted)
{
        if (!aslam_gate_observations || !hipMalloc || !hipFree || !hipMemcpy)
                throw std::runtime_error("this core cannot gate observations");
        const size_t count = sensor_landmark.size();
        std::vector<float> ob(2 * count);
        for (size_t j = 0; j < count; ++j)
        {
                LaserData &obs = sensor_landmark[j];
                obs.bearing = normalizeAngle(obs.bearing);
                ob[2 * j] = obs.range;
                ob[2 * j + 1] = obs.bearing;
        }
        // the device array: the indices of the message, and behind them (with the joint test on) D2 and log det C, the two counters, and the
        // increment of every pairing -- finite where the joint test saw a usable candidate, so finite and -1 names a pairing it refused
        const bool joint = joint_prob > 0.0;
        const size_t idx_bytes = (sizeof(int32_t) * count + 15) / 16 * 16;
        const size_t tail = joint ? 32 + sizeof(double) * count : 0; // [2] f64 | [2] i32 and padding | [count] f64
        if (count > gate_cap)
        {
                if (gate_dev)
                        (void)hipFree(gate_dev);
                gate_dev = nullptr;
                gate_cap = 0;
                const size_t cap = std::max<size_t>(64, 2 * count);
                if (hipMalloc(&gate_dev, (sizeof(int32_t) + sizeof(double)) * cap + 48) != 0) // (room for the joint test's tail at any count <= cap)
                        throw std::runtime_error("associateGated: hipMalloc failed");
                gate_cap = cap;
        }
        const int32_t n_obs = (int32_t)count;
        std::vector<unsigned char> back(idx_bytes + tail);
        check(aslam_gate_observations(ctx, ob.data(), (int)count, 0, &n_obs, &assoc_gate, static_cast<int32_t *>(gate_dev), nullptr, nullptr),
              "aslam_gate_observations");
        if (joint)
        {
                char *tail_dev = static_cast<char *>(gate_dev) + idx_bytes;
                int32_t *idx = static_cast<int32_t *>(gate_dev);
                check(aslam_joint_compat(ctx, ob.data(), (int)count, 0, &n_obs, idx, joint_tab.data(), idx, reinterpret_cast<double *>(tail_dev + 32),
                                         reinterpret_cast<double *>(tail_dev), reinterpret_cast<int32_t *>(tail_dev + 16), nullptr),
                      "aslam_joint_compat");
        }
        if (hipMemcpy(back.data(), gate_dev, back.size(), 2 /* hipMemcpyDeviceToHost: waits for the launches on the default stream */) != 0)
                throw std::runtime_error("associateGated: hipMemcpy failed");
        std::vector<int32_t> assoc(count, -1);
        std::vector<double> incr(count, INFINITY);
        std::memcpy(assoc.data(), back.data(), sizeof(int32_t) * count);
        if (joint)
                std::memcpy(incr.data(), back.data() + idx_bytes + 32, sizeof(double) * count);
        for (size_t j = 0; j < count; ++j)
        {
                const LaserData &obs = sensor_landmark[j];
                if (assoc[j] >= 0 && (uint32_t)assoc[j] < mapped)
                {
                        param_Z[3 + 2 * assoc[j]] = obs.range;
                        param_Z[4 + 2 * assoc[j]] = obs.bearing;
                        sighted[assoc[j]] = 1;
                        continue;
                }
                if (std::isfinite(incr[j]))
                {
                        joint_rejected += 1; // dropped: the gate paired it, the joint test refuses the pairing beside the ones before it
                        continue;
                }
                // the reference's own test (updateZ below), for the verdict alone
                const WorldPoint seen = project(obs, param_Z);
                float best_d = 0.0f;
                for (uint32_t k = 0; k < mapped; ++k)
                {
                        const WorldPoint known = {(float)param_X[3 + 2 * k], (float)param_X[4 + 2 * k]};
                        const float dk = separation(seen, known);
                        if (k == 0 || dk < best_d)
                                best_d = dk;
                }
                if (best_d < prm.assoc_dist)
                        assoc_rejected += 1; // dropped: the Euclidean rule would have made it a match, the gate says it is none
                else
                        updateNewLandmarkWait(obs);
        }
}

int FilterNode::removeStale(uint32_t max_age)
{
        std::vector<int> stale;
        for (size_t i = 0; i < lm_seen.size(); ++i)
                if (sight_clock - lm_seen[i] > max_age)
                        stale.push_back((int)i);
        removeLandmarks(stale);
        return (int)stale.size();
}

Landmarks FilterNode::landmarks() const
{
        Landmarks out;
        for (uint32_t i = 0; i + 3 < N; i += 2)
        {
                out.x.push_back(param_X[3 + i]);
                out.y.push_back(param_X[4 + i]);
        }
        return out;
}

/// updateZandA (ekf.cpp:137-213) / updateZ (ukf.cpp:113-180)
void FilterNode::updateZ(const Odometry &msg, float delta_time)
{
        param_Z[0] = msg.px;
        param_Z[1] = msg.py;
        param_Z[2] = quat2euler(msg.qw, msg.qx, msg.qy, msg.qz);

        const uint32_t mapped = (N - 3) / 2;
        sight_clock += 1;
        std::vector<uint8_t> &sighted = lm_sighted; // several observations on one landmark are one hit; the mask of this callback
        sighted.assign(mapped, 0);
        const bool gated = assoc_gate > 0.0 && mapped > 0 && !sensor_landmark.empty();
        if (gated)
                associateGated(mapped, sighted);
        else // the reference's rule, line for line what it was
        for (LaserData &obs : sensor_landmark)
        {
                obs.bearing = normalizeAngle(obs.bearing);
                bool associated = false;
                if (mapped > 0)
                {
                        const WorldPoint seen = project(obs, param_Z);
                        uint32_t best = 0;
                        float best_d = 0.0f;
                        for (uint32_t k = 0; k < mapped; ++k)
                        {
                                const WorldPoint known = {(float)param_X[3 + 2 * k], (float)param_X[4 + 2 * k]};
                                const float dk = separation(seen, known);
                                if (k == 0 || dk < best_d)
                                {
                                        best = k;
                                        best_d = dk;
                                }
                        }
                        if (best_d < prm.assoc_dist)
                        {
                                param_Z[3 + 2 * best] = obs.range;
                                param_Z[4 + 2 * best] = obs.bearing;
                                sighted[best] = 1;
                                associated = true;
                        }
                }
                if (!associated)
                        updateNewLandmarkWait(obs);
        }

        for (uint32_t k = 0; k < mapped; ++k)
                if (sighted[k])
                {
                        lm_seen[k] = sight_clock;
                        lm_hits[k] += 1;
                }

        std::vector<LaserData> promoted;
        for (auto &entry : new_landmark_wait)
        {
                if (entry.second == prm.promote_count)
                {
                        promoted.push_back(entry.first);
                        entry.second += 1;
                }
        }
        if (!promoted.empty())
                updateNewLandmark(promoted);

        if (filter == ASLAM_EKF && msg.vx && msg.wz)
        {
                const float delta_theta = msg.wz * delta_time;
                const float r = msg.vx / msg.wz;
                a00 = r * (-std::cos(param_Z[2]) + std::cos(param_Z[2] + delta_theta));
                a10 = r * (-std::sin(param_Z[2]) + std::sin(param_Z[2] + delta_theta));
        }
}

/// ekf.cpp:217-253 / ukf.cpp:184-220
void FilterNode::updateNewLandmarkWait(const LaserData &data)
{
        if (!new_landmark_wait.empty())
        {
                const WorldPoint seen = project(data, param_Z);
                size_t best = 0;
                float best_d = 0.0f;
                for (size_t i = 0; i < new_landmark_wait.size(); ++i)
                {
                        const float di = separation(seen, project(new_landmark_wait[i].first, param_Z));
                        if (i == 0 || di < best_d)
                        {
                                best = i;
                                best_d = di;
                        }
                }
                if (best_d < prm.assoc_dist)
                {
                        new_landmark_wait[best].second++;
                        return;
                }
        }
        new_landmark_wait.push_back({data, 1});
}

/// ekf.cpp:255-290 / ukf.cpp:222-257: the vectors grow here, the matrices grow on the device (aslam_grow)
void FilterNode::updateNewLandmark(const std::vector<LaserData> &new_landmark)
{
        const uint32_t cacheN = N;
        const uint32_t grown = N + 2 * (uint32_t)new_landmark.size();
        if (grown >= (uint32_t)MAX_LANDMARK_COUNT)
        {
                growth_refused = true; // "[WARN] MAXIMUM LANDMARK COUNT IS SET TO ..." in the reference
                return;
        }
        N = grown;
        param_X.resize(N, 0.0);
        param_Z.resize(N, 0.0);
        lm_seen.resize((N - 3) / 2, sight_clock); // promoted now, never sighted as a landmark
        lm_hits.resize((N - 3) / 2, 0u);
        lm_sighted.resize((N - 3) / 2, 0); // initialised from this very reading: not sighted
        for (size_t k = 0; k < new_landmark.size(); ++k)
        {
                const uint32_t i = cacheN + 2 * (uint32_t)k;
                param_Z[i] = new_landmark[k].range;
                param_Z[i + 1] = new_landmark[k].bearing;
                param_X[i] = param_Z[0] + param_Z[i] * std::cos(param_Z[2] + param_Z[i + 1]);
                param_X[i + 1] = param_Z[1] + param_Z[i] * std::sin(param_Z[2] + param_Z[i + 1]);
        }
        check(aslam_grow(ctx, 0, (int)N, &param_X[cacheN], &param_Z[cacheN]), "aslam_grow");
}

void FilterNode::slam(float vx, float az, float delta_time)
{
        if (filter == ASLAM_EKF && sighted_only)
        {
                lm_sighted.resize(std::max<size_t>(1, (N - 3) / 2), 0); // (a valid pointer with no landmark mapped yet)
                check(aslam_ekf_step_sighted(ctx, 0, vx, az, delta_time, param_Z.data(), lm_sighted.data(), a00, a10, param_X.data(), nullptr),
                      "aslam_ekf_step_sighted");
                lm_sighted.resize((N - 3) / 2);
        }
        else if (filter == ASLAM_EKF)
                check(aslam_ekf_step(ctx, 0, vx, az, delta_time, param_Z.data(), a00, a10, param_X.data(), nullptr),
                      "aslam_ekf_step");
        else
                check(aslam_ukf_step(ctx, 0, vx, az, delta_time, param_Z.data(), param_X.data(), nullptr), "aslam_ukf_step");
}
} // namespace aslam

// ---- C shim -----------------------------------------------------------------------------------------------
struct aslam_node
{
        aslam::FilterNode *impl;
};

namespace
{
thread_local std::string g_node_err;
}

extern "C" {

aslam_node *aslam_node_create(int filter, int max_landmark_count, int device)
{
        return aslam_node_create_at(filter, max_landmark_count, device, 0.0);
}

aslam_node *aslam_node_create_at(int filter, int max_landmark_count, int device, double now_init)
{
        try
        {
                aslam_node *n = new aslam_node();
                n->impl = new aslam::FilterNode(filter, max_landmark_count, device, now_init);
                return n;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return nullptr;
        }
}

void aslam_node_destroy(aslam_node *n)
{
        if (n)
        {
                delete n->impl;
                delete n;
        }
}

const char *aslam_node_error(void)
{
        return g_node_err.c_str();
}

int aslam_node_sensor(aslam_node *n, int count, const double *x, const double *y)
{
        aslam::Landmarks m;
        m.x.assign(x, x + count);
        m.y.assign(y, y + count);
        n->impl->cbSensorLandmark(m);
        return 0;
}

static aslam::Odometry to_msg(const double v[8])
{
        aslam::Odometry m;
        m.px = v[0];
        m.py = v[1];
        m.qw = v[2];
        m.qx = v[3];
        m.qy = v[4];
        m.qz = v[5];
        m.vx = v[6];
        m.wz = v[7];
        return m;
}

int aslam_node_odom(aslam_node *n, const double msg[8], float delta_time)
{
        try
        {
                return n->impl->cbOdomDt(to_msg(msg), delta_time) ? 1 : 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_odom_now(aslam_node *n, const double msg[8], double now)
{
        try
        {
                return n->impl->cbOdom(to_msg(msg), now) ? 1 : 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_dim(const aslam_node *n)
{
        return (int)n->impl->dim();
}

int aslam_node_get(const aslam_node *n, double *X, double *Z, double *a00, double *a10)
{
        const uint32_t N = n->impl->dim();
        if (X)
                std::copy(n->impl->X().begin(), n->impl->X().begin() + N, X);
        if (Z)
                std::copy(n->impl->Z().begin(), n->impl->Z().begin() + N, Z);
        if (a00)
                *a00 = n->impl->A00();
        if (a10)
                *a10 = n->impl->A10();
        return 0;
}

int aslam_node_wait(const aslam_node *n, float *range, float *bearing, uint32_t *count, int cap)
{
        const auto &w = n->impl->waitList();
        const int k = std::min<int>(cap, (int)w.size());
        for (int i = 0; i < k; ++i)
        {
                range[i] = w[i].first.range;
                bearing[i] = w[i].first.bearing;
                count[i] = w[i].second;
        }
        return (int)w.size();
}

aslam_ctx *aslam_node_core(const aslam_node *n)
{
        return n->impl->core();
}

int aslam_node_enable_innovation(aslam_node *n, int on)
{
        try
        {
                n->impl->enableInnovation(on != 0);
                return 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_set_sighted_only(aslam_node *n, int on)
{
        try
        {
                n->impl->setSightedOnly(on != 0);
                return 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_set_params(aslam_node *n, const aslam_params *p)
{
        try
        {
                if (!p)
                        throw std::runtime_error("null argument");
                n->impl->setParams(*p);
                return 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_remove_landmarks(aslam_node *n, const int32_t *indices, int count)
{
        try
        {
                if (!n || count < 0 || (count && !indices))
                        throw std::runtime_error("null argument");
                n->impl->removeLandmarks(std::vector<int>(indices, indices + count));
                return 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_merge_landmarks(aslam_node *n, const int32_t *pairs, int count, double noise_var)
{
        try
        {
                if (!n || count < 0 || (count && !pairs))
                        throw std::runtime_error("null argument");
                std::vector<std::pair<int, int>> pr;
                for (int k = 0; k < count; ++k)
                        pr.emplace_back(pairs[2 * k], pairs[2 * k + 1]);
                return n->impl->mergeLandmarks(pr, noise_var);
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_merge_duplicates(aslam_node *n, double gate, double max_dist, double noise_var)
{
        try
        {
                if (!n)
                        throw std::runtime_error("null argument");
                return n->impl->mergeDuplicates(gate, max_dist, noise_var);
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_join_map(aslam_node *n, const void *blob, int64_t bytes, int record, const double *frame12, const uint8_t *select, int select_len)
{
        try
        {
                if (!n)
                        throw std::runtime_error("null argument");
                return n->impl->joinMap(blob, bytes, record, frame12, select, select_len);
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_set_assoc_gate(aslam_node *n, double gate)
{
        try
        {
                if (!n)
                        throw std::runtime_error("null argument");
                n->impl->setAssocGate(gate);
                return 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

uint64_t aslam_node_assoc_rejected(const aslam_node *n)
{
        return n->impl->assocRejected();
}

int aslam_node_set_joint_prob(aslam_node *n, double prob)
{
        try
        {
                if (!n)
                        throw std::runtime_error("null argument");
                n->impl->setJointProb(prob);
                return 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

uint64_t aslam_node_joint_rejected(const aslam_node *n)
{
        return n->impl->jointRejected();
}

int aslam_node_get_sightings(const aslam_node *n, uint32_t *last_seen, uint32_t *hits, int cap, uint32_t *clock)
{
        const auto &s = n->impl->lastSeen();
        const auto &h = n->impl->hits();
        const int k = std::max(0, std::min<int>(cap, (int)s.size()));
        if (last_seen)
                std::copy(s.begin(), s.begin() + k, last_seen);
        if (hits)
                std::copy(h.begin(), h.begin() + k, hits);
        if (clock)
                *clock = n->impl->clock();
        return (int)s.size();
}

int aslam_node_remove_stale(aslam_node *n, uint32_t max_age)
{
        try
        {
                if (!n)
                        throw std::runtime_error("null argument");
                return n->impl->removeStale(max_age);
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

int aslam_node_get_params(const aslam_node *n, aslam_params *p)
{
        if (!p)
                return -1;
        *p = n->impl->params();
        return 0;
}

int aslam_node_innovation(const aslam_node *n, double *nis, double *logdet)
{
        try
        {
                double a = 0.0, b = 0.0;
                n->impl->innovation(a, b);
                if (nis)
                        *nis = a;
                if (logdet)
                        *logdet = b;
                return 0;
        }
        catch (const std::exception &e)
        {
                g_node_err = e.what();
                return -1;
        }
}

void aslam_host_narrow_odom(int64_t count, const double *odom, double *pose, float *yaw, double *twist)
{
        for (int64_t i = 0; i < count; ++i)
        {
                const double *m = odom + 8 * i;
                pose[2 * i] = m[0];
                pose[2 * i + 1] = m[1];
                yaw[i] = aslam::quat2euler(m[2], m[3], m[4], m[5]);
                twist[2 * i] = m[6];
                twist[2 * i + 1] = m[7];
        }
}

} // extern "C"

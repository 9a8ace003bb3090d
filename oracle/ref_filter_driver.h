// Driver over one of the reference's filter nodes, exporting the orc_* interface of aslam_oracle.h.  TEST INFRASTRUCTURE ONLY.
// Included by ref_ekf.cpp / ref_ukf.cpp after the reference's own .cpp (one translation unit per node: both node headers
// define `struct Parameters`), with RefNode, REF_KIND and REF_IS_EKF set.  Built with -fno-access-control: the private members
// are read here, nothing of the node is restated.  Messages go through the callbacks that the node subscribed.
#include "aslam_oracle.h"

#include <cstring>

struct orc_filter
{
        RefNode node;
        // delta_time is a local of the node's cbOdom and cannot be read.  orc_odom restates `std::min(now - last_time, 1.0)` on the
        // node's own last_time and counts the callbacks at which that is not the dt asked for: a guard on the clock handed in, not
        // an observation.  What the node really derives is observed through its outputs: the clock cases of
        // tests/reference_cases.py drive, and tests/test_reference_parity.py shows that other readings miss the recording.
        int64_t dt_mismatch = 0;
};

static std::shared_ptr<const nav_msgs::Odometry> make_odom(double px, double py, double qw, double qx, double qy, double qz,
                                                           double vx, double wz)
{
        auto m = std::make_shared<nav_msgs::Odometry>();
        m->pose.pose.position.x = px;
        m->pose.pose.position.y = py;
        m->pose.pose.orientation.w = qw;
        m->pose.pose.orientation.x = qx;
        m->pose.pose.orientation.y = qy;
        m->pose.pose.orientation.z = qz;
        m->twist.twist.linear.x = vx;
        m->twist.twist.angular.z = wz;
        return m;
}

extern "C" {

// the node is constructed (and initialize() reads the clock) at `now`
orc_filter *ref_create_at(int kind, int max_landmark_count, double now)
{
        if (kind != REF_KIND || max_landmark_count != MAX_LANDMARK_COUNT)
                return nullptr; // the reference is one filter with a compile-time cap
        ros::Time::setNow(now);
        return new orc_filter();
}

orc_filter *orc_create(int kind, int max_landmark_count)
{
        return ref_create_at(kind, max_landmark_count, 0.0);
}

void orc_destroy(orc_filter *f)
{
        delete f;
}

void orc_sensor(orc_filter *f, int n, const double *x, const double *y)
{
        auto m = std::make_shared<awesome_slam_msgs::Landmarks>();
        m->x.assign(x, x + n);
        m->y.assign(y, y + n);
        f->node.nh.deliver<awesome_slam_msgs::Landmarks>("/out/landmarks/sensor", m);
}

// an odom message at the absolute clock value `now`
int ref_odom_at(orc_filter *f, double px, double py, double qw, double qx, double qy, double qz, double vx, double wz, double now)
{
        const int ran = f->node.init_z ? 0 : 1;
        ros::Time::setNow(now);
        f->node.nh.deliver<nav_msgs::Odometry>("/odom", make_odom(px, py, qw, qx, qy, qz, vx, wz));
        return ran;
}

int orc_odom(orc_filter *f, double px, double py, double qw, double qx, double qy, double qz, double vx, double wz,
             float delta_time)
{
        const double now = (double)f->node.last_time + (double)delta_time;
        const float derived = std::min(now - f->node.last_time, 1.0);
        if (!f->node.init_z && std::memcmp(&derived, &delta_time, sizeof(float)) != 0)
                ++f->dt_mismatch;
        return ref_odom_at(f, px, py, qw, qx, qy, qz, vx, wz, now);
}

int64_t ref_dt_mismatches(const orc_filter *f)
{
        return f->dt_mismatch;
}

float ref_last_time(const orc_filter *f)
{
        return f->node.last_time;
}

void orc_slam(orc_filter *f, float vx, float az, float delta_time)
{
        f->node.slam(vx, az, delta_time);
}

int orc_dim(const orc_filter *f)
{
        return (int)f->node.N;
}

void orc_get(const orc_filter *f, double *X, double *Z, double *P)
{
        const int n = (int)f->node.N;
        for (int i = 0; i < n; ++i)
        {
                if (X)
                        X[i] = f->node.param.X(i);
                if (Z)
                        Z[i] = f->node.param.Z(i);
                for (int j = 0; P && j < n; ++j)
                        P[(size_t)i * n + j] = f->node.param.P(i, j);
        }
}

void orc_get_A(const orc_filter *f, double *a00, double *a10)
{
#if REF_IS_EKF
        *a00 = f->node.param.A(0, 0);
        *a10 = f->node.param.A(1, 0);
#else
        (void)f;
        *a00 = 1.0;
        *a10 = 0.0;
#endif
}

// the members as N/2-1 calls of updateNewLandmark would have left them, with X, Z, P (row-major) as given
void orc_set(orc_filter *f, int N, const double *X, const double *Z, const double *P, double a00, double a10)
{
        RefNode &a = f->node;
        a.initialize();
        a.sensor_landmark.clear();
        a.new_landmark_wait.clear();
        a.init_z = false;
        a.init_x = false;
        a.N = N;
        a.param.Q.conservativeResizeLike(MatrixXd::Zero(N, N));
#if REF_IS_EKF
        a.param.I.conservativeResizeLike(MatrixXd::Identity(N, N));
        a.param.A.conservativeResizeLike(MatrixXd::Identity(N, N));
        a.param.H.conservativeResizeLike(MatrixXd::Identity(N, N));
        a.param.A(0, 0) = a00;
        a.param.A(1, 0) = a10;
#else
        (void)a00;
        (void)a10;
        a.param.updateWeights(N);
#endif
        a.param.R.conservativeResizeLike(MatrixXd::Identity(N, N) * UKF_KR);
        a.param.X = VectorXd::Zero(N);
        a.param.Z = VectorXd::Zero(N);
        a.param.P = MatrixXd::Zero(N, N);
        for (int i = 0; i < N; ++i)
        {
                a.param.X(i) = X[i];
                a.param.Z(i) = Z[i];
                for (int j = 0; j < N; ++j)
                        a.param.P(i, j) = P[(size_t)i * N + j];
        }
}

int orc_wait_size(const orc_filter *f)
{
        return (int)f->node.new_landmark_wait.size();
}

void orc_get_wait(const orc_filter *f, float *range, float *bearing, uint32_t *count)
{
        for (size_t i = 0; i < f->node.new_landmark_wait.size(); ++i)
        {
                range[i] = f->node.new_landmark_wait[i].first.range;
                bearing[i] = f->node.new_landmark_wait[i].first.bearing;
                count[i] = f->node.new_landmark_wait[i].second;
        }
}

int orc_sensor_size(const orc_filter *f)
{
        return (int)f->node.sensor_landmark.size();
}

void orc_get_sensor(const orc_filter *f, float *range, float *bearing)
{
        for (size_t i = 0; i < f->node.sensor_landmark.size(); ++i)
        {
                range[i] = f->node.sensor_landmark[i].range;
                bearing[i] = f->node.sensor_landmark[i].bearing;
        }
}

void orc_get_weights(const orc_filter *f, double *w, float *lambda)
{
#if REF_IS_EKF
        (void)f;
        (void)w;
        *lambda = 0.0f;
#else
        for (int i = 0; i < f->node.param.weights.size(); ++i)
                w[i] = f->node.param.weights(i);
        *lambda = f->node.param.lambda;
#endif
}

int64_t orc_replay(orc_filter *f, int64_t T, const double *odom, const float *dt, const uint8_t *obs_new,
                   const int32_t *n_obs, const double *obs, int max_obs, double *poses_out, int32_t *dims_out)
{
        int64_t ran = 0;
        std::vector<double> xs((size_t)max_obs), ys((size_t)max_obs);
        for (int64_t t = 0; t < T; ++t)
        {
                if (obs_new[t])
                {
                        const double *o = obs + (size_t)t * max_obs * 2;
                        for (int i = 0; i < n_obs[t]; ++i)
                        {
                                xs[(size_t)i] = o[2 * i];
                                ys[(size_t)i] = o[2 * i + 1];
                        }
                        orc_sensor(f, n_obs[t], xs.data(), ys.data());
                }
                const double *m = odom + (size_t)t * 8;
                const int r = orc_odom(f, m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], dt[t]);
                ran += r;
                for (int k = 0; poses_out && k < 3; ++k)
                        poses_out[3 * t + k] = r ? f->node.param.X(k) : 0.0;
                if (dims_out)
                        dims_out[t] = (int32_t)f->node.N;
        }
        return ran;
}

float orc_normalize_angle(float theta)
{
        return normalizeAngle(theta);
}

float orc_quat2euler(float w, float x, float y, float z)
{
        return quat2euler(w, x, y, z);
}

} // extern "C"

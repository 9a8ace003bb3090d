// The reference's scan node (sensor_landmark.cpp) behind a C entry (recipe: `make ref`).  TEST INFRASTRUCTURE ONLY.
// The node's source is compiled from the reference's own directory, given on the command line; none of it is copied here.
// Built with REF_SHIM_ASSERT_THROWS: the node's own assert, evaluated as written, ends the callback with an exception that is
// reported as status 1 (REF_ABORT) for that scan.
#include "sensor_landmark.cpp"

// The node writes `bearing2pose(theta, msg->ranges[theta++])`: which value of theta the first argument sees is the
// compiler's choice.  This probe has the same form and is compiled by the same compiler with the same flags.
static __attribute__((noinline)) int probe_first(const int16_t first, const float &second)
{
        return (int)first + 0 * (int)second;
}

extern "C" {

// 1: the first argument is evaluated before the increment (beam theta meets table entry theta); 0: after it (entry theta + 1)
int ref_scan_left_to_right(void)
{
        const float r[2] = {0.0f, 0.0f};
        volatile uint16_t start = 0;
        uint16_t theta = start;
        return probe_first(theta, r[theta++]) == 0 ? 1 : 0;
}

// ranges [count][360] -> status [count] (0 ok, 1 the node's assert failed), n [count], range/bearing [count][max_out]
// (binary32: the node publishes LaserData's floats widened to float64).  Landmarks past max_out are counted, not stored.
void ref_scan(int64_t count, const float *ranges, int max_out, int32_t *status, int32_t *n, float *range, float *bearing)
{
        aslam::LandMarks node;
        for (int64_t s = 0; s < count; ++s)
        {
                auto msg = std::make_shared<sensor_msgs::LaserScan>();
                msg->ranges.assign(ranges + s * 360, ranges + (s + 1) * 360);
                const uint64_t before = node.pub_landmarks.count();
                status[s] = 0;
                n[s] = 0;
                try
                {
                        node.nh.deliver<sensor_msgs::LaserScan>("/laser/scan", msg);
                }
                catch (const ros_shim::AssertFailed &)
                {
                        status[s] = 1;
                        continue;
                }
                if (node.pub_landmarks.count() != before + 1)
                {
                        status[s] = -1;
                        continue;
                }
                auto out = node.pub_landmarks.last<awesome_slam_msgs::Landmarks>();
                n[s] = (int32_t)out->x.size();
                for (int i = 0; i < n[s] && i < max_out; ++i)
                {
                        range[s * max_out + i] = (float)out->x[(size_t)i];
                        bearing[s * max_out + i] = (float)out->y[(size_t)i];
                }
        }
}

} // extern "C"

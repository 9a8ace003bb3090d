// Shim message (see ros/ros.h): the fields the nodes read.
#ifndef REF_SHIM_SENSOR_MSGS_LASERSCAN_H
#define REF_SHIM_SENSOR_MSGS_LASERSCAN_H

#include <memory>
#include <vector>

namespace sensor_msgs
{
struct LaserScan
{
        std::vector<float> ranges;
        typedef std::shared_ptr<LaserScan> Ptr;
        typedef std::shared_ptr<const LaserScan> ConstPtr;
};
} // namespace sensor_msgs

#endif

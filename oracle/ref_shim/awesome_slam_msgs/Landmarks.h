// Shim message (see ros/ros.h): Landmarks.msg is two float64 arrays.
#ifndef REF_SHIM_AWESOME_SLAM_MSGS_LANDMARKS_H
#define REF_SHIM_AWESOME_SLAM_MSGS_LANDMARKS_H

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace awesome_slam_msgs
{
struct Landmarks
{
        std::vector<double> x, y;
        typedef std::shared_ptr<Landmarks> Ptr;
        typedef std::shared_ptr<const Landmarks> ConstPtr;
};
} // namespace awesome_slam_msgs

#endif

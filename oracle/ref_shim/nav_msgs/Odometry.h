// Shim message (see ros/ros.h): the fields the nodes read.
#ifndef REF_SHIM_NAV_MSGS_ODOMETRY_H
#define REF_SHIM_NAV_MSGS_ODOMETRY_H

#include <geometry_msgs/Twist.h>

#include <memory>

namespace geometry_msgs
{
struct Point
{
        double x = 0.0, y = 0.0, z = 0.0;
};
struct Quaternion
{
        double x = 0.0, y = 0.0, z = 0.0, w = 1.0;
};
struct Pose
{
        Point position;
        Quaternion orientation;
};
struct PoseWithCovariance
{
        Pose pose;
};
struct TwistWithCovariance
{
        Twist twist;
};
} // namespace geometry_msgs

namespace nav_msgs
{
struct Odometry
{
        geometry_msgs::PoseWithCovariance pose;
        geometry_msgs::TwistWithCovariance twist;
        typedef std::shared_ptr<Odometry> Ptr;
        typedef std::shared_ptr<const Odometry> ConstPtr;
};
} // namespace nav_msgs

#endif

// Shim message (see ros/ros.h): the fields the nodes read.
#ifndef REF_SHIM_GEOMETRY_MSGS_TWIST_H
#define REF_SHIM_GEOMETRY_MSGS_TWIST_H

#include <memory>

namespace geometry_msgs
{
struct Vector3
{
        double x = 0.0, y = 0.0, z = 0.0;
};
struct Twist
{
        Vector3 linear, angular;
        typedef std::shared_ptr<Twist> Ptr;
        typedef std::shared_ptr<const Twist> ConstPtr;
};
} // namespace geometry_msgs

#endif

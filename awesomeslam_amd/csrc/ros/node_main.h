// ros/node_main.h -- the reference's node surface (awesome_slam/src/ekf/ekf.cpp:39-46,74-114,313-326; src/ukf/ukf.cpp:39-46,70-110,394-407)
// on top of the host mirror aslam::EKFSlam / aslam::UKFSlam (../host/aslam_node.h), whose covariance and slam() live on the MI355X behind
// include/aslam_core.h.  One template for both executables: they differ in the filter class, the node name, the subscriber queue size
// (1 for the EKF, 10 for the UKF) and the start-up message, exactly as the reference's two main() do.
//
// Compile-gated: built only where catkin/roscpp and awesome_slam_msgs exist (ros/CMakeLists.txt).  This repository's image has no ROS;
// tests/test_ros_wrappers.py compiles and links both executables against the minimal interface stubs in tests/ros_stub/ (syntax, types and
// the aslam_node.h calls -- nothing about ROS behaviour).
#pragma once

#include <type_traits>
#include <awesome_slam_msgs/Landmarks.h>
#include <nav_msgs/Odometry.h>
#include <ros/ros.h>

#include <iostream>

#include "../host/aslam_node.h"

namespace aslam_ros
{
template <class Filter> struct Node
{
        Filter filter;
        ros::NodeHandle nh;
        ros::Subscriber sub_odom, sub_sensor_landmark;
        ros::Publisher pub_landmark;
        // forgetting policy (~forget_after, ~forget_period; in callbacks): every forget_period counted callbacks the landmarks last sighted more than
        // forget_after callbacks ago are removed (FilterNode::removeStale).  forget_after = 0, the default: never
        uint32_t forget_after = 0, forget_period = 1;
        // duplicate merging (~merge_gate, ~merge_dist, ~merge_period): every merge_period counted callbacks the landmark pairs within merge_dist
        // of each other whose Mahalanobis distance is below merge_gate are fused and one of each removed (FilterNode::mergeDuplicates;
        // 5.99 is the 95 % point of chi-square with 2 degrees of freedom).  merge_gate = 0, the default: never
        double merge_gate = 0.0, merge_dist = 1.0;
        uint32_t merge_period = 1;

        /// the reference's constructor (ekf.cpp:39-46): subscribe, advertise, initialize() -- whose `last_time = ros::Time::now().toSec()`
        /// (ekf.cpp:54) is the `now_init` of the mirror
        Node(int max_landmark_count, uint32_t queue_size) : filter(max_landmark_count, 0, ros::Time::now().toSec())
        {
                sub_odom = nh.subscribe("/odom", queue_size, &Node::cbOdom, this);
                sub_sensor_landmark = nh.subscribe("/out/landmarks/sensor", queue_size, &Node::cbSensorLandmark, this);
                pub_landmark = nh.template advertise<awesome_slam_msgs::Landmarks>("out/landmarks/kalman", 1);
        }

        /// ekf.cpp:74-99: delta_time from the clock, updateZandA, slam(), publish the landmark estimates
        void cbOdom(const nav_msgs::Odometry::ConstPtr &msg)
        {
                const aslam::Odometry o{msg->pose.pose.position.x,    msg->pose.pose.position.y,    msg->pose.pose.orientation.w,
                                        msg->pose.pose.orientation.x, msg->pose.pose.orientation.y, msg->pose.pose.orientation.z,
                                        msg->twist.twist.linear.x,    msg->twist.twist.angular.z};
                if (!filter.cbOdom(o, ros::Time::now().toSec()))
                        return; // no sensor message yet (ekf.cpp:76-77)
                if (forget_after && filter.clock() % forget_period == 0)
                        filter.removeStale(forget_after);
                if (merge_gate > 0.0 && filter.clock() % merge_period == 0)
                        filter.mergeDuplicates(merge_gate, merge_dist);
                const aslam::Landmarks l = filter.landmarks(); // convertToLandmarkMsg, common.h:93-108
                awesome_slam_msgs::Landmarks out;
                out.x = l.x;
                out.y = l.y;
                pub_landmark.publish(out);
        }

        /// ekf.cpp:102-114
        void cbSensorLandmark(const awesome_slam_msgs::Landmarks::ConstPtr &msg)
        {
                filter.cbSensorLandmark(aslam::Landmarks{msg->x, msg->y});
        }
};

/// the reference's main() (ekf.cpp:313-326): init, Rate(FREQ), the node object, the 1 Hz spin loop
template <class Filter> int node_main(int argc, char **argv, const char *node_name, uint32_t queue_size, const char *banner)
{
        ros::init(argc, argv, node_name);
        ros::Time::init();
        ros::Rate rate(1); // FREQ, config.h:42
        int max_landmark_count = 30; // config.h:45; a private parameter here instead of a recompile
        ros::param::param("~max_landmark_count", max_landmark_count, 30);
        // the filter constants of config.h:43-66, private parameters too (aslam_params, aslam_core.h; the defaults are the reference's values)
        aslam_params prm = ASLAM_PARAMS_DEFAULT_INIT;
        const aslam_params def = prm;
        ros::param::param("~r_xy", prm.r_xy, def.r_xy);
        ros::param::param("~r_yaw", prm.r_yaw, def.r_yaw);
        ros::param::param("~r_range", prm.r_range, def.r_range);
        ros::param::param("~r_bearing", prm.r_bearing, def.r_bearing);
        ros::param::param("~q_xy", prm.q_xy, def.q_xy);
        ros::param::param("~q_yaw", prm.q_yaw, def.q_yaw);
        ros::param::param("~p0_pose", prm.p0_pose, def.p0_pose);
        ros::param::param("~p0_landmark", prm.p0_landmark, def.p0_landmark);
        ros::param::param("~var_a", prm.var_a, def.var_a);
        double assoc_dist = def.assoc_dist; // (the parameter server has no binary32 and no unsigned type)
        int promote_count = (int)def.promote_count;
        ros::param::param("~assoc_dist", assoc_dist, (double)def.assoc_dist);
        ros::param::param("~promote_count", promote_count, (int)def.promote_count);
        prm.assoc_dist = (float)assoc_dist;
        prm.promote_count = promote_count < 0 ? 0u : (uint32_t)promote_count; // (0 is refused by setParams, with the field's name)
        int forget_after = 0, forget_period = 1;
        ros::param::param("~forget_after", forget_after, 0);
        ros::param::param("~forget_period", forget_period, 1);
        double merge_gate = 0.0, merge_dist = 1.0;
        int merge_period = 1;
        ros::param::param("~merge_gate", merge_gate, 0.0);
        ros::param::param("~merge_dist", merge_dist, 1.0);
        ros::param::param("~merge_period", merge_period, 1);
        // ~assoc_gate: associate by the Mahalanobis gate (FilterNode::setAssocGate; 9.21 is the 99 % point of chi-square with 2 degrees of
        // freedom) and drop the observations it refuses although they lie within assoc_dist.  0, the default: the reference's Euclidean rule
        double assoc_gate = 0.0;
        ros::param::param("~assoc_gate", assoc_gate, 0.0);
        // ~joint_prob: behind the gate, test the gated pairings of a message jointly (FilterNode::setJointProb) at this chi-square probability
        // and drop the ones the set refuses.  0, the default: off; values outside (0, 1) are taken as 0.  No effect while ~assoc_gate is 0
        double joint_prob = 0.0;
        ros::param::param("~joint_prob", joint_prob, 0.0);
        Node<Filter> a(max_landmark_count, queue_size);
        a.filter.setAssocGate(assoc_gate > 0.0 ? assoc_gate : 0.0);
        a.filter.setJointProb(joint_prob > 0.0 && joint_prob < 1.0 ? joint_prob : 0.0);
        a.merge_gate = merge_gate > 0.0 ? merge_gate : 0.0;
        a.merge_dist = merge_dist > 0.0 ? merge_dist : 1.0;
        a.merge_period = merge_period < 1 ? 1u : (uint32_t)merge_period;
        a.forget_after = forget_after < 0 ? 0u : (uint32_t)forget_after;
        a.forget_period = forget_period < 1 ? 1u : (uint32_t)forget_period;
        a.filter.setParams(prm); // before the first callback: p0_pose applies
        if constexpr (std::is_same<Filter, aslam::EKFSlam>::value)
        {
                // ~sighted_only (EKF executable): update with the landmarks each callback sighted, not with the stale readings of the rest
                bool sighted_only = false;
                ros::param::param("~sighted_only", sighted_only, false);
                if (sighted_only)
                        a.filter.setSightedOnly(true);
        }
        std::cerr << banner;
        while (ros::ok())
        {
                ros::spinOnce();
                rate.sleep();
        }
        return 0;
}
} // namespace aslam_ros

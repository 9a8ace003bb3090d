// Shim of the slice of roscpp that the reference's nodes use.  TEST INFRASTRUCTURE ONLY (see eigen3/Eigen/Core); our own text.
// There is no middleware: subscribe() keeps the member callback so that a driver can hand it a message, advertise()/publish()
// keep the last message, Time::now() reads a clock that the driver sets, and init/ok/spinOnce/Rate do nothing.
#ifndef REF_SHIM_ROS_H
#define REF_SHIM_ROS_H

// the real header brings these in, and the nodes rely on it
#include <cassert>
#include <cmath>
#include <cstdint>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef REF_SHIM_ASSERT_THROWS
// The scan driver has to survive the node's own assert (the nodes are built without NDEBUG, as the reference's CMake builds
// them): the condition is evaluated as written, a failure is reported as an exception in place of abort().
namespace ros_shim
{
struct AssertFailed : std::runtime_error
{
        explicit AssertFailed(const char *what) : std::runtime_error(what) {}
};
} // namespace ros_shim
#undef assert
#define assert(expr) ((expr) ? static_cast<void>(0) : throw ros_shim::AssertFailed(#expr))
#endif

namespace ros
{
inline double &shim_clock()
{
        static double now = 0.0;
        return now;
}

class Time
{
      public:
        Time() : sec_(0.0) {}
        explicit Time(double s) : sec_(s) {}
        static void init() {}
        static Time now() { return Time(shim_clock()); }
        static void setNow(double s) { shim_clock() = s; }
        double toSec() const { return sec_; }

      private:
        double sec_;
};

class Rate
{
      public:
        explicit Rate(double) {}
        bool sleep() { return true; }
};

inline void init(int &, char **, const std::string &) {}
inline bool ok() { return false; }
inline void spinOnce() {}

class Subscriber
{
};

class Publisher
{
      public:
        Publisher() : last_(std::make_shared<std::shared_ptr<void>>()), count_(std::make_shared<uint64_t>(0)) {}
        template <typename M> void publish(const M &msg) const
        {
                *last_ = std::make_shared<M>(msg);
                ++*count_;
        }
        template <typename M> std::shared_ptr<const M> last() const { return std::static_pointer_cast<const M>(*last_); }
        uint64_t count() const { return *count_; }

      private:
        std::shared_ptr<std::shared_ptr<void>> last_;
        std::shared_ptr<uint64_t> count_;
};

class NodeHandle
{
      public:
        NodeHandle() : subs_(std::make_shared<std::map<std::string, std::function<void(const std::shared_ptr<const void> &)>>>()) {}

        template <typename M, typename T>
        Subscriber subscribe(const std::string &topic, uint32_t, void (T::*fp)(const std::shared_ptr<const M> &), T *obj)
        {
                (*subs_)[topic] = [fp, obj](const std::shared_ptr<const void> &m) { (obj->*fp)(std::static_pointer_cast<const M>(m)); };
                return Subscriber();
        }

        template <typename M> Publisher advertise(const std::string &, uint32_t) { return Publisher(); }

        // driver side: run the callback subscribed to `topic`; false when nobody subscribed
        template <typename M> bool deliver(const std::string &topic, const std::shared_ptr<const M> &msg) const
        {
                auto it = subs_->find(topic);
                if (it == subs_->end())
                        return false;
                it->second(msg);
                return true;
        }

      private:
        std::shared_ptr<std::map<std::string, std::function<void(const std::shared_ptr<const void> &)>>> subs_;
};
} // namespace ros

#endif

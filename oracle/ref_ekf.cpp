// The reference's EKF node behind the orc_* interface (see ref_filter_driver.h; recipe: `make ref`).  TEST INFRASTRUCTURE ONLY.
// The node's source is compiled from the reference's own directory, given on the command line; none of it is copied here.
#include "ekf.cpp"

typedef aslam::EKFSlam RefNode;
#define REF_KIND ORC_EKF
#define REF_IS_EKF 1
#include "ref_filter_driver.h"

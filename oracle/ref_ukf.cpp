// The reference's UKF node behind the orc_* interface (see ref_filter_driver.h; recipe: `make ref`).  TEST INFRASTRUCTURE ONLY.
// The node's source is compiled from the reference's own directory, given on the command line; none of it is copied here.
#include "ukf.cpp"

typedef aslam::UKFSlam RefNode;
#define REF_KIND ORC_UKF
#define REF_IS_EKF 0
#include "ref_filter_driver.h"

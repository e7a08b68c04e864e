// modules/egomotion.hpp -- an extension module (the reference estimates no pose): stereo visual odometry from the ORB matches of
// the "feature_matches" module, through cart_ego_* (include/cart_engine.h), spec DESIGN.md S23.  Factory type "ego_motion".
#pragma once
#include <memory>

#include "../cartslam.hpp"
#include "cart_engine.h"
#include "features.hpp"
#include "matches.hpp"

#define CARTSLAM_KEY_EGO_MOTION "ego_motion"

namespace cart {
struct EgoMotion {
    cart_ego_result result;   // p_cur = R p_prev + t against the previous frame; status 0 with the identity for frame 1
    double pose[12];          // accumulated camera-to-world 3 x 4 in KITTI pose order: T_w(t) = T_w(t-1) inv(T_rel); kept when status is 0
    image_t landmarks;        // device, one row of bytes: double [capacity][4] = (X, Y, Z, valid) per left keypoint index of the frame
};
static_assert(sizeof(cart_ego_result) == 120, "cart_ego_result layout");

// All defaults are build-owned choices that no data set has tuned.
struct EgoMotionOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    double minDisparity = 1.0, inlierThreshold = 2.0;      // cart_ego_default_params
    int hypotheses = 256, refineIterations = 4;
    uint64_t seed = 0;
};

// T_w(t) = T_w(t-1) inv(T_rel) with inv = (R^T, -R^T t), in plain double loops (restated in tests/np_ego.py, chain)
void chainPose(const double previous[12], const cart_ego_result &relative, double out[12]);

class EgoPool;

class EgoMotionModule : public SyncWrapperSystemModule {
   public:
    explicit EgoMotionModule(const EgoMotionOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~EgoMotionModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const EgoMotionOptions options;
    std::shared_ptr<EgoPool> pool;
};
}  // namespace cart

// modules/fusion.hpp -- an extension module (the reference fuses nothing over time): the previous frame's fused disparity carried through
// the relative pose into this frame and fused with this frame's "disparity", through cart_fusion_* (include/cart_engine.h), spec
// DESIGN.md S28.  No optical flow.  Factory type "temporal_fusion".
#pragma once
#include <memory>
#include <mutex>
#include <string>

#include "../cartslam.hpp"
#include "cart_engine.h"

#define CARTSLAM_KEY_DISPARITY_FUSED "disparity_fused"                  // CV_16SC1, the format of "disparity"
#define CARTSLAM_KEY_DISPARITY_AGE "disparity_age"                      // CV_8UC1: frames a pixel's depth has been confirmed for
#define CARTSLAM_KEY_DISPARITY_SOURCE "disparity_source"                // CV_8UC1: CART_FUSION_*
#define CARTSLAM_KEY_DISPARITY_FUSION_COUNTS "disparity_fusion_counts"  // FusionCounts

namespace cart {
struct FusionCounts {
    int32_t pixels[5];   // per source class, CART_FUSION_NONE .. CART_FUSION_PREDICTED
};

// The five parameters are build-owned choices that no data set has tuned.
struct TemporalFusionOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    double minDisparity = 1.0, agreeThreshold = 1.0, splatRadius = 0.75;   // cart_fusion_default_params
    int maxWeight = 4, minAge = 2;
    bool useMotion = false;               // "motion" of this frame masks the prediction, of the previous frame the sources
    std::string poseKey = "ego_motion";   // the blackboard EgoMotion whose relative pose carries the image; "dense_ego" = the refined one
};

class TemporalFusionModule : public SyncWrapperSystemModule {
   public:
    explicit TemporalFusionModule(const TemporalFusionOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~TemporalFusionModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const TemporalFusionOptions options;
    std::mutex mutex;                // one frame at a time: every frame feeds on the one before
    cart_fusion *object = nullptr;   // made for the first frame's size
    DeviceScratch scratch;           // the one stream; the counts on the device and the pinned buffer they are downloaded through
};
}  // namespace cart

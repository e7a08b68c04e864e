// modules/motionseg.hpp -- an extension module (the reference has no such stage): which pixels moved on their own, from this frame's
// and the previous frame's "disparity", the "optflow" that links them and the relative pose of "ego_motion", through
// cart_motion_segment (include/cart_engine.h), spec DESIGN.md S25.  Factory type "motion_seg".
#pragma once
#include <memory>
#include <mutex>

#include "../cartslam.hpp"
#include "cart_engine.h"

#ifndef CV_16SC4
#define CV_16SC4 27  // OpenCV's code: depth 3 (16S) + ((4 - 1) << 3)
#endif
#define CARTSLAM_KEY_MOTION "motion"                            // CV_8UC1: 0 static, 1 moving, 2 unknown (the Plane enum's values)
#define CARTSLAM_KEY_MOTION_UNSMOOTHED "motion_unsmoothed"      // the raw labels
#define CARTSLAM_KEY_MOTION_RESIDUAL "motion_residual"          // CV_16SC4: (Q(eu), Q(ev), Q(ed), raw label)
#define CARTSLAM_KEY_PLANES_STATIC "planes_static"              // "planes" with the moving pixels UNKNOWN ("planes": true)
#define CARTSLAM_KEY_MOTION_COMPONENTS "motion_components"      // as "plane_components" and its table and count ("components": true)
#define CARTSLAM_KEY_MOTION_COMPONENT_TABLE "motion_component_table"
#define CARTSLAM_KEY_MOTION_COMPONENT_COUNT "motion_component_count"

namespace cart {
// The five parameters are build-owned choices that no data set has tuned.
struct MotionSegOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    double minDisparity = 1.0, flowThreshold = 2.0, disparityThreshold = 1.0;   // cart_motion_default_params
    int radius = 2, supportPercent = 50;
    bool planes = false, components = true;
};

class MotionSegModule : public SyncWrapperSystemModule {
   public:
    explicit MotionSegModule(const MotionSegOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~MotionSegModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    struct Outputs {
        std::shared_ptr<image_t> labels, raw, residual, components, componentTable, componentCount;
    };
    void label(const Outputs &out);   // cart_plane_ccl_table on out.labels
    const MotionSegOptions options;
    std::mutex mutex;                 // guards the lazy creation and the enqueue on the one stream; released before the frame's wait, so frames overlap their host side
    cart_engine *engine = nullptr;
    DeviceScratch scratch;            // the one stream (no buffers)
    std::shared_ptr<Outputs> unknown; // what every frame without an estimate publishes, made once
};
}  // namespace cart

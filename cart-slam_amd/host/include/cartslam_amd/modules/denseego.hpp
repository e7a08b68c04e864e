// modules/denseego.hpp -- an extension module (the reference estimates no pose): the relative pose of "ego_motion" refined over every
// static pixel of this frame's and the previous frame's "disparity" and the "optflow" that links them, through cart_dense_ego_*
// (include/cart_engine.h), spec DESIGN.md S26.  Factory type "dense_ego".
#pragma once
#include <memory>
#include <mutex>

#include "../cartslam.hpp"
#include "cart_engine.h"
#include "egomotion.hpp"

#define CARTSLAM_KEY_DENSE_EGO "dense_ego"                 // EgoMotion: the relative pose that was chained and the accumulated pose
#define CARTSLAM_KEY_DENSE_EGO_RESULT "dense_ego_result"   // cart_dense_ego_result as the device wrote it

namespace cart {
static_assert(sizeof(cart_dense_ego_result) == 136, "cart_dense_ego_result layout");

// The seven parameters are build-owned choices that no data set has tuned.
struct DenseEgoOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    double minDisparity = 1.0, flowThreshold = 2.0, disparityThreshold = 1.0, disparityWeight = 1.0;   // cart_dense_ego_default_params
    int iterations = 4, stride = 1, minInliers = 1024;
    bool useMotion = false;   // leave out the pixels "motion" calls MOVING
};

// The consumer's rule of S26: the refined pose iff status == 1, all 12 entries are finite and n_inliers >= n_initial.
bool acceptDenseEgo(const cart_dense_ego_result &r);
// The consumer's rule of spec S34 (frame-to-model tracking, the voxel_map module's "track"): the refined pose is taken iff status == 1, every
// number of the record is finite, rms <= rms_initial and n_inliers >= minInliers (restated in tests/np_modeltrack.py, accept).
bool acceptModelTrack(const cart_model_track_result &r, int minInliers);
// The consumer's rule of spec S38 (colour-aided tracking, the voxel_map module's "track_color"): the refined pose is taken iff status == 1,
// every number of the record is finite, cost <= cost_initial and n_inliers >= minInliers (restated in tests/np_modeltrack_color.py, accept).
bool acceptModelTrackColor(const cart_model_track_color_result &r, int minInliers);

class DenseEgoModule : public SyncWrapperSystemModule {
   public:
    explicit DenseEgoModule(const DenseEgoOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~DenseEgoModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const DenseEgoOptions options;
    std::mutex mutex;                    // one frame at a time: every frame chains on the one before
    cart_dense_ego *object = nullptr;    // made for the first frame's size
    DeviceScratch scratch;               // the one stream; the result on the device and the pinned buffer it is downloaded through
};
}  // namespace cart

// modules/localba.hpp -- an extension module (the reference refines no trajectory): the last `window` frames, the feature tracks they
// share and a windowed bundle adjustment over both, through cart_local_ba_* (include/cart_engine.h, spec DESIGN.md S32).  Every frame
// publishes the refined pose as an EgoMotion under "local_ba", so "pose_key": "local_ba" hands it to plane_map and temporal_fusion.
// Factory type "local_ba".
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../cartslam.hpp"
#include "cart_engine.h"
#include "egomotion.hpp"

#define CARTSLAM_KEY_LOCAL_BA "local_ba"
#define CARTSLAM_KEY_LOCAL_BA_RESULT "local_ba_result"
#define CARTSLAM_KEY_LOCAL_BA_WINDOW "local_ba_window"

namespace cart {
struct LocalBARecord {
    cart_local_ba_result result;   // of this frame's optimise; all zeros on a frame that did not optimise
    int32_t counts[8];             // of this frame's push: {left keypoints, stereo-valid, continued, born, dropped, freed, live points, frames in window}
    int32_t taken;                 // 1 = the published pose is the optimised one; 0 = the carried estimate (no optimise, status 0, or the cost rose)
    int32_t optimised;             // 1 = this frame optimised
};
static_assert(sizeof(LocalBARecord) == 80, "LocalBARecord layout (tests/np_localba.py MODULE_DTYPE)");

struct LocalBAWindow {             // the window after the frame, in age order (oldest first), rows past the frames in it zero
    std::vector<uint64_t> ids;     // [window]
    std::vector<double> poses;     // [window][12]
};

// All defaults are build-owned choices that no data set has tuned.
struct LocalBAOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    double minDisparity = 1.0, huber = 2.0, damping = 0.0;          // cart_local_ba_default_params
    int iterations = 4, minObservations = 2, minFrameObservations = 6;
    int window = 8, maxPoints = 8192;
    int interval = 1;                          // optimise on every interval-th frame
    std::string poseKey = CARTSLAM_KEY_EGO_MOTION;   // the blackboard EgoMotion whose chained pose is the odometry; "dense_ego" = the refined one
};

class LocalBAModule : public SyncWrapperSystemModule {
   public:
    explicit LocalBAModule(const LocalBAOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~LocalBAModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const LocalBAOptions options;
    std::mutex mutex;                    // one frame at a time: the window is the module's state
    cart_local_ba *ba = nullptr;
    int capacity = 0;                    // of the first frame's feature sets: the object is made for it
    DeviceScratch scratch;               // the one stream; the record, the poses before and after the optimise and the ids: on the device and the pinned buffer they come through
};
}  // namespace cart

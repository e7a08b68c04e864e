// modules/loopclosure.hpp -- an extension module (the reference recognises no place): every keyframe's left ORB features are scored
// against a device-resident ring of earlier keyframes through cart_place_* (include/cart_engine.h, spec DESIGN.md S27), the best
// candidates are verified by a cross-checked match and a relative pose (cart_matcher_match, cart_ego_estimate), and the frame is stored.
// Factory type "loop_closure".  Pose-graph optimisation is not done here: the module ends at the verified constraint, which modules/posegraph.hpp consumes.
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../cartslam.hpp"
#include "cart_engine.h"
#include "egomotion.hpp"

#define CARTSLAM_KEY_LOOP_CLOSURE "loop_closure"

namespace cart {
struct LoopClosure {           // all zeros on a frame that is no keyframe and on a keyframe without an accepted candidate
    int32_t detected;          // 1 = a stored keyframe was recognised and verified
    int32_t slot, score;       // the candidate's slot in the ring and its vote count
    int32_t reserved;
    uint64_t keyframeId;       // the frame id of the recognised keyframe
    cart_ego_result relative;  // p_cur = R p_kf + t
    double poseKeyframe[12];   // the accumulated pose the keyframe was stored with
    double poseLoop[12];       // chainPose(poseKeyframe, relative): where the loop says this frame is; compare with the chained pose
};
static_assert(sizeof(LoopClosure) == 336, "LoopClosure layout (tests/np_place.py LOOP_DTYPE)");

// All defaults are build-owned choices that no data set has tuned.
struct LoopClosureOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    int maxDistance = 64, ratio = 80, minScore = 30, maxCandidates = 4;   // cart_place_default_params; the first two also rule the verifying match
    uint64_t minGap = 50;
    int capacity = 256, keyframeInterval = 5, verify = 1, minInliers = 30;
    uint64_t seed = 0;
    double minDisparity = 1.0, inlierThreshold = 2.0;      // cart_ego_default_params
    int hypotheses = 256, refineIterations = 4;
    std::string poseKey = CARTSLAM_KEY_EGO_MOTION;         // the blackboard EgoMotion whose accumulated pose a keyframe is stored with; "dense_ego" = the refined one
};

class LoopClosureModule : public SyncWrapperSystemModule {
   public:
    explicit LoopClosureModule(const LoopClosureOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~LoopClosureModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    struct Keyframe {
        uint64_t id = 0;
        double pose[12] = {};
    };
    const LoopClosureOptions options;
    std::mutex mutex;                    // one frame at a time: the ring is the module's state
    int featureCapacity = 0;             // capacity of the feature sets the objects were made for (the first keyframe's)
    cart_place_db *db = nullptr;
    cart_matcher *matcher = nullptr;
    cart_ego *ego = nullptr;
    DeviceScratch scratch;               // the one stream; candidates, counts, the pose result and the match list on the device; the pinned buffer they come through
    std::vector<Keyframe> keyframes;     // per slot: what the ring holds there
};
}  // namespace cart

// modules/matches.hpp -- an extension module (the reference's feature module only draws its keypoints): stereo and temporal
// correspondences between the ORB features of the "features" module, through cart_matcher_* (include/cart_engine.h), spec
// DESIGN.md S22.  Factory type "orb_matches".
#pragma once
#include <memory>
#include <vector>

#include "../cartslam.hpp"
#include "cart_engine.h"
#include "features.hpp"

#define CARTSLAM_KEY_FEATURE_MATCHES "feature_matches"

namespace cart {
typedef cart_match FeatureMatch;   // query, train, distance, second
static_assert(sizeof(FeatureMatch) == 16, "cart_match layout");

struct FeatureMatches {
    std::vector<FeatureMatch> stereo;     // query = left, train = right of the frame
    std::vector<FeatureMatch> temporal;   // query = left of the frame, train = left of the previous frame; empty for frame 1

    // What cart_matcher_match wrote, still on the device and owned by the frame (empty when made from host data), for consumers
    // that stay on the device (modules/egomotion.hpp): list 0 = stereo, 1 = temporal; a list that was not matched has count 0.
    bool onDevice() const { return !records.empty(); }
    const int32_t *deviceCount(int list) const { return records.ptr<int32_t>() + list; }
    const FeatureMatch *deviceMatches(int list) const { return reinterpret_cast<const FeatureMatch *>(records.ptr<uint8_t>() + 16) + (size_t)list * capacity; }
    int deviceCapacity() const { return capacity; }   // records each list holds

    image_t records;   // one row of bytes: counts [2] int32, 8 B padding, matches [2][capacity]
    int capacity = 0;
};

struct FeatureMatcherOptions {
    bool stereo = true, temporal = true;
    int maxDistance = 64, ratio = 80;   // cart_match_default_params
    bool crossCheck = true;
    // The presets are build-owned choices, not tuned on any data set.
    float maxDisparity = 256.f;   // stereo gate: left.x - right.x in [0, maxDisparity]
    float maxDy = 2.f;            //              left.y - right.y in [-maxDy, maxDy]
    float searchRadius = 128.f;   // temporal gate: both offsets in [-searchRadius, searchRadius]
};

class MatcherPool;

class FeatureMatcherModule : public SyncWrapperSystemModule {
   public:
    explicit FeatureMatcherModule(const FeatureMatcherOptions &options = FeatureMatcherOptions());
    ~FeatureMatcherModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const FeatureMatcherOptions options;
    std::shared_ptr<MatcherPool> pool;
};
}  // namespace cart

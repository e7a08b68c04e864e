// modules/features.hpp -- mirrors include/modules/features.hpp + src/modules/features.cpp: the ORB feature detector module
// (same role, blackboard key and error text).  cv::cuda::ORB::detectAndComputeAsync + convert run behind cart_orb_*
// (include/cart_engine.h), spec DESIGN.md S20; the descriptors stay on the device, the keypoints come to the host.
#pragma once
#include <memory>
#include <utility>
#include <vector>

#include "../cartslam.hpp"
#include "cart_engine.h"

#define CARTSLAM_OPTION_KEYPOINTS 5000

#define CARTSLAM_KEY_FEATURES "features"

namespace cart {
typedef cart_keypoint KeyPoint;   // cv::KeyPoint's layout: pt.x, pt.y, size, angle, response, octave, class_id
static_assert(sizeof(KeyPoint) == 28, "cv::KeyPoint layout");

class ImageFeatures {
   public:
    ImageFeatures(std::vector<KeyPoint> keypoints, image_t descriptors) : keypoints(std::move(keypoints)), descriptors(descriptors) {}

    std::vector<KeyPoint> keypoints;
    image_t descriptors;   // CV_8UC1, keypoints.size() rows of 32 bytes (device)
};

// Per-thread cart_orb workspaces of one module (the frames of a run may overlap).
class OrbPool;

// The reference's detectOrbFeatures (features.cpp:48-66) for both images of a frame: one cart_orb_detect for the pair, one
// download of the counts and keypoints through the workspace slot's pinned buffer (the frame's one host synchronisation).
std::pair<ImageFeatures, ImageFeatures> detectOrbFeatures(OrbPool &pool, const image_t &left, const image_t &right);

class ImageFeatureDetectorModule : public SyncWrapperSystemModule {
   public:
    explicit ImageFeatureDetectorModule(int nfeatures = CARTSLAM_OPTION_KEYPOINTS);
    ~ImageFeatureDetectorModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    std::shared_ptr<OrbPool> pool;
};
}  // namespace cart

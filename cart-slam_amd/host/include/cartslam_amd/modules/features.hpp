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
    ImageFeatures(std::vector<KeyPoint> keypoints, image_t descriptors, image_t records, size_t countOffset, size_t keypointOffset, int capacity)
        : keypoints(std::move(keypoints)), descriptors(descriptors), records(records), countOffset(countOffset), keypointOffset(keypointOffset),
          capacity(capacity) {}

    std::vector<KeyPoint> keypoints;
    image_t descriptors;   // CV_8UC1, keypoints.size() rows of 32 bytes (device)

    // What cart_orb_detect wrote for this image, still on the device and owned by the frame (empty when made from host data):
    // the keypoint count and `capacity` keypoint records, for consumers that stay on the device (modules/matches.hpp).
    bool onDevice() const { return !records.empty(); }
    const int32_t *deviceCount() const { return reinterpret_cast<const int32_t *>(records.ptr<uint8_t>() + countOffset); }
    const KeyPoint *deviceKeypoints() const { return reinterpret_cast<const KeyPoint *>(records.ptr<uint8_t>() + keypointOffset); }
    int deviceCapacity() const { return capacity; }   // rows the descriptor image and the keypoint records hold

   private:
    image_t records;   // one row of bytes shared by both images of the frame: counts [2] int32, padding, keypoints [2][capacity]
    size_t countOffset = 0, keypointOffset = 0;
    int capacity = 0;
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

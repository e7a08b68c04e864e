// modules/objects.hpp -- an extension module (the reference tracks nothing): the moving things of a frame as objects in metres and
// their tracks from frame to frame, from the "motion_components" of motion_seg with their table and count, this frame's and the previous
// frame's "disparity", the "optflow" that links them and the relative and camera-to-world pose of "ego_motion", through
// cart_object_tracker_* (include/cart_engine.h), spec DESIGN.md S31.  Factory type "moving_objects".
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../cartslam.hpp"
#include "cart_engine.h"

#define CARTSLAM_KEY_MOVING_OBJECTS "moving_objects"   // MovingObjects

namespace cart {
struct MovingObjects {
    int32_t counts[8] = {};            // {table entries walked, n_selected, n_objects, n_valid, n_matched, n_born, n_dropped, n_live}
    std::vector<cart_object> objects;  // the frame's n_objects records, valid or not
    std::vector<cart_track> tracks;    // the live tracks in slot order
};

// The nine parameters are build-owned choices that no data set has tuned.
struct MovingObjectsOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    double minDisparity = 1.0, disparityBand = 2.0, maxSpeed = 5.0, gate = 2.0;   // cart_object_default_params
    int minArea = 64, minPoints = 16, gainPercent = 50, maxMissed = 3, minAge = 3;
    int maxObjects = 64, maxTracks = 64;
    std::string poseKey = "ego_motion";   // the blackboard EgoMotion: its result carries the image, its pose places the objects; "dense_ego" = the refined one
};

class MovingObjectsModule : public SyncWrapperSystemModule {
   public:
    explicit MovingObjectsModule(const MovingObjectsOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~MovingObjectsModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const MovingObjectsOptions options;
    std::mutex mutex;                       // one frame at a time: the tracks of a frame feed on the frame before
    cart_object_tracker *object = nullptr;  // made for the first frame's size
    DeviceScratch scratch;                  // the one stream; counts, objects and tracks on the device and the pinned buffer they are downloaded through
};
}  // namespace cart

// modules/planemap.hpp -- an extension module (the reference only paints one frame's vertical pixels into a picture,
// planeseg_vis.cu:58-107): the world-frame bird's-eye plane map through cart_plane_map_* (include/cart_engine.h), spec DESIGN.md S24.
// Every frame's "disparity" + "planes" vote into one rolling grid through the frame's camera-to-world pose, which comes from the
// "ego_motion" module or from a KITTI pose file.  Factory type "plane_map".
// With "rebuild" (spec S30) the module keeps every pose-graph keyframe's two images in a cart_plane_store, and on a frame whose graph was
// optimised it rebuilds the whole grid from them through the corrected node poses (cart_plane_map_rebuild) in place of the update.
#pragma once
#include <array>
#include <mutex>
#include <string>
#include <vector>

#include "../cartslam.hpp"
#include "cart_engine.h"

#define CARTSLAM_KEY_PLANE_MAP "plane_map"

namespace cart {
struct PlaneMap {
    int64_t originX = 0, originZ = 0;   // the window's first cell in absolute cells
    int cellsX = 0, cellsZ = 0;
    double cellSize = 0;
    image_t classes;                    // device u8 [cellsZ][cellsX] in window order: 0 free, 1 obstacle, 2 unknown
    std::vector<cart_plane_map_cell> cells;   // the cells in window order; filled only when CARTSLAM_PLANE_MAP_SNAPSHOT is set (--dump)
    int rebuilt = 0, rebuildUsed = 0;   // on a frame that rebuilt the grid (S30): the entries handed in, and those the store still held
    std::vector<uint64_t> rebuildIds;   // their frame ids
};

// The grid and vote defaults are build-owned choices that no data set has tuned; 20 and 10 are the reference's gates.
struct PlaneMapOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    int cellsX = 512, cellsZ = 512;
    double cellSize = 0.25, minDisparity = 1.0, maxDepth = 20.0, maxLateral = 10.0, heightQuantum = 0.05;   // cart_plane_map_default_params
    int minVotes = 3, obstaclePercent = 50;
    std::string planesKey = "planes";   // the blackboard image the map votes with; "planes_static" (motion_seg) maps the static world only
    std::string disparityKey = "disparity";   // the blackboard CV_16SC1 image the map votes with; "disparity_fused" = temporal_fusion's
    std::string poseKey = "ego_motion";   // the blackboard EgoMotion whose accumulated pose the map takes; "dense_ego" = the refined trajectory
    std::string poseFile;   // KITTI poses/NN.txt: 12 numbers per line, line id - 1 belongs to frame id; empty = the "ego_motion" module's pose
    bool rebuild = false;     // S30: re-vote the stored keyframes when pose_graph optimised; needs pose_key "pose_graph" and no pose_file
    int storeCapacity = 256;  // keyframes the store holds (a ring: the oldest leaves)
};

class PlaneMapModule : public SyncWrapperSystemModule {
   public:
    explicit PlaneMapModule(const PlaneMapOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~PlaneMapModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const PlaneMapOptions options;
    const bool snapshot;
    std::vector<std::array<double, 12>> poses;   // of the pose file
    std::vector<bool> poseGiven;
    std::mutex mutex;                            // the frames arrive one at a time (the -1 dependency); this guards the lazy creation
    cart_plane_map *map = nullptr;
    cart_plane_store *store = nullptr;           // with "rebuild": the keyframes' images
    std::vector<uint64_t> nodeFrame;             // frame id of every pose-graph node
    DeviceScratch scratch;                       // the one stream (no buffers)
};
}  // namespace cart

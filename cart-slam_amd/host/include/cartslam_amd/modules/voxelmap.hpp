// modules/voxelmap.hpp -- an extension module (the reference keeps no three-dimensional model): the rolling TSDF voxel map with model
// raycast through cart_voxel_map_* (include/cart_engine.h), spec DESIGN.md S33.  Every frame's disparity is integrated into one rolling
// volume through the frame's camera-to-world pose, and the volume is raycast from that pose into "disparity_model", an image in the
// format of "disparity".  Factory type "voxel_map".
// With "track" (spec DESIGN.md S34) the module keeps a pose chain of its own: every frame's predicted pose is refined against the volume
// through cart_model_track_* before the frame is integrated and raycast at the refined pose, published as "model_pose".
// With "rebuild" (spec DESIGN.md S35; needs "pose_key": "pose_graph" and no "track") the module keeps every keyframe's disparity in a
// device-resident store, and on a frame whose pose graph was optimised it rebuilds the whole volume from them through the corrected node
// poses (cart_voxel_map_rebuild) in place of the integrate, as the plane_map module does for its grid (S30).
// With "mesh" (spec DESIGN.md S36) every "mesh_interval"-th frame the module sees also extracts the window's surface after the integrate or
// rebuild (cart_voxel_map_mesh) and downloads the written records, published as "voxel_mesh".  The written counts size the download, so
// such a frame waits for the device twice; every other frame, and every frame without "mesh", once as before.
// With "color" (spec DESIGN.md S37) the module keeps a cart_voxel_color beside the map and colour-integrates the frame's reference image
// (8UC1 or 8UC3) right after the geometry integrate; on a frame that rebuilt the volume nothing is colour-integrated and the stored colours
// stay (the keyframe store holds no images).  With "raycast" it also publishes "image_model" and "image_model_alpha", the model's colours
// behind "disparity_model"; with "mesh", "voxel_mesh_colors" beside the unchanged "voxel_mesh".  Without "color" nothing changes.
// With "track_color" (spec DESIGN.md S38; needs "track" and "color") the frame's pose is refined through cart_model_track_refine_color with
// the frame's reference image, before the frame's geometry and colour integrates, so the model holds earlier frames only; the pose is
// taken by the cost rule and the whole record is published as "model_track_color_result" beside the unchanged "model_track_result".
#pragma once
#include <array>
#include <mutex>
#include <string>
#include <vector>

#include "../cartslam.hpp"
#include "cart_engine.h"

#define CARTSLAM_KEY_VOXEL_MAP "voxel_map"                                // VoxelMap
#define CARTSLAM_KEY_DISPARITY_MODEL "disparity_model"                    // CV_16SC1, the format of "disparity"; empty without "raycast"
#define CARTSLAM_KEY_DISPARITY_MODEL_STATUS "disparity_model_status"      // CV_8UC1: CART_VOXEL_RAY_*
#define CARTSLAM_KEY_DISPARITY_MODEL_COUNTS "disparity_model_counts"      // VoxelRayCounts
#define CARTSLAM_KEY_VOXEL_MESH "voxel_mesh"                              // VoxelMesh, with "mesh" only
#define CARTSLAM_KEY_VOXEL_COLOR "voxel_color"                            // VoxelColorFrame, with "color" only
#define CARTSLAM_KEY_IMAGE_MODEL "image_model"                            // CV_8UC3 (B, G, R), with "color" and "raycast"
#define CARTSLAM_KEY_IMAGE_MODEL_ALPHA "image_model_alpha"                // CV_8UC1: min(sum of the eight weights, 255); 0 = no colour
#define CARTSLAM_KEY_VOXEL_MESH_COLORS "voxel_mesh_colors"                // VoxelMeshColors, with "color" and "mesh"
#define CARTSLAM_KEY_MODEL_POSE "model_pose"                              // EgoMotion, with "track" only: the tracked pose and the relative pose between tracked poses
#define CARTSLAM_KEY_MODEL_TRACK_RESULT "model_track_result"              // cart_model_track_result as the device wrote it, with "track" only
#define CARTSLAM_KEY_MODEL_TRACK_COLOR_RESULT "model_track_color_result"  // cart_model_track_color_result as the device wrote it, with "track_color" only

namespace cart {
struct VoxelMap {
    int64_t origin[3] = {0, 0, 0};      // the window's first voxel in absolute voxels
    int32_t cells[3] = {0, 0, 0};       // cells_x, cells_y, cells_z
    double voxelSize = 0;
    int32_t counts[2] = {0, 0};         // of this frame's integrate: voxels updated, of them with f < 1
    std::vector<cart_voxel> voxels;     // the voxels in window order; filled only when CARTSLAM_VOXEL_MAP_SNAPSHOT is set
    int rebuilt = 0, rebuildUsed = 0;   // on a frame that rebuilt the volume (S35): the entries handed in, and those the store still held;
    int64_t rebuildCounts[2] = {0, 0};  // the rebuild's own counts (`counts` holds them cut to int32)
    std::vector<uint64_t> rebuildIds;   // the frame ids of the entries, in list order
};
struct VoxelMesh {                      // S36; `extracted` is false on the frames between two extractions, and everything else empty
    bool extracted = false;
    int64_t origin[3] = {0, 0, 0};      // the window the mesh belongs to
    double voxelSize = 0;
    int32_t counts[4] = {0, 0, 0, 0};   // vertices found, quads found, vertices written, quads written
    std::vector<cart_mesh_vertex> vertices;   // the written ones; positions relative to the window origin
    std::vector<cart_mesh_quad> quads;
};
struct VoxelColorFrame {                // S37
    bool integrated = false;            // false on a frame that rebuilt the volume: nothing was colour-integrated
    int32_t counts[2] = {0, 0};         // of this frame's colour integrate: voxels coloured, of them without a colour before
    int32_t rendered = 0;               // pixels of "image_model" with alpha > 0 (0 without "raycast")
    int64_t origin[3] = {0, 0, 0};      // the colour volume's window
    std::vector<cart_voxel_rgb> voxels; // the colour voxels in window order; filled only when CARTSLAM_VOXEL_MAP_SNAPSHOT is set
};
struct VoxelMeshColors {                // S37: one record per written vertex of the frame's "voxel_mesh", the weight byte holding alpha
    bool extracted = false;
    std::vector<cart_voxel_rgb> colors;
};
struct VoxelRayCounts {
    int32_t rays[3] = {0, 0, 0};        // CART_VOXEL_RAY_NONE, _HIT, _INSIDE
};

// Every default is a build-owned choice that no data set has tuned.
struct VoxelMapOptions : CameraOptions {   // the factory fills the camera from the data source's Q
    int cellsX = 256, cellsY = 64, cellsZ = 256;
    double voxelSize = 0.125, minDisparity = 1.0, minDepth = 0.5, maxDepth = 16.0, truncation = 0.25, disparitySigma = 0.5, lookahead = 8.0,
           marchStep = 0.125;             // cart_voxel_map_default_params
    int maxWeight = 64, minWeight = 1;
    std::string disparityKey = "disparity";   // the blackboard CV_16SC1 image that is integrated; "disparity_fused" = temporal_fusion's
    std::string poseKey = "ego_motion";       // the blackboard EgoMotion whose accumulated pose the map takes; "dense_ego", "local_ba", "pose_graph"
    bool useMotion = false;                   // "motion" of this frame masks the integration
    bool raycast = true;                      // publish the model image of every frame
    bool track = false;                       // S34: refine every frame's pose against the volume before integrating it
    bool rebuild = false;                     // S35: keep the keyframes' disparity and rebuild the volume when the pose graph was optimised
    int storeCapacity = 256;                  // keyframes the store holds (a ring: the oldest leaves)
    bool mesh = false;                        // S36: extract the window's surface every meshInterval-th frame
    int meshInterval = 10, meshMaxVertices = 1 << 20, meshMaxQuads = 1 << 20, meshMinWeight = 0;   // 0 = minWeight
    bool color = false;                       // S37: a colour volume beside the map, fed with the frame's reference image
    int colorMaxWeight = CART_VOXEL_COLOR_DEFAULT_MAX_WEIGHT;
    double residualGate = 0.9, damping = 0.01;   // cart_model_track_default_params
    int iterations = 4, stride = 1, minInliers = 1024;
    bool trackColor = false;                  // S38: "track" with the photometric term; needs track and color
    double photoWeight = 64.0, photoGate = 0.25;   // cart_model_track_color_default_params
    int colorMinWeight = 1;
};

static_assert(sizeof(cart_model_track_result) == 136, "cart_model_track_result layout");
static_assert(sizeof(cart_model_track_color_result) == 176, "cart_model_track_color_result layout");

class VoxelMapModule : public SyncWrapperSystemModule {
   public:
    explicit VoxelMapModule(const VoxelMapOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~VoxelMapModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const VoxelMapOptions options;
    const bool snapshot;
    std::mutex mutex;                 // the frames arrive one at a time (the -1 dependency); this guards the lazy creation
    cart_voxel_map *map = nullptr;
    cart_model_track *tracker = nullptr;   // with "track": made with the map
    cart_plane_store *store = nullptr;     // with "rebuild": made with the map
    cart_voxel_color *color = nullptr;     // with "color": made with the map
    std::vector<uint64_t> nodeFrame;       // with "rebuild": the frame id of every pose-graph node
    image_t zeroPlane;                     // with "rebuild" and without "use_motion": the stored u8 plane, zeroed once
    bool haveTracked = false;         // with "track": `tracked` holds the previous frame's tracked pose
    double tracked[12] = {};
    DeviceScratch meshBuffers;        // with "mesh": the device vertices and quads of one extraction (no stream, no host side)
    long long meshFrames = 0;         // with "mesh": frames seen
    DeviceScratch scratch;            // the one stream; the tracking records and the counts on the device and the pinned buffer they are downloaded through
};
}  // namespace cart

// voxelmap.cpp -- VoxelMapModule (cartslam_amd/modules/voxelmap.hpp): the rolling TSDF voxel map with model raycast, spec DESIGN.md S33; its rebuild from stored keyframes, S35; its surface mesh, S36; its colour companion, S37; colour-aided tracking, S38.
#include "cartslam_amd/modules/voxelmap.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "cartslam_amd/modules/denseego.hpp"
#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/motionseg.hpp"
#include "cartslam_amd/modules/posegraph.hpp"
#include "module_support.hpp"

namespace cart {
namespace {
cart_voxel_map_params paramsOf(const VoxelMapOptions &o) {
    return cart_voxel_map_params{o.voxelSize, o.minDisparity, o.minDepth, o.maxDepth, o.truncation, o.disparitySigma, o.lookahead, o.marchStep, o.maxWeight, o.minWeight};
}
cart_model_track_params trackParamsOf(const VoxelMapOptions &o) { return cart_model_track_params{o.residualGate, o.damping, o.iterations, o.stride, o.minInliers}; }
cart_model_track_color_params trackColorParamsOf(const VoxelMapOptions &o) { return cart_model_track_color_params{o.photoWeight, o.photoGate, o.colorMinWeight, 0}; }

// p_cur = R p_prev + t between two camera-to-world poses: R = Rc^T Rp, t = Rc^T (tp - tc), in plain double loops
void relativeOf(const double prev[12], const double cur[12], double R[9], double t[3]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (cur[r] * prev[c] + cur[4 + r] * prev[4 + c]) + cur[8 + r] * prev[8 + c];
        t[r] = (cur[r] * (prev[3] - cur[3]) + cur[4 + r] * (prev[7] - cur[7])) + cur[8 + r] * (prev[11] - cur[11]);
    }
}

constexpr size_t kCountsOffset = sizeof(cart_model_track_result);   // of the five counts in the scratch buffers, after the tracking record
constexpr size_t kRebuildCountsOffset = kCountsOffset + 8 * sizeof(int32_t);   // of the rebuild's two int64 counts, 8-byte aligned
static_assert(kRebuildCountsOffset % 8 == 0, "the rebuild's counts are int64");
constexpr size_t kMeshCountsOffset = kRebuildCountsOffset + 2 * sizeof(int64_t);   // of the mesh's four counts
constexpr size_t kColorCountsOffset = kMeshCountsOffset + 4 * sizeof(int32_t);   // of the colour integrate's two counts and the render's one
constexpr size_t kTrackColorOffset = kColorCountsOffset + 4 * sizeof(int32_t);   // of the colour-aided tracking record (S38), 8-byte aligned
static_assert(kTrackColorOffset % 8 == 0, "the colour-aided tracking record holds doubles");
constexpr size_t kScratchBytes = kTrackColorOffset + sizeof(cart_model_track_color_result);
}  // namespace

VoxelMapModule::VoxelMapModule(const VoxelMapOptions &options)
    : SyncWrapperSystemModule("VoxelMap"), options(options), snapshot(std::getenv("CARTSLAM_VOXEL_MAP_SNAPSHOT") != nullptr) {
    checkCamera(options);
    // the library's own checks, without a device: everything valid gets as far as the missing engine
    const cart_voxel_map_params p = paramsOf(options);
    cart_voxel_map *none = nullptr;
    (void)cart_voxel_map_create(nullptr, options.cellsX, options.cellsY, options.cellsZ, &p, &none);
    requireLibraryAccepts();
    if (options.disparityKey.empty()) throw std::invalid_argument("disparity_key must name a blackboard image");
    if (options.poseKey.empty()) throw std::invalid_argument("pose_key must name a blackboard pose");
    if (options.track) {
        // the tracked chain is the previous tracked pose and this frame's relative pose: the record must carry one, and past poses must stay
        if (options.poseKey != CARTSLAM_KEY_EGO_MOTION && options.poseKey != "dense_ego")
            throw std::invalid_argument("track needs a pose_key whose record carries a relative pose and never revises past poses (ego_motion, dense_ego), not " + options.poseKey);
        const cart_ego_camera cam = cameraOf(options);
        const cart_model_track_params tp = trackParamsOf(options);
        (void)cart_model_track_refine(nullptr, nullptr, &cam, kIdentityPose, &tp, nullptr, 0, nullptr, 0, 1, 1, nullptr, nullptr);
        requireLibraryAccepts();
    }
    if (options.trackColor) {
        if (!options.track || !options.color) throw std::invalid_argument("track_color requires \"track\": true and \"color\": true");
        const cart_ego_camera cam = cameraOf(options);
        const cart_model_track_params tp = trackParamsOf(options);
        const cart_model_track_color_params cp = trackColorParamsOf(options);
        (void)cart_model_track_refine_color(nullptr, nullptr, nullptr, &cam, kIdentityPose, &tp, &cp, nullptr, 0, nullptr, 0, 1, nullptr, 0, 1, 1, nullptr, nullptr);
        requireLibraryAccepts();
    }
    if (options.rebuild) {
        if (options.poseKey != CARTSLAM_KEY_POSE_GRAPH || options.track)
            throw std::invalid_argument("rebuild requires \"pose_key\": \"pose_graph\" and no track");
        cart_plane_store *none = nullptr;
        (void)cart_plane_store_create(nullptr, 1, 1, options.storeCapacity, &none);
        if (std::strcmp(cart_last_error(nullptr), "bad arguments") != 0) throw std::invalid_argument(std::string("store_capacity: ") + cart_last_error(nullptr));
    }
    if (options.mesh) {
        if (options.meshInterval < 1) throw std::invalid_argument("mesh_interval must be at least 1");
        if (options.meshMaxVertices < 1 || options.meshMaxVertices > 1 << 26) throw std::invalid_argument("mesh_max_vertices must be in [1, 2^26]");
        if (options.meshMaxQuads < 1 || options.meshMaxQuads > 1 << 26) throw std::invalid_argument("mesh_max_quads must be in [1, 2^26]");
        if (options.meshMinWeight < 0 || options.meshMinWeight > 65535) throw std::invalid_argument("mesh_min_weight must be 0 (min_weight) or in [1, 65535]");
    }
    if (options.color) {
        cart_voxel_color *none = nullptr;
        (void)cart_voxel_color_create(nullptr, nullptr, options.colorMaxWeight, &none);
        if (std::strcmp(cart_last_error(nullptr), "bad arguments") != 0) throw std::invalid_argument(std::string("color_max_weight: ") + cart_last_error(nullptr));
    }
    this->requiresData.push_back(module_dependency_t(options.disparityKey));
    this->requiresData.push_back(module_dependency_t(options.poseKey));
    if (options.useMotion) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION));
    if (options.rebuild) {
        this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_POSE_GRAPH_RESULT));
        this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_POSE_GRAPH_NODES));
    }
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_VOXEL_MAP, -1));   // one frame at a time, in order
    this->providesData.push_back(CARTSLAM_KEY_VOXEL_MAP);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_MODEL);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_MODEL_STATUS);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_MODEL_COUNTS);
    if (options.track) {
        this->providesData.push_back(CARTSLAM_KEY_MODEL_POSE);
        this->providesData.push_back(CARTSLAM_KEY_MODEL_TRACK_RESULT);
        if (options.trackColor) this->providesData.push_back(CARTSLAM_KEY_MODEL_TRACK_COLOR_RESULT);
    }
    if (options.mesh) this->providesData.push_back(CARTSLAM_KEY_VOXEL_MESH);
    if (options.color) {
        this->providesData.push_back(CARTSLAM_KEY_VOXEL_COLOR);
        this->providesData.push_back(CARTSLAM_KEY_IMAGE_MODEL);
        this->providesData.push_back(CARTSLAM_KEY_IMAGE_MODEL_ALPHA);
        if (options.mesh) this->providesData.push_back(CARTSLAM_KEY_VOXEL_MESH_COLORS);
    }
}

VoxelMapModule::~VoxelMapModule() {
    cart_model_track_destroy(tracker);
    cart_voxel_color_destroy(color);
    cart_voxel_map_destroy(map);
    cart_plane_store_destroy(store);
}

system_data_t VoxelMapModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(options.disparityKey);
    if (!disparity || disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    const int rows = disparity->rows, cols = disparity->cols;
    std::shared_ptr<image_t> mask;
    if (options.useMotion) {
        mask = data.getData<image_t>(CARTSLAM_KEY_MOTION);
        requireImage(mask, CV_8UC1, rows, cols, "VoxelMapModule: motion must be a CV_8UC1 image of the disparity's size");
    }
    double pose[12];   // a frame whose pose status is 0 carries the kept pose
    auto ego = data.getData<EgoMotion>(options.poseKey);
    std::memcpy(pose, ego->pose, sizeof(pose));
    auto result = std::make_shared<VoxelMap>();
    auto rays = std::make_shared<VoxelRayCounts>();
    auto model = options.raycast ? std::make_shared<image_t>(rows, cols, CV_16SC1) : std::make_shared<image_t>();
    auto status = options.raycast ? std::make_shared<image_t>(rows, cols, CV_8UC1) : std::make_shared<image_t>();
    std::lock_guard<std::mutex> lock(mutex);
    if (!map) {   // the map keeps the device of the engine it is made on, not the engine
        const cart_voxel_map_params p = paramsOf(options);
        makeOnPostEngine(cols, rows, [&](cart_engine *e) {
            return cart_voxel_map_create(e, options.cellsX, options.cellsY, options.cellsZ, &p, &map) ? "cart_voxel_map_create" : nullptr;
        });
        if (options.track)
            makeOnPostEngine(cols, rows, [&](cart_engine *e) { return cart_model_track_create(e, cols, rows, &tracker) ? "cart_model_track_create" : nullptr; });
        if (options.rebuild) {
            makeOnPostEngine(cols, rows, [&](cart_engine *e) { return cart_plane_store_create(e, cols, rows, options.storeCapacity, &store) ? "cart_plane_store_create" : nullptr; });
            if (!options.useMotion) {   // the store keeps a u8 plane beside every disparity: zeros, which mask nothing
                zeroPlane.create(rows, cols, CV_8UC1);
                zeroPlane.setTo(0);
                hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize after zeroing the store's plane");
            }
        }
        if (options.color)
            makeOnPostEngine(cols, rows, [&](cart_engine *e) { return cart_voxel_color_create(e, map, options.colorMaxWeight, &color) ? "cart_voxel_color_create" : nullptr; });
        scratch.create();
        scratch.reserve(kScratchBytes, kScratchBytes);
        if (options.mesh)   // the vertices, the quads and, with "color", one 4-byte colour per vertex
            meshBuffers.reserve((size_t)options.meshMaxVertices * (sizeof(cart_mesh_vertex) + (options.color ? sizeof(cart_voxel_rgb) : 0)) +
                                    (size_t)options.meshMaxQuads * sizeof(cart_mesh_quad), 0);
    }
    const cart_ego_camera cam = cameraOf(options);
    hipStream_t s = scratch.stream();
    int32_t *counts = reinterpret_cast<int32_t *>(scratch.dev<char>() + kCountsOffset);   // [0, 2): integrate; [2, 5): raycast
    std::shared_ptr<EgoMotion> modelPose;
    std::shared_ptr<cart_model_track_result> trackResult;
    std::shared_ptr<cart_model_track_color_result> trackColorResult;
    if (options.track) {
        // the prediction: the previous tracked pose chained with this frame's relative pose (kept where the frame has none); frame 1 takes the pose itself
        if (haveTracked) chainPose(tracked, ego->result, pose);
        const cart_model_track_params tp = trackParamsOf(options);
        bool take = false;
        if (options.trackColor) {   // S38: against both volumes as the earlier frames left them, with this frame's reference image
            const image_t image = getReferenceImage(data.dataElement);
            if ((image.type() != CV_8UC3 && image.type() != CV_8UC1) || image.rows != rows || image.cols != cols)
                throw std::runtime_error("VoxelMapModule: track_color needs a CV_8UC1 or CV_8UC3 reference image of the disparity's size");
            const cart_model_track_color_params cp = trackColorParamsOf(options);
            cart_model_track_color_result *record = reinterpret_cast<cart_model_track_color_result *>(scratch.dev<char>() + kTrackColorOffset);
            if (cart_model_track_refine_color(tracker, map, color, &cam, pose, &tp, &cp, disparity->ptr<int16_t>(), disparity->step, image.ptr<uint8_t>(), image.step,
                                              image.type() == CV_8UC3 ? 3 : 1, mask ? mask->ptr<uint8_t>() : nullptr, mask ? mask->step : 0, cols, rows, record, s) != 0)
                failAbi("cart_model_track_refine_color");
            hipCheck(hipMemcpyAsync(scratch.host<char>() + kTrackColorOffset, record, sizeof(*record), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the colour-aided tracking result");
            scratch.wait();   // the pose decides where the frame is integrated: the host must see the record first
            trackColorResult = std::make_shared<cart_model_track_color_result>();
            std::memcpy(trackColorResult.get(), scratch.host<char>() + kTrackColorOffset, sizeof(*trackColorResult));
            trackResult = std::make_shared<cart_model_track_result>();   // the first 136 bytes have its layout and meaning
            std::memcpy(trackResult.get(), trackColorResult.get(), sizeof(*trackResult));
            take = acceptModelTrackColor(*trackColorResult, options.minInliers);
        } else {
            if (cart_model_track_refine(tracker, map, &cam, pose, &tp, disparity->ptr<int16_t>(), disparity->step, mask ? mask->ptr<uint8_t>() : nullptr, mask ? mask->step : 0,
                                        cols, rows, scratch.dev<cart_model_track_result>(), s) != 0)
                failAbi("cart_model_track_refine");
            hipCheck(hipMemcpyAsync(scratch.host(), scratch.dev(), sizeof(cart_model_track_result), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the model tracking result");
            scratch.wait();   // the pose decides where the frame is integrated: the host must see the record first
            trackResult = std::make_shared<cart_model_track_result>();
            std::memcpy(trackResult.get(), scratch.host(), sizeof(*trackResult));
            take = acceptModelTrack(*trackResult, options.minInliers);
        }
        if (take)
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) pose[4 * r + c] = trackResult->R[3 * r + c];
                pose[4 * r + 3] = trackResult->t[r];
            }
        modelPose = std::make_shared<EgoMotion>();
        modelPose->result = ego->result;   // the counts of the estimate the prediction came from; R and t are replaced below
        if (haveTracked) {
            relativeOf(tracked, pose, modelPose->result.R, modelPose->result.t);
            modelPose->result.status = 1;
        } else {
            const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            std::memcpy(modelPose->result.R, I, sizeof(I));
            modelPose->result.t[0] = modelPose->result.t[1] = modelPose->result.t[2] = 0.0;
            modelPose->result.status = 0;
        }
        std::memcpy(modelPose->pose, pose, sizeof(pose));
        std::memcpy(tracked, pose, sizeof(pose));
        haveTracked = true;
    }
    const std::vector<double> *nodes = nullptr;   // S35: every node's estimate, on the frames whose graph was optimised
    if (options.rebuild) {
        const int32_t node = data.getData<PoseGraphRecord>(CARTSLAM_KEY_POSE_GRAPH_RESULT)->node;
        if (node >= 0) {   // a keyframe: its disparity goes into the store under the frame's id, with the motion labels or the zeroed plane
            const image_t &plane = mask ? *mask : zeroPlane;
            if (cart_plane_store_insert(store, data.id, disparity->ptr<int16_t>(), disparity->step, plane.ptr<uint8_t>(), plane.step, cols, rows, s) != 0)
                failAbi("cart_plane_store_insert");
            if (nodeFrame.size() <= (size_t)node) nodeFrame.resize((size_t)node + 1, 0);
            nodeFrame[node] = data.id;
        }
        const auto published = data.getData<std::vector<double>>(CARTSLAM_KEY_POSE_GRAPH_NODES);
        if (published && !published->empty()) nodes = published.get();
    }
    int64_t *rebuildCounts = reinterpret_cast<int64_t *>(scratch.dev<char>() + kRebuildCountsOffset);
    if (nodes) {   // this frame is the newest node and is in the store: it is integrated once, after every other keyframe, in node order
        const size_t count = std::min(nodes->size() / 12, nodeFrame.size());
        result->rebuildIds.assign(nodeFrame.begin(), nodeFrame.begin() + count);
        if (cart_voxel_map_rebuild(map, store, &cam, result->rebuildIds.data(), nodes->data(), (int)count, pose, options.useMotion ? 1 : 0, &result->rebuildUsed,
                                   rebuildCounts, s) != 0)
            failAbi("cart_voxel_map_rebuild");
        result->rebuilt = (int)count;
        hipCheck(hipMemcpyAsync(scratch.host<char>() + kRebuildCountsOffset, rebuildCounts, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s),
                 "hipMemcpyAsync of the voxel map rebuild counts");
    } else if (cart_voxel_map_integrate(map, &cam, pose, disparity->ptr<int16_t>(), disparity->step, cols, rows, mask ? mask->ptr<uint8_t>() : nullptr,
                                        mask ? mask->step : 0, counts, s) != 0) {
        failAbi("cart_voxel_map_integrate");
    }
    if (options.raycast &&
        cart_voxel_map_raycast(map, &cam, pose, cols, rows, model->ptr<int16_t>(), model->step, nullptr, 0, status->ptr<uint8_t>(), status->step, counts + 2, s) != 0)
        failAbi("cart_voxel_map_raycast");
    std::shared_ptr<VoxelColorFrame> colour;
    auto imageModel = std::make_shared<image_t>(), imageAlpha = std::make_shared<image_t>();
    if (options.color) {   // S37: the frame's image into the colour volume right after the geometry, then the model's colours behind the model disparity
        colour = std::make_shared<VoxelColorFrame>();
        int32_t *colorCounts = reinterpret_cast<int32_t *>(scratch.dev<char>() + kColorCountsOffset);
        if (!nodes) {   // a rebuild frame colour-integrates nothing and the stored colours stay: the store holds no images
            const image_t image = getReferenceImage(data.dataElement);
            if ((image.type() != CV_8UC3 && image.type() != CV_8UC1) || image.rows != rows || image.cols != cols)
                throw std::runtime_error("VoxelMapModule: color needs a CV_8UC1 or CV_8UC3 reference image of the disparity's size");
            if (cart_voxel_color_integrate(color, map, &cam, pose, disparity->ptr<int16_t>(), disparity->step, image.ptr<uint8_t>(), image.step,
                                           image.type() == CV_8UC3 ? 3 : 1, cols, rows, mask ? mask->ptr<uint8_t>() : nullptr, mask ? mask->step : 0, colorCounts, s) != 0)
                failAbi("cart_voxel_color_integrate");
            colour->integrated = true;
        }
        if (options.raycast) {
            imageModel = std::make_shared<image_t>(rows, cols, CV_8UC3);
            imageAlpha = std::make_shared<image_t>(rows, cols, CV_8UC1);
            if (cart_voxel_color_render(color, &cam, pose, model->ptr<int16_t>(), model->step, cols, rows, imageModel->ptr<uint8_t>(), imageModel->step,
                                        imageAlpha->ptr<uint8_t>(), imageAlpha->step, colorCounts + 2, s) != 0)
                failAbi("cart_voxel_color_render");
        }
        hipCheck(hipMemcpyAsync(scratch.host<char>() + kColorCountsOffset, colorCounts, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the colour counts");
    }
    int32_t *hostCounts = reinterpret_cast<int32_t *>(scratch.host<char>() + kCountsOffset);
    hipCheck(hipMemcpyAsync(hostCounts, counts, (options.raycast ? 5 : 2) * sizeof(int32_t), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the voxel map counts");
    std::shared_ptr<VoxelMesh> mesh;
    std::shared_ptr<VoxelMeshColors> meshColors;
    if (options.mesh) {
        mesh = std::make_shared<VoxelMesh>();
        if (options.color) meshColors = std::make_shared<VoxelMeshColors>();
        if (++meshFrames % options.meshInterval == 0) {   // S36: the surface of the window as this frame left it
            cart_mesh_vertex *vertices = meshBuffers.dev<cart_mesh_vertex>();
            cart_mesh_quad *quads = reinterpret_cast<cart_mesh_quad *>(meshBuffers.dev<char>() + (size_t)options.meshMaxVertices * sizeof(cart_mesh_vertex));
            int32_t *meshCounts = reinterpret_cast<int32_t *>(scratch.dev<char>() + kMeshCountsOffset);
            if (cart_voxel_map_mesh(map, options.meshMinWeight, vertices, options.meshMaxVertices, quads, options.meshMaxQuads, meshCounts, mesh->origin, s) != 0)
                failAbi("cart_voxel_map_mesh");
            cart_voxel_rgb *colors = reinterpret_cast<cart_voxel_rgb *>(reinterpret_cast<char *>(quads) + (size_t)options.meshMaxQuads * sizeof(cart_mesh_quad));
            if (options.color &&   // the written count is read on the device: no round trip between the two calls
                cart_voxel_color_vertices(color, vertices, meshCounts + 2, options.meshMaxVertices, mesh->origin, colors, s) != 0)
                failAbi("cart_voxel_color_vertices");
            hipCheck(hipMemcpyAsync(scratch.host<char>() + kMeshCountsOffset, meshCounts, sizeof(mesh->counts), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the mesh counts");
            scratch.wait();   // the second synchronisation of such a frame: the written counts size the download
            std::memcpy(mesh->counts, scratch.host<char>() + kMeshCountsOffset, sizeof(mesh->counts));
            mesh->vertices.resize((size_t)mesh->counts[2]);
            mesh->quads.resize((size_t)mesh->counts[3]);
            if (mesh->counts[2])
                hipCheck(hipMemcpyAsync(mesh->vertices.data(), vertices, mesh->vertices.size() * sizeof(cart_mesh_vertex), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the mesh vertices");
            if (mesh->counts[3])
                hipCheck(hipMemcpyAsync(mesh->quads.data(), quads, mesh->quads.size() * sizeof(cart_mesh_quad), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the mesh quads");
            if (options.color) {
                meshColors->colors.resize((size_t)mesh->counts[2]);
                if (mesh->counts[2])
                    hipCheck(hipMemcpyAsync(meshColors->colors.data(), colors, meshColors->colors.size() * sizeof(cart_voxel_rgb), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the mesh colours");
                meshColors->extracted = true;
            }
            mesh->voxelSize = options.voxelSize;
            mesh->extracted = true;
        }
    }
    int valid = 0;
    if (cart_voxel_map_window(map, result->origin, result->cells, &valid) != 0) failAbi("cart_voxel_map_window");
    result->voxelSize = options.voxelSize;
    if (snapshot) {   // synchronises
        result->voxels.resize((size_t)options.cellsX * options.cellsY * options.cellsZ);
        if (cart_voxel_map_read(map, result->voxels.data(), result->origin, s) != 0) failAbi("cart_voxel_map_read");
    }
    if (options.color && snapshot) {   // synchronises
        colour->voxels.resize((size_t)options.cellsX * options.cellsY * options.cellsZ);
        if (cart_voxel_color_read(color, colour->voxels.data(), colour->origin, s) != 0) failAbi("cart_voxel_color_read");
    }
    scratch.wait();   // the frame's only blocking synchronisation
    if (options.color) {
        const int32_t *cc = reinterpret_cast<const int32_t *>(scratch.host<char>() + kColorCountsOffset);
        if (colour->integrated) std::memcpy(colour->counts, cc, sizeof(colour->counts));
        if (options.raycast) colour->rendered = cc[2];
    }
    std::memcpy(result->counts, hostCounts, sizeof(result->counts));
    if (result->rebuilt > 0) {   // the integrate's two words were not written on this frame: the rebuild's counts, cut to int32
        std::memcpy(result->rebuildCounts, scratch.host<char>() + kRebuildCountsOffset, sizeof(result->rebuildCounts));
        for (int k = 0; k < 2; ++k) result->counts[k] = (int32_t)std::min<int64_t>(result->rebuildCounts[k], INT32_MAX);
    }
    if (options.raycast) std::memcpy(rays->rays, hostCounts + 2, sizeof(rays->rays));
    system_data_t out = MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_VOXEL_MAP, result), MODULE_PAIR(CARTSLAM_KEY_DISPARITY_MODEL, model),
                                          MODULE_PAIR(CARTSLAM_KEY_DISPARITY_MODEL_STATUS, status), MODULE_PAIR(CARTSLAM_KEY_DISPARITY_MODEL_COUNTS, rays));
    if (options.mesh) out.push_back(MODULE_PAIR(CARTSLAM_KEY_VOXEL_MESH, mesh));
    if (options.color) {
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_VOXEL_COLOR, colour));
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_IMAGE_MODEL, imageModel));
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_IMAGE_MODEL_ALPHA, imageAlpha));
        if (options.mesh) out.push_back(MODULE_PAIR(CARTSLAM_KEY_VOXEL_MESH_COLORS, meshColors));
    }
    if (options.track) {
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_MODEL_POSE, modelPose));
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_MODEL_TRACK_RESULT, trackResult));
        if (options.trackColor) out.push_back(MODULE_PAIR(CARTSLAM_KEY_MODEL_TRACK_COLOR_RESULT, trackColorResult));
    }
    return out;
}
}  // namespace cart

// voxelmap.cpp -- VoxelMapModule (cartslam_amd/modules/voxelmap.hpp): the rolling TSDF voxel map with model raycast, spec DESIGN.md S33.
#include "cartslam_amd/modules/voxelmap.hpp"

#include <cstdlib>
#include <cstring>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/motionseg.hpp"
#include "module_support.hpp"

namespace cart {
namespace {
cart_voxel_map_params paramsOf(const VoxelMapOptions &o) {
    return cart_voxel_map_params{o.voxelSize, o.minDisparity, o.minDepth, o.maxDepth, o.truncation, o.disparitySigma, o.lookahead, o.marchStep, o.maxWeight, o.minWeight};
}
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
    this->requiresData.push_back(module_dependency_t(options.disparityKey));
    this->requiresData.push_back(module_dependency_t(options.poseKey));
    if (options.useMotion) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_VOXEL_MAP, -1));   // one frame at a time, in order
    this->providesData.push_back(CARTSLAM_KEY_VOXEL_MAP);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_MODEL);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_MODEL_STATUS);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_MODEL_COUNTS);
}

VoxelMapModule::~VoxelMapModule() { cart_voxel_map_destroy(map); }

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
    std::memcpy(pose, data.getData<EgoMotion>(options.poseKey)->pose, sizeof(pose));
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
        scratch.create();
        scratch.reserve(5 * sizeof(int32_t), 5 * sizeof(int32_t));
    }
    const cart_ego_camera cam = cameraOf(options);
    hipStream_t s = scratch.stream();
    int32_t *counts = scratch.dev<int32_t>();   // [0, 2): integrate; [2, 5): raycast
    if (cart_voxel_map_integrate(map, &cam, pose, disparity->ptr<int16_t>(), disparity->step, cols, rows, mask ? mask->ptr<uint8_t>() : nullptr, mask ? mask->step : 0,
                                 counts, s) != 0)
        failAbi("cart_voxel_map_integrate");
    if (options.raycast &&
        cart_voxel_map_raycast(map, &cam, pose, cols, rows, model->ptr<int16_t>(), model->step, nullptr, 0, status->ptr<uint8_t>(), status->step, counts + 2, s) != 0)
        failAbi("cart_voxel_map_raycast");
    hipCheck(hipMemcpyAsync(scratch.host(), scratch.dev(), (options.raycast ? 5 : 2) * sizeof(int32_t), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the voxel map counts");
    int valid = 0;
    if (cart_voxel_map_window(map, result->origin, result->cells, &valid) != 0) failAbi("cart_voxel_map_window");
    result->voxelSize = options.voxelSize;
    if (snapshot) {   // synchronises
        result->voxels.resize((size_t)options.cellsX * options.cellsY * options.cellsZ);
        if (cart_voxel_map_read(map, result->voxels.data(), result->origin, s) != 0) failAbi("cart_voxel_map_read");
    }
    scratch.wait();   // the frame's only blocking synchronisation
    std::memcpy(result->counts, scratch.host<int32_t>(), sizeof(result->counts));
    if (options.raycast) std::memcpy(rays->rays, scratch.host<int32_t>() + 2, sizeof(rays->rays));
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_VOXEL_MAP, result), MODULE_PAIR(CARTSLAM_KEY_DISPARITY_MODEL, model),
                             MODULE_PAIR(CARTSLAM_KEY_DISPARITY_MODEL_STATUS, status), MODULE_PAIR(CARTSLAM_KEY_DISPARITY_MODEL_COUNTS, rays));
}
}  // namespace cart

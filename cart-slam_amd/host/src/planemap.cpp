// planemap.cpp -- PlaneMapModule (cartslam_amd/modules/planemap.hpp): the world-frame bird's-eye plane map, spec DESIGN.md S24.
#include "cartslam_amd/modules/planemap.hpp"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/planeseg.hpp"

namespace cart {
namespace {
[[noreturn]] void failAbi(const char *what) { throw std::runtime_error(std::string(what) + ": " + cart_last_error(nullptr)); }
void hipCheck(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

PlaneMapModule::PlaneMapModule(const PlaneMapOptions &options)
    : SyncWrapperSystemModule("PlaneMap"), options(options), snapshot(std::getenv("CARTSLAM_PLANE_MAP_SNAPSHOT") != nullptr) {
    const auto positive = [](double v) { return v > 0 && std::isfinite(v); };
    if (!positive(options.fx)) throw std::invalid_argument("fx must be a positive number (a source without calibration needs the camera keys)");
    if (!positive(options.fy)) throw std::invalid_argument("fy must be a positive number");
    if (!std::isfinite(options.cx)) throw std::invalid_argument("cx must be finite");
    if (!std::isfinite(options.cy)) throw std::invalid_argument("cy must be finite");
    if (!positive(options.baseline)) throw std::invalid_argument("baseline must be a positive number");
    // the library's own checks, without a device: everything valid gets as far as the missing engine
    const cart_plane_map_params p{options.cellSize, options.minDisparity, options.maxDepth, options.maxLateral, options.heightQuantum};
    cart_plane_map *none = nullptr;
    (void)cart_plane_map_create(nullptr, options.cellsX, options.cellsZ, &p, &none);
    if (std::strcmp(cart_last_error(nullptr), "bad arguments") != 0) throw std::invalid_argument(cart_last_error(nullptr));
    if (options.minVotes < 1) throw std::invalid_argument("min_votes must be at least 1");
    if (options.obstaclePercent < 1 || options.obstaclePercent > 100) throw std::invalid_argument("obstacle_percent must be in [1, 100]");
    if (!options.poseFile.empty()) {
        std::ifstream file(options.poseFile);
        if (!file.is_open()) throw std::invalid_argument("pose_file " + options.poseFile + " cannot be opened");
        for (std::string line; std::getline(file, line);) {
            std::array<double, 12> pose{};
            const char *s = line.c_str();
            int n = 0;
            for (; n < 12; ++n) {
                char *end = nullptr;
                pose[n] = std::strtod(s, &end);
                if (end == s) break;
                s = end;
            }
            poses.push_back(pose);
            poseGiven.push_back(n == 12);
        }
    }
    if (options.disparityKey.empty()) throw std::invalid_argument("disparity_key must name a blackboard image");
    this->requiresData.push_back(module_dependency_t(options.disparityKey));
    if (options.planesKey.empty()) throw std::invalid_argument("planes_key must name a blackboard image");
    this->requiresData.push_back(module_dependency_t(options.planesKey));
    if (options.poseKey.empty()) throw std::invalid_argument("pose_key must name a blackboard pose");
    if (options.poseFile.empty()) this->requiresData.push_back(module_dependency_t(options.poseKey));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_PLANE_MAP, -1));   // one frame at a time, in order
    this->providesData.push_back(CARTSLAM_KEY_PLANE_MAP);
}

PlaneMapModule::~PlaneMapModule() {
    cart_plane_map_destroy(map);
    if (stream) (void)hipStreamDestroy(static_cast<hipStream_t>(stream));
}

system_data_t PlaneMapModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(options.disparityKey);
    auto planes = data.getData<image_t>(options.planesKey);
    if (!disparity || disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    if (!planes || planes->empty() || planes->type() != CV_8UC1 || planes->rows != disparity->rows || planes->cols != disparity->cols)
        throw std::runtime_error("PlaneMapModule: " + options.planesKey + " must be a CV_8UC1 image of the disparity's size");
    double pose[12];
    if (options.poseFile.empty()) {   // a frame whose ego_motion.status is 0 carries the kept pose
        std::memcpy(pose, data.getData<EgoMotion>(options.poseKey)->pose, sizeof(pose));
    } else {
        const size_t line = (size_t)data.id - 1;
        if (data.id < 1 || line >= poses.size() || !poseGiven[line])
            throw std::runtime_error("PlaneMapModule: pose_file has no pose for frame " + std::to_string(data.id) + " (line " + std::to_string(data.id) + ")");
        std::memcpy(pose, poses[line].data(), sizeof(pose));
    }
    std::lock_guard<std::mutex> lock(mutex);
    if (!map) {   // the map keeps the device of the engine it is made on, not the engine
        cart_engine_params ep;
        cart_engine_default_params(&ep);
        ep.width = disparity->cols; ep.height = disparity->rows; ep.num_disparities = 0; ep.paths = 0; ep.max_inflight = 1;
        cart_engine *engine = nullptr;
        if (cart_engine_create(&ep, &engine) != 0) failAbi("cart_engine_create");
        const cart_plane_map_params p{options.cellSize, options.minDisparity, options.maxDepth, options.maxLateral, options.heightQuantum};
        const int rc = cart_plane_map_create(engine, options.cellsX, options.cellsZ, &p, &map);
        const std::string error = rc ? cart_last_error(nullptr) : "";
        cart_engine_destroy(engine);
        if (rc) throw std::runtime_error("cart_plane_map_create: " + error);
        hipStream_t s = nullptr;
        hipCheck(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreateWithFlags");
        stream = s;
    }
    const cart_ego_camera cam{options.fx, options.fy, options.cx, options.cy, options.baseline};
    auto result = std::make_shared<PlaneMap>();
    result->cellsX = options.cellsX; result->cellsZ = options.cellsZ; result->cellSize = options.cellSize;
    result->classes = image_t(options.cellsZ, options.cellsX, CV_8UC1);
    if (cart_plane_map_update(map, &cam, pose, disparity->ptr<int16_t>(), disparity->step, planes->ptr<uint8_t>(), planes->step, disparity->cols,
                              disparity->rows, stream) != 0)
        failAbi("cart_plane_map_update");
    if (cart_plane_map_classify(map, options.minVotes, options.obstaclePercent, result->classes.ptr<uint8_t>(), result->classes.step, stream) != 0)
        failAbi("cart_plane_map_classify");
    int valid = 0;
    if (cart_plane_map_window(map, &result->originX, &result->originZ, &valid) != 0) failAbi("cart_plane_map_window");
    if (snapshot) {   // synchronises
        result->cells.resize((size_t)options.cellsX * options.cellsZ);
        if (cart_plane_map_read(map, result->cells.data(), &result->originX, &result->originZ, stream) != 0) failAbi("cart_plane_map_read");
    }
    hipCheck(hipStreamSynchronize(static_cast<hipStream_t>(stream)), "hipStreamSynchronize");   // the frame's only blocking synchronisation
    return MODULE_RETURN(CARTSLAM_KEY_PLANE_MAP, result);
}
}  // namespace cart

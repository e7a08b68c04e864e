// planemap.cpp -- PlaneMapModule (cartslam_amd/modules/planemap.hpp): the world-frame bird's-eye plane map, spec DESIGN.md S24.
#include "cartslam_amd/modules/planemap.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/planeseg.hpp"
#include "cartslam_amd/modules/posegraph.hpp"
#include "module_support.hpp"

namespace cart {
PlaneMapModule::PlaneMapModule(const PlaneMapOptions &options)
    : SyncWrapperSystemModule("PlaneMap"), options(options), snapshot(std::getenv("CARTSLAM_PLANE_MAP_SNAPSHOT") != nullptr) {
    checkCamera(options);
    // the library's own checks, without a device: everything valid gets as far as the missing engine
    const cart_plane_map_params p{options.cellSize, options.minDisparity, options.maxDepth, options.maxLateral, options.heightQuantum};
    cart_plane_map *none = nullptr;
    (void)cart_plane_map_create(nullptr, options.cellsX, options.cellsZ, &p, &none);
    requireLibraryAccepts();
    if (options.minVotes < 1) throw std::invalid_argument("min_votes must be at least 1");
    if (options.obstaclePercent < 1 || options.obstaclePercent > 100) throw std::invalid_argument("obstacle_percent must be in [1, 100]");
    if (options.rebuild) {
        if (options.poseKey != CARTSLAM_KEY_POSE_GRAPH || !options.poseFile.empty())
            throw std::invalid_argument("rebuild requires \"pose_key\": \"pose_graph\" and no pose_file");
        cart_plane_store *none = nullptr;
        (void)cart_plane_store_create(nullptr, 1, 1, options.storeCapacity, &none);
        if (std::strcmp(cart_last_error(nullptr), "bad arguments") != 0) throw std::invalid_argument(std::string("store_capacity: ") + cart_last_error(nullptr));
    }
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
    if (options.rebuild) {
        this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_POSE_GRAPH_RESULT));
        this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_POSE_GRAPH_NODES));
    }
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_PLANE_MAP, -1));   // one frame at a time, in order
    this->providesData.push_back(CARTSLAM_KEY_PLANE_MAP);
}

PlaneMapModule::~PlaneMapModule() {
    cart_plane_map_destroy(map);
    cart_plane_store_destroy(store);
}

system_data_t PlaneMapModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(options.disparityKey);
    auto planes = data.getData<image_t>(options.planesKey);
    if (!disparity || disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    if (!isImage(planes, CV_8UC1, disparity->rows, disparity->cols))
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
        const cart_plane_map_params p{options.cellSize, options.minDisparity, options.maxDepth, options.maxLateral, options.heightQuantum};
        makeOnPostEngine(disparity->cols, disparity->rows, [&](cart_engine *e) {
            if (cart_plane_map_create(e, options.cellsX, options.cellsZ, &p, &map)) return "cart_plane_map_create";
            if (options.rebuild && cart_plane_store_create(e, disparity->cols, disparity->rows, options.storeCapacity, &store)) return "cart_plane_store_create";
            return static_cast<const char *>(nullptr);
        });
        scratch.create();
    }
    const cart_ego_camera cam = cameraOf(options);
    auto result = std::make_shared<PlaneMap>();
    result->cellsX = options.cellsX; result->cellsZ = options.cellsZ; result->cellSize = options.cellSize;
    result->classes = image_t(options.cellsZ, options.cellsX, CV_8UC1);
    const std::vector<double> *nodes = nullptr;   // S30: every node's estimate, on the frames whose graph was optimised
    if (options.rebuild) {
        const int32_t node = data.getData<PoseGraphRecord>(CARTSLAM_KEY_POSE_GRAPH_RESULT)->node;
        if (node >= 0) {   // a keyframe: its images go into the store under the frame's id
            if (cart_plane_store_insert(store, data.id, disparity->ptr<int16_t>(), disparity->step, planes->ptr<uint8_t>(), planes->step, disparity->cols,
                                        disparity->rows, scratch.stream()) != 0)
                failAbi("cart_plane_store_insert");
            if (nodeFrame.size() <= (size_t)node) nodeFrame.resize((size_t)node + 1, 0);
            nodeFrame[node] = data.id;
        }
        const auto published = data.getData<std::vector<double>>(CARTSLAM_KEY_POSE_GRAPH_NODES);
        if (published && !published->empty()) nodes = published.get();
    }
    if (nodes) {   // this frame is the newest node and is in the store: it votes once, with every other keyframe
        const size_t count = std::min(nodes->size() / 12, nodeFrame.size());
        result->rebuildIds.assign(nodeFrame.begin(), nodeFrame.begin() + count);
        if (cart_plane_map_rebuild(map, store, &cam, result->rebuildIds.data(), nodes->data(), (int)count, pose, &result->rebuildUsed, scratch.stream()) != 0)
            failAbi("cart_plane_map_rebuild");
        result->rebuilt = (int)count;
    } else if (cart_plane_map_update(map, &cam, pose, disparity->ptr<int16_t>(), disparity->step, planes->ptr<uint8_t>(), planes->step, disparity->cols,
                                     disparity->rows, scratch.stream()) != 0) {
        failAbi("cart_plane_map_update");
    }
    if (cart_plane_map_classify(map, options.minVotes, options.obstaclePercent, result->classes.ptr<uint8_t>(), result->classes.step, scratch.stream()) != 0)
        failAbi("cart_plane_map_classify");
    int valid = 0;
    if (cart_plane_map_window(map, &result->originX, &result->originZ, &valid) != 0) failAbi("cart_plane_map_window");
    if (snapshot) {   // synchronises
        result->cells.resize((size_t)options.cellsX * options.cellsZ);
        if (cart_plane_map_read(map, result->cells.data(), &result->originX, &result->originZ, scratch.stream()) != 0) failAbi("cart_plane_map_read");
    }
    scratch.wait();   // the frame's only blocking synchronisation
    return MODULE_RETURN(CARTSLAM_KEY_PLANE_MAP, result);
}
}  // namespace cart

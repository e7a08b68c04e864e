// posegraph.cpp -- PoseGraphModule (cartslam_amd/modules/posegraph.hpp): pose-graph optimisation over keyframes, spec DESIGN.md S29.
#include "cartslam_amd/modules/posegraph.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "cartslam_amd/modules/denseego.hpp"
#include "cartslam_amd/modules/loopclosure.hpp"
#include "module_support.hpp"

namespace cart {
namespace {
constexpr size_t kPosesAt = sizeof(cart_pose_graph_result);   // the module's buffers: the result record, then 12 doubles per node

// (R | t) 3 x 4 in row order: inv = (R^T, -(R^T t)), and the product, every sum left to right
void invertPose(const double p[12], double out[12]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[4 * r + c] = p[4 * c + r];
    for (int r = 0; r < 3; ++r) out[4 * r + 3] = -((out[4 * r] * p[3] + out[4 * r + 1] * p[7]) + out[4 * r + 2] * p[11]);
}
void multiplyPose(const double a[12], const double b[12], double out[12]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = (a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c]) + a[4 * r + 2] * b[8 + c];
        out[4 * r + 3] = ((a[4 * r] * b[3] + a[4 * r + 1] * b[7]) + a[4 * r + 2] * b[11]) + a[4 * r + 3];
    }
}
}  // namespace

void carryPose(const double est[12], const double odomNode[12], const double odomNow[12], double out[12]) {
    double inverse[12], relative[12];
    invertPose(odomNode, inverse);
    multiplyPose(inverse, odomNow, relative);
    multiplyPose(est, relative, out);
}

PoseGraphModule::PoseGraphModule(const PoseGraphOptions &options) : SyncWrapperSystemModule("PoseGraph"), options(options) {
    // the library's own checks, without a device: everything valid gets as far as the missing engine / object
    cart_pose_graph *none = nullptr;
    (void)cart_pose_graph_create(nullptr, options.maxNodes, options.maxLoops, &none);
    requireLibraryAccepts();
    const cart_pose_graph_params p{options.iterations};
    (void)cart_pose_graph_optimize(nullptr, &p, nullptr, nullptr);
    requireLibraryAccepts("graph is NULL");
    if (!positiveNumber(options.weightRotation)) throw std::invalid_argument("weight_rotation must be a positive number");
    if (!positiveNumber(options.weightTranslation)) throw std::invalid_argument("weight_translation must be a positive number");
    if (!positiveNumber(options.loopWeight) || !positiveNumber(options.weightRotation * options.loopWeight) || !positiveNumber(options.weightTranslation * options.loopWeight))
        throw std::invalid_argument("loop_weight must be a positive number that keeps both loop weights finite and above zero");
    if (options.keyframeInterval < 1) throw std::invalid_argument("keyframe_interval must be at least 1");
    if (options.loopClosureInterval > 0 && options.loopClosureInterval != options.keyframeInterval)
        throw std::invalid_argument("keyframe_interval must equal loop_closure's (" + std::to_string(options.loopClosureInterval) + ")");
    if (options.poseKey != CARTSLAM_KEY_EGO_MOTION && options.poseKey != CARTSLAM_KEY_DENSE_EGO)
        throw std::invalid_argument("pose_key must be \"ego_motion\" or \"dense_ego\"");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_LOOP_CLOSURE));
    this->requiresData.push_back(module_dependency_t(options.poseKey));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_POSE_GRAPH, -1));   // frames pass in order: the graph grows in frame order
    this->providesData.push_back(CARTSLAM_KEY_POSE_GRAPH);
    this->providesData.push_back(CARTSLAM_KEY_POSE_GRAPH_RESULT);
    this->providesData.push_back(CARTSLAM_KEY_POSE_GRAPH_NODES);
}

PoseGraphModule::~PoseGraphModule() { cart_pose_graph_destroy(graph); }

system_data_t PoseGraphModule::runInternal(System &, SystemRunData &data) {
    auto source = data.getData<EgoMotion>(options.poseKey);
    auto loop = data.getData<LoopClosure>(CARTSLAM_KEY_LOOP_CLOSURE);
    auto record = std::make_shared<PoseGraphRecord>();
    std::memset(record.get(), 0, sizeof(*record));
    record->node = -1;
    auto nodes = std::make_shared<std::vector<double>>();
    auto result = std::make_shared<EgoMotion>();
    result->result = source->result;
    result->landmarks = source->landmarks;
    std::lock_guard<std::mutex> lock(mutex);
    if (data.id % (uint32_t)options.keyframeInterval == 0) {
        if (!graph) {   // the graph keeps the device of the engine it is made on, not the engine
            makeOnPostEngine(64, 32, [&](cart_engine *e) {
                return cart_pose_graph_create(e, options.maxNodes, options.maxLoops, &graph) ? "cart_pose_graph_create" : nullptr;
            });
            scratch.create();
            const size_t bytes = kPosesAt + (size_t)options.maxNodes * 12 * sizeof(double);
            scratch.reserve(bytes, bytes);
        }
        if ((int)nodeFrames.size() >= options.maxNodes) {
            full = 1;
        } else {
            hipStream_t s = scratch.stream();
            int32_t node = -1;
            if (cart_pose_graph_add_node(graph, source->pose, options.weightRotation, options.weightTranslation, &node, s) != 0) failAbi("cart_pose_graph_add_node");
            nodeFrames.push_back(data.id);
            record->node = node;
            bool optimised = false;
            if (loop->detected) {
                const auto at = std::find(nodeFrames.begin(), nodeFrames.end() - 1, loop->keyframeId);
                int loops = 0;
                if (cart_pose_graph_size(graph, nullptr, &loops) != 0) failAbi("cart_pose_graph_size");
                if (at != nodeFrames.end() - 1 && loops < options.maxLoops) {
                    if (cart_pose_graph_add_loop(graph, (int)(at - nodeFrames.begin()), node, loop->relative.R, loop->relative.t, options.weightRotation * options.loopWeight,
                                                 options.weightTranslation * options.loopWeight, s) != 0)
                        failAbi("cart_pose_graph_add_loop");
                    const cart_pose_graph_params p{options.iterations};
                    if (cart_pose_graph_optimize(graph, &p, scratch.dev<cart_pose_graph_result>(), s) != 0) failAbi("cart_pose_graph_optimize");
                    optimised = true;
                    record->loopAdded = 1;
                } else {
                    loopsSkipped += 1;
                }
            }
            // this node's estimate, or after an optimise the result and every node's, through the pinned buffer: the frame's only synchronisation
            const int first = optimised ? 0 : node, count = optimised ? node + 1 : 1;
            uint8_t *d = scratch.dev<uint8_t>(), *h = scratch.host<uint8_t>();
            if (cart_pose_graph_poses(graph, first, count, reinterpret_cast<double *>(d + kPosesAt), s) != 0) failAbi("cart_pose_graph_poses");
            const size_t from = optimised ? 0 : kPosesAt, bytes = kPosesAt + (size_t)count * 12 * sizeof(double) - from;
            hipCheck(hipMemcpyAsync(h + from, d + from, bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the pose graph's estimates");
            scratch.wait();
            const double *estimates = reinterpret_cast<const double *>(h + kPosesAt);
            if (optimised) {
                std::memcpy(&last, h, sizeof(last));
                nodes->assign(estimates, estimates + (size_t)count * 12);
            }
            std::memcpy(estNode, estimates + (size_t)(count - 1) * 12, sizeof(estNode));
            std::memcpy(odomNode, source->pose, sizeof(odomNode));
            haveNode = true;
        }
    }
    record->result = last;
    record->loopsSkipped = loopsSkipped;
    record->full = full;
    if (haveNode) carryPose(estNode, odomNode, source->pose, result->pose);
    else std::memcpy(result->pose, source->pose, sizeof(result->pose));
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_POSE_GRAPH, result), MODULE_PAIR(CARTSLAM_KEY_POSE_GRAPH_RESULT, record), MODULE_PAIR(CARTSLAM_KEY_POSE_GRAPH_NODES, nodes));
}
}  // namespace cart

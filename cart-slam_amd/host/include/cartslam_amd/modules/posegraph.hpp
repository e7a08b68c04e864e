// modules/posegraph.hpp -- an extension module (the reference optimises no trajectory): every keyframe becomes a node of a pose graph
// on the device, a loop that the "loop_closure" module verified becomes a loop edge and the graph is optimised at once, through
// cart_pose_graph_* (include/cart_engine.h, spec DESIGN.md S29).  Every frame publishes the corrected trajectory as an EgoMotion under
// "pose_graph", so "pose_key": "pose_graph" hands it to plane_map and temporal_fusion.  Factory type "pose_graph".
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../cartslam.hpp"
#include "cart_engine.h"
#include "egomotion.hpp"

#define CARTSLAM_KEY_POSE_GRAPH "pose_graph"
#define CARTSLAM_KEY_POSE_GRAPH_RESULT "pose_graph_result"
#define CARTSLAM_KEY_POSE_GRAPH_NODES "pose_graph_nodes"   // std::vector<double>, 12 per node: on the frames that optimised, else empty

namespace cart {
struct PoseGraphRecord {
    cart_pose_graph_result result;   // of the last optimise so far (all zeros before the first)
    int32_t node;                    // the node this frame became, -1 on a frame that is no keyframe or found the table full
    int32_t loopAdded;               // 1 = this frame added a loop edge and optimised
    int32_t loopsSkipped;            // so far: loops whose keyframe is no node, or that found the loop table full
    int32_t full;                    // 1 = the node table is full: nothing more is added, the last node's correction is carried on
};
static_assert(sizeof(PoseGraphRecord) == 48, "PoseGraphRecord layout (tests/np_posegraph.py MODULE_DTYPE)");

// All defaults are build-owned choices that no data set has tuned.
struct PoseGraphOptions {
    int keyframeInterval = 5;                 // must equal loop_closure's: its keyframes are the nodes
    int loopClosureInterval = 0;              // the factory fills it from the loop_closure module before it (0 = unknown, not compared)
    int maxNodes = 1024, maxLoops = 64, iterations = 4;
    double weightRotation = 10000.0, weightTranslation = 100.0;   // of every odometry edge
    double loopWeight = 1.0;                  // multiplies both weights for a loop edge
    std::string poseKey = CARTSLAM_KEY_EGO_MOTION;   // the blackboard EgoMotion whose chained pose is the odometry; "dense_ego" = the refined one
};

// est (odom_k^-1 odom_t) with inv = (R^T, -(R^T t)), in plain double loops (restated in tests/np_posegraph.py, carry)
void carryPose(const double est[12], const double odomNode[12], const double odomNow[12], double out[12]);

class PoseGraphModule : public SyncWrapperSystemModule {
   public:
    explicit PoseGraphModule(const PoseGraphOptions &options);   // throws std::invalid_argument naming the key that is out of range
    ~PoseGraphModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const PoseGraphOptions options;
    std::mutex mutex;                    // one frame at a time: the graph is the module's state
    cart_pose_graph *graph = nullptr;
    DeviceScratch scratch;               // the one stream; the result record, then every node's estimate: on the device and the pinned buffer they come through
    std::vector<uint64_t> nodeFrames;    // frame id of every node
    bool haveNode = false;
    double odomNode[12] = {}, estNode[12] = {};   // the last node: the pose it was handed in with and its estimate
    cart_pose_graph_result last{};       // of the last optimise
    int32_t loopsSkipped = 0, full = 0;
};
}  // namespace cart

// engine_posegraph.hip -- C ABI of the pose-graph optimisation (include/cart_engine.h): argument checks and the
// cart_pose_graph device object, which owns the nodes, the edges, the factor and the solver's workspaces.  The node and loop counts
// are host state: every launch gets them as arguments.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

struct cart_pose_graph : DeviceObject {
    using DeviceObject::DeviceObject;
    PoseGraphStore store{};
    int nodes = 0, loops = 0;   // guarded by mu
};

void cart_pose_graph_default_params(cart_pose_graph_params *p) {
    if (!p) return;
    *p = cart_pose_graph_params{4};
}

int cart_pose_graph_create(cart_engine *e, int max_nodes, int max_loops, cart_pose_graph **out) {
    if (max_nodes < 1 || max_nodes > CART_POSE_GRAPH_MAX_NODES) return fail("max_nodes must be in [1, 4096]");
    if (max_loops < 0 || max_loops > CART_POSE_GRAPH_MAX_LOOPS) return fail("max_loops must be in [0, 64]");
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_pose_graph *pg = new (std::nothrow) cart_pose_graph(e);
    if (!pg) return fail("out of host memory");
    PoseGraphStore &s = pg->store;
    s.max_nodes = max_nodes; s.max_loops = max_loops;
    const size_t n = (size_t)max_nodes, m = 6 * (size_t)max_loops, d = sizeof(double);
    if (pg->alloc(&s.odom, n * 12 * d) || pg->alloc(&s.est, n * 12 * d) || pg->alloc(&s.snap, n * 12 * d) ||
        pg->alloc(&s.edges, (n + max_loops) * sizeof(PgEdge)) || pg->alloc(&s.lin, (n + 1) * kPgLinDoubles * d) ||
        pg->alloc(&s.lin_loop, (size_t)max_loops * kPgLoopDoubles * d) || pg->alloc(&s.fac, (n + 1) * kPgFacDoubles * d) ||
        pg->alloc(&s.cols, n * 6 * (1 + m) * d) || pg->alloc(&s.lc, m * (m + 1) * d) || pg->alloc(&s.lr, m * m * d) || pg->alloc(&s.cd, m * d) ||
        pg->alloc(&s.ld, m * d) || pg->create_event()) {
        destroy_object(pg);
        return fail("allocating the pose graph failed");
    }
    *out = pg;
    return 0;
}

void cart_pose_graph_destroy(cart_pose_graph *pg) { destroy_object(pg); }

int cart_pose_graph_clear(cart_pose_graph *pg, void *stream_) {
    if (!pg) return fail("graph is NULL");
    ObjectCall call(*pg, static_cast<hipStream_t>(stream_));
    if (call.begin()) return -1;
    pg->nodes = pg->loops = 0;   // every later launch is ordered behind the earlier ones by the object's event
    return 0;
}

int cart_pose_graph_size(cart_pose_graph *pg, int *nodes, int *loops) {
    if (!pg) return fail("graph is NULL");
    std::lock_guard<std::mutex> lk(pg->mu);
    if (nodes) *nodes = pg->nodes;
    if (loops) *loops = pg->loops;
    return 0;
}

int cart_pose_graph_add_node(cart_pose_graph *pg, const double *pose, double w_rot, double w_trans, int32_t *node_out, void *stream_) {
    if (check_pose("pose", pose) || check_positive("w_rot", w_rot) || check_positive("w_trans", w_trans)) return -1;
    if (!pg) return fail("graph is NULL");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*pg, stream);
    if (call.begin()) return -1;
    if (pg->nodes >= pg->store.max_nodes) return fail("the node table is full (max_nodes = " + std::to_string(pg->store.max_nodes) + ")");
    PoseGraphNodeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g = pg->store;
    std::memcpy(a.pose, pose, sizeof(a.pose));
    a.w_rot = w_rot; a.w_trans = w_trans; a.n = pg->nodes;
    launch_pose_graph_add_node(a, stream);
    HIP_TRY(hipGetLastError());
    if (node_out) *node_out = pg->nodes;
    pg->nodes += 1;
    return 0;
}

int cart_pose_graph_add_loop(cart_pose_graph *pg, int a_, int b_, const double *R, const double *t, double w_rot, double w_trans, void *stream_) {
    if (!R) return fail("R is NULL");
    if (!t) return fail("t is NULL");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(R[k])) return fail("R[" + std::to_string(k) + "] must be finite");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(t[k])) return fail("t[" + std::to_string(k) + "] must be finite");
    if (check_positive("w_rot", w_rot) || check_positive("w_trans", w_trans)) return -1;
    if (a_ == b_) return fail("a and b must be different nodes");
    if (!pg) return fail("graph is NULL");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*pg, stream);
    if (call.begin()) return -1;
    if (a_ < 0 || a_ >= pg->nodes) return fail("a must be a node in [0, " + std::to_string(pg->nodes - 1) + "]");
    if (b_ < 0 || b_ >= pg->nodes) return fail("b must be a node in [0, " + std::to_string(pg->nodes - 1) + "]");
    if (pg->loops >= pg->store.max_loops) return fail("the loop table is full (max_loops = " + std::to_string(pg->store.max_loops) + ")");
    PoseGraphLoopArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g = pg->store;
    std::memcpy(a.edge.R, R, sizeof(a.edge.R));
    std::memcpy(a.edge.t, t, sizeof(a.edge.t));
    a.edge.w_rot = w_rot; a.edge.w_trans = w_trans; a.edge.a = a_; a.edge.b = b_;
    a.e = pg->loops;
    launch_pose_graph_add_loop(a, stream);
    HIP_TRY(hipGetLastError());
    pg->loops += 1;
    return 0;
}

int cart_pose_graph_optimize(cart_pose_graph *pg, const cart_pose_graph_params *params, cart_pose_graph_result *result, void *stream_) {
    if (!params) return fail("params is NULL");
    if (params->iterations < 0 || params->iterations > CART_POSE_GRAPH_MAX_ITERATIONS) return fail("iterations must be in [0, 16]");
    if (!pg) return fail("graph is NULL");
    if (reinterpret_cast<uintptr_t>(result) & 7) return fail("result must be 8-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*pg, stream);
    if (call.begin()) return -1;
    PoseGraphArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g = pg->store;
    a.n_nodes = pg->nodes; a.n_loops = pg->loops; a.iterations = params->iterations;
    a.result = result;
    launch_pose_graph_optimize(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// first + count against the node count, under the object's lock
static int check_range(const cart_pose_graph *pg, int first, int count) {
    if ((int64_t)first + count > pg->nodes) return fail("first + count exceeds the " + std::to_string(pg->nodes) + " nodes");
    return 0;
}

int cart_pose_graph_poses(cart_pose_graph *pg, int first, int count, double *out, void *stream_) {
    if (first < 0) return fail("first must not be negative");
    if (count < 0) return fail("count must not be negative");
    if (!pg) return fail("graph is NULL");
    if (!out) return fail("out is NULL");
    if (reinterpret_cast<uintptr_t>(out) & 7) return fail("out must be 8-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*pg, stream);
    if (call.begin()) return -1;
    if (check_range(pg, first, count)) return -1;
    const size_t bytes = (size_t)count * 12 * sizeof(double);
    if (bytes) HIP_TRY(hipMemcpyAsync(out, pg->store.est + 12 * (size_t)first, bytes, hipMemcpyDeviceToDevice, stream));
    return 0;
}

int cart_pose_graph_read(cart_pose_graph *pg, int first, int count, double *out_host) {
    if (first < 0) return fail("first must not be negative");
    if (count < 0) return fail("count must not be negative");
    if (!pg) return fail("graph is NULL");
    if (!out_host) return fail("out_host is NULL");
    hipStream_t stream = nullptr;
    ObjectCall call(*pg, stream);
    if (call.begin()) return -1;
    if (check_range(pg, first, count)) return -1;
    const size_t bytes = (size_t)count * 12 * sizeof(double);
    if (bytes) HIP_TRY(hipMemcpyAsync(out_host, pg->store.est + 12 * (size_t)first, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"

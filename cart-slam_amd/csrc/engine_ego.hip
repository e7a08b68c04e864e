// engine_ego.hip -- C ABI of the stereo visual odometry stage (include/cart_engine.h): argument checks and the
// cart_ego device object.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

struct cart_ego : DeviceObject {
    using DeviceObject::DeviceObject;
    int max_features = 0;
    int last_hypotheses = 0;           // params.hypotheses of the last estimate call (guarded by mu)
    double *corr = nullptr;            // [kEgoCorrRows][max_features]
    int32_t *corr_k = nullptr;         // [max_features]
    int32_t *n = nullptr;
    EgoHyp *hyp = nullptr;             // [CART_EGO_MAX_HYPOTHESES]
    cart_ego_hypothesis *table = nullptr;
};

void cart_ego_default_params(cart_ego_params *p) {
    if (!p) return;
    *p = cart_ego_params{1.0, 2.0, 256, 4};
}

int cart_ego_create(cart_engine *e, int max_features, cart_ego **out) {
    if (!e || !out) return fail("bad arguments");
    if (max_features < 1 || max_features > CART_ORB_MAX_FEATURES) return fail("max_features must be in [1, 65536]");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_ego *g = new (std::nothrow) cart_ego(e);
    if (!g) return fail("out of host memory");
    g->max_features = max_features;
    if (g->alloc(&g->corr, (size_t)kEgoCorrRows * max_features * sizeof(double)) || g->alloc(&g->corr_k, (size_t)max_features * sizeof(int32_t)) ||
        g->alloc(&g->n, sizeof(int32_t)) || g->alloc(&g->hyp, (size_t)CART_EGO_MAX_HYPOTHESES * sizeof(EgoHyp)) ||
        g->alloc(&g->table, (size_t)CART_EGO_MAX_HYPOTHESES * sizeof(cart_ego_hypothesis)) || g->create_event()) {
        destroy_object(g);
        return fail("allocating the ego-motion workspaces failed");
    }
    *out = g;
    return 0;
}

void cart_ego_destroy(cart_ego *g) { destroy_object(g); }

static int check_camera_and_params(const cart_ego_camera *cam, const cart_ego_params *p) {
    if (!cam) return fail("camera is NULL");
    if (!p) return fail("params is NULL");
    if (check_camera(cam) || check_positive("min_disparity", p->min_disparity) || check_positive("inlier_threshold", p->inlier_threshold)) return -1;
    if (p->hypotheses < 1 || p->hypotheses > CART_EGO_MAX_HYPOTHESES) return fail("hypotheses must be in [1, 1024]");
    if (p->refine_iterations < 0 || p->refine_iterations > CART_EGO_MAX_REFINE) return fail("refine_iterations must be in [0, 16]");
    return 0;
}

static bool misaligned(std::initializer_list<const void *> ptrs, uintptr_t mask) {
    uintptr_t all = 0;
    for (const void *p : ptrs) all |= reinterpret_cast<uintptr_t>(p);
    return (all & mask) != 0;
}

int cart_ego_triangulate(cart_ego *g, const cart_ego_camera *cam, const cart_ego_params *params, const cart_keypoint *kpL, const cart_keypoint *kpR,
                         const int32_t *left_count, const cart_match *stereo_matches, const int32_t *stereo_count, double *landmarks, void *stream_) {
    if (!g) return fail("ego is NULL");
    if (check_camera_and_params(cam, params)) return -1;
    if (!kpL || !kpR || !left_count || !stereo_matches || !stereo_count || !landmarks) return fail("NULL pointer");
    if (misaligned({kpL, kpR, left_count, stereo_matches, stereo_count}, 3)) return fail("keypoints, matches and counts must be 4-byte aligned");
    if (misaligned({landmarks}, 7)) return fail("landmarks must be 8-byte aligned");
    EgoArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam = *cam; a.p = *params; a.cap = g->max_features;
    a.kpL = kpL; a.kpR = kpR; a.left_count = left_count; a.stereo = stereo_matches; a.stereo_count = stereo_count; a.landmarks = landmarks;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*g, stream);
    if (call.begin()) return -1;
    launch_ego_triangulate(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_ego_estimate(cart_ego *g, const cart_ego_camera *cam, const cart_ego_params *params, const double *cur_landmarks, const cart_keypoint *cur_kpL,
                      const double *prev_landmarks, const cart_match *temporal_matches, const int32_t *temporal_count, uint64_t seed, uint64_t frame_id,
                      cart_ego_result *result, int32_t *inlier_mask, void *stream_) {
    if (!g) return fail("ego is NULL");
    if (check_camera_and_params(cam, params)) return -1;
    if (!cur_landmarks || !cur_kpL || !prev_landmarks || !temporal_matches || !temporal_count || !result) return fail("NULL pointer");
    if (misaligned({cur_kpL, temporal_matches, temporal_count, inlier_mask}, 3)) return fail("keypoints, matches, the count and the mask must be 4-byte aligned");
    if (misaligned({cur_landmarks, prev_landmarks, result}, 7)) return fail("landmarks and the result must be 8-byte aligned");
    EgoArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam = *cam; a.p = *params; a.cap = g->max_features;
    a.cur = cur_landmarks; a.cur_kp = cur_kpL; a.prev = prev_landmarks; a.temporal = temporal_matches; a.temporal_count = temporal_count;
    a.seed = seed; a.frame = frame_id;
    a.corr = g->corr; a.corr_k = g->corr_k; a.n = g->n; a.hyp = g->hyp; a.table = g->table;
    a.result = result; a.mask = inlier_mask;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*g, stream);
    if (call.begin()) return -1;
    g->last_hypotheses = params->hypotheses;
    launch_ego_estimate(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_ego_debug_hypotheses(cart_ego *g, cart_ego_hypothesis *host_dst, int capacity, int *n_hypotheses, void *stream_) {
    if (!g) return fail("ego is NULL");
    if (!host_dst || !n_hypotheses) return fail("NULL pointer");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*g, stream);
    if (call.begin()) return -1;
    if (g->last_hypotheses < 1) return fail("no cart_ego_estimate call yet");
    if (capacity < g->last_hypotheses) return fail("capacity is below the last call's hypotheses");
    HIP_TRY(hipMemcpyAsync(host_dst, g->table, (size_t)g->last_hypotheses * sizeof(cart_ego_hypothesis), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *n_hypotheses = g->last_hypotheses;
    return 0;
}

}  // extern "C"

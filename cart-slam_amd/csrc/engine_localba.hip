// engine_localba.hip -- C ABI of the windowed bundle adjustment (include/cart_engine.h): argument checks and the
// cart_local_ba device object, which owns the frame ring, the point and observation tables and the optimiser's workspaces.  The number of
// pushed frames is host state: every launch gets the ring positions as arguments.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

struct cart_local_ba : DeviceObject {
    using DeviceObject::DeviceObject;
    LbaStore store{};
    long long pushed = 0;   // frames pushed since the last clear (guarded by mu)
    std::vector<std::pair<void *, size_t>> zeroed;   // what a clear sets to zero

    int frames() const { return (int)std::min<long long>(pushed, store.window); }
    int first_slot() const { return (int)((pushed - frames()) % store.window); }
    int clear(hipStream_t stream) {
        for (const auto &z : zeroed) HIP_TRY(hipMemsetAsync(z.first, 0, z.second, stream));
        for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(store.track[k], 0xff, (size_t)store.max_features * sizeof(int32_t), stream));
        pushed = 0;
        return 0;
    }
};

void cart_local_ba_default_params(cart_local_ba_params *p) {
    if (!p) return;
    *p = cart_local_ba_params{1.0, 2.0, 0.0, 4, 2, 6};
}

static_assert(sizeof(cart_local_ba_result) == 40 && alignof(cart_local_ba_result) == 8, "cart_local_ba_result layout (DESIGN.md S32)");
static_assert(sizeof(cart_local_ba_params) == 40, "cart_local_ba_params layout (DESIGN.md S32)");

int cart_local_ba_create(cart_engine *e, int max_features, int window, int max_points, cart_local_ba **out) {
    if (max_features < 1 || max_features > CART_ORB_MAX_FEATURES) return fail("max_features must be in [1, 65536]");
    if (window < 2 || window > CART_LOCAL_BA_MAX_WINDOW) return fail("window must be in [2, 16]");
    if (max_points < 64 || max_points > CART_LOCAL_BA_MAX_POINTS) return fail("max_points must be in [64, 65536]");
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_local_ba *ba = new (std::nothrow) cart_local_ba(e);
    if (!ba) return fail("out of host memory");
    LbaStore &s = ba->store;
    s.max_features = max_features; s.window = window; s.max_points = max_points;
    const size_t f = (size_t)max_features, w = (size_t)window, m = (size_t)max_points, d = sizeof(double), i4 = sizeof(int32_t);
    const size_t order = 6 * (w - 1);
    if (ba->alloc(&s.odom, w * 12 * d) || ba->alloc(&s.est, w * 12 * d) || ba->alloc(&s.lin_est, w * 12 * d) || ba->alloc(&s.snap_est, w * 12 * d) ||
        ba->alloc(&s.frame_id, w * sizeof(uint64_t)) || ba->alloc(&s.X, m * 3 * d) || ba->alloc(&s.snap_X, m * 3 * d) ||
        ba->alloc(&s.n_obs, m * i4) || ba->alloc(&s.state, m * i4) || ba->alloc(&s.obs, m * w * sizeof(LbaObs)) ||
        ba->alloc(&s.sobs, f * sizeof(LbaObs)) || ba->alloc(&s.tmatch, f * i4) || ba->alloc(&s.claim, m * i4) || ba->alloc(&s.free_list, m * i4) ||
        ba->alloc(&s.track[0], f * i4) || ba->alloc(&s.track[1], f * i4) || ba->alloc(&s.counts, 9 * i4) ||
        ba->alloc(&s.blocks, (size_t)kLbaPointRows * m * d) || ba->alloc(&s.used, m * i4) || ba->alloc(&s.ctl, sizeof(LbaControl)) ||
        ba->alloc(&s.S, (order + 1) * order * d) || ba->alloc(&s.delta, order * d) || ba->create_event()) {
        destroy_object(ba);
        return fail("allocating the local bundle adjustment failed");
    }
    ba->zeroed = {{s.odom, w * 12 * d}, {s.est, w * 12 * d}, {s.frame_id, w * sizeof(uint64_t)}, {s.X, m * 3 * d}, {s.n_obs, m * i4}, {s.state, m * i4},
                  {s.obs, m * w * sizeof(LbaObs)}, {s.counts, 9 * i4}, {s.ctl, sizeof(LbaControl)}};
    if (ba->clear(nullptr) || hipDeviceSynchronize() != hipSuccess) {   // everything is in place before any stream can use the object
        destroy_object(ba);
        return fail("initialising the local bundle adjustment failed");
    }
    *out = ba;
    return 0;
}

void cart_local_ba_destroy(cart_local_ba *ba) { destroy_object(ba); }

int cart_local_ba_clear(cart_local_ba *ba, void *stream_) {
    if (!ba) return fail("ba is NULL");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*ba, stream);
    if (call.begin()) return -1;
    return ba->clear(stream);
}

int cart_local_ba_size(cart_local_ba *ba, int *frames, int *points_capacity) {
    if (!ba) return fail("ba is NULL");
    std::lock_guard<std::mutex> lk(ba->mu);
    if (frames) *frames = ba->frames();
    if (points_capacity) *points_capacity = ba->store.max_points;
    return 0;
}

static int check_params(const cart_local_ba_params *p) {
    if (!p) return fail("params is NULL");
    if (check_positive("min_disparity", p->min_disparity) || check_positive("huber", p->huber)) return -1;
    if (!(p->damping >= 0) || !std::isfinite(p->damping)) return fail("damping must be a finite number that is not negative");
    if (p->iterations < 0 || p->iterations > CART_LOCAL_BA_MAX_ITERATIONS) return fail("iterations must be in [0, 16]");
    if (p->min_observations < 1 || p->min_observations > CART_LOCAL_BA_MAX_WINDOW) return fail("min_observations must be in [1, 16]");
    if (p->min_frame_observations < 0 || p->min_frame_observations > CART_LOCAL_BA_MAX_POINTS) return fail("min_frame_observations must be in [0, 65536]");
    return 0;
}

static Extent block(const char *name, const void *ptr, size_t bytes, size_t elem) { return Extent{name, ptr, bytes, elem, bytes, 1}; }
static int check_aligned(const Extent &x) {
    if (x.ptr && x.begin() % x.elem) return fail(std::string(x.name) + " must be " + std::to_string(x.elem) + "-byte aligned");
    return 0;
}

int cart_local_ba_push(cart_local_ba *ba, const cart_ego_camera *cam, const cart_local_ba_params *params, uint64_t frame_id, const double *pose,
                       const cart_keypoint *kpL, const cart_keypoint *kpR, const int32_t *left_count, const cart_match *stereo, const int32_t *stereo_count,
                       const cart_match *temporal, const int32_t *temporal_count, int32_t *counts_out, void *stream_) {
    if (check_params(params) || check_camera(cam) || check_pose("pose", pose)) return -1;
    if (!ba) return fail("ba is NULL");
    const size_t f = (size_t)ba->store.max_features;
    enum { kKpL, kKpR, kLeftCount, kStereo, kStereoCount, kTemporal, kTemporalCount, kCounts, kAll, kOutputs = kCounts };
    const Extent all[] = {block("kpL", kpL, f * sizeof(cart_keypoint), 4), block("kpR", kpR, f * sizeof(cart_keypoint), 4),
                          block("left_count", left_count, sizeof(int32_t), 4), block("stereo_matches", stereo, f * sizeof(cart_match), 4),
                          block("stereo_count", stereo_count, sizeof(int32_t), 4), block("temporal_matches", temporal, f * sizeof(cart_match), 4),
                          block("temporal_count", temporal_count, sizeof(int32_t), 4), block("counts_out", counts_out, 8 * sizeof(int32_t), 4)};
    static_assert(sizeof(all) / sizeof(all[0]) == kAll, "one entry per index");
    for (int i = 0; i < kAll; ++i)
        if (!all[i].ptr && i != kCounts) return fail(std::string(all[i].name) + " is NULL");
    for (int i = 0; i < kAll; ++i)
        if (check_aligned(all[i])) return -1;
    if (check_outputs_apart(all, kOutputs, kAll)) return -1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*ba, stream);
    if (call.begin()) return -1;
    const int w = ba->store.window;
    LbaPushArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g = ba->store; a.cam = *cam; a.min_disparity = params->min_disparity;
    std::memcpy(a.pose, pose, sizeof(a.pose));
    a.frame_id = frame_id;
    a.slot = (int)(ba->pushed % w);
    a.prev_slot = ba->pushed > 0 ? (int)((ba->pushed - 1) % w) : -1;
    a.evict = ba->pushed >= w ? 1 : 0;
    a.cur = (int)(ba->pushed & 1);
    a.frames = (int)std::min<long long>(ba->pushed + 1, w);
    a.kpL = kpL; a.kpR = kpR; a.left_count = left_count; a.stereo = stereo; a.stereo_count = stereo_count;
    a.temporal = temporal; a.temporal_count = temporal_count; a.counts_out = counts_out;
    launch_local_ba_push(a, stream);
    HIP_TRY(hipGetLastError());
    ba->pushed += 1;
    return 0;
}

int cart_local_ba_optimize(cart_local_ba *ba, const cart_ego_camera *cam, const cart_local_ba_params *params, cart_local_ba_result *result, void *stream_) {
    if (check_params(params) || check_camera(cam)) return -1;
    if (!ba) return fail("ba is NULL");
    if (check_aligned(block("result", result, sizeof(cart_local_ba_result), 8))) return -1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*ba, stream);
    if (call.begin()) return -1;
    LbaOptArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g = ba->store; a.cam = *cam; a.p = *params;
    a.frames = ba->frames(); a.first_slot = ba->first_slot();
    a.result = result;
    launch_local_ba_optimize(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_local_ba_poses(cart_local_ba *ba, double *out, uint64_t *ids_out, void *stream_) {
    if (!ba) return fail("ba is NULL");
    const size_t w = (size_t)ba->store.window;
    const Extent all[] = {block("out", out, w * 12 * sizeof(double), 8), block("ids_out", ids_out, w * sizeof(uint64_t), 8)};
    if (!out) return fail("out is NULL");
    if (check_aligned(all[0]) || check_aligned(all[1]) || check_outputs_apart(all, 0, 2)) return -1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*ba, stream);
    if (call.begin()) return -1;
    launch_local_ba_poses(ba->store, ba->frames(), ba->first_slot(), out, ids_out, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_local_ba_points(cart_local_ba *ba, double *out, void *stream_) {
    if (!ba) return fail("ba is NULL");
    if (!out) return fail("out is NULL");
    if (check_aligned(block("out", out, 0, 8))) return -1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*ba, stream);
    if (call.begin()) return -1;
    launch_local_ba_points(ba->store, out, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_local_ba_track_of(cart_local_ba *ba, int32_t *out, void *stream_) {
    if (!ba) return fail("ba is NULL");
    if (!out) return fail("out is NULL");
    if (check_aligned(block("out", out, 0, 4))) return -1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*ba, stream);
    if (call.begin()) return -1;
    // the newest frame wrote track[(pushed - 1) & 1]; after a clear both hold -1
    HIP_TRY(hipMemcpyAsync(out, ba->store.track[(ba->pushed + 1) & 1], (size_t)ba->store.max_features * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    return 0;
}

}  // extern "C"

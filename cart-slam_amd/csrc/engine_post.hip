// engine_post.hip -- C ABI of the stages behind the disparity image (include/cart_engine.h): interpolation, derivatives, plane
// classification and its schedule, connected components, temporal vote, reprojection, optical flow, resize, the narrow copy
// and the host-side peak finder.
#include <cstdlib>

#include "engine_host.h"

using namespace cart_amd;

namespace {
// Kernels that access a pair or a word as one 4-byte value need the base on a 4-byte boundary as well as the steps.
bool misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

// The strided and the _multi form of a plane stage share one body.  Frame f of an image argument is base + f * frame stride
// bytes or, with pointer tables (base NULL, frame stride 0), the table's f-th entry; a launch takes at most kLaunchFrames of those.
template <typename T>
FrameTable frame_table(T *const *table, int f0, int n) {
    FrameTable t{};
    t.scattered = 1;
    for (int f = 0; table && f < n; ++f) t.p[f] = table[f0 + f];
    return t;
}

int plane_derivative_hist(cart_engine *e, int n_frames, const int16_t *disp, const int16_t *const *disps, size_t disp_step, size_t disp_fs, int16_t *out,
                          int16_t *const *outs, size_t out_step, size_t out_fs, int32_t *hist256, size_t hist_fs, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!(disp || disps) || !(out || outs) || !hist256) return fail("NULL pointer");
    if (n_frames <= 0) return fail("n_frames must be positive");
    const Geometry &g = e->g;
    if (disp_step < (size_t)g.w * 2 || out_step < (size_t)g.w * 2 || ((disp_step | out_step | disp_fs | out_fs) & 1)) return fail("bad step");
    for (int f = 0; disps && f < n_frames; ++f)
        if (!disps[f] || !outs[f]) return fail("NULL image pointer in a pointer table");
    HIP_TRY(hipSetDevice(e->params.device_id));
    const int chunk = disps ? kLaunchFrames : n_frames;   // strided frames: one launch
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int n = std::min(chunk, n_frames - f0);
        const FrameTable dt = frame_table(disps, f0, n), ot = frame_table(outs, f0, n);
        launch_plane_derivative(disp, disp_step, disp_fs, out, out_step, out_fs, hist256 + (size_t)f0 * hist_fs, hist_fs, g.w, g.h, n,
                                static_cast<hipStream_t>(stream_), disps ? &dt : nullptr, disps ? &ot : nullptr);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int plane_classify(cart_engine *e, int n_frames, const int16_t *deriv, const int16_t *const *derivs, size_t deriv_step, size_t deriv_fs,
                   const cart_plane_params *params, int params_per_frame, uint8_t *planes, uint8_t *const *planess, size_t planes_step, size_t planes_fs,
                   void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!(deriv || derivs) || !(planes || planess) || !params) return fail("NULL pointer");
    if (n_frames <= 0) return fail("n_frames must be positive");
    const Geometry &g = e->g;
    if (deriv_step < (size_t)g.w * 2 || planes_step < (size_t)g.w || ((deriv_step | deriv_fs) & 1)) return fail("bad step");
    for (int f = 0; derivs && f < n_frames; ++f)
        if (!derivs[f] || !planess[f]) return fail("NULL image pointer in a pointer table");
    HIP_TRY(hipSetDevice(e->params.device_id));
    static_assert(kMaxBatchArgs >= kLaunchFrames, "one ClassifyParams covers a launch");
    const int chunk = derivs ? kLaunchFrames : kMaxBatchArgs;
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int n = std::min(chunk, n_frames - f0);
        ClassifyParams cp;
        if (params_per_frame) std::memcpy(cp.p, params + f0, sizeof(cart_plane_params) * (size_t)n);
        else cp.p[0] = params[0];
        const FrameTable dt = frame_table(derivs, f0, n), pt = frame_table(planess, f0, n);
        launch_classify(reinterpret_cast<const int16_t *>(reinterpret_cast<const uint8_t *>(deriv) + (size_t)f0 * deriv_fs), deriv_step, deriv_fs, cp,
                        params_per_frame, planes + (size_t)f0 * planes_fs, planes_step, planes_fs, g.w, g.h, n, static_cast<hipStream_t>(stream_),
                        derivs ? &dt : nullptr, derivs ? &pt : nullptr);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" {

int cart_interpolate(cart_engine *e, int n_frames, int16_t *disp, size_t step, size_t frame_stride, int radius,
                     int iterations, int min_disp16, int max_disp, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!disp) return fail("NULL image pointer");
    if (n_frames <= 0) return fail("n_frames must be positive");
    if (radius <= 0 || iterations <= 0) return 0;
    if (radius > 8) return fail("radius must be <= 8");
    const Geometry &g = e->g;
    if (step < (size_t)g.w * 2 || (step & 1) || (frame_stride & 1)) return fail("bad step");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(e->params.device_id));
    SlotLease l;
    if (l.begin(e, n_frames, stream)) return -1;
    int16_t *ta = e->tmp_a + (size_t)l.s0 * g.npx, *tb = e->tmp_b + (size_t)l.s0 * g.npx;
    const size_t ts = (size_t)g.w * 2, tfs = g.npx * 2;
    // pass 0 reads the caller's buffer, the last pass writes it; an extra tight copy keeps Jacobi semantics
    launch_interpolate(disp, step, frame_stride, strided_out(ta, ts, tfs), g.w, g.h, radius, min_disp16, max_disp, n_frames, stream);
    int16_t *src = ta, *dst = tb;
    for (int it = 1; it < iterations; ++it) {
        launch_interpolate(src, ts, tfs, strided_out(dst, ts, tfs), g.w, g.h, radius, min_disp16, max_disp, n_frames, stream);
        std::swap(src, dst);
    }
    hipError_t err = hipSuccess;
    for (int f = 0; f < n_frames && err == hipSuccess; ++f)
        err = hipMemcpy2DAsync(reinterpret_cast<uint8_t *>(disp) + (size_t)f * frame_stride, step, src + (size_t)f * g.npx, ts, ts,
                               g.h, hipMemcpyDeviceToDevice, stream);
    if (err == hipSuccess) err = hipGetLastError();
    if (err != hipSuccess) return fail(std::string("interpolate failed: ") + hipGetErrorString(err));
    return 0;
}

int cart_disparity_derivative(cart_engine *e, int n_frames, const int16_t *disp, size_t disp_step,
                              size_t disp_frame_stride, int16_t *out, size_t out_step, size_t out_frame_stride,
                              int32_t *hist512, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!disp || !out || !hist512) return fail("NULL pointer");
    if (n_frames <= 0) return fail("n_frames must be positive");
    const Geometry &g = e->g;
    if (disp_step < (size_t)g.w * 2 || out_step < (size_t)g.w * 4 || (out_step & 3) || (out_frame_stride & 3) || (disp_step & 1) || (disp_frame_stride & 1))
        return fail("bad step (derivative rows must be 4-byte aligned)");
    if (misaligned4(out)) return fail("out must be 4-byte aligned");
    HIP_TRY(hipSetDevice(e->params.device_id));
    launch_dir_derivative(disp, disp_step, disp_frame_stride, out, out_step, out_frame_stride, hist512, g.w, g.h, n_frames,
                          static_cast<hipStream_t>(stream_));
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_plane_derivative_hist(cart_engine *e, int n_frames, const int16_t *disp, size_t disp_step,
                               size_t disp_frame_stride, int16_t *out, size_t out_step, size_t out_frame_stride,
                               int32_t *hist256, size_t hist_frame_stride_elems, void *stream) {
    return plane_derivative_hist(e, n_frames, disp, nullptr, disp_step, disp_frame_stride, out, nullptr, out_step, out_frame_stride, hist256,
                                 hist_frame_stride_elems, stream);
}

int cart_plane_derivative_hist_multi(cart_engine *e, int n_frames, const int16_t *const *disp, size_t disp_step, int16_t *const *out,
                                     size_t out_step, int32_t *hist256, size_t hist_frame_stride_elems, void *stream) {
    return plane_derivative_hist(e, n_frames, nullptr, disp, disp_step, 0, nullptr, out, out_step, 0, hist256, hist_frame_stride_elems, stream);
}

int cart_plane_classify(cart_engine *e, int n_frames, const int16_t *deriv, size_t deriv_step, size_t deriv_frame_stride,
                        const cart_plane_params *params, int params_per_frame, uint8_t *planes, size_t planes_step,
                        size_t planes_frame_stride, void *stream) {
    return plane_classify(e, n_frames, deriv, nullptr, deriv_step, deriv_frame_stride, params, params_per_frame, planes, nullptr, planes_step,
                          planes_frame_stride, stream);
}

int cart_plane_classify_multi(cart_engine *e, int n_frames, const int16_t *const *deriv, size_t deriv_step, const cart_plane_params *params,
                              int params_per_frame, uint8_t *const *planes, size_t planes_step, void *stream) {
    return plane_classify(e, n_frames, nullptr, deriv, deriv_step, 0, params, params_per_frame, nullptr, planes, planes_step, 0, stream);
}

int cart_plane_ccl(cart_engine *e, int n_frames, const uint8_t *planes, size_t planes_step, size_t planes_frame_stride,
                   int32_t *ids, size_t ids_step, size_t ids_frame_stride, int32_t *n_components, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!planes || !ids) return fail("NULL pointer");
    if (n_frames <= 0) return fail("n_frames must be positive");
    const Geometry &g = e->g;
    if (planes_step < (size_t)g.w || ids_step < (size_t)g.w * 4 || (ids_step & 3) || (ids_frame_stride & 3)) return fail("bad step");
    if (misaligned4(ids)) return fail("ids must be 4-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(e->params.device_id));
    SlotLease l;
    if (l.begin(e, n_frames, stream)) return -1;
    launch_ccl(planes, planes_step, planes_frame_stride, e->ccl_work + (size_t)l.s0 * g.npx, ids, ids_step, ids_frame_stride,
               n_components, g.w, g.h, n_frames, stream);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(std::string("ccl failed: ") + hipGetErrorString(err));
    return 0;
}

namespace {
// The component-table workspace: [slots][npx][kCclStatInts] statistics scratch, then [slots][h][tile columns] root counts (post_kernels.hip).
// The scratch is zeroed ONCE, when it is allocated: every call returns it to zero (ccl_table_kernel collects and clears exactly the entries
// the call grew).
int ensure_ccl_stats_ws(cart_engine *e) { return ensure_ws(e, &e->ccl_stats_ws, ccl_stats_ws_ints(e->g.w, e->g.h) * sizeof(int32_t), true); }
int32_t *ccl_stat_of(cart_engine *e, int slot) { return e->ccl_stats_ws + (size_t)slot * e->g.npx * kCclStatInts; }
int32_t *ccl_seg_of(cart_engine *e, int slot) {
    const size_t stat_ints = e->g.npx * kCclStatInts;
    return e->ccl_stats_ws + e->slots.size() * stat_ints + (size_t)slot * (ccl_stats_ws_ints(e->g.w, e->g.h) - stat_ints);
}
}  // namespace

int cart_plane_ccl_stats(cart_engine *e, int n_frames, const uint8_t *planes, size_t planes_step, size_t planes_frame_stride,
                         const int32_t *ids, size_t ids_step, size_t ids_frame_stride, cart_component *table, int max_components,
                         int32_t *n_components, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!planes || !ids || !table) return fail("NULL pointer");
    if (max_components < 1) return fail("max_components must be positive");
    if (n_frames <= 0) return fail("n_frames must be positive");
    const Geometry &g = e->g;
    if (planes_step < (size_t)g.w || ids_step < (size_t)g.w * 4 || (ids_step & 3) || (ids_frame_stride & 3)) return fail("bad step");
    if (misaligned4(ids)) return fail("ids must be 4-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(e->params.device_id));
    if (ensure_ccl_stats_ws(e)) return -1;
    SlotLease l;
    if (l.begin(e, n_frames, stream)) return -1;
    launch_ccl_stats(planes, planes_step, planes_frame_stride, ids, ids_step, ids_frame_stride, ccl_stat_of(e, l.s0), ccl_seg_of(e, l.s0), table, max_components,
                     n_components, g.w, g.h, n_frames, stream);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(std::string("ccl stats failed: ") + hipGetErrorString(err));
    return 0;
}

int cart_plane_ccl_table(cart_engine *e, int n_frames, const uint8_t *planes, size_t planes_step, size_t planes_frame_stride, int32_t *ids, size_t ids_step,
                         size_t ids_frame_stride, cart_component *table, int max_components, int32_t *n_components, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!planes || !ids || !table) return fail("NULL pointer");
    if (max_components < 1) return fail("max_components must be positive");
    if (n_frames <= 0) return fail("n_frames must be positive");
    const Geometry &g = e->g;
    if (planes_step < (size_t)g.w || ids_step < (size_t)g.w * 4 || (ids_step & 3) || (ids_frame_stride & 3)) return fail("bad step");
    if (misaligned4(ids)) return fail("ids must be 4-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(e->params.device_id));
    if (ensure_ccl_stats_ws(e)) return -1;
    SlotLease l;
    if (l.begin(e, n_frames, stream)) return -1;
    launch_ccl(planes, planes_step, planes_frame_stride, e->ccl_work + (size_t)l.s0 * g.npx, ids, ids_step, ids_frame_stride, n_components, g.w, g.h, n_frames, stream,
               ccl_stat_of(e, l.s0), ccl_seg_of(e, l.s0), table, max_components);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(std::string("ccl failed: ") + hipGetErrorString(err));
    return 0;
}

struct cart_plane_schedule {
    int device_id;         // the engine's; kept here so that the schedule can outlive the engine it was created on
    ScheduleState *state;  // device
    int provider, update_interval, reset_interval;
};

int cart_plane_schedule_create(cart_engine *e, int provider, const cart_plane_params *initial, int update_interval,
                               int reset_interval, cart_plane_schedule **out) {
    if (!e || !out) return fail("bad arguments");
    if (provider != 0 && provider != 1) return fail("Unknown parameter provider type.");
    if (update_interval < 1 || reset_interval < 1) return fail("intervals must be >= 1");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_plane_schedule *s = new (std::nothrow) cart_plane_schedule{e->params.device_id, nullptr, provider, update_interval, reset_interval};
    if (!s) return fail("out of host memory");
    ScheduleState init;
    std::memset(&init, 0, sizeof(init));
    if (initial) init.params = *initial;
    if (hipMalloc(reinterpret_cast<void **>(&s->state), sizeof(ScheduleState)) != hipSuccess ||
        hipMemcpy(s->state, &init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) {
        cart_plane_schedule_destroy(s);
        return fail("hipMalloc/hipMemcpy of the schedule state failed");
    }
    *out = s;
    return 0;
}

void cart_plane_schedule_destroy(cart_plane_schedule *s) {
    if (!s) return;
    (void)hipSetDevice(s->device_id);   // the caller's current device may be another one
    if (s->state) (void)hipFree(s->state);
    delete s;
}

int cart_plane_schedule_advance(cart_plane_schedule *s, int first_id, int n_frames, const int32_t *hists,
                                cart_plane_params *params_out, void *stream) {
    if (!s || !hists || !params_out) return fail("bad arguments");
    if (n_frames <= 0 || first_id < 1) return fail("n_frames must be positive and ids are 1-based");
    HIP_TRY(hipSetDevice(s->device_id));
    launch_plane_schedule(s->state, s->provider, first_id, n_frames, s->update_interval, s->reset_interval, hists, params_out,
                          static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_plane_schedule_read(cart_plane_schedule *s, cart_plane_params *params_host, int32_t cum_hist_host[256]) {
    if (!s) return fail("bad arguments");
    HIP_TRY(hipSetDevice(s->device_id));
    HIP_TRY(hipDeviceSynchronize());
    ScheduleState st;
    HIP_TRY(hipMemcpy(&st, s->state, sizeof(st), hipMemcpyDeviceToHost));
    if (params_host) *params_host = st.params;
    if (cum_hist_host) std::memcpy(cum_hist_host, st.cum, sizeof(st.cum));
    return 0;
}

int cart_plane_classify_dev(cart_engine *e, int n_frames, const int16_t *deriv, size_t deriv_step, size_t deriv_frame_stride,
                            const cart_plane_params *params_dev, int params_stride, uint8_t *planes, size_t planes_step,
                            size_t planes_frame_stride, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!deriv || !planes || !params_dev) return fail("NULL pointer");
    if (n_frames <= 0) return fail("n_frames must be positive");
    const Geometry &g = e->g;
    if (deriv_step < (size_t)g.w * 2 || planes_step < (size_t)g.w || (deriv_step & 1) || (deriv_frame_stride & 1)) return fail("bad step");
    HIP_TRY(hipSetDevice(e->params.device_id));
    launch_classify_dev(deriv, deriv_step, deriv_frame_stride, params_dev, params_stride ? 1 : 0, planes, planes_step, planes_frame_stride,
                        g.w, g.h, n_frames, static_cast<hipStream_t>(stream_));
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_plane_temporal_vote(cart_engine *e, const uint8_t *planes, size_t planes_step, int n_prev, const uint8_t *const *prev_planes,
                             const size_t *prev_steps, const int16_t *const *flows, const size_t *flow_steps, uint8_t *smoothed,
                             size_t smoothed_step, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!planes || !smoothed) return fail("NULL pointer");
    if (n_prev < 0 || n_prev > CART_MAX_TEMPORAL) return fail("n_prev must be in [0, CART_MAX_TEMPORAL]");
    if (n_prev > 0 && (!prev_planes || !prev_steps || !flows || !flow_steps)) return fail("NULL table");
    const Geometry &g = e->g;
    if (planes_step < (size_t)g.w || smoothed_step < (size_t)g.w) return fail("bad step");
    TemporalArgs t;
    std::memset(&t, 0, sizeof(t));
    t.n_prev = n_prev;
    for (int k = 0; k < n_prev; ++k) {
        if (!prev_planes[k] || !flows[k]) return fail("NULL entry in the temporal tables");
        if (prev_steps[k] < (size_t)g.w || flow_steps[k] < (size_t)g.w * 4 || (flow_steps[k] & 3)) return fail("bad step in the temporal tables");
        if (misaligned4(flows[k])) return fail("flow images must be 4-byte aligned");
        t.prev[k] = prev_planes[k]; t.prev_step[k] = prev_steps[k]; t.flow[k] = flows[k]; t.flow_step[k] = flow_steps[k];
    }
    HIP_TRY(hipSetDevice(e->params.device_id));
    launch_temporal_vote(planes, planes_step, t, smoothed, smoothed_step, g.w, g.h, static_cast<hipStream_t>(stream_));
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_reproject_depth(cart_engine *e, int n_frames, const int16_t *disp, size_t disp_step, size_t disp_frame_stride, const float Q[16],
                         float *xyz, size_t xyz_step, size_t xyz_frame_stride, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!disp || !xyz || !Q) return fail("NULL pointer");
    if (n_frames <= 0) return fail("n_frames must be positive");
    const Geometry &g = e->g;
    if (disp_step < (size_t)g.w * 2 || (disp_step & 1) || (disp_frame_stride & 1) || xyz_step < (size_t)g.w * 12 || (xyz_step & 3) || (xyz_frame_stride & 3))
        return fail("bad step");
    if (misaligned4(xyz)) return fail("xyz must be 4-byte aligned");
    HIP_TRY(hipSetDevice(e->params.device_id));
    QMatrix q;
    std::memcpy(q.q, Q, sizeof(q.q));
    launch_reproject(disp, disp_step, disp_frame_stride, q, xyz, xyz_step, xyz_frame_stride, g.w, g.h, n_frames, static_cast<hipStream_t>(stream_));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- optical flow (oracle S15) ----
int cart_optical_flow(cart_engine *e, const uint8_t *cur, size_t cur_step, const uint8_t *prev, size_t prev_step, int channels,
                      int radius, int block, int16_t *flow, size_t flow_step, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!cur || !prev || !flow) return fail("NULL image pointer");
    if (channels != 1 && channels != 3) return fail("channels must be 1 (gray) or 3 (BGR)");
    if (radius < 1 || radius > 16) return fail("radius must be in [1, 16]");
    if (block < 1 || block > 3) return fail("block must be in [1, 3]");
    const Geometry &g = e->g;
    if (cur_step < (size_t)g.w * channels || prev_step < (size_t)g.w * channels) return fail("input step smaller than a row");
    if (flow_step < (size_t)g.w * 4 || (flow_step & 3) || (reinterpret_cast<uintptr_t>(flow) & 3)) return fail("bad step");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(e->params.device_id));
    const size_t cen_bytes = g.census_elems * sizeof(uint32_t);
    const size_t ws_bytes = ((2 * g.npx + 255) & ~(size_t)255) + 2 * cen_bytes + g.npx * sizeof(uint32_t);
    if (ensure_ws(e, &e->flow_ws, ws_bytes)) return -1;
    SlotLease l;
    if (l.begin(e, 1, stream)) return -1;
    uint8_t *ws = e->flow_ws + (size_t)l.s0 * ws_bytes;
    uint8_t *gray_c = ws, *gray_p = ws + g.npx;
    uint32_t *cen_c = reinterpret_cast<uint32_t *>(ws + ((2 * g.npx + 255) & ~(size_t)255));
    uint32_t *cen_p = cen_c + g.census_elems;
    uint32_t *scratch = cen_p + g.census_elems;   // census_kernel also resets a right-view plane: unused here
    const ImageBatch cb = strided_images(cur, cur_step, 0), pb = strided_images(prev, prev_step, 0);
    launch_census(cb, pb, channels, 1, gray_c, gray_p, cen_c, cen_p, scratch, g, stream);
    launch_block_flow(cen_c, cen_p, g, radius, block, flow, flow_step, stream);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(err));
    return 0;
}

// ---- coarse-to-fine optical flow (spec S21) ----
namespace {
constexpr int kFlowMaxLevels = 6, kFlowMinW = 24, kFlowMinH = 16;

int flow_level_sizes(int w, int h, int levels, int *lw, int *lh) {
    int n = 1, cw = w, ch = h;
    if (lw) lw[0] = w;
    if (lh) lh[0] = h;
    while (n < levels) {
        const int nw = (cw + 1) >> 1, nh = (ch + 1) >> 1;
        if (nw < kFlowMinW || nh < kFlowMinH) break;
        cw = nw; ch = nh;
        if (lw) lw[n] = cw;
        if (lh) lh[n] = ch;
        ++n;
    }
    return n;
}

// One slot of the pyramid workspace, laid out for the most levels a call may ask for (every region 256-byte aligned).
struct FlowPyrLayout {
    int n;                          // levels of the kFlowMaxLevels plan
    Geometry g[kFlowMaxLevels];     // w, h, npx, cpitch, cpadl, census_elems of a level: what launch_census and the flow kernels read
    size_t gray_c[kFlowMaxLevels], gray_p[kFlowMaxLevels], cen_c[kFlowMaxLevels], cen_p[kFlowMaxLevels];
    size_t raw[kFlowMaxLevels], flow[kFlowMaxLevels];   // winners before the median / the level's flow, s16 [h][w][2]
    size_t sink, scratch;           // launch_census also writes a gray copy (levels >= 1: of its own input) and resets a right-view plane
    size_t bytes;

    explicit FlowPyrLayout(const Geometry &eg) {
        int lw[kFlowMaxLevels], lh[kFlowMaxLevels];
        n = flow_level_sizes(eg.w, eg.h, kFlowMaxLevels, lw, lh);
        size_t off = 0;
        auto take = [&off](size_t b) { const size_t at = off; off += (b + 255) & ~(size_t)255; return at; };
        for (int l = 0; l < n; ++l) {
            Geometry &q = g[l];
            q = Geometry{};
            q.w = lw[l]; q.h = lh[l];
            q.cpadl = 16;                                  // census rows: 16 zero features left, at least 16 right
            q.cpitch = ((q.cpadl + q.w + 16 + 15) / 16) * 16;
            q.npx = (size_t)q.w * q.h;
            q.census_elems = (size_t)q.h * q.cpitch;
            gray_c[l] = take(q.npx); gray_p[l] = take(q.npx);
            cen_c[l] = take(q.census_elems * 4); cen_p[l] = take(q.census_elems * 4);
            raw[l] = take(q.npx * 4); flow[l] = take(q.npx * 4);
        }
        sink = take(2 * g[n > 1 ? 1 : 0].npx);
        scratch = take(g[0].npx * 4);
        bytes = off;
    }
};

struct FlowPyrLast { const cart_engine *e = nullptr; int slot = 0, levels = 0; };
thread_local FlowPyrLast g_flow_last;   // cart_flow_debug_level
}  // namespace

void cart_flow_default_params(cart_flow_params *p) {
    if (p) *p = cart_flow_params{4, 4, 2, 2, 1};
}

int cart_flow_pyramid_levels(int width, int height, int levels, int *level_w, int *level_h) {
    if (width < 1 || height < 1 || levels < 1 || levels > kFlowMaxLevels) return fail("bad size, or levels not in [1, 6]");
    return flow_level_sizes(width, height, levels, level_w, level_h);
}

int cart_optical_flow_pyramid(cart_engine *e, const uint8_t *cur, size_t cur_step, const uint8_t *prev, size_t prev_step, int channels,
                              const cart_flow_params *fp, int16_t *flow, size_t flow_step, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!cur || !prev || !flow || !fp) return fail("NULL pointer");
    if (channels != 1 && channels != 3) return fail("channels must be 1 (gray) or 3 (BGR)");
    if (fp->levels < 1 || fp->levels > kFlowMaxLevels) return fail("levels must be in [1, 6]");
    if (fp->radius < 1 || fp->radius > 16) return fail("radius must be in [1, 16]");
    if (fp->refine_radius < 1 || fp->refine_radius > 4) return fail("refine_radius must be in [1, 4]");
    if (fp->block < 1 || fp->block > 3) return fail("block must be in [1, 3]");
    if (fp->median != 0 && fp->median != 1) return fail("median must be 0 or 1");
    const Geometry &g = e->g;
    if (cur_step < (size_t)g.w * channels || prev_step < (size_t)g.w * channels) return fail("input step smaller than a row");
    if (flow_step < (size_t)g.w * 4 || (flow_step & 3) || (reinterpret_cast<uintptr_t>(flow) & 3)) return fail("bad step");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(e->params.device_id));
    const FlowPyrLayout L(g);
    const int n = std::min(fp->levels, L.n);   // = flow_level_sizes(w, h, levels): the plans share their first levels
    // zeroed once: nothing ever writes the padding left and right of a census row
    if (ensure_ws(e, &e->flow_pyr_ws, L.bytes, true)) return -1;
    bool gather;
    { std::lock_guard<std::mutex> lk(e->mu); gather = e->opt_flow_gather != 0; }
    SlotLease l;
    if (l.begin(e, 1, stream)) return -1;
    g_flow_last = FlowPyrLast{e, l.s0, n};
    uint8_t *ws = e->flow_pyr_ws + (size_t)l.s0 * L.bytes;
    auto u32 = [ws](size_t off) { return reinterpret_cast<uint32_t *>(ws + off); };
    auto s16 = [ws](size_t off) { return reinterpret_cast<int16_t *>(ws + off); };
    launch_census(strided_images(cur, cur_step, 0), strided_images(prev, prev_step, 0), channels, 1, ws + L.gray_c[0], ws + L.gray_p[0], u32(L.cen_c[0]),
                  u32(L.cen_p[0]), u32(L.scratch), L.g[0], stream);
    for (int k = 1; k < n; ++k) {
        const Geometry &q = L.g[k];
        launch_flow_downsample(ws + L.gray_c[k - 1], ws + L.gray_p[k - 1], L.g[k - 1].w, L.g[k - 1].h, ws + L.gray_c[k], ws + L.gray_p[k], stream);
        launch_census(strided_images(ws + L.gray_c[k], (size_t)q.w, 0), strided_images(ws + L.gray_p[k], (size_t)q.w, 0), 1, 1, ws + L.sink,
                      ws + L.sink + q.npx, u32(L.cen_c[k]), u32(L.cen_p[k]), u32(L.scratch), q, stream);
    }
    // Coarsest level first.  A level's search writes its winners to raw[k] and the median makes flow[k] of them; without the median the
    // search writes flow[k] itself.  Whatever makes flow[0] also writes the caller's S10.5 image -- the S15 kernel cannot write both,
    // so a single level without the median takes the median kernel as a plain copy.
    for (int k = n - 1; k >= 0; --k) {
        const Geometry &q = L.g[k];
        const bool coarsest = k == n - 1, second = fp->median || (coarsest && k == 0);
        int16_t *win = s16(second ? L.raw[k] : L.flow[k]);
        int16_t *out32 = k == 0 ? flow : nullptr;
        if (coarsest) launch_block_flow(u32(L.cen_c[k]), u32(L.cen_p[k]), q, fp->radius, fp->block, win, (size_t)q.w * 4, stream, 1);
        else launch_flow_refine(u32(L.cen_c[k]), u32(L.cen_p[k]), q, s16(L.flow[k + 1]), L.g[k + 1].w, fp->refine_radius, fp->block, gather, win,
                                second ? nullptr : out32, flow_step, stream);
        if (second) launch_flow_median(win, q.w, q.h, fp->median != 0, s16(L.flow[k]), out32, flow_step, stream);
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(err));
    return 0;
}

int cart_flow_debug_level(cart_engine *e, int level, int what, void *host_dst, size_t bytes) {
    if (!e || !host_dst) return fail("bad arguments");
    if (what < 0 || what > 2) return fail("what must be 0 (cur image), 1 (prev image) or 2 (flow)");
    if (g_flow_last.e != e || !e->flow_pyr_ws) return fail("this thread has made no cart_optical_flow_pyramid call on this engine");
    if (level < 0 || level >= g_flow_last.levels) return fail("that call did not build this level");
    const FlowPyrLayout L(e->g);
    const size_t want = L.g[level].npx * (what == 2 ? 4 : 1);
    if (bytes != want) return fail("bytes must be the size of the level");
    HIP_TRY(hipSetDevice(e->params.device_id));
    HIP_TRY(hipDeviceSynchronize());
    const size_t off = what == 0 ? L.gray_c[level] : what == 1 ? L.gray_p[level] : L.flow[level];
    HIP_TRY(hipMemcpy(host_dst, e->flow_pyr_ws + (size_t)g_flow_last.slot * L.bytes + off, want, hipMemcpyDeviceToHost));
    return 0;
}

int cart_resize_linear(int device_id, const uint8_t *src, size_t src_step, int sw, int sh, int channels, uint8_t *dst, size_t dst_step, int dw,
                       int dh, void *stream_) {
    if (!src || !dst) return fail("NULL image pointer");
    if (channels != 1 && channels != 3) return fail("channels must be 1 or 3");
    if (sw < 1 || sh < 1 || dw < 1 || dh < 1 || sw > 16384 || sh > 16384 || dw > 16384 || dh > 16384) return fail("unsupported image size");
    if (src_step < (size_t)sw * channels || dst_step < (size_t)dw * channels) return fail("step smaller than a row");
    HIP_TRY(hipSetDevice(device_id));
    launch_resize_linear(src, src_step, sw, sh, channels, dst, dst_step, dw, dh, static_cast<hipStream_t>(stream_));
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_copy_narrow(cart_engine *e, void *dst, const void *src, size_t bytes, int workgroups, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (!dst || !src) return fail("NULL pointer");
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) return fail("buffers must be 16-byte aligned");
    if (workgroups < 0 || workgroups > 1024) return fail("workgroups must be in [0, 1024]");
    if (bytes == 0) return 0;
    HIP_TRY(hipSetDevice(e->params.device_id));
    launch_narrow_copy(src, dst, bytes, workgroups ? workgroups : 8, static_cast<hipStream_t>(stream_));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- host-side peak finder (replaces src/utils/peaks.cpp:12-72 and planeseg.cu:405-458) ----
int cart_find_peaks(const int32_t *data, int n, int *born, int *died, int *left, int *right) {
    if (!data || n <= 0 || !born || !died || !left || !right) return fail("bad arguments");
    try {
    std::vector<int> order(n), owner(n, -1);
    for (int i = 0; i < n; ++i) order[i] = i;
    // descending value, ties by ascending index (oracle S11; the reference's std::sort leaves ties open)
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return data[a] > data[b]; });
    int np = 0;
    for (int idx : order) {
        const int il = (idx > 0) ? owner[idx - 1] : -1;
        const int ir = (idx < n - 1) ? owner[idx + 1] : -1;
        if (il < 0 && ir < 0) {  // a new component is born at a local maximum
            born[np] = left[np] = right[np] = idx; died[np] = -1;
            owner[idx] = np++;
        } else if (il >= 0 && ir < 0) {
            right[il] += 1; owner[idx] = il;
        } else if (il < 0 && ir >= 0) {
            left[ir] -= 1; owner[idx] = ir;
        } else if (data[born[il]] > data[born[ir]]) {  // the younger (lower) peak dies at this saddle
            died[ir] = idx; right[il] = right[ir];
            owner[right[il]] = owner[idx] = il;
        } else {
            died[il] = idx; left[ir] = left[il];
            owner[left[ir]] = owner[idx] = ir;
        }
    }
    std::vector<int> perm(np);
    for (int i = 0; i < np; ++i) perm[i] = i;
    auto persistence = [&](int k) -> long long { return died[k] < 0 ? (long long)INT32_MAX : (long long)data[born[k]] - data[died[k]]; };
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return persistence(a) > persistence(b); });
    std::vector<int> b2(np), d2(np), l2(np), r2(np);
    for (int i = 0; i < np; ++i) { b2[i] = born[perm[i]]; d2[i] = died[perm[i]]; l2[i] = left[perm[i]]; r2[i] = right[perm[i]]; }
    for (int i = 0; i < np; ++i) { born[i] = b2[i]; died[i] = d2[i]; left[i] = l2[i]; right[i] = r2[i]; }
    return np;
    } catch (const std::bad_alloc &) { return fail("out of host memory"); }   // nothing is thrown across the C ABI
}

int cart_find_plane_params(const int32_t hist[256], cart_plane_params *io) {
    if (!hist || !io) return fail("bad arguments");
    int born[256], died[256], left[256], right[256];
    const int np = cart_find_peaks(hist, 256, born, died, left, right);
    if (np < 2) return 0;  // planeseg.cu:408-411
    int pv = born[0], ph = born[1];
    if (std::abs(pv - 128) > std::abs(ph - 128)) std::swap(pv, ph);  // vertical = nearer to zero derivative (:414-416)
    io->vertical_center = pv - 128;
    io->horizontal_center = ph - 128;
    int valley = std::min(pv, ph);
    for (int i = valley; i < std::max(pv, ph); ++i)
        if (hist[i] < hist[valley]) valley = i;  // :422-428
    const int vdist = std::abs(valley - pv), hdist = std::abs(valley - ph);
    if (vdist == 0 || hdist == 0) return 0;  // :436-439
    const int vslope = (hist[pv] - hist[valley]) / vdist, hslope = (hist[ph] - hist[valley]) / hdist;
    if (vslope == 0 || hslope == 0) return 0;  // :444-447
    const int vwidth = hist[pv] / vslope, hwidth = hist[ph] / hslope;
    io->vertical_min = pv - vwidth - 128; io->vertical_max = valley - 127;      // :452
    io->horizontal_min = valley - 127; io->horizontal_max = ph + hwidth - 127;  // :453
    return 1;
}

}  // extern "C"

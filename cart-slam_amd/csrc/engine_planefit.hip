// engine_planefit.hip -- C ABI of superpixel plane fitting (include/cart_engine.h): the cart_planefit device
// object and the host-side plane cluster.
#include <set>

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

// ---- superpixel plane fitting ----
struct cart_planefit : DeviceObject {
    using DeviceObject::DeviceObject;
    int cap_L1 = 0, ntiles = 0;
    int32_t *cursor = nullptr;    // [ntiles][cap_L1] tile counts -> tile offsets
    int32_t *cnt = nullptr;       // [cap_L1][2]
    int32_t *npts = nullptr;      // [cap_L1]
    int32_t *start = nullptr;     // [cap_L1 + 1]
    int32_t *err = nullptr;       // [2] words.  [0], cleared by label_planes and by adjacency (cart_planefit_status): label out of range
                                  // (bit 0), adjacency capacity (bit 1)
    int32_t *lp_err = nullptr;    // = err + 1, cleared by label_planes alone: label out of range in the call cart_planefit_fit rests on
    float4 *pts = nullptr;        // [w*h]
    double *planes17 = nullptr;   // [cap_L1][4]
    uint32_t *bits = nullptr;     // [cap_L1][words] adjacency bitmap (allocated by the first adjacency call)
    int32_t *adj_cnt = nullptr;   // [cap_L1]
    PfFitState *state = nullptr;
    double *local = nullptr;      // [kPfMaxLocal][4]
    uint64_t *accept = nullptr;   // [cap_L1]
    int last_L1 = 0, last_pred = -1;
};

namespace {
int pf_grid_slots(int w, int h) {   // selectRandomSuperpixels(4, 3) positions (planefit.cu:333-351)
    const int ys = h / 5, xs = w / 6;
    return (ys > 0 && xs > 0) ? ((h - 1) / ys) * ((w - 1) / xs) : 0;
}
Extent pf_xyz_extent(const float *xyz, size_t step, const Geometry &g) {   // CV_32FC3: 12-byte pixels, pointer and step on 4 bytes
    return Extent{"xyz", xyz, step, 4, (size_t)g.w * 12, g.h};
}
}  // namespace

int cart_planefit_create(cart_engine *e, int max_label_capacity, cart_planefit **out) {
    if (!e || !out) return fail("bad arguments");
    if (max_label_capacity < 0 || max_label_capacity >= kSpMaxLabels) return fail("max_label_capacity must be in [0, 16383]");
    const Geometry &g = e->g;
    if (pf_grid_slots(g.w, g.h) > kPfMaxLocal) return fail("image too small for the planefit sampling grid");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_planefit *pf = new (std::nothrow) cart_planefit(e);
    if (!pf) return fail("out of host memory");
    pf->cap_L1 = max_label_capacity + 1; pf->ntiles = pf_tiles(g.w, g.h);
    const size_t L1 = (size_t)pf->cap_L1;
    if (pf->alloc(&pf->cursor, (size_t)pf->ntiles * L1 * 4) || pf->alloc(&pf->cnt, L1 * 8) || pf->alloc(&pf->npts, L1 * 4) ||
        pf->alloc(&pf->start, (L1 + 1) * 4) || pf->alloc(&pf->err, 8) || pf->alloc(&pf->pts, g.npx * sizeof(float4)) ||
        pf->alloc(&pf->planes17, L1 * 32) || pf->alloc(&pf->adj_cnt, L1 * 4) || pf->alloc(&pf->state, sizeof(PfFitState)) ||
        pf->alloc(&pf->local, (size_t)kPfMaxLocal * 32) || pf->alloc(&pf->accept, L1 * 8) || hipMemset(pf->err, 0, 8) != hipSuccess ||
        pf->create_event()) {
        destroy_object(pf);
        return fail("allocating the planefit workspaces failed");
    }
    pf->lp_err = pf->err + 1;
    *out = pf;
    return 0;
}

void cart_planefit_destroy(cart_planefit *pf) { destroy_object(pf); }

int cart_planefit_label_planes(cart_planefit *pf, const uint16_t *labels, size_t labels_step, int max_label, const float *xyz, size_t xyz_step,
                               int predicate, double thr, uint64_t seed, uint64_t frame_id, double *planes, int32_t *npoints, int32_t *counts,
                               void *stream_) {
    if (!pf) return fail("planefit is NULL");
    if (!labels || !xyz) return fail("NULL image pointer");
    if (max_label < 0 || max_label + 1 > pf->cap_L1) return fail("max_label must be in [0, max_label_capacity]");
    if (predicate != CART_PLANE_PREDICATE_PLANEFIT && predicate != CART_PLANE_PREDICATE_PLANECLUSTER) return fail("unknown predicate");
    if (!(thr > 0)) return fail("thr must be positive");
    const Geometry &g = pf->g;
    if (check_pitched(Extent::image("labels", labels, labels_step, 2, g.w, g.h)) || check_pitched(pf_xyz_extent(xyz, xyz_step, g))) return -1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*pf, stream);
    if (call.begin()) return -1;
    const int L1 = max_label + 1;
    HIP_TRY(hipMemsetAsync(pf->cursor, 0, (size_t)pf->ntiles * L1 * 4, stream));
    HIP_TRY(hipMemsetAsync(pf->cnt, 0, (size_t)L1 * 8, stream));
    HIP_TRY(hipMemsetAsync(pf->err, 0, 8, stream));   // both words: the status flag and this call's own
    launch_pf_points(labels, labels_step, xyz, xyz_step, g.w, g.h, L1, predicate, pf->cursor, pf->ntiles, pf->cnt, pf->npts, pf->start,
                     pf->pts, pf->err, pf->lp_err, stream);
    launch_pf_ransac(pf->pts, pf->start, pf->npts, L1, thr, seed, frame_id, pf->planes17, stream);
    HIP_TRY(hipGetLastError());
    if (planes) HIP_TRY(hipMemcpyAsync(planes, pf->planes17, (size_t)L1 * 32, hipMemcpyDeviceToDevice, stream));
    if (npoints) HIP_TRY(hipMemcpyAsync(npoints, pf->npts, (size_t)L1 * 4, hipMemcpyDeviceToDevice, stream));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, pf->cnt, (size_t)L1 * 8, hipMemcpyDeviceToDevice, stream));
    pf->last_L1 = L1;
    pf->last_pred = predicate;
    return 0;
}

int cart_planefit_points(cart_planefit *pf, float *points, size_t capacity, int32_t *offsets, void *stream_) {
    if (!pf) return fail("planefit is NULL");
    if (!points || !offsets) return fail("NULL pointer");
    if (pf->last_L1 == 0) return fail("no label_planes call yet");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*pf, stream);
    if (call.begin()) return -1;
    int32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, pf->start + pf->last_L1, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if ((size_t)total > capacity) return fail("capacity is smaller than the number of points");
    HIP_TRY(hipMemcpyAsync(points, pf->pts, (size_t)total * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(offsets, pf->start, ((size_t)pf->last_L1 + 1) * 4, hipMemcpyDeviceToDevice, stream));
    return 0;
}

int cart_planefit_adjacency(cart_planefit *pf, const uint16_t *labels, size_t labels_step, int max_label, int32_t *offsets, int32_t *neighbours,
                            size_t capacity, void *stream_) {
    if (!pf) return fail("planefit is NULL");
    if (!labels || !offsets || !neighbours) return fail("NULL pointer");
    if (max_label < 0 || max_label + 1 > pf->cap_L1) return fail("max_label must be in [0, max_label_capacity]");
    const Geometry &g = pf->g;
    if (check_pitched(Extent::image("labels", labels, labels_step, 2, g.w, g.h))) return -1;
    const size_t L1 = (size_t)max_label + 1;
    if (capacity < std::min(8 * g.npx, L1 * (L1 - 1))) return fail("capacity must be >= min(8 * width * height, (max_label + 1) * max_label)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*pf, stream);
    if (call.begin()) return -1;
    const size_t words = ((size_t)pf->cap_L1 + 31) / 32;
    if (!pf->bits && pf->alloc(&pf->bits, (size_t)pf->cap_L1 * words * 4)) return -1;
    const size_t used_words = (L1 + 31) / 32;
    HIP_TRY(hipMemsetAsync(pf->bits, 0, L1 * used_words * 4, stream));
    HIP_TRY(hipMemsetAsync(pf->err, 0, 4, stream));   // the status flag only: lp_err stays with the label_planes call that fit uses
    launch_pf_adjacency(labels, labels_step, g.w, g.h, (int)L1, pf->bits, pf->adj_cnt, offsets, neighbours, capacity, pf->err, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_planefit_fit(cart_planefit *pf, const uint16_t *labels, size_t labels_step, uint64_t seed, uint64_t frame_id, double *planes,
                      uint64_t *assignments, int32_t *n_planes, int *launches, void *stream_) {
    if (!pf) return fail("planefit is NULL");
    if (!labels || !planes || !assignments || !n_planes) return fail("NULL pointer");
    if (pf->last_L1 == 0 || pf->last_pred != CART_PLANE_PREDICATE_PLANEFIT)
        return fail("cart_planefit_fit needs a preceding label_planes call with CART_PLANE_PREDICATE_PLANEFIT");
    const Geometry &g = pf->g;
    if (check_pitched(Extent::image("labels", labels, labels_step, 2, g.w, g.h))) return -1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*pf, stream);
    if (call.begin()) return -1;
    PfFitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.labels = labels; a.lstep = labels_step; a.w = g.w; a.h = g.h; a.L1 = pf->last_L1; a.seed = seed; a.frame = frame_id;
    a.cnt = pf->cnt; a.npts = pf->npts; a.start = pf->start; a.err = pf->lp_err; a.pts = pf->pts; a.planes17 = pf->planes17;
    a.state = pf->state; a.local = pf->local; a.accept = pf->accept; a.planes_out = planes; a.assign = assignments; a.nplanes_out = n_planes;
    const int n = launch_pf_fit(a, stream);
    HIP_TRY(hipGetLastError());
    if (launches) *launches = n;
    return 0;
}

int cart_planefit_status(cart_planefit *pf, int *bad_labels) {
    if (!pf || !bad_labels) return fail("bad arguments");
    HIP_TRY(hipSetDevice(pf->device_id));
    std::lock_guard<std::mutex> lk(pf->mu);
    int32_t err = 0;
    if (pf->used) HIP_TRY(hipEventSynchronize(pf->done));
    HIP_TRY(hipMemcpy(&err, pf->err, 4, hipMemcpyDeviceToHost));
    if (err & 2) return fail("internal error: adjacency capacity exceeded");
    *bad_labels = err & 1;
    return 0;
}

int cart_plane_cluster(const double *planes, int max_label, const int32_t *offsets, const int32_t *neighbours, double *planes_out,
                       uint64_t *assignments, int *n_planes) {
    if (!planes || !offsets || !neighbours || !planes_out || !assignments || !n_planes) return fail("NULL pointer");
    if (max_label < 0 || max_label >= kSpMaxLabels) return fail("max_label must be in [0, 16383]");
    const int L1 = max_label + 1;
    if (offsets[0] != 0) return fail("offsets[0] must be 0");
    for (int l = 0; l < L1; ++l)
        if (offsets[l] > offsets[l + 1]) return fail("offsets are not ascending");
    for (int32_t k = offsets[0]; k < offsets[L1]; ++k)
        if (neighbours[k] < 0 || neighbours[k] >= L1) return fail("neighbour label out of range");
    struct Stats { double d, ys, yc, ps, pc; };   // planecluster.cpp:8-17 (the fields the merge reads)
    std::vector<Stats> st(L1);
    std::vector<char> zero(L1);
    for (int l = 0; l < L1; ++l) {
        const double *p = planes + (size_t)l * 4;
        zero[l] = p[0] == 0 && p[1] == 0 && p[2] == 0 && p[3] == 0;
        if (zero[l]) continue;
        const double length = std::sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);   // planecluster.cpp:58-66
        const double yaw = std::atan2(p[1], p[0]), pitch = std::atan2(p[2], length);
        st[l] = Stats{p[3], std::sin(yaw), std::cos(yaw), std::sin(pitch), std::cos(pitch)};
    }
    std::vector<int> seeds;          // seed label of every plane, in order
    std::fill(assignments, assignments + L1, (uint64_t)0);
    std::vector<char> seen(L1);
    std::vector<int> similar;
    std::set<int> frontier;
    for (int l = 0; l < L1; ++l) {   // planecluster.cpp:98-167 with one thread: ascending seeds
        if (assignments[l] != 0 || zero[l]) continue;
        const Stats &s = st[l];
        similar.assign(1, l);
        std::fill(seen.begin(), seen.end(), 0);
        seen[l] = 1;
        frontier.clear();
        frontier.insert(neighbours + offsets[l], neighbours + offsets[l + 1]);
        while (!frontier.empty()) {
            const int o = *frontier.begin();
            frontier.erase(frontier.begin());
            seen[o] = 1;
            if (zero[o]) continue;
            const Stats &t = st[o];
            const double yawd = std::abs(s.ys - t.ys) + std::abs(s.yc - t.yc);
            const double pitchd = std::abs(s.ps - t.ps) + std::abs(s.pc - t.pc);
            const double dd = std::abs(s.d - t.d);
            if (yawd < 0.2 && pitchd < 0.2 && dd < 3) {
                const uint64_t cur = assignments[o];
                if (cur != 0) {   // kept literally: dDiff on both sides (planecluster.cpp:137)
                    const Stats &u = st[seeds[cur - 1]];
                    const double cy = std::abs(u.ys - t.ys) + std::abs(u.yc - t.yc);
                    const double cp = std::abs(u.ps - t.ps) + std::abs(u.pc - t.pc);
                    if (cy + cp + dd < yawd + pitchd + dd) continue;
                }
                similar.push_back(o);
                for (int32_t k = offsets[o]; k < offsets[o + 1]; ++k)
                    if (!seen[neighbours[k]]) frontier.insert(neighbours[k]);
            }
        }
        if (similar.size() < 32) continue;
        seeds.push_back(l);
        for (int q : similar) assignments[q] = seeds.size();
    }
    for (size_t k = 0; k < seeds.size(); ++k)
        for (int j = 0; j < 4; ++j) planes_out[k * 4 + j] = planes[(size_t)seeds[k] * 4 + j];
    *n_planes = (int)seeds.size();
    return 0;
}

}  // extern "C"

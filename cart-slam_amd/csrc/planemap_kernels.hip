// planemap_kernels.hip -- the world-frame bird's-eye plane map (spec S24; C ABI in engine_planemap.hip):
//   plane_map_clear     empties a rectangle of the window (the strips a window move brings in, or the whole grid)
//   plane_map_vote      one frame's votes.  A lane walks kMapStrip rows of one image column and keeps one pending run of equal
//                       (cell, label) keys in registers; when a lane's key changes, the wave merges the pending runs of neighbouring
//                       lanes that hold the same key (compare with the lane below, ballot the run heads, segmented suffix reduction)
//                       and only the run heads issue the global atomics.  Counts, minima and maxima are integers: exact in any order.
//   plane_map_classify  cell -> class
//   plane_store_insert  one frame's pitched disparity + labels -> the packed planes of a store slot (spec S30)
//   plane_map_revote    the votes of many stored frames at once, each through its own pose into one fixed window.  Grid z is the
//                       entry; a lane walks kRevoteStrip rows of one column, kMapStrip rows at a time with the next group's loads in
//                       flight, and keeps ONE pending run open over the whole strip: a wall column costs one flush per tall strip.
//                       vote_key and wave_emit are the per-frame kernel's.
// fp64 with + - * / floor only, in the association order of warp_device.h, which holds the warp chain.

#include "engine_internal.h"
#include "warp_device.h"

namespace cart_amd {

namespace {

__device__ __forceinline__ int map_slot(const PlaneMapGrid &g, int rx, int rz) {
    int sx = rx + g.mx, sz = rz + g.mz;
    if (sx >= g.nx) sx -= g.nx;
    if (sz >= g.nz) sz -= g.nz;
    return sz * g.nx + sx;
}

__global__ __launch_bounds__(256) void plane_map_clear_kernel(PlaneMapGrid g, int rx0, int rw, int rz0, int rh) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rw * rh) return;
    const int slot = map_slot(g, rx0 + i % rw, rz0 + i / rw);
    reinterpret_cast<int4 *>(g.cells)[slot] = make_int4(0, 0, INT32_MAX, INT32_MIN);
}

// S24's gates in their order -> the key 2 * storage slot + label of an accepted in-window pixel, -1 for every other; q for label 1
__device__ __forceinline__ int vote_key(const PlaneMapVoteArgs &a, const double *pose, int x, int y, int s, unsigned l, int &q) {
    if (l > 1u || s == -32768) return -1;
    const double d = (double)s / 16.0;
    if (!(d >= a.p.min_disparity)) return -1;
    const double Z = (a.cam.fx * a.cam.baseline) / d;
    if (!(Z <= a.p.max_depth)) return -1;
    const double X = back_project_x(a.cam, x, Z);
    if (!(X >= -a.p.max_lateral && X <= a.p.max_lateral)) return -1;
    const WarpPoint p{X, back_project_y(a.cam, y, Z), Z};   // Y only after the X gate
    const double Xw = pose_row(pose, 0, p), Zw = pose_row(pose, 2, p);
    const double gx = floor(Xw / a.p.cell_size), gz = floor(Zw / a.p.cell_size);
    if (!(gx >= a.ox && gx < a.ox + (double)a.grid.nx && gz >= a.oz && gz < a.oz + (double)a.grid.nz)) return -1;
    if (l == 1u) {
        const double Yw = pose_row(pose, 1, p);
        double qd = floor(Yw / a.p.height_quantum);
        qd = qd < -1073741824.0 ? -1073741824.0 : (qd > 1073741824.0 ? 1073741824.0 : qd);
        q = (int)qd;
    }
    return 2 * map_slot(a.grid, (int)(gx - a.ox), (int)(gz - a.oz)) + (int)l;
}

// Wave-collective: every lane brings a run (key, cnt, mn, mx) or key = -1.  Neighbouring lanes with the same key form one run, the
// run's head lane gets its totals and issues the atomics.
__device__ __forceinline__ void wave_emit(cart_plane_map_cell *cells, int key, unsigned cnt, int mn, int mx) {
    const int lane = threadIdx.x & 63;
    const int below = __shfl_up(key, 1);
    const bool head = lane == 0 || key != below;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = above ? lane + __ffsll((long long)above) - 1 : 63;   // last lane of this lane's run
    const bool extent = __any(key >= 0 && (key & 1));                     // a vertical run somewhere: min / max are needed
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned c = __shfl_down(cnt, d);
        const bool in = lane + d <= end;
        if (in) cnt += c;
        if (extent) {
            const int lo = __shfl_down(mn, d), hi = __shfl_down(mx, d);
            if (in) { mn = min(mn, lo); mx = max(mx, hi); }
        }
    }
    if (head && key >= 0) {
        cart_plane_map_cell *c = cells + (key >> 1);
        if (key & 1) {
            atomicAdd(&c->vertical, cnt);
            atomicMin(&c->y_min, mn);
            atomicMax(&c->y_max, mx);
        } else {
            atomicAdd(&c->horizontal, cnt);
        }
    }
}

__global__ __launch_bounds__(256) void plane_map_vote_kernel(PlaneMapVoteArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y0 = blockIdx.y * kMapStrip;
    int s[kMapStrip];
    unsigned l[kMapStrip];
#pragma unroll
    for (int r = 0; r < kMapStrip; ++r) {   // every load of the strip before the first use
        const bool in = x < a.w && y0 + r < a.h;
        s[r] = in ? *(reinterpret_cast<const int16_t *>(reinterpret_cast<const uint8_t *>(a.disp) + (size_t)(y0 + r) * a.disp_step) + x) : -32768;
        l[r] = in ? a.planes[(size_t)(y0 + r) * a.planes_step + x] : 2u;
    }
    int run = -1, mn = INT32_MAX, mx = INT32_MIN;
    unsigned cnt = 0;
#pragma unroll
    for (int r = 0; r < kMapStrip; ++r) {
        int q = 0;
        const int key = vote_key(a, a.pose, x, y0 + r, s[r], l[r], q);
        const bool flush = key >= 0 && run >= 0 && key != run;   // a rejected pixel leaves the pending run open
        if (__any(flush)) wave_emit(a.grid.cells, flush ? run : -1, cnt, mn, mx);
        if (flush) { cnt = 0; mn = INT32_MAX; mx = INT32_MIN; }
        if (key >= 0) {
            run = key;
            ++cnt;
            if (key & 1) { mn = min(mn, q); mx = max(mx, q); }
        }
    }
    if (__any(run >= 0)) wave_emit(a.grid.cells, run, cnt, mn, mx);
}

__global__ __launch_bounds__(256) void plane_store_insert_kernel(const int16_t *__restrict__ disp, size_t disp_step, const uint8_t *__restrict__ planes, size_t planes_step,
                                                                 int16_t *__restrict__ dst_disp, uint8_t *__restrict__ dst_planes, int w) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;   // a workgroup per 256 pixels of one row: a KITTI frame is 1875 of them
    if (x >= w) return;
    dst_disp[(size_t)y * w + x] = row_ptr(disp, disp_step, y)[x];
    dst_planes[(size_t)y * w + x] = row_ptr(planes, planes_step, y)[x];
}

// kMapStrip rows of column x from the packed planes of one stored frame; rows and columns outside the image carry a rejected pixel
__device__ __forceinline__ void revote_load(const int16_t *disp, const uint8_t *planes, int w, int h, int x, int y0, int (&s)[kMapStrip], unsigned (&l)[kMapStrip]) {
#pragma unroll
    for (int r = 0; r < kMapStrip; ++r) {
        const bool in = x < w && y0 + r < h;
        const size_t at = (size_t)(y0 + r) * w + x;
        s[r] = in ? disp[at] : -32768;
        l[r] = in ? planes[at] : 2u;
    }
}

__global__ __launch_bounds__(256) void plane_map_revote_kernel(PlaneMapVoteArgs a, const PlaneRevoteRecord *__restrict__ records) {
    const PlaneRevoteRecord *rec = records + blockIdx.z;
    double pose[12];   // uniform over the workgroup: read once, ahead of every store
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = rec->pose[k];
    const size_t plane = (size_t)a.w * a.h;
    const int16_t *disp = a.disp + (size_t)rec->slot * plane;
    const uint8_t *planes = a.planes + (size_t)rec->slot * plane;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y0 = blockIdx.y * kRevoteStrip;
    const int y1 = min(a.h, y0 + kRevoteStrip);   // uniform: every lane of the wave walks the same groups
    int s[kMapStrip], ns[kMapStrip];
    unsigned l[kMapStrip], nl[kMapStrip];
    revote_load(disp, planes, a.w, a.h, x, y0, s, l);
    int run = -1, mn = INT32_MAX, mx = INT32_MIN;
    unsigned cnt = 0;
#pragma unroll 1
    for (int yg = y0; yg < y1; yg += kMapStrip) {
        if (yg + kMapStrip < y1) revote_load(disp, planes, a.w, a.h, x, yg + kMapStrip, ns, nl);   // the next group, before this one is consumed
#pragma unroll
        for (int r = 0; r < kMapStrip; ++r) {
            int q = 0;
            const int key = vote_key(a, pose, x, yg + r, s[r], l[r], q);
            const bool flush = key >= 0 && run >= 0 && key != run;   // a rejected pixel leaves the pending run open
            if (__any(flush)) wave_emit(a.grid.cells, flush ? run : -1, cnt, mn, mx);
            if (flush) { cnt = 0; mn = INT32_MAX; mx = INT32_MIN; }
            if (key >= 0) {
                run = key;
                ++cnt;
                if (key & 1) { mn = min(mn, q); mx = max(mx, q); }
            }
        }
#pragma unroll
        for (int r = 0; r < kMapStrip; ++r) { s[r] = ns[r]; l[r] = nl[r]; }
    }
    if (__any(run >= 0)) wave_emit(a.grid.cells, run, cnt, mn, mx);
}

__global__ __launch_bounds__(256) void plane_map_classify_kernel(PlaneMapGrid g, int empty, unsigned min_votes, unsigned percent, uint8_t *out, size_t out_step) {
    const int rx = blockIdx.x * 64 + (threadIdx.x & 63), rz = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (rx >= g.nx || rz >= g.nz) return;
    uint8_t cls = 2;
    if (!empty) {
        const int4 c = reinterpret_cast<const int4 *>(g.cells)[map_slot(g, rx, rz)];
        const unsigned long long h = (unsigned)c.x, v = (unsigned)c.y, n = h + v;
        if (n >= min_votes) cls = v * 100ull >= (unsigned long long)percent * n ? 1 : 0;
    }
    out[(size_t)rz * out_step + rx] = cls;
}

}  // namespace

void launch_plane_map_clear(const PlaneMapGrid &grid, int rx0, int rw, int rz0, int rh, hipStream_t s) {
    if (rw <= 0 || rh <= 0) return;
    hipLaunchKernelGGL(plane_map_clear_kernel, dim3((unsigned)((rw * rh + 255) / 256)), dim3(256), 0, s, grid, rx0, rw, rz0, rh);
}

void launch_plane_map_vote(const PlaneMapVoteArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(plane_map_vote_kernel, dim3((unsigned)((a.w + 255) / 256), (unsigned)((a.h + kMapStrip - 1) / kMapStrip)), dim3(256), 0, s, a);
}

void launch_plane_store_insert(const int16_t *disp, size_t disp_step, const uint8_t *planes, size_t planes_step, int16_t *dst_disp, uint8_t *dst_planes, int w, int h,
                               hipStream_t s) {
    hipLaunchKernelGGL(plane_store_insert_kernel, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, s, disp, disp_step, planes, planes_step, dst_disp,
                       dst_planes, w);
}

void launch_plane_map_revote(const PlaneMapVoteArgs &a, const PlaneRevoteRecord *records, int entries, hipStream_t s) {
    if (entries <= 0) return;
    hipLaunchKernelGGL(plane_map_revote_kernel, dim3((unsigned)((a.w + 255) / 256), (unsigned)((a.h + kRevoteStrip - 1) / kRevoteStrip), (unsigned)entries), dim3(256), 0, s,
                       a, records);
}

void launch_plane_map_classify(const PlaneMapGrid &grid, int empty, unsigned min_votes, unsigned percent, uint8_t *out, size_t out_step, hipStream_t s) {
    hipLaunchKernelGGL(plane_map_classify_kernel, dim3((unsigned)((grid.nx + 63) / 64), (unsigned)((grid.nz + 3) / 4)), dim3(256), 0, s, grid, empty, min_votes,
                       percent, out, out_step);
}

}  // namespace cart_amd

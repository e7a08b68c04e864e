// voxel_rebuild_kernels.hip -- the TSDF volume rebuilt from stored keyframes (spec S35; C ABI in engine_voxelmap.hip):
//   voxel_rebuild    every used entry of the list into one fixed window, in list order, in one launch.  The workgroup shape is
//                    voxel_integrate_kernel's (lanes along x, 64 x 4 voxels per slice, kVoxelSlices voxels of a lane at a time), but a
//                    lane owns its voxels for the whole rebuild: (t, w) start at (0, 0) in registers, the lane walks the entries in order,
//                    and the word is stored once at the end.  The volume is never read, so no clear precedes the launch, and there is one
//                    ticket per workgroup for the whole call.  The entry records are uniform over the grid and travel through scalar loads.
//                    An entry whose frustum cannot reach the group's 64 x 4 x kVoxelSlices box is skipped (six linear functionals of q over
//                    the box, conservative: CART_VOXEL_REBUILD_CULL).
// The gates are S33's (voxelmap_kernels.hip, voxel_integrate_kernel), value for value: fp64 with + - * / floor only, in the association
// order of warp_device.h.  Two rearrangements, neither of which can change a bit:
//   - p_a = ((double)g_a + 0.5) voxel_size does not depend on the entry and is computed once per group; d = p - t is still its own rounding;
//   - gate 6 in 32 bits: 2 (w t + obs) + (w + 1) = 2 (w + 1) t + (2 (obs - t) + (w + 1)), so t' = t + floor_div(2 (obs - t) + (w + 1),
//     2 (w + 1)) exactly, and |2 (obs - t) + (w + 1)| < 2^18.
// A voxel that failed gate 1 or 2 carries the invalid disparity -32768 into gate 3, which fails it.  No atomic on the volume.

#include "engine_internal.h"
#include "warp_device.h"

// The three choices below were taken by measurement (profiles/voxel_rebuild.txt); the other forms stay behind their macros
// as the record of the A/B.  None of them can change a byte.
#ifndef CART_VOXEL_REBUILD_PREFETCH
#define CART_VOXEL_REBUILD_PREFETCH 0   // 1: the image loads of entry k + 1 are issued before gates 3 to 6 of entry k are consumed.  14 more VGPRs,
#endif                                  // 5 waves per SIMD in place of 7, and 2 to 3 % slower: the waves hide the loads better than the pipeline
#ifndef CART_VOXEL_REBUILD_DEPTH
#define CART_VOXEL_REBUILD_DEPTH 4      // z slices per workgroup.  The integrate's 16 (CART_VOXEL_DEPTH) saves tickets, and a rebuild has one ticket
#endif                                  // per workgroup whatever the depth; four times the workgroups balance the uneven work: 27 % faster than 16
#ifndef CART_VOXEL_REBUILD_CULL
#define CART_VOXEL_REBUILD_CULL 1       // an entry whose frustum cannot reach the group's box is skipped: level where every entry sees the window,
#endif                                  // 1.7 times faster at 256 entries along a path

namespace cart_amd {

namespace {

constexpr int kRebuildDepth = CART_VOXEL_REBUILD_DEPTH;
static_assert(kRebuildDepth % kVoxelSlices == 0, "a workgroup walks whole groups of slices");

__device__ __forceinline__ int wrap(int v, int n) { return v >= n ? v - n : v; }

struct RebuildPending {                 // what gates 1 and 2 of one entry leave for gates 3 to 6, per slice
    int s[kVoxelSlices];                // the disparity word, -32768 where gate 1 or 2 failed
    unsigned m[kVoxelSlices];           // the u8 plane, 0 where it is not read
    double qz[kVoxelSlices];
};

#if CART_VOXEL_REBUILD_CULL
// voxel_box_culled of voxelmap_kernels.hip for one entry: b = the box's base corner minus t, e = its three edges.  True only if no voxel of
// the box can pass gates 1, 2 and 4 (six linear functionals of q over the box, with a million times their rounding error as slack).
__device__ __forceinline__ double dabs(double v) { return v < 0.0 ? -v : v; }
__device__ __forceinline__ bool rebuild_box_culled(const VoxelRebuildArgs &a, const double *P, const double (&b)[3], const double (&e)[3]) {
    const double slack = 1e-8 * (1.0 + dabs(b[0]) + dabs(b[1]) + dabs(b[2]) + e[0] + e[1] + e[2] + dabs(P[3]) + dabs(P[7]) + dabs(P[11]));
    const double fxb = a.cam.fx * a.cam.baseline;
    const double zfar = (a.p.max_depth + (a.p.truncation + a.p.disparity_sigma * ((a.p.max_depth * a.p.max_depth) / fxb))) * (1.0 + 1e-9);
    const double kx[6] = {0.0, a.cam.fx, 0.0, 0.0, a.cam.fx, 0.0};
    const double ky[6] = {0.0, 0.0, a.cam.fy, 0.0, 0.0, a.cam.fy};
    const double kz[6] = {1.0, a.cam.cx + 0.5, a.cam.cy + 0.5, 1.0, a.cam.cx - ((double)a.w - 0.5), a.cam.cy - ((double)a.h - 0.5)};
    const double bound[6] = {a.p.min_depth, 0.0, 0.0, zfar, 0.0, 0.0};
    const double scale[6] = {1.0, a.cam.fx + dabs(a.cam.cx) + 1.0, a.cam.fy + dabs(a.cam.cy) + 1.0, 1.0, a.cam.fx + dabs(a.cam.cx) + (double)a.w,
                             a.cam.fy + dabs(a.cam.cy) + (double)a.h};
    bool culled = false;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        double lo = 0.0, hi = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double c = (kx[f] * P[4 * r] + ky[f] * P[4 * r + 1]) + kz[f] * P[4 * r + 2];
            const double at = c * b[r], edge = c * e[r];
            lo += at + (edge < 0.0 ? edge : 0.0);
            hi += at + (edge > 0.0 ? edge : 0.0);
        }
        const double s = 8.0 * slack * scale[f];
        culled = culled || (f < 3 ? hi + s < bound[f] : lo - s > bound[f]);
    }
    return culled;
}
#endif

// Gates 1 and 2 of one entry for the lane's kVoxelSlices voxels at (px, py, pz[k]), and the image loads of those that got this far.
__device__ __forceinline__ void rebuild_fetch(const VoxelRebuildArgs &a, const PlaneRevoteRecord *__restrict__ rec, bool in, double px, double py,
                                              const double (&pz)[kVoxelSlices], const double (&box)[3], const double (&edge)[3], RebuildPending &n) {
    double P[12];                             // uniform over the grid
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = rec->pose[k];
    const size_t at0 = (size_t)rec->slot * ((size_t)a.w * a.h);
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) { n.s[k] = -32768; n.m[k] = 0u; n.qz[k] = 0.0; }
#if CART_VOXEL_REBUILD_CULL
    const double b[3] = {box[0] - P[3], box[1] - P[7], box[2] - P[11]};
    if (rebuild_box_culled(a, P, b, edge)) return;   // uniform over the workgroup
#endif
    if (!in) return;
    const double d0 = px - P[3], d1 = py - P[7];
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        const double d2 = pz[k] - P[11];
        WarpPoint q;
        q.x = (P[0] * d0 + P[4] * d1) + P[8] * d2;
        q.y = (P[1] * d0 + P[5] * d1) + P[9] * d2;
        q.z = (P[2] * d0 + P[6] * d1) + P[10] * d2;
        if (!(q.z >= a.p.min_depth)) continue;
        const double xd = floor(project_u(a.cam, q) + 0.5), yd = floor(project_v(a.cam, q) + 0.5);
        if (!(xd >= 0.0 && xd <= (double)(a.w - 1) && yd >= 0.0 && yd <= (double)(a.h - 1))) continue;   // a NaN fails
        const size_t at = at0 + ((size_t)(int)yd * a.w + (size_t)(int)xd);
        n.s[k] = a.disp[at];
        if (a.planes) n.m[k] = a.planes[at];
        n.qz[k] = q.z;
    }
}

// Gates 3 to 6 of one entry on the registers (t, w) of the lane's voxels.
__device__ __forceinline__ void rebuild_consume(const VoxelRebuildArgs &a, double fxb, const RebuildPending &n, int (&t)[kVoxelSlices], int (&w)[kVoxelSlices],
                                                unsigned &n_updated, unsigned &n_near) {
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        if (n.s[k] == -32768) continue;
        const double d = (double)n.s[k] / 16.0;
        if (!(d >= a.p.min_disparity)) continue;
        const double Z = fxb / d;
        if (!(Z <= a.p.max_depth) || n.m[k] == 1u) continue;
        const double tr = a.p.truncation + a.p.disparity_sigma * ((Z * Z) / fxb);
        const double sdf = Z - n.qz[k];
        if (!(sdf >= -tr)) continue;
        double f = sdf / tr;
        n_near += f < 1.0 ? 1u : 0u;
        if (f > 1.0) f = 1.0;
        const int obs = (int)floor(f * 32767.0 + 0.5);
        const int num = 2 * (obs - t[k]) + (w[k] + 1), den = 2 * (w[k] + 1);
        t[k] += num / den - ((num % den != 0) && (num < 0));   // floor division, den > 0
        w[k] = w[k] + 1 < a.p.max_weight ? w[k] + 1 : a.p.max_weight;
        n_updated += 1u;
    }
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;                                 // in lane 0
}

__global__ __launch_bounds__(256) void voxel_rebuild_kernel(VoxelRebuildArgs a, const PlaneRevoteRecord *__restrict__ records) {
    __shared__ unsigned wave_counts[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rx = blockIdx.x * 64 + lane, ry = blockIdx.y * 4 + wave;
    const bool in = rx < a.grid.nx;           // ny is a multiple of 8: no guard on y
    const double fxb = a.cam.fx * a.cam.baseline;
    const double vs = a.p.voxel_size;
    const double px = ((a.grid.ox + (double)rx) + 0.5) * vs, py = ((a.grid.oy + (double)ry) + 0.5) * vs;
    unsigned n_updated = 0, n_near = 0;       // at most kRebuildDepth x 4096 per lane
    // kRebuildDepth slices of z per workgroup, kVoxelSlices at a time; nz is a multiple of kVoxelSlices, so a group of slices is inside or outside whole
#pragma unroll 1
    for (int rz0 = blockIdx.z * kRebuildDepth; rz0 < min((int)(blockIdx.z + 1) * kRebuildDepth, a.grid.nz); rz0 += kVoxelSlices) {
        double pz[kVoxelSlices];
#pragma unroll
        for (int k = 0; k < kVoxelSlices; ++k) pz[k] = ((a.grid.oz + (double)(rz0 + k)) + 0.5) * vs;
        // the group's box for the cull: its base corner and its edges
        const int bx0 = (int)blockIdx.x * 64, bx1 = min(bx0 + 63, a.grid.nx - 1);
        const double box[3] = {((a.grid.ox + (double)bx0) + 0.5) * vs, ((a.grid.oy + (double)((int)blockIdx.y * 4)) + 0.5) * vs, pz[0]};
        const double edge[3] = {(double)(bx1 - bx0) * vs, 3.0 * vs, (double)(kVoxelSlices - 1) * vs};
        int t[kVoxelSlices], w[kVoxelSlices];
#pragma unroll
        for (int k = 0; k < kVoxelSlices; ++k) { t[k] = 0; w[k] = 0; }
#if CART_VOXEL_REBUILD_PREFETCH
        RebuildPending cur, nxt;
        if (a.entries > 0) rebuild_fetch(a, records, in, px, py, pz, box, edge, cur);
        nxt = cur;
#pragma unroll 1
        for (int e = 0; e < a.entries; ++e) {
            if (e + 1 < a.entries) rebuild_fetch(a, records + (e + 1), in, px, py, pz, box, edge, nxt);   // the next entry's loads, before this one is consumed
            rebuild_consume(a, fxb, cur, t, w, n_updated, n_near);
            cur = nxt;
        }
#else
#pragma unroll 1
        for (int e = 0; e < a.entries; ++e) {
            RebuildPending cur;
            rebuild_fetch(a, records + e, in, px, py, pz, box, edge, cur);
            rebuild_consume(a, fxb, cur, t, w, n_updated, n_near);
        }
#endif
        if (in) {
#pragma unroll
            for (int k = 0; k < kVoxelSlices; ++k) {
                const size_t slot = ((size_t)wrap(rz0 + k + a.grid.mz, a.grid.nz) * a.grid.ny + wrap(ry + a.grid.my, a.grid.ny)) * a.grid.nx + wrap(rx + a.grid.mx, a.grid.nx);
                a.grid.voxels[slot] = ((uint32_t)(uint16_t)(int16_t)t[k]) | ((uint32_t)w[k] << 16);
            }
        }
    }                                         // the groups of slices
    if (!a.counts) return;                    // uniform over the grid
    n_updated = wave_sum(n_updated);
    n_near = wave_sum(n_near);
    if (lane == 0) { wave_counts[wave][0] = n_updated; wave_counts[wave][1] = n_near; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long u = (unsigned long long)wave_counts[0][0] + wave_counts[1][0] + wave_counts[2][0] + wave_counts[3][0];
        const unsigned long long n = (unsigned long long)wave_counts[0][1] + wave_counts[1][1] + wave_counts[2][1] + wave_counts[3][1];
        // the map's counter block, uint64 words 4 to 6: the two sums and the ticket; the workgroup with the last ticket hands the sums over
        // and zeroes the words again (as hand_over of voxelmap_kernels.hip, with whole words for the sums: they pass 2^32)
        unsigned long long *c = reinterpret_cast<unsigned long long *>(a.counters) + 4;
        if (u) atomicAdd(c + 0, u);
        if (n) atomicAdd(c + 1, n);
        __threadfence();                      // this workgroup's additions before its ticket
        const unsigned long long before = atomicAdd(c + 2, 1ull);
        if (before == (unsigned long long)gridDim.x * gridDim.y * gridDim.z - 1ull) {
            __threadfence();                  // the last workgroup: every other one's additions are visible
            a.counts[0] = (long long)atomicExch(c + 0, 0ull);
            a.counts[1] = (long long)atomicExch(c + 1, 0ull);
            atomicExch(c + 2, 0ull);
        }
    }
}

}  // namespace

void launch_voxel_rebuild(const VoxelRebuildArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(voxel_rebuild_kernel, dim3((unsigned)((a.grid.nx + 63) / 64), (unsigned)(a.grid.ny / 4), (unsigned)((a.grid.nz + kRebuildDepth - 1) / kRebuildDepth)), dim3(256), 0, s,
                       a, a.records);
}

}  // namespace cart_amd

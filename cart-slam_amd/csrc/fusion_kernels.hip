// fusion_kernels.hip -- temporal disparity fusion through ego-motion (spec S28; C ABI in engine_fusion.hip):
//   fusion_splat  per previous pixel: the point it saw, carried through the relative pose and projected into this frame, writes its key
//                 to the up to 2 x 2 pixels within splat_radius by an integer atomicMax into the z-buffer.  A lane takes kFusionStrip rows
//                 of one column and issues the loads of its pixels (disparity, age, mask) together, then the arithmetic.  Neighbouring
//                 lanes of a row mostly hit overlapping targets (lane i's second column is lane i + 1's first): with CART_FUSION_MERGE
//                 a lane takes over the key its upper neighbour would send to the same address, so that pair costs one atomic.
//   fusion_fuse   per current pixel: the z-buffer key against this frame's disparity -> fused, age, source.  A lane takes kFusionRows rows of
//                 one column.  It writes back the zero it found the z-buffer in (the buffer is all zero between calls, no clear launch) and
//                 counts the source classes by wave ballots; a workgroup adds its counts to the object's counters in three 64-bit integer
//                 atomics, and the workgroup that finishes last moves those to the caller's `counts` and zeroes them again.
// fp64 with + - * / floor only, in the association order of warp_device.h, which holds the warp chain.
// The only atomics are integer maxima and additions: the result cannot depend on execution order.

#include "engine_internal.h"
#include "warp_device.h"

namespace cart_amd {

namespace {

__device__ __forceinline__ double dabs(double v) { return v < 0.0 ? -v : v; }

// The targets of one source: tx / ty hold the up to two columns / rows inside the image (-1: none), key[i][j] the key for (tx[i], ty[j]).
__device__ __forceinline__ void splat_targets(const FusionArgs &a, int xp, int yp, int s, unsigned age, unsigned mask, int tx[2], int ty[2], unsigned key[2][2]) {
    tx[0] = tx[1] = ty[0] = ty[1] = -1;
    key[0][0] = key[0][1] = key[1][0] = key[1][1] = 0u;
    const double dp = (double)s / 16.0;
    if (age < 1u || s == -32768 || !(dp >= a.p.min_disparity) || mask == 1u) return;
    const double fxb = a.cam.fx * a.cam.baseline;
    const WarpPoint q = pose_carry(a.rel, back_project(a.cam, fxb, xp, yp, dp));
    if (!(q.z > 0)) return;
    const double u = project_u(a.cam, q), v = project_v(a.cam, q);
    const double swd = floor((fxb / q.z) * 16.0 + 0.5);
    if (!(swd >= 1.0 && swd <= 32767.0)) return;
    const unsigned sw = (unsigned)(int)swd;
    const double r = a.p.splat_radius;
    const double cd[2] = {-floor(-(u - r)), floor(u + r)}, rd[2] = {-floor(-(v - r)), floor(v + r)};
    double du[2], dv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {   // the second of two equal targets is dropped, and both when the first lies beyond the second
        const bool cok = cd[0] <= cd[1] && (i == 0 || cd[1] != cd[0]) && cd[i] >= 0.0 && cd[i] <= (double)(a.w - 1);
        const bool rok = rd[0] <= rd[1] && (i == 0 || rd[1] != rd[0]) && rd[i] >= 0.0 && rd[i] <= (double)(a.h - 1);
        tx[i] = cok ? (int)cd[i] : -1;
        ty[i] = rok ? (int)rd[i] : -1;
        du[i] = dabs(cd[i] - u);
        dv[i] = dabs(rd[i] - v);
    }
    const unsigned base = ((sw >> 4) << 16) | ((sw & 15u) << 8) | age;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (tx[i] < 0 || ty[j] < 0) continue;
            const double f = floor(16.0 * (du[i] > dv[j] ? du[i] : dv[j]));   // in [0, 16): both distances are at most splat_radius < 1
            const unsigned c = 15u - (f < 15.0 ? (unsigned)(int)f : 15u);
            key[i][j] = base | (c << 12);
        }
}

__global__ __launch_bounds__(256) void fusion_splat_kernel(FusionArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y0 = blockIdx.y * kFusionStrip;
    int sp[kFusionStrip];
    unsigned ap[kFusionStrip], mp[kFusionStrip];
#pragma unroll
    for (int r = 0; r < kFusionStrip; ++r) {   // every load of the strip before the first use
        const bool in = x < a.w && y0 + r < a.h;
        sp[r] = in ? row_ptr(a.prev_disp, a.prev_disp_step, y0 + r)[x] : -32768;
        ap[r] = in ? row_ptr(a.prev_age, a.prev_age_step, y0 + r)[x] : 0u;
        mp[r] = in && a.mask_prev ? row_ptr(a.mask_prev, a.mask_prev_step, y0 + r)[x] : 0u;
    }
#if CART_FUSION_MERGE
    const int lane = threadIdx.x & 63;
#endif
#pragma unroll
    for (int r = 0; r < kFusionStrip; ++r) {
        int tx[2], ty[2];
        unsigned key[2][2];
        splat_targets(a, x, y0 + r, sp[r], ap[r], mp[r], tx, ty, key);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // -1 = no target; an index is below 2^28 (16384 x 16384)
            int first = tx[0] >= 0 && ty[j] >= 0 ? ty[j] * a.w + tx[0] : -1;
            const int second = tx[1] >= 0 && ty[j] >= 0 ? ty[j] * a.w + tx[1] : -1;
            unsigned k1 = key[1][j];
#if CART_FUSION_MERGE
            // Wave-collective: a lane's second column takes over the key of the lane above's first column when both name one address.
            // Second columns only take and first columns are only taken, so no key travels further than one lane.
            const int up_first = __shfl_down(first, 1);
            const unsigned up_key = __shfl_down(key[0][j], 1);
            const int down_second = __shfl_up(second, 1);
            if (lane < 63 && second >= 0 && up_first == second) k1 = up_key > k1 ? up_key : k1;
            if (lane > 0 && first >= 0 && down_second == first) first = -1;
#endif
            if (first >= 0) atomicMax(a.zbuf + first, key[0][j]);
            if (second >= 0) atomicMax(a.zbuf + second, k1);
        }
    }
}

__global__ __launch_bounds__(256) void fusion_fuse_kernel(FusionArgs a) {
    __shared__ unsigned wave_counts[4][5];
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y0 = blockIdx.y * kFusionRows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int sc[kFusionRows];
    unsigned mc[kFusionRows], P[kFusionRows];
#pragma unroll
    for (int r = 0; r < kFusionRows; ++r) {   // every load of the lane's rows before the first use
        const bool in = x < a.w && y0 + r < a.h;
        sc[r] = in ? row_ptr(a.disp_cur, a.disp_cur_step, y0 + r)[x] : -32768;
        mc[r] = in && a.mask_cur ? row_ptr(a.mask_cur, a.mask_cur_step, y0 + r)[x] : 0u;
        P[r] = in && a.prev_disp ? a.zbuf[(size_t)(y0 + r) * a.w + x] : 0u;
    }
    unsigned n[5] = {0u, 0u, 0u, 0u, 0u};     // the wave's pixels per class (the same in every lane)
#pragma unroll
    for (int r = 0; r < kFusionRows; ++r) {
        const bool in = x < a.w && y0 + r < a.h;
        unsigned src = 5u;                    // no class: a lane outside the image
        if (in) {
            if (P[r]) a.zbuf[(size_t)(y0 + r) * a.w + x] = 0u;   // all zero again for the next call
            const unsigned key = mc[r] == 1u ? 0u : P[r];
            const int sw = (int)(((key >> 16) << 4) | ((key >> 8) & 15u)), aw = (int)(key & 255u);
            const bool valid = sc[r] != -32768 && (double)sc[r] / 16.0 >= a.p.min_disparity;
            int fused = sc[r], age = 0;
            src = 0u;
            if (valid) {
                age = 1; src = 1u;
                if (key) {
                    const double e = (double)(sc[r] - sw) / 16.0;
                    if (e * e <= a.p.agree_threshold * a.p.agree_threshold) {
                        const int w = aw < a.p.max_weight ? aw : a.p.max_weight;
                        fused = (w * sw + sc[r] + (w + 1) / 2) / (w + 1);
                        age = aw + 1 < 255 ? aw + 1 : 255;
                        src = 2u;
                    } else {
                        src = 3u;
                    }
                }
            } else if (key && aw >= a.p.min_age) {
                fused = sw; age = aw - 1; src = 4u;
            }
            row_ptr(a.fused, a.fused_step, y0 + r)[x] = (int16_t)fused;
            row_ptr(a.age, a.age_step, y0 + r)[x] = (uint8_t)age;
            if (a.source) row_ptr(a.source, a.source_step, y0 + r)[x] = (uint8_t)src;
        }
        if (a.counts) {
#pragma unroll
            for (unsigned k = 0; k < 5u; ++k) n[k] += (unsigned)__popcll(__ballot(src == k));
        }
    }
    if (!a.counts) return;                    // uniform over the grid
    // One workgroup = three 64-bit additions, whatever its size: the classes in pairs, the last with the workgroup ticket in its upper half
    // (per-wave additions to one address serialise in L2: 26 000 of them cost 0.2 ms at 1242 x 375).
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) wave_counts[wave][k] = n[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) t[k] = (unsigned long long)wave_counts[0][k] + wave_counts[1][k] + wave_counts[2][k] + wave_counts[3][k];
        unsigned long long *c = reinterpret_cast<unsigned long long *>(a.counters);
        if (t[0] | t[1]) atomicAdd(c + 0, t[0] | (t[1] << 32));
        if (t[2] | t[3]) atomicAdd(c + 1, t[2] | (t[3] << 32));
        __threadfence();                      // this workgroup's additions before its ticket
        const unsigned long long before = atomicAdd(c + 2, t[4] | (1ull << 32));
        if ((unsigned)(before >> 32) == gridDim.x * gridDim.y - 1u) {   // the last workgroup: every other one's additions are visible
            __threadfence();
            const unsigned long long c01 = atomicExch(c + 0, 0ull), c23 = atomicExch(c + 1, 0ull), c4 = atomicExch(c + 2, 0ull);
            a.counts[0] = (int32_t)(unsigned)c01; a.counts[1] = (int32_t)(c01 >> 32);
            a.counts[2] = (int32_t)(unsigned)c23; a.counts[3] = (int32_t)(c23 >> 32);
            a.counts[4] = (int32_t)(unsigned)c4;
        }
    }
}

}  // namespace

void launch_fusion_splat(const FusionArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(fusion_splat_kernel, dim3((unsigned)((a.w + 255) / 256), (unsigned)((a.h + kFusionStrip - 1) / kFusionStrip)), dim3(256), 0, s, a);
}

void launch_fusion_fuse(const FusionArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(fusion_fuse_kernel, dim3((unsigned)((a.w + 255) / 256), (unsigned)((a.h + kFusionRows - 1) / kFusionRows)), dim3(256), 0, s, a);
}

}  // namespace cart_amd

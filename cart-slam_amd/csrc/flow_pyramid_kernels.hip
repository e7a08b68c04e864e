// flow_pyramid_kernels.hip -- the kernels of the coarse-to-fine census flow (spec S21) that the single-level
// block match (flow_kernels.hip) does not already have: the 2x2 downsample, the per-pixel-prior refinement search and the 3x3
// median of the flow components.  Level flows travel between the kernels as tight s16 [h][w][2] in whole pixels.
//
// Refinement (the hot path).  Every pixel searches (pu + u, pv + v), |u|, |v| <= r, around its OWN prior, so the lanes of a wave
// test different displacements and block_flow_kernel's exchange of column sums between lanes has nothing to share.  Instead a
// lane keeps its (2B+1)^2 current features in registers and shares the PREVIOUS features between its own candidates: for one v
// and one window row it reads the 2(B+r)+1 previous features that the 2r+1 candidates u of that row touch once, and feeds them
// to all of them -- (2r+1)(2B+1)(2(B+r)+1) LDS reads per pixel instead of (2r+1)^2 (2B+1)^2 (225 against 625 at r = B = 2).
// A workgroup owns a 32x8 tile.  It first reduces the range of its pixels' priors; when the previous-frame window for that range
// fits kRefLdsWords it is staged in LDS with coalesced row reads, otherwise every read goes to global memory (L1 / L2) with a
// bounds check.  Both paths read the same values, so they give the same bits.
#include <climits>

#include "engine_internal.h"

namespace cart_amd {

namespace {
constexpr int RT_W = 32, RT_H = 8;        // refinement tile = 256 threads, one pixel each
constexpr int kRefLdsWords = 4096;        // staged previous-frame window: at most 16 KiB of LDS (priors that differ by ~30 px inside a tile)

__device__ __forceinline__ short2 *flow_px(int16_t *f, int w, int x, int y) { return reinterpret_cast<short2 *>(f) + (size_t)y * w + x; }
__device__ __forceinline__ short2 flow_at(const int16_t *f, int w, int x, int y) { return reinterpret_cast<const short2 *>(f)[(size_t)y * w + x]; }

// the level-0 result also goes to the caller's image, as S10.5
__device__ __forceinline__ void emit_s10_5(int16_t *out32, size_t step, int x, int y, int u, int v) {
    if (!out32) return;
    int16_t *row = reinterpret_cast<int16_t *>(reinterpret_cast<uint8_t *>(out32) + (size_t)y * step);
    *reinterpret_cast<short2 *>(row + 2 * x) = make_short2((short)(u * 32), (short)(v * 32));
}
}  // namespace

// ---- level l -> level l + 1 of both frames (blockIdx.z = frame) ----
__global__ __launch_bounds__(256) void flow_downsample_kernel(const uint8_t *src_c, const uint8_t *src_p, int sw, int sh, uint8_t *dst_c,
                                                              uint8_t *dst_p, int dw, int dh) {
    const uint8_t *src = blockIdx.z ? src_p : src_c;
    uint8_t *dst = blockIdx.z ? dst_p : dst_c;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    const int x0 = 2 * x, x1 = min(2 * x + 1, sw - 1), y0 = 2 * y, y1 = min(2 * y + 1, sh - 1);
    const unsigned s = src[(size_t)y0 * sw + x0] + src[(size_t)y0 * sw + x1] + src[(size_t)y1 * sw + x0] + src[(size_t)y1 * sw + x1];
    dst[(size_t)y * dw + x] = (uint8_t)((s + 2) >> 2);
}

void launch_flow_downsample(const uint8_t *src_c, const uint8_t *src_p, int sw, int sh, uint8_t *dst_c, uint8_t *dst_p, hipStream_t s) {
    const int dw = (sw + 1) >> 1, dh = (sh + 1) >> 1;
    hipLaunchKernelGGL(flow_downsample_kernel, dim3((dw + 63) / 64, (dh + 3) / 4, 2), dim3(256), 0, s, src_c, src_p, sw, sh, dst_c, dst_p, dw, dh);
}

// ---- refinement of level l from the flow of level l + 1 ----
template <int B, int R>
__global__ __launch_bounds__(256) void flow_refine_kernel(const uint32_t *cen_cur, const uint32_t *cen_prev, int cpitch, int cpadl, int w, int h,
                                                          const int16_t *coarse, int cw, int force_gather, int16_t *flow, int16_t *out32,
                                                          size_t out32_step) {
    constexpr int WIN = 2 * B + 1, SPAN = 2 * (B + R) + 1, CW = RT_W + 2 * B, CH = RT_H + 2 * B;
    __shared__ uint32_t s_cur[CH * CW];   // tile position (ty, tx) = image (y0 - B + ty, x0 - B + tx); 0 outside the image
    __shared__ int s_range[4];            // min pu, max pu, min pv, max pv over the tile's pixels
    extern __shared__ uint32_t s_prev[];  // [ph][pw] from image (oy, ox) when the window is staged
    const int tid = threadIdx.x, lx = tid & (RT_W - 1), ly = tid / RT_W;
    const int x0 = blockIdx.x * RT_W, y0 = blockIdx.y * RT_H, x = x0 + lx, y = y0 + ly;
    const bool live = x < w && y < h;
    if (tid < 4) s_range[tid] = (tid & 1) ? INT_MIN : INT_MAX;
    for (int i = tid; i < CH * CW; i += 256) {
        const int ty = i / CW, tx = i - ty * CW;
        const int gx = x0 - B + tx, gy = y0 - B + ty;
        s_cur[i] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? cen_cur[(size_t)gy * cpitch + cpadl + gx] : 0u;
    }
    int pu = 0, pv = 0;
    if (live) {
        const short2 c = flow_at(coarse, cw, x >> 1, y >> 1);   // always inside level l + 1
        pu = 2 * c.x; pv = 2 * c.y;
    }
    __syncthreads();
    if (live) {
        atomicMin(&s_range[0], pu); atomicMax(&s_range[1], pu);
        atomicMin(&s_range[2], pv); atomicMax(&s_range[3], pv);
    }
    __syncthreads();
    // previous-frame positions the tile reads: q - (pu + u, pv + v) over its window positions q, priors and candidates
    const int ox = x0 - B - s_range[1] - R, oy = y0 - B - s_range[3] - R;
    const int pw = RT_W + 2 * (B + R) + (s_range[1] - s_range[0]), ph = RT_H + 2 * (B + R) + (s_range[3] - s_range[2]);
    const bool staged = !force_gather && pw * ph <= kRefLdsWords;   // the same for the whole workgroup
    if (staged) {
        for (int i = tid; i < pw * ph; i += 256) {
            const int ty = i / pw, tx = i - ty * pw;
            const int gx = ox + tx, gy = oy + ty;
            s_prev[i] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? cen_prev[(size_t)gy * cpitch + cpadl + gx] : 0u;
        }
        __syncthreads();
    }
    if (!live) return;

    uint32_t cc[WIN][WIN], mk[WIN][WIN];   // current features of the window; mask = 0 where the position is outside the image
#pragma unroll
    for (int dy = 0; dy < WIN; ++dy)
#pragma unroll
        for (int dx = 0; dx < WIN; ++dx) {
            const int qx = x + dx - B, qy = y + dy - B;
            cc[dy][dx] = s_cur[(ly + dy) * CW + lx + dx];
            mk[dy][dx] = (qx >= 0 && qx < w && qy >= 0 && qy < h) ? 0xffffffffu : 0u;
        }
    // image position of the previous feature under window position (0, 0) for candidate u = +R of row v: (x - B - pu - R, y - B - pv - v)
    const int bx = x - B - pu - R;
    unsigned best = 0xffffffffu, c00 = 0;
    int bu = 0, bv = 0;
#pragma unroll 1
    for (int v = -R; v <= R; ++v) {
        unsigned acc[2 * R + 1];
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) acc[k] = 0;
#pragma unroll
        for (int dy = 0; dy < WIN; ++dy) {
            const int py = y - B - pv - v + dy;
            uint32_t pr[SPAN];   // previous features of row py, columns bx .. bx + SPAN - 1
            if (staged) {
                const uint32_t *row = s_prev + (py - oy) * pw + (bx - ox);
#pragma unroll
                for (int k = 0; k < SPAN; ++k) pr[k] = row[k];
            } else {
                const bool row_in = py >= 0 && py < h;
                const uint32_t *row = cen_prev + (size_t)(row_in ? py : 0) * cpitch + cpadl;
#pragma unroll
                for (int k = 0; k < SPAN; ++k) pr[k] = (row_in && bx + k >= 0 && bx + k < w) ? row[bx + k] : 0u;
            }
            // candidate u reads column qx - pu - u = bx + (R - u) + dx
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k)
#pragma unroll
                for (int dx = 0; dx < WIN; ++dx) acc[k] += (unsigned)__builtin_popcount((cc[dy][dx] ^ pr[2 * R - k + dx]) & mk[dy][dx]);
        }
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {   // u = k - R ascending
            if (acc[k] < best) { best = acc[k]; bu = k - R; bv = v; }
        }
        if (v == 0) c00 = acc[R];
    }
    // S21: the winner starts as the prior and only a strictly smaller cost replaces it
    if (c00 <= best) { bu = 0; bv = 0; }
    const int fu = pu + bu, fv = pv + bv;
    *flow_px(flow, w, x, y) = make_short2((short)fu, (short)fv);
    emit_s10_5(out32, out32_step, x, y, fu, fv);
}

template <int B>
static void launch_refine_b(int r, dim3 grid, hipStream_t s, const uint32_t *cen_cur, const uint32_t *cen_prev, const Geometry &g, const int16_t *coarse,
                            int cw, int force_gather, int16_t *flow, int16_t *out32, size_t out32_step) {
    const size_t lds = (size_t)kRefLdsWords * sizeof(uint32_t);
#define CART_REFINE(RR) \
    hipLaunchKernelGGL((flow_refine_kernel<B, RR>), grid, dim3(256), lds, s, cen_cur, cen_prev, g.cpitch, g.cpadl, g.w, g.h, coarse, cw, force_gather, flow, out32, out32_step)
    switch (r) {
        case 1: CART_REFINE(1); break;
        case 2: CART_REFINE(2); break;
        case 3: CART_REFINE(3); break;
        default: CART_REFINE(4); break;
    }
#undef CART_REFINE
}

void launch_flow_refine(const uint32_t *cen_cur, const uint32_t *cen_prev, const Geometry &g, const int16_t *coarse, int coarse_w, int refine_radius,
                        int block, bool force_gather, int16_t *flow, int16_t *out32, size_t out32_step, hipStream_t s) {
    const dim3 grid((g.w + RT_W - 1) / RT_W, (g.h + RT_H - 1) / RT_H);
    switch (block) {
        case 1: launch_refine_b<1>(refine_radius, grid, s, cen_cur, cen_prev, g, coarse, coarse_w, force_gather, flow, out32, out32_step); break;
        case 2: launch_refine_b<2>(refine_radius, grid, s, cen_cur, cen_prev, g, coarse, coarse_w, force_gather, flow, out32, out32_step); break;
        default: launch_refine_b<3>(refine_radius, grid, s, cen_cur, cen_prev, g, coarse, coarse_w, force_gather, flow, out32, out32_step); break;
    }
}

// ---- 3x3 median of each flow component (the one-pixel border passes through, as in S7); filter = 0 only copies ----
__device__ __forceinline__ void sort2(int &a, int &b) { const int lo = min(a, b); b = max(a, b); a = lo; }
__device__ __forceinline__ int median9(int (&p)[9]) {   // the 19-exchange network
    sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]); sort2(p[0], p[1]); sort2(p[3], p[4]); sort2(p[6], p[7]);
    sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]); sort2(p[0], p[3]); sort2(p[5], p[8]); sort2(p[4], p[7]);
    sort2(p[3], p[6]); sort2(p[1], p[4]); sort2(p[2], p[5]); sort2(p[4], p[7]); sort2(p[4], p[2]); sort2(p[6], p[4]);
    sort2(p[4], p[2]);
    return p[4];
}

__global__ __launch_bounds__(256) void flow_median_kernel(const int16_t *in, int w, int h, int filter, int16_t *out, int16_t *out32, size_t out32_step) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    short2 c = flow_at(in, w, x, y);
    if (filter && x >= 1 && x < w - 1 && y >= 1 && y < h - 1) {
        int pu[9], pv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const short2 n = flow_at(in, w, x + k % 3 - 1, y + k / 3 - 1);
            pu[k] = n.x; pv[k] = n.y;
        }
        c = make_short2((short)median9(pu), (short)median9(pv));
    }
    *flow_px(out, w, x, y) = c;
    emit_s10_5(out32, out32_step, x, y, c.x, c.y);
}

void launch_flow_median(const int16_t *in, int w, int h, bool filter, int16_t *out, int16_t *out32, size_t out32_step, hipStream_t s) {
    hipLaunchKernelGGL(flow_median_kernel, dim3((w + 63) / 64, (h + 3) / 4), dim3(256), 0, s, in, w, h, filter ? 1 : 0, out, out32, out32_step);
}

}  // namespace cart_amd

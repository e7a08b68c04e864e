// sgm_post.hip -- post stage of the SGM core: 3x3 medians, left-right check, range fix (stage overview: sgm_census.hip).
#include <cstdlib>

#include "sgm_device.h"

namespace cart_amd {

// ------------------------------------------------------------------ median x2 + LR check + range fix
// Median of 9 from sorted columns: with every 3-element column sorted into (lo, mid, hi),
//   median9 = med3( max3(lo0, lo1, lo2), med3(mid0, mid1, mid2), min3(hi0, hi1, hi2) ).
// A column costs three instructions (v_min3 / v_med3 / v_max3), a median four more, and adjacent pixels share columns.
__device__ __forceinline__ uint32_t med3u(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
struct SortedCol { uint32_t lo, mid, hi; };
__device__ __forceinline__ SortedCol sort_col(uint32_t a, uint32_t b, uint32_t c) {
    return SortedCol{min(min(a, b), c), med3u(a, b, c), max(max(a, b), c)};
}
__device__ __forceinline__ uint32_t median_cols(const SortedCol &c0, const SortedCol &c1, const SortedCol &c2) {
    return med3u(max(max(c0.lo, c1.lo), c2.lo), med3u(c0.mid, c1.mid, c2.mid), min(min(c0.hi, c1.hi), c2.hi));
}

// S7 median of the packed right view (low 16 bits) at (x, y); the image border keeps its own value -- or, with the S7 variant
// (CART_OPT_SPEC_S7_REPLICATE_BORDER), is filtered over the replicated border like every other pixel
__device__ __forceinline__ uint32_t right_median_at(const uint32_t *img, int x, int y, int w, int h, bool replicate) {
    const uint32_t *p = img + (size_t)y * w + x;
    if (x < 1 || x >= w - 1 || y < 1 || y >= h - 1) {
        if (!replicate) return p[0] & 0xffffu;
        SortedCol c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t *q = img + min(max(x + k - 1, 0), w - 1);
            c[k] = sort_col(q[(size_t)max(y - 1, 0) * w] & 0xffffu, q[(size_t)y * w] & 0xffffu, q[(size_t)min(y + 1, h - 1) * w] & 0xffffu);
        }
        return median_cols(c[0], c[1], c[2]);
    }
    SortedCol c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = sort_col(p[k - 1 - w] & 0xffffu, p[k - 1] & 0xffffu, p[k - 1 + w] & 0xffffu);
    return median_cols(c[0], c[1], c[2]);
}

// S7 median of the left WTA map at (x, y); border as above
__device__ __forceinline__ uint32_t left_median_at(const uint16_t *img, int x, int y, int w, int h, bool replicate) {
    const uint16_t *p = img + (size_t)y * w + x;
    if (x < 1 || x >= w - 1 || y < 1 || y >= h - 1) {
        if (!replicate) return p[0];
        SortedCol c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint16_t *q = img + min(max(x + k - 1, 0), w - 1);
            c[k] = sort_col(q[(size_t)max(y - 1, 0) * w], q[(size_t)y * w], q[(size_t)min(y + 1, h - 1) * w]);
        }
        return median_cols(c[0], c[1], c[2]);
    }
    SortedCol c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = sort_col(p[k - 1 - w], p[k - 1], p[k - 1 + w]);
    return median_cols(c[0], c[1], c[2]);
}

// One pixel per thread: the right-view median is a gather at x - d, so the launch wants as many independent threads as
// it can get (four pixels per thread with shared left columns measured 50 % slower).
// spec: bit 0 = S8 variant (integer disparity 0 is invalid too), bit 1 = S7 variant (replicated-border medians); 0 = oracle S7 / S8
__device__ __forceinline__ int post_value(const uint16_t *wl, const uint32_t *rp, const uint8_t *gray, int x, int y, const Geometry &g, int spec) {
    const bool replicate = (spec & 2) != 0;
    const uint32_t ml = left_median_at(wl, x, y, g.w, g.h, replicate);
    bool invalid = gray[(size_t)y * g.w + x] == 0 || ml == kWtaInvalid || ((spec & 1) && (ml >> 4) == 0);
    if (!invalid) {
        const int d = (int)(ml >> 4);
        const int k = x - d;
        if (k >= 0 && k < g.w) {
            const int mr = (int)right_median_at(rp, k, y, g.w, g.h, replicate);
            if (abs(mr - d) > 1) invalid = true;
        }
    }
    return invalid ? (g.min_disp - 1) * 16 : (int)ml + g.min_disp * 16;
}

__global__ __launch_bounds__(256) void post_kernel(const uint16_t *wta_l, const uint32_t *right_pk,
                                                   const uint8_t *gray_l, OutBatch out, Geometry g, int spec) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, frame = blockIdx.z;
    if (x >= g.w || y >= g.h) return;
    const int v = post_value(wta_l + (size_t)frame * g.npx, right_pk + (size_t)frame * g.npx, gray_l + (size_t)frame * g.npx, x, y, g, spec);
    uint8_t *obase = out.scattered ? reinterpret_cast<uint8_t *>(out.frames[frame]) : reinterpret_cast<uint8_t *>(out.ptr) + (size_t)frame * out.frame_stride;
    reinterpret_cast<int16_t *>(obase + (size_t)y * out.step)[x] = (int16_t)v;
}

// post_kernel + the first Jacobi pass of disparity::interpolate at radius 2 (interpolateKernel, interpolation.cu:17-82: the 3 x 3 window mean of
// the values inside (min_disp16, max_disp), count > r*r + 1 -- post_kernels.hip, interpolate_r2_kernel) in one launch: a workgroup computes the post
// values of its 64 x 16 tile and a one-pixel halo into LDS (66 x 18: 16 % more post work) and smooths from there, so the intermediate image is never
// written and the step has one launch less.  Out-of-image halo cells hold a value below every valid range (skipped like the reference's
// out-of-image taps).  Same bits as the two launches (tests: every disparity comparison with smoothing_radius = 2).
constexpr int PI_W = 64, PI_H = 16, PI_LW = PI_W + 2, PI_LH = PI_H + 2, PI_PITCH = 68;
__global__ __launch_bounds__(256) void post_interp_kernel(const uint16_t *wta_l, const uint32_t *right_pk, const uint8_t *gray_l, OutBatch out, Geometry g,
                                                          int spec, int min_disp16, int max_disp) {
    __shared__ int16_t tile[PI_LH][PI_PITCH];
    const int x0 = blockIdx.x * PI_W, y0 = blockIdx.y * PI_H, frame = blockIdx.z, tid = threadIdx.x;
    const uint16_t *wl = wta_l + (size_t)frame * g.npx;
    const uint32_t *rp = right_pk + (size_t)frame * g.npx;
    const uint8_t *gray = gray_l + (size_t)frame * g.npx;
    for (int i = tid; i < PI_LH * PI_LW; i += 256) {
        const int ty = i / PI_LW, tx = i - ty * PI_LW;
        const int x = x0 - 1 + tx, y = y0 - 1 + ty;
        int v = -32768;   // outside the image: never inside (min_disp16, max_disp) -- min_disp16 >= 0
        if (x >= 0 && x < g.w && y >= 0 && y < g.h) v = post_value(wl, rp, gray, x, y, g, spec);
        tile[ty][tx] = (int16_t)v;
    }
    __syncthreads();
    // thread -> 4 adjacent pixels of one row: tile columns 4 q + 1 .. 4 q + 4 of tile row r + 1
    const int q = tid & 15, r = tid >> 4;
    const int xb = x0 + 4 * q, y = y0 + r;
    if (xb >= g.w || y >= g.h) return;
    int csum[6], ccnt[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { csum[c] = 0; ccnt[c] = 0; }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const int v = tile[r + l][4 * q + c];
            if (v > min_disp16 && v < max_disp) { csum[c] += v; ++ccnt[c]; }
        }
    }
    uint8_t *obase = out.scattered ? reinterpret_cast<uint8_t *>(out.frames[frame]) : reinterpret_cast<uint8_t *>(out.ptr) + (size_t)frame * out.frame_stride;
    int16_t *orow = reinterpret_cast<int16_t *>(obase + (size_t)y * out.step);
    int16_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sum = csum[i] + csum[i + 1] + csum[i + 2], count = ccnt[i] + ccnt[i + 1] + ccnt[i + 2];
        o[i] = count > 5 ? (int16_t)(int)((float)sum / (float)count) : (int16_t)CART_DISPARITY_INVALID;   // interpolation.cu:33: count > r*r + 1 = 5
    }
    if (((reinterpret_cast<uintptr_t>(orow) | out.step) & 7) == 0 && xb + 4 <= g.w) {
        *reinterpret_cast<uint2 *>(orow + xb) = make_uint2((uint16_t)o[0] | ((uint32_t)(uint16_t)o[1] << 16), (uint16_t)o[2] | ((uint32_t)(uint16_t)o[3] << 16));
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (xb + i < g.w) orow[xb + i] = o[i];
    }
}

// can the post stage take the first interpolation pass with it?  (radius 2, the range test representable in the tile's s16 sentinel scheme)
bool post_interp_fusable(int radius, int min_disp16, int max_disp) { return radius == 2 && min_disp16 >= 0 && min_disp16 < (1 << 15) && max_disp > min_disp16; }
void launch_post_interp(const uint16_t *wta_l, const uint32_t *right_pk, const uint8_t *gray_l, const OutBatch &out, const Geometry &g, int n_frames,
                        hipStream_t s, int spec, int min_disp16, int max_disp) {
    dim3 grid((g.w + PI_W - 1) / PI_W, (g.h + PI_H - 1) / PI_H, n_frames), block(256);
    hipLaunchKernelGGL(post_interp_kernel, grid, block, 0, s, wta_l, right_pk, gray_l, out, g, spec, min_disp16, max_disp);
}

void launch_post(const uint16_t *wta_l, const uint32_t *right_pk, const uint8_t *gray_l, const OutBatch &out, const Geometry &g,
                 int n_frames, hipStream_t s, int spec) {
    dim3 grid((g.w + 63) / 64, (g.h + 3) / 4, n_frames), block(64, 4);
    hipLaunchKernelGGL(post_kernel, grid, block, 0, s, wta_l, right_pk, gray_l, out, g, spec);
}

}  // namespace cart_amd

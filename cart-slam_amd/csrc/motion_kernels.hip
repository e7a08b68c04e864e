// motion_kernels.hip -- motion segmentation from flow, disparity and ego-motion (spec S25; C ABI in engine_motion.hip):
//   motion_residual  per pixel: the previous frame's point (flow + previous disparity) carried through the relative pose and projected
//                    back, against where this frame's image and disparity see it -> raw label and, if asked, the residual record.
//                    A lane takes kMotionStrip rows of one column: the loads of its pixels (disparity, flow) are issued together, then
//                    the gathers from the previous disparity together, then the arithmetic.
//   motion_filter    majority of the raw labels over the known neighbours of a (2 radius + 1)^2 window.  The raw labels of a tile and
//                    its halo are staged in LDS, cells outside the image as UNKNOWN, so the window clips at the edges by itself.  The
//                    counts are separable: one pass of row sums over the staged rows (both counts packed in 16 bits), one pass of
//                    column sums over those -- (2 radius + 1) (1 + (tile rows + 2 radius) / tile rows) LDS reads per pixel against
//                    (2 radius + 1)^2 for the direct walk (22 against 81 at radius 4).
// fp64 with + - * / floor only, in the association order of warp_device.h, which holds the warp chain.
// No atomics: the result cannot depend on execution order.

#include "engine_internal.h"
#include "warp_device.h"

namespace cart_amd {

namespace {

__device__ __forceinline__ int16_t quantise(double e) {   // Q(e) = clamp(floor(16 e + 0.5), -32767, 32767)
    const double v = floor(e * 16.0 + 0.5);
    return (int16_t)(!(v > -32767.0) ? -32767.0 : (v > 32767.0 ? 32767.0 : v));
}

__global__ __launch_bounds__(256) void motion_residual_kernel(MotionArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y0 = blockIdx.y * kMotionStrip;
    int sc[kMotionStrip], fl[kMotionStrip];
    bool in[kMotionStrip];
#pragma unroll
    for (int r = 0; r < kMotionStrip; ++r) {   // every load of the strip before the first use
        in[r] = x < a.w && y0 + r < a.h;
        sc[r] = in[r] ? row_ptr(a.disp_cur, a.disp_cur_step, y0 + r)[x] : -32768;
        fl[r] = in[r] ? reinterpret_cast<const int *>(row_ptr(a.flow, a.flow_step, y0 + r))[x] : 0;
    }
    int xp[kMotionStrip], yp[kMotionStrip], sp[kMotionStrip];
    double dc[kMotionStrip];
#pragma unroll
    for (int r = 0; r < kMotionStrip; ++r) {   // gates 1 and 2, then every gather of the strip before the first use
        dc[r] = (double)sc[r] / 16.0;
        const int2 prev = flow_previous(fl[r], x, y0 + r);
        xp[r] = prev.x;
        yp[r] = prev.y;
        const bool ok = in[r] && sc[r] != -32768 && dc[r] >= a.p.min_disparity && xp[r] >= 0 && xp[r] < a.w && yp[r] >= 0 && yp[r] < a.h;
        sp[r] = ok ? row_ptr(a.disp_prev, a.disp_prev_step, yp[r])[xp[r]] : -32768;
    }
    const double fxb = a.cam.fx * a.cam.baseline;
    const double ft2 = a.p.flow_threshold * a.p.flow_threshold, dt2 = a.p.disparity_threshold * a.p.disparity_threshold;
#pragma unroll
    for (int r = 0; r < kMotionStrip; ++r) {
        if (!in[r]) continue;
        short4 rec = make_short4(-32768, -32768, -32768, 2);
        const double dp = (double)sp[r] / 16.0;
        if (sp[r] != -32768 && dp >= a.p.min_disparity) {   // gate 3 (a failed gate 1 or 2 left sp invalid)
            const WarpPoint q = pose_carry(a.rel, back_project(a.cam, fxb, xp[r], yp[r], dp));
            if (q.z > 0) {                                   // gate 4
                const double eu = project_u(a.cam, q) - (double)x;
                const double ev = project_v(a.cam, q) - (double)(y0 + r);
                const double ed = fxb / q.z - dc[r];
                const bool moving = eu * eu + ev * ev > ft2 || ed * ed > dt2;
                rec = make_short4(quantise(eu), quantise(ev), quantise(ed), moving ? 1 : 0);
            }
        }
        row_ptr(a.raw, a.raw_step, y0 + r)[x] = (uint8_t)rec.w;
        if (a.residual) reinterpret_cast<short4 *>(row_ptr(a.residual, a.residual_step, y0 + r))[x] = rec;   // one 8-byte store
    }
}

__global__ __launch_bounds__(256) void motion_filter_kernel(MotionArgs a) {
    constexpr int kHaloW = kMotionTileW + 2 * kMotionMaxRadius, kHaloH = kMotionTileH + 2 * kMotionMaxRadius;
    __shared__ uint8_t tile[kHaloH * kHaloW];            // raw labels, rows of tw = kMotionTileW + 2 radius
    __shared__ uint16_t sums[kHaloH * kMotionTileW];     // row sums: MOVING in the low byte, STATIC in the high byte (each <= 9)
    const int rad = a.p.radius;
    const int tw = kMotionTileW + 2 * rad, th = kMotionTileH + 2 * rad;
    const int x0 = blockIdx.x * kMotionTileW, y0 = blockIdx.y * kMotionTileH;
    for (int i = threadIdx.x; i < tw * th; i += 256) {   // the tile with its halo; outside the image a cell is UNKNOWN: it counts for nothing
        const int ty = i / tw, tx = i - ty * tw;
        const int gx = x0 + tx - rad, gy = y0 + ty - rad;
        tile[i] = (gx >= 0 && gx < a.w && gy >= 0 && gy < a.h) ? row_ptr(a.raw, a.raw_step, gy)[gx] : (uint8_t)2;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < th * kMotionTileW; i += 256) {
        const int ty = i / kMotionTileW, tx = i % kMotionTileW;
        const uint8_t *src = tile + ty * tw + tx;
        unsigned s = 0;
        for (int k = 0; k <= 2 * rad; ++k) {
            const unsigned v = src[k];
            s += v == 1u ? 1u : (v == 0u ? 256u : 0u);
        }
        sums[i] = (uint16_t)s;
    }
    __syncthreads();
    const int tx = threadIdx.x % kMotionTileW, gx = x0 + tx;
    if (gx >= a.w) return;
    for (int ty = threadIdx.x / kMotionTileW; ty < kMotionTileH; ty += 256 / kMotionTileW) {
        const int gy = y0 + ty;
        if (gy >= a.h) break;
        const unsigned own = tile[(ty + rad) * tw + tx + rad];
        unsigned label = 2;
        if (own != 2u) {
            unsigned nm = 0, ns = 0;
            for (int k = 0; k <= 2 * rad; ++k) {
                const unsigned s = sums[(ty + k) * kMotionTileW + tx];
                nm += s & 255u;
                ns += s >> 8;
            }
            label = nm * 100u >= (unsigned)a.p.support_percent * (nm + ns) ? 1u : 0u;
        }
        row_ptr(a.labels, a.labels_step, gy)[gx] = (uint8_t)label;
        if (a.planes) row_ptr(a.planes_static, a.planes_static_step, gy)[gx] = label == 1u ? (uint8_t)2 : row_ptr(a.planes, a.planes_step, gy)[gx];
    }
}

}  // namespace

void launch_motion_residual(const MotionArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(motion_residual_kernel, dim3((unsigned)((a.w + 255) / 256), (unsigned)((a.h + kMotionStrip - 1) / kMotionStrip)), dim3(256), 0, s, a);
}

void launch_motion_filter(const MotionArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(motion_filter_kernel, dim3((unsigned)((a.w + kMotionTileW - 1) / kMotionTileW), (unsigned)((a.h + kMotionTileH - 1) / kMotionTileH)),
                       dim3(256), 0, s, a);
}

}  // namespace cart_amd

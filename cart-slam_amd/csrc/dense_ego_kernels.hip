// dense_ego_kernels.hip -- dense ego-motion refinement from flow and disparity (spec S26; C ABI in engine_dense_ego.hip).
// One call is iterations + 1 evaluations of the normal equations over every static pixel, each a pair of launches:
//   dense_ego_rows   one workgroup of kDenseLanes lanes per sampled row.  A lane walks its sampled columns l, l + 256, ... in ascending
//                    order, kDenseCols at a time: their loads (disparity, flow as one 4-byte word, mask) are issued together, then the
//                    gathers from the previous disparity (guarded by gates 1 and 2), then the arithmetic into 28 fp64 accumulators.
//                    The butterfly v[l] += v[l ^ o] ascends: o = 1 .. 32 are exchanges inside a wave, o = 64 and 128 combine the four
//                    waves' values through a [28][4] LDS array.  Lanes 0 .. 28 store the row partial (28 sums, then the two counts).
//   dense_ego_step   one workgroup: lane l adds the partials of sampled rows l, l + 256, ..., the same butterfly, then lane 0 solves
//                    the 6 x 6 system (ego_solve.h, S23's), updates the pose in device memory and, at a stop, writes the result.
// The pose of evaluation 0 is the call's rel0 (a kernel argument); later evaluations read the state the previous step wrote.  After a
// stop (too few inliers, a pivot that is not > 0, or the last evaluation) the state's flag makes every later launch leave at once.
// fp64 with + - * / sqrt only, in the association order of warp_device.h, which holds the warp chain.
// No floating-point atomics: the result cannot depend on execution order.

#include "engine_internal.h"
#include "dense_reduce.h"
#include "ego_solve.h"
#include "warp_device.h"

#pragma clang fp contract(off)

namespace cart_amd {

namespace {

__global__ __launch_bounds__(kDenseLanes) void dense_ego_rows_kernel(DenseEgoArgs a, int eval) {
    const DenseEgoState *st = a.state;
    if (eval > 0 && st->stop) return;   // uniform
    double P[12];   // the pose as 3 x 4 (R | t): rel0 as it comes, later the state's R and t
#pragma unroll
    for (int q = 0; q < 9; ++q) P[4 * (q / 3) + q % 3] = eval == 0 ? a.rel0[4 * (q / 3) + q % 3] : st->R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) P[4 * q + 3] = eval == 0 ? a.rel0[4 * q + 3] : st->t[q];
    const int lane = threadIdx.x, stride = a.p.stride;
    const int y = blockIdx.x * stride;
    const double fx = a.cam.fx, fy = a.cam.fy, cx = a.cam.cx, cy = a.cam.cy, wd = a.p.disparity_weight;
    const double fxb = fx * a.cam.baseline;
    const double ft2 = a.p.flow_threshold * a.p.flow_threshold, dt2 = a.p.disparity_threshold * a.p.disparity_threshold;
    const int16_t *cur_row = row_ptr(a.disp_cur, a.disp_cur_step, y);
    const int *flow_row = reinterpret_cast<const int *>(row_ptr(a.flow, a.flow_step, y));
    const uint8_t *mask_row = a.mask ? row_ptr(a.mask, a.mask_step, y) : nullptr;
    double acc[kDenseSums];
#pragma unroll
    for (int k = 0; k < kDenseSums; ++k) acc[k] = 0.0;
    int cnt = 0, ncand = 0;
    for (int i0 = 0; i0 < a.ni; i0 += kDenseCols * kDenseLanes) {   // uniform
        int sc[kDenseCols], fl[kDenseCols], sp[kDenseCols];
        bool in[kDenseCols];
#pragma unroll
        for (int r = 0; r < kDenseCols; ++r) {   // every load of the group before the first use
            const int x = (i0 + r * kDenseLanes + lane) * stride;
            in[r] = i0 + r * kDenseLanes + lane < a.ni;   // then x < w
            sc[r] = in[r] ? cur_row[x] : -32768;
            fl[r] = in[r] ? flow_row[x] : 0;
            if (in[r] && mask_row && mask_row[x] == 1) sc[r] = -32768;   // a MOVING pixel is no candidate
        }
#pragma unroll
        for (int r = 0; r < kDenseCols; ++r) {   // gates 1 and 2, then every gather of the group before the first use
            const int x = (i0 + r * kDenseLanes + lane) * stride;
            const int2 prev = flow_previous(fl[r], x, y);
            const int xp = prev.x, yp = prev.y;
            const bool ok = in[r] && sc[r] != -32768 && (double)sc[r] / 16.0 >= a.p.min_disparity && xp >= 0 && xp < a.w && yp >= 0 && yp < a.h;
            sp[r] = ok ? row_ptr(a.disp_prev, a.disp_prev_step, yp)[xp] : -32768;
        }
#pragma unroll
        for (int r = 0; r < kDenseCols; ++r) {
            const double dp = (double)sp[r] / 16.0;
            if (sp[r] == -32768 || !(dp >= a.p.min_disparity)) continue;   // gate 3 (a failed gate 1 or 2 or the mask left sp invalid)
            ++ncand;
            const int x = (i0 + r * kDenseLanes + lane) * stride;
            const int2 prev = flow_previous(fl[r], x, y);
            const int xp = prev.x, yp = prev.y;
            const WarpPoint q = pose_carry(P, back_project(a.cam, fxb, xp, yp, dp));
            const double qx = q.x, qy = q.y, qz = q.z;
            if (!(qz > 0)) continue;
            // warp_device.h's projection, written out: through project_u / project_v the kernel's instructions come out in another order
            // and a refinement takes 1 % longer (profiles/pose_warp_refactor.txt)
            const double eu = ((fx * qx) / qz + cx) - (double)x;
            const double ev = ((fy * qy) / qz + cy) - (double)y;
            const double ed = fxb / qz - (double)sc[r] / 16.0;
            const double ef = eu * eu + ev * ev;
            if (!(ef < ft2 && ed * ed < dt2)) continue;
            ++cnt;
            const double ja = fx / qz, jb = -((fx * qx) / (qz * qz));
            const double jc = fy / qz, jd = -((fy * qy) / (qz * qz));
            const double jg = -(fxb / (qz * qz));
            const double Ju[6] = {jb * qy, ja * qz - jb * qx, -(ja * qy), ja, 0.0, jb};
            const double Jv[6] = {jd * qy - jc * qz, -(jd * qx), jc * qx, 0.0, jc, jd};
            const double Jd[6] = {jg * qy, -(jg * qx), 0.0, 0.0, 0.0, jg};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j, ++k) acc[k] = acc[k] + ((Ju[i] * Ju[j] + Jv[i] * Jv[j]) + wd * (Jd[i] * Jd[j]));
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + ((Ju[i] * eu + Jv[i] * ev) + wd * (Jd[i] * ed));
            acc[27] = acc[27] + (ef + wd * (ed * ed));
        }
    }
    double tot;
    dense_reduce(acc, cnt, ncand, tot);
    const size_t j = blockIdx.x;
    if (lane < kDenseSums) a.partial[(size_t)lane * a.rows_cap + j] = tot;
    if (lane == kDenseSums) reinterpret_cast<int2 *>(a.partial + (size_t)kDenseSums * a.rows_cap)[j] = make_int2(cnt, ncand);
}

__global__ __launch_bounds__(kDenseLanes) void dense_ego_step_kernel(DenseEgoArgs a, int eval) {
    __shared__ double s_tot[kDenseSums];
    DenseEgoState *st = a.state;
    if (eval > 0 && st->stop) return;   // uniform
    const int lane = threadIdx.x;
    double acc[kDenseSums];
#pragma unroll
    for (int k = 0; k < kDenseSums; ++k) acc[k] = 0.0;
    int cnt = 0, ncand = 0;
    const int2 *counts = reinterpret_cast<const int2 *>(a.partial + (size_t)kDenseSums * a.rows_cap);
    for (int j = lane; j < a.nj; j += kDenseLanes) {   // ascending rows; a row without a contributor adds its +0.0
#pragma unroll
        for (int k = 0; k < kDenseSums; ++k) acc[k] = acc[k] + a.partial[(size_t)k * a.rows_cap + j];
        const int2 c = counts[j];
        cnt += c.x;
        ncand += c.y;
    }
    double tot;
    dense_reduce(acc, cnt, ncand, tot);
    if (lane < kDenseSums) s_tot[lane] = tot;
    __syncthreads();
    if (lane != 0) return;
    const double rms = cnt ? sqrt(s_tot[27] / (double)cnt) : 0.0;
    double R[9], t[3];
    for (int q = 0; q < 9; ++q) R[q] = eval == 0 ? a.rel0[4 * (q / 3) + q % 3] : st->R[q];
    for (int q = 0; q < 3; ++q) t[q] = eval == 0 ? a.rel0[4 * q + 3] : st->t[q];
    int steps = eval == 0 ? 0 : st->steps;
    const double rms_initial = eval == 0 ? rms : st->rms_initial;
    const int n_initial = eval == 0 ? cnt : st->n_initial;
    bool stop = eval >= a.p.iterations;   // the last evaluation only measures
    if (!stop) stop = cnt < a.p.min_inliers;
    if (!stop) {
        double H[6][6], g[6], d[6];
        int k = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++k) H[i][j] = s_tot[k];
        for (int i = 0; i < 6; ++i) g[i] = s_tot[21 + i];
        stop = !ego_solve6(H, g, d);
        if (!stop) {
            ego_update(d, R, t);
            ++steps;
        }
    }
    if (stop) {   // this evaluation is the last one at the pose: its count and error are the final ones
        cart_dense_ego_result r;
        for (int q = 0; q < 9; ++q) r.R[q] = R[q];
        for (int q = 0; q < 3; ++q) r.t[q] = t[q];
        r.rms_initial = rms_initial; r.rms = rms;
        r.status = steps > 0 ? 1 : 0; r.n_candidates = ncand; r.n_initial = n_initial; r.n_inliers = cnt; r.steps = steps; r.reserved = 0;
        *a.result = r;
    }
    for (int q = 0; q < 9; ++q) st->R[q] = R[q];
    for (int q = 0; q < 3; ++q) st->t[q] = t[q];
    st->rms_initial = rms_initial;
    st->n_initial = n_initial; st->n_candidates = ncand; st->steps = steps; st->stop = stop ? 1 : 0;
}

}  // namespace

void launch_dense_ego(const DenseEgoArgs &a, hipStream_t s) {
    for (int eval = 0; eval <= a.p.iterations; ++eval) {
        hipLaunchKernelGGL(dense_ego_rows_kernel, dim3((unsigned)a.nj), dim3(kDenseLanes), 0, s, a, eval);
        hipLaunchKernelGGL(dense_ego_step_kernel, dim3(1), dim3(kDenseLanes), 0, s, a, eval);
    }
}

}  // namespace cart_amd

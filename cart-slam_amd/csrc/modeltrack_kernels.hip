// modeltrack_kernels.hip -- frame-to-model pose tracking against the TSDF volume (spec S34; C ABI in engine_modeltrack.hip).
// One call is iterations + 1 evaluations of the normal equations of sum F(P p)^2 over the frame's back-projected pixels, each a pair of
// launches after dense_ego_kernels.hip:
//   model_track_rows   one workgroup of kDenseLanes lanes per sampled row.  A lane walks its sampled columns l, l + 256, ... in ascending
//                      order, kTrackCols at a time: their image loads (disparity, mask) are issued together, then per column the pixel
//                      gates, the point and the eight corner gathers of its sample (voxel_sample.h), all gathers of the group before the
//                      first use, then the arithmetic into 28 fp64 accumulators.  The butterfly and the row partial are S26's (dense_reduce.h).
//   model_track_step   one workgroup: lane l adds the partials of sampled rows l, l + 256, ..., the same butterfly, then lane 0 damps and
//                      solves the 6 x 6 system (ego_solve.h), updates the pose in device memory and, at a stop, writes the result.
// The pose of evaluation 0 is the call's pose0 (a kernel argument); later evaluations read the state the previous step wrote.  After a
// stop the state's flag makes every later launch leave at once.  The volume is only read.
// fp64 with + - * / floor sqrt only, in the written association order.  No floating-point atomics.

#include "engine_internal.h"
#include "dense_reduce.h"
#include "ego_solve.h"
#include "voxel_sample.h"
#include "warp_device.h"

#pragma clang fp contract(off)

namespace cart_amd {

namespace {

__global__ __launch_bounds__(kDenseLanes) void model_track_rows_kernel(ModelTrackArgs a, int eval) {
    const DenseEgoState *st = a.state;
    if (eval > 0 && st->stop) return;   // uniform
    double P[12];   // the pose as 3 x 4 (R | t): pose0 as it comes, later the state's R and t
#pragma unroll
    for (int q = 0; q < 9; ++q) P[4 * (q / 3) + q % 3] = eval == 0 ? a.pose0[4 * (q / 3) + q % 3] : st->R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) P[4 * q + 3] = eval == 0 ? a.pose0[4 * q + 3] : st->t[q];
    const int lane = threadIdx.x, stride = a.p.stride;
    const int y = blockIdx.x * stride;
    const double fxb = a.cam.fx * a.cam.baseline;
    const double gs = 32767.0 * a.mp.voxel_size;
    const int16_t *disp_row = row_ptr(a.disp, a.disp_step, y);
    const uint8_t *mask_row = a.mask ? row_ptr(a.mask, a.mask_step, y) : nullptr;
    double acc[kDenseSums];
#pragma unroll
    for (int k = 0; k < kDenseSums; ++k) acc[k] = 0.0;
    int cnt = 0, ncand = 0;
    for (int i0 = 0; i0 < a.ni; i0 += kTrackCols * kDenseLanes) {   // uniform
        int sc[kTrackCols];
#pragma unroll
        for (int r = 0; r < kTrackCols; ++r) {   // every image load of the group before the first use
            const int x = (i0 + r * kDenseLanes + lane) * stride;
            const bool in = i0 + r * kDenseLanes + lane < a.ni;   // then x < w
            sc[r] = in ? disp_row[x] : -32768;
            if (in && mask_row && mask_row[x] == 1) sc[r] = -32768;   // a MOVING pixel is no candidate
        }
        WarpPoint p[kTrackCols];
        VoxelCorners c[kTrackCols];
#pragma unroll
        for (int r = 0; r < kTrackCols; ++r) {   // the pixel gates, then every gather of the group before the first use
            const int x = (i0 + r * kDenseLanes + lane) * stride;
            const double d = (double)sc[r] / 16.0;
            const double Z = fxb / d;
            const bool ok = !a.empty && sc[r] != -32768 && d >= a.mp.min_disparity && Z >= a.mp.min_depth && Z <= a.mp.max_depth;
            p[r] = pose_carry(P, WarpPoint{back_project_x(a.cam, x, Z), back_project_y(a.cam, y, Z), Z});
            voxel_gather(a.grid, a.mp.voxel_size, p[r], ok, c[r]);
        }
#pragma unroll
        for (int r = 0; r < kTrackCols; ++r) {
            VoxelSample s;
            if (!voxel_value(c[r], a.mp.min_weight, s)) continue;
            ++ncand;
            const double res = s.F / 32767.0;
            if (!((res < 0.0 ? -res : res) < a.p.residual_gate)) continue;
            ++cnt;
            const double Gx = s.gx / gs, Gy = s.gy / gs, Gz = s.gz / gs;
            const double J[6] = {p[r].y * Gz - p[r].z * Gy, p[r].z * Gx - p[r].x * Gz, p[r].x * Gy - p[r].y * Gx, Gx, Gy, Gz};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j, ++k) acc[k] = acc[k] + J[i] * J[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + J[i] * res;
            acc[27] = acc[27] + res * res;
        }
    }
    double tot;
    dense_reduce(acc, cnt, ncand, tot);
    const size_t j = blockIdx.x;
    if (lane < kDenseSums) a.partial[(size_t)lane * a.rows_cap + j] = tot;
    if (lane == kDenseSums) reinterpret_cast<int2 *>(a.partial + (size_t)kDenseSums * a.rows_cap)[j] = make_int2(cnt, ncand);
}

__global__ __launch_bounds__(kDenseLanes) void model_track_step_kernel(ModelTrackArgs a, int eval) {
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
    for (int q = 0; q < 9; ++q) R[q] = eval == 0 ? a.pose0[4 * (q / 3) + q % 3] : st->R[q];
    for (int q = 0; q < 3; ++q) t[q] = eval == 0 ? a.pose0[4 * q + 3] : st->t[q];
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
        for (int i = 0; i < 6; ++i) H[i][i] = H[i][i] + a.p.damping * (double)cnt;
        for (int i = 0; i < 6; ++i) g[i] = s_tot[21 + i];
        stop = !ego_solve6(H, g, d);
        if (!stop) {
            ego_update(d, R, t);
            ++steps;
        }
    }
    if (stop) {   // this evaluation is the last one at the pose: its counts and error are the final ones
        cart_model_track_result r;
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

void launch_model_track(const ModelTrackArgs &a, hipStream_t s) {
    for (int eval = 0; eval <= a.p.iterations; ++eval) {
        hipLaunchKernelGGL(model_track_rows_kernel, dim3((unsigned)a.nj), dim3(kDenseLanes), 0, s, a, eval);
        hipLaunchKernelGGL(model_track_step_kernel, dim3(1), dim3(kDenseLanes), 0, s, a, eval);
    }
}

}  // namespace cart_amd

// modeltrack_color_kernels.hip -- colour-aided frame-to-model pose tracking (spec S38; C ABI in engine_modeltrack_color.hip):
// S34's geometric term against the TSDF volume plus a photometric term against the luminance of the colour volume (S37).
// One call is iterations + 1 evaluations, each a pair of launches after modeltrack_kernels.hip:
//   model_track_color_rows   one workgroup of kDenseLanes lanes per sampled row.  A lane walks its sampled columns l, l + 256, ... in
//                            ascending order, kTrackColorCols at a time: their image loads (disparity, mask, the image bytes) are issued
//                            together, then per column the pixel gates, the point and the sixteen corner gathers of its two samples
//                            (voxel_sample.h, color_sample.h), all gathers of the group before the first use, then the arithmetic into
//                            29 fp64 accumulators: a pixel's geometric terms first, then its photometric terms.
//   model_track_color_step   one workgroup: lane l adds the partials of sampled rows l, l + 256, ..., the same butterfly
//                            (track_color_reduce.h), then lane 0 damps and solves the 6 x 6 system (ego_solve.h), updates the pose in
//                            device memory and, at a stop, writes the result.
// With photo_weight == 0 (or a colour object without a window) neither the image nor the colour volume is read.  Both volumes are only read.
// fp64 with + - * / floor sqrt only, in the written association order.  No floating-point atomics.

#include "engine_internal.h"
#include "color_sample.h"
#include "ego_solve.h"
#include "track_color_reduce.h"
#include "voxel_sample.h"
#include "warp_device.h"

#pragma clang fp contract(off)

namespace cart_amd {

namespace {

__global__ __launch_bounds__(kDenseLanes) void model_track_color_rows_kernel(ModelTrackColorArgs a, int eval) {
    const ModelTrackColorState *st = a.state;
    if (eval > 0 && st->stop) return;   // uniform
    double P[12];   // the pose as 3 x 4 (R | t): pose0 as it comes, later the state's R and t
#pragma unroll
    for (int q = 0; q < 9; ++q) P[4 * (q / 3) + q % 3] = eval == 0 ? a.pose0[4 * (q / 3) + q % 3] : st->R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) P[4 * q + 3] = eval == 0 ? a.pose0[4 * q + 3] : st->t[q];
    const int lane = threadIdx.x, stride = a.p.stride;
    const int y = blockIdx.x * stride;
    const double fxb = a.cam.fx * a.cam.baseline;
    const double gs = 32767.0 * a.mp.voxel_size, gsc = 1020.0 * a.mp.voxel_size;
    const double lambda = a.cp.photo_weight;
    const bool photo = lambda > 0.0 && !a.cempty;   // uniform
    const int16_t *disp_row = row_ptr(a.disp, a.disp_step, y);
    const uint8_t *mask_row = a.mask ? row_ptr(a.mask, a.mask_step, y) : nullptr;
    const uint8_t *image_row = photo ? row_ptr(a.image, a.image_step, y) : nullptr;
    double acc[kTrackColorSums];
#pragma unroll
    for (int k = 0; k < kTrackColorSums; ++k) acc[k] = 0.0;
    int cnt = 0, ncand = 0, nphoto = 0;
    for (int i0 = 0; i0 < a.ni; i0 += kTrackColorCols * kDenseLanes) {   // uniform
        int sc[kTrackColorCols], lobs[kTrackColorCols];
#pragma unroll
        for (int r = 0; r < kTrackColorCols; ++r) {   // every image load of the group before the first use
            const int x = (i0 + r * kDenseLanes + lane) * stride;
            const bool in = i0 + r * kDenseLanes + lane < a.ni;   // then x < w
            sc[r] = in ? disp_row[x] : -32768;
            if (in && mask_row && mask_row[x] == 1) sc[r] = -32768;   // a MOVING pixel is no candidate
            lobs[r] = 0;
            if (in && photo) {
                if (a.channels == 3) {
                    const uint8_t *px = image_row + (size_t)x * 3;
                    lobs[r] = (int)px[0] + 2 * (int)px[1] + (int)px[2];
                } else {
                    lobs[r] = 4 * (int)image_row[x];
                }
            }
        }
        WarpPoint p[kTrackColorCols];
        VoxelCorners c[kTrackColorCols], cc[kTrackColorCols];
#pragma unroll
        for (int r = 0; r < kTrackColorCols; ++r) {   // the pixel gates, then every gather of the group before the first use
            const int x = (i0 + r * kDenseLanes + lane) * stride;
            const double d = (double)sc[r] / 16.0;
            const double Z = fxb / d;
            const bool ok = !a.empty && sc[r] != -32768 && d >= a.mp.min_disparity && Z >= a.mp.min_depth && Z <= a.mp.max_depth;
            p[r] = pose_carry(P, WarpPoint{back_project_x(a.cam, x, Z), back_project_y(a.cam, y, Z), Z});
            voxel_gather(a.grid, a.mp.voxel_size, p[r], ok, c[r]);
            color_gather(a.cgrid, a.mp.voxel_size, p[r], ok && photo, cc[r]);
        }
#pragma unroll
        for (int r = 0; r < kTrackColorCols; ++r) {
            VoxelSample s;
            if (!voxel_value(c[r], a.mp.min_weight, s)) continue;
            ++ncand;
            const double res = s.F / 32767.0;
            if (!((res < 0.0 ? -res : res) < a.p.residual_gate)) continue;
            ++cnt;
            {
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
            VoxelSample sc_;
            if (!color_value(cc[r], a.cp.color_min_weight, sc_)) continue;   // not inside (or no photometric term at all), or a corner too light
            const double rc = (sc_.F - (double)lobs[r]) / 1020.0;
            if (!((rc < 0.0 ? -rc : rc) < a.cp.photo_gate)) continue;
            ++nphoto;
            const double Gx = sc_.gx / gsc, Gy = sc_.gy / gsc, Gz = sc_.gz / gsc;
            const double J[6] = {p[r].y * Gz - p[r].z * Gy, p[r].z * Gx - p[r].x * Gz, p[r].x * Gy - p[r].y * Gx, Gx, Gy, Gz};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double wj = lambda * J[i];
#pragma unroll
                for (int j = i; j < 6; ++j, ++k) acc[k] = acc[k] + wj * J[j];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + (lambda * J[i]) * rc;
            acc[28] = acc[28] + rc * rc;
        }
    }
    double tot;
    track_color_reduce(acc, cnt, ncand, nphoto, tot);
    const size_t j = blockIdx.x;
    if (lane < kTrackColorSums) a.partial[(size_t)lane * a.rows_cap + j] = tot;
    if (lane == kTrackColorSums) reinterpret_cast<int2 *>(a.partial + (size_t)kTrackColorSums * a.rows_cap)[j] = make_int2(cnt, ncand);
    if (lane == kTrackColorSums + 1) reinterpret_cast<int2 *>(a.partial + (size_t)(kTrackColorSums + 1) * a.rows_cap)[j] = make_int2(nphoto, 0);
}

__global__ __launch_bounds__(kDenseLanes) void model_track_color_step_kernel(ModelTrackColorArgs a, int eval) {
    __shared__ double s_tot[kTrackColorSums];
    ModelTrackColorState *st = a.state;
    if (eval > 0 && st->stop) return;   // uniform
    const int lane = threadIdx.x;
    double acc[kTrackColorSums];
#pragma unroll
    for (int k = 0; k < kTrackColorSums; ++k) acc[k] = 0.0;
    int cnt = 0, ncand = 0, nphoto = 0;
    const int2 *counts = reinterpret_cast<const int2 *>(a.partial + (size_t)kTrackColorSums * a.rows_cap);
    const int2 *photos = reinterpret_cast<const int2 *>(a.partial + (size_t)(kTrackColorSums + 1) * a.rows_cap);
    for (int j = lane; j < a.nj; j += kDenseLanes) {   // ascending rows; a row without a contributor adds its +0.0
#pragma unroll
        for (int k = 0; k < kTrackColorSums; ++k) acc[k] = acc[k] + a.partial[(size_t)k * a.rows_cap + j];
        const int2 c = counts[j];
        cnt += c.x;
        ncand += c.y;
        nphoto += photos[j].x;
    }
    double tot;
    track_color_reduce(acc, cnt, ncand, nphoto, tot);
    if (lane < kTrackColorSums) s_tot[lane] = tot;
    __syncthreads();
    if (lane != 0) return;
    const double lambda = a.cp.photo_weight;
    const double rms = cnt ? sqrt(s_tot[27] / (double)cnt) : 0.0;
    const double rms_photo = nphoto ? sqrt(s_tot[28] / (double)nphoto) : 0.0;
    const double den = (double)cnt + lambda * (double)nphoto;
    const double cost = den != 0.0 ? sqrt((s_tot[27] + lambda * s_tot[28]) / den) : 0.0;
    double R[9], t[3];
    for (int q = 0; q < 9; ++q) R[q] = eval == 0 ? a.pose0[4 * (q / 3) + q % 3] : st->R[q];
    for (int q = 0; q < 3; ++q) t[q] = eval == 0 ? a.pose0[4 * q + 3] : st->t[q];
    int steps = eval == 0 ? 0 : st->steps;
    const double rms_initial = eval == 0 ? rms : st->rms_initial;
    const double rms_photo_initial = eval == 0 ? rms_photo : st->rms_photo_initial;
    const double cost_initial = eval == 0 ? cost : st->cost_initial;
    const int n_initial = eval == 0 ? cnt : st->n_initial;
    const int n_photo_initial = eval == 0 ? nphoto : st->n_photo_initial;
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
    if (stop) {   // this evaluation is the last one at the pose: its counts and errors are the final ones
        cart_model_track_color_result r;
        for (int q = 0; q < 9; ++q) r.R[q] = R[q];
        for (int q = 0; q < 3; ++q) r.t[q] = t[q];
        r.rms_initial = rms_initial; r.rms = rms;
        r.status = steps > 0 ? 1 : 0; r.n_candidates = ncand; r.n_initial = n_initial; r.n_inliers = cnt; r.steps = steps; r.reserved = 0;
        r.rms_photo_initial = rms_photo_initial; r.rms_photo = rms_photo; r.cost_initial = cost_initial; r.cost = cost;
        r.n_photo_initial = n_photo_initial; r.n_photo = nphoto;
        *a.result = r;
    }
    for (int q = 0; q < 9; ++q) st->R[q] = R[q];
    for (int q = 0; q < 3; ++q) st->t[q] = t[q];
    st->rms_initial = rms_initial; st->rms_photo_initial = rms_photo_initial; st->cost_initial = cost_initial;
    st->n_initial = n_initial; st->n_photo_initial = n_photo_initial; st->n_candidates = ncand; st->steps = steps; st->stop = stop ? 1 : 0;
    st->reserved = 0;
}

}  // namespace

void launch_model_track_color(const ModelTrackColorArgs &a, hipStream_t s) {
    for (int eval = 0; eval <= a.p.iterations; ++eval) {
        hipLaunchKernelGGL(model_track_color_rows_kernel, dim3((unsigned)a.nj), dim3(kDenseLanes), 0, s, a, eval);
        hipLaunchKernelGGL(model_track_color_step_kernel, dim3(1), dim3(kDenseLanes), 0, s, a, eval);
    }
}

}  // namespace cart_amd

// ego_kernels.hip -- stereo visual odometry from the ORB matches.  The launches of the two calls:
//   ego_clear / ego_triangulate   one lane per keypoint slot / per stereo match: the landmark table of a frame
//   ego_compact    the usable temporal matches in match order (ballot + prefix in one workgroup, as match_select): the
//                  correspondence list as SoA rows, the match index of every entry and the count n, all on the device
//   ego_fit        one lane per hypothesis: three distinct draws from the S17 stream, the triad fit, the pose into a table
//   ego_score      one lane owns one hypothesis (R, t in registers), a tile of kEgoTile correspondences staged in LDS and read as a
//                  broadcast; grid = hypothesis blocks x correspondence tiles, the integer (count, qerr) partials of a tile are
//                  added to the hypothesis table with integer atomics (exact in any order)
//   ego_refine     one workgroup of kEgoLanes threads: arg-max over the table, every Gauss-Newton step (sums per lane, a tree in
//                  LDS that gives lane 0 of the S23 butterfly, lane 0 solves the 6 x 6 system, the pose goes back through LDS),
//                  the final statistics and the inlier mask
// The list sizes are read on the device; the grids are sized by the capacity and surplus workgroups leave at once.
// All pose arithmetic is IEEE double in the spec's operation order, no FMA contraction.
#include "engine_internal.h"
#include "ego_solve.h"

#pragma clang fp contract(off)

namespace cart_amd {

namespace {

__device__ inline uint64_t ego_mix(uint64_t z) {   // S17's generator (planefit_kernels.hip)
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline uint64_t ego_stream(uint64_t seed, uint64_t tag, uint64_t a, uint64_t b, uint64_t c) {
    return ego_mix(ego_mix(ego_mix(ego_mix(seed ^ tag) ^ a) ^ b) ^ c);
}
__device__ inline uint32_t ego_uniform(uint64_t s, uint64_t c, uint32_t n) { return (uint32_t)(((ego_mix(s + c) >> 32) * (uint64_t)n) >> 32); }

constexpr uint64_t kEgoTag = 3;
constexpr int kEgoMaxDraws = 64;
constexpr double kEgoDegenerate = 1e-12;
constexpr double kEgoQerrScale = 16777216.0;
constexpr int kEgoMinRefine = 6;

__device__ __forceinline__ int ego_count(const int32_t *p, int cap) { return min(max(*p, 0), cap); }

struct V3 { double x, y, z; };
__device__ inline V3 sub3(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline double dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline V3 div3(V3 a, double s) { return V3{a.x / s, a.y / s, a.z / s}; }

// orthonormal frame of three points; false when they are coincident or collinear
__device__ inline bool ego_triad(V3 p0, V3 p1, V3 p2, V3 &e1, V3 &e2, V3 &e3) {
    const V3 u1 = sub3(p1, p0), u2 = sub3(p2, p0);
    const double l1 = dot3(u1, u1);
    if (l1 <= kEgoDegenerate) return false;
    e1 = div3(u1, sqrt(l1));
    const V3 nrm = cross3(e1, u2);
    const double ln = dot3(nrm, nrm);
    if (ln <= kEgoDegenerate) return false;
    e3 = div3(nrm, sqrt(ln));
    e2 = cross3(e3, e1);
    return true;
}

__global__ __launch_bounds__(256) void ego_clear_kernel(EgoArgs a) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ego_count(a.left_count, a.cap)) return;
    double *o = a.landmarks + 4 * (size_t)s;
    o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0;
}

__global__ __launch_bounds__(256) void ego_triangulate_kernel(EgoArgs a) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ego_count(a.stereo_count, a.cap)) return;
    const cart_match m = a.stereo[s];
    if (m.query < 0 || m.query >= ego_count(a.left_count, a.cap) || m.train < 0 || m.train >= a.cap) return;
    const double xl = (double)a.kpL[m.query].x, yl = (double)a.kpL[m.query].y;
    const double d = xl - (double)a.kpR[m.train].x;
    if (!(d >= a.p.min_disparity)) return;   // a NaN fails
    const double Z = (a.cam.fx * a.cam.baseline) / d;
    double *o = a.landmarks + 4 * (size_t)m.query;
    o[0] = ((xl - a.cam.cx) * Z) / a.cam.fx;
    o[1] = ((yl - a.cam.cy) * Z) / a.cam.fy;
    o[2] = Z;
    o[3] = 1.0;
}

constexpr int kCompactThreads = 1024;
__global__ __launch_bounds__(kCompactThreads) void ego_compact_kernel(EgoArgs a) {
    __shared__ int s_wave[kCompactThreads / 64];
    __shared__ int s_base;
    const int nk = ego_count(a.temporal_count, a.cap);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    for (int k0 = 0; k0 < nk; k0 += kCompactThreads) {   // uniform
        const int k = k0 + threadIdx.x;
        bool ok = false;
        int i = 0, j = 0;
        if (k < nk) {
            const cart_match m = a.temporal[k];
            i = m.query; j = m.train;
            ok = i >= 0 && i < a.cap && j >= 0 && j < a.cap && a.cur[4 * (size_t)i + 3] == 1.0 && a.prev[4 * (size_t)j + 3] == 1.0;
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = s_base, total = 0;
        for (int w = 0; w < kCompactThreads / 64; ++w) {
            const int n = s_wave[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (ok) {
            const int c = before + __popcll(m & ((1ull << lane) - 1));
            const double *pa = a.prev + 4 * (size_t)j, *pb = a.cur + 4 * (size_t)i;
            const size_t cap = (size_t)a.cap;
            a.corr[0 * cap + c] = pa[0]; a.corr[1 * cap + c] = pa[1]; a.corr[2 * cap + c] = pa[2];
            a.corr[3 * cap + c] = pb[0]; a.corr[4 * cap + c] = pb[1]; a.corr[5 * cap + c] = pb[2];
            a.corr[6 * cap + c] = (double)a.cur_kp[i].x;
            a.corr[7 * cap + c] = (double)a.cur_kp[i].y;
            a.corr_k[c] = k;
        }
        __syncthreads();
        if (threadIdx.x == 0) s_base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *a.n = s_base;
}

__global__ __launch_bounds__(kEgoHypLanes) void ego_fit_kernel(EgoArgs a) {
    const int h = blockIdx.x * kEgoHypLanes + threadIdx.x;
    if (h >= a.p.hypotheses) return;
    const int n = *a.n;
    bool ok = n >= 3;
    int idx[3] = {0, 0, 0};
    if (ok) {
        const uint64_t s = ego_stream(a.seed, kEgoTag, a.frame, (uint64_t)h, 0);
        int got = 0;
        for (int c = 0; c < kEgoMaxDraws && got < 3; ++c) {
            const int v = (int)ego_uniform(s, (uint64_t)c, (uint32_t)n);
            if ((got > 0 && v == idx[0]) || (got > 1 && v == idx[1])) continue;
            idx[got++] = v;
        }
        ok = got == 3;
    }
    EgoHyp hyp;
    if (ok) {
        const size_t cap = (size_t)a.cap;
        V3 A[3], B[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            A[k] = V3{a.corr[0 * cap + idx[k]], a.corr[1 * cap + idx[k]], a.corr[2 * cap + idx[k]]};
            B[k] = V3{a.corr[3 * cap + idx[k]], a.corr[4 * cap + idx[k]], a.corr[5 * cap + idx[k]]};
        }
        V3 e1, e2, e3, f1, f2, f3;
        ok = ego_triad(A[0], A[1], A[2], e1, e2, e3) && ego_triad(B[0], B[1], B[2], f1, f2, f3);
        if (ok) {
            const double e[3][3] = {{e1.x, e1.y, e1.z}, {e2.x, e2.y, e2.z}, {e3.x, e3.y, e3.z}};
            const double f[3][3] = {{f1.x, f1.y, f1.z}, {f2.x, f2.y, f2.z}, {f3.x, f3.y, f3.z}};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) hyp.R[3 * r + c] = (f[0][r] * e[0][c] + f[1][r] * e[1][c]) + f[2][r] * e[2][c];
            const double ca[3] = {((A[0].x + A[1].x) + A[2].x) / 3.0, ((A[0].y + A[1].y) + A[2].y) / 3.0, ((A[0].z + A[1].z) + A[2].z) / 3.0};
            const double cb[3] = {((B[0].x + B[1].x) + B[2].x) / 3.0, ((B[0].y + B[1].y) + B[2].y) / 3.0, ((B[0].z + B[1].z) + B[2].z) / 3.0};
#pragma unroll
            for (int r = 0; r < 3; ++r) hyp.t[r] = cb[r] - ((hyp.R[3 * r] * ca[0] + hyp.R[3 * r + 1] * ca[1]) + hyp.R[3 * r + 2] * ca[2]);
        }
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) hyp.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        hyp.t[0] = hyp.t[1] = hyp.t[2] = 0.0;
    }
    a.hyp[h] = hyp;
    a.table[h] = cart_ego_hypothesis{0ull, 0, ok ? 0 : 1};
}

// One correspondence under the pose (R, t): the camera-frame point q and, in front of the camera, the reprojection residual.
struct EgoRes { double qx, qy, qz, eu, ev, e2; bool inlier; };
__device__ __forceinline__ EgoRes ego_residual(const cart_ego_camera &cam, const double R[9], const double t[3], double ax, double ay, double az,
                                               double u, double v, double thr2) {
    EgoRes r;
    r.qx = ((R[0] * ax + R[1] * ay) + R[2] * az) + t[0];
    r.qy = ((R[3] * ax + R[4] * ay) + R[5] * az) + t[1];
    r.qz = ((R[6] * ax + R[7] * ay) + R[8] * az) + t[2];
    r.eu = r.ev = r.e2 = 0.0;
    r.inlier = false;
    if (r.qz <= 0) return r;
    r.eu = ((cam.fx * r.qx) / r.qz + cam.cx) - u;
    r.ev = ((cam.fy * r.qy) / r.qz + cam.cy) - v;
    r.e2 = r.eu * r.eu + r.ev * r.ev;
    r.inlier = r.e2 < thr2;
    return r;
}

__global__ __launch_bounds__(kEgoHypLanes) void ego_score_kernel(EgoArgs a) {
    __shared__ double s_c[5][kEgoTile];   // a.x, a.y, a.z, u, v
    const int n = *a.n;
    const int c0 = blockIdx.y * kEgoTile;
    if (n < 3 || c0 >= n) return;   // uniform
    const int nt = min(kEgoTile, n - c0);
    const size_t cap = (size_t)a.cap;
    for (int t = threadIdx.x; t < nt; t += kEgoHypLanes) {
        s_c[0][t] = a.corr[0 * cap + c0 + t]; s_c[1][t] = a.corr[1 * cap + c0 + t]; s_c[2][t] = a.corr[2 * cap + c0 + t];
        s_c[3][t] = a.corr[6 * cap + c0 + t]; s_c[4][t] = a.corr[7 * cap + c0 + t];
    }
    __syncthreads();
    const int h = blockIdx.x * kEgoHypLanes + threadIdx.x;
    if (h >= a.p.hypotheses || a.table[h].skipped) return;
    const EgoHyp hyp = a.hyp[h];
    const double thr2 = a.p.inlier_threshold * a.p.inlier_threshold;
    int count = 0;
    unsigned long long qerr = 0;
    for (int t = 0; t < nt; ++t) {
        const EgoRes r = ego_residual(a.cam, hyp.R, hyp.t, s_c[0][t], s_c[1][t], s_c[2][t], s_c[3][t], s_c[4][t], thr2);
        if (r.inlier) {
            ++count;
            qerr += (unsigned long long)floor((r.e2 / thr2) * kEgoQerrScale);
        }
    }
    if (count) {
        atomicAdd(&a.table[h].count, count);
        atomicAdd(reinterpret_cast<unsigned long long *>(&a.table[h].qerr), qerr);
    }
}

constexpr int kEgoSums = 27;   // 21 upper entries of J^T J (row-major, i <= j), then the 6 of J^T r

// s_red[k][l] += s_red[k][l + o] for o = 128 .. 1: entry [k][0] ends as lane 0 of the butterfly v[l] += v[l ^ o]
__device__ inline void ego_tree(double (*s_red)[kEgoLanes], int rows) {
    for (int o = kEgoLanes / 2; o > 0; o >>= 1) {
        __syncthreads();
        for (int e = threadIdx.x; e < rows * o; e += kEgoLanes) {
            const int k = e / o, l = e - k * o;
            s_red[k][l] = s_red[k][l] + s_red[k][l + o];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kEgoLanes) void ego_refine_kernel(EgoArgs a) {
    __shared__ double s_red[kEgoSums][kEgoLanes];
    __shared__ double s_pose[12];
    __shared__ unsigned long long s_bq[kEgoLanes];
    __shared__ int s_bc[kEgoLanes], s_bh[kEgoLanes];
    __shared__ int s_count, s_stop;
    const int lane = threadIdx.x;
    const int n = *a.n;
    const size_t cap = (size_t)a.cap;
    // ---- arg-max (count, -qerr, -h) over the scored hypotheses with count >= 3
    int bc = -1, bh = -1;
    unsigned long long bq = 0;
    for (int h = lane; h < a.p.hypotheses; h += kEgoLanes) {   // ascending h: a tie keeps the earlier one
        const cart_ego_hypothesis e = a.table[h];
        if (e.skipped || e.count < 3) continue;
        if (bh < 0 || e.count > bc || (e.count == bc && e.qerr < bq)) { bc = e.count; bq = e.qerr; bh = h; }
    }
    s_bc[lane] = bc; s_bq[lane] = bq; s_bh[lane] = bh;
    for (int o = kEgoLanes / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (lane < o) {
            const int c2 = s_bc[lane + o], h2 = s_bh[lane + o];
            const unsigned long long q2 = s_bq[lane + o];
            const int c1 = s_bc[lane], h1 = s_bh[lane];
            const unsigned long long q1 = s_bq[lane];
            if (h2 >= 0 && (h1 < 0 || c2 > c1 || (c2 == c1 && (q2 < q1 || (q2 == q1 && h2 < h1))))) { s_bc[lane] = c2; s_bq[lane] = q2; s_bh[lane] = h2; }
        }
    }
    __syncthreads();
    const int best = s_bh[0];
    // the mask starts as all zeros; the final inliers are set after the barriers below
    if (a.mask)
        for (int k = lane; k < a.cap; k += kEgoLanes) a.mask[k] = 0;
    if (best < 0) {   // uniform
        if (lane == 0) {
            cart_ego_result r;
            for (int k = 0; k < 9; ++k) r.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
            r.t[0] = r.t[1] = r.t[2] = 0.0;
            r.rms = 0.0;
            r.status = 0; r.n_correspondences = n; r.n_inliers = 0; r.best_hypothesis = -1;
            *a.result = r;
        }
        return;
    }
    double R[9], t[3];
    {
        const EgoHyp hyp = a.hyp[best];
        for (int k = 0; k < 9; ++k) R[k] = hyp.R[k];
        for (int k = 0; k < 3; ++k) t[k] = hyp.t[k];
    }
    const double thr2 = a.p.inlier_threshold * a.p.inlier_threshold;
    const double *ax = a.corr, *ay = a.corr + cap, *az = a.corr + 2 * cap, *cu = a.corr + 6 * cap, *cv = a.corr + 7 * cap;
    // ---- Gauss-Newton steps
    for (int it = 0; it < a.p.refine_iterations; ++it) {   // uniform
        if (lane == 0) { s_count = 0; s_stop = 0; }
        double acc[kEgoSums];
#pragma unroll
        for (int k = 0; k < kEgoSums; ++k) acc[k] = 0.0;
        int cnt = 0;
        for (int c = lane; c < n; c += kEgoLanes) {
            const EgoRes r = ego_residual(a.cam, R, t, ax[c], ay[c], az[c], cu[c], cv[c], thr2);
            if (!r.inlier) continue;
            ++cnt;
            const double au = a.cam.fx / r.qz, bu = -((a.cam.fx * r.qx) / (r.qz * r.qz));
            const double av = a.cam.fy / r.qz, bv = -((a.cam.fy * r.qy) / (r.qz * r.qz));
            const double Ju[6] = {bu * r.qy, au * r.qz - bu * r.qx, -(au * r.qy), au, 0.0, bu};
            const double Jv[6] = {bv * r.qy - av * r.qz, -(bv * r.qx), av * r.qx, 0.0, av, bv};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j, ++k) acc[k] = acc[k] + (Ju[i] * Ju[j] + Jv[i] * Jv[j]);
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + (Ju[i] * r.eu + Jv[i] * r.ev);
        }
#pragma unroll
        for (int k = 0; k < kEgoSums; ++k) s_red[k][lane] = acc[k];
        __syncthreads();   // s_count = 0 is visible
        if (cnt) atomicAdd(&s_count, cnt);
        ego_tree(s_red, kEgoSums);
        if (lane == 0) {
            bool stop = s_count < kEgoMinRefine;
            if (!stop) {
                double H[6][6], g[6], d[6];
                int k = 0;
                for (int i = 0; i < 6; ++i)
                    for (int j = i; j < 6; ++j, ++k) H[i][j] = s_red[k][0];
                for (int i = 0; i < 6; ++i) g[i] = s_red[21 + i][0];
                stop = !ego_solve6(H, g, d);
                if (!stop) {
                    double Rn[9], tn[3];
                    for (int q = 0; q < 9; ++q) Rn[q] = R[q];
                    for (int q = 0; q < 3; ++q) tn[q] = t[q];
                    ego_update(d, Rn, tn);
                    for (int q = 0; q < 9; ++q) s_pose[q] = Rn[q];
                    for (int q = 0; q < 3; ++q) s_pose[9 + q] = tn[q];
                }
            }
            s_stop = stop ? 1 : 0;
        }
        __syncthreads();
        const bool stop = s_stop != 0;
        if (!stop) {
            for (int q = 0; q < 9; ++q) R[q] = s_pose[q];
            for (int q = 0; q < 3; ++q) t[q] = s_pose[9 + q];
        }
        __syncthreads();   // everyone has read s_stop and s_pose before the next step rewrites them
        if (stop) break;   // uniform
    }
    // ---- final statistics and the mask
    if (lane == 0) s_count = 0;
    double e2sum = 0.0;
    int cnt = 0;
    __syncthreads();   // the zeros of the mask are written, s_count = 0 is visible
    for (int c = lane; c < n; c += kEgoLanes) {
        const EgoRes r = ego_residual(a.cam, R, t, ax[c], ay[c], az[c], cu[c], cv[c], thr2);
        if (!r.inlier) continue;
        ++cnt;
        e2sum = e2sum + r.e2;
        if (a.mask) a.mask[a.corr_k[c]] = 1;
    }
    s_red[0][lane] = e2sum;
    if (cnt) atomicAdd(&s_count, cnt);
    ego_tree(s_red, 1);
    if (lane == 0) {
        cart_ego_result r;
        for (int k = 0; k < 9; ++k) r.R[k] = R[k];
        for (int k = 0; k < 3; ++k) r.t[k] = t[k];
        const int inl = s_count;
        r.rms = inl ? sqrt(s_red[0][0] / (double)inl) : 0.0;
        r.status = 1; r.n_correspondences = n; r.n_inliers = inl; r.best_hypothesis = best;
        *a.result = r;
    }
}
}  // namespace

void launch_ego_triangulate(const EgoArgs &a, hipStream_t s) {
    const int blocks = (a.cap + 255) / 256;
    hipLaunchKernelGGL(ego_clear_kernel, dim3(blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ego_triangulate_kernel, dim3(blocks), dim3(256), 0, s, a);
}

void launch_ego_estimate(const EgoArgs &a, hipStream_t s) {
    const int hblocks = (a.p.hypotheses + kEgoHypLanes - 1) / kEgoHypLanes;
    hipLaunchKernelGGL(ego_compact_kernel, dim3(1), dim3(kCompactThreads), 0, s, a);
    hipLaunchKernelGGL(ego_fit_kernel, dim3(hblocks), dim3(kEgoHypLanes), 0, s, a);
    hipLaunchKernelGGL(ego_score_kernel, dim3(hblocks, (a.cap + kEgoTile - 1) / kEgoTile), dim3(kEgoHypLanes), 0, s, a);
    hipLaunchKernelGGL(ego_refine_kernel, dim3(1), dim3(kEgoLanes), 0, s, a);
}

}  // namespace cart_amd

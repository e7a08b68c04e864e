// localba_kernels.hip -- windowed bundle adjustment over the last frames (spec S32).  The launches of the calls:
//   push      local_ba_push_frame   one lane per point slot / feature: the evicted frame's column, the scratch of the push, lane 0 the ring entry
//             local_ba_push_lists   one lane per match: the stereo observation and the temporal partner of every left index
//             local_ba_push_claim   one lane per left index: the smallest index that continues a point (integer atomicMin)
//             local_ba_push_assign  one workgroup: the free slots and the new points as two stable compactions (ballot + prefix, as
//                                   ego_compact), the observations, track_of and the counts
//   optimise  local_ba_begin        one workgroup: the snapshot, cost_before, the counts of the result
//             per step: _count (usable observations per frame, integer atomics), _linearise (one lane per point slot: V_p, its Cholesky,
//             V_p^-1 and g_p), _reduce (one workgroup per block pair (a <= b) and per right-hand-side block, <= 135, S23's virtual lanes),
//             _solve (one workgroup, the reduced system in LDS, the pose updates), _update (one lane per point slot)
//             local_ba_end          one workgroup: the restore after a failed pivot or cost_after, the result
// No kernel stores the Jacobians: every kernel that needs an observation's blocks computes them again with lba_observe from the estimate the
// step linearises at, which gives the same bits everywhere and keeps the per-point memory at 12 doubles.
// IEEE double with + - * / sqrt only, every sum in the order of the spec, no FMA contraction, no floating-point atomics.  Every loop bound is
// a kernel argument clamped to the capacities; indices read from the lists are compared against them before use.

#include "ego_solve.h"
#include "engine_internal.h"
#include "warp_device.h"

#pragma clang fp contract(off)

namespace cart_amd {
namespace {

constexpr int kLbaAssignThreads = 1024;
constexpr int kLbaSolveThreads = 128;                        // one lane per row of the reduced system and its right-hand side
constexpr int kLbaMaxOrder = 6 * (kLbaMaxWindow - 1);        // 90
constexpr int kLbaTreeRows = 21;                             // sums one pass of the LDS tree reduces
static_assert(kLbaMaxOrder + 1 <= kLbaSolveThreads, "one lane per row");

__device__ __forceinline__ int lba_count(const int32_t *p, int cap) { return min(max(*p, 0), cap); }
__device__ __forceinline__ int lba_slot(int first_slot, int a, int window) { return (first_slot + a) % window; }

// ---- one observation: residual, Huber weight, Jacobians -------------------------------------------------------------------------------
struct LbaLin {
    bool front;            // q.z > 0; nothing else is set without it
    double w, rho, e[3];
    double Jc[3][6];       // d (eu, ev, er) / d (omega, upsilon) = J_q [ [q]x | -I ]
    double Jp[3][3];       // d (eu, ev, er) / d X = J_q R^T
};

__device__ __forceinline__ void lba_camera_point(const double *P, const double X[3], double q[3]) {   // q = R^T (X - t)
    const double d0 = X[0] - P[3], d1 = X[1] - P[7], d2 = X[2] - P[11];
    q[0] = (P[0] * d0 + P[4] * d1) + P[8] * d2;
    q[1] = (P[1] * d0 + P[5] * d1) + P[9] * d2;
    q[2] = (P[2] * d0 + P[6] * d1) + P[10] * d2;
}

__device__ inline LbaLin lba_observe(const cart_ego_camera &cam, const double *P, const double X[3], const LbaObs &ob, double huber) {
    LbaLin o;
    double q[3];
    lba_camera_point(P, X, q);
    o.front = q[2] > 0;
    if (!o.front) return o;
    const double qx = q[0], qy = q[1], qz = q[2];
    o.e[0] = ((cam.fx * qx) / qz + cam.cx) - (double)ob.u;
    o.e[1] = ((cam.fy * qy) / qz + cam.cy) - (double)ob.v;
    o.e[2] = ((cam.fx * (qx - cam.baseline)) / qz + cam.cx) - (double)ob.ur;
    const double n2 = (o.e[0] * o.e[0] + o.e[1] * o.e[1]) + o.e[2] * o.e[2];
    const double root = sqrt(n2);
    const bool inside = n2 <= huber * huber;
    o.w = inside ? 1.0 : huber / root;
    o.rho = inside ? n2 : (2.0 * huber) * root - huber * huber;
    const double a = cam.fx / qz, b = -((cam.fx * qx) / (qz * qz));
    const double c = cam.fy / qz, d = -((cam.fy * qy) / (qz * qz));
    const double br = -((cam.fx * (qx - cam.baseline)) / (qz * qz));
    o.Jc[0][0] = -(b * qy); o.Jc[0][1] = b * qx - a * qz; o.Jc[0][2] = a * qy; o.Jc[0][3] = -a; o.Jc[0][4] = 0.0; o.Jc[0][5] = -b;
    o.Jc[1][0] = c * qz - d * qy; o.Jc[1][1] = d * qx; o.Jc[1][2] = -(c * qx); o.Jc[1][3] = 0.0; o.Jc[1][4] = -c; o.Jc[1][5] = -d;
    o.Jc[2][0] = -(br * qy); o.Jc[2][1] = br * qx - a * qz; o.Jc[2][2] = a * qy; o.Jc[2][3] = -a; o.Jc[2][4] = 0.0; o.Jc[2][5] = -br;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        o.Jp[0][m] = a * P[4 * m] + b * P[4 * m + 2];
        o.Jp[1][m] = c * P[4 * m + 1] + d * P[4 * m + 2];
        o.Jp[2][m] = a * P[4 * m] + br * P[4 * m + 2];
    }
    return o;
}

// w ((A_u[i] B_u[j] + A_v[i] B_v[j]) + A_r[i] B_r[j]) and w ((A_u[i] eu + A_v[i] ev) + A_r[i] er)
#define LBA_JTJ(o, A, i, B, j) ((o).w * (((o).A[0][i] * (o).B[0][j] + (o).A[1][i] * (o).B[1][j]) + (o).A[2][i] * (o).B[2][j]))
#define LBA_JTE(o, A, i) ((o).w * (((o).A[0][i] * (o).e[0] + (o).A[1][i] * (o).e[1]) + (o).A[2][i] * (o).e[2]))

__device__ __forceinline__ double lba_dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// W = w J_c^T J_p, 6 x 3
__device__ __forceinline__ void lba_w_block(const LbaLin &o, double W[6][3]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) W[i][k] = LBA_JTJ(o, Jc, i, Jp, k);
}

__device__ __forceinline__ void lba_load_point(const LbaStore &g, int p, double X[3]) {
    X[0] = g.X[3 * (size_t)p]; X[1] = g.X[3 * (size_t)p + 1]; X[2] = g.X[3 * (size_t)p + 2];
}
__device__ __forceinline__ bool lba_active(const LbaStore &g, int p, int min_observations) { return g.state[p] != 0 && g.n_obs[p] >= min_observations; }
__device__ __forceinline__ bool lba_held(const LbaOptArgs &a, const int32_t *count, int age) { return age >= 1 && count[age] < a.p.min_frame_observations; }

// s_red[k][l] += s_red[k][l + o] for o = 128 .. 1: entry [k][0] ends as lane 0 of the butterfly v[l] += v[l ^ o] (ego_tree)
__device__ inline void lba_tree(double (*s_red)[kLbaLanes], int rows) {
    for (int o = kLbaLanes / 2; o > 0; o >>= 1) {
        __syncthreads();
        for (int e = threadIdx.x; e < rows * o; e += kLbaLanes) {
            const int k = e / o, l = e - k * o;
            s_red[k][l] = s_red[k][l] + s_red[k][l + o];
        }
    }
    __syncthreads();
}

// ---- push -------------------------------------------------------------------------------------------------------------------------------
struct LbaPose { double R[9], t[3]; };
__device__ inline LbaPose lba_load(const double *m) {
    LbaPose p;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.R[3 * r + c] = m[4 * r + c];
        p.t[r] = m[4 * r + 3];
    }
    return p;
}
__device__ inline void lba_store(double *m, const LbaPose &p) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m[4 * r + c] = p.R[3 * r + c];
        m[4 * r + 3] = p.t[r];
    }
}
__device__ inline LbaPose lba_inv(const LbaPose &p) {    // (R^T, -(R^T t)), S29's
    LbaPose o;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o.R[3 * r + c] = p.R[3 * c + r];
    for (int r = 0; r < 3; ++r) o.t[r] = -((o.R[3 * r] * p.t[0] + o.R[3 * r + 1] * p.t[1]) + o.R[3 * r + 2] * p.t[2]);
    return o;
}
__device__ inline LbaPose lba_mul(const LbaPose &A, const LbaPose &B) {   // S29's product
    LbaPose o;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o.R[3 * r + c] = (A.R[3 * r] * B.R[c] + A.R[3 * r + 1] * B.R[3 + c]) + A.R[3 * r + 2] * B.R[6 + c];
        o.t[r] = ((A.R[3 * r] * B.t[0] + A.R[3 * r + 1] * B.t[1]) + A.R[3 * r + 2] * B.t[2]) + A.t[r];
    }
    return o;
}

__global__ __launch_bounds__(256) void local_ba_push_frame_kernel(LbaPushArgs a) {
    const LbaStore &g = a.g;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < g.max_points) {
        LbaObs *o = g.obs + (size_t)i * g.window + a.slot;
        if (a.evict) {
            if (o->valid) {
                const int n = g.n_obs[i] - 1;
                g.n_obs[i] = n;
                if (n == 0) {
                    g.state[i] = 0;
                    g.X[3 * (size_t)i] = 0.0; g.X[3 * (size_t)i + 1] = 0.0; g.X[3 * (size_t)i + 2] = 0.0;
                    atomicAdd(g.counts + 8, 1);
                }
            }
            *o = LbaObs{0.f, 0.f, 0.f, 0};
        }
        g.claim[i] = 0x7fffffff;
    }
    if (i < g.max_features) {
        g.sobs[i] = LbaObs{0.f, 0.f, 0.f, 0};
        g.tmatch[i] = -1;
    }
    if (i == 0) {
        const size_t s = (size_t)a.slot;
        g.frame_id[s] = a.frame_id;
        for (int k = 0; k < 12; ++k) g.odom[12 * s + k] = a.pose[k];
        if (a.prev_slot < 0) {
            for (int k = 0; k < 12; ++k) g.est[12 * s + k] = a.pose[k];
        } else {
            const size_t sp = (size_t)a.prev_slot;
            lba_store(g.est + 12 * s, lba_mul(lba_load(g.est + 12 * sp), lba_mul(lba_inv(lba_load(g.odom + 12 * sp)), lba_load(a.pose))));
        }
    }
}

__global__ __launch_bounds__(256) void local_ba_push_lists_kernel(LbaPushArgs a) {
    const LbaStore &g = a.g;
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int cap = g.max_features, nl = lba_count(a.left_count, cap);
    if (k < lba_count(a.stereo_count, cap)) {
        const cart_match m = a.stereo[k];
        if (m.query >= 0 && m.query < nl && m.train >= 0 && m.train < cap) {
            const float u = a.kpL[m.query].x, v = a.kpL[m.query].y, ur = a.kpR[m.train].x;
            if ((double)u - (double)ur >= a.min_disparity) g.sobs[m.query] = LbaObs{u, v, ur, 1};   // a NaN fails
        }
    }
    if (a.prev_slot >= 0 && k < lba_count(a.temporal_count, cap)) {
        const cart_match m = a.temporal[k];
        if (m.query >= 0 && m.query < nl && m.train >= 0 && m.train < cap) g.tmatch[m.query] = m.train;
    }
}

// the point a left index would continue, -1 without: a valid observation, a temporal partner and that partner's point
__device__ __forceinline__ int lba_candidate(const LbaPushArgs &a, int i) {
    const LbaStore &g = a.g;
    if (!g.sobs[i].valid) return -1;
    const int j = g.tmatch[i];
    if (j < 0) return -1;
    const int p = g.track[a.cur ^ 1][j];
    return p >= 0 && p < g.max_points ? p : -1;
}

__global__ __launch_bounds__(256) void local_ba_push_claim_kernel(LbaPushArgs a) {
    const LbaStore &g = a.g;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= lba_count(a.left_count, g.max_features)) return;
    const int p = lba_candidate(a, i);
    if (p >= 0 && g.state[p] != 0) atomicMin(g.claim + p, i);
}

__global__ __launch_bounds__(kLbaAssignThreads) void local_ba_push_assign_kernel(LbaPushArgs a) {
    __shared__ int s_wave[kLbaAssignThreads / 64];
    __shared__ int s_base, s_valid, s_continued;
    const LbaStore &g = a.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nl = lba_count(a.left_count, g.max_features);
    if (threadIdx.x == 0) { s_base = 0; s_valid = 0; s_continued = 0; }
    __syncthreads();
    // ---- the free slots in ascending order
    for (int p0 = 0; p0 < g.max_points; p0 += kLbaAssignThreads) {   // uniform
        const int p = p0 + threadIdx.x;
        const bool is_free = p < g.max_points && g.state[p] == 0;
        const unsigned long long m = __ballot(is_free);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = s_base, total = 0;
        for (int w = 0; w < kLbaAssignThreads / 64; ++w) {
            const int n = s_wave[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (is_free) g.free_list[before + __popcll(m & ((1ull << lane) - 1))] = p;
        __syncthreads();
        if (threadIdx.x == 0) s_base += total;
        __syncthreads();
    }
    const int n_free = s_base;
    __syncthreads();
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    // ---- every left index: continue its point, take the next free slot, or drop
    const double fxb = a.cam.fx * a.cam.baseline;
    const double *est = g.est + 12 * (size_t)a.slot;
    int32_t *track = g.track[a.cur];
    for (int i0 = 0; i0 < g.max_features; i0 += kLbaAssignThreads) {   // uniform
        const int i = i0 + threadIdx.x;
        bool valid = false, continued = false;
        int p = -1;
        LbaObs ob{0.f, 0.f, 0.f, 0};
        if (i < nl) {
            ob = g.sobs[i];
            valid = ob.valid != 0;
            p = lba_candidate(a, i);
            continued = p >= 0 && g.claim[p] == i;   // a claim is only ever made on a live point
        }
        const bool is_new = valid && !continued;
        const unsigned long long m = __ballot(is_new);
        if (lane == 0) s_wave[wave] = __popcll(m);
        if (valid) atomicAdd(&s_valid, 1);
        if (continued) atomicAdd(&s_continued, 1);
        __syncthreads();
        int before = s_base, total = 0;
        for (int w = 0; w < kLbaAssignThreads / 64; ++w) {
            const int n = s_wave[w];
            before += w < wave ? n : 0;
            total += n;
        }
        int slot = -1;
        if (continued) {
            slot = p;
            g.n_obs[p] += 1;
        } else if (is_new) {
            const int r = before + __popcll(m & ((1ull << lane) - 1));
            if (r < n_free) {
                slot = g.free_list[r];
                const double u = (double)ob.u, v = (double)ob.v;
                const WarpPoint X = pose_carry(est, back_project(a.cam, fxb, u, v, u - (double)ob.ur));
                g.X[3 * (size_t)slot] = X.x; g.X[3 * (size_t)slot + 1] = X.y; g.X[3 * (size_t)slot + 2] = X.z;
                g.state[slot] = 1;
                g.n_obs[slot] = 1;
            }
        }
        if (slot >= 0) g.obs[(size_t)slot * g.window + a.slot] = ob;
        if (i < g.max_features) track[i] = slot;
        __syncthreads();
        if (threadIdx.x == 0) s_base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int n_new = s_base, born = min(n_new, n_free), freed = g.counts[8];
        const int32_t c[8] = {nl, s_valid, s_continued, born, n_new - born, freed, g.max_points - n_free + born, a.frames};
        for (int k = 0; k < 8; ++k) {
            g.counts[k] = c[k];
            if (a.counts_out) a.counts_out[k] = c[k];
        }
        g.counts[8] = 0;
    }
}

// ---- optimise ---------------------------------------------------------------------------------------------------------------------------
// sum of rho over the usable observations of the active points at the estimates P, S23's order; every thread returns the sum
__device__ inline double lba_cost(const LbaOptArgs &a, const double *P, double (*s_red)[kLbaLanes], int *n_active, int *n_observations) {
    const LbaStore &g = a.g;
    const int tid = threadIdx.x;
    double acc = 0.0;
    int na = 0, no = 0;
    for (int p = tid; p < g.max_points; p += kLbaLanes) {
        if (!lba_active(g, p, a.p.min_observations)) continue;
        ++na;
        double X[3], c = 0.0;
        lba_load_point(g, p, X);
        for (int age = 0; age < a.frames; ++age) {
            const int s = lba_slot(a.first_slot, age, g.window);
            const LbaObs ob = g.obs[(size_t)p * g.window + s];
            if (!ob.valid) continue;
            const LbaLin o = lba_observe(a.cam, P + 12 * (size_t)s, X, ob, a.p.huber);
            if (!o.front) continue;
            c = c + o.rho;
            ++no;
        }
        acc = acc + c;
    }
    s_red[0][tid] = acc;
    if (n_active) {
        if (na) atomicAdd(n_active, na);
        if (no) atomicAdd(n_observations, no);
    }
    lba_tree(s_red, 1);
    const double sum = s_red[0][0];
    __syncthreads();   // s_red may be rewritten
    return sum;
}

__global__ __launch_bounds__(kLbaLanes) void local_ba_begin_kernel(LbaOptArgs a) {
    __shared__ double s_red[1][kLbaLanes];
    __shared__ int s_active, s_observations;
    const LbaStore &g = a.g;
    const int tid = threadIdx.x;
    if (tid == 0) { s_active = 0; s_observations = 0; }
    for (int k = tid; k < 12 * g.window; k += kLbaLanes) g.snap_est[k] = g.est[k];
    for (size_t k = tid; k < 3 * (size_t)g.max_points; k += kLbaLanes) g.snap_X[k] = g.X[k];
    __syncthreads();
    const double cost = lba_cost(a, g.est, s_red, &s_active, &s_observations);
    if (tid == 0) {
        LbaControl c;
        c.fail = 0;
        c.skip = (a.frames < 2 || s_active == 0) ? 1 : 0;
        c.n_active = s_active; c.n_observations = s_observations; c.n_held = 0;
        for (int k = 0; k < kLbaMaxWindow; ++k) c.count[0][k] = c.count[1][k] = 0;
        c.pad = 0;
        c.cost_before = cost;
        *g.ctl = c;
    }
}

__global__ __launch_bounds__(256) void local_ba_count_kernel(LbaOptArgs a, int step) {
    __shared__ int s_count[kLbaMaxWindow];
    const LbaStore &g = a.g;
    if (g.ctl->fail | g.ctl->skip) return;   // uniform
    const int tid = threadIdx.x, p = blockIdx.x * 256 + tid;
    if (tid < kLbaMaxWindow) s_count[tid] = 0;
    if (blockIdx.x == 0) {   // nobody reads these two in this launch
        for (int k = tid; k < 12 * g.window; k += 256) g.lin_est[k] = g.est[k];
        if (tid < kLbaMaxWindow) g.ctl->count[(step + 1) & 1][tid] = 0;
    }
    __syncthreads();
    if (p < g.max_points && lba_active(g, p, a.p.min_observations)) {
        double X[3], q[3];
        lba_load_point(g, p, X);
        for (int age = 1; age < a.frames; ++age) {
            const int s = lba_slot(a.first_slot, age, g.window);
            if (!g.obs[(size_t)p * g.window + s].valid) continue;
            lba_camera_point(g.est + 12 * (size_t)s, X, q);
            if (q[2] > 0) atomicAdd(&s_count[age], 1);
        }
    }
    __syncthreads();
    if (tid >= 1 && tid < a.frames && s_count[tid]) atomicAdd(&g.ctl->count[step & 1][tid], s_count[tid]);
}

__global__ __launch_bounds__(256) void local_ba_linearise_kernel(LbaOptArgs a, int step) {
    const LbaStore &g = a.g;
    if (g.ctl->fail | g.ctl->skip) return;   // uniform
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.max_points) return;
    if (!lba_active(g, p, a.p.min_observations)) {
        g.used[p] = 0;
        return;
    }
    const int32_t *count = g.ctl->count[step & 1];
    double X[3], V[3][3], gp[3];
    lba_load_point(g, p, X);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gp[k] = 0.0;
#pragma unroll
        for (int l = 0; l < 3; ++l) V[k][l] = 0.0;
    }
    unsigned used = 0;
    for (int age = 0; age < a.frames; ++age) {   // the frames in age order
        if (lba_held(a, count, age)) continue;
        const int s = lba_slot(a.first_slot, age, g.window);
        const LbaObs ob = g.obs[(size_t)p * g.window + s];
        if (!ob.valid) continue;
        const LbaLin o = lba_observe(a.cam, g.lin_est + 12 * (size_t)s, X, ob, a.p.huber);
        if (!o.front) continue;
        used |= 1u << age;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int l = k; l < 3; ++l) V[k][l] = V[k][l] + LBA_JTJ(o, Jp, k, Jp, l);
            gp[k] = gp[k] + LBA_JTE(o, Jp, k);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) V[k][k] = V[k][k] + a.p.damping;
    // the 3 x 3 unpivoted Cholesky, ego_solve6's order
    double L[3][3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double s = V[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0)) ok = false;
        L[j][j] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 3; ++i) {
            s = V[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    if (ok) used |= 1u << kLbaInBit;
    g.used[p] = (int32_t)used;
    if (!ok) return;
    const size_t M = (size_t)g.max_points;
#pragma unroll
    for (int c = 0; c < 3; ++c) {   // column c of V^-1: L L^T x = e_c
        double y[3], x[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double s = i == c ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
            y[i] = s / L[i][i];
        }
#pragma unroll
        for (int i = 2; i >= 0; --i) {
            double s = y[i];
#pragma unroll
            for (int k = i + 1; k < 3; ++k) s = s - L[k][i] * x[k];
            x[i] = s / L[i][i];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) g.blocks[(size_t)(3 * r + c) * M + p] = x[r];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) g.blocks[(size_t)(9 + k) * M + p] = gp[k];
}

// the lanes' sums acc[0 .. n) -> lane 0 of the butterfly, kLbaTreeRows at a time; thread k < n of a pass ends with its sum in out
template <int N>
__device__ inline void lba_reduce_rows(const double (&acc)[N], double (*s_red)[kLbaLanes], double *s_out) {
#pragma unroll
    for (int r0 = 0; r0 < N; r0 += kLbaTreeRows) {
        const int rows = N - r0 < kLbaTreeRows ? N - r0 : kLbaTreeRows;
#pragma unroll
        for (int k = 0; k < kLbaTreeRows; ++k)
            if (r0 + k < N) s_red[k][threadIdx.x] = acc[r0 + k];
        lba_tree(s_red, rows);
        if ((int)threadIdx.x < rows) s_out[r0 + threadIdx.x] = s_red[threadIdx.x][0];
        __syncthreads();
    }
}

__device__ __forceinline__ void lba_load_vinv(const LbaStore &g, int p, double Vi[3][3]) {
    const size_t M = (size_t)g.max_points;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Vi[r][c] = g.blocks[(size_t)(3 * r + c) * M + p];
}

// Y = W V^-1, 6 x 3
__device__ __forceinline__ void lba_y_block(const double W[6][3], const double Vi[3][3], double Y[6][3]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) Y[i][k] = (W[i][0] * Vi[0][k] + W[i][1] * Vi[1][k]) + W[i][2] * Vi[2][k];
}

// block pair (age_a <= age_b) of the reduced system: S_ab = delta_ab U_a - sum_p Y_a W_b^T into the lower entries of g.S
template <bool kDiag>
__device__ inline void lba_reduce_pair(const LbaOptArgs &a, int step, int age_a, int age_b, double (*s_red)[kLbaLanes], double *s_out) {
    constexpr int kT = kDiag ? 21 : 36, kN = kDiag ? 42 : 36;   // T (upper entries on the diagonal block), then U
    const LbaStore &g = a.g;
    const int sa = lba_slot(a.first_slot, age_a, g.window), sb = lba_slot(a.first_slot, age_b, g.window);
    const unsigned need = (1u << kLbaInBit) | (1u << age_a) | (1u << age_b);
    double acc[kN];
#pragma unroll
    for (int k = 0; k < kN; ++k) acc[k] = 0.0;
    for (int p = threadIdx.x; p < g.max_points; p += kLbaLanes) {
        if (((unsigned)g.used[p] & need) != need) continue;
        double X[3], Vi[3][3], Wa[6][3], Wb[6][3], Y[6][3];
        lba_load_point(g, p, X);
        lba_load_vinv(g, p, Vi);
        const LbaLin oa = lba_observe(a.cam, g.lin_est + 12 * (size_t)sa, X, g.obs[(size_t)p * g.window + sa], a.p.huber);
        lba_w_block(oa, Wa);
        lba_y_block(Wa, Vi, Y);
        if constexpr (kDiag) {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j, ++k) {
                    acc[k] = acc[k] + lba_dot3(Y[i], Wa[j]);
                    acc[kT + k] = acc[kT + k] + LBA_JTJ(oa, Jc, i, Jc, j);
                }
        } else {
            const LbaLin ob = lba_observe(a.cam, g.lin_est + 12 * (size_t)sb, X, g.obs[(size_t)p * g.window + sb], a.p.huber);
            lba_w_block(ob, Wb);
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) acc[6 * i + j] = acc[6 * i + j] + lba_dot3(Y[i], Wb[j]);
        }
    }
    lba_reduce_rows<kN>(acc, s_red, s_out);
    const int n = 6 * (g.window - 1);
    const bool held = kDiag && lba_held(a, g.ctl->count[step & 1], age_a);
    if ((int)threadIdx.x < kT) {
        int i, j;
        if constexpr (kDiag) {
            int k = threadIdx.x;
            for (i = 0; k >= 6 - i; ++i) k -= 6 - i;
            j = i + k;
        } else {
            i = threadIdx.x / 6; j = threadIdx.x % 6;
        }
        double v;
        if constexpr (kDiag) {
            double u = s_out[kT + threadIdx.x];
            if (i == j) u = u + a.p.damping;
            v = u - s_out[threadIdx.x];
            if (held && i == j) v = 1.0;   // a held frame's block is the identity
        } else {
            v = 0.0 - s_out[threadIdx.x];
        }
        g.S[(size_t)(6 * (age_b - 1) + j) * n + 6 * (age_a - 1) + i] = v;
    }
}

__global__ __launch_bounds__(kLbaLanes) void local_ba_reduce_kernel(LbaOptArgs a, int step) {
    __shared__ double s_red[kLbaTreeRows][kLbaLanes];
    __shared__ double s_out[42];
    const LbaStore &g = a.g;
    if (g.ctl->fail | g.ctl->skip) return;   // uniform
    const int nf = a.frames - 1, n_pairs = nf * (nf + 1) / 2;
    int b = blockIdx.x;
    if (b < n_pairs) {   // uniform: pair (age_a, age_b), age_a <= age_b, rows of age_a first
        int age_a = 1;
        while (b >= nf - (age_a - 1)) { b -= nf - (age_a - 1); ++age_a; }
        const int age_b = age_a + b;
        if (age_a == age_b) lba_reduce_pair<true>(a, step, age_a, age_b, s_red, s_out);
        else lba_reduce_pair<false>(a, step, age_a, age_b, s_red, s_out);
        return;
    }
    // the right-hand side of one frame: r_a = -g_a + sum_p Y_a g_p
    const int age = 1 + (b - n_pairs);
    if (age >= a.frames) return;
    const int sa = lba_slot(a.first_slot, age, g.window);
    const unsigned need = (1u << kLbaInBit) | (1u << age);
    const size_t M = (size_t)g.max_points;
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (int p = threadIdx.x; p < g.max_points; p += kLbaLanes) {
        if (((unsigned)g.used[p] & need) != need) continue;
        double X[3], Vi[3][3], Wa[6][3], Y[6][3];
        lba_load_point(g, p, X);
        lba_load_vinv(g, p, Vi);
        const double gp[3] = {g.blocks[9 * M + p], g.blocks[10 * M + p], g.blocks[11 * M + p]};
        const LbaLin oa = lba_observe(a.cam, g.lin_est + 12 * (size_t)sa, X, g.obs[(size_t)p * g.window + sa], a.p.huber);
        lba_w_block(oa, Wa);
        lba_y_block(Wa, Vi, Y);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            acc[i] = acc[i] + LBA_JTE(oa, Jc, i);
            acc[6 + i] = acc[6 + i] + lba_dot3(Y[i], gp);
        }
    }
    lba_reduce_rows<12>(acc, s_red, s_out);
    const int n = 6 * (g.window - 1);
    if (threadIdx.x < 6) g.S[(size_t)(6 * (a.frames - 1)) * n + 6 * (age - 1) + threadIdx.x] = (-s_out[threadIdx.x]) + s_out[6 + threadIdx.x];
}

// S delta = r by the unpivoted Cholesky of S29's loop system: left-looking, row tid, the right-hand side rides along as the last row; every
// row recomputes the pivot of the column, so one barrier per column.  Then the poses move.
__global__ __launch_bounds__(kLbaSolveThreads) void local_ba_solve_kernel(LbaOptArgs a, int step) {
    __shared__ double s_l[(kLbaMaxOrder + 1) * (kLbaMaxOrder + 2) / 2];   // lower entries by rows: (i, j) at i (i + 1) / 2 + j
    __shared__ double s_diag[kLbaMaxOrder], s_y[kLbaMaxOrder];
    __shared__ int s_fail;
    const LbaStore &g = a.g;
    if (g.ctl->fail | g.ctl->skip) return;   // uniform
    const int tid = threadIdx.x;
    const int n = 6 * (a.frames - 1), ld = 6 * (g.window - 1);
    if (tid == 0) s_fail = 0;
    if (tid <= n)
        for (int j = 0; j <= min(tid, n - 1); ++j) s_l[tid * (tid + 1) / 2 + j] = g.S[(size_t)tid * ld + j];
    __syncthreads();
    for (int j = 0; j < n; ++j) {   // uniform
        if (tid >= j && tid <= n) {
            const double *rj = s_l + j * (j + 1) / 2, *ri = s_l + tid * (tid + 1) / 2;
            double sd = rj[j], s = tid > j ? ri[j] : 0.0;
            for (int k = 0; k < j; ++k) {
                const double ljk = rj[k];
                sd = sd - ljk * ljk;
                if (tid > j) s = s - ri[k] * ljk;
            }
            const double d = sqrt(sd);
            if (tid == j) {
                if (!(sd > 0)) s_fail = 1;
                s_diag[j] = d;
            } else {
                s_l[tid * (tid + 1) / 2 + j] = s / d;
            }
        }
        __syncthreads();
    }
    if (s_fail) {   // uniform
        if (tid == 0) g.ctl->fail = 1;
        return;
    }
    double s = tid < n ? s_l[n * (n + 1) / 2 + tid] : 0.0;   // L^T y = w, column by column from the last
    for (int k = n - 1; k >= 0; --k) {   // uniform
        if (tid == k) s_y[k] = s / s_diag[k];
        __syncthreads();
        if (tid < k) s = s - s_l[k * (k + 1) / 2 + tid] * s_y[k];
    }
    __syncthreads();
    if (tid < n) g.delta[tid] = s_y[tid];
    const int32_t *count = g.ctl->count[step & 1];
    if (tid >= 1 && tid < a.frames && !lba_held(a, count, tid)) {   // one lane per free frame
        double d[6], R[9], t[3];
        for (int r = 0; r < 6; ++r) d[r] = s_y[6 * (tid - 1) + r];
        double *m = g.est + 12 * (size_t)lba_slot(a.first_slot, tid, g.window);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R[3 * r + c] = m[4 * r + c];
            t[r] = m[4 * r + 3];
        }
        ego_update_right(d, R, t);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) m[4 * r + c] = R[3 * r + c];
            m[4 * r + 3] = t[r];
        }
    }
    if (tid == 0) {
        int held = 0;
        for (int age = 1; age < a.frames; ++age) held += lba_held(a, count, age) ? 1 : 0;
        g.ctl->n_held += held;
    }
}

// dX_p = V_p^-1 (-g_p - sum_a W_pa^T delta_a), a ascending
__global__ __launch_bounds__(256) void local_ba_update_kernel(LbaOptArgs a) {
    const LbaStore &g = a.g;
    if (g.ctl->fail | g.ctl->skip) return;   // uniform
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.max_points) return;
    const unsigned used = (unsigned)g.used[p];
    if (!(used >> kLbaInBit)) return;
    const size_t M = (size_t)g.max_points;
    double X[3], Vi[3][3], h[3];
    lba_load_point(g, p, X);
    lba_load_vinv(g, p, Vi);
#pragma unroll
    for (int k = 0; k < 3; ++k) h[k] = -g.blocks[(size_t)(9 + k) * M + p];
    for (int age = 1; age < a.frames; ++age) {
        if (!((used >> age) & 1u)) continue;
        const int s = lba_slot(a.first_slot, age, g.window);
        const LbaLin o = lba_observe(a.cam, g.lin_est + 12 * (size_t)s, X, g.obs[(size_t)p * g.window + s], a.p.huber);
        double W[6][3];
        lba_w_block(o, W);
        const double *d = g.delta + 6 * (age - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double sum = W[0][k] * d[0];
#pragma unroll
            for (int i = 1; i < 6; ++i) sum = sum + W[i][k] * d[i];
            h[k] = h[k] - sum;
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) g.X[3 * (size_t)p + r] = X[r] + lba_dot3(Vi[r], h);
}

__global__ __launch_bounds__(kLbaLanes) void local_ba_end_kernel(LbaOptArgs a) {
    __shared__ double s_red[1][kLbaLanes];
    const LbaStore &g = a.g;
    const int tid = threadIdx.x;
    const LbaControl c = *g.ctl;
    double cost_after = c.cost_before;
    if (c.fail) {   // uniform
        for (int k = tid; k < 12 * g.window; k += kLbaLanes) g.est[k] = g.snap_est[k];
        for (size_t k = tid; k < 3 * (size_t)g.max_points; k += kLbaLanes) g.X[k] = g.snap_X[k];
    } else if (!c.skip) {
        cost_after = lba_cost(a, g.est, s_red, nullptr, nullptr);
    }
    if (tid == 0 && a.result)
        *a.result = cart_local_ba_result{c.fail ? 0 : 1, a.frames, c.n_active, c.n_observations, c.fail ? 0 : c.n_held, a.p.iterations, c.cost_before, cost_after};
}

__global__ __launch_bounds__(256) void local_ba_poses_kernel(LbaStore g, int frames, int first_slot, double *out, uint64_t *ids_out) {
    const int k = threadIdx.x;
    if (k >= 12 * g.window) return;
    const int age = k / 12;
    const size_t s = (size_t)lba_slot(first_slot, age, g.window);
    out[k] = age < frames ? g.est[12 * s + k % 12] : 0.0;
    if (ids_out && k % 12 == 0) ids_out[age] = age < frames ? g.frame_id[s] : 0ull;
}

__global__ __launch_bounds__(256) void local_ba_points_kernel(LbaStore g, double *out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.max_points) return;
    const bool live = g.state[p] != 0;
    double *o = out + 4 * (size_t)p;
    for (int k = 0; k < 3; ++k) o[k] = live ? g.X[3 * (size_t)p + k] : 0.0;
    o[3] = live ? (double)g.n_obs[p] : 0.0;
}
}  // namespace

void launch_local_ba_push(const LbaPushArgs &a, hipStream_t s) {
    const int n = a.g.max_points > a.g.max_features ? a.g.max_points : a.g.max_features;
    const int fblocks = (a.g.max_features + 255) / 256;
    hipLaunchKernelGGL(local_ba_push_frame_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(local_ba_push_lists_kernel, dim3(fblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(local_ba_push_claim_kernel, dim3(fblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(local_ba_push_assign_kernel, dim3(1), dim3(kLbaAssignThreads), 0, s, a);
}

void launch_local_ba_optimize(const LbaOptArgs &a, hipStream_t s) {
    const int pblocks = (a.g.max_points + 255) / 256;
    const int nf = a.frames > 1 ? a.frames - 1 : 1;
    hipLaunchKernelGGL(local_ba_begin_kernel, dim3(1), dim3(kLbaLanes), 0, s, a);
    for (int step = 0; step < a.p.iterations; ++step) {
        hipLaunchKernelGGL(local_ba_count_kernel, dim3(pblocks), dim3(256), 0, s, a, step);
        hipLaunchKernelGGL(local_ba_linearise_kernel, dim3(pblocks), dim3(256), 0, s, a, step);
        hipLaunchKernelGGL(local_ba_reduce_kernel, dim3(nf * (nf + 1) / 2 + nf), dim3(kLbaLanes), 0, s, a, step);
        hipLaunchKernelGGL(local_ba_solve_kernel, dim3(1), dim3(kLbaSolveThreads), 0, s, a, step);
        hipLaunchKernelGGL(local_ba_update_kernel, dim3(pblocks), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(local_ba_end_kernel, dim3(1), dim3(kLbaLanes), 0, s, a);
}

void launch_local_ba_poses(const LbaStore &g, int frames, int first_slot, double *out, uint64_t *ids_out, hipStream_t s) {
    hipLaunchKernelGGL(local_ba_poses_kernel, dim3(1), dim3(256), 0, s, g, frames, first_slot, out, ids_out);
}

void launch_local_ba_points(const LbaStore &g, double *out, hipStream_t s) {
    hipLaunchKernelGGL(local_ba_points_kernel, dim3((g.max_points + 255) / 256), dim3(256), 0, s, g, out);
}

}  // namespace cart_amd

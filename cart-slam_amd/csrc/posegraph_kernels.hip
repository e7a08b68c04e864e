// posegraph_kernels.hip -- pose-graph optimisation over keyframes (spec S29), three kernels:
//   pose_graph_add_node / pose_graph_add_loop   one lane: the node's estimate and its odometry edge / the loop edge, from kernel arguments
//   pose_graph_optimize   one persistent workgroup of kPgThreads for all Gauss-Newton steps.  Per step: one lane per edge linearises; lane 0
//                  factors the block-tridiagonal chain node by node and hands every node's blocks through LDS (two buffers) to the column lanes
//                  (one per right-hand side: b and the 6 columns of every loop edge), which substitute forward one node behind it; the back
//                  substitution reads the factor with broadcast loads and needs no barrier; then the loop system C = I + U^T Z is assembled,
//                  factored left-looking with one row per lane and one barrier per column (its right-hand side rides along as an extra row, which
//                  is the forward solve), solved backwards with one barrier per column, and the correction and the update are applied.
// IEEE double with + - * / sqrt only, every sum in the order of the spec, no FMA contraction, no atomics.  Every loop bound is a kernel
// argument clamped to the capacities; the indices a, b of a loop edge are compared, never used as a bound.

#include "ego_solve.h"
#include "engine_internal.h"

#pragma clang fp contract(off)

namespace cart_amd {
namespace {

constexpr int kPgThreads = 512;
constexpr int kPgCostLanes = 256;                  // S23's virtual lanes
constexpr int kPgFirstColumnLane = 64;             // wave 0 factors, the column lanes start with wave 1
constexpr int kPgMaxColumns = 1 + 6 * kPgMaxLoops; // 385 <= kPgThreads - kPgFirstColumnLane
static_assert(kPgMaxColumns <= kPgThreads - kPgFirstColumnLane, "one lane per column");
static_assert(6 * kPgMaxLoops + 1 <= kPgThreads, "one lane per row of the loop system");

struct PgPose { double R[9], t[3]; };

__device__ inline PgPose pg_load(const double *m) {   // 3 x 4 in row order
    PgPose p;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.R[3 * r + c] = m[4 * r + c];
        p.t[r] = m[4 * r + 3];
    }
    return p;
}
__device__ inline void pg_store(double *m, const PgPose &p) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m[4 * r + c] = p.R[3 * r + c];
        m[4 * r + 3] = p.t[r];
    }
}
__device__ inline void pg_mat3(const double A[9], const double B[9], double out[9]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
__device__ inline PgPose pg_inv(const PgPose &p) {    // (R^T, -(R^T t))
    PgPose o;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o.R[3 * r + c] = p.R[3 * c + r];
    for (int r = 0; r < 3; ++r) o.t[r] = -((o.R[3 * r] * p.t[0] + o.R[3 * r + 1] * p.t[1]) + o.R[3 * r + 2] * p.t[2]);
    return o;
}
__device__ inline PgPose pg_mul(const PgPose &A, const PgPose &B) {
    PgPose o;
    pg_mat3(A.R, B.R, o.R);
    for (int r = 0; r < 3; ++r) o.t[r] = ((A.R[3 * r] * B.t[0] + A.R[3 * r + 1] * B.t[1]) + A.R[3 * r + 2] * B.t[2]) + A.t[r];
    return o;
}

// edge number e of the cost order: the odometry edges (n - 1, n) for n = 1 .. n_nodes - 1, then the loops
__device__ inline const PgEdge &pg_edge(const PoseGraphStore &g, int n_nodes, int e) {
    return e < n_nodes - 1 ? g.edges[e + 1] : g.edges[g.max_nodes + (e - (n_nodes - 1))];
}

struct PgResidual { double Re[9], r[6]; };   // r = (rho, tau)

__device__ inline PgResidual pg_residual(const PgEdge &ed, const double *est) {
    PgPose M;
    for (int k = 0; k < 9; ++k) M.R[k] = ed.R[k];
    for (int k = 0; k < 3; ++k) M.t[k] = ed.t[k];
    const PgPose E = pg_mul(M, pg_mul(pg_inv(pg_load(est + 12 * (size_t)ed.a)), pg_load(est + 12 * (size_t)ed.b)));
    PgResidual o;
    for (int k = 0; k < 9; ++k) o.Re[k] = E.R[k];
    o.r[0] = 0.5 * (E.R[7] - E.R[5]);
    o.r[1] = 0.5 * (E.R[2] - E.R[6]);
    o.r[2] = 0.5 * (E.R[3] - E.R[1]);
    for (int k = 0; k < 3; ++k) o.r[3 + k] = E.t[k];
    return o;
}

__device__ inline double pg_cost_term(const PgEdge &ed, const double r[6]) {
    return ed.w_rot * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + ed.w_trans * ((r[3] * r[3] + r[4] * r[4]) + r[5] * r[5]);
}

// sum over the edges in S23's order: lane l adds edges l, l + 256, ..., then the halving tree; every thread returns the sum
__device__ inline double pg_cost(const PoseGraphStore &g, int n_nodes, int n_edges, double *s_red) {
    const int tid = threadIdx.x;
    if (tid < kPgCostLanes) {
        double acc = 0.0;
        for (int e = tid; e < n_edges; e += kPgCostLanes) {
            const PgEdge &ed = pg_edge(g, n_nodes, e);
            const PgResidual res = pg_residual(ed, g.est);
            acc = acc + pg_cost_term(ed, res.r);
        }
        s_red[tid] = acc;
    }
    for (int o = kPgCostLanes / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (tid < o) s_red[tid] = s_red[tid] + s_red[tid + o];
    }
    __syncthreads();
    const double sum = s_red[0];
    __syncthreads();   // s_red may be rewritten
    return sum;
}

// sum over k ascending of (X[k][r] w_k) Y[k][c], w_k = w_rot for the three rotation rows, w_trans for the others
__device__ inline double pg_wdot(const double X[6][6], int r, const double Y[6][6], int c, double w_rot, double w_trans) {
    double s = (X[0][r] * w_rot) * Y[0][c];
    for (int k = 1; k < 6; ++k) s = s + (X[k][r] * (k < 3 ? w_rot : w_trans)) * Y[k][c];
    return s;
}
__device__ inline double pg_wdotv(const double X[6][6], int r, const double v[6], double w_rot, double w_trans) {
    double s = (X[0][r] * w_rot) * v[0];
    for (int k = 1; k < 6; ++k) s = s + (X[k][r] * (k < 3 ? w_rot : w_trans)) * v[k];
    return s;
}

// the two Jacobian blocks of an edge at its residual (first order): d r / d delta_a and d r / d delta_b for the right perturbation
__device__ inline void pg_jacobians(const PgEdge &ed, const PgResidual &res, double Ja[6][6], double Jb[6][6]) {
    const double *Re = res.Re, *te = res.r + 3;
    const double tr = (Re[0] + Re[4]) + Re[8];
    double A11[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double d = r == c ? tr : 0.0;
            Jb[r][c] = 0.5 * (d - Re[3 * c + r]);
            Jb[r][3 + c] = 0.0;
            Jb[3 + r][c] = 0.0;
            Jb[3 + r][3 + c] = Re[3 * r + c];
            A11[3 * r + c] = 0.5 * (d - Re[3 * r + c]);
        }
    const double A21[9] = {0.0, te[2], -te[1], -te[2], 0.0, te[0], te[1], -te[0], 0.0};            // -[t_e]x
    const double K[9] = {0.0, -ed.t[2], ed.t[1], ed.t[2], 0.0, -ed.t[0], -ed.t[1], ed.t[0], 0.0};  // [t_m]x
    double TL[9], P[9], Q[9];
    pg_mat3(A11, ed.R, TL);
    pg_mat3(A21, ed.R, P);
    pg_mat3(K, ed.R, Q);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            Ja[r][c] = -TL[3 * r + c];
            Ja[r][3 + c] = 0.0;
            Ja[3 + r][c] = -(P[3 * r + c] + Q[3 * r + c]);
            Ja[3 + r][3 + c] = -ed.R[3 * r + c];
        }
}

__global__ __launch_bounds__(64) void pose_graph_add_node_kernel(PoseGraphNodeArgs a) {
    if (threadIdx.x != 0 || a.n < 0 || a.n >= a.g.max_nodes) return;
    const size_t n = (size_t)a.n;
    for (int k = 0; k < 12; ++k) a.g.odom[12 * n + k] = a.pose[k];
    if (a.n == 0) {
        for (int k = 0; k < 12; ++k) a.g.est[k] = a.pose[k];
        return;
    }
    const PgPose cur = pg_load(a.pose), prev = pg_load(a.g.odom + 12 * (n - 1));
    pg_store(a.g.est + 12 * n, pg_mul(pg_load(a.g.est + 12 * (n - 1)), pg_mul(pg_inv(prev), cur)));
    const PgPose M = pg_mul(pg_inv(cur), prev);
    PgEdge e;
    for (int k = 0; k < 9; ++k) e.R[k] = M.R[k];
    for (int k = 0; k < 3; ++k) e.t[k] = M.t[k];
    e.w_rot = a.w_rot; e.w_trans = a.w_trans;
    e.a = a.n - 1; e.b = a.n; e.pad[0] = e.pad[1] = 0;
    a.g.edges[n] = e;
}

__global__ __launch_bounds__(64) void pose_graph_add_loop_kernel(PoseGraphLoopArgs a) {
    if (threadIdx.x != 0 || a.e < 0 || a.e >= a.g.max_loops) return;
    a.g.edges[(size_t)a.g.max_nodes + a.e] = a.edge;
}

__global__ __launch_bounds__(kPgThreads) void pose_graph_optimize_kernel(PoseGraphArgs a) {
    __shared__ double s_fac[2][kPgFacDoubles];
    __shared__ double s_red[kPgCostLanes];
    __shared__ double s_y[6 * kPgMaxLoops];
    __shared__ int s_fail;
    const PoseGraphStore &g = a.g;
    const int tid = threadIdx.x;
    const int N = min(max(a.n_nodes, 0), g.max_nodes), L = min(max(a.n_loops, 0), g.max_loops);
    const int iterations = min(max(a.iterations, 0), kPgMaxIterations);
    const int n_edges = N > 1 ? (N - 1) + L : 0;
    if (n_edges == 0) {   // uniform: one node or none, nothing to do
        if (tid == 0 && a.result) *a.result = cart_pose_graph_result{1, N, L, iterations, 0.0, 0.0};
        return;
    }
    const int M = 6 * L, ncols = 1 + M;              // the loop system's order, the right-hand sides of the chain
    const size_t ldw = 1 + 6 * (size_t)g.max_loops;  // doubles per row of the column workspace
    const size_t ldc = 6 * (size_t)g.max_loops + 1;  // rows per column of lc: row M is the right-hand side
    const size_t ldr = 6 * (size_t)g.max_loops;
    if (tid == 0) s_fail = 0;
    for (int k = tid; k < 12 * N; k += kPgThreads) g.snap[k] = g.est[k];
    const double cost_before = pg_cost(g, N, n_edges, s_red);   // its barriers order the snapshot and s_fail too
    bool failed = false;

    for (int it = 0; it < iterations; ++it) {   // uniform
        // ---- 1. linearisation: one lane per edge
        for (int e = tid; e < n_edges; e += kPgThreads) {
            const PgEdge ed = pg_edge(g, N, e);
            const PgResidual res = pg_residual(ed, g.est);
            double Ja[6][6], Jb[6][6];
            pg_jacobians(ed, res, Ja, Jb);
            if (e < N - 1) {
                double *o = g.lin + (size_t)(e + 1) * kPgLinDoubles;
                for (int r = 0; r < 6; ++r)
                    for (int c = 0; c < 6; ++c) {
                        o[6 * r + c] = pg_wdot(Ja, r, Ja, c, ed.w_rot, ed.w_trans);
                        o[36 + 6 * r + c] = pg_wdot(Jb, r, Jb, c, ed.w_rot, ed.w_trans);
                        o[72 + 6 * r + c] = pg_wdot(Jb, r, Ja, c, ed.w_rot, ed.w_trans);
                    }
                for (int r = 0; r < 6; ++r) {
                    o[108 + r] = pg_wdotv(Ja, r, res.r, ed.w_rot, ed.w_trans);
                    o[114 + r] = pg_wdotv(Jb, r, res.r, ed.w_rot, ed.w_trans);
                }
            } else {
                double *o = g.lin_loop + (size_t)(e - (N - 1)) * kPgLoopDoubles;
                const double sr = sqrt(ed.w_rot), st = sqrt(ed.w_trans);
                for (int k = 0; k < 6; ++k)
                    for (int c = 0; c < 6; ++c) {
                        o[6 * k + c] = Ja[c][k] * (c < 3 ? sr : st);
                        o[36 + 6 * k + c] = Jb[c][k] * (c < 3 ? sr : st);
                    }
                for (int r = 0; r < 6; ++r) {
                    o[72 + r] = pg_wdotv(Ja, r, res.r, ed.w_rot, ed.w_trans);
                    o[78 + r] = pg_wdotv(Jb, r, res.r, ed.w_rot, ed.w_trans);
                }
            }
        }
        __syncthreads();
        // ---- 2. the right-hand side b = -gradient into column 0: the node's two odometry edges, then the loops in their order
        for (int k = tid; k < 6 * (N - 1); k += kPgThreads) {
            const int i = 1 + k / 6, r = k % 6;
            double s = g.lin[(size_t)i * kPgLinDoubles + 114 + r];
            if (i + 1 < N) s = s + g.lin[(size_t)(i + 1) * kPgLinDoubles + 108 + r];
            for (int e = 0; e < L; ++e) {
                const PgEdge &ed = g.edges[(size_t)g.max_nodes + e];
                if (ed.a == i) s = s + g.lin_loop[(size_t)e * kPgLoopDoubles + 72 + r];
                if (ed.b == i) s = s + g.lin_loop[(size_t)e * kPgLoopDoubles + 78 + r];
            }
            g.cols[(size_t)(6 * i + r) * ldw] = -s;
        }
        __syncthreads();
        // ---- 3. the chain: lane 0 factors node `step`, the column lanes substitute node `step - 1` forward
        const int col = tid - kPgFirstColumnLane;
        const bool column_lane = col >= 0 && col < ncols;
        int la = -1, lb = -1;                 // the nodes of this lane's loop edge
        double ua[6], ub[6];                  // its column of the U blocks there
        for (int k = 0; k < 6; ++k) ua[k] = ub[k] = 0.0;
        if (column_lane && col > 0) {
            const int e = (col - 1) / 6, c = (col - 1) % 6;
            const PgEdge &ed = g.edges[(size_t)g.max_nodes + e];
            la = ed.a; lb = ed.b;
            for (int k = 0; k < 6; ++k) {
                ua[k] = g.lin_loop[(size_t)e * kPgLoopDoubles + 6 * k + c];
                ub[k] = g.lin_loop[(size_t)e * kPgLoopDoubles + 36 + 6 * k + c];
            }
        }
        double Lp[6][6], invp[6];             // lane 0: the previous node's diagonal block
        double y[6];                          // column lanes: the previous node's solution
        for (int r = 0; r < 6; ++r) {
            y[r] = 0.0; invp[r] = 0.0;
            for (int c = 0; c < 6; ++c) Lp[r][c] = 0.0;
        }
        for (int step = 1; step <= N; ++step) {   // uniform
            if (tid == 0 && step < N) {
                const double *lin = g.lin + (size_t)step * kPgLinDoubles;
                double Mb[6][6];
                for (int r = 0; r < 6; ++r)
                    for (int c = 0; c < 6; ++c) Mb[r][c] = 0.0;
                if (step >= 2)   // the sub-diagonal block: M L_prev^T = T_{step, step - 1}
                    for (int r = 0; r < 6; ++r)
                        for (int c = 0; c < 6; ++c) {
                            double m = lin[72 + 6 * r + c];
                            for (int k = 0; k < c; ++k) m = m - Mb[r][k] * Lp[c][k];
                            Mb[r][c] = m * invp[c];
                        }
                // S = T_{step, step} - M M^T, an entry (r, c >= r) at a time: the node's own edge, the next edge, then the six products
                const auto S = [&](int r, int c) {
                    double s = lin[36 + 6 * r + c];
                    if (step + 1 < N) s = s + lin[kPgLinDoubles + 6 * r + c];
                    if (step >= 2)
                        for (int k = 0; k < 6; ++k) s = s - Mb[r][k] * Mb[c][k];
                    return s;
                };
                bool bad = false;
                for (int j = 0; j < 6; ++j) {   // ego_solve6's order
                    double s = S(j, j);
                    for (int k = 0; k < j; ++k) s = s - Lp[j][k] * Lp[j][k];
                    if (!(s > 0)) bad = true;
                    Lp[j][j] = sqrt(s);
                    for (int i = j + 1; i < 6; ++i) {
                        s = S(j, i);
                        for (int k = 0; k < j; ++k) s = s - Lp[i][k] * Lp[j][k];
                        Lp[i][j] = s / Lp[j][j];
                    }
                }
                if (bad) s_fail = 1;
                for (int j = 0; j < 6; ++j) invp[j] = 1.0 / Lp[j][j];
                double *sf = s_fac[step & 1], *gf = g.fac + (size_t)step * kPgFacDoubles;
                for (int r = 0; r < 6; ++r) {
                    for (int c = 0; c < 6; ++c) {
                        const double l = c <= r ? Lp[r][c] : 0.0;
                        sf[6 * r + c] = l; gf[6 * r + c] = l;
                        sf[42 + 6 * r + c] = Mb[r][c]; gf[42 + 6 * r + c] = Mb[r][c];
                    }
                    sf[36 + r] = invp[r]; gf[36 + r] = invp[r];
                }
            }
            const int i = step - 1;
            if (column_lane && i >= 1) {
                const double *sf = s_fac[i & 1];
                double s[6];
                for (int r = 0; r < 6; ++r) {
                    const size_t at = (size_t)(6 * i + r) * ldw + col;
                    s[r] = col == 0 ? g.cols[at] : (i == la ? ua[r] : (i == lb ? ub[r] : 0.0));
                }
                if (i >= 2)
                    for (int r = 0; r < 6; ++r)
                        for (int k = 0; k < 6; ++k) s[r] = s[r] - sf[42 + 6 * r + k] * y[k];
                for (int r = 0; r < 6; ++r) {
                    double v = s[r];
                    for (int k = 0; k < r; ++k) v = v - sf[6 * r + k] * y[k];
                    y[r] = v * sf[36 + r];
                }
                for (int r = 0; r < 6; ++r) g.cols[(size_t)(6 * i + r) * ldw + col] = y[r];
            }
            __syncthreads();
        }
        if (s_fail) { failed = true; break; }   // uniform: s_fail is written before the last barrier
        // ---- 4. back substitution: every column lane on its own, the factor by broadcast loads
        if (column_lane) {
            double z[6];
            for (int r = 0; r < 6; ++r) z[r] = 0.0;
            for (int i = N - 1; i >= 1; --i) {
                const double *f = g.fac + (size_t)i * kPgFacDoubles;
                double s[6];
                for (int r = 0; r < 6; ++r) s[r] = g.cols[(size_t)(6 * i + r) * ldw + col];
                if (i + 1 < N)
                    for (int r = 0; r < 6; ++r)
                        for (int k = 0; k < 6; ++k) s[r] = s[r] - f[kPgFacDoubles + 42 + 6 * k + r] * z[k];
                for (int r = 5; r >= 0; --r) {
                    double v = s[r];
                    for (int k = r + 1; k < 6; ++k) v = v - f[6 * k + r] * z[k];
                    z[r] = v * f[36 + r];
                }
                for (int r = 0; r < 6; ++r) g.cols[(size_t)(6 * i + r) * ldw + col] = z[r];
            }
        }
        __syncthreads();
        if (M > 0) {   // uniform
            // ---- 5. C = I + U^T Z and v = U^T x0: entry (p, q), q <= p; row M holds v
            for (int k = tid; k < (M + 1) * M; k += kPgThreads) {
                const int p = k / M, q = k % M;
                if (q > p) continue;
                const int u = p == M ? q : p;           // the column of U
                const size_t zc = p == M ? 0 : 1 + (size_t)q;   // the column of the workspace
                const int e = u / 6, c = u % 6;
                const PgEdge &ed = g.edges[(size_t)g.max_nodes + e];
                const double *blk = g.lin_loop + (size_t)e * kPgLoopDoubles;
                const int lo = min(ed.a, ed.b), hi = max(ed.a, ed.b);
                const double *ulo = ed.a < ed.b ? blk : blk + 36, *uhi = ed.a < ed.b ? blk + 36 : blk;
                double s = p == q ? 1.0 : 0.0;
                if (lo >= 1 && lo < N) {
                    double d = ulo[c] * g.cols[(size_t)(6 * lo) * ldw + zc];
                    for (int r = 1; r < 6; ++r) d = d + ulo[6 * r + c] * g.cols[(size_t)(6 * lo + r) * ldw + zc];
                    s = s + d;
                }
                if (hi >= 1 && hi < N) {
                    double d = uhi[c] * g.cols[(size_t)(6 * hi) * ldw + zc];
                    for (int r = 1; r < 6; ++r) d = d + uhi[6 * r + c] * g.cols[(size_t)(6 * hi + r) * ldw + zc];
                    s = s + d;
                }
                if (p == q) g.cd[p] = s;
                else g.lc[(size_t)q * ldc + p] = s;
            }
            __syncthreads();
            // ---- 6. left-looking Cholesky, row tid; every row recomputes the pivot of the column, so one barrier per column
            for (int j = 0; j < M; ++j) {   // uniform
                if (tid >= j && tid <= M) {
                    double sd = g.cd[j], s = tid > j ? g.lc[(size_t)j * ldc + tid] : 0.0;
                    for (int k = 0; k < j; ++k) {
                        const double ljk = g.lc[(size_t)k * ldc + j];
                        sd = sd - ljk * ljk;
                        if (tid > j) s = s - g.lc[(size_t)k * ldc + tid] * ljk;
                    }
                    const double d = sqrt(sd);
                    if (tid == j) {
                        if (!(sd > 0)) s_fail = 1;
                        g.ld[j] = d;
                    } else {
                        const double l = s / d;
                        g.lc[(size_t)j * ldc + tid] = l;
                        if (tid < M) g.lr[(size_t)tid * ldr + j] = l;
                    }
                }
                __syncthreads();
            }
            if (s_fail) { failed = true; break; }   // uniform
            // ---- 7. L^T y = w, column by column from the last
            double s = tid < M ? g.lc[(size_t)tid * ldc + M] : 0.0;
            for (int k = M - 1; k >= 0; --k) {   // uniform
                if (tid == k) s_y[k] = s / g.ld[k];
                __syncthreads();
                if (tid < k) s = s - g.lr[(size_t)k * ldr + tid] * s_y[k];
            }
            // ---- 8. x = x0 - Z y, one row per lane, the sum over the columns ascending
            for (int k = tid; k < 6 * (N - 1); k += kPgThreads) {
                double *row = g.cols + (size_t)(6 + k) * ldw;
                double t = row[1] * s_y[0];
                for (int q = 1; q < M; ++q) t = t + row[1 + q] * s_y[q];
                row[0] = row[0] - t;
            }
            __syncthreads();
        }
        // ---- 9. the update, one lane per node; node 0 is the gauge
        for (int i = 1 + tid; i < N; i += kPgThreads) {
            double d[6];
            for (int r = 0; r < 6; ++r) d[r] = g.cols[(size_t)(6 * i + r) * ldw];
            PgPose p = pg_load(g.est + 12 * (size_t)i);
            ego_update_right(d, p.R, p.t);
            pg_store(g.est + 12 * (size_t)i, p);
        }
        __syncthreads();
    }
    double cost_after = cost_before;
    if (failed) {   // uniform
        for (int k = tid; k < 12 * N; k += kPgThreads) g.est[k] = g.snap[k];
    } else {
        cost_after = pg_cost(g, N, n_edges, s_red);
    }
    if (tid == 0 && a.result) *a.result = cart_pose_graph_result{failed ? 0 : 1, N, L, iterations, cost_before, cost_after};
}
}  // namespace

void launch_pose_graph_add_node(const PoseGraphNodeArgs &a, hipStream_t s) { hipLaunchKernelGGL(pose_graph_add_node_kernel, dim3(1), dim3(64), 0, s, a); }
void launch_pose_graph_add_loop(const PoseGraphLoopArgs &a, hipStream_t s) { hipLaunchKernelGGL(pose_graph_add_loop_kernel, dim3(1), dim3(64), 0, s, a); }
void launch_pose_graph_optimize(const PoseGraphArgs &a, hipStream_t s) { hipLaunchKernelGGL(pose_graph_optimize_kernel, dim3(1), dim3(kPgThreads), 0, s, a); }

}  // namespace cart_amd

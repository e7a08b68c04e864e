"""numpy restatement of spec S29: pose-graph optimisation over keyframes.  IEEE double with + - * / sqrt only and every
sum written out in the order of the spec: scalar Python floats where one lane works, element-wise numpy over the right-hand-side columns
where the column lanes work (one entry per lane, so the order per entry is the scalar one).  No `@`, no BLAS call.  The GPU equals this
byte for byte (tests/test_gpu_posegraph.py)."""
import math

import numpy as np

import np_ego as E

RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_nodes", "<i4"), ("n_loops", "<i4"), ("iterations", "<i4"), ("cost_before", "<f8"),
                         ("cost_after", "<f8")])                                              # cart_pose_graph_result
MODULE_DTYPE = np.dtype([("result", RESULT_DTYPE), ("node", "<i4"), ("loop_added", "<i4"), ("loops_skipped", "<i4"), ("full", "<i4")])   # cart::PoseGraphRecord
DEFAULT_ITERATIONS = 4
MAX_NODES, MAX_LOOPS, MAX_ITERATIONS = 4096, 64, 16
MODULE_DEFAULTS = dict(keyframe_interval=5, max_nodes=1024, max_loops=64, iterations=4, weight_rotation=10000.0, weight_translation=100.0, loop_weight=1.0)


# ---- poses: (R [9], t [3]) of a 3 x 4 in row order --------------------------------------------------------------------------------
def split(m):
    m = [float(v) for v in m]
    return [m[4 * r + c] for r in range(3) for c in range(3)], [m[4 * r + 3] for r in range(3)]


def join(p):
    R, t = p
    return [R[3 * r + c] if c < 3 else t[r] for r in range(3) for c in range(4)]


def mat3(A, B):
    return [(A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c] for r in range(3) for c in range(3)]


def inv(p):
    R, t = p
    Ri = [R[3 * c + r] for r in range(3) for c in range(3)]
    return Ri, [-((Ri[3 * r] * t[0] + Ri[3 * r + 1] * t[1]) + Ri[3 * r + 2] * t[2]) for r in range(3)]


def mul(A, B):
    return mat3(A[0], B[0]), [((A[0][3 * r] * B[1][0] + A[0][3 * r + 1] * B[1][1]) + A[0][3 * r + 2] * B[1][2]) + A[1][r] for r in range(3)]


def update_right(p, d):
    """R <- R Rq(omega), t <- t + R upsilon with the R from before; Rq is S23's (np_ego.quat_rotation)."""
    R, t = p
    Rq = E.quat_rotation(d[:3])
    Rn = [(R[3 * r] * Rq[c] + R[3 * r + 1] * Rq[3 + c]) + R[3 * r + 2] * Rq[6 + c] for r in range(3) for c in range(3)]
    tn = [t[r] + ((R[3 * r] * d[3] + R[3 * r + 1] * d[4]) + R[3 * r + 2] * d[5]) for r in range(3)]
    return Rn, tn


# ---- one edge: (a, b, R_m [9], t_m [3], w_rot, w_trans), p_b = R_m p_a + t_m ----------------------------------------------------------
def residual(edge, est):
    """-> (R_e [9], r [6] = (rho, tau)) of E = M (est_a^-1 est_b)."""
    a, b, Rm, tm = edge[:4]
    Re, te = mul((Rm, tm), mul(inv(est[a]), est[b]))
    return Re, [0.5 * (Re[7] - Re[5]), 0.5 * (Re[2] - Re[6]), 0.5 * (Re[3] - Re[1]), te[0], te[1], te[2]]


def cost_term(edge, r):
    return edge[4] * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + edge[5] * ((r[3] * r[3] + r[4] * r[4]) + r[5] * r[5])


def jacobians(edge, Re, r):
    """-> (Ja, Jb) 6 x 6 lists: J_b = blockdiag(0.5 (tr I - R_e^T), R_e), J_a = -J_eta Ad_M."""
    Rm, tm = edge[2], edge[3]
    te = r[3:]
    tr = (Re[0] + Re[4]) + Re[8]
    Ja, Jb = [[0.0] * 6 for _ in range(6)], [[0.0] * 6 for _ in range(6)]
    A11 = [0.0] * 9
    for i in range(3):
        for c in range(3):
            d = tr if i == c else 0.0
            Jb[i][c] = 0.5 * (d - Re[3 * c + i])
            Jb[3 + i][3 + c] = Re[3 * i + c]
            A11[3 * i + c] = 0.5 * (d - Re[3 * i + c])
    A21 = [0.0, te[2], -te[1], -te[2], 0.0, te[0], te[1], -te[0], 0.0]
    K = [0.0, -tm[2], tm[1], tm[2], 0.0, -tm[0], -tm[1], tm[0], 0.0]
    TL, P, Q = mat3(A11, Rm), mat3(A21, Rm), mat3(K, Rm)
    for i in range(3):
        for c in range(3):
            Ja[i][c] = -TL[3 * i + c]
            Ja[3 + i][c] = -(P[3 * i + c] + Q[3 * i + c])
            Ja[3 + i][3 + c] = -Rm[3 * i + c]
    return Ja, Jb


def wdot(X, r, Y, c, wr, wt):
    s = (X[0][r] * wr) * Y[0][c]
    for k in range(1, 6):
        s = s + (X[k][r] * (wr if k < 3 else wt)) * Y[k][c]
    return s


def wdotv(X, r, v, wr, wt):
    s = (X[0][r] * wr) * v[0]
    for k in range(1, 6):
        s = s + (X[k][r] * (wr if k < 3 else wt)) * v[k]
    return s


class Graph:
    """The state of a cart_pose_graph: odom, est per node, the odometry edges (edge n joins n - 1 and n) and the loop edges."""

    def __init__(self, max_nodes=MAX_NODES, max_loops=MAX_LOOPS):
        self.max_nodes, self.max_loops = max_nodes, max_loops
        self.clear()

    def clear(self):
        self.odom, self.est, self.edges, self.loops = [], [], [None], []

    def add_node(self, pose, w_rot=1.0, w_trans=1.0):
        if len(self.odom) >= self.max_nodes:
            raise ValueError("the node table is full")
        cur = split(pose)
        if not self.odom:
            self.odom.append(cur)
            self.est.append((list(cur[0]), list(cur[1])))
            return 0
        prev = self.odom[-1]
        self.est.append(mul(self.est[-1], mul(inv(prev), cur)))
        M = mul(inv(cur), prev)
        n = len(self.odom)
        self.edges.append((n - 1, n, M[0], M[1], float(w_rot), float(w_trans)))
        self.odom.append(cur)
        return n

    def add_loop(self, a, b, R, t, w_rot=1.0, w_trans=1.0):
        if a == b or not (0 <= a < len(self.odom) and 0 <= b < len(self.odom)):
            raise ValueError("a and b must be two different nodes")
        if len(self.loops) >= self.max_loops:
            raise ValueError("the loop table is full")
        self.loops.append((int(a), int(b), [float(v) for v in np.asarray(R).reshape(-1)], [float(v) for v in np.asarray(t).reshape(-1)], float(w_rot), float(w_trans)))

    def all_edges(self):
        return self.edges[1:] + self.loops

    def poses(self):
        return np.array([join(p) for p in self.est], np.float64).reshape(-1, 12)

    def cost(self):
        edges = self.all_edges()
        if not edges:
            return 0.0
        terms = np.array([cost_term(e, residual(e, self.est)[1]) for e in edges], np.float64)
        return E.lane_sum(terms, np.ones(len(terms), bool))

    # ---- one Gauss-Newton step ------------------------------------------------------------------------------------------------
    def linearise(self):
        """-> (lin per odometry edge n: Haa, Hbb, Hba, ga, gb; per loop: UA, UB [k][c], ga, gb)."""
        lin, lin_loop = [None], []
        for e in self.edges[1:]:
            Re, r = residual(e, self.est)
            Ja, Jb = jacobians(e, Re, r)
            wr, wt = e[4], e[5]
            Haa = [[wdot(Ja, i, Ja, c, wr, wt) for c in range(6)] for i in range(6)]
            Hbb = [[wdot(Jb, i, Jb, c, wr, wt) for c in range(6)] for i in range(6)]
            Hba = [[wdot(Jb, i, Ja, c, wr, wt) for c in range(6)] for i in range(6)]
            lin.append((Haa, Hbb, Hba, [wdotv(Ja, i, r, wr, wt) for i in range(6)], [wdotv(Jb, i, r, wr, wt) for i in range(6)]))
        for e in self.loops:
            Re, r = residual(e, self.est)
            Ja, Jb = jacobians(e, Re, r)
            wr, wt = e[4], e[5]
            sr, st = math.sqrt(wr), math.sqrt(wt)
            UA = [[Ja[c][k] * (sr if c < 3 else st) for c in range(6)] for k in range(6)]
            UB = [[Jb[c][k] * (sr if c < 3 else st) for c in range(6)] for k in range(6)]
            lin_loop.append((UA, UB, [wdotv(Ja, i, r, wr, wt) for i in range(6)], [wdotv(Jb, i, r, wr, wt) for i in range(6)]))
        return lin, lin_loop

    def rhs(self, lin, lin_loop):
        """b = -gradient per node 1 .. N - 1: the node's own edge, the next edge, then the loops in their order."""
        N = len(self.odom)
        b = [None] * N
        for i in range(1, N):
            row = []
            for r in range(6):
                s = lin[i][4][r]
                if i + 1 < N:
                    s = s + lin[i + 1][3][r]
                for e, loop in enumerate(self.loops):
                    if loop[0] == i:
                        s = s + lin_loop[e][2][r]
                    if loop[1] == i:
                        s = s + lin_loop[e][3][r]
                row.append(-s)
            b[i] = row
        return b

    def factor(self, lin):
        """Block Cholesky of the chain in node order -> per node (L lower 6 x 6, 1 / diagonal, the sub-diagonal block), or None at a pivot
        that is not > 0."""
        N = len(self.odom)
        fac = [None] * N
        Lp, invp = None, None
        for n in range(1, N):
            Mb = [[0.0] * 6 for _ in range(6)]
            if n >= 2:
                for r in range(6):
                    for c in range(6):
                        m = lin[n][2][r][c]
                        for k in range(c):
                            m = m - Mb[r][k] * Lp[c][k]
                        Mb[r][c] = m * invp[c]

            def S(r, c):
                s = lin[n][1][r][c]
                if n + 1 < N:
                    s = s + lin[n + 1][0][r][c]
                if n >= 2:
                    for k in range(6):
                        s = s - Mb[r][k] * Mb[c][k]
                return s
            L = [[0.0] * 6 for _ in range(6)]
            for j in range(6):
                s = S(j, j)
                for k in range(j):
                    s = s - L[j][k] * L[j][k]
                if not s > 0:
                    return None
                L[j][j] = math.sqrt(s)
                for i in range(j + 1, 6):
                    s = S(j, i)
                    for k in range(j):
                        s = s - L[i][k] * L[j][k]
                    L[i][j] = s / L[j][j]
            Lp, invp = L, [1.0 / L[j][j] for j in range(6)]
            fac[n] = (L, invp, Mb)
        return fac

    def substitute(self, fac, b, lin_loop):
        """T^-1 [b | U] -> Z [N][6] arrays over the 1 + 6 L columns (column 0 = x0)."""
        N, nl = len(self.odom), len(self.loops)
        ncols = 1 + 6 * nl
        rhs = [[np.zeros(ncols) for _ in range(6)] for _ in range(N)]
        for i in range(1, N):
            for r in range(6):
                rhs[i][r][0] = b[i][r]
        for e, loop in enumerate(self.loops):
            for c in range(6):
                for k in range(6):
                    rhs[loop[0]][k][1 + 6 * e + c] = lin_loop[e][0][k][c]
                    rhs[loop[1]][k][1 + 6 * e + c] = lin_loop[e][1][k][c]
        Y = [None] * N
        y = None
        for i in range(1, N):
            L, iv, Mb = fac[i]
            s = [rhs[i][r].copy() for r in range(6)]
            if i >= 2:
                for r in range(6):
                    for k in range(6):
                        s[r] = s[r] - Mb[r][k] * y[k]
            cur = []
            for r in range(6):
                v = s[r]
                for k in range(r):
                    v = v - L[r][k] * cur[k]
                cur.append(v * iv[r])
            Y[i] = y = cur
        Z = [None] * N
        z = None
        for i in range(N - 1, 0, -1):
            L, iv, _ = fac[i]
            s = [Y[i][r] for r in range(6)]
            if i + 1 < N:
                Mn = fac[i + 1][2]
                for r in range(6):
                    for k in range(6):
                        s[r] = s[r] - Mn[k][r] * z[k]
            cur = [None] * 6
            for r in range(5, -1, -1):
                v = s[r]
                for k in range(r + 1, 6):
                    v = v - L[k][r] * cur[k]
                cur[r] = v * iv[r]
            Z[i] = z = cur
        return Z

    def loop_system(self, Z, lin_loop):
        """C = I + U^T Z (lower entries) and v = U^T x0 as the extra row M: each entry two block terms, the lower node first; the block of
        node 0 is dropped."""
        Mo = 6 * len(self.loops)
        C = [[0.0] * Mo for _ in range(Mo + 1)]
        for p in range(Mo + 1):
            for q in range(min(p, Mo - 1) + 1):
                u = q if p == Mo else p
                zc = 0 if p == Mo else 1 + q
                e, c = divmod(u, 6)
                a, b = self.loops[e][0], self.loops[e][1]
                blocks = sorted(((a, lin_loop[e][0]), (b, lin_loop[e][1])), key=lambda nb: nb[0])
                s = 1.0 if p == q else 0.0
                for node, U in blocks:
                    if node >= 1:
                        d = U[0][c] * float(Z[node][0][zc])
                        for r in range(1, 6):
                            d = d + U[r][c] * float(Z[node][r][zc])
                        s = s + d
                C[p][q] = s
        return C

    def loop_solve(self, C):
        """Unpivoted Cholesky of C with the right-hand side as row M (its row of the factor is the forward solve), then L^T y = w by
        columns from the last -> y [M], or None at a pivot that is not > 0."""
        Mo = len(C) - 1
        Lf = [[0.0] * Mo for _ in range(Mo + 1)]
        for j in range(Mo):
            sd = C[j][j]
            for k in range(j):
                sd = sd - Lf[j][k] * Lf[j][k]
            if not sd > 0:
                return None
            d = math.sqrt(sd)
            Lf[j][j] = d
            for i in range(j + 1, Mo + 1):
                s = C[i][j]
                for k in range(j):
                    s = s - Lf[i][k] * Lf[j][k]
                Lf[i][j] = s / d
        s = list(Lf[Mo])
        y = [0.0] * Mo
        for k in range(Mo - 1, -1, -1):
            y[k] = s[k] / Lf[k][k]
            for i in range(k):
                s[i] = s[i] - Lf[k][i] * y[k]
        return y

    def step(self):
        """-> the update delta per node (None for node 0), or None at a pivot that is not > 0."""
        N = len(self.odom)
        lin, lin_loop = self.linearise()
        b = self.rhs(lin, lin_loop)
        fac = self.factor(lin)
        if fac is None:
            return None
        Z = self.substitute(fac, b, lin_loop)
        x = [None] + [[float(Z[i][r][0]) for r in range(6)] for i in range(1, N)]
        if self.loops:
            y = self.loop_solve(self.loop_system(Z, lin_loop))
            if y is None:
                return None
            for i in range(1, N):
                for r in range(6):
                    row = Z[i][r]
                    t = float(row[1]) * y[0]
                    for q in range(1, len(y)):
                        t = t + float(row[1 + q]) * y[q]
                    x[i][r] = x[i][r] - t
        return x

    def optimize(self, iterations=DEFAULT_ITERATIONS):
        """-> RESULT_DTYPE [1]; the estimates move unless a pivot fails."""
        N = len(self.odom)
        res = np.zeros(1, RESULT_DTYPE)
        res["status"], res["n_nodes"], res["n_loops"], res["iterations"] = 1, N, len(self.loops), iterations
        if N < 2:
            return res
        before = [(list(p[0]), list(p[1])) for p in self.est]
        res["cost_before"] = res["cost_after"] = self.cost()
        for _ in range(iterations):
            x = self.step()
            if x is None:
                self.est = before
                res["status"] = 0
                return res
            for i in range(1, N):
                self.est[i] = update_right(self.est[i], x[i])
        res["cost_after"] = self.cost()
        return res


# ---- the dense normal equations, for the spec test only ----------------------------------------------------------------------------
def dense_step(graph):
    """np.linalg.solve of the densely assembled normal equations at the graph's estimates -> delta [N - 1][6]."""
    N = len(graph.odom)
    H, g = np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
    for e in graph.all_edges():
        Re, r = residual(e, graph.est)
        Ja, Jb = (np.array(J) for J in jacobians(e, Re, r))
        W = np.diag([e[4]] * 3 + [e[5]] * 3)
        J = np.zeros((6, 6 * N))
        J[:, 6 * e[0]:6 * e[0] + 6], J[:, 6 * e[1]:6 * e[1] + 6] = Ja, Jb
        H += J.T.dot(W).dot(J)
        g += J.T.dot(W).dot(np.array(r))
    return np.linalg.solve(H[6:, 6:], -g[6:]).reshape(N - 1, 6)


# ---- the host module (cartslam_amd/modules/posegraph.hpp) --------------------------------------------------------------------------
def carry(est_k, odom_k, odom_t):
    """est_k (odom_k^-1 odom_t) as 12 doubles."""
    return join(mul(split(est_k), mul(inv(split(odom_k)), split(odom_t))))


def module(poses, loops, **keys):
    """The "pose_graph" module over frames 1 .. n: poses[f] = the source's chained pose (12 doubles), loops[f] = the LOOP_DTYPE record of
    np_place.loop_closure.  -> per frame (MODULE_DTYPE [1], pose [12], every node's estimate [nodes, 12] on a frame that optimised, else None)."""
    k = dict(MODULE_DEFAULTS, **keys)
    graph = Graph(k["max_nodes"], k["max_loops"])
    node_frames, out = [], []
    last = np.zeros(1, RESULT_DTYPE)
    skipped, full = 0, 0
    odom_k = est_k = None
    for f, (pose, loop) in enumerate(zip(poses, loops)):
        fid = f + 1
        rec = np.zeros(1, MODULE_DTYPE)
        rec["node"] = -1
        nodes = None
        if fid % k["keyframe_interval"] == 0:
            if len(graph.odom) >= k["max_nodes"]:
                full = 1
            else:
                n = graph.add_node(pose, k["weight_rotation"], k["weight_translation"])
                node_frames.append(fid)
                rec["node"] = n
                if int(loop["detected"]):
                    kf = int(loop["keyframe_id"])
                    if kf in node_frames and node_frames.index(kf) != n and len(graph.loops) < k["max_loops"]:
                        rel = loop["relative"]
                        graph.add_loop(node_frames.index(kf), n, rel["R"], rel["t"], k["weight_rotation"] * k["loop_weight"], k["weight_translation"] * k["loop_weight"])
                        last = graph.optimize(k["iterations"])
                        rec["loop_added"] = 1
                        nodes = graph.poses()
                    else:
                        skipped += 1
                odom_k, est_k = list(pose), join(graph.est[n])
        rec["result"], rec["loops_skipped"], rec["full"] = last[0], skipped, full
        out.append((rec, carry(est_k, odom_k, pose) if est_k is not None else [float(v) for v in pose], nodes))
    return out

"""numpy restatement of spec S32: windowed bundle adjustment over the last frames.  The track building is integer logic
in plain Python; the optimiser is element-wise numpy over the point slots (one entry per slot, so the order per entry is the scalar one)
with every sum over slots in S23's virtual-lane order.  IEEE double with + - * / sqrt only, no `@`, no BLAS call, no numpy `sum` on floating
point.  The GPU equals this byte for byte (tests/test_gpu_localba.py)."""
import numpy as np

import np_ego as E
import np_posegraph as P

LANES = E.LANES
OBS_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("valid", "<i4")])                      # one observation, 16 bytes
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_frames", "<i4"), ("n_points_active", "<i4"), ("n_observations", "<i4"), ("n_held", "<i4"),
                         ("iterations", "<i4"), ("cost_before", "<f8"), ("cost_after", "<f8")])         # cart_local_ba_result, 40 bytes
MAX_WINDOW, MAX_ITERATIONS = 16, 16


def params(**over):
    """cart_local_ba_default_params: build-owned, no data set has tuned them."""
    p = dict(min_disparity=1.0, huber=2.0, damping=0.0, iterations=4, min_observations=2, min_frame_observations=6)
    p.update(over)
    return p


# ---- sums over the point slots ------------------------------------------------------------------------------------------------------
def lane_sums(rows, mask):
    """S23's virtual-lane sum of every row of `rows` [K, M] over the slots in `mask` [M] -> K floats: lane l adds slots l, l + 256, ... in
    ascending order to a zero (a skipped slot adds nothing), then v[l] += v[l ^ o] for o = 128 .. 1."""
    rows = np.asarray(rows, np.float64).reshape(len(rows), -1)
    K, M = rows.shape
    chunks = (M + LANES - 1) // LANES
    x = np.zeros((K, chunks * LANES))
    x[:, :M] = np.where(np.asarray(mask, bool)[None, :], rows, 0.0)   # adding +0.0 to a sum that began as +0.0 changes no bit of it
    x = x.reshape(K, chunks, LANES)
    v = np.zeros((K, LANES))
    with np.errstate(all="ignore"):
        for c in range(chunks):
            v = v + x[:, c, :]
        lanes = np.arange(LANES)
        o = LANES // 2
        while o:
            v = v + v[:, lanes ^ o]
            o //= 2
    return [float(s) for s in v[:, 0]]


# ---- one observation ------------------------------------------------------------------------------------------------------------------
def observe(cam, est, X, u, v, ur, huber):
    """The residual, the Huber weight and the Jacobians of the observations (u, v, ur) of the points X = (x, y, z) in the frame with
    est = 12 doubles (3 x 4, camera-to-world); arrays over the slots or scalars.  -> dict; entries where `front` is False mean nothing."""
    fx, fy, cx, cy, bl = (cam[k] for k in ("fx", "fy", "cx", "cy", "baseline"))
    R = [[est[4 * r + c] for c in range(3)] for r in range(3)]
    t = [est[4 * r + 3] for r in range(3)]
    with np.errstate(all="ignore"):
        d = [X[0] - t[0], X[1] - t[1], X[2] - t[2]]
        qx = (R[0][0] * d[0] + R[1][0] * d[1]) + R[2][0] * d[2]
        qy = (R[0][1] * d[0] + R[1][1] * d[1]) + R[2][1] * d[2]
        qz = (R[0][2] * d[0] + R[1][2] * d[1]) + R[2][2] * d[2]
        front = qz > 0
        eu = ((fx * qx) / qz + cx) - u
        ev = ((fy * qy) / qz + cy) - v
        er = ((fx * (qx - bl)) / qz + cx) - ur
        n2 = (eu * eu + ev * ev) + er * er
        k = huber
        root = np.sqrt(n2)
        inside = n2 <= k * k
        w = np.where(inside, 1.0, k / root)
        rho = np.where(inside, n2, (2.0 * k) * root - k * k)
        a = fx / qz
        b = -((fx * qx) / (qz * qz))
        c = fy / qz
        dd = -((fy * qy) / (qz * qz))
        br = -((fx * (qx - bl)) / (qz * qz))
        zero = np.zeros_like(qz) if np.ndim(qz) else 0.0
        # J_c = J_q [ [q]x | -I ], J_p = J_q R^T
        Ju = [-(b * qy), b * qx - a * qz, a * qy, -a, zero, -b]
        Jv = [c * qz - dd * qy, dd * qx, -(c * qx), zero, -c, -dd]
        Jr = [-(br * qy), br * qx - a * qz, a * qy, -a, zero, -br]
        Pu = [a * R[m][0] + b * R[m][2] for m in range(3)]
        Pv = [c * R[m][1] + dd * R[m][2] for m in range(3)]
        Pr = [a * R[m][0] + br * R[m][2] for m in range(3)]
    return dict(front=front, q=(qx, qy, qz), e=(eu, ev, er), n2=n2, w=w, rho=rho, Jc=(Ju, Jv, Jr), Jp=(Pu, Pv, Pr))


def jtj(o, A, i, B, j):
    """w ((A_u[i] B_u[j] + A_v[i] B_v[j]) + A_r[i] B_r[j]): one entry of a weighted J^T J block of observation o."""
    return o["w"] * ((A[0][i] * B[0][j] + A[1][i] * B[1][j]) + A[2][i] * B[2][j])


def jte(o, A, i):
    return o["w"] * ((A[0][i] * o["e"][0] + A[1][i] * o["e"][1]) + A[2][i] * o["e"][2])


def chol3(V):
    """Unpivoted Cholesky of the symmetric 3 x 3 V (upper entries V[k][l], k <= l) in ego_solve6's order -> (L lower, every pivot > 0)."""
    L = [[None] * 3 for _ in range(3)]
    ok = True
    with np.errstate(all="ignore"):
        for j in range(3):
            s = V[j][j]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            ok = ok & (s > 0)
            L[j][j] = np.sqrt(s)
            for i in range(j + 1, 3):
                s = V[j][i]
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                L[i][j] = s / L[j][j]
    return L, ok


def solve3(L, b):
    """L L^T x = b, forward then backward as ego_solve6."""
    with np.errstate(all="ignore"):
        y = [None] * 3
        for i in range(3):
            s = b[i]
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s / L[i][i]
        x = [None] * 3
        for i in range(2, -1, -1):
            s = y[i]
            for k in range(i + 1, 3):
                s = s - L[k][i] * x[k]
            x[i] = s / L[i][i]
    return x


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


class Window:
    """The state of a cart_local_ba: the frame ring, the point table and the dense observation table."""

    def __init__(self, max_features, window=8, max_points=8192):
        self.max_features, self.window, self.max_points = int(max_features), int(window), int(max_points)
        self.clear()

    def clear(self):
        W, M = self.window, self.max_points
        self.n_pushed = 0
        self.frame_id = np.zeros(W, np.uint64)
        self.odom, self.est = np.zeros((W, 12)), np.zeros((W, 12))
        self.track_of = np.full(self.max_features, -1, np.int32)
        self.X = np.zeros((M, 3))
        self.n_obs, self.state = np.zeros(M, np.int32), np.zeros(M, np.int32)
        self.obs = np.zeros((M, W), OBS_DTYPE)

    # ---- the window in age order ---------------------------------------------------------------------------------------------------
    def frames(self):
        return min(self.n_pushed, self.window)

    def slot(self, a):
        return (self.n_pushed - self.frames() + a) % self.window

    def poses(self):
        """-> (float64 [W, 12] in age order, unused rows zero; uint64 [W] frame ids)."""
        out, ids = np.zeros((self.window, 12)), np.zeros(self.window, np.uint64)
        for a in range(self.frames()):
            out[a], ids[a] = self.est[self.slot(a)], self.frame_id[self.slot(a)]
        return out, ids

    def points(self):
        """-> float64 [max_points, 4]: (X, Y, Z, n_obs), zeros in a free slot."""
        return np.concatenate([self.X, self.n_obs[:, None].astype(np.float64)], axis=1)

    # ---- push ------------------------------------------------------------------------------------------------------------------------
    def push(self, cam, p, frame_id, pose, kpL, kpR, stereo, temporal):
        """-> counts int32 [8] = {left keypoints, stereo-valid, continued, born, dropped, freed, live points, frames in window}."""
        W, cap = self.window, self.max_features
        nl = min(len(kpL), cap)
        s = self.n_pushed % W
        freed = 0
        if self.n_pushed >= W:                                     # 1. the frame in slot s leaves
            seen = self.obs["valid"][:, s] != 0
            self.n_obs[seen] -= 1
            dead = seen & (self.n_obs == 0)
            self.state[dead] = 0
            self.X[dead] = 0.0
            freed = int(dead.sum())
            self.obs[:, s] = 0
        cur = P.split(pose)                                        # 2. the estimate carries the window's correction forward
        if self.n_pushed == 0:
            est = cur
        else:
            sp = (self.n_pushed - 1) % W
            est = P.mul(P.split(self.est[sp]), P.mul(P.inv(P.split(self.odom[sp])), cur))
        self.frame_id[s], self.odom[s], self.est[s] = frame_id, P.join(cur), P.join(est)
        est12 = [float(v) for v in self.est[s]]
        so = np.zeros(nl, OBS_DTYPE)                               # 3. the stereo observation of every left index
        for m in stereo:
            i, j = int(m["query"]), int(m["train"])
            if not (0 <= i < nl and 0 <= j < cap and j < len(kpR)):
                continue
            u, v, ur = kpL["x"][i], kpL["y"][i], kpR["x"][j]
            if float(u) - float(ur) >= p["min_disparity"]:
                so[i] = (u, v, ur, 1)
        tm = np.full(nl, -1, np.int64)                             # 4. continuation: the smallest i that names a point wins it
        if self.n_pushed > 0:
            for m in temporal:
                i, j = int(m["query"]), int(m["train"])
                if 0 <= i < nl and 0 <= j < cap:
                    tm[i] = j
        claim = {}
        for i in range(nl):
            if so["valid"][i] and tm[i] >= 0:
                pt = int(self.track_of[tm[i]])
                if pt >= 0 and self.state[pt] != 0:
                    claim[pt] = min(claim.get(pt, i), i)
        free = [int(k) for k in np.nonzero(self.state == 0)[0]]   # 5. births take the free slots in ascending order
        track = np.full(cap, -1, np.int32)
        continued = born = dropped = 0
        fxb = cam["fx"] * cam["baseline"]
        for i in range(nl):
            if not so["valid"][i]:
                continue
            pt = int(self.track_of[tm[i]]) if tm[i] >= 0 else -1
            if pt >= 0 and claim.get(pt, -1) == i:
                continued += 1
                self.n_obs[pt] += 1
            elif born < len(free):
                pt = free[born]
                born += 1
                u, v, ur = float(so["u"][i]), float(so["v"][i]), float(so["ur"][i])
                Z = fxb / (u - ur)
                c = (((u - cam["cx"]) * Z) / cam["fx"], ((v - cam["cy"]) * Z) / cam["fy"], Z)
                self.X[pt] = [((est12[4 * r] * c[0] + est12[4 * r + 1] * c[1]) + est12[4 * r + 2] * c[2]) + est12[4 * r + 3] for r in range(3)]
                self.state[pt], self.n_obs[pt] = 1, 1
            else:
                dropped += 1
                continue
            self.obs[pt, s] = so[i]                                # 6.
            track[i] = pt
        self.track_of = track
        self.n_pushed += 1
        return np.array([nl, int(so["valid"].sum()), continued, born, dropped, freed, int((self.state != 0).sum()), self.frames()], np.int32)

    # ---- optimise --------------------------------------------------------------------------------------------------------------------
    def active(self, p):
        return (self.state != 0) & (self.n_obs >= p["min_observations"])

    def linearise(self, cam, p):
        """-> per age a: (the observation record of every slot, usable = active, seen and in front)."""
        act = self.active(p)
        lin = []
        X = (self.X[:, 0], self.X[:, 1], self.X[:, 2])
        for a in range(self.frames()):
            s = self.slot(a)
            ob = self.obs[:, s]
            o = observe(cam, [float(v) for v in self.est[s]], X, ob["u"].astype(np.float64), ob["v"].astype(np.float64), ob["ur"].astype(np.float64),
                        p["huber"])
            lin.append((o, act & (ob["valid"] != 0) & o["front"]))
        return act, lin

    def cost(self, cam, p):
        """-> (sum of rho over the usable observations of the active points, their number, the active points)."""
        act, lin = self.linearise(cam, p)
        c = np.zeros(self.max_points)
        for o, usable in lin:
            c = np.where(usable, c + np.where(usable, o["rho"], 0.0), c)
        return lane_sums([c], act)[0], int(sum(int(u.sum()) for _, u in lin)), int(act.sum())

    def system(self, cam, p):
        """The linearisation and the reduced system of one step -> dict (held, used, per-point blocks, C = the reduced system's lower
        entries with the right-hand side as its last row)."""
        F, M, damping = self.frames(), self.max_points, p["damping"]
        act, lin = self.linearise(cam, p)
        held = [a >= 1 and int(lin[a][1].sum()) < p["min_frame_observations"] for a in range(F)]
        used = [lin[a][1] & (not held[a]) for a in range(F)]
        V = [[np.zeros(M) for _ in range(3)] for _ in range(3)]
        gp = [np.zeros(M) for _ in range(3)]
        with np.errstate(all="ignore"):
            for a in range(F):                                      # the point blocks, over the frames in age order
                o = lin[a][0]
                for k in range(3):
                    for l in range(k, 3):
                        V[k][l] = np.where(used[a], V[k][l] + jtj(o, o["Jp"], k, o["Jp"], l), V[k][l])
                    gp[k] = np.where(used[a], gp[k] + jte(o, o["Jp"], k), gp[k])
            for k in range(3):
                V[k][k] = V[k][k] + damping
            L, ok = chol3(V)
            inp = act & ok
            one, zero = np.ones(M), np.zeros(M)
            cols = [solve3(L, [one if r == k else zero for r in range(3)]) for k in range(3)]
            Vi = [[cols[k][r] for k in range(3)] for r in range(3)]
            Wb = [None] * F
            for a in range(1, F):
                o = lin[a][0]
                Wb[a] = [[jtj(o, o["Jc"], i, o["Jp"], k) for k in range(3)] for i in range(6)]
            n = 6 * (F - 1)
            C = [[0.0] * n for _ in range(n + 1)]
            for a in range(1, F):
                if held[a]:
                    for i in range(6):
                        C[6 * (a - 1) + i][6 * (a - 1) + i] = 1.0
                    continue
                o, m = lin[a][0], inp & used[a]
                Y = [[dot3(Wb[a][i], [Vi[0][k], Vi[1][k], Vi[2][k]]) for k in range(3)] for i in range(6)]
                idx = [(i, j) for i in range(6) for j in range(i, 6)]
                U = lane_sums([jtj(o, o["Jc"], i, o["Jc"], j) for i, j in idx], m)
                g = lane_sums([jte(o, o["Jc"], i) for i in range(6)], m)
                z = lane_sums([dot3(Y[i], gp) for i in range(6)], m)
                for i in range(6):
                    C[n][6 * (a - 1) + i] = (-g[i]) + z[i]
                for b in range(a, F):
                    pairs = idx if a == b else [(i, j) for i in range(6) for j in range(6)]
                    T = lane_sums([dot3(Y[i], Wb[b][j]) for i, j in pairs], m & used[b])
                    for (i, j), tv in zip(pairs, T):
                        u = 0.0
                        if a == b:
                            u = U[idx.index((i, j))]
                            if i == j:
                                u = u + damping
                        C[6 * (b - 1) + j][6 * (a - 1) + i] = u - tv
        return dict(held=held, used=used, inp=inp, Vi=Vi, gp=gp, W=Wb, C=C, V=V, lin=lin)

    def deltas(self, cam, p):
        """The solved step -> (the system, delta [F] of 6 floats per free frame (None for the gauge), dX [max_points, 3], zero for a point
        that does not move), or None at a pivot of the reduced system that is not > 0."""
        F = self.frames()
        sy = self.system(cam, p)
        y = P.Graph.loop_solve(None, sy["C"])
        if y is None:
            return None
        delta = [None] + [y[6 * (a - 1):6 * a] for a in range(1, F)]
        dX = np.zeros((self.max_points, 3))
        with np.errstate(all="ignore"):
            h = [-sy["gp"][k] for k in range(3)]
            for a in range(1, F):
                if sy["held"][a]:
                    continue
                for k in range(3):
                    s = sy["W"][a][0][k] * delta[a][0]
                    for i in range(1, 6):
                        s = s + sy["W"][a][i][k] * delta[a][i]
                    h[k] = np.where(sy["used"][a], h[k] - s, h[k])
            for r in range(3):
                dX[:, r] = np.where(sy["inp"], dot3(sy["Vi"][r], h), 0.0)
        return sy, delta, dX

    def step(self, cam, p):
        """One Gauss-Newton step in place -> the number of held frames, or None at a pivot of the reduced system that is not > 0."""
        got = self.deltas(cam, p)
        if got is None:
            return None
        sy, delta, dX = got
        for r in range(3):
            self.X[:, r] = np.where(sy["inp"], self.X[:, r] + dX[:, r], self.X[:, r])
        for a in range(1, self.frames()):
            if not sy["held"][a]:
                s = self.slot(a)
                self.est[s] = P.join(P.update_right(P.split(self.est[s]), [float(v) for v in delta[a]]))
        return sum(1 for hd in sy["held"] if hd)

    def optimize(self, cam, p):
        """-> RESULT_DTYPE [1]; the estimates and the points move unless a pivot fails."""
        res = np.zeros(1, RESULT_DTYPE)
        cost, n_obs, n_act = self.cost(cam, p)
        res["status"], res["n_frames"], res["n_points_active"], res["n_observations"], res["iterations"] = 1, self.frames(), n_act, n_obs, p["iterations"]
        res["cost_before"] = res["cost_after"] = cost
        if self.frames() < 2 or n_act == 0:
            return res
        before = (self.est.copy(), self.X.copy())
        held = 0
        for _ in range(p["iterations"]):
            h = self.step(cam, p)
            if h is None:
                self.est, self.X = before
                res["status"] = 0
                return res
            held += h
        res["n_held"] = held
        res["cost_after"] = self.cost(cam, p)[0]
        return res


# ---- the host module (cartslam_amd/modules/localba.hpp) ----------------------------------------------------------------------------------
MODULE_DTYPE = np.dtype([("result", RESULT_DTYPE), ("counts", "<i4", 8), ("taken", "<i4"), ("optimised", "<i4")])   # cart::LocalBARecord, 80 bytes
MODULE_DEFAULTS = dict(window=8, max_points=8192, interval=1)


def module(cam, frames, max_features, **keys):
    """The "local_ba" module over frames 1 .. n: frames[f] = dict(kpL, kpR, stereo, temporal, status = the source's result.status, pose =
    the source's chained pose, R, t = the source's relative pose).  A frame with status 0 clears the window and starts a new one.
    -> per frame (MODULE_DTYPE [1], pose [12], ids uint64 [W], poses [W, 12], R [9], t [3])."""
    k = dict(MODULE_DEFAULTS, **keys)
    p = params(**{n: k[n] for n in params() if n in k})
    win = Window(max_features, k["window"], k["max_points"])
    out = []
    for f, fr in enumerate(frames):
        fid = f + 1
        rec = np.zeros(1, MODULE_DTYPE)
        restart = int(fr["status"]) == 0
        if restart:
            win.clear()
        rec["counts"][0] = win.push(cam, p, fid, fr["pose"], fr["kpL"], fr["kpR"], fr["stereo"], fr["temporal"])
        carried = win.poses()[0]
        if not restart and fid % k["interval"] == 0:
            with np.errstate(all="ignore"):
                rec["result"] = win.optimize(cam, p)[0]
            rec["optimised"] = 1
            res = rec["result"][0]
            rec["taken"] = int(res["status"] == 1 and res["cost_after"] <= res["cost_before"])
        final, ids = win.poses()
        poses = final if int(rec["taken"][0]) else carried
        F = win.frames()
        R, t = [float(v) for v in fr["R"]], [float(v) for v in fr["t"]]
        if not restart and F >= 2:
            R, t = P.mul(P.inv(P.split(poses[F - 1])), P.split(poses[F - 2]))
        out.append((rec, poses[F - 1].copy(), ids, final, R, t))
    return out


# ---- a synthetic drive, for the tests and the measurements ------------------------------------------------------------------------------
def rot(axis_angle):
    """Rodrigues, for building scenes only (not part of the spec)."""
    w = np.asarray(axis_angle, np.float64)
    th = float(np.sqrt((w * w).sum()))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * K.dot(K)


def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).reshape(12)


def drive(seed, n_frames, n_points, cam=None, width=320, height=192, step=0.6, yaw_deg=2.0, pixel=0.25, missing=0.15, rot_noise_deg=0.15,
          trans_noise=0.02, z_range=(5.0, 30.0), clip=True):
    """A drive past n_points world points: per frame the true pose, the noisy chained odometry and the keypoint / match lists that
    `Window.push` takes (keypoints quantised to `pixel`, a share `missing` of the visible observations dropped; clip=False keeps the observations outside the image too).
    -> list of dict(true, odom, kpL, kpR, stereo, temporal)."""
    cam = cam or E.camera(cx=width / 2.0, cy=height / 2.0)
    rng = np.random.RandomState(seed)
    # points in a box that the whole drive sees: placed in the camera frame of a random frame
    true = []
    R, t = np.eye(3), np.zeros(3)
    for f in range(n_frames):
        if f:
            R = R.dot(rot([0.0, np.deg2rad(yaw_deg), 0.0]))
            t = t + R.dot([0.0, 0.0, step])
        true.append((R.copy(), t.copy()))
    pts = np.zeros((n_points, 3))
    for k in range(n_points):
        f = rng.randint(n_frames)
        Z = rng.uniform(*z_range)
        u, v = rng.uniform(0, width), rng.uniform(0, height)
        pts[k] = true[f][0].dot([(u - cam["cx"]) * Z / cam["fx"], (v - cam["cy"]) * Z / cam["fy"], Z]) + true[f][1]
    frames, prev_index = [], {}
    oR, ot = np.eye(3), np.zeros(3)
    for f in range(n_frames):
        R, t = true[f]
        if f:
            Rp, tp = true[f - 1]
            dR, dt = Rp.T.dot(R), Rp.T.dot(t - tp)
            dR = dR.dot(rot(np.deg2rad(rot_noise_deg) * rng.standard_normal(3)))
            dt = dt + trans_noise * rng.standard_normal(3)
            ot = ot + oR.dot(dt)
            oR = oR.dot(dR)
        q = (pts - t).dot(R)
        kl, kr, index = [], [], {}
        for k in range(n_points):
            if q[k, 2] <= 1.0:
                continue
            u, v = cam["fx"] * q[k, 0] / q[k, 2] + cam["cx"], cam["fy"] * q[k, 1] / q[k, 2] + cam["cy"]
            ur = cam["fx"] * (q[k, 0] - cam["baseline"]) / q[k, 2] + cam["cx"]
            if (clip and not (0 <= u < width and 0 <= v < height and 0 <= ur < width)) or rng.uniform() < missing:
                continue
            if pixel:
                u, v, ur = (np.round(x / pixel) * pixel for x in (u, v, ur))
            index[k] = len(kl)
            kl.append((u, v)); kr.append((ur, v))
        kpL, kpR = np.zeros(len(kl), E.KEYPOINT_DTYPE), np.zeros(len(kr), E.KEYPOINT_DTYPE)
        if kl:
            kpL["x"], kpL["y"] = np.array(kl, np.float32).T
            kpR["x"], kpR["y"] = np.array(kr, np.float32).T
        stereo = np.zeros(len(kl), E.MATCH_DTYPE)
        stereo["query"] = stereo["train"] = np.arange(len(kl))
        common = sorted((i, prev_index[k]) for k, i in index.items() if k in prev_index)
        temporal = np.zeros(len(common), E.MATCH_DTYPE)
        if common:
            temporal["query"], temporal["train"] = np.array(common).T
        frames.append(dict(true=pose12(R, t), odom=pose12(oR, ot), kpL=kpL, kpR=kpR, stereo=stereo, temporal=temporal))
        prev_index = index
    return frames


def pose_errors(est, true):
    """Worst translation (m) and rotation (degrees) error of est [n, 12] against true [n, 12], both expressed relative to their row 0."""
    def rel(P0, Pk):
        R0, t0, Rk, tk = P0.reshape(3, 4)[:, :3], P0.reshape(3, 4)[:, 3], Pk.reshape(3, 4)[:, :3], Pk.reshape(3, 4)[:, 3]
        return R0.T.dot(Rk), R0.T.dot(tk - t0)
    wt = wr = 0.0
    for k in range(1, len(est)):
        Re, te = rel(est[0], est[k])
        Rt, tt = rel(true[0], true[k])
        wt = max(wt, float(np.linalg.norm(te - tt)))
        c = min(1.0, max(-1.0, (np.trace(Re.T.dot(Rt)) - 1.0) / 2.0))
        wr = max(wr, float(np.degrees(np.arccos(c))))
    return wt, wr

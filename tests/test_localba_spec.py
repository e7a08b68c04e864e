"""CPU tests of spec S32, windowed bundle adjustment over the last frames: the restatement tests/np_localba.py against a
hand-worked case, a scalar twin, central differences, a dense solve of the full normal equations and the edge cases of the spec; the
track building; the accuracy of the spec on a synthetic drive; the exported interface and the argument checks that need no device.
The scenes at the top are shared with tests/test_gpu_localba.py."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import np_ego as E
import np_localba as B
import np_posegraph as P

CAM = E.camera(cx=160.0, cy=96.0)                                        # the scene of the accuracy figures: 320 x 192, fx = fy = 300
HAND = E.camera(fx=256.0, fy=256.0, cx=8.0, cy=4.0, baseline=0.5)        # S25's hand camera: fx * baseline = 128


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def truncate(frames, n):
    """The drive with every keypoint list cut to its first n entries and the match lists to what is left."""
    out, n_prev = [], 0
    for f in frames:
        k = min(n, len(f["kpL"]))
        st = f["stereo"][(f["stereo"]["query"] < k) & (f["stereo"]["train"] < k)]
        te = f["temporal"][(f["temporal"]["query"] < k) & (f["temporal"]["train"] < n_prev)]
        out.append(dict(f, kpL=f["kpL"][:k], kpR=f["kpR"][:k], stereo=st, temporal=te))
        n_prev = k
    return out


def rigid(n_points, n_frames, seed, **kw):
    """A slow drive in which every frame sees every point: exactly n_points points, each observed n_frames times."""
    return B.drive(seed, n_frames, n_points, CAM, step=0.1, yaw_deg=0.3, missing=0.0, clip=False, z_range=(6.0, 20.0), **kw)


def pushed(frames, window, max_points, p=None, cam=CAM, max_features=None, optimise=False):
    """-> (the Window after pushing the frames (and optimising after each), the counts and results per frame)."""
    p = p or B.params()
    win = B.Window(max_features or max(len(f["kpL"]) for f in frames) + 1, window, max_points)
    log = []
    for k, f in enumerate(frames):
        c = win.push(cam, p, k + 1, f["odom"], f["kpL"], f["kpR"], f["stereo"], f["temporal"])
        log.append((c, win.optimize(cam, p) if optimise else None))
    return win, log


def turned(frames, k, yaw_deg=80.0):
    """The drive with frame k's pose turned about the vertical axis: most of what it observes lies behind that pose."""
    out = [dict(f) for f in frames]
    m = np.array(out[k]["odom"]).reshape(3, 4)
    m[:, :3] = m[:, :3].dot(B.rot([0.0, np.deg2rad(yaw_deg), 0.0]))
    out[k]["odom"] = m.reshape(12)
    return out


def starved(frames, k, keep=3):
    """The drive with frame k's temporal list cut to `keep` matches: it continues `keep` points only."""
    out = [dict(f) for f in frames]
    out[k]["temporal"] = out[k]["temporal"][:keep]
    return out


def degenerate():
    """Two frames that share one point (and bear others that stay inactive): three residual rows per frame cannot fix six pose
    parameters, the reduced system is singular."""
    frames = rigid(5, 2, seed=3)
    frames[1]["temporal"] = frames[1]["temporal"][:1]
    return frames, B.params(min_frame_observations=0)


def hand_case():
    """Two frames at the origin with the identity rotation, three points at Z = 2; frame 1 sees every point one pixel to the right in both
    images, which is what a camera 1 / 128 m to the left sees.  -> (Window, params)."""
    pts = [(0.0, 0.0, 2.0), (1.0, 0.0, 2.0), (0.0, 1.0, 2.0)]
    kpL, kpR = np.zeros(3, E.KEYPOINT_DTYPE), np.zeros(3, E.KEYPOINT_DTYPE)
    for k, (x, y, z) in enumerate(pts):
        kpL[k]["x"], kpL[k]["y"] = 256.0 * x / z + 8.0, 256.0 * y / z + 4.0
        kpR[k]["x"], kpR[k]["y"] = 256.0 * (x - 0.5) / z + 8.0, kpL[k]["y"]
    m = np.zeros(3, E.MATCH_DTYPE)
    m["query"] = m["train"] = np.arange(3)
    p = B.params(min_frame_observations=3)
    win = B.Window(4, 2, 64)
    win.push(HAND, p, 1, E.POSE_IDENTITY, kpL, kpR, m, m[:0])
    kpL1, kpR1 = kpL.copy(), kpR.copy()
    kpL1["x"] += 1.0
    kpR1["x"] += 1.0
    win.push(HAND, p, 2, E.POSE_IDENTITY, kpL1, kpR1, m, m)
    return win, p


# ---- the hand-worked case ----------------------------------------------------------------------------------------------------------------
def test_hand_worked_case():
    """Point 0 = (0, 0, 2) in both frames: a = c = 128, b = d = 0, b_r = 32, so J_q = J_p = [[128, 0, 0], [0, 128, 0], [128, 0, 32]] and
    J_c rows (0, -256, 0, -128, 0, 0), (256, 0, 0, 0, -128, 0), (0, -256, 0, -128, 0, -32); every weight is 1 (n2 = 2 <= 4).
      V_0 = 2 J_p^T J_p = [[65536, 0, 8192], [0, 32768, 0], [8192, 0, 2048]]
      W_0,1 = J_c^T J_p = [[0, 32768, 0], [-65536, 0, -8192], [0, 0, 0], [-32768, 0, -4096], [0, -16384, 0], [-4096, 0, -1024]]
      g_0 = J_p^T e with e = (-1, 0, -1): (-256, 0, -32)
    The step is exact: the residuals are linear in a sideways translation at a fixed depth, so delta = (0, 0, 0, -1/128, 0, 0) and no point
    moves; S and r are checked against exact rational arithmetic over the three points."""
    win, p = hand_case()
    assert win.points()[:3].tolist() == [[0.0, 0.0, 2.0, 2.0], [1.0, 0.0, 2.0, 2.0], [0.0, 1.0, 2.0, 2.0]] and win.track_of[:3].tolist() == [0, 1, 2]
    sy = win.system(HAND, p)
    V = [[float(sy["V"][k][l][0]) for l in range(3)] for k in range(3)]
    assert [V[0][0], V[0][1], V[0][2], V[1][1], V[1][2], V[2][2]] == [65536.0, 0.0, 8192.0, 32768.0, 0.0, 2048.0]
    W = [[float(sy["W"][1][i][k][0]) for k in range(3)] for i in range(6)]
    assert W == [[0.0, 32768.0, 0.0], [-65536.0, 0.0, -8192.0], [0.0, 0.0, 0.0], [-32768.0, 0.0, -4096.0], [0.0, -16384.0, 0.0], [-4096.0, 0.0, -1024.0]]
    assert [float(sy["gp"][k][0]) for k in range(3)] == [-256.0, 0.0, -32.0]
    # S = U - sum W V^-1 W^T and r = -g + sum W V^-1 g_p in rationals, from the same Jacobians
    S = [[Fraction(0)] * 6 for _ in range(6)]
    r = [Fraction(0)] * 6
    for k in range(3):
        o = {n: [[Fraction(float(v[k])) for v in row] for row in sy["lin"][1][0][n]] for n in ("Jc", "Jp")}
        e = [Fraction(-1), Fraction(0), Fraction(-1)]
        Vp = [[2 * sum(o["Jp"][m][a] * o["Jp"][m][b] for m in range(3)) for b in range(3)] for a in range(3)]
        Wp = [[sum(o["Jc"][m][i] * o["Jp"][m][a] for m in range(3)) for a in range(3)] for i in range(6)]
        gpp = [sum(o["Jp"][m][a] * e[m] for m in range(3)) for a in range(3)]
        inv = frac_inverse(Vp)
        Y = [[sum(Wp[i][a] * inv[a][b] for a in range(3)) for b in range(3)] for i in range(6)]
        for i in range(6):
            r[i] += -sum(o["Jc"][m][i] * e[m] for m in range(3)) + sum(Y[i][a] * gpp[a] for a in range(3))
            for j in range(6):
                S[i][j] += sum(o["Jc"][m][i] * o["Jc"][m][j] for m in range(3)) - sum(Y[i][a] * Wp[j][a] for a in range(3))
    for i in range(6):
        assert float(r[i]) == pytest.approx(sy["C"][6][i], rel=1e-12, abs=1e-9)
        for j in range(i, 6):
            assert float(S[i][j]) == pytest.approx(sy["C"][j][i], rel=1e-12, abs=1e-6)
    _, delta, dX = win.deltas(HAND, p)
    assert np.allclose(delta[1], [0, 0, 0, -1.0 / 128, 0, 0], atol=1e-12) and np.abs(dX).max() < 1e-12
    res = win.optimize(HAND, dict(p, iterations=1))
    assert res["status"] == 1 and res["cost_before"] == 6.0 and res["cost_after"] < 1e-20 and (res["n_points_active"], res["n_observations"]) == (3, 6)
    assert np.allclose(win.poses()[0][1], [1, 0, 0, -1.0 / 128, 0, 1, 0, 0, 0, 0, 1, 0], atol=1e-13)


def frac_inverse(A):
    n = len(A)
    M = [list(row) + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(A)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c:
                M[r] = [a - M[r][c] * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


# ---- the vectorised restatement against a scalar twin ------------------------------------------------------------------------------------
def scalar_lane_sum(values, mask):
    v = [0.0] * B.LANES
    for k, (x, m) in enumerate(zip(values, mask)):
        if m:
            v[k % B.LANES] = v[k % B.LANES] + x
    o = B.LANES // 2
    while o:
        v = [v[l] + v[l ^ o] for l in range(B.LANES)]
        o //= 2
    return v[0]


def scalar_system(win, cam, p):
    """One point and one observation at a time with Python floats: -> (C, the update of every point slot [M][3] or None, held)."""
    F, M = win.frames(), win.max_points
    est = [[float(v) for v in win.est[win.slot(a)]] for a in range(F)]
    act = [bool(win.state[k] != 0 and win.n_obs[k] >= p["min_observations"]) for k in range(M)]

    def obs(k, a):
        ob = win.obs[k, win.slot(a)]
        if not act[k] or not ob["valid"]:
            return None
        o = B.observe(cam, est[a], [np.float64(v) for v in win.X[k]], np.float64(ob["u"]), np.float64(ob["v"]), np.float64(ob["ur"]), p["huber"])
        return o if bool(o["front"]) else None
    lin = [[obs(k, a) for a in range(F)] for k in range(M)]
    held = [a >= 1 and sum(1 for k in range(M) if lin[k][a] is not None) < p["min_frame_observations"] for a in range(F)]
    blocks = [None] * M
    for k in range(M):
        if not act[k]:
            continue
        V, gp = [[0.0] * 3 for _ in range(3)], [0.0] * 3
        for a in range(F):
            o = lin[k][a]
            if o is None or held[a]:
                continue
            for i in range(3):
                for j in range(i, 3):
                    V[i][j] = V[i][j] + float(B.jtj(o, o["Jp"], i, o["Jp"], j))
                gp[i] = gp[i] + float(B.jte(o, o["Jp"], i))
        for i in range(3):
            V[i][i] = V[i][i] + p["damping"]
        L = [[0.0] * 3 for _ in range(3)]
        ok = True
        for j in range(3):
            s = V[j][j]
            for q in range(j):
                s = s - L[j][q] * L[j][q]
            if not s > 0:
                ok = False
                break
            L[j][j] = math.sqrt(s)
            for i in range(j + 1, 3):
                s = V[j][i]
                for q in range(j):
                    s = s - L[i][q] * L[j][q]
                L[i][j] = s / L[j][j]
        if not ok:
            continue
        cols = [B.solve3(L, [1.0 if r == c else 0.0 for r in range(3)]) for c in range(3)]
        Vi = [[cols[c][r] for c in range(3)] for r in range(3)]
        Wb = {a: [[float(B.jtj(lin[k][a], lin[k][a]["Jc"], i, lin[k][a]["Jp"], q)) for q in range(3)] for i in range(6)]
              for a in range(1, F) if lin[k][a] is not None and not held[a]}
        blocks[k] = (Vi, gp, Wb)
    n = 6 * (F - 1)
    Cm = [[0.0] * n for _ in range(n + 1)]
    for a in range(1, F):
        if held[a]:
            for i in range(6):
                Cm[6 * (a - 1) + i][6 * (a - 1) + i] = 1.0
            continue
        use = [blocks[k] is not None and a in blocks[k][2] for k in range(M)]
        Y = [[[B.dot3(blocks[k][2][a][i], [blocks[k][0][0][q], blocks[k][0][1][q], blocks[k][0][2][q]]) for q in range(3)] for i in range(6)] if use[k] else None
             for k in range(M)]
        for i in range(6):
            g = scalar_lane_sum([float(B.jte(lin[k][a], lin[k][a]["Jc"], i)) if use[k] else 0.0 for k in range(M)], use)
            z = scalar_lane_sum([B.dot3(Y[k][i], blocks[k][1]) if use[k] else 0.0 for k in range(M)], use)
            Cm[n][6 * (a - 1) + i] = (-g) + z
        for b in range(a, F):
            both = [use[k] and b in blocks[k][2] for k in range(M)]
            for i in range(6):
                for j in range(i if a == b else 0, 6):
                    t = scalar_lane_sum([B.dot3(Y[k][i], blocks[k][2][b][j]) if both[k] else 0.0 for k in range(M)], both)
                    u = 0.0
                    if a == b:
                        u = scalar_lane_sum([float(B.jtj(lin[k][a], lin[k][a]["Jc"], i, lin[k][a]["Jc"], j)) if use[k] else 0.0 for k in range(M)], use)
                        if i == j:
                            u = u + p["damping"]
                    Cm[6 * (b - 1) + j][6 * (a - 1) + i] = u - t
    y = P.Graph.loop_solve(None, Cm)
    dX = None
    if y is not None:
        dX = [[0.0] * 3 for _ in range(M)]
        for k in range(M):
            if blocks[k] is None:
                continue
            Vi, gp, Wb = blocks[k]
            h = [-gp[q] for q in range(3)]
            for a in sorted(Wb):
                for q in range(3):
                    s = Wb[a][0][q] * y[6 * (a - 1)]
                    for i in range(1, 6):
                        s = s + Wb[a][i][q] * y[6 * (a - 1) + i]
                    h[q] = h[q] - s
            dX[k] = [B.dot3(Vi[r], h) for r in range(3)]
    return Cm, dX, held


@pytest.mark.parametrize("case", ["drive", "held", "behind", "damped"])
def test_vectorised_restatement_equals_the_scalar_twin(case):
    frames = truncate(B.drive(7, 4, 200, CAM, step=0.4, yaw_deg=1.5), 40)
    p = B.params(damping=0.5 if case == "damped" else 0.0)
    if case == "held":
        frames = starved(frames, 3, keep=2)
    if case == "behind":
        frames = turned(frames, 2, 100.0)
    win, _ = pushed(frames, 4, 64, p=p)
    with np.errstate(all="ignore"):
        Cm, dX, held = scalar_system(win, CAM, p)
        sy = win.system(CAM, p)
        got = win.deltas(CAM, p)
    assert held == sy["held"] and (case != "held" or held == [False, False, False, True])
    assert np.array(Cm).tobytes() == np.array(sy["C"]).tobytes()
    assert got is not None and np.array(dX).tobytes() == got[2].tobytes() and np.abs(got[2]).max() > 0


def test_lane_sums_is_s23s_sum():
    rng = np.random.RandomState(5)
    for n in (1, 255, 256, 257, 513, 1000):
        x, m = rng.standard_normal((3, n)) * 10.0 ** rng.randint(-6, 6, (3, n)), rng.uniform(size=n) < 0.7
        got = B.lane_sums(x, m)
        assert got == [E.lane_sum(x[k], m) for k in range(3)] == [scalar_lane_sum(x[k], m) for k in range(3)]
    assert B.lane_sums([np.array([np.inf, 1.0])], [False, True]) == [1.0]          # a skipped slot adds nothing, whatever it holds


# ---- Jacobians, the Schur step ---------------------------------------------------------------------------------------------------------
def test_jacobians_against_central_differences():
    """Step 1e-6 on the pose (through update_right) and on the point; 20 random observations with a residual of a few pixels.  Measured
    largest difference over the largest entry: 1.2e-10 (pose block), 1.2e-9 (point block); asserted at 1e-7, as S29's Jacobians are:
    the rounding error of the difference quotient, some 1e-16 / 1e-6 times the residual's size, leaves that margin."""
    rng = np.random.RandomState(11)
    worst = [0.0, 0.0]
    for _ in range(20):
        est = B.pose12(B.rot(rng.uniform(-0.3, 0.3, 3)), rng.uniform(-1, 1, 3))
        q = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 20)])
        X = est.reshape(3, 4)[:, :3].dot(q) + est.reshape(3, 4)[:, 3]
        u, v, ur = (np.float64(np.float32(x)) for x in (300 * q[0] / q[2] + 160 + rng.uniform(-3, 3), 300 * q[1] / q[2] + 96 + rng.uniform(-3, 3),
                                                        300 * (q[0] - 0.5) / q[2] + 160 + rng.uniform(-3, 3)))

        def e(est_, X_):
            return np.array([float(x) for x in B.observe(CAM, [float(x) for x in est_], [np.float64(x) for x in X_], u, v, ur, 2.0)["e"]])
        o = B.observe(CAM, [float(x) for x in est], [np.float64(x) for x in X], u, v, ur, 2.0)
        Jc, Jp = np.array([[float(x) for x in row] for row in o["Jc"]]), np.array([[float(x) for x in row] for row in o["Jp"]])
        h = 1e-6
        for k in range(6):
            d = [0.0] * 6
            d[k] = h
            plus, minus = P.join(P.update_right(P.split(est), d)), P.join(P.update_right(P.split(est), [-x for x in d]))
            worst[0] = max(worst[0], np.abs((e(plus, X) - e(minus, X)) / (2 * h) - Jc[:, k]).max() / np.abs(Jc).max())
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            worst[1] = max(worst[1], np.abs((e(est, X + d) - e(est, X - d)) / (2 * h) - Jp[:, k]).max() / np.abs(Jp).max())
    print("central differences: pose block %.3g, point block %.3g" % tuple(worst))
    assert max(worst) < 1e-7


def dense_step(win, cam, p):
    """np.linalg.solve of the densely assembled normal equations over the free frames and the active points -> (delta [F - 1, 6], dX)."""
    F, M = win.frames(), win.max_points
    act, lin = win.linearise(cam, p)
    idx = {int(k): n for n, k in enumerate(np.nonzero(act)[0])}
    n = 6 * (F - 1) + 3 * len(idx)
    H, g = np.zeros((n, n)), np.zeros(n)
    for a in range(F):
        o, usable = lin[a]
        for k in np.nonzero(usable)[0]:
            J = np.zeros((3, n))
            if a >= 1:
                J[:, 6 * (a - 1):6 * a] = [[float(o["Jc"][m][i][k]) for i in range(6)] for m in range(3)]
            c0 = 6 * (F - 1) + 3 * idx[int(k)]
            J[:, c0:c0 + 3] = [[float(o["Jp"][m][i][k]) for i in range(3)] for m in range(3)]
            w = float(o["w"][k])
            H += w * J.T.dot(J)
            g += w * J.T.dot([float(o["e"][m][k]) for m in range(3)])
    x = np.linalg.solve(H, -g)
    dX = np.zeros((M, 3))
    for k, m in idx.items():
        dX[k] = x[6 * (F - 1) + 3 * m:6 * (F - 1) + 3 * m + 3]
    return x[:6 * (F - 1)].reshape(F - 1, 6), dX


def test_schur_step_against_a_dense_solve():
    """The largest difference over the largest entry of the step.  Measured: 7.7e-13 at (W, points) = (4, 150), 9.9e-12 at (8, 300); the
    bound is 100 times that and no more than 1e-8."""
    for (W, n, seed), measured in (((4, 150, 21), 7.7e-13), ((8, 300, 22), 9.9e-12)):
        win, _ = pushed(B.drive(seed, W, n, CAM), W, 1024)
        p = B.params(min_frame_observations=1)
        _, delta, dX = win.deltas(CAM, p)
        want_delta, want_dX = dense_step(win, CAM, p)
        got = np.concatenate([np.array(delta[1:]).reshape(-1), dX.reshape(-1)])
        want = np.concatenate([want_delta.reshape(-1), want_dX.reshape(-1)])
        diff = np.abs(got - want).max() / np.abs(want).max()
        print("schur vs dense at (%d, %d): %.3g" % (W, n, diff))
        assert diff <= min(100 * measured, 1e-8)


# ---- the edge cases of a step ---------------------------------------------------------------------------------------------------------------
def test_huber_at_the_threshold():
    """n2 = k k exactly keeps the quadratic branch; one ulp above takes the other, and the two branches meet there."""
    est, X = E.POSE_IDENTITY, [np.float64(0.0), np.float64(0.0), np.float64(2.0)]
    o = B.observe(HAND, est, X, np.float64(10.0), np.float64(4.0), np.float64(-56.0), 2.0)         # e = (-2, 0, 0)
    assert [float(x) for x in o["e"]] == [-2.0, 0.0, 0.0] and float(o["n2"]) == 4.0 and float(o["w"]) == 1.0 and float(o["rho"]) == 4.0
    k = float(np.nextafter(2.0, 0.0))
    o = B.observe(HAND, est, X, np.float64(10.0), np.float64(4.0), np.float64(-56.0), k)
    assert float(o["w"]) == k / 2.0 < 1.0 and float(o["rho"]) == (2.0 * k) * 2.0 - k * k and abs(float(o["rho"]) - 4.0) < 1e-14
    o = B.observe(HAND, est, X, np.float64(108.0), np.float64(4.0), np.float64(-56.0), 2.0)        # a gross error is kept, with a small weight
    assert float(o["w"]) == 2.0 / 100.0 and float(o["rho"]) == 4.0 * 100.0 - 4.0


def test_a_point_behind_the_camera_is_skipped_not_an_error():
    for z, front in ((2.0, True), (0.0, False), (-2.0, False)):
        o = B.observe(HAND, E.POSE_IDENTITY, [np.float64(0.0), np.float64(0.0), np.float64(z)], np.float64(8.0), np.float64(4.0), np.float64(-56.0), 2.0)
        assert bool(o["front"]) == front
    frames = turned(truncate(B.drive(7, 4, 200, CAM, step=0.4, yaw_deg=1.5), 40), 2, 100.0)
    win, _ = pushed(frames, 4, 64)
    act, lin = win.linearise(CAM, B.params())
    seen = act & (win.obs["valid"][:, win.slot(2)] != 0)
    assert 0 < int(lin[2][1].sum()) < int(seen.sum())                                              # some of frame 2's observations are behind it
    cost, n_obs, _ = win.cost(CAM, B.params())
    assert n_obs == sum(int(u.sum()) for _, u in lin) and np.isfinite(cost)
    sy = win.system(CAM, B.params())
    assert np.isfinite(np.array(sy["C"])).all()


def test_a_held_frame_keeps_its_pose_and_gives_nothing():
    frames = starved(truncate(B.drive(7, 4, 200, CAM, step=0.4, yaw_deg=1.5), 40), 3, keep=2)
    win, _ = pushed(frames, 4, 64)
    p = B.params(iterations=1)
    sy = win.system(CAM, p)
    assert sy["held"] == [False, False, False, True] and not sy["used"][3].any()
    Cm = np.array(sy["C"])
    assert (Cm[12:18, 12:18] == np.eye(6)).all() and not Cm[12:18, :12].any() and not Cm[18, 12:].any()
    newest = win.est[win.slot(3)].copy()
    res = win.optimize(CAM, p)
    assert res["status"] == 1 and res["n_held"] == 1 and (win.est[win.slot(3)] == newest).all()
    assert B.params()["min_frame_observations"] == 6 and win.optimize(CAM, B.params(min_frame_observations=2))["n_held"] == 0


def test_a_failed_pivot_moves_nothing():
    """The premise of the GPU test of the same name: two frames that share one active point."""
    frames, p = degenerate()
    win, _ = pushed(frames, 2, 64, p=p, max_features=8)
    assert int(win.active(p).sum()) == 1 and win.deltas(CAM, p) is None
    before = (win.est.copy(), win.X.copy())
    res = win.optimize(CAM, p)
    assert res["status"] == 0 and res["cost_after"] == res["cost_before"] > 0 and res["n_held"] == 0
    assert (win.est == before[0]).all() and (win.X == before[1]).all()
    # with the default min_frame_observations the frame is held instead and the call succeeds without moving a pose
    res = win.optimize(CAM, B.params())
    assert res["status"] == 1 and res["n_held"] == 4 and (win.est == before[0]).all()


def test_a_window_of_one_frame_and_one_without_active_points():
    frames = truncate(B.drive(7, 3, 200, CAM), 30)
    win, _ = pushed(frames[:1], 4, 64)
    res = win.optimize(CAM, B.params())
    assert res["status"] == 1 and res["n_frames"] == 1 and res["n_points_active"] == 0 and res["cost_before"] == res["cost_after"] == 0.0
    res = win.optimize(CAM, B.params(min_observations=1))                   # active points, but nothing to move
    assert res["status"] == 1 and res["n_points_active"] == int((win.state != 0).sum()) > 0 and res["cost_after"] == res["cost_before"]
    empty = B.Window(8, 4, 64)
    assert empty.optimize(CAM, B.params())["status"] == 1
    win2, _ = pushed([frames[0], dict(frames[1], temporal=frames[1]["temporal"][:0])], 4, 128)   # two frames that share nothing
    before = win2.est.copy()
    res = win2.optimize(CAM, B.params())
    assert res["status"] == 1 and res["n_frames"] == 2 and res["n_points_active"] == 0 and (win2.est == before).all()


# ---- track building --------------------------------------------------------------------------------------------------------------------------
def keypoints(disparities, x0=100.0):
    """Left / right keypoint records: keypoint k at (x0 + 10 k, 50 + k) with the given disparity."""
    n = len(disparities)
    kpL, kpR = np.zeros(n, E.KEYPOINT_DTYPE), np.zeros(n, E.KEYPOINT_DTYPE)
    kpL["x"], kpL["y"] = x0 + 10.0 * np.arange(n), 50.0 + np.arange(n)
    kpR["x"], kpR["y"] = kpL["x"] - np.array(disparities, np.float32), kpL["y"]
    return kpL, kpR


def matches(pairs):
    m = np.zeros(len(pairs), E.MATCH_DTYPE)
    if pairs:
        m["query"], m["train"] = np.array(pairs).T
    return m


def identity(n):
    return matches([(k, k) for k in range(n)])


def consistent(win):
    """The tables agree with each other: n_obs counts the row's observations, a slot is live iff it has one, a free slot is all zero."""
    valid = win.obs["valid"] != 0
    assert (win.n_obs == valid.sum(axis=1)).all() and ((win.state != 0) == (win.n_obs > 0)).all()
    assert not win.X[win.state == 0].any() and not valid[:, [s for s in range(win.window) if s >= win.n_pushed]].any()
    live = win.track_of[win.track_of >= 0]
    assert len(set(live.tolist())) == len(live) and (win.state[live] != 0).all()
    s = (win.n_pushed - 1) % win.window
    assert sorted(live.tolist()) == np.nonzero(valid[:, s])[0].tolist()


def test_continuation_birth_and_the_slot_order():
    p = B.params()
    win = B.Window(8, 4, 64)
    kpL, kpR = keypoints([8, 8, 8, 8])
    c = win.push(CAM, p, 1, E.POSE_IDENTITY, kpL, kpR, identity(4), matches([(0, 0)]))            # the first push ignores its temporal list
    assert c.tolist() == [4, 4, 0, 4, 0, 0, 4, 1] and win.track_of.tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    Z = (300.0 * 0.5) / 8.0
    assert win.X[1].tolist() == [((110.0 - 160.0) * Z) / 300.0, ((51.0 - 96.0) * Z) / 300.0, Z] and win.n_obs[:5].tolist() == [1, 1, 1, 1, 0]
    kpL, kpR = keypoints([8, 8, 8, 8, 0.5, 8])
    c = win.push(CAM, p, 2, E.POSE_IDENTITY, kpL, kpR, identity(6), matches([(0, 2), (1, 0), (3, 3), (4, 1)]))
    # 0, 1 and 3 continue points 2, 0 and 3; 4 has a temporal match but no valid observation; 2 and 5 are born into slots 4 and 5
    assert c.tolist() == [6, 5, 3, 2, 0, 0, 6, 2] and win.track_of.tolist() == [2, 0, 4, 3, -1, 5, -1, -1]
    assert win.n_obs[:7].tolist() == [2, 1, 2, 2, 1, 1, 0] and win.obs[2, 1].tolist() == (100.0, 50.0, 92.0, 1) and win.obs[2, 0].tolist() == (120.0, 52.0, 112.0, 1)
    consistent(win)


def test_of_several_indices_that_name_one_point_the_smallest_wins():
    p = B.params()
    win = B.Window(8, 3, 64)
    kpL, kpR = keypoints([8, 8, 8])
    win.push(CAM, p, 1, E.POSE_IDENTITY, kpL, kpR, identity(3), matches([]))
    c = win.push(CAM, p, 2, E.POSE_IDENTITY, kpL, kpR, identity(3), matches([(0, 1), (1, 1), (2, 1)]))   # cross_check off: three queries, one train
    assert c.tolist() == [3, 3, 1, 2, 0, 0, 5, 2] and win.track_of[:3].tolist() == [1, 3, 4]
    # the winner must have a valid observation: with index 0 invalid, index 1 wins
    win = B.Window(8, 3, 64)
    win.push(CAM, p, 1, E.POSE_IDENTITY, kpL, kpR, identity(3), matches([]))
    kpL2, kpR2 = keypoints([0.25, 8, 8])
    c = win.push(CAM, p, 2, E.POSE_IDENTITY, kpL2, kpR2, identity(3), matches([(0, 1), (1, 1), (2, 1)]))
    assert c.tolist() == [3, 2, 1, 1, 0, 0, 4, 2] and win.track_of[:3].tolist() == [-1, 1, 3]
    consistent(win)


def test_eviction_frees_points_and_the_same_push_reuses_their_slots():
    """W + 3 pushes at W = 3.  Frame f holds 6 keypoints; keypoint k continues keypoint k of the frame before while k >= f mod 3, so every
    frame bears points and lets tracks end."""
    p = B.params()
    win = B.Window(8, 3, 64)
    kpL, kpR = keypoints([8] * 6)
    log = []
    for f in range(6):
        before = win.state.copy()
        temporal = matches([(k, k) for k in range(6) if k >= f % 3])
        doomed = 0
        if win.n_pushed >= 3:
            s = win.n_pushed % 3
            seen = win.obs["valid"][:, s] != 0
            doomed = int((seen & (win.n_obs == 1)).sum())
            doomed_slots = np.nonzero(seen & (win.n_obs == 1))[0]
        c = win.push(CAM, p, f + 1, E.POSE_IDENTITY, kpL, kpR, identity(6), temporal)
        consistent(win)
        assert c[5] == doomed and c[2] == (6 - f % 3 if f else 0) and c[3] == 6 - c[2] and c[7] == min(f + 1, 3)
        if doomed and c[3]:
            free_before = sorted(set(np.nonzero(before == 0)[0].tolist()) | set(doomed_slots.tolist()))
            born = sorted(int(t) for t in win.track_of[:6] if before[t] == 0 or t in doomed_slots)
            assert born == free_before[:len(born)]                                                     # the lowest free slots, those just freed included
        log.append(c.tolist())
    assert sum(c[5] for c in log) > 0 and log[-1][6] == int((win.state != 0).sum())
    assert win.poses()[1].tolist() == [4, 5, 6]
    # frees and reuse in one push: three frames without a temporal match at W = 2; the third evicts the first and takes its three slots
    win = B.Window(8, 2, 64)
    kpL, kpR = keypoints([8] * 3)
    for f, (counts, track) in enumerate((([3, 3, 0, 3, 0, 0, 3, 1], [0, 1, 2]), ([3, 3, 0, 3, 0, 0, 6, 2], [3, 4, 5]), ([3, 3, 0, 3, 0, 3, 6, 2], [0, 1, 2]))):
        assert win.push(CAM, p, f + 1, E.POSE_IDENTITY, kpL, kpR, identity(3), matches([])).tolist() == counts and win.track_of[:3].tolist() == track
        consistent(win)


def test_a_full_point_table_drops_and_counts():
    p = B.params()
    win = B.Window(80, 2, 64)
    kpL, kpR = keypoints([8] * 70)
    c = win.push(CAM, p, 1, E.POSE_IDENTITY, kpL, kpR, identity(70), matches([]))
    assert c.tolist() == [70, 70, 0, 64, 6, 0, 64, 1] and win.track_of[:70].tolist() == list(range(64)) + [-1] * 6
    c = win.push(CAM, p, 2, E.POSE_IDENTITY, kpL, kpR, identity(70), identity(70))
    assert c.tolist() == [70, 70, 64, 0, 6, 0, 64, 2]                                                  # 64 .. 69 match a keypoint that has no point
    consistent(win)


def test_an_invalid_stereo_observation_is_no_observation():
    p = B.params(min_disparity=1.0)
    kpL, kpR = keypoints([1.0, 0.999, -3.0, 8.0, 8.0])
    kpR["x"][3] = np.nan
    win = B.Window(8, 2, 64)
    stereo = matches([(0, 0), (1, 1), (2, 2), (3, 3), (4, 7), (9, 0), (-1, 0), (4, -1)])               # train 7: beyond kpR; queries outside the set
    c = win.push(CAM, p, 1, E.POSE_IDENTITY, kpL, kpR, stereo, matches([]))
    assert c.tolist() == [5, 1, 0, 1, 0, 0, 1, 1] and win.track_of[:5].tolist() == [0, -1, -1, -1, -1]
    c = win.push(CAM, p, 2, E.POSE_IDENTITY, kpL, kpR, stereo, matches([(0, 0), (1, 0), (0, 8), (0, -1)]))   # trains outside [0, max_features)
    assert c.tolist() == [5, 1, 1, 0, 0, 0, 1, 2]
    consistent(win)


# ---- accuracy of the spec -------------------------------------------------------------------------------------------------------------------
# (window, points, iterations) -> the worst errors over seeds 0 .. 4, measured on this restatement: (metres, degrees) before and after
ACCURACY = {(8, 300, 4): ((0.1243, 0.872), (0.0024, 0.011)), (16, 400, 4): ((0.1799, 1.322), (0.0030, 0.013)), (2, 40, 4): ((0.0340, 0.317), (0.0051, 0.023))}


@pytest.mark.parametrize("case", sorted(ACCURACY), ids=str)
def test_accuracy_on_the_synthetic_drive(case):
    """fx = fy = 300, baseline 0.5, 320 x 192, points at Z in [5, 30] m, quarter-pixel observations with 15 % missing, 0.6 m and 2 degrees
    per frame, odometry noise of 0.15 degrees per axis and 2 cm per frame, chained; five seeds.  The worst pose error over the window
    relative to its oldest frame, asserted after the optimise at twice the measured figure; the Huber cost falls in every run."""
    W, n, it = case
    worst_before, worst_after = [0.0, 0.0], [0.0, 0.0]
    for seed in range(5):
        frames = B.drive(seed, W, n, CAM)
        p = B.params(iterations=it)
        win, _ = pushed(frames, W, 1024, p=p)
        true = np.array([f["true"] for f in frames])
        before = B.pose_errors(win.poses()[0], true)
        res = win.optimize(CAM, p)
        after = B.pose_errors(win.poses()[0], true)
        assert res["status"] == 1 and res["cost_after"] < res["cost_before"]
        worst_before = [max(a, b) for a, b in zip(worst_before, before)]
        worst_after = [max(a, b) for a, b in zip(worst_after, after)]
    print("accuracy at", case, "before %.4f m %.3f deg, after %.4f m %.3f deg" % tuple(worst_before + worst_after))
    assert worst_after[0] <= 2 * ACCURACY[case][1][0] and worst_after[1] <= 2 * ACCURACY[case][1][1]
    assert worst_after[0] < worst_before[0] / 4 and worst_after[1] < worst_before[1] / 4


def test_noise_free_observations_are_fitted_exactly():
    frames = B.drive(0, 8, 300, CAM, pixel=0)
    p = B.params(iterations=6)
    win, _ = pushed(frames, 8, 1024, p=p)
    res = win.optimize(CAM, p)
    wt, wr = B.pose_errors(win.poses()[0], np.array([f["true"] for f in frames]))
    assert res["status"] == 1 and wt < 1e-5 and wr < 1e-4 and res["cost_after"] < 1e-5          # float32 keypoints: 2e-5 pixels


# ---- the exported interface (fails before this feature) ------------------------------------------------------------------------------------
def test_defaults_struct_sizes_and_exports():
    import cartslam
    from cartslam import _lib
    p = cartslam.local_ba_params()
    assert {n: getattr(p, n) for n, _ in p._fields_} == B.params()
    assert C.sizeof(cartslam.LocalBAParams) == 40 and C.sizeof(cartslam.LocalBAResult) == 40 == B.RESULT_DTYPE.itemsize == cartslam.LOCAL_BA_RESULT_DTYPE.itemsize
    assert cartslam.LOCAL_BA_RESULT_DTYPE == B.RESULT_DTYPE and B.OBS_DTYPE.itemsize == 16
    assert [n for n, _ in cartslam.LocalBAResult._fields_] == list(B.RESULT_DTYPE.names)
    assert (_lib.LOCAL_BA_MAX_WINDOW, _lib.LOCAL_BA_MAX_POINTS, _lib.LOCAL_BA_MAX_ITERATIONS) == (B.MAX_WINDOW, 65536, B.MAX_ITERATIONS)
    lib = _lib.load()
    for name in ("default_params", "create", "destroy", "clear", "size", "push", "optimize", "poses", "points", "track_of"):
        assert hasattr(lib, "cart_local_ba_" + name) and "cart_local_ba_" + name in _lib.PROTOTYPES
    for name in ("LocalBA", "LocalBAParams", "LocalBAResult", "local_ba_params", "LOCAL_BA_RESULT_DTYPE"):
        assert hasattr(cartslam, name)
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cart_engine.h")).read()
    declared = [ln for ln in header.splitlines() if "cart_local_ba_" in ln and ln.startswith(("int ", "void "))]
    assert len(declared) == 10
    for ln in declared:
        above = header[:header.index(ln)].rstrip()
        comment = above[above.rindex("/*"):]
        assert "Extension" in comment and "S32" in comment, ln


def test_local_ba_params():
    import cartslam
    p = cartslam.local_ba_params(huber=1.5, iterations=2, min_frame_observations=0)
    assert (p.huber, p.iterations, p.min_frame_observations, p.min_disparity, p.damping, p.min_observations) == (1.5, 2, 0, 1.0, 0.0, 2)
    with pytest.raises(ValueError, match="cart_local_ba_params has no field inlier_threshold"):
        cartslam.local_ba_params(inlier_threshold=2.0)


def test_argument_checks_that_need_no_device():
    """Values and sizes are checked before the engine and before the object: every message names its argument."""
    import cartslam
    from cartslam import _lib
    lib = _lib.load()
    err = lambda: lib.cart_last_error(None).decode()   # noqa: E731
    out = C.c_void_p()
    for args, word in (((0, 8, 64), "max_features must be in [1, 65536]"), ((65537, 8, 64), "max_features"), ((8, 1, 64), "window must be in [2, 16]"),
                       ((8, 17, 64), "window"), ((8, 8, 63), "max_points must be in [64, 65536]"), ((8, 8, 65537), "max_points"), ((8, 8, 64), "bad arguments")):
        assert lib.cart_local_ba_create(None, *args, C.byref(out)) != 0 and word in err(), (args, err())
    cam = cartslam.EgoCamera(300.0, 300.0, 160.0, 96.0, 0.5)
    pose = (C.c_double * 12)(*E.POSE_IDENTITY)

    def push(p, camera=cam, pose_=pose):
        return lib.cart_local_ba_push(None, C.byref(camera) if camera else None, C.byref(p) if p else None, 1, pose_, *[None] * 9)
    for fields, word in ((dict(min_disparity=0.0), "min_disparity must be a positive number"), (dict(huber=float("nan")), "huber must be a positive number"),
                         (dict(damping=-0.5), "damping"), (dict(damping=float("inf")), "damping"), (dict(iterations=-1), "iterations must be in [0, 16]"),
                         (dict(iterations=17), "iterations"), (dict(min_observations=0), "min_observations must be in [1, 16]"), (dict(min_observations=17), "min_observations"),
                         (dict(min_frame_observations=-1), "min_frame_observations must be in [0, 65536]"), (dict(min_frame_observations=65537), "min_frame_observations")):
        p = cartslam.local_ba_params(**fields)
        assert push(p) != 0 and word in err(), (fields, err())
        assert lib.cart_local_ba_optimize(None, C.byref(cam), C.byref(p), None, None) != 0 and word in err(), (fields, err())
    ok = cartslam.local_ba_params()
    assert push(None) != 0 and "params is NULL" in err()
    assert push(ok, camera=None) != 0 and "camera is NULL" in err()
    assert push(ok, camera=cartslam.EgoCamera(300.0, 300.0, 160.0, 96.0, 0.0)) != 0 and "baseline" in err()
    assert push(ok, pose_=None) != 0 and "pose is NULL" in err()
    assert push(ok) != 0 and "ba is NULL" in err()                       # values first, then the object
    assert lib.cart_local_ba_optimize(None, C.byref(cam), C.byref(ok), None, None) != 0 and "ba is NULL" in err()
    for fn in (lib.cart_local_ba_clear, lib.cart_local_ba_points, lib.cart_local_ba_track_of):
        assert fn(None, None, None) != 0 if fn is not lib.cart_local_ba_clear else fn(None, None) != 0
        assert "ba is NULL" in err()
    lib.cart_local_ba_destroy(None)                                       # harmless
    lib.cart_local_ba_default_params(None)

"""CPU tests of spec S26, dense ego-motion refinement from flow and disparity: the numpy restatement
tests/np_dense_ego.py against its scalar twin (the two-level lane order included) and against a hand-worked case, the threshold edges,
the stop rules, the accuracy of the spec on S25's synthetic scene, and the library's host-side checks (no GPU: validation comes before
any device call).  tests/test_gpu_dense_ego.py runs the scenes built here on the device."""
import ctypes as C
import math

import numpy as np
import pytest

import np_dense_ego as D
import np_motion as M
import test_motion_spec as S

CAM = S.CAM   # fx = fy = 256, cx = 8, cy = 4, baseline 0.5: fx * baseline = 128


def small_rel(yaw_deg=0.0, pitch_deg=0.0, t=(0.0, 0.0, 0.0)):
    """(R | t) of a small yaw about y, then a small pitch about x."""
    cy_, sy = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    cp, sp = math.cos(math.radians(pitch_deg)), math.sin(math.radians(pitch_deg))
    Ry = np.array([[cy_, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy_]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    return [float(v) for v in np.hstack([Rx @ Ry, np.array(t, np.float64).reshape(3, 1)]).reshape(-1)]


def scene_camera(w, h):
    return M.camera(fx=256.0, fy=256.0, cx=w / 2.0, cy=h / 2.0, baseline=0.5)


def smooth_scene(w, h, rel, seed=0, invalid=0.0):
    """A smooth surface (Z between 4 and 12 m: a slant plus a ripple) in the previous frame, seen again after the motion `rel`: the
    previous disparity, the flow (S10.5, rounded) and this frame's disparity of the point the floored flow reaches, all quantised as the
    pipeline's are.  -> (camera, disp_cur, disp_prev, flow)."""
    cam = scene_camera(w, h)
    fx, fy, cx, cy, fxb = cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["fx"] * cam["baseline"]
    R, t = D.split(rel)
    rng = np.random.default_rng(seed)

    def depth(x, y):
        return 8.0 + 2.5 * (x / max(w, 8) - 0.5) + 1.5 * (y / max(h, 8) - 0.5) + 0.5 * np.sin(x / 9.0) * np.cos(y / 7.0)

    def forward(xp, yp, Z):
        X, Y = (xp - cx) * Z / fx, (yp - cy) * Z / fy
        q = [R[3 * r] * X + R[3 * r + 1] * Y + R[3 * r + 2] * Z + t[r] for r in range(3)]
        return fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy, q[2]

    y, x = (a.astype(np.float64) for a in np.indices((h, w)))
    disp_prev = np.round(16.0 * fxb / depth(x, y)).astype(np.int16)
    xp, yp = x.copy(), y.copy()
    for _ in range(8):                                  # the previous position whose point lands on (x, y)
        u, v, _ = forward(xp, yp, depth(xp, yp))
        xp, yp = xp - (u - x), yp - (v - y)
    flow = np.stack([np.round((x - xp) * 32.0), np.round((y - yp) * 32.0)], -1).astype(np.int16)
    xi, yi = x.astype(np.int64) - (flow[..., 0].astype(np.int64) >> 5), y.astype(np.int64) - (flow[..., 1].astype(np.int64) >> 5)
    inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    xi, yi = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
    _, _, qz = forward(xi.astype(np.float64), yi.astype(np.float64), fxb / (disp_prev[yi, xi] / 16.0))
    disp_cur = np.where(inside, np.round(16.0 * fxb / qz), 16.0 * fxb / depth(x, y)).astype(np.int16)
    if invalid:
        disp_cur[rng.random((h, w)) < invalid] = -32768
        disp_prev[rng.random((h, w)) < invalid] = -32768
    return cam, disp_cur, disp_prev, flow


TRUE_REL = small_rel(0.6, -0.2, (0.03, -0.01, -0.25))
START_REL = small_rel(0.7, -0.15, (0.035, -0.012, -0.24))        # the true pose perturbed: about 0.1 degree and 1 cm


# ---- the restatement against its scalar twin ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,stride", [(7, 5, 1), (23, 9, 2), (300, 3, 1), (40, 7, 3), (9, 260, 1)])
def test_vectorised_restatement_equals_the_scalar_loop(w, h, stride):
    cam, dc, dp, fl = smooth_scene(w, h, TRUE_REL, seed=w, invalid=0.05)
    mask = (np.random.default_rng(h).random((h, w)) < 0.2).astype(np.uint8)
    for k, (rel, mk) in enumerate(((START_REL, None), (TRUE_REL, mask), (small_rel(t=(0.0, 0.0, -9.0)), None))):
        p = D.params(stride=stride, min_inliers=6, disparity_weight=(1.0, 0.5, 2.0)[k])
        R, t = D.split(rel)
        c = D.candidates(cam, p, dc, dp, fl, mk)
        ok, vals = D.terms(cam, p, R, t, c)
        count, ncand, sums = D.scalar_evaluate(cam, p, R, t, dc, dp, fl, mk)
        assert (count, ncand) == (int(ok.sum()), int(c["cand"].sum()))
        assert np.array(sums).tobytes() == D.two_level(vals, ok).tobytes(), k
        if k < 2 and w * h > 100:
            assert 6 < count <= ncand < c["cand"].size     # some pixels contribute, some are no candidates
        if k == 2:
            assert count == 0 and ncand > 0 and all(v == 0.0 for v in sums)      # every point behind the camera


def test_the_order_of_the_sums_matters():
    """Columns 0 and 256 of a row belong to one lane: walked in the other order, the sums differ in the last bits."""
    w, h = 600, 2
    cam, dc, dp, fl = smooth_scene(w, h, TRUE_REL, seed=3)
    p = D.params(min_inliers=6)
    R, t = D.split(START_REL)
    a = D.scalar_evaluate(cam, p, R, t, dc, dp, fl)
    b = D.scalar_evaluate(cam, p, R, t, dc, dp, fl, order=list(reversed(range(w))))
    assert a[:2] == b[:2] and a[0] > 512
    assert np.array(a[2]).tobytes() != np.array(b[2]).tobytes()
    assert np.allclose(a[2], b[2], rtol=1e-12, atol=1e-9)


def test_hand_worked_three_pixels():
    """Three pixels of a plane at d = 16 (Z = 8) under t = (1 / 32, 0, 0), identity rotation, no flow: q = (X + 1 / 32, Y, 8), so
    a = c = 32, b = -4 q.x, d = -4 q.y, g = -2, eu = 32 / 32 = 1, ev = ed = 0.  Every value below is exact in binary."""
    cam = M.camera(fx=256.0, fy=256.0, cx=1.0, cy=0.0, baseline=0.5)
    dc, dp, fl = S.flat(1, 3, 256, 256)
    p = D.params(min_inliers=6, disparity_weight=0.5)
    R, t = D.split(S.rel_t(tx=0.03125))
    ok, vals = D.terms(cam, p, R, t, D.candidates(cam, p, dc, dp, fl))
    assert ok.all()
    H = np.zeros((6, 6))
    g = np.zeros(6)
    e2 = 0.0
    for x in range(3):
        qx, qy, qz = (x - 1.0) / 32.0 + 0.03125, 0.0, 8.0
        a, b, c, d, gg = 32.0, -4.0 * qx, 32.0, -4.0 * qy, -2.0
        Ju = np.array([b * qy, a * qz - b * qx, -(a * qy), a, 0.0, b])
        Jv = np.array([d * qy - c * qz, -(d * qx), c * qx, 0.0, c, d])
        Jd = np.array([gg * qy, -(gg * qx), 0.0, 0.0, 0.0, gg])
        assert Jd.tolist() == [0.0, 2.0 * qx, 0.0, 0.0, 0.0, -2.0]
        H += np.outer(Ju, Ju) + np.outer(Jv, Jv) + 0.5 * np.outer(Jd, Jd)
        g += Ju * 1.0 + Jv * 0.0 + 0.5 * Jd * 0.0
        e2 += 1.0
    n, Hm, gm, e2m = D.evaluate(cam, p, R, t, D.candidates(cam, p, dc, dp, fl))
    assert n == 3 and e2m == e2 == 3.0
    assert gm == g.tolist()
    assert [[Hm[i][j] for j in range(i, 6)] for i in range(6)] == [[H[i][j] for j in range(i, 6)] for i in range(6)]
    assert Hm[3][3] == 3 * 32.0 * 32.0 and Hm[5][5] == sum((4.0 * ((x - 1.0) / 32.0 + 0.03125)) ** 2 for x in range(3)) + 0.5 * 3 * 4.0
    count, ncand, sums = D.scalar_evaluate(cam, p, R, t, dc, dp, fl)
    assert (count, ncand) == (3, 3) and sums[27] == 3.0 and sums[21:27] == gm


def contributing(cam, p, rel, dc, dp, fl, mask=None):
    R, t = D.split(rel)
    return int(D.terms(cam, p, R, t, D.candidates(cam, p, dc, dp, fl, mask))[0].sum())


def test_threshold_edges_are_strict():
    """S25's exact cases: a residual that equals a threshold does not contribute (<, not <=); S25 calls the same pixel STATIC (not >)."""
    n = 16 * 8
    p = D.params(min_inliers=6)
    assert contributing(S.CAM150, p, M.REL_IDENTITY, *S.flat(8, 16, 184, 200)) == 0            # ed = 1.0
    assert contributing(S.CAM150, p, M.REL_IDENTITY, *S.flat(8, 16, 185, 200)) == n            # ed = 0.9375
    assert contributing(S.CAM150, D.params(disparity_threshold=1.0625), M.REL_IDENTITY, *S.flat(8, 16, 184, 200)) == n
    assert contributing(CAM, p, S.rel_t(tx=0.0625), *S.flat(8, 16, 256, 256)) == 0              # eu = 2.0
    assert contributing(CAM, p, S.rel_t(tx=0.0625 - 2.0 ** -10), *S.flat(8, 16, 256, 256)) == n
    assert contributing(CAM, D.params(flow_threshold=2.03125), S.rel_t(tx=0.0625), *S.flat(8, 16, 256, 256)) == n
    assert contributing(CAM, p, S.rel_t(tz=-8.0), *S.flat(8, 16, 256, 256)) == 0                # q.z = 0 is not > 0
    assert contributing(CAM, p, M.REL_IDENTITY, *S.flat(8, 16, 16, 16)) == n                    # d = min_disparity passes
    assert contributing(CAM, p, M.REL_IDENTITY, *S.flat(8, 16, 15, 16)) == 0 and contributing(CAM, p, M.REL_IDENTITY, *S.flat(8, 16, 16, 15)) == 0
    mask = np.zeros((8, 16), np.uint8)
    mask[2, 3], mask[4, 5], mask[6, 7] = 1, 2, 0                                                # only MOVING leaves
    assert contributing(CAM, p, M.REL_IDENTITY, *S.flat(8, 16, 256, 256), mask) == n - 1
    c = D.candidates(CAM, D.params(stride=3), *S.flat(8, 16, 256, 256))
    assert c["cand"].shape == (3, 6) and c["x"][0].tolist() == [0.0, 3.0, 6.0, 9.0, 12.0, 15.0] and c["y"][:, 0].tolist() == [0.0, 3.0, 6.0]


def test_stops():
    cam, dc, dp, fl = smooth_scene(64, 40, TRUE_REL, seed=1)
    full = D.refine(cam, D.params(min_inliers=6), START_REL, dc, dp, fl)
    assert full["status"][0] == 1 and full["steps"][0] == 4 and full["n_inliers"][0] >= full["n_initial"][0] > 1000
    # min_inliers above what the frame holds: no step, the pose is rel0, the counts and errors are those at rel0
    few = D.refine(cam, D.params(min_inliers=64 * 40 + 1), START_REL, dc, dp, fl)
    assert few["status"][0] == 0 and few["steps"][0] == 0 and D.join(few["R"][0].tolist(), few["t"][0].tolist()) == START_REL
    assert few["n_inliers"][0] == few["n_initial"][0] == full["n_initial"][0] and few["rms"][0] == few["rms_initial"][0] == full["rms_initial"][0]
    assert D.accept(few, START_REL) == START_REL and D.accept(full, START_REL) == D.join(full["R"][0].tolist(), full["t"][0].tolist())
    # iterations = 0
    none = D.refine(cam, D.params(min_inliers=6, iterations=0), START_REL, dc, dp, fl)
    assert none.tobytes() == few.tobytes()
    one = D.refine(cam, D.params(min_inliers=6, iterations=1), START_REL, dc, dp, fl)
    assert one["steps"][0] == 1 and one["status"][0] == 1 and one["rms"][0] < one["rms_initial"][0]


def test_pivot_stop_on_a_degenerate_plane():
    """One image row through the principal point (Y = 0) of a fronto-parallel plane, 16 pixels placed symmetrically about cx: column 0
    of the Jacobian is -Z times column 4 (and Jd is zero in both), every product is exact in binary, and the pivot of column 4 is
    exactly 0.0 -- the solve stops there instead of dividing by it, at disparity_weight 0 and at 1 alike."""
    cam = M.camera(fx=256.0, fy=256.0, cx=7.5, cy=0.0, baseline=0.5)
    dc, dp, fl = S.flat(1, 16, 256, 256)
    for wd in (0.0, 1.0):
        p = D.params(min_inliers=6, disparity_weight=wd)
        n, H, g, _ = D.evaluate(cam, p, *D.split(M.REL_IDENTITY), D.candidates(cam, p, dc, dp, fl))
        assert n == 16 and D.solve6(H, g) is None
        r = D.refine(cam, p, S.rel_t(tx=0.0078125), dc, dp, fl)
        assert r["status"][0] == 0 and r["steps"][0] == 0 and r["n_inliers"][0] == 16 and r["rms"][0] == 0.25
        assert np.isfinite(r["R"][0]).all() and np.isfinite(r["t"][0]).all()
    # a whole fronto-parallel plane at disparity_weight 0 is well-posed (the reprojection alone fixes the pose): no NaN either way
    r = D.refine(CAM, D.params(min_inliers=6, disparity_weight=0.0), S.rel_t(tx=0.01), *S.flat(8, 16, 256, 256))
    assert all(np.isfinite(r[k][0]).all() for k in ("R", "t", "rms", "rms_initial"))


def test_accept_rule():
    r = np.zeros(1, D.RESULT_DTYPE)
    r["R"][0], r["t"][0] = D.split(TRUE_REL)
    r["status"], r["n_initial"], r["n_inliers"] = 1, 100, 100
    assert D.accept(r, START_REL) == TRUE_REL
    for key, bad in (("status", 0), ("n_inliers", 99)):
        q = r.copy()
        q[key] = bad
        assert D.accept(q, START_REL) == START_REL
    q = r.copy()
    q["t"][0][1] = np.nan
    assert D.accept(q, START_REL) == START_REL


# ---- accuracy of the spec -----------------------------------------------------------------------------------------------------
def pose_errors(R, t, true_rel):
    """-> (rotation error in degrees, translation error in metres) of (R, t) against the 3 x 4 true_rel."""
    Rt, tt = D.split(true_rel)
    E = np.array(R, np.float64).reshape(3, 3) @ np.array(Rt).reshape(3, 3).T
    return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(E) - 1.0) / 2.0)))), float(np.linalg.norm(np.array(t, np.float64) - np.array(tt)))


ACCURACY_START = S.yaw_rel(0.15, (0.125 + 0.02, 0.0, 0.03))     # the true pose (t_x = 1 / 8) turned by 0.15 degrees and moved by 3.6 cm


def run_accuracy():
    (cam, mp, true_rel, dc, dp, fl), _, _ = S.accuracy_scene()
    labels = M.segment(cam, mp, ACCURACY_START, dc, dp, fl)["labels"]      # the labels a pipeline has at this point: those at rel0
    plain = D.refine(cam, D.params(), ACCURACY_START, dc, dp, fl)
    masked = D.refine(cam, D.params(), ACCURACY_START, dc, dp, fl, labels)
    R0, t0 = D.split(ACCURACY_START)
    return pose_errors(R0, t0, true_rel), plain, pose_errors(plain["R"][0], plain["t"][0], true_rel), masked, pose_errors(masked["R"][0], masked["t"][0], true_rel)


def test_accuracy_on_the_motion_scene():
    """S25's scene (a fronto-parallel background at Z = 8 m, one pixel = 3.1 cm there, a rectangle that moves on its own, quarter-pixel
    disparity noise, 5 % invalid pixels), rel0 = the true pose turned by 0.15 degrees of yaw and moved by (2, 0, 3) cm.  Measured on the
    restatement at the defaults: see MEASURED below and DESIGN.md 7.8.  The bounds are twice the measured errors (the convention of 7.5)."""
    e0, plain, ep, masked, em = run_accuracy()
    print(f"rel0: {e0[0]:.4f} deg {100 * e0[1]:.3f} cm; refined: {ep[0]:.4f} deg {100 * ep[1]:.3f} cm; with the mask: {em[0]:.4f} deg {100 * em[1]:.3f} cm")
    for r in (plain, masked):
        assert r["status"][0] == 1 and r["steps"][0] == 4 and D.accept(r, ACCURACY_START) != ACCURACY_START
    assert ep[0] <= 2 * MEASURED["plain"][0] and ep[1] <= 2 * MEASURED["plain"][1]
    assert em[0] <= 2 * MEASURED["masked"][0] and em[1] <= 2 * MEASURED["masked"][1]
    assert em[0] <= ep[0] and em[1] <= ep[1]
    assert ep[0] < e0[0] and ep[1] < e0[1] and em[0] < e0[0] and em[1] < e0[1]


# (degrees, metres) on the restatement: rel0 0.1500 deg / 3.606 cm; refined 0.0442 deg / 0.679 cm without a mask and the same with it (the
# mask removes 1659 candidates, the rectangle and its occlusion strip, none of which contributed: the 2-pixel gate had left them out already)
MEASURED = dict(rel0=(0.15, 0.03606), plain=(0.04420, 0.006795), masked=(0.04420, 0.006795))


def slow_object_scene(seed=26, w=160, h=96):
    """The background of S25's scene (d = 16, a 4-pixel flow under t_x = 1 / 8, quarter-pixel disparity noise, 5 % invalid pixels) and a
    60 x 60 rectangle at the same depth whose flow is 3 pixels: it moved by one pixel on its own, inside the 2-pixel gate."""
    rng = np.random.default_rng(seed)
    y, x = np.indices((h, w))
    rect = (x >= 50) & (x < 110) & (y >= 20) & (y < 80)
    dc = np.full((h, w), 256) + rng.integers(-4, 5, (h, w))
    dp = np.full((h, w), 256) + rng.integers(-4, 5, (h, w))
    dc[rng.random((h, w)) < 0.05] = -32768
    dp[rng.random((h, w)) < 0.05] = -32768
    fl = np.zeros((h, w, 2), np.int16)
    fl[..., 0] = np.where(rect, 3 * 32, 4 * 32)
    return CAM, S.rel_t(tx=0.125), dc.astype(np.int16), dp.astype(np.int16), fl, rect


SLOW_START = S.yaw_rel(0.05, (0.125 + 0.005, 0.0, 0.01))          # 0.05 degrees and 1.1 cm off
SLOW_MEASURED = dict(plain=(0.6326, 0.10307), masked=(0.05321, 0.008252))   # (degrees, metres) on the restatement


def test_the_mask_matters_for_an_object_inside_the_gate():
    """An object that moves by less than flow_threshold passes the gate and votes.  Measured on the restatement: without a mask the
    refinement follows it to 0.633 degrees / 10.3 cm (from rel0's 0.050 degrees / 1.12 cm: worse than no refinement); with the labels of a
    motion segmentation at flow_threshold 0.75 as the mask (90 % of the rectangle MOVING, 0.01 % of the background) it ends at 0.053
    degrees / 0.83 cm.  Bounds at twice the measured errors of the masked run; the unmasked one must be the worse of the two."""
    cam, true, dc, dp, fl, rect = slow_object_scene()
    labels = M.segment(cam, M.params(flow_threshold=0.75), SLOW_START, dc, dp, fl)["labels"]
    assert (labels[rect] == M.MOVING).mean() > 0.8 and (labels[~rect] == M.MOVING).mean() < 0.01
    plain = D.refine(cam, D.params(), SLOW_START, dc, dp, fl)
    masked = D.refine(cam, D.params(), SLOW_START, dc, dp, fl, labels)
    ep, em = pose_errors(plain["R"][0], plain["t"][0], true), pose_errors(masked["R"][0], masked["t"][0], true)
    print(f"refined: {ep[0]:.4f} deg {100 * ep[1]:.3f} cm; with the mask: {em[0]:.4f} deg {100 * em[1]:.3f} cm")
    assert plain["steps"][0] == masked["steps"][0] == 4 and masked["n_candidates"][0] < plain["n_candidates"][0]
    assert em[0] <= 2 * SLOW_MEASURED["masked"][0] and em[1] <= 2 * SLOW_MEASURED["masked"][1]
    assert em[0] < ep[0] / 4 and em[1] < ep[1] / 4          # measured: a twelfth of both
    assert em[1] < pose_errors(*D.split(SLOW_START), true)[1]


# ---- the library's host side --------------------------------------------------------------------------------------------------
def lib_error(cam=CAM, rel=M.REL_IDENTITY, p=None, w=16, h=8, params_null=False):
    from cartslam import _lib, dense_ego_params
    lib = _lib.load()
    c = _lib.EgoCamera(*[cam[k] for k in ("fx", "fy", "cx", "cy", "baseline")]) if cam is not None else None
    dp = dense_ego_params(**(p or {}))
    r = (C.c_double * 12)(*rel) if rel is not None else None
    rc = lib.cart_dense_ego_refine(None, C.byref(c) if c is not None else None, r, None if params_null else C.byref(dp), None, 0, None, 0, None, 0, None, 0,
                                   w, h, None, None)
    assert rc != 0
    return lib.cart_last_error(None).decode()


def test_defaults_and_layout():
    from cartslam import DENSE_EGO_RESULT_DTYPE, DenseEgoParams, DenseEgoResult, _lib, dense_ego_params
    assert C.sizeof(DenseEgoParams) == 4 * 8 + 4 * 4 and DenseEgoParams.iterations.offset == 32 and DenseEgoParams.min_inliers.offset == 40
    assert C.sizeof(DenseEgoResult) == 14 * 8 + 6 * 4 == DENSE_EGO_RESULT_DTYPE.itemsize == D.RESULT_DTYPE.itemsize == 136
    assert DENSE_EGO_RESULT_DTYPE == D.RESULT_DTYPE
    assert [(n, DENSE_EGO_RESULT_DTYPE.fields[n][1]) for n in DENSE_EGO_RESULT_DTYPE.names] == [(n, getattr(DenseEgoResult, n).offset) for n, _ in DenseEgoResult._fields_]
    p = dense_ego_params()
    assert {k: getattr(p, k) for k in D.DEFAULTS} == D.DEFAULTS
    assert (p.min_disparity, p.flow_threshold, p.disparity_threshold, p.disparity_weight, p.iterations, p.stride, p.min_inliers) == (1.0, 2.0, 1.0, 1.0, 4, 1, 1024)
    assert dense_ego_params(stride=3).stride == 3
    with pytest.raises(ValueError):
        dense_ego_params(radius=3)
    _lib.load().cart_dense_ego_default_params(None)   # a NULL pointer is ignored


def test_argument_checks_without_an_object():
    from cartslam import _lib
    assert lib_error() == "bad arguments"                                       # a valid configuration gets as far as the missing object
    assert lib_error(p=dict(iterations=16, stride=16, min_inliers=1 << 30, disparity_weight=0.0), w=16384, h=1) == "bad arguments"
    assert lib_error(p=dict(iterations=0, min_inliers=6)) == "bad arguments"
    assert "params" in lib_error(params_null=True)
    for key, bad in (("min_disparity", 0.0), ("min_disparity", float("nan")), ("flow_threshold", -1.0), ("flow_threshold", float("inf")),
                     ("disparity_threshold", 0.0), ("disparity_threshold", float("inf")), ("disparity_weight", -0.5), ("disparity_weight", float("nan")),
                     ("disparity_weight", float("inf")), ("iterations", -1), ("iterations", 17), ("stride", 0), ("stride", 17), ("min_inliers", 5),
                     ("min_inliers", (1 << 30) + 1)):
        assert key in lib_error(p={key: bad}), (key, bad)
    assert "camera" in lib_error(cam=None)
    for key in ("fx", "fy", "baseline"):
        assert key in lib_error(cam=dict(CAM, **{key: 0.0}))
    assert "cx" in lib_error(cam=dict(CAM, cx=float("inf")))
    assert "rel0" in lib_error(rel=None)
    for k, bad in ((0, 2.5), (5, float("nan")), (3, 2e6), (11, -float("inf"))):
        r = list(M.REL_IDENTITY)
        r[k] = bad
        assert f"rel0[{k}]" in lib_error(rel=r)
    assert lib_error(rel=S.rel_t(tx=-1e6, tz=1e6)) == "bad arguments"
    for kw, word in ((dict(w=0), "width"), (dict(w=16385), "width"), (dict(h=0), "height"), (dict(h=20000), "height")):
        assert word in lib_error(**kw)
    # the order: params before camera before rel0 before sizes
    assert "stride" in lib_error(p=dict(stride=99), cam=None, rel=None, w=0)
    assert "camera" in lib_error(cam=None, rel=None, w=0)
    assert "rel0" in lib_error(rel=None, w=0)
    lib = _lib.load()
    out = C.c_void_p()
    for args, word in (((None, 0, 8), "max_width"), ((None, 16385, 8), "max_width"), ((None, 8, 0), "max_height"), ((None, 8, 16385), "max_height"), ((None, 8, 8), "bad arguments")):
        assert lib.cart_dense_ego_create(*args, C.byref(out)) != 0 and word in lib.cart_last_error(None).decode()
    lib.cart_dense_ego_destroy(None)   # a NULL object is ignored

"""CPU tests of spec S25, motion segmentation from flow, disparity and ego-motion: the numpy restatement
tests/np_motion.py against its scalar twin and against hand-worked cases, the filter's counts, Q(), the accuracy of the spec on a
synthetic scene, and the library's host-side checks (no GPU: validation comes before any device call).  tests/test_gpu_motion.py
runs the cases built here on the device."""
import ctypes as C

import numpy as np
import pytest

import np_motion as M

# fx * baseline = 128 and disparities that are powers of two keep every intermediate of the hand-worked cases exact
CAM = M.camera(fx=256.0, fy=256.0, cx=8.0, cy=4.0, baseline=0.5)
# the issue's example: fx * baseline = 150, s_p = 200 -> d_p = 12.5, Zp = 12, predicted d = 12.5
CAM150 = M.camera(fx=300.0, fy=300.0, cx=80.0, cy=8.0, baseline=0.5)


def rel_t(tx=0.0, ty=0.0, tz=0.0):
    r = list(M.REL_IDENTITY)
    r[3], r[7], r[11] = tx, ty, tz
    return r


def yaw_rel(deg, t=(0.0, 0.0, 0.0)):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return [c, 0.0, s, t[0], 0.0, 1.0, 0.0, t[1], -s, 0.0, c, t[2]]


def flat(h, w, s_cur, s_prev, flow=(0, 0)):
    fl = np.zeros((h, w, 2), np.int16)
    fl[..., 0], fl[..., 1] = flow
    return np.full((h, w), s_cur, np.int16), np.full((h, w), s_prev, np.int16), fl


def threshold_cases():
    """(name, camera, params, rel, disp_cur, disp_prev, flow, expected raw label of every pixel, expected record or None) on 16 x 8
    frames: each threshold of the spec met exactly and missed by one step."""
    p = M.params(radius=0)
    out = []
    # disparity threshold: ed = 12.5 - s_c / 16
    out.append(("ed = 1.0 is not > 1.0", CAM150, p, M.REL_IDENTITY, *flat(8, 16, 184, 200), M.STATIC, None))
    out.append(("ed = 1.0625", CAM150, p, M.REL_IDENTITY, *flat(8, 16, 183, 200), M.MOVING, None))
    out.append(("ed = -1.0", CAM150, p, M.REL_IDENTITY, *flat(8, 16, 216, 200), M.STATIC, None))
    out.append(("ed = -1.0625", CAM150, p, M.REL_IDENTITY, *flat(8, 16, 217, 200), M.MOVING, None))
    # flow threshold: s = 256 -> d = 16, Z = 8; t_x = 1 / 16 shifts the image by 256 / 16 / 8 = 2 pixels, all exact
    out.append(("eu = 2.0 is not > 2.0", CAM, p, rel_t(tx=0.0625), *flat(8, 16, 256, 256), M.STATIC, (32, 0, 0, 0)))
    out.append(("eu = 3.0", CAM, p, rel_t(tx=0.09375), *flat(8, 16, 256, 256), M.MOVING, (48, 0, 0, 1)))
    out.append(("ev = -2.0", CAM, p, rel_t(ty=-0.0625), *flat(8, 16, 256, 256), M.STATIC, (0, -32, 0, 0)))
    out.append(("eu^2 + ev^2 = 5", CAM, p, rel_t(tx=0.0625, ty=0.03125), *flat(8, 16, 256, 256), M.MOVING, (32, 16, 0, 1)))
    out.append(("eu = 2.03125 with a lower threshold just above", CAM, M.params(radius=0, flow_threshold=2.03125), rel_t(tx=0.0625 + 2.0 ** -10),
                *flat(8, 16, 256, 256), M.STATIC, (33, 0, 0, 0)))   # Q(2.03125) = floor(32.5 + 0.5) = 33: the .5 rounds up
    # min_disparity, in either image (gate 1 and gate 3): d = 1.0 passes, 15 / 16 does not
    out.append(("d_c = min_disparity", CAM, p, M.REL_IDENTITY, *flat(8, 16, 16, 16), M.STATIC, (0, 0, 0, 0)))
    out.append(("d_c one step under", CAM, p, M.REL_IDENTITY, *flat(8, 16, 15, 16), M.UNKNOWN, (-32768, -32768, -32768, 2)))
    out.append(("d_p one step under", CAM, p, M.REL_IDENTITY, *flat(8, 16, 16, 15), M.UNKNOWN, (-32768, -32768, -32768, 2)))
    out.append(("d_c = 2.5 = min_disparity", CAM, M.params(radius=0, min_disparity=2.5), M.REL_IDENTITY, *flat(8, 16, 40, 40), M.STATIC, (0, 0, 0, 0)))
    out.append(("d_p under 2.5", CAM, M.params(radius=0, min_disparity=2.5), M.REL_IDENTITY, *flat(8, 16, 40, 39), M.UNKNOWN, None))
    return out


@pytest.mark.parametrize("case", threshold_cases(), ids=lambda c: c[0])
def test_hand_worked_thresholds(case):
    _, cam, p, rel, dc, dp, fl, label, record = case
    for got in (M.segment(cam, p, rel, dc, dp, fl), M.scalar_segment(cam, p, rel, dc, dp, fl)):
        assert (got["raw"] == label).all() and (got["labels"] == label).all()
        if record is not None:
            assert (got["residual"] == np.array(record, np.int16)).all(), got["residual"][0, 0]


def test_flow_sign_and_arithmetic_shift():
    """A point that moved 2 pixels right has flow +64: the previous position is x - 2, and the 2-pixel shift of t_x = 1 / 16 is explained.
    -1 >> 5 is -1: a flow of -1 / 32 pixel reads the pixel to the right / below."""
    dc, dp, fl = flat(8, 16, 256, 256, flow=(64, 0))
    got = M.segment(CAM, M.params(radius=0), rel_t(tx=0.0625), dc, dp, fl)
    assert (got["raw"][:, 2:] == M.STATIC).all() and (got["residual"][:, 2:, :3] == 0).all()
    assert (got["raw"][:, :2] == M.UNKNOWN).all() and (got["gate"][:, :2] == 2).all()       # the previous position left the image
    dc, dp, fl = flat(8, 16, 256, 256, flow=(-1, -1))
    dp[3, 5] = -32768
    got = M.segment(CAM, M.params(radius=0), M.REL_IDENTITY, dc, dp, fl)
    assert got["gate"][2, 4] == 3 and (got["gate"] == 3).sum() == 1                          # pixel (4, 2) read (5, 3)
    assert (got["gate"][:, 15] == 2).all() and (got["gate"][7, :] == 2).all()
    assert (got["residual"][0, 0] == (16, 16, 0, 0)).all()                                   # eu = ev = 1 pixel


def test_points_behind_the_camera_are_unknown():
    dc, dp, fl = flat(8, 16, 256, 256)
    got = M.segment(CAM, M.params(radius=0), rel_t(tz=-8.0), dc, dp, fl)                     # q.z = 8 - 8 = 0 is not > 0
    assert (got["gate"] == 4).all() and (got["raw"] == M.UNKNOWN).all()
    got = M.segment(CAM, M.params(radius=0), rel_t(tz=-7.0), dc, dp, fl)                     # q.z = 1: d = 128, far off
    assert (got["raw"] == M.MOVING).all() and (got["residual"][..., 2] == (128 - 16) * 16).all()


def random_frame(seed, w, h, big_flow=False):
    """Frames with every label and every gate: a plane at d = 16 with disparity steps around the threshold, invalid and sub-minimum
    pixels in both images, flows of both signs with fractional parts (large ones leave the image or gather from anywhere)."""
    rng = np.random.default_rng(seed)
    dp = (256 + rng.integers(-3, 4, (h, w))).astype(np.int16)
    dc = (256 + rng.integers(-24, 25, (h, w))).astype(np.int16)
    for d in (dc, dp):
        d[rng.random((h, w)) < 0.08] = -32768
        sub = rng.random((h, w)) < 0.08
        d[sub] = rng.integers(-40, 16, (h, w))[sub]
    reach = np.array([w, h] if big_flow else [3, 3])                                          # per component: up to the whole image
    fl = (rng.integers(-reach, reach + 1, (h, w, 2)) * 32 + rng.integers(0, 32, (h, w, 2))).astype(np.int16)
    fl[rng.random((h, w)) < 0.5] = rng.integers(-32, 32, 2)                                   # half of the pixels barely move
    return dc, dp, fl, rng.integers(0, 3, (h, w)).astype(np.uint8)


def premises(ref, gates=(1, 2, 3)):
    """A comparison against `ref` says something only if every label and every listed gate occurs in it."""
    for v in (M.STATIC, M.MOVING, M.UNKNOWN):
        assert (ref["raw"] == v).sum() > 0, f"no raw label {v}"
    for g in gates:
        assert (ref["gate"] == g).sum() > 0, f"no pixel stopped by gate {g}"


@pytest.mark.parametrize("w,h,radius", [(5, 3, 4), (23, 9, 0), (23, 9, 1), (40, 17, 2), (33, 21, 4)])
def test_vectorised_restatement_equals_the_scalar_loop(w, h, radius):
    for k, rel in enumerate((M.REL_IDENTITY, yaw_rel(2.0, (-0.05, 0.01, -0.2)), rel_t(tz=-9.0))):
        dc, dp, fl, planes = random_frame(100 * w + k, w, h, big_flow=k == 1)
        p = M.params(radius=radius, support_percent=(50, 30, 80)[k])
        a, b = M.segment(CAM, p, rel, dc, dp, fl, planes), M.scalar_segment(CAM, p, rel, dc, dp, fl, planes)
        for key in ("residual", "raw", "labels", "planes_static"):
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (key, k)
        if k == 0 and w > 5:
            premises(a)
        if k == 2:
            assert (a["gate"] == 4).sum() > 0 and set(np.unique(a["gate"])) == {1, 2, 3, 4}
        assert ((a["planes_static"] == 2) >= (a["labels"] == 1)).all() and (a["planes_static"][a["labels"] != 1] == planes[a["labels"] != 1]).all()


def test_filter_counts_at_corners_edges_and_the_ratio():
    raw = np.ones((5, 7), np.uint8)
    _, nm, ns = M.majority(raw, 1, 50)
    assert nm[0, 0] == 4 and nm[0, 3] == 6 and nm[2, 0] == 6 and nm[2, 3] == 9 and nm[4, 6] == 4 and (ns == 0).all()    # clipped, not replicated
    _, nm, _ = M.majority(raw, 4, 50)
    assert (nm[:, 3] == 35).all() and nm[0, 0] == 5 * 5 and nm[4, 6] == 5 * 5                  # a window larger than the image
    raw = np.array([[1, 0], [0, 0]], np.uint8)                                                 # n_m = 1, n_s = 3 everywhere: 25 %
    assert (M.majority(raw, 1, 25)[0] == 1).all() and (M.majority(raw, 1, 26)[0] == 0).all()
    raw = np.array([[1, 2, 0], [2, 0, 2], [0, 2, 1]], np.uint8)                                # UNKNOWN stays, and does not count
    out, nm, ns = M.majority(raw, 1, 40)
    assert nm[1, 1] == 2 and ns[1, 1] == 3 and out[1, 1] == 1 and (out[raw == 2] == 2).all()   # 2 of 5 known = 40 %
    assert M.majority(raw, 1, 41)[0][1, 1] == 0
    assert out[0, 0] == 1 and nm[0, 0] == 1 and ns[0, 0] == 1                                  # corner: itself and the centre
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 3, (9, 11)).astype(np.uint8)
    assert (M.majority(raw, 0, 50)[0] == raw).all() and (M.majority(raw, 0, 1)[0] == raw).all() and (M.majority(raw, 0, 100)[0] == raw).all()
    y, x = np.indices((8, 12))
    out = M.majority(((x + y) % 2).astype(np.uint8), 1, 50)[0]                                 # checkerboard: the centre colour has 5 of 9
    assert (out[1:-1, 1:-1] == ((x + y) % 2)[1:-1, 1:-1]).all()
    assert (M.majority((x % 2).astype(np.uint8), 1, 50)[0][:, 1:-1] == 1 - (x % 2)[:, 1:-1]).all()   # stripes: the other colour has 6 of 9


def test_quantiser():
    e = np.array([0.0, 0.03125, 0.03124, -0.03125, -0.03126, 0.09375, 2047.9375, 2047.97, 5000.0, -2047.9375, -2048.0, -5000.0, np.inf, -np.inf, 1.0, np.nan])
    assert M.quantise(e).tolist() == [0, 1, 0, 0, -1, 2, 32767, 32767, 32767, -32767, -32767, -32767, 32767, -32767, 16, -32767]   # Q(NaN) = -32767
    assert [M._q(float(v)) for v in e] == M.quantise(e).tolist()


# ---- accuracy of the spec ---------------------------------------------------------------------------------------------------
def accuracy_scene(seed=25, w=160, h=96):
    """A fronto-parallel background at d = 16 (Z = 8) seen by a camera that moved t_x = 1 / 8 (a 4-pixel flow), and a rectangle that came
    nearer (d = 28 -> 32) and moved 2 pixels the other way: against the 8 pixels the ego-motion predicts at its depth that is 10
    pixels of flow (5 x the threshold), and 4 of disparity (4 x the threshold).  Quarter-pixel disparity noise, 5 % invalid pixels in
    each image.  -> (inputs, interior mask of the rectangle, background mask)."""
    rng = np.random.default_rng(seed)
    y, x = np.indices((h, w))
    rect = (x >= 60) & (x < 100) & (y >= 30) & (y < 70)
    rect_prev = (x >= 62) & (x < 102) & (y >= 30) & (y < 70)
    dc = np.where(rect, 32 * 16, 16 * 16) + rng.integers(-4, 5, (h, w))
    dp = np.where(rect_prev, 28 * 16, 16 * 16) + rng.integers(-4, 5, (h, w))
    dc[rng.random((h, w)) < 0.05] = -32768
    dp[rng.random((h, w)) < 0.05] = -32768
    fl = np.zeros((h, w, 2), np.int16)
    fl[..., 0] = np.where(rect, -2 * 32, 4 * 32)
    interior = (x >= 62) & (x < 98) & (y >= 32) & (y < 68)
    return (CAM, M.params(), rel_t(tx=0.125), dc.astype(np.int16), dp.astype(np.int16), fl), interior, ~rect


def test_accuracy_on_a_synthetic_scene():
    """Measured on the restatement at the defaults (radius 2, 50 %): 90.97 % of the rectangle's interior MOVING (1179 of 1296 pixels; the
    other 9.03 % are UNKNOWN, what two 5 % invalidations leave, and none is STATIC) and 1.51 % of the background MOVING (208 of 13760
    pixels, all in the strip x = 100..105 right of the rectangle whose previous position lies on the rectangle of frame t-1: an
    occlusion, not noise).  Each bound sits at twice the measured distance to the ideal (100 % inside, 0 % outside), so that the
    measured value lies half-way between the bound and the ideal: 100 - 2 x 9.03 = 81.94 % and 2 x 1.51 = 3.02 %."""
    args, interior, background = accuracy_scene()
    got = M.segment(*args)
    inside = float((got["labels"][interior] == M.MOVING).mean())
    outside = float((got["labels"][background] == M.MOVING).mean())
    print(f"moving inside {100 * inside:.2f} %, moving outside {100 * outside:.2f} %")
    assert (got["labels"][interior] != M.STATIC).all()
    assert inside >= INSIDE_BOUND, inside
    assert outside <= OUTSIDE_BOUND, outside


INSIDE_BOUND, OUTSIDE_BOUND = 0.8194, 0.0302   # test_accuracy_on_a_synthetic_scene's docstring derives them


# ---- the library's host side ------------------------------------------------------------------------------------------------
def lib_error(cam=CAM, rel=M.REL_IDENTITY, p=None, w=16, h=8, params_null=False):
    from cartslam import _lib
    lib = _lib.load()
    c = _lib.EgoCamera(*[cam[k] for k in ("fx", "fy", "cx", "cy", "baseline")]) if cam is not None else None
    mp = _lib.MotionParams()
    lib.cart_motion_default_params(C.byref(mp))
    for k, v in (p or {}).items():
        setattr(mp, k, v)
    r = (C.c_double * 12)(*rel) if rel is not None else None
    rc = lib.cart_motion_segment(None, C.byref(c) if c is not None else None, r, None if params_null else C.byref(mp), None, 0, None, 0, None, 0, w, h,
                                 None, 0, None, 0, None, 0, None, 0, None, 0, None)
    assert rc != 0
    return lib.cart_last_error(None).decode()


def test_defaults_and_layout():
    from cartslam import MotionParams, _lib, motion_params
    assert C.sizeof(MotionParams) == 3 * 8 + 2 * 4 and MotionParams.radius.offset == 24 and MotionParams.support_percent.offset == 28
    p = motion_params()
    assert (p.min_disparity, p.flow_threshold, p.disparity_threshold, p.radius, p.support_percent) == (1.0, 2.0, 1.0, 2, 50)
    assert {k: getattr(p, k) for k in M.DEFAULTS} == M.DEFAULTS
    assert motion_params(radius=4).radius == 4
    with pytest.raises(ValueError):
        motion_params(window=3)
    _lib.load().cart_motion_default_params(None)   # a NULL pointer is ignored


def test_argument_checks_without_an_engine():
    assert lib_error() == "bad arguments"                                       # a valid configuration gets as far as the missing engine
    assert lib_error(p=dict(radius=4, support_percent=100), w=16384, h=1) == "bad arguments"
    assert "params" in lib_error(params_null=True)
    for key, bad in (("min_disparity", 0.0), ("min_disparity", float("nan")), ("flow_threshold", -1.0), ("flow_threshold", float("inf")),
                     ("disparity_threshold", 0.0), ("radius", -1), ("radius", 5), ("support_percent", 0), ("support_percent", 101)):
        assert key in lib_error(p={key: bad}), (key, bad)
    assert "camera" in lib_error(cam=None)
    for key in ("fx", "fy", "baseline"):
        assert key in lib_error(cam=dict(CAM, **{key: 0.0}))
    assert "cx" in lib_error(cam=dict(CAM, cx=float("inf")))
    assert "rel" in lib_error(rel=None)
    for k, bad in ((0, 2.5), (5, float("nan")), (3, 2e6), (11, -float("inf"))):
        r = list(M.REL_IDENTITY)
        r[k] = bad
        assert f"rel[{k}]" in lib_error(rel=r)
    assert lib_error(rel=rel_t(tx=-1e6, tz=1e6)) == "bad arguments"
    for kw, word in ((dict(w=0), "width"), (dict(w=16385), "width"), (dict(h=0), "height"), (dict(h=20000), "height")):
        assert word in lib_error(**kw)
    # the order: params before camera before rel before sizes
    assert "radius" in lib_error(p=dict(radius=9), cam=None, rel=None, w=0)
    assert "camera" in lib_error(cam=None, rel=None, w=0)
    assert "rel" in lib_error(rel=None, w=0)

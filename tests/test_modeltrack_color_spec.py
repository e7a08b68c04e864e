"""CPU tests of spec S38, colour-aided frame-to-model tracking: the numpy restatement tests/np_modeltrack_color.py against
its scalar twin (a pure-Python loop over pixels), the hand-worked sample, the analytic luminance gradient against central differences, the
reductions to S34 (photo_weight = 0, an empty colour volume), a colour window that lags the map's, the cost rule, the accuracy of the spec
on the synthetic corridor with noisy images (tests/modeltrack_color_scenes.py), and the library's host-side checks (no GPU: validation
comes before any device call).  tests/test_gpu_modeltrack_color.py runs the cases built here on the device."""
import ctypes as C
import math

import numpy as np
import pytest

import modeltrack_color_scenes as CS
import modeltrack_scenes as S
import np_modeltrack as T
import np_modeltrack_color as TC
import np_voxelcolor as K
import np_voxelmap as V
from test_modeltrack_spec import PLAIN, SINGLE, SMALL_TRACK, START_A, START_B, H, W, hand_map
from test_voxelmap_spec import ACC_CAM, ACC_SHAPE, SMALL, SMALL_CAM, pose_t, small_frame, yaw_pose

INV = V.INVALID


def small_image(seed, w=24, h=10, gray=False):
    """A smooth pattern plus +-8 levels of noise: the colour volume gets a gradient and neighbouring voxels differ.  -> uint8 [h, w, 3] or [h, w]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    levels = [128 + 90 * np.sin(0.45 * x + 0.3 * y), 128 + 90 * np.sin(0.6 * y - 0.25 * x), 128 + 90 * np.cos(0.35 * x)]
    im = np.clip(np.stack([np.floor(v + 0.5) for v in levels], axis=2) + rng.integers(-8, 9, (h, w, 3)), 0, 255).astype(np.uint8)
    return im[..., 1].copy() if gray else im


def small_model(shape=(16, 16, 24), frames=3, origin_shift=(0.0, 0.0, 0.0), cam=SMALL_CAM, w=24, h=10, gray=False, colour_frames=None, **mp):
    """test_modeltrack_spec.small_map with a colour volume beside it: `frames` of small_frame integrated into the map, the first
    `colour_frames` of them (default: all) into the colour volume too.  -> (Map, Color, last pose)."""
    m = V.Map(*shape, V.params(**dict(SMALL, **mp)))
    c = K.Color(m)
    pose = None
    for k in range(frames):
        pose = yaw_pose(1.5 * k, (origin_shift[0] + 0.03 * k, origin_shift[1], origin_shift[2] + 0.05 * k))
        d, _ = small_frame(20 + k, w=w, h=h, cam=cam)
        m.integrate(cam, pose, d)
        if colour_frames is None or k < colour_frames:
            c.integrate(cam, pose, d, small_image(50 + k, w, h, gray))
    return m, c, pose


def same_sums(m, c, p, cp, pose, disp, image, mask, cam=SMALL_CAM):
    R, t = T.split(pose)
    n, nc, nph, s = TC.evaluate(m, c, cam, p, cp, R, t, disp, image, mask)
    sn, snc, snph, sums = TC.scalar_evaluate(m, c, cam, p, cp, R, t, disp, image, mask)
    assert (n, nc, nph) == (sn, snc, snph)
    assert np.array(s).tobytes() == np.array(sums).tobytes()
    return n, nc, nph


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("gray", [False, True])
def test_vectorised_restatement_equals_the_scalar_loop(gray, masked, stride):
    m, c, pose = small_model(gray=gray)
    disp, mask = small_frame(31)
    image = small_image(61, gray=gray)
    p, cp = T.params(stride=stride, **SMALL_TRACK), TC.params()
    photo = 0
    for start in (pose, S.perturb(pose, (0.04, -0.02, 0.03), 1.0), S.perturb(pose, (-0.6, 0.1, 0.3), -8.0)):
        n, nc, nph = same_sums(m, c, p, cp, start, disp, image, mask if masked else None)
        assert nph <= n <= nc
        photo += nph
    assert photo > 0


def test_the_scalar_loop_agrees_off_the_defaults():
    """A gate that drops photometric inliers, a colour weight gate above some voxels' weight, and a window whose origin is no multiple of
    the volume size on any axis."""
    m, c, pose = small_model(origin_shift=(2.2, -1.3, -1.3))
    assert all(o % n for o, n in zip(c.origin, (c.nx, c.ny, c.nz))) and c.origin == m.origin
    disp, mask = small_frame(32)
    image = small_image(62)
    p = T.params(**SMALL_TRACK)
    n_all, _, ph_all = same_sums(m, c, p, TC.params(photo_gate=1.0), pose, disp, image, mask)
    n_gate, _, ph_gate = same_sums(m, c, p, TC.params(photo_gate=0.02), pose, disp, image, mask)
    n_w, _, ph_w = same_sums(m, c, p, TC.params(photo_gate=1.0, color_min_weight=3), pose, disp, image, mask)
    assert n_all == n_gate == n_w and 0 < ph_gate < ph_all and 0 < ph_w < ph_all
    assert int((c.weight >= 3).sum()) < int((c.weight >= 1).sum())


def scalar_eval(m, c, cam, p, cp, R, t, d, im, mk):
    return TC.scalar_evaluate(m, c, cam, p, cp, R, t, d, im, mk)


def test_refine_through_the_scalar_evaluation_gives_the_same_record():
    m, c, pose = small_model()
    disp, mask = small_frame(33)
    image = small_image(63)
    p, cp = T.params(iterations=2, **SMALL_TRACK), TC.params(photo_weight=4.0)
    start = S.perturb(pose, (0.03, 0.0, -0.02), 0.7)
    a = TC.refine(m, c, SMALL_CAM, p, cp, start, disp, image, mask)
    b = TC.refine(m, c, SMALL_CAM, p, cp, start, disp, image, mask, evaluate=scalar_eval)
    assert a.tobytes() == b.tobytes()
    assert int(a["steps"][0]) == 2 and int(a["status"][0]) == 1 and int(a["n_photo"][0]) > 0 and int(a["n_photo_initial"][0]) > 0
    assert a.tobytes()[:136] != T.refine(m, SMALL_CAM, p, start, disp, mask).tobytes()       # the term moved the estimate


# ---- the hand-worked sample ------------------------------------------------------------------------------------
HAND_BGR = {(0, 0): ((20, 30, 20), (60, 90, 60)), (0, 1): ((40, 60, 40), (100, 200, 100)),          # [dz][dy] = (dx 0, dx 1) as (b, g, r)
            (1, 0): ((10, 10, 10), (20, 40, 20)), (1, 1): ((0, 0, 0), (200, 200, 200))}


def hand_color(m):
    """The colour companion of test_modeltrack_spec.hand_map: the cell i0 = (2, 1, 2) holds eight colours whose luminances b + 2 g + r are
    t[0][0] = (100, 300), t[0][1] = (200, 600), t[1][0] = (40, 120), t[1][1] = (0, 800), each with weight 1."""
    c = K.Color(m)
    c.origin = (0, 0, 0)
    for (dz, dy), row in HAND_BGR.items():
        for dx in (0, 1):
            c.c[2 + dz, 1 + dy, 2 + dx] = row[dx]
            c.weight[2 + dz, 1 + dy, 2 + dx] = 1
    return c


def test_hand_worked_sample():
    """p and fr as in 7.16: p = (0.34375, 0.21875, 0.40625) m, i0 = (2, 1, 2), fr = (0.25, 0.25, 0.75).
    D[dy][dz]: D00 = 200, D10 = 400, D01 = 80, D11 = 800.  c = t0 + 0.25 D: c00 = 150, c10 = 300, c01 = 60, c11 = 200.
    h0 = 150, h1 = 140; e0 = 150 + 0.25 * 150 = 187.5, e1 = 60 + 0.25 * 140 = 95; gc_z = -92.5; C = 187.5 + 0.75 * -92.5 = 118.125.
    gc_y = 150 + 0.75 * -10 = 142.5.  a0 = 200 + 0.25 * 200 = 250, a1 = 80 + 0.25 * 720 = 260, gc_x = 250 + 0.75 * 10 = 257.5.
    The pixel is (b, g, r) = (10, 25, 20): L_obs = 10 + 50 + 20 = 80, rc = (118.125 - 80) / 1020 = 38.125 / 1020.
    Gc = gc / (1020 * 0.125) = gc / 127.5; p x gc = (-78.125, 136.40625, -7.34375), so Jc = (p x gc, gc) / 127.5 up to the rounding of the
    divisions taken first."""
    m = hand_map()
    c = hand_color(m)
    px, py, pz = 0.34375, 0.21875, 0.40625
    cp = TC.params()
    lum = TC.Luminance(c, cp)
    Cv, gx, gy, gz, fr, t = T.scalar_sample(lum, px, py, pz)
    assert fr == [0.25, 0.25, 0.75] and (Cv, gx, gy, gz) == (118.125, 257.5, 142.5, -92.5)
    assert t == [[[100, 300], [200, 600]], [[40, 120], [0, 800]]]
    known, Cvv, gxv, gyv, gzv = T.sample(lum, [np.array([v]) for v in (px, py, pz)], np.array([True]))
    assert bool(known[0]) and (float(Cvv[0]), float(gxv[0]), float(gyv[0]), float(gzv[0])) == (118.125, 257.5, 142.5, -92.5)
    # through one pixel: the optical axis of a 1 x 1 image at disparity 256 (Z = 0.5) and a pose that carries (0, 0, 0.5) to p
    cam = V.camera(fx=256.0, fy=256.0, cx=0.0, cy=0.0, baseline=0.5)
    disp = np.array([[4096]], np.int16)
    image = np.array([[[10, 25, 20]]], np.uint8)
    assert int(TC.observed(image)[0, 0]) == 80 == TC.scalar_observed(image, 0, 0) and int(TC.observed(np.array([[20]], np.uint8))[0, 0]) == 80
    R, tt = T.split(pose_t(px, py, pz - 0.5))
    p = T.params(**SMALL_TRACK)
    cand, inl, pin, gv, cv = TC.terms(m, c, cam, p, cp, R, tt, disp, image)
    assert bool(cand[0, 0]) and bool(inl[0, 0]) and bool(pin[0, 0])
    gs = 1020.0 * 0.125
    G = [257.5 / gs, 142.5 / gs, -92.5 / gs]
    J = [py * G[2] - pz * G[1], pz * G[0] - px * G[2], px * G[1] - py * G[0]] + G
    rc = (118.125 - 80.0) / 1020.0
    lam = 64.0
    expect = [(lam * J[i]) * J[j] for i in range(6) for j in range(i, 6)] + [(lam * J[i]) * rc for i in range(6)] + [0.0, rc * rc]
    assert [float(v) for v in cv[:, 0, 0]] == expect
    assert np.allclose(J[:3], [-78.125 / gs, 136.40625 / gs, -7.34375 / gs], rtol=1e-14, atol=0.0)
    got = TC.scalar_pixel(m, c, cam, p, cp, R, tt, disp, image, None, 0, 0)
    assert got[0] is True and got[2] == expect and got[1] == [float(v) for v in gv[:, 0, 0]]
    # the geometric values are S34's, the sums are geometric + photometric in that order, and sums 27 and 28 keep to their own term
    n, nc, nph, s = TC.evaluate(m, c, cam, p, cp, R, tt, disp, image)
    assert (n, nc, nph) == (1, 1, 1) and s[27] == got[1][27] and s[28] == rc * rc and s[0] == got[1][0] + expect[0]
    # the photometric gate, a corner below color_min_weight, photo_weight = 0 and no colour window: a geometric inlier only
    for bad in (TC.params(photo_gate=0.037), TC.params(color_min_weight=2), TC.params(photo_weight=0.0)):
        assert TC.evaluate(m, c, cam, p, bad, R, tt, disp, image)[:3] == (1, 1, 0) == TC.scalar_evaluate(m, c, cam, p, bad, R, tt, disp, image)[:3]
    assert TC.evaluate(m, c, cam, p, TC.params(photo_gate=0.038), R, tt, disp, image)[2] == 1                 # |rc| = 0.03738
    c.origin = None
    assert TC.evaluate(m, c, cam, p, cp, R, tt, disp, image)[:3] == (1, 1, 0) == TC.scalar_evaluate(m, c, cam, p, cp, R, tt, disp, image)[:3]


def test_the_gradient_is_the_central_difference_of_C_inside_a_cell():
    """C is trilinear inside a cell, so a central difference reproduces the analytic gradient up to rounding: |C| <= 1020 and a step of
    1 / 64 voxel put the difference quotient's rounding error below 64 * 4 * 2^-53 * 1020 < 1e-10 luminance units per voxel."""
    rng = np.random.default_rng(3)
    m = V.Map(16, 16, 16, V.params(**SMALL))
    c = K.Color(m)
    c.origin = (-8, 8, 24)
    c.c[:] = rng.integers(0, 256, c.c.shape)
    c.weight[:] = 1
    lum = TC.Luminance(c, TC.params())
    assert int(lum.tsdf.max()) > 900 and int(lum.tsdf.min()) < 100
    vs, h = 0.125, 1.0 / 64.0
    for _ in range(50):
        cell = rng.integers(0, 15, 3) + np.array(c.origin)
        a = cell + 0.125 + 0.75 * rng.random(3)                                # well inside the cell
        pt = [(float(v) + 0.5) * vs for v in a]
        Cv, gx, gy, gz = T.scalar_sample(lum, *pt)[:4]
        for axis, g in enumerate((gx, gy, gz)):
            lo, hi = list(pt), list(pt)
            lo[axis] -= h * vs
            hi[axis] += h * vs
            fd = (T.scalar_sample(lum, *hi)[0] - T.scalar_sample(lum, *lo)[0]) / (2.0 * h)
            assert abs(fd - g) < 1e-7, (axis, fd, g)                           # 1e-10 from the quotient, the rest from p / vs - 0.5 not being exact


# ---- the reductions to S34 -----------------------------------------------------------------------------------------------------
def test_photo_weight_zero_is_S34_byte_for_byte():
    m, c, pose = small_model()
    disp, mask = small_frame(34)
    p = T.params(**SMALL_TRACK)
    start = S.perturb(pose, (0.03, 0.01, -0.02), 0.7)
    ref = T.refine(m, SMALL_CAM, p, start, disp, mask)
    got = TC.refine(m, c, SMALL_CAM, p, TC.params(photo_weight=0.0), start, disp, small_image(64), mask)
    assert int(ref["status"][0]) == 1 and got.tobytes()[:136] == ref.tobytes()
    r = got[0]
    assert (int(r["n_photo"]), int(r["n_photo_initial"]), float(r["rms_photo"]), float(r["rms_photo_initial"])) == (0, 0, 0.0, 0.0)
    assert float(r["cost"]) == float(r["rms"]) and float(r["cost_initial"]) == float(r["rms_initial"])


def test_an_empty_colour_volume_is_S34():
    m, c, pose = small_model()
    disp, mask = small_frame(34)
    p = T.params(**SMALL_TRACK)
    start = S.perturb(pose, (0.03, 0.01, -0.02), 0.7)
    ref = T.refine(m, SMALL_CAM, p, start, disp, mask)
    c.clear()
    got = TC.refine(m, c, SMALL_CAM, p, TC.params(), start, disp, small_image(64), mask)
    assert got.tobytes()[:136] == ref.tobytes() and int(got["n_photo"][0]) == 0 == int(got["n_photo_initial"][0])
    assert float(got["cost"][0]) == float(got["rms"][0]) and TC.accept(got, start, p) == T.accept(ref, start, p)
    # a window whose voxels are all empty behaves the same
    c.origin = m.origin
    again = TC.refine(m, c, SMALL_CAM, p, TC.params(), start, disp, small_image(64), mask)
    assert again.tobytes() == got.tobytes()


def lagging_model():
    """The map integrates one more frame than the colour volume, at a pose one metre ahead: its window moves by 8 voxels on z and the
    colour object stays where its last integrate left it."""
    m, c, pose = small_model(frames=3)
    ahead = yaw_pose(3.0, (0.06, 0.0, 1.1))
    d, _ = small_frame(23)
    m.integrate(SMALL_CAM, ahead, d)
    return m, c, pose


def test_a_colour_window_that_lags_the_maps_is_sampled_by_its_own_origin():
    m, c, pose = lagging_model()
    assert c.origin is not None and c.origin != m.origin and c.origin[2] + 8 == m.origin[2]
    disp, mask = small_frame(35)
    image = small_image(65)
    p, cp = T.params(**SMALL_TRACK), TC.params(photo_gate=1.0)
    mid = S.perturb(pose, (0.0, 0.0, 0.4), 0.5)
    n, nc, nph = same_sums(m, c, p, cp, mid, disp, image, mask)
    assert 0 < nph <= n
    # the same colours read with the map's indices (the colour volume shifted by the move) give other sums: the origin matters
    R, t = T.split(mid)
    shifted = K.Color(m)
    shifted.c, shifted.weight, shifted.origin = c.c, c.weight, m.origin
    assert TC.evaluate(m, shifted, SMALL_CAM, p, cp, R, t, disp, image, mask)[3] != TC.evaluate(m, c, SMALL_CAM, p, cp, R, t, disp, image, mask)[3]
    # and a colour volume moved to the map's window by S33's rule (what the next colour integrate does first) gives the lagging one's
    # samples wherever both windows hold the cell
    moved = K.Color(m)
    moved.c, moved.weight, moved.origin = c.c.copy(), c.weight.copy(), c.origin
    moved._move(m.origin)
    lum_a, lum_b = TC.Luminance(c, cp), TC.Luminance(moved, cp)
    hits = 0
    for rz, ry, rx in np.argwhere(c.weight >= 1)[::7]:                       # points in coloured voxels of the lagging window
        pt = [(float(c.origin[a] + r) + 0.8) * 0.125 for a, r in enumerate((rx, ry, rz))]
        a, b = T.scalar_sample(lum_a, *pt), T.scalar_sample(lum_b, *pt)
        if a is not None and b is not None:
            assert a[:4] == b[:4]
            hits += 1
    assert hits > 10


# ---- the consumer's rule ---------------------------------------------------------------------------------------------------------
def record(**kw):
    r = np.zeros(1, TC.RESULT_DTYPE)
    r["R"][0], r["t"][0] = [1, 0, 0, 0, 1, 0, 0, 0, 1], [0.1, 0.2, 0.3]
    base = dict(status=1, steps=4, n_candidates=3000, n_initial=2000, n_inliers=2000, rms_initial=0.4, rms=0.2, rms_photo_initial=0.05, rms_photo=0.01,
                cost_initial=0.07, cost=0.03, n_photo_initial=1900, n_photo=1990)
    for k, v in dict(base, **kw).items():
        r[k] = v
    return r


def test_the_cost_rule():
    p = T.params()
    pose0 = pose_t(1.0, 2.0, 3.0)
    taken, pose = TC.accept(record(), pose0, p)
    assert taken and pose == T.join([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.1, 0.2, 0.3])
    assert TC.accept(record(rms=0.41), pose0, p)[0]                           # the geometric rms may rise: the cost decides
    assert TC.accept(record(cost=0.07), pose0, p)[0]                          # equal is taken
    assert TC.accept(record(n_photo=0, n_photo_initial=0, rms_photo=0.0, rms_photo_initial=0.0), pose0, p)[0]   # no photometric inlier is legal
    for bad in (dict(cost=0.0700001), dict(status=0), dict(n_inliers=1023), dict(cost=float("nan")), dict(rms=float("inf")), dict(rms_photo=float("nan")),
                dict(cost_initial=float("inf")), dict(rms_photo_initial=float("nan")), dict(rms_initial=float("nan"))):
        assert TC.accept(record(**bad), pose0, p) == (False, pose0), bad
    r = record()
    r["t"][0][1] = float("nan")
    assert TC.accept(r, pose0, p) == (False, pose0)
    # cost: the weighted mean residual; rms at photo_weight 0 or without photometric inliers; 0 at a zero denominator
    assert TC.cost_of(8.0, 2, 3.0, 1, 64.0) == math.sqrt((8.0 + 64.0 * 3.0) / (2.0 + 64.0 * 1.0))
    assert TC.cost_of(8.0, 2, 0.0, 0, 64.0) == math.sqrt(8.0 / 2.0) == TC.cost_of(8.0, 2, 3.0, 5, 0.0) and TC.cost_of(0.0, 0, 0.0, 0, 64.0) == 0.0


# ---- accuracy of the spec -----------------------------------------------------------------------------------------------------------
# measured on the restatement at seed 5 (modeltrack_color_scenes: one frame against a model of six, every image with +-3 levels of noise,
# defaults, 4 iterations; DESIGN.md 7.20 has the sweep over photo_weight): start -> (along-axis, cross-axis error in m, rotation error in
# degrees) at the end on the plain corridor, (translation error in m, rotation error in degrees) on the corridor with the four boxes
PLAIN_COLOR = {START_A: (0.0007, 0.0034, 0.0216), START_B: (0.0029, 0.0033, 0.0201)}
BOXED_COLOR = {START_A: (0.0167, 0.1114), START_B: (0.0176, 0.1099)}
_MODELS = {}


def corridor(boxed):
    if boxed not in _MODELS:
        _MODELS[boxed] = CS.build(ACC_CAM, ACC_SHAPE, W, H, boxes=S.BOXES if boxed else ())
    return _MODELS[boxed]


@pytest.mark.parametrize("start", [START_A, START_B])
def test_the_plain_corridor_recovers_the_offset_along_the_axis(start):
    """S34 alone leaves the along-axis offset where the prediction put it (photo_weight = 0 below: 0.0775 -> 0.0842 m, 0.155 -> 0.1575 m);
    the photometric term recovers it.  Rotation and cross-axis error stay within twice S34's own figures (test_modeltrack_spec.PLAIN), and
    every figure within twice its own measured value."""
    s, e, true, res = CS.track(corridor(False), ACC_CAM, *start)
    along0, cross0, _, rot0 = CS.errors(s, true)
    along, cross, _, rot = CS.errors(e, true)
    print(start, (along0, cross0, rot0), (along, cross, rot), res)
    assert TC.accept(res, s, T.params())[0]
    assert along < along0
    assert cross <= 2 * PLAIN[start][0] and rot <= 2 * PLAIN[start][1]
    m = PLAIN_COLOR[start]
    assert along <= 2 * m[0] and cross <= 2 * m[1] and rot <= 2 * m[2]
    # the same run without the term is S34's: the offset along the axis is not recovered
    _, e0, _, res0 = CS.track(corridor(False), ACC_CAM, *start, cp=TC.params(photo_weight=0.0))
    assert not CS.errors(e0, true)[0] < along0 and int(res0["n_photo"][0]) == 0


@pytest.mark.parametrize("start", [START_A, START_B])
def test_the_boxed_corridor_ends_no_worse_than_S34(start):
    s, e, true, res = CS.track(corridor(True), ACC_CAM, *start)
    _, _, tot, rot = CS.errors(e, true)
    print(start, CS.errors(s, true), (tot, rot), res)
    assert TC.accept(res, s, T.params())[0]
    assert tot <= 2 * SINGLE[start][0] and rot <= 2 * SINGLE[start][1]
    assert tot <= 2 * BOXED_COLOR[start][0] and rot <= 2 * BOXED_COLOR[start][1]


# ---- the library's host side --------------------------------------------------------------------------------------------------------
def _lib():
    from cartslam import _lib
    return _lib, _lib.load()


CAM = V.camera(fx=256.0, fy=256.0, cx=8.0, cy=4.0, baseline=0.5)


def refine_error(p=None, cp=None, params_null=False, color_params_null=False, channels=3, cam=CAM, pose=V.POSE_IDENTITY, w=16, h=8):
    """cart_model_track_refine_color without an object: a valid configuration gets as far as the missing object."""
    L, lib = _lib()
    tp, tcp = L.ModelTrackParams(), L.ModelTrackColorParams()
    lib.cart_model_track_default_params(C.byref(tp))
    lib.cart_model_track_color_default_params(C.byref(tcp))
    for k, v in (p or {}).items():
        setattr(tp, k, v)
    for k, v in (cp or {}).items():
        setattr(tcp, k, v)
    c = L.EgoCamera(*[cam[k] for k in ("fx", "fy", "cx", "cy", "baseline")]) if cam is not None else None
    P = (C.c_double * 12)(*pose) if pose is not None else None
    rc = lib.cart_model_track_refine_color(None, None, None, C.byref(c) if c is not None else None, P, None if params_null else C.byref(tp),
                                           None if color_params_null else C.byref(tcp), None, 0, None, 0, channels, None, 0, w, h, None, None)
    assert rc != 0
    return lib.cart_last_error(None).decode()


def test_defaults_layout_and_exports():
    from cartslam import MODEL_TRACK_COLOR_RESULT_DTYPE, MODEL_TRACK_RESULT_DTYPE, ModelTrack, ModelTrackColorParams, ModelTrackColorResult, model_track_color_params
    L, lib = _lib()
    assert C.sizeof(ModelTrackColorParams) == 24 and [n for n, _ in ModelTrackColorParams._fields_] == list(TC.DEFAULTS) + ["reserved"]
    assert (ModelTrackColorParams.photo_weight.offset, ModelTrackColorParams.photo_gate.offset, ModelTrackColorParams.color_min_weight.offset,
            ModelTrackColorParams.reserved.offset) == (0, 8, 16, 20)
    assert C.sizeof(ModelTrackColorResult) == 176 == MODEL_TRACK_COLOR_RESULT_DTYPE.itemsize and MODEL_TRACK_COLOR_RESULT_DTYPE == TC.RESULT_DTYPE
    assert [n for n, _ in ModelTrackColorResult._fields_] == list(MODEL_TRACK_COLOR_RESULT_DTYPE.names)
    assert list(MODEL_TRACK_COLOR_RESULT_DTYPE.names)[:len(MODEL_TRACK_RESULT_DTYPE.names)] == list(MODEL_TRACK_RESULT_DTYPE.names)
    for name in MODEL_TRACK_RESULT_DTYPE.names:                              # the first 136 bytes are cart_model_track_result's
        assert MODEL_TRACK_COLOR_RESULT_DTYPE.fields[name][1] == MODEL_TRACK_RESULT_DTYPE.fields[name][1] == getattr(ModelTrackColorResult, name).offset
    assert (ModelTrackColorResult.rms_photo_initial.offset, ModelTrackColorResult.rms_photo.offset, ModelTrackColorResult.cost_initial.offset,
            ModelTrackColorResult.cost.offset, ModelTrackColorResult.n_photo_initial.offset, ModelTrackColorResult.n_photo.offset) == (136, 144, 152, 160, 168, 172)
    p = model_track_color_params()
    assert {k: getattr(p, k) for k in TC.DEFAULTS} == TC.DEFAULTS == dict(photo_weight=64.0, photo_gate=0.25, color_min_weight=1) and p.reserved == 0
    assert model_track_color_params(photo_weight=4.0).photo_weight == 4.0
    with pytest.raises(ValueError) as err:
        model_track_color_params(window=3)
    assert str(err.value) == "cart_model_track_color_params has no field window"
    lib.cart_model_track_color_default_params(None)                           # a NULL pointer is ignored
    for name in ("cart_model_track_color_default_params", "cart_model_track_refine_color"):
        assert hasattr(lib, name) and name in L.PROTOTYPES
    assert hasattr(ModelTrack, "refine_color")
    assert C.sizeof(L.ModelTrackParams) == 32 and C.sizeof(L.ModelTrackResult) == 136      # S34's structs gained nothing


def test_every_parameter_is_checked_before_any_object():
    assert refine_error() == "bad arguments"                                  # a valid configuration gets as far as the missing object
    assert refine_error(params_null=True) == "params is NULL" and refine_error(color_params_null=True) == "color_params is NULL"
    nan, inf = float("nan"), float("inf")
    bad = (("photo_weight", -1e-9), ("photo_weight", nan), ("photo_weight", inf), ("photo_gate", 0.0), ("photo_gate", -0.5), ("photo_gate", 1.0000001),
           ("photo_gate", nan), ("photo_gate", inf), ("color_min_weight", 0), ("color_min_weight", 256), ("reserved", 1))
    for name, value in bad:
        assert name in refine_error(cp={name: value}), (name, value)
    for name, value in (("residual_gate", 0.0), ("damping", -1.0), ("iterations", 17), ("stride", 0), ("min_inliers", 5)):
        assert name in refine_error(p={name: value}), (name, value)
    for ok in (dict(photo_weight=0.0), dict(photo_weight=1e300), dict(photo_gate=1.0), dict(photo_gate=1e-300), dict(color_min_weight=1), dict(color_min_weight=255)):
        assert refine_error(cp=ok) == "bad arguments", ok
    # the order: params, color_params, channels, camera, pose0, sizes, then the objects
    assert "stride" in refine_error(p=dict(stride=0), cp=dict(photo_gate=0.0), channels=2)
    assert "photo_gate" in refine_error(cp=dict(photo_gate=0.0), channels=2, cam=None)
    for ch in (0, 2, 4):
        assert refine_error(channels=ch, cam=None) == "channels must be 1 or 3"
    assert refine_error(channels=1) == "bad arguments"
    assert "camera" in refine_error(cam=None, pose=None, w=0)
    assert refine_error(pose=None, w=0) == "pose0 is NULL"
    for kw, word in ((dict(w=0), "width"), (dict(w=16385), "width"), (dict(h=0), "height")):
        assert word in refine_error(**kw)


def test_all_zero_arguments_are_refused_with_a_message():
    L, lib = _lib()
    assert lib.cart_model_track_refine_color(None, None, None, None, None, None, None, None, 0, None, 0, 0, None, 0, 0, 0, None, None) != 0
    assert lib.cart_last_error(None).decode() == "params is NULL"

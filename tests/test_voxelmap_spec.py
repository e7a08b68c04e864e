"""CPU tests of spec S33, the rolling TSDF voxel map with model raycast: the numpy restatement tests/np_voxelmap.py against a
scalar twin written here (a pure-Python loop over voxels and rays in Python floats, IEEE doubles with one rounding per operation, and Python
integers), the hand-worked case, the accuracy of the spec on a synthetic corridor, and the library's host-side checks (no GPU: validation
comes before any device call).  tests/test_gpu_voxelmap.py runs the cases built here on the device."""
import ctypes as C
import math

import numpy as np
import pytest

import np_voxelmap as V

INV = V.INVALID
CAM = V.camera(fx=256.0, fy=256.0, cx=8.0, cy=4.0, baseline=0.5)          # the hand-worked case's
SMALL_CAM = V.camera(fx=24.0, fy=24.0, cx=11.5, cy=4.5, baseline=0.5)     # a 24 x 10 image that sees a 2 x 2 x 3 m volume
# a 16 x 16 x 24 volume of 0.125 m voxels is 2 x 2 x 3 m: the depth range and the look-ahead are cut to it
SMALL = dict(max_depth=3.0, lookahead=1.5, min_depth=0.25)


def pose_t(tx=0.0, ty=0.0, tz=0.0):
    p = list(V.POSE_IDENTITY)
    p[3], p[7], p[11] = tx, ty, tz
    return p


def yaw_pose(deg, t=(0.0, 0.0, 0.0)):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [c, 0.0, s, t[0], 0.0, 1.0, 0.0, t[1], -s, 0.0, c, t[2]]


# exact quarter turns: camera z along world x, and along world -z
POSE_90 = [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0]
POSE_180 = [-1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0]


def small_frame(seed, w=24, h=10, cam=SMALL_CAM, depth=1.5, holes=0.1, masked=True):
    """A fronto-parallel wall at about `depth` metres with a step two columns right of the optical axis, +-1/4 px noise, holes and sub-minimum pixels, and a MOVING block in the mask.
    -> (disp int16 [h, w], mask uint8 [h, w])."""
    rng = np.random.default_rng(seed)
    d = np.full((h, w), cam["fx"] * cam["baseline"] / depth * 16.0)
    d[:, w // 2 + 2:] = cam["fx"] * cam["baseline"] / (depth + 0.6) * 16.0
    disp = (np.round(d) + rng.integers(-4, 5, (h, w))).astype(np.int16)
    disp[rng.random((h, w)) < holes] = INV
    disp[rng.random((h, w)) < 0.03] = 8                                   # below min_disparity
    mask = (2 * rng.integers(0, 2, (h, w))).astype(np.uint8) if masked else None          # STATIC and UNKNOWN, and one MOVING block
    if masked:
        mask[2:5, 3:9] = V.MOVING
    return disp, mask


# ---- the scalar twin ----------------------------------------------------------------------------------------------------------------
class ScalarMap:
    """Spec S33 one voxel and one ray at a time.  The volume is a dict over absolute voxels: a voxel outside the window does not exist."""

    def __init__(self, nx, ny, nz, p):
        self.n, self.p = (nx, ny, nz), p
        self.origin, self.vox = None, {}

    def clear(self):
        self.origin, self.vox = None, {}

    def window_origin(self, P):
        out = []
        for a in range(3):
            c = math.floor((P[4 * a + 3] + self.p["lookahead"] * P[4 * a + 2]) / self.p["voxel_size"])
            out.append(8 * ((c - self.n[a] // 2) // 8))
        return tuple(out)

    def inside(self, g):
        return all(self.origin[a] <= g[a] < self.origin[a] + self.n[a] for a in range(3))

    def integrate(self, cam, pose, disp, mask=None):
        p, P = self.p, [float(v) for v in pose]
        h, w = disp.shape
        self.origin = self.window_origin(P)
        self.vox = {g: v for g, v in self.vox.items() if self.inside(g)}      # what left is forgotten; what entered is absent = empty
        fxb = cam["fx"] * cam["baseline"]
        updated = near = 0
        o = self.origin
        for gz in range(o[2], o[2] + self.n[2]):
            for gy in range(o[1], o[1] + self.n[1]):
                for gx in range(o[0], o[0] + self.n[0]):
                    d0, d1, d2 = (float(gx) + 0.5) * p["voxel_size"] - P[3], (float(gy) + 0.5) * p["voxel_size"] - P[7], (float(gz) + 0.5) * p["voxel_size"] - P[11]
                    q = [(P[c] * d0 + P[4 + c] * d1) + P[8 + c] * d2 for c in range(3)]
                    if not q[2] >= p["min_depth"]:
                        continue
                    u, v = (cam["fx"] * q[0]) / q[2] + cam["cx"], (cam["fy"] * q[1]) / q[2] + cam["cy"]
                    xd, yd = math.floor(u + 0.5), math.floor(v + 0.5)
                    if not (0 <= xd <= w - 1 and 0 <= yd <= h - 1):
                        continue
                    s = int(disp[yd, xd])
                    if s == INV:
                        continue
                    d = s / 16.0
                    if not d >= p["min_disparity"]:
                        continue
                    Z = fxb / d
                    if not Z <= p["max_depth"]:
                        continue
                    if mask is not None and int(mask[yd, xd]) == V.MOVING:
                        continue
                    tr = p["truncation"] + p["disparity_sigma"] * ((Z * Z) / fxb)
                    sdf = Z - q[2]
                    if not sdf >= -tr:
                        continue
                    f = sdf / tr
                    near += f < 1.0
                    f = 1.0 if f > 1.0 else f
                    obs = int(math.floor(f * 32767.0 + 0.5))
                    t, wt = self.vox.get((gx, gy, gz), (0, 0))
                    self.vox[(gx, gy, gz)] = ((2 * (wt * t + obs) + (wt + 1)) // (2 * (wt + 1)), min(wt + 1, p["max_weight"]))
                    updated += 1
        return np.array([updated, near], np.int32)

    def read(self):
        out = np.zeros((self.n[2], self.n[1], self.n[0]), V.VOXEL_DTYPE)
        for (gx, gy, gz), (t, wt) in self.vox.items():
            out[gz - self.origin[2], gy - self.origin[1], gx - self.origin[0]] = (t, wt)
        return out, (self.origin if self.origin is not None else (0, 0, 0))

    def raycast(self, cam, pose, width, height):
        p, P = self.p, [float(v) for v in pose]
        fxb = cam["fx"] * cam["baseline"]
        disp = np.full((height, width), INV, np.int16)
        weight = np.zeros((height, width), np.uint16)
        status = np.zeros((height, width), np.uint8)
        K = int(math.floor((p["max_depth"] - p["min_depth"]) / p["march_step"]))
        for y in range(height):
            for x in range(width):
                have_prev, Fp, zp = False, 0.0, 0.0
                for k in range(K + 1 if self.origin is not None else 0):
                    z = p["min_depth"] + float(k) * p["march_step"]
                    X, Y = ((float(x) - cam["cx"]) * z) / cam["fx"], ((float(y) - cam["cy"]) * z) / cam["fy"]
                    pw = [((P[4 * r] * X + P[4 * r + 1] * Y) + P[4 * r + 2] * z) + P[4 * r + 3] for r in range(3)]
                    a = [c / p["voxel_size"] - 0.5 for c in pw]
                    i0 = [math.floor(c) for c in a]
                    fr = [a[c] - i0[c] for c in range(3)]
                    corners = {(dx, dy, dz): (i0[0] + dx, i0[1] + dy, i0[2] + dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
                    known = all(self.inside(g) for g in corners.values())
                    if known:
                        vals = {k3: self.vox.get(g, (0, 0)) for k3, g in corners.items()}
                        wmin = min(v[1] for v in vals.values())
                        known = wmin >= p["min_weight"]
                    if not known:
                        have_prev = False
                        continue
                    c = {(dy, dz): float(vals[(0, dy, dz)][0]) + fr[0] * float(vals[(1, dy, dz)][0] - vals[(0, dy, dz)][0]) for dy in (0, 1) for dz in (0, 1)}
                    e0 = c[(0, 0)] + fr[1] * (c[(1, 0)] - c[(0, 0)])
                    e1 = c[(0, 1)] + fr[1] * (c[(1, 1)] - c[(0, 1)])
                    F = e0 + fr[2] * (e1 - e0)
                    if F > 0.0:
                        have_prev, Fp, zp = True, F, z
                        continue
                    if not have_prev:
                        status[y, x] = V.INSIDE
                        break
                    zs = zp + (p["march_step"] * Fp) / (Fp - F)
                    sw = math.floor((fxb / zs) * 16.0 + 0.5)
                    if 1 <= sw <= 32767:
                        disp[y, x], weight[y, x], status[y, x] = sw, wmin, V.HIT
                    break
        counts = np.array([(status == k).sum() for k in (V.NONE, V.HIT, V.INSIDE)], np.int32)
        return dict(disp=disp, weight=weight, status=status, counts=counts)


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def compare_chain(frames, p, shape=(16, 16, 24), cam=SMALL_CAM, ray=(24, 10)):
    """frames = [(pose, disp, mask)]: both maps integrate every frame and raycast after each from its pose.  -> the restatement's results."""
    a, b = V.Map(*shape, p), ScalarMap(*shape, p)
    results = []
    for k, (pose, disp, mask) in enumerate(frames):
        ca, cb = a.integrate(cam, pose, disp, mask), b.integrate(cam, pose, disp, mask)
        same(ca, cb, ("counts", k))
        (va, oa), (vb, ob) = a.read(), b.read()
        assert tuple(oa) == tuple(ob), ("origin", k)
        same(va, vb, ("voxels", k))
        ra, rb = a.raycast(cam, pose, *ray), b.raycast(cam, pose, *ray)
        for name in ("disp", "weight", "status", "counts"):
            same(ra[name], rb[name], (name, k))
        results.append(dict(counts=ca, origin=tuple(oa), voxels=va, ray=ra))
    return results


# the window cases of the issue, each a chain of frames on the small volume: (name, [pose per frame], masked)
CHAINS = {
    "still": [pose_t()] * 3,
    "forward": [pose_t(tz=0.5 * k) for k in range(4)],                        # 4 voxels per frame: the window moves 8 on z every other frame
    "lateral": [pose_t(), pose_t(tx=1.0), pose_t(tx=1.0, ty=-1.0)],           # one move on x, then one on y
    "jump": [pose_t(), pose_t(tz=0.25), pose_t(tz=40.0), pose_t(tz=40.25)],   # a move of >= N on z empties everything
    "rotated": [yaw_pose(0.0), yaw_pose(7.0, (0.05, -0.02, 0.1)), yaw_pose(-11.0, (0.1, 0.0, 0.3))],
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_vectorised_restatement_equals_the_scalar_loop(name):
    poses = CHAINS[name]
    frames = []
    for k, pose in enumerate(poses):
        disp, mask = small_frame(31 * len(name) + k)
        frames.append((pose, disp, mask if k % 2 == 0 else None))
    res = compare_chain(frames, V.params(**SMALL))
    assert all(r["counts"][0] > 50 and 0 < r["counts"][1] < r["counts"][0] for r in res), [r["counts"] for r in res]
    origins = [r["origin"] for r in res]
    if name == "forward":
        assert [o[2] for o in origins] == [0, 0, 8, 8] and res[-1]["voxels"]["weight"].max() == 4
    if name == "lateral":
        assert origins[1][0] == origins[0][0] + 8 and origins[2][1] == origins[1][1] - 8
    if name == "jump":
        assert origins[2][2] - origins[1][2] >= 24 and res[2]["voxels"]["weight"].max() == 1 and res[1]["voxels"]["weight"].max() == 2
    if name == "still":
        assert res[-1]["voxels"]["weight"].max() == 3
        assert (res[-1]["ray"]["counts"] > 0).all(), res[-1]["ray"]["counts"]    # the premise: NONE, HIT and INSIDE all occur
    # masked pixels and holes left their mark: frame 0 was masked
    assert res[0]["counts"][0] < compare_chain([(poses[0], frames[0][1], None)], V.params(**SMALL))[0]["counts"][0]


def test_all_three_ray_statuses_occur_and_a_hit_is_close_to_the_wall():
    disp, _ = small_frame(5, holes=0.0, masked=False)
    m = V.Map(16, 16, 24, V.params(**SMALL))
    m.integrate(SMALL_CAM, pose_t(), disp)
    r = m.raycast(SMALL_CAM, pose_t(), 24, 10)
    assert (r["counts"] > 0).all() and r["counts"].sum() == 240
    hit = r["status"] == V.HIT
    assert (r["weight"][hit] >= 1).all() and (r["weight"][~hit] == 0).all() and (r["disp"][~hit] == INV).all()
    ok = hit & (disp >= 16)
    assert ok.sum() > 40 and np.abs(r["disp"][ok].astype(int) - disp[ok]).max() <= 16 * 3    # a step of 0.6 m lies between the two halves
    # min_weight = 2 after one frame: nothing is known; before any integrate: everything is NONE
    m2 = V.Map(16, 16, 24, V.params(min_weight=2, **SMALL))
    assert m2.raycast(SMALL_CAM, pose_t(), 24, 10)["counts"].tolist() == [240, 0, 0]
    m2.integrate(SMALL_CAM, pose_t(), disp)
    assert m2.raycast(SMALL_CAM, pose_t(), 24, 10)["counts"].tolist() == [240, 0, 0]
    m2.integrate(SMALL_CAM, pose_t(), disp)
    assert m2.raycast(SMALL_CAM, pose_t(), 24, 10)["counts"][1] > 0


def test_hand_worked_voxel():
    """Identity pose, fx = fy = 256, cx = 8, cy = 4, baseline 0.5, constant disparity 64 px, voxel g = (0, 0, 7).  The case as it was worked
    by hand has the voxel's centre at (0.125, 0.125, 1.875) = (g + 0.5) 0.25: that is a voxel of 0.25 m with every other parameter at its
    default (at the default 0.125 m the same g has its centre at half those coordinates; that voxel's own numbers are checked last).
    u = 256 * 0.125 / 1.875 + 8 = 25.07 and v = 21.07: pixel (25, 21); Z = 128 / 64 = 2, tr = 0.25 + 0.5 * (4 / 128) = 0.265625,
    sdf = 0.125, f = 0.470588..., obs = floor(15419.76 + 0.5) = 15420; it holds (15420, 1) after one integrate and (15420, 2) after two."""
    disp = np.full((48, 48), 64 * 16, np.int16)
    for cls in (V.Map, ScalarMap):
        m = cls(32, 32, 64, V.params(voxel_size=0.25))
        m.integrate(CAM, V.POSE_IDENTITY, disp)
        vox, o = m.read()
        assert tuple(o) == (-16, -16, 0)
        assert tuple(vox[7 - o[2], 0 - o[1], 0 - o[0]]) == (15420, 1)
        m.integrate(CAM, V.POSE_IDENTITY, disp)
        vox, o = m.read()
        assert tuple(vox[7 - o[2], 0 - o[1], 0 - o[0]]) == (15420, 2)
    assert math.floor((0.125 / 0.265625) * 32767.0 + 0.5) == 15420
    assert math.floor(256 * 0.125 / 1.875 + 8 + 0.5) == 25 and math.floor(256 * 0.125 / 1.875 + 4 + 0.5) == 21
    # the defaults (0.125 m): voxel (0, 0, 15) has its centre at (0.0625, 0.0625, 1.9375) and projects to (16, 12); sdf = 0.0625,
    # f = 0.0625 / 0.265625 = 0.235294..., obs = floor(7709.88 + 0.5) = 7710
    m = V.Map(32, 32, 160)
    m.integrate(CAM, V.POSE_IDENTITY, disp)
    vox, o = m.read()
    assert tuple(vox[15 - o[2], 0 - o[1], 0 - o[0]]) == (7710, 1)


def test_running_average_rounds_half_up_and_the_weight_saturates():
    def step(t, w, obs, max_weight=64):
        return (2 * (w * t + obs) + (w + 1)) // (2 * (w + 1)), min(w + 1, max_weight)
    assert step(0, 0, 15420) == (15420, 1) and step(15420, 1, 15420) == (15420, 2)
    assert step(100, 1, 101) == (101, 2)                                      # 100.5 rounds up
    assert step(-100, 1, -101) == (-100, 2)                                   # -100.5 rounds up, towards +inf
    assert step(-32767, 65535, -32767, 65535) == (-32767, 65535)
    assert step(7, 1, 9, max_weight=1) == (8, 1)                              # max_weight = 1: the mean of the stored and the new value
    m = V.Map(16, 16, 24, V.params(max_weight=2, **SMALL))
    disp, _ = small_frame(9, masked=False)
    for _ in range(4):
        m.integrate(SMALL_CAM, pose_t(), disp)
    assert m.read()[0]["weight"].max() == 2


# ---- accuracy of the spec -----------------------------------------------------------------------------------------------------------
ACC_CAM = V.camera(fx=128.0, fy=128.0, cx=79.5, cy=25.0, baseline=0.5)
ACC_SHAPE = (96, 64, 160)                                                      # 12 x 8 x 20 m of 0.125 m voxels


def corridor_run(step, seed=11, frames=6, w=160, h=64):
    """Six frames of synth.road_corridor (the same image at every forward position) with uniform +-1/4 pixel noise and 10 % fresh holes per
    frame, integrated at the defaults and raycast from the last pose; np_fusion's S28 on the same frames.  -> figures of the last frame
    against the noise-free truth."""
    import np_fusion as F
    from cartslam import synth
    truth, _ = synth.road_corridor(w, h, *[ACC_CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline")])
    rng = np.random.default_rng(seed)
    ok = truth != INV
    m = V.Map(*ACC_SHAPE)
    prev, fused, d, holes, pose = None, None, None, None, None
    for k in range(frames):
        d = truth.copy()
        d[ok] += rng.integers(-4, 5, int(ok.sum())).astype(np.int16)
        holes = ok & (rng.random((h, w)) < 0.10)
        d[holes] = INV
        pose = pose_t(tz=step * k)
        m.integrate(ACC_CAM, pose, d)
        rel = list(F.REL_IDENTITY)
        rel[11] = -step
        fused = F.update(ACC_CAM, F.params(), rel, d, prev)
        prev = (fused["fused"], fused["age"])
    r = m.raycast(ACC_CAM, pose, w, h)
    hit = r["status"] == V.HIT
    err = (r["disp"].astype(np.float64) - truth) / 16.0
    with np.errstate(divide="ignore"):
        within = ok & (truth >= 16) & (ACC_CAM["fx"] * ACC_CAM["baseline"] / (truth / 16.0) <= V.DEFAULTS["max_depth"])
    raw = ok & ~holes
    agreed = fused["source"] == F.AGREED
    ferr = (fused["fused"].astype(np.float64) - truth) / 16.0
    return dict(rms_hit=float(np.sqrt((err[hit & ok] ** 2).mean())), hit_percent=100.0 * float(hit[within].mean()),
                max_hit=float(np.abs(err[hit & ok]).max()), sky_hits=int((hit & ~ok).sum()),
                rms_raw=float(np.sqrt((((d.astype(np.float64) - truth) / 16.0)[raw] ** 2).mean())),
                rms_fusion_agreed=float(np.sqrt((ferr[agreed] ** 2).mean())), statuses=r["counts"].tolist())


# forward step (m per frame) -> measured on the restatement at seed 11: rms error at HIT pixels (px), valid pixels within max_depth that are
# HIT (%), largest error at a HIT pixel (px); test_accuracy_on_the_corridor's docstring derives the bounds
ACCURACY = {0.0: (0.0564, 87.96, 0.25), 0.25: (0.0506, 98.99, 0.25), 0.5: (0.0561, 98.21, 0.3125)}


@pytest.mark.parametrize("step", sorted(ACCURACY))
def test_accuracy_on_the_corridor(step):
    """Measured values: see ACCURACY and DESIGN.md 7.15.  Each bound sits at twice the measured distance to the ideal (0 px of error, 100 % of
    the pixels filled), so that the measured value lies half-way between the bound and the ideal.  The raw single-frame rms error is
    0.161 px (uniform noise of +-4 sixteenths); np_fusion's AGREED pixels on the same frames have 0.077 px standing still and 0.167 / 0.156 px at
    0.25 / 0.5 m per frame: under motion the model beats S28 threefold, standing still by a quarter.  Standing still fewer pixels are HIT:
    a free-space voxel is known only if it projects to a valid pixel within max_depth, so from one viewpoint the space in front of far
    surfaces next to the vanishing point stays unknown and those rays end INSIDE or NONE; other viewpoints fill it."""
    got = corridor_run(step)
    print(step, got)
    rms_hit, percent, max_hit = ACCURACY[step]
    assert got["sky_hits"] == 0                                               # the sky stays empty
    assert got["rms_hit"] <= 2 * rms_hit
    assert got["hit_percent"] >= 100.0 - 2 * (100.0 - percent)
    assert got["max_hit"] <= 2 * max_hit


# ---- the library's host side --------------------------------------------------------------------------------------------------------
def _lib():
    from cartslam import _lib
    return _lib, _lib.load()


def create_error(nx=16, ny=16, nz=16, p=None, params_null=False):
    L, lib = _lib()
    vp = L.VoxelMapParams()
    lib.cart_voxel_map_default_params(C.byref(vp))
    for k, v in (p or {}).items():
        setattr(vp, k, v)
    out = C.c_void_p()
    assert lib.cart_voxel_map_create(None, nx, ny, nz, None if params_null else C.byref(vp), C.byref(out)) != 0
    return lib.cart_last_error(None).decode()


def call_error(fn, cam=CAM, pose=V.POSE_IDENTITY, w=16, h=8):
    """cart_voxel_map_integrate / _raycast without an object: a valid configuration gets as far as the missing map."""
    L, lib = _lib()
    c = L.EgoCamera(*[cam[k] for k in ("fx", "fy", "cx", "cy", "baseline")]) if cam is not None else None
    P = (C.c_double * 12)(*pose) if pose is not None else None
    cref = C.byref(c) if c is not None else None
    if fn == "integrate":
        rc = lib.cart_voxel_map_integrate(None, cref, P, None, 0, w, h, None, 0, None, None)
    else:
        rc = lib.cart_voxel_map_raycast(None, cref, P, w, h, None, 0, None, 0, None, 0, None, None)
    assert rc != 0
    return lib.cart_last_error(None).decode()


def test_defaults_layout_and_exports():
    from cartslam import VOXEL_DTYPE, Voxel, VoxelMap, VoxelMapParams, voxel_map_params  # noqa: F401
    L, lib = _lib()
    assert C.sizeof(VoxelMapParams) == 8 * 8 + 2 * 4 and VoxelMapParams.march_step.offset == 56 and VoxelMapParams.max_weight.offset == 64
    assert VoxelMapParams.min_weight.offset == 68 and C.sizeof(Voxel) == 4 and VOXEL_DTYPE.itemsize == 4 and VOXEL_DTYPE == V.VOXEL_DTYPE
    p = voxel_map_params()
    assert {k: getattr(p, k) for k in V.DEFAULTS} == V.DEFAULTS
    assert list(V.DEFAULTS) == [n for n, _ in VoxelMapParams._fields_]
    assert voxel_map_params(min_weight=7).min_weight == 7
    with pytest.raises(ValueError) as err:
        voxel_map_params(window=3)
    assert str(err.value) == "cart_voxel_map_params has no field window"
    lib.cart_voxel_map_default_params(None)                                   # a NULL pointer is ignored
    lib.cart_voxel_map_destroy(None)                                          # as every destroy: NULL is ignored
    for name in ("default_params", "create", "destroy", "clear", "window", "integrate", "raycast", "read"):
        assert hasattr(lib, "cart_voxel_map_" + name) and "cart_voxel_map_" + name in L.PROTOTYPES
    assert (L.VOXEL_RAY_NONE, L.VOXEL_RAY_HIT, L.VOXEL_RAY_INSIDE) == (V.NONE, V.HIT, V.INSIDE) == (0, 1, 2)


def test_create_checks_sizes_and_every_parameter_before_the_engine():
    assert create_error() == "bad arguments"                                  # a valid configuration gets as far as the missing engine
    assert create_error(1024, 64, 1024) == "bad arguments" and create_error(256, 64, 256) == "bad arguments"
    for kw, word in ((dict(nx=8), "cells_x"), (dict(nx=1032), "cells_x"), (dict(nx=20), "cells_x"), (dict(ny=0), "cells_y"), (dict(ny=12), "cells_y"),
                     (dict(nz=15), "cells_z"), (dict(nz=2048), "cells_z"), (dict(nx=1024, ny=1024, nz=72), "2^26")):
        assert word in create_error(**kw), kw
    assert create_error(1024, 1024, 64) == "bad arguments"                    # exactly 2^26
    assert "params" in create_error(params_null=True)
    nan, inf = float("nan"), float("inf")
    bad = (("voxel_size", 0.009), ("voxel_size", nan), ("voxel_size", inf), ("min_disparity", 0.0), ("min_disparity", nan), ("min_depth", 0.0),
           ("min_depth", inf), ("max_depth", 0.5), ("max_depth", inf), ("max_depth", nan), ("truncation", 0.0), ("truncation", inf),
           ("disparity_sigma", -0.1), ("disparity_sigma", nan), ("lookahead", 1000.5), ("lookahead", -1001.0), ("lookahead", nan),
           ("march_step", 0.0), ("march_step", 0.26), ("march_step", nan), ("max_weight", 0), ("max_weight", 65536), ("min_weight", 0),
           ("min_weight", 65536))
    for name, value in bad:
        assert name in create_error(p={name: value}), (name, value)
    assert "8192" in create_error(p=dict(max_depth=1100.0, truncation=0.125))  # (1100 - 0.5) / 0.125 = 8796 steps
    for ok in (dict(voxel_size=0.01), dict(disparity_sigma=0.0), dict(lookahead=-1000.0), dict(lookahead=1000.0), dict(march_step=0.25),
               dict(max_weight=65535, min_weight=65535), dict(max_weight=1), dict(max_depth=1024.5)):
        assert create_error(p=ok) == "bad arguments", ok
    # the order: sizes before params before the engine
    assert "cells_y" in create_error(ny=4, p=dict(voxel_size=0.0)) and "voxel_size" in create_error(p=dict(voxel_size=0.0, min_weight=0))


@pytest.mark.parametrize("fn", ["integrate", "raycast"])
def test_argument_checks_without_an_object(fn):
    assert call_error(fn) == "map is NULL"
    assert call_error(fn, w=16384, h=1) == "map is NULL" and call_error(fn, w=1, h=16384) == "map is NULL"
    assert "camera" in call_error(fn, cam=None)
    for name in ("fx", "fy", "baseline"):
        assert name in call_error(fn, cam=dict(CAM, **{name: 0.0}))
    assert "cy" in call_error(fn, cam=dict(CAM, cy=float("nan")))
    assert call_error(fn, pose=None) == "pose is NULL"
    for k, bad in ((0, 2.5), (5, float("nan")), (3, 2e6), (11, -float("inf"))):
        P = list(V.POSE_IDENTITY)
        P[k] = bad
        assert f"pose[{k}]" in call_error(fn, pose=P)
    for kw, word in ((dict(w=0), "width"), (dict(w=16385), "width"), (dict(h=0), "height"), (dict(h=20000), "height")):
        assert word in call_error(fn, **kw)
    # the order: camera before pose before sizes before the object
    assert "camera" in call_error(fn, cam=None, pose=None, w=0)
    assert "pose" in call_error(fn, pose=None, w=0)
    assert "width" in call_error(fn, w=0)


def test_the_host_entry_points_name_their_missing_argument():
    L, lib = _lib()
    o, n, v = (C.c_int64 * 3)(), (C.c_int32 * 3)(), C.c_int(0)
    for rc in (lib.cart_voxel_map_clear(None), lib.cart_voxel_map_window(None, o, n, C.byref(v)), lib.cart_voxel_map_read(None, None, o, None)):
        assert rc != 0 and lib.cart_last_error(None).decode() == "map is NULL"

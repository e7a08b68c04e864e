"""CPU tests of spec S37: colour for the TSDF voxel map.  The numpy restatement tests/np_voxelcolor.py against its own scalar
loops, the spec's hand-worked cases, the properties the spec states (rounding, saturation, the coloured set, the window rule, gray = BGR),
the accuracy of a rendered model image on the corridor of 7.15, and the library's host side without a device."""
import ctypes as C
import math

import numpy as np
import pytest

import np_voxelcolor as K
import np_voxelmap as V
import np_voxelmesh as M
import test_voxelmap_spec as S

SHAPE = (16, 16, 24)                                                          # test_voxelmap_spec's small volume: 2 x 2 x 3 m


def image_for(seed, w=24, h=10, channels=3):
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, 256, (h, w, 3) if channels == 3 else (h, w), dtype=np.uint8)


def pair(max_weight=K.DEFAULT_MAX_WEIGHT, shape=SHAPE, **p):
    m = V.Map(*shape, V.params(**dict(S.SMALL, **p)))
    return m, K.Color(m, max_weight)


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a != b).sum())} values differ"


# ---- the scalar twin ----------------------------------------------------------------------------------------------------------------
CHAINS = {
    "still_gray": ([S.pose_t()] * 3, 1, True),
    "forward_bgr": ([S.pose_t(tz=0.5 * k) for k in range(4)], 3, True),
    "sideways_and_turned": ([S.pose_t(), S.pose_t(tx=1.0), S.yaw_pose(20.0, (1.0, 0.0, 0.25)), S.pose_t(tx=-1.0, ty=-1.0)], 3, False),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_vectorised_restatement_equals_the_scalar_loop(name):
    poses, channels, masked = CHAINS[name]
    (m, vec), (_, sca) = pair(max_weight=3), pair(max_weight=3)
    sca.map = m                                                               # one map under both
    coloured, twice = [], 0
    for k, pose in enumerate(poses):
        disp, mask = S.small_frame(20 + k, masked=masked)
        image = image_for(k, channels=channels)
        m.integrate(S.SMALL_CAM, pose, disp, mask)
        n = vec.integrate(S.SMALL_CAM, pose, disp, image, mask)
        same(n, sca.integrate_scalar(S.SMALL_CAM, pose, disp, image, mask), "counts")
        same(vec.read()[0], sca.read()[0], "volume")
        assert vec.read()[1] == sca.read()[1] == m.origin
        coloured.append(int(n[0]))
        twice = max(twice, int((vec.weight >= 2).sum()))
        ray =m.raycast(S.SMALL_CAM, pose, 24, 10)
        a, b = vec.render(S.SMALL_CAM, pose, ray["disp"]), sca.render_scalar(S.SMALL_CAM, pose, ray["disp"])
        for key in ("image", "alpha", "counts"):
            same(a[key], b[key], key)
        mesh = M.extract(m.tsdf, m.weight, 1, m.p["voxel_size"])
        same(vec.colorize(mesh["vertices"], m.origin), sca.colorize_scalar(mesh["vertices"], m.origin), "vertex colours")
    assert min(coloured) >= 30, coloured
    assert twice >= 10 and a["counts"][0] > 0 and len(mesh["vertices"]) > 10


# ---- the hand-worked cases ----------------------------------------------------------------------------------------------------------
def test_hand_worked_voxel():
    """S33's case (test_voxelmap_spec.test_hand_worked_voxel): voxel (0, 0, 7) of 0.25 m projects to pixel (25, 21) with f = 0.125 /
    0.265625 < 1.  Gray 200 there leaves (200, 200, 200, 1); 101 in a second frame gives (2 (200 + 101) + 2) / 4 = 604 / 4 = 151, weight 2;
    0 in a third gives (2 (2 151 + 0) + 3) / 6 = 607 / 6 = 101, weight 3."""
    disp = np.full((48, 48), 64 * 16, np.int16)
    for scalar in (False, True):
        m = V.Map(32, 32, 64, V.params(voxel_size=0.25))
        c = K.Color(m)
        for value, expect in ((200, (200, 200, 200, 1)), (101, (151, 151, 151, 2)), (0, (101, 101, 101, 3))):
            image = np.full((48, 48), 7, np.uint8)
            image[21, 25] = value
            m.integrate(S.CAM, V.POSE_IDENTITY, disp)
            (c.integrate_scalar if scalar else c.integrate)(S.CAM, V.POSE_IDENTITY, disp, image)
            vox, o = c.read()
            assert tuple(o) == (-16, -16, 0)
            assert tuple(vox[7 - o[2], 0 - o[1], 0 - o[0]]) == expect
    assert 604 // 4 == 151 and 607 // 6 == 101 and 0.125 / 0.265625 < 1.0


def test_hand_worked_sample():
    """Two coloured corners (b = 10, w = 1) and (b = 20, w = 3) and six empty ones: W = 4, b = (2 (10 + 60) + 4) / 8 = 144 / 8 = 18."""
    m, c = pair()
    vox = np.zeros((24, 16, 16), K.VOXEL_RGB_DTYPE)
    vox[5, 4, 3] = (10, 0, 255, 1)
    vox[6, 5, 4] = (20, 0, 255, 3)
    c.write(vox, (8, -8, 16))
    got = c.sample(np.array([11.0]), np.array([-4.0]), np.array([21.0]))[0]
    assert tuple(got) == (18, 0, 255, 4) and c.sample_scalar(11.0, -4.0, 21.0) == (18, 0, 255, 4)
    assert tuple(c.sample(np.array([12.0]), np.array([-4.0]), np.array([21.0]))[0]) == (20, 0, 255, 3)    # the first corner is no longer among the eight
    assert tuple(c.sample(np.array([13.0]), np.array([-4.0]), np.array([21.0]))[0]) == (0, 0, 0, 0)       # W = 0
    # the last i0 with both corners inside is o + N - 2; beyond it, below the origin and at a NaN the sample is empty
    vox[:] = (9, 9, 9, 255)
    c.write(vox, (8, -8, 16))
    assert c.sample_scalar(8.0 + 14, -8.0, 16.0) == (9, 9, 9, 255)            # W = 2040: alpha saturates
    for i0 in ((8.0 + 15, -8.0, 16.0), (7.0, -8.0, 16.0), (8.0, -8.0, 16.0 + 23), (8.0, float("nan"), 16.0)):
        assert c.sample_scalar(*i0) == (0, 0, 0, 0) and tuple(c.sample(*[np.array([v]) for v in i0])[0]) == (0, 0, 0, 0)
    c.clear()
    assert c.sample_scalar(10.0, 0.0, 20.0) == (0, 0, 0, 0)                   # no window


def test_running_average_rounds_half_up_and_the_weight_saturates():
    def step(c, w, obs, max_weight=64):
        return (2 * (w * c + obs) + (w + 1)) // (2 * (w + 1)), min(w + 1, max_weight)
    assert step(0, 0, 200) == (200, 1) and step(200, 1, 101) == (151, 2) and step(151, 2, 0) == (101, 3)
    assert step(100, 1, 101) == (101, 2)                                      # 100.5 rounds up
    assert step(255, 255, 255, 255) == (255, 255) and step(0, 255, 255, 255) == (1, 255)   # 255 / 256 + 1 / 2 rounds to 1
    assert step(7, 1, 9, max_weight=1) == (8, 1)
    m, c = pair(max_weight=2)
    disp, _ = S.small_frame(9, masked=False)
    for k in range(4):
        m.integrate(S.SMALL_CAM, S.pose_t(), disp)
        c.integrate(S.SMALL_CAM, S.pose_t(), disp, image_for(k))
    assert c.read()[0]["weight"].max() == 2


def test_a_constant_image_leaves_exactly_that_colour():
    m, c = pair()
    image = np.empty((10, 24, 3), np.uint8)
    image[:] = (13, 200, 77)
    for k in range(3):
        disp, mask = S.small_frame(30 + k)
        m.integrate(S.SMALL_CAM, S.pose_t(tz=0.125 * k), disp, mask)
        c.integrate(S.SMALL_CAM, S.pose_t(tz=0.125 * k), disp, image, mask)
    vox = c.read()[0]
    on = vox["weight"] > 0
    assert on.sum() > 100 and (vox["weight"] >= 2).sum() > 10
    assert (vox["b"][on] == 13).all() and (vox["g"][on] == 200).all() and (vox["r"][on] == 77).all()
    assert (vox.view(np.uint32)[~on] == 0).all()                              # the empty word
    ray = m.raycast(S.SMALL_CAM, S.pose_t(tz=0.25), 24, 10)
    out = c.render(S.SMALL_CAM, S.pose_t(tz=0.25), ray["disp"])
    seen = out["alpha"] > 0
    assert seen.sum() > 20 and (out["image"][seen] == (13, 200, 77)).all() and (out["image"][~seen] == 0).all()


def test_the_coloured_set_is_the_set_s33_counts_as_near():
    """counts[1] of cart_voxel_map_integrate = the updated voxels with f < 1: on fresh volumes they are the voxels whose colour weight is 1."""
    for seed, pose in ((40, S.pose_t()), (41, S.yaw_pose(15.0, (0.2, 0.0, 0.1)))):
        m, c = pair()
        disp, mask = S.small_frame(seed)
        near = m.integrate(S.SMALL_CAM, pose, disp, mask)[1]
        n = c.integrate(S.SMALL_CAM, pose, disp, image_for(seed), mask)
        assert n[0] == n[1] == near > 30 and (c.weight == 1).sum() == near
        assert ((c.weight == 1) <= (m.weight == 1)).all() and (m.weight == 1).sum() > near   # a subset: free space in front of the band has no colour


def test_a_window_move_keeps_what_stays_and_empties_what_enters():
    m, c = pair()
    disp, _ = S.small_frame(50, masked=False)
    m.integrate(S.SMALL_CAM, S.pose_t(), disp)
    c.integrate(S.SMALL_CAM, S.pose_t(), disp, image_for(50))
    before, o0 = c.read()
    blank = np.full((10, 24), V.INVALID, np.int16)                            # a frame that colours nothing: only the window rule acts
    m.integrate(S.SMALL_CAM, S.pose_t(tx=1.0, tz=1.0), blank)
    assert c.integrate(S.SMALL_CAM, S.pose_t(tx=1.0, tz=1.0), blank, image_for(51)).tolist() == [0, 0]
    after, o1 = c.read()
    assert (o1[0] - o0[0], o1[1] - o0[1], o1[2] - o0[2]) == (8, 0, 8)
    assert after[:-8, :, :-8].tobytes() == before[8:, :, 8:].tobytes() and (before[8:, :, 8:]["weight"] > 0).sum() > 10   # anchored in the world
    assert (after[-8:].view(np.uint32) == 0).all() and (after[:, :, -8:].view(np.uint32) == 0).all()                       # the slabs that entered
    m.integrate(S.SMALL_CAM, S.pose_t(tz=40.0), blank)                         # a jump of >= N: everything is emptied
    c.integrate(S.SMALL_CAM, S.pose_t(tz=40.0), blank, image_for(52))
    assert (c.read()[0].view(np.uint32) == 0).all() and c.read()[1] == m.origin
    fresh = K.Color(V.Map(*SHAPE, V.params(**S.SMALL)))
    with pytest.raises(ValueError, match="no window"):
        fresh.integrate(S.SMALL_CAM, S.pose_t(), disp, image_for(53))


def test_gray_equals_bgr_with_three_equal_channels():
    m, a = pair()
    b = K.Color(m)
    for k in range(2):
        disp, mask = S.small_frame(60 + k)
        gray = image_for(60 + k, channels=1)
        m.integrate(S.SMALL_CAM, S.pose_t(), disp, mask)
        same(a.integrate(S.SMALL_CAM, S.pose_t(), disp, gray, mask), b.integrate(S.SMALL_CAM, S.pose_t(), disp, np.repeat(gray[:, :, None], 3, axis=2), mask), "counts")
    same(a.read()[0], b.read()[0], "volume")
    vox = a.read()[0]
    assert (vox["weight"] >= 2).sum() > 10 and (vox["b"] == vox["g"]).all() and (vox["g"] == vox["r"]).all()


# ---- accuracy of the spec -----------------------------------------------------------------------------------------------------------
def paint(cam, pose, truth):
    """The corridor's paint, a smooth function of the WORLD point p = (X, Y, Z) behind each pixel of the noise-free disparity `truth`:
    b = floor(128 + 100 sin(0.8 X + 0.5 Z) + 0.5), g = floor(128 + 100 sin(1.1 Y + 0.7 Z) + 0.5), r = floor(128 + 100 sin(0.9 Z) + 0.5): periods of
    6 to 12 m, 50 to 100 voxels, so a level changes by at most 100 * 1.3 * 0.125 = 16 per voxel.  Sky pixels are black.  -> uint8 [h, w, 3]."""
    h, w = truth.shape
    ok = truth != V.INVALID
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = np.where(ok, cam["fx"] * cam["baseline"] / (np.where(ok, truth, 16) / 16.0), 0.0)
    X, Y = (x - cam["cx"]) * Z / cam["fx"] + pose[3], (y - cam["cy"]) * Z / cam["fy"] + pose[7]
    Z = Z + pose[11]
    levels = [128 + 100 * np.sin(0.8 * X + 0.5 * Z), 128 + 100 * np.sin(1.1 * Y + 0.7 * Z), 128 + 100 * np.sin(0.9 * Z)]
    return np.where(ok[..., None], np.stack([np.floor(v + 0.5) for v in levels], axis=2), 0).astype(np.uint8)


def corridor_colour_run(step, seed=11, frames=6, w=160, h=64):
    """The frames of test_voxelmap_spec.corridor_run (160 x 64, ACC_CAM, +-1/4 px noise, 10 % fresh holes per frame, a forward step per frame),
    each with the image `paint` gives it, integrated into the map and the colour volume at the defaults; the model is raycast from the last
    pose and rendered behind that model disparity.  -> mean absolute error per channel against the last frame's own image at HIT pixels, and
    the share of HIT pixels with alpha > 0."""
    from cartslam import synth
    truth, _ = synth.road_corridor(w, h, *[S.ACC_CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline")])
    rng = np.random.default_rng(seed)
    ok = truth != V.INVALID
    m = V.Map(*S.ACC_SHAPE)
    c = K.Color(m)
    pose, image = None, None
    for k in range(frames):
        d = truth.copy()
        d[ok] += rng.integers(-4, 5, int(ok.sum())).astype(np.int16)
        d[ok & (rng.random((h, w)) < 0.10)] = V.INVALID
        pose = S.pose_t(tz=step * k)
        image = paint(S.ACC_CAM, pose, truth)
        m.integrate(S.ACC_CAM, pose, d)
        c.integrate(S.ACC_CAM, pose, d, image)
    ray = m.raycast(S.ACC_CAM, pose, w, h)
    out = c.render(S.ACC_CAM, pose, ray["disp"])
    hit = ray["status"] == V.HIT
    both = hit & (out["alpha"] > 0)
    err = np.abs(out["image"].astype(np.int64) - image.astype(np.int64))[both]
    return dict(mae=[float(err[:, k].mean()) for k in range(3)], alpha_percent=100.0 * float(both.sum()) / float(hit.sum()), hits=int(hit.sum()),
                sky=int((out["alpha"][~ok] > 0).sum()))


# forward step (m per frame) -> measured on the restatement at seed 11: mean absolute error of b, g, r at HIT pixels with a colour (levels of
# 255), HIT pixels with alpha > 0 (%)
COLOUR_ACCURACY = {0.0: ((3.72, 5.60, 6.79), 100.0), 0.25: ((3.11, 4.93, 5.60), 100.0), 0.5: ((3.29, 4.89, 5.91), 100.0)}


@pytest.mark.parametrize("step", sorted(COLOUR_ACCURACY))
def test_colour_accuracy_on_the_corridor(step):
    """Measured values: see COLOUR_ACCURACY and DESIGN.md 7.19.  As test_voxelmap_spec.test_accuracy_on_the_corridor, each bound sits at twice
    the measured distance to the ideal (no error, every HIT pixel coloured), so that the measured value lies half-way between the bound and
    the ideal.  The error is the paint's change over the half voxel between a surface point and the voxel centres that hold its colour, plus
    the rounding of the stored bytes."""
    got = corridor_colour_run(step)
    print(step, got)
    mae, percent = COLOUR_ACCURACY[step]
    assert got["hits"] > 3000 and got["sky"] == 0
    for k in range(3):
        assert got["mae"][k] <= 2 * mae[k]
    assert got["alpha_percent"] >= 100.0 - 2 * (100.0 - percent)


# ---- the library's host side --------------------------------------------------------------------------------------------------------
def _lib():
    from cartslam import _lib
    return _lib, _lib.load()


def test_exports_and_layout():
    from cartslam import VOXEL_RGB_DTYPE, VoxelColor, VoxelRgb
    L, lib = _lib()
    for name in ("create", "destroy", "clear", "window", "integrate", "vertices", "render", "read", "write"):
        assert hasattr(lib, "cart_voxel_color_" + name) and "cart_voxel_color_" + name in L.PROTOTYPES
    for name in ("integrate", "colorize", "render", "window", "read", "write", "clear", "close"):
        assert hasattr(VoxelColor, name)
    assert C.sizeof(VoxelRgb) == 4 == VOXEL_RGB_DTYPE.itemsize == K.VOXEL_RGB_DTYPE.itemsize and VOXEL_RGB_DTYPE == K.VOXEL_RGB_DTYPE
    assert [VOXEL_RGB_DTYPE.fields[n][1] for n in ("b", "g", "r", "weight")] == [0, 1, 2, 3]   # b | g << 8 | r << 16 | weight << 24
    assert L.VOXEL_COLOR_DEFAULT_MAX_WEIGHT == K.DEFAULT_MAX_WEIGHT == 64


def test_refusals_before_the_engine():
    """max_weight and channels are checked first: without an engine, a map or a device the message names them."""
    L, lib = _lib()
    out = C.c_void_p()
    for bad in (0, 256, -1):
        assert lib.cart_voxel_color_create(None, None, bad, C.byref(out)) != 0
        assert lib.cart_last_error(None).decode() == "max_weight must be in [1, 255]" and not out.value
    assert lib.cart_voxel_color_create(None, None, 64, C.byref(out)) != 0 and lib.cart_last_error(None).decode() == "bad arguments"
    cam = L.EgoCamera(*[S.CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline")])
    P = (C.c_double * 12)(*V.POSE_IDENTITY)

    def integrate(channels, cam_=C.byref(cam), pose=P, w=16, h=8):
        assert lib.cart_voxel_color_integrate(None, None, cam_, pose, None, 0, None, 0, channels, w, h, None, 0, None, None) != 0
        return lib.cart_last_error(None).decode()

    for bad in (0, 2, 4):
        assert integrate(bad, cam_=None, pose=None, w=0, h=0) == "channels must be 1 or 3"
    assert integrate(1, cam_=None) == "camera is NULL" and "pose" in integrate(3, pose=None) and "width" in integrate(3, w=0)
    assert integrate(1) == "color is NULL" == integrate(3)
    assert lib.cart_voxel_color_render(None, C.byref(cam), P, None, 0, 16, 8, None, 0, None, 0, None, None) != 0
    assert lib.cart_last_error(None).decode() == "color is NULL"
    o = (C.c_int64 * 3)(0, 0, 0)
    assert lib.cart_voxel_color_vertices(None, None, None, 0, o, None, None) != 0 and "max_vertices" in lib.cart_last_error(None).decode()
    assert lib.cart_voxel_color_vertices(None, None, None, 5, None, None, None) != 0 and lib.cart_last_error(None).decode() == "origin3 is NULL"
    o[1] = (1 << 27) + 1
    assert lib.cart_voxel_color_vertices(None, None, None, 5, o, None, None) != 0 and "origin3[1]" in lib.cart_last_error(None).decode()
    o[1] = 12
    assert lib.cart_voxel_color_write(None, None, o, None) != 0 and "origin3[1]" in lib.cart_last_error(None).decode()
    o[1] = 16
    assert lib.cart_voxel_color_write(None, None, o, None) != 0 and lib.cart_last_error(None).decode() == "color is NULL"
    for fn, args in (("clear", ()), ("window", (None, None, None)), ("read", (None, None, None))):
        assert getattr(lib, "cart_voxel_color_" + fn)(None, *args) != 0 and lib.cart_last_error(None).decode() == "color is NULL"
    lib.cart_voxel_color_destroy(None)                                        # a no-op


def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nq = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    props = [l.split()[1:] for l in lines if l.startswith("property") and "list" not in l]
    dt = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    v = np.frombuffer(body, dt, nv)
    f = np.frombuffer(body, np.dtype([("k", "u1"), ("v", "<i4", 4)]), nq, nv * dt.itemsize)
    assert len(body) == nv * dt.itemsize + nq * 17
    return v, f, [name for _, name in props]


def test_write_ply_with_colours_round_trips_and_without_is_unchanged(tmp_path):
    from cartslam import write_ply
    tsdf, weight = np.zeros((8, 8, 8), np.int64), np.ones((8, 8, 8), np.int64)
    tsdf[:] = (np.arange(8)[:, None, None] * 2 - 7) * 1000                    # a plane between z = 3 and z = 4
    mesh = M.extract(tsdf, weight, 1, 0.125)
    n = len(mesh["vertices"])
    assert n == 49 and len(mesh["quads"]) == 36
    rng = np.random.default_rng(3)
    colors = np.frombuffer(rng.integers(0, 256, 4 * n, dtype=np.uint8).tobytes(), K.VOXEL_RGB_DTYPE)
    plain, again, coloured = (str(tmp_path / f) for f in ("plain.ply", "again.ply", "coloured.ply"))
    write_ply(plain, mesh["vertices"], mesh["quads"], (8, -16, 24), 0.125)
    write_ply(again, mesh["vertices"], mesh["quads"], (8, -16, 24), 0.125, colors=None)
    write_ply(coloured, mesh["vertices"], mesh["quads"], (8, -16, 24), 0.125, colors=colors)
    assert open(plain, "rb").read() == open(again, "rb").read()
    v0, f0, names0 = read_ply(plain)
    assert names0 == ["x", "y", "z", "nx", "ny", "nz"] and len(open(plain, "rb").read().split(b"end_header\n", 1)[1]) == 24 * n + 17 * 36
    v1, f1, names1 = read_ply(coloured)
    assert names1 == names0 + ["red", "green", "blue", "alpha"]
    for name in names0:
        assert v1[name].tobytes() == v0[name].tobytes()
    assert f1.tobytes() == f0.tobytes() and (f1["v"] == mesh["quads"]["v"]).all()
    for ply, field in (("red", "r"), ("green", "g"), ("blue", "b"), ("alpha", "weight")):
        assert (v1[ply] == colors[field]).all()
    with pytest.raises(Exception, match="one record per vertex"):
        write_ply(coloured, mesh["vertices"], mesh["quads"], (0, 0, 0), 0.125, colors=colors[:-1])

"""GPU tests of the colour-aided frame-to-model tracking (spec S38): cart_model_track_refine_color against the numpy
restatement tests/np_modeltrack_color.py, the whole 176-byte record byte for byte, on pitched buffers that start at an offset and whose
slack would pass every gate (a three-channel image gets a step that is no multiple of 3).  Beside every byte comparison stands a premise on
the restatement (steps taken, inliers, photometric inliers), so that no comparison passes on an empty case.  The volumes are the small
ones of tests/test_gpu_modeltrack.py; every model a case tracks against is built once and never changed by a test."""
import ctypes as C

import numpy as np
import pytest

import modeltrack_scenes as MS
import np_modeltrack as T
import np_modeltrack_color as TC
import np_voxelcolor as K
import np_voxelmap as V
import test_voxelmap_spec as S
from test_gpu_modeltrack import MODEL_SIZE, SHAPES, START, TRACK, model_frames, valid_points
from test_gpu_voxelcolor import Rows, color_integrate
from test_gpu_voxelmap import SMALL, cam_for, cam_tuple, engine, frame_for, integrate, pitched
from test_modeltrack_color_spec import small_image

pytestmark = pytest.mark.gpu

COLOR_SHAPES = SHAPES + [(513, 2)]           # the column group is one column: 256 sampled columns per trip at every stride


def _torch():
    import torch
    return torch


def coloured(frames, gray=False):
    """model_frames' [(pose, disp, mask)] -> [(pose, disp, mask, image)]"""
    w, h = MODEL_SIZE
    return [(pose, d, mk, small_image(70 + k, w, h, gray)) for k, (pose, d, mk) in enumerate(frames)]


_REFS, _DEVICE = {}, {}
_FRAMES = {"default": lambda: coloured(model_frames()),
           "gray": lambda: coloured(model_frames(), gray=True),
           "three": lambda: coloured(model_frames(3)),
           "seams": lambda: coloured(model_frames(3, base=(2.6, -2.0, -1.5), yaw=25.0), gray=True),
           "flat": lambda: coloured(model_frames(1, flat=True))}
_VOLUME = {"seams": (24, 16, 40)}


def ref_model(key="default"):
    """-> (the restated Map, the restated Color, the frames) with every frame of `key` integrated into both."""
    if key not in _REFS:
        shape = _VOLUME.get(key, (16, 16, 24))
        m = V.Map(*shape, V.params(**SMALL))
        c = K.Color(m)
        cam = cam_for(*MODEL_SIZE)
        frames = _FRAMES[key]()
        for pose, d, mk, im in frames:
            m.integrate(cam, pose, d, mk)
            c.integrate(cam, pose, d, im, mk)
        _REFS[key] = (m, c, frames)
    return _REFS[key]


def device_model(key="default"):
    """-> (the device VoxelMap, its VoxelColor) of ref_model(key)."""
    from cartslam import VoxelColor, VoxelMap, voxel_map_params
    if key not in _DEVICE:
        m, _, frames = ref_model(key)
        obj = VoxelMap(engine(), m.nx, m.ny, m.nz, voxel_map_params(**SMALL))
        col = VoxelColor(engine(), obj)
        cam = cam_for(*MODEL_SIZE)
        for pose, d, mk, im in frames:
            integrate(obj, cam, pose, d, mk, counts=False)
            color_integrate(col, obj, cam, pose, d, im, mk, counts=False)
        _torch().cuda.synchronize()
        _DEVICE[key] = (obj, col)
    return _DEVICE[key]


_OBJ = []


def tracker():
    from cartslam import ModelTrack
    if not _OBJ:
        _OBJ.append(ModelTrack(engine(), 1242, 520))
    return _OBJ[0]


def run(obj, vmap, vcol, cam, p, cp, pose0, disp, image, mask=None, stream=None):
    """cart_model_track_refine_color on pitched inputs that start at an offset and whose slack would pass every gate (a valid disparity in
    range, a white image, a mask label that is not MOVING) -> the device record as a float64 tensor of 22 words."""
    from cartslam import _lib, model_track_color_params, model_track_params
    torch = _torch()
    lib = _lib.load()
    h, w = disp.shape
    channels = 3 if image.ndim == 3 else 1
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d = pitched(disp, 3, 340, 1)                         # 21.25 px: the wall's own disparity
        mk = pitched(mask, 5, 0, 3) if mask is not None else None
        res = torch.full((22,), 77.0, dtype=torch.float64, device="cuda")
    im = Rows(h, channels * w, 4 if (channels * w + 4) % 3 else 5, 2, fill=255, data=image, stream=stream)
    tp, tcp = model_track_params(**p), model_track_color_params(**cp)
    P = (C.c_double * 12)(*[float(v) for v in pose0])
    sp = C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)
    rc = lib.cart_model_track_refine_color(obj._h, vmap._h, vcol._h, C.byref(_lib.EgoCamera(*cam_tuple(cam))), P, C.byref(tp), C.byref(tcp),
                                           C.c_void_p(d.data_ptr()), d.stride(0) * 2, *im.arg(), channels,
                                           C.c_void_p(mk.data_ptr()) if mk is not None else None, mk.stride(0) if mk is not None else 0, w, h,
                                           C.c_void_p(res.data_ptr()), sp)
    assert rc == 0, lib.cart_last_error(None).decode()
    res.keep = (d, mk, im)                                   # the inputs live until the record has been read
    return res


def record(res):
    _torch().cuda.synchronize()
    return res.cpu().numpy().view(TC.RESULT_DTYPE).reshape(-1)


def same(got, exp):
    assert got.tobytes() == exp.tobytes(), f"\n{got}\n{exp}"


def pose_of(rec):
    return T.join(rec["R"][0].tolist(), rec["t"][0].tolist())


def check(key, cam, p, cp, pose0, disp, image, mask=None, exp=None):
    """The device's record of one call on the model `key` against the restatement's (`exp` if the caller has it already) -> that record."""
    if exp is None:
        exp = expected(key, cam, p, cp, pose0, disp, image, mask)
    vmap, vcol = device_model(key)
    same(record(run(tracker(), vmap, vcol, cam, p, cp, pose0, disp, image, mask)), exp)
    return exp


def expected(key, cam, p, cp, pose0, disp, image, mask=None):
    m, c, _ = ref_model(key)
    return TC.refine(m, c, cam, p, cp, pose0, disp, image, mask)


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("w,h", COLOR_SHAPES)
def test_shapes_that_straddle_the_lane_and_row_strides(w, h, stride):
    """Gray frames at odd w + stride, B, G, R frames at even."""
    cam = cam_for(w, h)
    disp, mask = frame_for(w + h, w, h, cam)
    image = small_image(w + h, w, h, gray=(w + stride) % 2 == 1)
    p, cp = T.params(stride=stride, **TRACK), TC.params()
    exp = expected("default", cam, p, cp, START, disp, image, mask)
    if (w, h) == (1, 1) or ((w, h) == (7, 5) and stride > 1):    # from the restatement: one or two candidates, below min_inliers, no step
        assert exp["status"][0] == 0 and exp["steps"][0] == 0 and 1 <= exp["n_candidates"][0] <= 2 and pose_of(exp) == START
    else:
        assert exp["status"][0] == 1 and exp["steps"][0] >= 1 and exp["n_initial"][0] >= 6
        assert exp["n_photo_initial"][0] <= exp["n_initial"][0] and exp["n_photo"][0] <= exp["n_inliers"][0]
        if (w, h) != (3, 257):               # three columns of a tall frame see too little of the model's colours at the start
            assert exp["n_photo_initial"][0] + exp["n_photo"][0] > 0
    check("default", cam, p, cp, START, disp, image, mask, exp=exp)


@pytest.mark.parametrize("gray_frame", [False, True])
def test_a_gray_model_and_windows_off_the_volume_size_with_samples_on_both_sides_of_every_seam(gray_frame):
    """Both windows' origins are no multiple of the volume's size on any axis, so each toroidal storage wraps inside its window on every
    axis; a wall seen under 25 degrees of yaw has known samples, geometric and photometric, on both sides of each seam."""
    m, c, frames = ref_model("seams")
    shape = (m.nx, m.ny, m.nz)
    assert all(o % n for o, n in zip(m.origin, shape)) and c.origin == m.origin
    w, h = MODEL_SIZE
    cam = cam_for(w, h)
    disp, mask = frame_for(9, w, h, cam)
    image = small_image(9, w, h, gray=gray_frame)
    pose0 = MS.perturb(frames[-1][0], (0.02, 0.01, -0.02), -0.6)
    p, cp = T.params(**TRACK), TC.params(photo_gate=1.0)
    exp = expected("seams", cam, p, cp, pose0, disp, image, mask)
    assert exp["status"][0] == 1 and exp["steps"][0] == 4 and exp["n_inliers"][0] > 1000 and exp["n_photo"][0] > 500
    R, t = T.split(pose0)                                                      # the call's first evaluation
    _, _, pin, _, _ = TC.terms(m, c, cam, p, cp, R, t, disp, image, mask)
    assert int(pin.sum()) == exp["n_photo_initial"][0]
    i0 = valid_points(m, cam, pose0, np.where(pin, disp, V.INVALID))           # the photometric inliers are geometric inliers too
    for a in range(3):
        seam = m.origin[a] + shape[a] - m.origin[a] % shape[a]                 # the first global index of the window that is stored at 0
        assert (i0[:, a] < seam - 1).any() and (i0[:, a] >= seam).any() and (i0[:, a] == seam - 1).any(), a   # below, above and across the seam
    check("seams", cam, p, cp, pose0, disp, image, mask, exp=exp)


def test_a_colour_window_that_lags_the_maps_by_one_move():
    """The map integrates a frame one metre ahead that the colour object does not get: the windows differ by 8 voxels on z, and the call
    samples each volume under its own origin."""
    from cartslam import VoxelColor, VoxelMap, voxel_map_params
    m = V.Map(16, 16, 24, V.params(**SMALL))
    c = K.Color(m)
    mcam = cam_for(*MODEL_SIZE)
    frames = coloured(model_frames(3))
    ahead = (S.yaw_pose(2.0, (0.05, 0.0, 1.05)), frames[0][1])
    w, h = 130, 33
    cam = cam_for(w, h)
    disp, mask = frame_for(15, w, h, cam)
    image = small_image(15, w, h)
    p, cp = T.params(**TRACK), TC.params(photo_gate=1.0)
    pose0 = START
    with VoxelMap(engine(), 16, 16, 24, voxel_map_params(**SMALL)) as obj, VoxelColor(engine(), obj) as col:
        for pose, d, mk, im in frames:
            m.integrate(mcam, pose, d, mk)
            c.integrate(mcam, pose, d, im, mk)
            integrate(obj, mcam, pose, d, mk, counts=False)
            color_integrate(col, obj, mcam, pose, d, im, mk, counts=False)
        m.integrate(mcam, *ahead)
        integrate(obj, mcam, *ahead, counts=False)
        assert c.origin[2] + 8 == m.origin[2] and obj.window()[0] == tuple(m.origin) and col.window()[0] == tuple(c.origin)
        exp = TC.refine(m, c, cam, p, cp, pose0, disp, image, mask)
        assert exp["status"][0] == 1 and exp["n_photo"][0] > 100 and exp["n_photo_initial"][0] > 100
        shifted = K.Color(m)
        shifted.c, shifted.weight, shifted.origin = c.c, c.weight, m.origin
        assert TC.refine(m, shifted, cam, p, cp, pose0, disp, image, mask).tobytes() != exp.tobytes()     # the map's indices give another record
        same(record(run(tracker(), obj, col, cam, p, cp, pose0, disp, image, mask)), exp)


def test_colour_corners_below_color_min_weight_and_a_small_photo_gate():
    w, h = 65, 33
    cam = cam_for(w, h)
    disp, mask = frame_for(6, w, h, cam)
    image = small_image(6, w, h)
    p = T.params(**TRACK)
    c = ref_model("three")[1]
    assert 0 < int((c.weight >= 3).sum()) < int((c.weight >= 1).sum())
    loose = expected("three", cam, p, TC.params(photo_gate=1.0), START, disp, image, mask)
    exp = expected("three", cam, p, TC.params(photo_gate=1.0, color_min_weight=3), START, disp, image, mask)
    assert exp["status"][0] == 1 and 0 < exp["n_photo_initial"][0] < loose["n_photo_initial"][0]
    check("three", cam, p, TC.params(photo_gate=1.0, color_min_weight=3), START, disp, image, mask, exp=exp)
    # a gate that drops photometric inliers during the refinement: the count changes between the first and the last evaluation
    cp = TC.params(photo_gate=0.06)
    exp = expected("three", cam, p, cp, START, disp, image, mask)
    assert exp["status"][0] == 1 and exp["steps"][0] == 4 and 0 < exp["n_photo"][0] < exp["n_inliers"][0] and exp["n_photo"][0] != exp["n_photo_initial"][0]
    assert exp["n_photo_initial"][0] < loose["n_photo_initial"][0]
    check("three", cam, p, cp, START, disp, image, mask, exp=exp)


def test_edge_states_empty_colour_no_window_invalid_and_masked_frames():
    from cartslam import VoxelColor, VoxelMap, voxel_map_params
    w, h = 65, 9
    cam = cam_for(w, h)
    disp, mask = frame_for(3, w, h, cam)
    image = small_image(3, w, h)
    p, cp = T.params(**TRACK), TC.params()
    m, c, frames = ref_model("default")
    vmap, vcol = device_model("default")
    mcam = cam_for(*MODEL_SIZE)
    with_colour = expected("default", cam, p, cp, START, disp, image, mask)
    assert with_colour["status"][0] == 1 and with_colour["n_photo"][0] > 0
    s34 = T.refine(m, cam, p, START, disp, mask)
    with VoxelMap(engine(), 16, 16, 24, voxel_map_params(**SMALL)) as fresh, VoxelColor(engine(), fresh) as empty:
        # no map window: the volumes' memory is whatever it is
        none = TC.refine(V.Map(16, 16, 24, V.params(**SMALL)), K.Color(V.Map(16, 16, 24, V.params(**SMALL))), cam, p, cp, START, disp, image, mask)
        assert none["status"][0] == 0 and none["n_candidates"][0] == 0 and pose_of(none) == START and none["cost"][0] == 0.0 == none["rms_photo"][0]
        same(record(run(tracker(), fresh, empty, cam, p, cp, START, disp, image, mask)), none)
        # a map with a window and a colour object that never got a frame: S34's record, no photometric inlier, cost == rms
        for pose, d, mk, _ in frames:
            integrate(fresh, mcam, pose, d, mk, counts=False)
        ec = K.Color(m)
        exp = TC.refine(m, ec, cam, p, cp, START, disp, image, mask)
        assert exp.tobytes()[:136] == s34.tobytes() and exp["n_photo"][0] == 0 == exp["n_photo_initial"][0] and exp["cost"][0] == exp["rms"][0] > 0.0
        same(record(run(tracker(), fresh, empty, cam, p, cp, START, disp, image, mask)), exp)
        # the colour integrated, then cleared: the words are still there, the window is not
        for pose, d, mk, im in frames:
            color_integrate(empty, fresh, mcam, pose, d, im, mk, counts=False)
        same(record(run(tracker(), fresh, empty, cam, p, cp, START, disp, image, mask)), with_colour)
        empty.clear()
        same(record(run(tracker(), fresh, empty, cam, p, cp, START, disp, image, mask)), exp)
        assert not empty.window()[2] and fresh.window()[2]
    # all-invalid and all-masked frames
    none = np.full_like(disp, V.INVALID)
    exp = expected("default", cam, p, cp, START, none, image)
    assert exp["status"][0] == 0 and exp["n_candidates"][0] == 0 and exp["cost"][0] == 0.0 and pose_of(exp) == START
    check("default", cam, p, cp, START, none, image, exp=exp)
    ones = np.ones((h, w), np.uint8)
    exp = expected("default", cam, p, cp, START, disp, image, ones)
    assert exp["status"][0] == 0 and exp["n_candidates"][0] == 0
    check("default", cam, p, cp, START, disp, image, ones, exp=exp)


def test_photo_weight_zero_is_the_geometric_call_on_the_device():
    from cartslam import model_track_params
    w, h = 130, 33
    cam = cam_for(w, h)
    disp, mask = frame_for(16, w, h, cam)
    image = small_image(16, w, h)
    p, cp = T.params(**TRACK), TC.params(photo_weight=0.0)
    exp = check("default", cam, p, cp, START, disp, image, mask)
    s34 = T.refine(ref_model("default")[0], cam, p, START, disp, mask)
    assert exp["status"][0] == 1 and exp.tobytes()[:136] == s34.tobytes() and exp["n_photo"][0] == 0 and exp["cost"][0] == exp["rms"][0]
    vmap, _ = device_model("default")
    got = tracker().refine(vmap, cam_tuple(cam), START, pitched(disp, 3, 340, 1), params=model_track_params(**p), mask=pitched(mask, 5, 0, 3), raw=True)
    _torch().cuda.synchronize()
    assert got.cpu().numpy().tobytes() == exp.tobytes()[:136]                  # cart_model_track_refine's own record on the device
    assert exp.tobytes() != expected("default", cam, p, TC.params(), START, disp, image, mask).tobytes()


@pytest.mark.parametrize("iterations", [0, 1, 16])
def test_iterations(iterations):
    w, h = 96, 40
    cam = cam_for(w, h)
    disp, mask = frame_for(10, w, h, cam)
    image = small_image(10, w, h)
    p, cp = T.params(iterations=iterations, **TRACK), TC.params()
    exp = expected("default", cam, p, cp, START, disp, image, mask)
    assert exp["steps"][0] == iterations and exp["status"][0] == (1 if iterations else 0) and exp["n_photo_initial"][0] > 0
    if iterations == 0:
        assert pose_of(exp) == START and exp["cost"][0] == exp["cost_initial"][0] > 0.0 and exp["n_photo"][0] == exp["n_photo_initial"][0]
    check("default", cam, p, cp, START, disp, image, mask, exp=exp)


def test_stops_on_the_device():
    """Too few inliers, and the pivot stop: without damping and without colour a single fronto-parallel plane leaves H[2][2] = 0 exactly
    (S34's case; photo_weight = 0 here), and the colour term alone makes the system solvable."""
    w, h = 65, 33
    cam = cam_for(w, h)
    disp, mask = frame_for(8, w, h, cam)
    image = small_image(8, w, h)
    p, cp = T.params(min_inliers=w * h + 1), TC.params()
    exp = expected("default", cam, p, cp, START, disp, image, mask)
    assert exp["status"][0] == 0 and exp["n_inliers"][0] == exp["n_initial"][0] > 500 and pose_of(exp) == START and exp["n_photo"][0] == exp["n_photo_initial"][0] > 0
    check("default", cam, p, cp, START, disp, image, mask, exp=exp)
    flat = np.full((h, w), int(cam["fx"] * cam["baseline"] / 1.5 * 16.0), np.int16)
    pose0 = S.pose_t(0.0, 0.0, 0.01)
    for lam, status in ((0.0, 0), (64.0, 1)):
        p, cp = T.params(damping=0.0, **TRACK), TC.params(photo_weight=lam, photo_gate=1.0)
        exp = expected("flat", cam, p, cp, pose0, flat, image)
        assert exp["status"][0] == status and exp["n_inliers"][0] > 500 and exp["rms_initial"][0] > 0.0
        got = check("flat", cam, p, cp, pose0, flat, image)
        assert np.isfinite(got["R"]).all() and np.isfinite(got["t"]).all() and np.isfinite(got["cost"]).all()


def test_back_to_back_calls_the_geometric_call_between_and_a_second_object_on_another_stream():
    from cartslam import ModelTrack, model_track_params
    torch = _torch()
    m, c, _ = ref_model("default")
    vmap, vcol = device_model("default")
    p, cp = T.params(**TRACK), TC.params()
    big_cam, small_cam = cam_for(300, 40), cam_for(33, 7)
    big, small = frame_for(11, 300, 40, big_cam), frame_for(12, 33, 7, small_cam)
    big_im, small_im = small_image(11, 300, 40), small_image(12, 33, 7, gray=True)
    p16 = T.params(iterations=16, **TRACK)
    exp_big = TC.refine(m, c, big_cam, p16, cp, START, big[0], big_im, big[1])
    exp_small = TC.refine(m, c, small_cam, p, cp, START, small[0], small_im, small[1])
    s34_small = T.refine(m, small_cam, p, START, *small)
    assert exp_big["steps"][0] == 16 and exp_small["status"][0] == 1 and exp_small["n_photo"][0] > 0
    with ModelTrack(engine(), 300, 40) as a, ModelTrack(engine(), 300, 40) as b:
        first = run(a, vmap, vcol, big_cam, p16, cp, START, big[0], big_im, big[1])        # back to back on one object, no synchronisation between
        second = run(a, vmap, vcol, small_cam, p, cp, START, small[0], small_im, small[1])
        plain = a.refine(vmap, cam_tuple(small_cam), START, pitched(small[0], 3, 340, 1), params=model_track_params(**p), mask=pitched(small[1], 5, 0, 3), raw=True)
        third = run(a, vmap, vcol, small_cam, p, cp, START, small[0], small_im, small[1])  # after cart_model_track_refine on the same object
        same(record(first), exp_big)
        same(record(second), exp_small)                                                    # the larger call's row partials do not leak
        assert plain.cpu().numpy().tobytes() == s34_small.tobytes()                        # the geometric call is what it was, between two colour calls
        same(record(third), exp_small)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        exp_big4 = TC.refine(m, c, big_cam, p, cp, START, big[0], big_im, big[1])
        outs = []
        for k, (o, s) in enumerate(((a, s1), (b, s2), (b, s1), (a, s2))):
            args = (big_cam, p, cp, START, big[0], big_im, big[1]) if k % 2 else (small_cam, p, cp, START, small[0], small_im, small[1])
            outs.append(run(o, vmap, vcol, *args, stream=s))
        for k, out in enumerate(outs):
            same(record(out), exp_big4 if k % 2 else exp_small)


def test_bad_arguments_touch_no_output():
    torch = _torch()
    from cartslam import VoxelColor, VoxelMap, _lib, model_track_color_params, model_track_params, voxel_map_params
    lib = _lib.load()
    m, c, _ = ref_model("default")
    vmap, vcol = device_model("default")
    w, h = 130, 9
    cam_d = cam_for(w, h)
    disp_h, _ = frame_for(14, w, h, cam_d, masked=False)
    image_h = small_image(14, w, h)
    disp = torch.from_numpy(disp_h).cuda()
    image = torch.from_numpy(image_h).cuda()
    gray = torch.from_numpy(np.ascontiguousarray(image_h[..., 1])).cuda()
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    res = torch.full((22 + 4,), 77.0, dtype=torch.float64, device="cuda")
    cam, p, cp, pose = _lib.EgoCamera(*cam_tuple(cam_d)), model_track_params(**TRACK), model_track_color_params(), (C.c_double * 12)(*START)
    base = dict(disp=(disp.data_ptr(), 2 * w), image=(image.data_ptr(), 3 * w), channels=3, mask=(mask.data_ptr(), w), size=(w, h), result=res.data_ptr(), cp=cp)

    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as other_map, VoxelColor(engine(), other_map) as other_col:
        def call(obj=True, vm=True, vc=True, **kw):
            a = dict(base, **kw)
            col = (a["vc_obj"] if "vc_obj" in a else vcol)._h if vc else None
            rc = lib.cart_model_track_refine_color(tracker()._h if obj else None, vmap._h if vm else None, col, C.byref(cam), pose, C.byref(p), C.byref(a["cp"]),
                                                   C.c_void_p(a["disp"][0]), a["disp"][1], C.c_void_p(a["image"][0]), a["image"][1], a["channels"],
                                                   C.c_void_p(a["mask"][0]), a["mask"][1], *a["size"], C.c_void_p(a["result"]), None)
            return rc, lib.cart_last_error(None).decode()

        bad = [(dict(obj=False), "bad arguments"), (dict(vm=False), "map is NULL"), (dict(vc=False), "color is NULL"), (dict(vc_obj=other_col), "the map's shape is not the colour object's"),
               (dict(cp=model_track_color_params(photo_weight=-1.0)), "photo_weight"), (dict(cp=model_track_color_params(photo_gate=0.0)), "photo_gate"),
               (dict(cp=model_track_color_params(color_min_weight=0)), "color_min_weight"), (dict(cp=model_track_color_params(reserved=3)), "reserved"),
               (dict(channels=2), "channels must be 1 or 3"), (dict(result=None), "result is NULL"), (dict(result=res.data_ptr() + 4), "result must be 8-byte aligned"),
               (dict(size=(1243, h)), "exceeds"), (dict(size=(w, 521)), "exceeds"), (dict(size=(0, h)), "width"), (dict(disp=(None, 2 * w)), "disp is NULL"),
               (dict(image=(None, 3 * w)), "image is NULL"), (dict(disp=(disp.data_ptr() + 1, 2 * w)), "disp"), (dict(disp=(disp.data_ptr(), 2 * w + 1)), "disp"),
               (dict(disp=(disp.data_ptr(), 2 * w - 2)), "disp_step"), (dict(image=(image.data_ptr(), 3 * w - 1)), "image_step"), (dict(image=(gray.data_ptr(), w - 1), channels=1), "image_step"),
               (dict(mask=(mask.data_ptr(), w - 1)), "mask_step"), (dict(result=disp.data_ptr() + 2 * w * (h - 1)), "result and disp must not overlap"),
               (dict(result=image.data_ptr() + 3 * w * (h - 1)), "result and image must not overlap"), (dict(result=mask.data_ptr() + w * (h - 1)), "result and mask must not overlap")]
        for kw, word in bad:
            rc, err = call(**kw)
            assert rc != 0 and word in err, (kw, err)
        torch.cuda.synchronize()
        assert bool((res == 77.0).all())               # no refused call touched the output
        rc, err = call(mask=(None, 0))
        assert rc == 0, err
        torch.cuda.synchronize()
        assert not bool((res[:22] == 77.0).any()) and bool((res[22:] == 77.0).all())
        same(res[:22].cpu().numpy().view(TC.RESULT_DTYPE), TC.refine(m, c, cam_d, T.params(**TRACK), TC.params(), START, disp_h, image_h))
        rc, err = call(mask=(None, 0), image=(gray.data_ptr(), w), channels=1)
        assert rc == 0, err
        torch.cuda.synchronize()
        same(res[:22].cpu().numpy().view(TC.RESULT_DTYPE), TC.refine(m, c, cam_d, T.params(**TRACK), TC.params(), START, disp_h, image_h[..., 1]))


def test_refine_color_through_the_python_object():
    """ModelTrack.refine_color on host arrays and on device tensors, with and without raw."""
    torch = _torch()
    from cartslam import MODEL_TRACK_COLOR_RESULT_DTYPE, EngineError, model_track_color_params, model_track_params
    vmap, vcol = device_model("default")
    w, h = 96, 40
    cam = cam_for(w, h)
    disp, mask = frame_for(17, w, h, cam)
    image = small_image(17, w, h)
    p, cp = T.params(**TRACK), TC.params(photo_weight=16.0)
    exp = expected("default", cam, p, cp, START, disp, image, mask)
    assert exp["status"][0] == 1 and exp["n_photo"][0] > 0
    kw = dict(params=model_track_params(**p), color_params=model_track_color_params(**cp))
    got = tracker().refine_color(vmap, vcol, cam_tuple(cam), START, disp, image, mask=mask, **kw)
    assert got.dtype == MODEL_TRACK_COLOR_RESULT_DTYPE
    same(got, exp)
    raw = tracker().refine_color(vmap, vcol, cam_tuple(cam), START, torch.from_numpy(disp).cuda(), torch.from_numpy(image).cuda(), mask=torch.from_numpy(mask).cuda(), raw=True, **kw)
    same(record(raw), exp)
    same(tracker().refine_color(vmap, vcol, cam_tuple(cam), START, disp, image[..., 1].copy(), mask=mask, **kw), expected("default", cam, p, cp, START, disp, image[..., 1], mask))
    with pytest.raises(EngineError, match="image"):
        tracker().refine_color(vmap, vcol, cam_tuple(cam), START, disp, image[:-1], mask=mask, **kw)


# ---- the C++ frame loop ------------------------------------------------------------------------------------------------------------
def test_voxel_map_module_tracks_with_colour_in_the_frame_loop(tmp_path):
    """cart_slam_amd over four synthetic frames with "track", "color" and "track_color" against the chain of restatements np_ego ->
    np_modeltrack_color -> np_voxelmap -> np_voxelcolor: every frame is tracked against both volumes as the earlier frames left them, with
    its own reference image, before its geometry and colour integrates.  <id>_model_track_color.bin is the device record, <id>_model_pose.bin
    its first 136 bytes and the pose the cost rule took, and both volumes are the restated ones after every frame.  With "track_color"
    false every dump equals the run without the key, and no model_track_color file appears."""
    import json
    import os

    import np_ego as E
    import oracle_lib as O
    from test_gpu_ego import restated_frames
    from test_gpu_matches import noise_frame, noise_world
    from test_gpu_voxelmap import read_dump
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n, w, h = 4, 320, 96
    world = noise_world(79)
    images = [noise_frame(world, f) for f in range(n)]
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for side in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, side))
    for f, (l, r) in enumerate(images):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    # test_gpu_modeltrack's scene: a textured plane at 6 px of disparity, 25 m away, half-metre voxels
    vp = dict(voxel_size=0.5, min_disparity=3.5, max_depth=40.0, truncation=1.0, march_step=0.5, lookahead=16.0, max_weight=3)
    tp = dict(iterations=3, stride=2, min_inliers=500, damping=0.05)
    tcp = dict(photo_weight=64.0, photo_gate=0.25, color_min_weight=1)              # the defaults, spelled out
    shape = dict(cells_x=64, cells_y=16, cells_z=64)
    head = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
            {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion")]
    ecam, vcam = E.camera(**keys), V.camera(**keys)
    feats, stereo, temporal = restated_frames(images, 5000)
    lms = [E.triangulate(ecam, feats[f][0][0], feats[f][1][0], stereo[f]) for f in range(n)]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    module = dict(keys, type="voxel_map", track=True, color=True, **shape, **vp, **tp)
    r = run_exe(src, head + [dict(module, track_color=True, **tcp)], tmp, ("--dump", d), env={"CARTSLAM_VOXEL_MAP_SNAPSHOT": "1"})
    assert r.returncode == 0, r.stderr
    ref = V.Map(64, 16, 64, V.params(**vp))
    cref = K.Color(ref)
    p, cp = T.params(**tp), TC.params(**tcp)
    tracked, ego_pose, taken, photo = None, list(E.POSE_IDENTITY), 0, 0
    for f in range(n):
        l, rr = images[f]
        disp = O.disparity_module(l, rr, 64, 8, 4, radius=2, iterations=1)
        res = E.estimate(ecam, E.params(), lms[f], feats[f][0][0], lms[max(f - 1, 0)], temporal[f], 0, f + 1)[0]
        ego_pose = E.chain(ego_pose, res)
        pred = list(ego_pose) if tracked is None else list(E.chain(tracked, res))
        exp = TC.refine(ref, cref, vcam, p, cp, pred, disp, l)                 # before this frame's integrates
        took, tracked = TC.accept(exp, pred, p)
        taken += took
        photo += int(exp["n_photo"][0]) > 0
        raw = open(os.path.join(d, f"{f + 1}_model_track_color.bin"), "rb").read()
        assert len(raw) == 176
        same(np.frombuffer(raw, TC.RESULT_DTYPE, 1), exp)
        raw = open(os.path.join(d, f"{f + 1}_model_pose.bin"), "rb").read()
        assert len(raw) == 136 + 96 and raw[:136] == exp.tobytes()[:136]
        assert raw[136:] == np.array(tracked, np.float64).tobytes(), f"frame {f + 1}: the tracked pose"
        rn = ref.integrate(vcam, tracked, disp)
        cref.integrate(vcam, tracked, disp, l)
        got = read_dump(os.path.join(d, f"{f + 1}_voxel_map.bin"), w, h)
        assert got["origin"] == ref.origin and got["counts"].tobytes() == rn.tobytes(), f"frame {f + 1}: counts"
        assert open(os.path.join(d, f"{f + 1}_voxel_map_voxels.bin"), "rb").read() == ref.read()[0].tobytes(), f"frame {f + 1}: voxels"
        raw = open(os.path.join(d, f"{f + 1}_voxel_color_voxels.bin"), "rb").read()
        assert raw[:24] == np.array(cref.origin, np.int64).tobytes() and raw[24:] == cref.read()[0].tobytes(), f"frame {f + 1}: colour voxels"
    assert taken >= 2 and photo >= 2                   # refinements were accepted, and the photometric term had inliers

    # "track_color": false is the run without the key, byte for byte, and publishes no colour record
    dumps = {}
    for name, extra in (("off", dict(track_color=False, **tcp)), ("absent", {})):
        dumps[name] = os.path.join(tmp, "dump_" + name)
        os.makedirs(dumps[name])
        r = run_exe(src, head + [dict(module, **extra)], tmp, ("--dump", dumps[name]), env={"CARTSLAM_VOXEL_MAP_SNAPSHOT": "1"})
        assert r.returncode == 0, r.stderr
    files = sorted(os.listdir(dumps["absent"]))
    assert files == sorted(os.listdir(dumps["off"])) and len(files) >= 4 * n and not [k for k in files if "model_track_color" in k]
    assert [k for k in files if "model_pose" in k]
    for k in files:
        assert open(os.path.join(dumps["off"], k), "rb").read() == open(os.path.join(dumps["absent"], k), "rb").read(), k

    # configuration errors name their key
    for bad, word in ((dict(module, track_color=True, photo_weight=-1.0), "photo_weight"), (dict(module, track_color=True, photo_gate=0.0), "photo_gate"),
                      (dict(module, track_color=True, color_min_weight=0), "color_min_weight"), (dict(module, track_color=True, color=False), "track_color"),
                      (dict(module, track_color=True, track=False), "track_color")):
        r = run_exe(src, head + [bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)

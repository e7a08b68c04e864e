"""GPU tests of the frame-to-model pose tracking (spec S34): cart_model_track_refine against the numpy restatement
tests/np_modeltrack.py, the whole result record byte for byte, on pitched buffers that start at an offset and whose slack would pass every
gate.  Beside every byte comparison stands a premise on the restatement (steps taken, inliers, status), so that no comparison passes on an
empty case.  The volumes are the small ones of tests/test_gpu_voxelmap.py; the model every case tracks against is built once."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import modeltrack_scenes as MS
import np_modeltrack as T
import np_voxelmap as V
import test_voxelmap_spec as S
from test_gpu_voxelmap import SMALL, cam_for, cam_tuple, engine, frame_for, integrate, pitched

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (255, 3), (256, 2), (257, 2), (1025, 2), (3, 257), (40, 513)]   # width x height: the lane, column-group and row strides
MODEL_SIZE = (130, 70)                       # the frames the model is built from: a frustum a few pixels thin leaves no sample with eight known corners
TRACK = dict(min_inliers=6)
BASE = S.pose_t(0.02, 0.0, 0.03)
START = MS.perturb(BASE, (0.02, -0.01, 0.03), 0.5)


def _torch():
    import torch
    return torch


def model_frames(n=2, base=(0.0, 0.0, 0.0), yaw=0.0, flat=False):
    """[(pose, disp, mask)] of n frames of MODEL_SIZE: a wall at 1.5 m with a step (test_voxelmap_spec.small_frame), or flat and noise-free."""
    w, h = MODEL_SIZE
    cam = cam_for(w, h)
    out = []
    for k in range(n):
        pose = S.yaw_pose(yaw, (base[0] + 0.02 * k, base[1], base[2] + 0.03 * k))
        if flat:
            d = np.full((h, w), int(cam["fx"] * cam["baseline"] / 1.5 * 16.0), np.int16)
        else:
            d, _ = frame_for(40 + k, w, h, cam, masked=False)
        out.append((pose, d, None))
    return out


_MODELS = {}


def model(shape=(16, 16, 24), frames_key="default", frames=None, **mp):
    """-> (the restated Map, the device VoxelMap) with `frames` integrated; built once per key and never changed by a test."""
    from cartslam import VoxelMap, voxel_map_params
    key = (shape, frames_key, tuple(sorted(mp.items())))
    if key not in _MODELS:
        p = dict(SMALL, **mp)
        ref = V.Map(*shape, V.params(**p))
        obj = VoxelMap(engine(), *shape, voxel_map_params(**p))
        cam = cam_for(*MODEL_SIZE)
        for pose, d, mk in (frames if frames is not None else model_frames()):
            ref.integrate(cam, pose, d, mk)
            integrate(obj, cam, pose, d, mk, counts=False)
        _torch().cuda.synchronize()
        _MODELS[key] = (ref, obj)
    return _MODELS[key]


_OBJ = []


def tracker():
    from cartslam import ModelTrack
    if not _OBJ:
        _OBJ.append(ModelTrack(engine(), 1242, 520))
    return _OBJ[0]


def run(obj, vmap, cam, p, pose0, disp, mask=None, stream=None):
    """cart_model_track_refine through ModelTrack.refine on pitched inputs that start at an offset and whose slack would pass every gate
    (a valid disparity in range, a mask label that is not MOVING) -> the device record."""
    from cartslam import model_track_params
    torch = _torch()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d = pitched(disp, 3, 340, 1)                         # 21.25 px: the wall's own disparity
        mk = pitched(mask, 5, 0, 3) if mask is not None else None
    return obj.refine(vmap, cam_tuple(cam), pose0, d, params=model_track_params(**p), mask=mk, stream=stream, raw=True)


def record(res):
    _torch().cuda.synchronize()
    return res.cpu().numpy().view(T.RESULT_DTYPE).reshape(-1)


def same(got, exp):
    assert got.tobytes() == exp.tobytes(), f"\n{got}\n{exp}"


def pose_of(rec):
    return T.join(rec["R"][0].tolist(), rec["t"][0].tolist())


def valid_points(ref, cam, pose, disp):
    """(i0 [n, 3] of every pixel that passes the pixel gates, as floats) for the premises about the window: plain numpy, not bit-critical."""
    s = disp.astype(np.float64)
    y, x = np.mgrid[0:disp.shape[0], 0:disp.shape[1]]
    with np.errstate(all="ignore"):
        Z = cam["fx"] * cam["baseline"] / (s / 16.0)
    ok = (disp != V.INVALID) & (s / 16.0 >= ref.p["min_disparity"]) & (Z >= ref.p["min_depth"]) & (Z <= ref.p["max_depth"])
    pc = np.stack([(x - cam["cx"]) * Z / cam["fx"], (y - cam["cy"]) * Z / cam["fy"], Z], -1)[ok]
    M = np.asarray(pose, np.float64).reshape(3, 4)
    pw = pc @ M[:, :3].T + M[:, 3]
    return np.floor(pw / ref.p["voxel_size"] - 0.5)


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_that_straddle_the_lane_and_row_strides(w, h, stride):
    ref, vmap = model()
    cam = cam_for(w, h)
    disp, mask = frame_for(w + h, w, h, cam)
    p = T.params(stride=stride, **TRACK)
    exp = T.refine(ref, cam, p, START, disp, mask)
    sampled = ((w + stride - 1) // stride) * ((h + stride - 1) // stride)
    if (w, h) == (1, 1) or ((w, h) == (7, 5) and stride > 1):    # from the restatement: one or two candidates, below min_inliers, no step
        assert exp["status"][0] == 0 and exp["steps"][0] == 0 and 1 <= exp["n_candidates"][0] <= 2 and pose_of(exp) == START
    else:                    # every other shape takes its four steps at every stride (7 x 5 at stride 1 on eight candidates)
        assert exp["status"][0] == 1 and exp["steps"][0] == 4 and exp["n_inliers"][0] >= 6 and exp["n_initial"][0] >= 6
        assert exp["n_candidates"][0] < sampled                                  # holes, sub-minimum pixels and the MOVING block left
    same(record(run(tracker(), vmap, cam, p, START, disp, mask)), exp)


def test_a_window_off_the_volume_size_with_samples_on_both_sides_of_every_seam():
    """The window's origin is no multiple of the volume's size on any axis, so the toroidal storage wraps inside the window on every axis;
    a wall seen under 25 degrees of yaw has known samples on both sides of each seam."""
    shape = (24, 16, 40)
    base = (2.6, -2.0, -1.5)
    frames = model_frames(3, base=base, yaw=25.0)
    ref, vmap = model(shape, "seams", frames)
    assert all(o % n for o, n in zip(ref.origin, shape)), ref.origin
    w, h = MODEL_SIZE
    cam = cam_for(w, h)
    disp, mask = frame_for(9, w, h, cam)
    pose0 = MS.perturb(frames[-1][0], (0.02, 0.01, -0.02), -0.6)
    p = T.params(**TRACK)
    exp = T.refine(ref, cam, p, pose0, disp, mask)
    assert exp["status"][0] == 1 and exp["steps"][0] == 4 and exp["n_inliers"][0] > 1000
    R, t = T.split(pose_of(exp))
    cand, _, _ = T.terms(ref, cam, p, R, t, disp, mask)
    i0 = valid_points(ref, cam, pose_of(exp), np.where(cand, disp, V.INVALID))
    for a in range(3):
        seam = ref.origin[a] + shape[a] - ref.origin[a] % shape[a]             # the first global index of the window that is stored at 0
        assert (i0[:, a] < seam - 1).any() and (i0[:, a] >= seam).any() and (i0[:, a] == seam - 1).any(), a   # below, above and across the seam
    same(record(run(tracker(), vmap, cam, p, pose0, disp, mask)), exp)


def test_no_window_and_a_cleared_map():
    from cartslam import VoxelMap, voxel_map_params
    w, h = 65, 9
    cam = cam_for(w, h)
    disp, mask = frame_for(3, w, h, cam)
    p = T.params(**TRACK)
    ref = V.Map(16, 16, 24, V.params(**SMALL))
    exp = T.refine(ref, cam, p, START, disp, mask)
    assert exp["status"][0] == 0 and exp["n_candidates"][0] == 0 and pose_of(exp) == START and exp["rms"][0] == 0.0
    with VoxelMap(engine(), 16, 16, 24, voxel_map_params(**SMALL)) as fresh:
        same(record(run(tracker(), fresh, cam, p, START, disp, mask)), exp)       # never integrated: the volume's memory is whatever it is
        mcam = cam_for(*MODEL_SIZE)
        for pose, d, mk in model_frames():
            integrate(fresh, mcam, pose, d, mk, counts=False)
        with_model = T.refine(model()[0], cam, p, START, disp, mask)
        assert with_model["status"][0] == 1 and with_model["n_candidates"][0] > 100
        same(record(run(tracker(), fresh, cam, p, START, disp, mask)), with_model)
        assert fresh.window()[2]
        fresh.clear()
        same(record(run(tracker(), fresh, cam, p, START, disp, mask)), exp)       # the voxels are still there, the window is not
        assert not fresh.window()[2]                                               # and the call did not bring one back


def test_all_invalid_and_all_masked():
    ref, vmap = model()
    w, h = 130, 9
    cam = cam_for(w, h)
    disp, _ = frame_for(4, w, h, cam, masked=False)
    p = T.params(**TRACK)
    none = np.full_like(disp, V.INVALID)
    exp = T.refine(ref, cam, p, START, none)
    assert exp["status"][0] == 0 and exp["n_candidates"][0] == 0 and exp["rms"][0] == 0.0 and pose_of(exp) == START
    same(record(run(tracker(), vmap, cam, p, START, none)), exp)
    ones = np.ones((h, w), np.uint8)
    exp = T.refine(ref, cam, p, START, disp, ones)
    assert exp["status"][0] == 0 and exp["n_candidates"][0] == 0
    same(record(run(tracker(), vmap, cam, p, START, disp, ones)), exp)
    some = (np.random.default_rng(4).integers(0, 3, (h, w))).astype(np.uint8)          # all three labels: only 1 leaves
    exp = T.refine(ref, cam, p, START, disp, some)
    plain = T.refine(ref, cam, p, START, disp)
    assert exp["status"][0] == 1 and 0 < exp["n_candidates"][0] < plain["n_candidates"][0] and exp.tobytes() != plain.tobytes()
    same(record(run(tracker(), vmap, cam, p, START, disp, some)), exp)
    same(record(run(tracker(), vmap, cam, p, START, disp)), plain)


@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_points_leave_the_window_on_every_side(sign):
    """A start pose well off on every axis, towards the low or the high faces, and depths from 0.3 to 2.9 m that fill the frustum: pixels that
    pass the pixel gates fall outside on that side of every axis, others are candidates.  Towards the high faces the refinement walks out of
    the known space (three steps, then no candidate is left): whatever the spec gives, the device gives."""
    ref, vmap = model()
    w, h = MODEL_SIZE
    cam = cam_for(w, h)
    rng = np.random.default_rng(12)
    disp = np.round(cam["fx"] * cam["baseline"] / rng.uniform(0.3, 2.9, (h, w)) * 16.0).astype(np.int16)
    pose0 = MS.perturb(BASE, (-0.7, -0.7, -1.5) if sign < 0 else (0.5, 0.5, 0.9), 3.0 * sign)
    p = T.params(**TRACK)
    exp = T.refine(ref, cam, p, pose0, disp)
    i0 = valid_points(ref, cam, pose0, disp)
    o, n = ref.origin, (ref.nx, ref.ny, ref.nz)
    for a in range(3):
        out = i0[:, a] < o[a] if sign < 0 else i0[:, a] > o[a] + n[a] - 2
        assert out.any() and not out.all(), (a, sign)
    assert 6 <= exp["n_initial"][0] < len(i0) and exp["steps"][0] >= 3 and np.isfinite(exp["rms"][0])
    assert (exp["n_candidates"][0] > 100) == (sign < 0)
    same(record(run(tracker(), vmap, cam, p, pose0, disp)), exp)


def test_min_weight_above_some_voxels_weight():
    frames = model_frames(3)
    ref1, _ = model((16, 16, 24), "three", frames)
    ref2, vmap2 = model((16, 16, 24), "three", frames, min_weight=2)
    assert 0 < int((ref2.weight >= 2).sum()) < int((ref2.weight >= 1).sum())
    w, h = 65, 33
    cam = cam_for(w, h)
    disp, mask = frame_for(6, w, h, cam)
    p = T.params(**TRACK)
    exp, loose = T.refine(ref2, cam, p, START, disp, mask), T.refine(ref1, cam, p, START, disp, mask)
    assert exp["status"][0] == 1 and 6 <= exp["n_candidates"][0] < loose["n_candidates"][0]
    same(record(run(tracker(), vmap2, cam, p, START, disp, mask)), exp)


def test_a_small_residual_gate_drops_inliers_during_the_refinement():
    ref, vmap = model()
    w, h = 65, 33
    cam = cam_for(w, h)
    disp, mask = frame_for(7, w, h, cam)
    p = T.params(residual_gate=0.2, **TRACK)
    exp = T.refine(ref, cam, p, START, disp, mask)
    assert exp["status"][0] == 1 and exp["steps"][0] == 4 and 6 <= exp["n_inliers"][0] < exp["n_candidates"][0] and exp["n_inliers"][0] != exp["n_initial"][0]
    same(record(run(tracker(), vmap, cam, p, START, disp, mask)), exp)


def test_stops_on_the_device():
    """Too few inliers, and the pivot stop: without damping a single fronto-parallel plane leaves H[2][2] = 0 exactly (the volume varies along z
    only, so g_x = g_y = 0 and J_2 = 0), the Cholesky stops at its third pivot and the record stays finite with status 0."""
    ref, vmap = model()
    w, h = 65, 33
    cam = cam_for(w, h)
    disp, mask = frame_for(8, w, h, cam)
    p = T.params(min_inliers=w * h + 1)
    exp = T.refine(ref, cam, p, START, disp, mask)
    assert exp["status"][0] == 0 and exp["n_inliers"][0] == exp["n_initial"][0] > 500 and pose_of(exp) == START
    same(record(run(tracker(), vmap, cam, p, START, disp, mask)), exp)
    flat_ref, flat_map = model((16, 16, 24), "flat", model_frames(1, flat=True))
    flat = np.full((h, w), int(cam["fx"] * cam["baseline"] / 1.5 * 16.0), np.int16)
    pose0 = S.pose_t(0.0, 0.0, 0.01)
    for damping, status in ((0.0, 0), (0.01, 1)):
        p = T.params(damping=damping, **TRACK)
        exp = T.refine(flat_ref, cam, p, pose0, flat)
        assert exp["status"][0] == status and exp["n_inliers"][0] > 500 and exp["rms_initial"][0] > 0.0
        got = record(run(tracker(), flat_map, cam, p, pose0, flat))
        same(got, exp)
        assert np.isfinite(got["R"]).all() and np.isfinite(got["t"]).all() and np.isfinite(got["rms"]).all()
    assert pose_of(T.refine(flat_ref, cam, T.params(damping=0.0, **TRACK), pose0, flat)) == pose0


@pytest.mark.parametrize("iterations", [0, 1, 16])
def test_iterations(iterations):
    ref, vmap = model()
    w, h = 96, 40
    cam = cam_for(w, h)
    disp, mask = frame_for(10, w, h, cam)
    p = T.params(iterations=iterations, **TRACK)
    exp = T.refine(ref, cam, p, START, disp, mask)
    assert exp["steps"][0] == iterations and exp["status"][0] == (1 if iterations else 0)
    if iterations == 0:
        assert pose_of(exp) == START and exp["rms"][0] == exp["rms_initial"][0] > 0.0
    same(record(run(tracker(), vmap, cam, p, START, disp, mask)), exp)


def test_back_to_back_calls_a_stale_workspace_and_a_second_object_on_another_stream():
    from cartslam import EngineError, ModelTrack
    torch = _torch()
    ref, vmap = model()
    p = T.params(**TRACK)
    big_cam, small_cam = cam_for(300, 40), cam_for(33, 7)
    big, small = frame_for(11, 300, 40, big_cam), frame_for(12, 33, 7, small_cam)
    exp_big = T.refine(ref, big_cam, T.params(iterations=16, **TRACK), START, *big)
    exp_small = T.refine(ref, small_cam, p, START, *small)
    assert exp_big["steps"][0] == 16 and exp_small["status"][0] == 1
    with ModelTrack(engine(), 300, 40) as a, ModelTrack(engine(), 300, 40) as b:
        first = run(a, vmap, big_cam, T.params(iterations=16, **TRACK), START, *big)        # back to back on one object, no synchronisation between
        second = run(a, vmap, small_cam, p, START, *small)
        same(record(first), exp_big)
        same(record(second), exp_small)                                                     # the larger call's row partials do not leak
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        outs = [run(o, vmap, big_cam if k % 2 else small_cam, p, START, *(big if k % 2 else small), stream=s) for k, (o, s) in enumerate(((a, s1), (b, s2), (b, s1), (a, s2)))]
        exp_big4 = T.refine(ref, big_cam, p, START, *big)
        for k, out in enumerate(outs):
            same(record(out), exp_big4 if k % 2 else exp_small)
        wide = frame_for(13, 301, 8, cam_for(301, 8))
        with pytest.raises(EngineError, match="exceeds"):
            run(a, vmap, cam_for(301, 8), p, START, *wide)


def test_bad_arguments_touch_no_output():
    torch = _torch()
    from cartslam import _lib, model_track_params
    lib = _lib.load()
    ref, vmap = model()
    w, h = 130, 9
    cam_d = cam_for(w, h)
    disp, _ = frame_for(14, w, h, cam_d, masked=False)
    disp = torch.from_numpy(disp).cuda()
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    res = torch.full((17 + 4,), 77.0, dtype=torch.float64, device="cuda")
    cam, p, pose = _lib.EgoCamera(*cam_tuple(cam_d)), model_track_params(**TRACK), (C.c_double * 12)(*START)
    base = dict(disp=(disp.data_ptr(), 2 * w), mask=(mask.data_ptr(), w), size=(w, h), result=res.data_ptr())

    def call(obj=True, vm=True, **kw):
        a = dict(base, **kw)
        flat = []
        for k in ("disp", "mask"):
            flat += [C.c_void_p(a[k][0]), a[k][1]]
        rc = lib.cart_model_track_refine(tracker()._h if obj else None, vmap._h if vm else None, C.byref(cam), pose, C.byref(p), *flat, *a["size"], C.c_void_p(a["result"]), None)
        return rc, lib.cart_last_error(None).decode()

    bad = [(dict(obj=False), "bad arguments"), (dict(vm=False), "map is NULL"), (dict(result=None), "result"), (dict(result=res.data_ptr() + 4), "result must be 8-byte aligned"),
           (dict(size=(1243, h)), "exceeds"), (dict(size=(w, 521)), "exceeds"), (dict(size=(0, h)), "width"), (dict(disp=(None, 2 * w)), "disp is NULL"),
           (dict(disp=(disp.data_ptr() + 1, 2 * w)), "disp"), (dict(disp=(disp.data_ptr(), 2 * w + 1)), "disp"), (dict(disp=(disp.data_ptr(), 2 * w - 2)), "disp_step"),
           (dict(mask=(mask.data_ptr(), w - 1)), "mask_step"), (dict(result=disp.data_ptr() + 2 * w * (h - 1)), "result and disp must not overlap"),
           (dict(result=mask.data_ptr() + w * (h - 1)), "result and mask must not overlap")]
    for kw, word in bad:
        rc, err = call(**kw)
        assert rc != 0 and word in err, (kw, err)
    torch.cuda.synchronize()
    assert bool((res == 77.0).all())               # no refused call touched the output
    rc, err = call(mask=(None, 0))
    assert rc == 0, err
    torch.cuda.synchronize()
    assert not bool((res[:17] == 77.0).any()) and bool((res[17:] == 77.0).all())
    got = res[:17].cpu().numpy().view(T.RESULT_DTYPE)
    same(got, T.refine(ref, cam_d, T.params(**TRACK), START, disp.cpu().numpy()))


# ---- the C++ frame loop ------------------------------------------------------------------------------------------------------------
def test_voxel_map_module_tracks_in_the_frame_loop(tmp_path):
    """cart_slam_amd over four synthetic frames with "track": true against the chain of restatements np_ego -> np_modeltrack -> np_voxelmap:
    <id>_model_pose.bin (the device record, then the tracked pose), the volume integrated and raycast at the tracked pose, and a plane_map fed
    "model_pose".  The same run with "track" off: every dump equals the run without the key, and no model_pose file appears."""
    import np_ego as E
    import np_planemap as PM
    import oracle_lib as O
    from test_gpu_ego import restated_frames
    from test_gpu_matches import noise_frame, noise_world
    from test_gpu_planemap import check_dump
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
    static = {"type": "static", "horizontal_range_min": 6, "horizontal_range_max": 18, "vertical_range_min": -5, "vertical_range_max": 6}
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    # test_gpu_voxelmap's scene: a textured plane at 6 px of disparity, 25 m away, half-metre voxels
    vp = dict(voxel_size=0.5, min_disparity=3.5, max_depth=40.0, truncation=1.0, march_step=0.5, lookahead=16.0, max_weight=3)
    tp = dict(iterations=3, stride=2, min_inliers=500, damping=0.05)
    shape = dict(cells_x=64, cells_y=16, cells_z=64)
    grid = dict(cells_x=64, cells_z=64, cell_size=1.0, max_depth=40.0, max_lateral=30.0)
    head = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
            {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion"), {"type": "disparity_planeseg", "parameter_provider": static}]
    ecam, vcam = E.camera(**keys), V.camera(**keys)
    feats, stereo, temporal = restated_frames(images, 5000)
    lms = [E.triangulate(ecam, feats[f][0][0], feats[f][1][0], stereo[f]) for f in range(n)]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, head + [dict(keys, type="voxel_map", track=True, **shape, **vp, **tp), dict(keys, type="plane_map", pose_key="model_pose", **grid)], tmp, ("--dump", d),
                env={"CARTSLAM_VOXEL_MAP_SNAPSHOT": "1"})
    assert r.returncode == 0, r.stderr
    ref = V.Map(64, 16, 64, V.params(**vp))
    ref_map = PM.Map(PM.camera(**keys), 64, 64, PM.params(cell_size=1.0, max_depth=40.0, max_lateral=30.0))
    p = T.params(**tp)
    tracked, ego_pose, taken, moved = None, list(E.POSE_IDENTITY), 0, 0
    for f in range(n):
        l, rr = images[f]
        disp = O.disparity_module(l, rr, 64, 8, 4, radius=2, iterations=1)
        planes = O.classify(O.plane_derivative(disp)[0], (6, 18, -5, 6, 12, 0))
        res = E.estimate(ecam, E.params(), lms[f], feats[f][0][0], lms[max(f - 1, 0)], temporal[f], 0, f + 1)[0]
        ego_pose = E.chain(ego_pose, res)
        pred = list(ego_pose) if tracked is None else list(E.chain(tracked, res))
        exp = T.refine(ref, vcam, p, pred, disp)
        took, tracked = T.accept(exp, pred, p)
        taken += took
        moved += tracked != list(ego_pose)
        raw = open(os.path.join(d, f"{f + 1}_model_pose.bin"), "rb").read()
        assert len(raw) == 136 + 96
        same(np.frombuffer(raw, T.RESULT_DTYPE, 1), exp)
        assert raw[136:] == np.array(tracked, np.float64).tobytes(), f"frame {f + 1}: the tracked pose"
        rn = ref.integrate(vcam, tracked, disp)
        ray = ref.raycast(vcam, tracked, w, h)
        got = read_dump(os.path.join(d, f"{f + 1}_voxel_map.bin"), w, h)
        assert got["origin"] == ref.origin and got["counts"].tobytes() == rn.tobytes() and got["rays"].tobytes() == ray["counts"].tobytes(), f"frame {f + 1}: counts"
        assert got["disp"].tobytes() == ray["disp"].tobytes() and got["status"].tobytes() == ray["status"].tobytes(), f"frame {f + 1}: model"
        assert open(os.path.join(d, f"{f + 1}_voxel_map_voxels.bin"), "rb").read() == ref.read()[0].tobytes(), f"frame {f + 1}: voxels"
        ref_map.update(disp, planes, tracked)
        check_dump(os.path.join(d, f"{f + 1}_plane_map.bin"), ref_map, 3, 50)
    assert taken >= 2 and moved >= 2                   # refinements were accepted, and the tracked chain left ego_motion's

    # "track": false is the run without the key, byte for byte, and publishes no model_pose
    dumps = {}
    for name, extra in (("off", dict(track=False, **tp)), ("absent", {})):
        dumps[name] = os.path.join(tmp, "dump_" + name)
        os.makedirs(dumps[name])
        r = run_exe(src, head + [dict(keys, type="voxel_map", **shape, **vp, **extra)], tmp, ("--dump", dumps[name]), env={"CARTSLAM_VOXEL_MAP_SNAPSHOT": "1"})
        assert r.returncode == 0, r.stderr
    files = sorted(os.listdir(dumps["absent"]))
    assert files == sorted(os.listdir(dumps["off"])) and len(files) >= 4 * n and not [k for k in files if "model_pose" in k]
    for k in files:
        assert open(os.path.join(dumps["off"], k), "rb").read() == open(os.path.join(dumps["absent"], k), "rb").read(), k

    # configuration errors name their key; a pose key without a relative pose, or one that revises past poses, is refused with "track"
    for bad, word in ((dict(keys, type="voxel_map", track=True, residual_gate=0.0), "residual_gate"), (dict(keys, type="voxel_map", track=True, damping=-1.0), "damping"),
                      (dict(keys, type="voxel_map", track=True, iterations=17), "iterations"), (dict(keys, type="voxel_map", track=True, stride=0), "stride"),
                      (dict(keys, type="voxel_map", track=True, min_inliers=5), "min_inliers"), (dict(keys, type="voxel_map", track=True, pose_key="pose_graph"), "pose_graph"),
                      (dict(keys, type="voxel_map", track=True, pose_key="local_ba"), "local_ba")):
        r = run_exe(src, head + [bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    r = run_exe(src, head + [dict(keys, type="voxel_map", **shape, **vp), dict(keys, type="plane_map", pose_key="model_pose", **grid)], tmp)
    assert r.returncode != 0 and 'requires "model_pose"' in r.stderr, r.stderr

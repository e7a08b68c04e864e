"""GPU tests of the dense ego-motion refinement (spec S26): cart_dense_ego_refine against the numpy restatement
tests/np_dense_ego.py, the whole result record byte for byte, on pitched, offset buffers.  Beside every byte comparison stands a premise
on the restatement (steps taken, inliers, status), so that no comparison passes on an empty case."""
import ctypes as C

import numpy as np
import pytest

import np_dense_ego as D
import np_motion as M
import test_dense_ego_spec as T
import test_motion_spec as S
from test_gpu_motion import cam_tuple, engine

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (255, 3), (256, 2), (257, 2), (513, 9), (3, 257), (40, 513)]


def _torch():
    import torch
    return torch


def offset(a, extra, fill):
    """`a` on the device inside a larger allocation: rows `extra` pixels longer than the image and two rows above it, all holding `fill`."""
    torch = _torch()
    full = np.full((a.shape[0] + 3, a.shape[1] + extra) + a.shape[2:], fill, a.dtype)
    full[2:2 + a.shape[0], 1:1 + a.shape[1]] = a
    return torch.from_numpy(full).cuda()[2:2 + a.shape[0], 1:1 + a.shape[1]]


def run(obj, cam, p, rel, dc, dp, fl, mask=None, stream=None):
    """cart_dense_ego_refine through DenseEgo.refine on pitched, offset inputs whose slack would pass every gate -> the device record."""
    from cartslam import dense_ego_params
    args = (offset(dc, 3, 256), offset(dp, 5, 256), offset(fl, 2, 0))
    mk = offset(mask, 7, 0) if mask is not None else None
    return obj.refine(cam_tuple(cam), rel, *args, params=dense_ego_params(**p), mask=mk, stream=stream, raw=True)


def record(res):
    _torch().cuda.synchronize()
    return res.cpu().numpy().view(D.RESULT_DTYPE).reshape(-1)


def same(got, exp):
    assert got.tobytes() == exp.tobytes(), f"\n{got}\n{exp}"


_OBJ = []


def dense():
    from cartslam import DenseEgo
    if not _OBJ:
        _OBJ.append(DenseEgo(engine(), 1242, 520))
    return _OBJ[0]


NARROW_TRUE = T.small_rel(0.02, -0.2, (0.0, -0.01, -0.25))          # nearly no sideways flow: a 3-pixel-wide frame keeps its candidates
NARROW_START = T.small_rel(0.03, -0.15, (0.001, -0.012, -0.24))


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_that_straddle_the_lane_and_row_strides(w, h, stride):
    true, start = (NARROW_TRUE, NARROW_START) if w < 16 else (T.TRUE_REL, T.START_REL)
    cam, dc, dp, fl = T.smooth_scene(w, h, true, seed=w + h)
    p = D.params(min_inliers=6, stride=stride)
    exp = D.refine(cam, p, start, dc, dp, fl)
    if (w, h) == (1, 1):     # one candidate, below min_inliers: no step
        assert exp["status"][0] == 0 and exp["steps"][0] == 0 and exp["n_initial"][0] == 1
    else:                    # from the restatement: every other shape takes its four steps at every stride (7 x 5 at stride 3 on exactly 6 pixels)
        assert exp["status"][0] == 1 and exp["steps"][0] == 4 and exp["n_inliers"][0] >= 6 and exp["n_initial"][0] >= 6
    same(record(run(dense(), cam, p, start, dc, dp, fl)), exp)


def test_all_invalid_and_all_masked():
    w, h = 130, 9
    cam, dc, dp, fl = T.smooth_scene(w, h, T.TRUE_REL)
    p = D.params(min_inliers=6)
    none = np.full_like(dc, -32768)
    exp = D.refine(cam, p, T.START_REL, none, dp, fl)
    assert exp["status"][0] == 0 and exp["n_candidates"][0] == 0 and exp["rms"][0] == 0.0
    same(record(run(dense(), cam, p, T.START_REL, none, dp, fl)), exp)
    ones = np.ones((h, w), np.uint8)
    exp = D.refine(cam, p, T.START_REL, dc, dp, fl, ones)
    assert exp["status"][0] == 0 and exp["n_candidates"][0] == 0
    same(record(run(dense(), cam, p, T.START_REL, dc, dp, fl, ones)), exp)
    some = (np.random.default_rng(4).integers(0, 3, (h, w))).astype(np.uint8)          # all three labels: only 1 leaves
    exp = D.refine(cam, p, T.START_REL, dc, dp, fl, some)
    plain = D.refine(cam, p, T.START_REL, dc, dp, fl)
    assert exp["status"][0] == 1 and 0 < exp["n_candidates"][0] < plain["n_candidates"][0] and exp.tobytes() != plain.tobytes()
    same(record(run(dense(), cam, p, T.START_REL, dc, dp, fl, some)), exp)
    same(record(run(dense(), cam, p, T.START_REL, dc, dp, fl)), plain)


def test_large_random_flows_leave_the_image_on_every_side():
    w, h = 261, 19
    dc, dp, fl, _ = S.random_frame(7, w, h, big_flow=True)
    p = D.params(min_inliers=6, flow_threshold=50.0, disparity_threshold=3.0)
    c = D.candidates(S.CAM, p, dc, dp, fl)
    xp, yp = c["xp"], c["yp"]
    assert (xp < 0).any() and (xp >= w).any() and (yp < 0).any() and (yp >= h).any() and 6 < c["cand"].sum() < w * h // 2
    exp = D.refine(S.CAM, p, M.REL_IDENTITY, dc, dp, fl)
    assert exp["n_initial"][0] >= 6
    same(record(run(dense(), S.CAM, p, M.REL_IDENTITY, dc, dp, fl)), exp)


def test_points_behind_the_camera():
    w, h = 70, 11
    cam, dc, dp, fl = T.smooth_scene(w, h, T.TRUE_REL)
    p = D.params(min_inliers=6)
    for tz in (-20.0, -8.0):                 # every point behind the camera; some behind, none near its disparity
        rel = S.rel_t(tz=tz)
        exp = D.refine(cam, p, rel, dc, dp, fl)
        assert exp["status"][0] == 0 and exp["n_candidates"][0] > 100 and exp["n_inliers"][0] == 0 and exp["rms"][0] == 0.0
        got = record(run(dense(), cam, p, rel, dc, dp, fl))
        same(got, exp)
        assert np.isfinite(got["R"]).all() and np.isfinite(got["t"]).all() and np.isfinite(got["rms"]).all()
    # a huge threshold lets points just in front of the camera contribute: whatever the spec gives (inf or NaN included), the device gives
    p = D.params(min_inliers=6, flow_threshold=1e30, disparity_threshold=1e30)
    rel = S.rel_t(tz=-8.0)
    exp = D.refine(cam, p, rel, dc, dp, fl)
    assert exp["n_initial"][0] > 6
    same(record(run(dense(), cam, p, rel, dc, dp, fl)), exp)


@pytest.mark.parametrize("iterations", [0, 1, 16])
def test_iterations(iterations):
    w, h = 96, 40
    cam, dc, dp, fl = T.smooth_scene(w, h, T.TRUE_REL, seed=2, invalid=0.05)
    p = D.params(min_inliers=6, iterations=iterations, disparity_weight=0.5)
    exp = D.refine(cam, p, T.START_REL, dc, dp, fl)
    assert exp["steps"][0] == iterations and exp["status"][0] == (1 if iterations else 0)
    if iterations == 0:
        assert D.join(exp["R"][0].tolist(), exp["t"][0].tolist()) == T.START_REL
    same(record(run(dense(), cam, p, T.START_REL, dc, dp, fl)), exp)


def test_stops_on_the_device():
    w, h = 96, 40
    cam, dc, dp, fl = T.smooth_scene(w, h, T.TRUE_REL, seed=2)
    p = D.params(min_inliers=w * h + 1)
    exp = D.refine(cam, p, T.START_REL, dc, dp, fl)
    assert exp["status"][0] == 0 and exp["n_inliers"][0] == exp["n_initial"][0] > 1000
    same(record(run(dense(), cam, p, T.START_REL, dc, dp, fl)), exp)
    cam = M.camera(fx=256.0, fy=256.0, cx=7.5, cy=0.0, baseline=0.5)                    # test_pivot_stop_on_a_degenerate_plane
    p = D.params(min_inliers=6, disparity_weight=0.0)
    exp = D.refine(cam, p, S.rel_t(tx=0.0078125), *S.flat(1, 16, 256, 256))
    assert exp["status"][0] == 0 and exp["n_inliers"][0] == 16
    same(record(run(dense(), cam, p, S.rel_t(tx=0.0078125), *S.flat(1, 16, 256, 256))), exp)


def test_a_stale_workspace_does_not_leak():
    from cartslam import DenseEgo, EngineError
    p = D.params(min_inliers=6)
    big = T.smooth_scene(300, 40, T.TRUE_REL, seed=5)
    small = T.smooth_scene(33, 7, T.TRUE_REL, seed=6)
    stopped = D.params(min_inliers=6, iterations=16)
    with DenseEgo(engine(), 300, 40) as a, DenseEgo(engine(), 300, 40) as fresh:
        first = record(run(a, big[0], stopped, T.START_REL, *big[1:]))
        second = record(run(a, small[0], p, T.START_REL, *small[1:]))
        alone = record(run(fresh, small[0], p, T.START_REL, *small[1:]))
        same(first, D.refine(big[0], stopped, T.START_REL, *big[1:]))
        same(second, alone)
        same(second, D.refine(small[0], p, T.START_REL, *small[1:]))
        wide = T.smooth_scene(301, 8, T.TRUE_REL)
        with pytest.raises(EngineError, match="exceeds"):
            run(a, wide[0], p, T.START_REL, *wide[1:])


_CORRIDOR = []


def corridor():
    if not _CORRIDOR:
        from test_gpu_motion import corridor_frame
        cam, rel, dc, dp, fl, planes, block = corridor_frame()
        rel0 = [float(v) for v in rel]
        rel0[3] += 0.01
        rel0[11] += 0.02
        labels = M.segment(cam, M.params(), rel0, dc, dp, fl)["labels"]
        _CORRIDOR.append((cam, rel0, dc, dp, fl, labels, D.refine(cam, D.params(), rel0, dc, dp, fl, labels)))
    return _CORRIDOR[0]


def test_full_size_corridor_on_two_streams():
    torch = _torch()
    cam, rel0, dc, dp, fl, labels, exp = corridor()
    assert exp["status"][0] == 1 and exp["steps"][0] == 4 and exp["n_inliers"][0] > 100000
    same(record(run(dense(), cam, D.params(), rel0, dc, dp, fl, labels)), exp)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = [run(dense(), cam, D.params(), rel0, dc, dp, fl, labels, stream=s) for s in (a, b, a, b)]   # one object: the calls are ordered by its event
    for out in outs:
        same(record(out), exp)


def test_bad_arguments_touch_no_output():
    torch = _torch()
    from cartslam import _lib, dense_ego_params
    lib = _lib.load()
    w, h = 130, 9
    cam_d, dc, dp, fl = T.smooth_scene(w, h, T.TRUE_REL)
    dc, dp, fl = (torch.from_numpy(a).cuda() for a in (dc, dp, fl))
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    res = torch.full((17 + 4,), 77.0, dtype=torch.float64, device="cuda")
    cam, p, rel = _lib.EgoCamera(*cam_tuple(cam_d)), dense_ego_params(min_inliers=6), (C.c_double * 12)(*T.START_REL)
    base = dict(disp_cur=(dc.data_ptr(), 2 * w), disp_prev=(dp.data_ptr(), 2 * w), flow=(fl.data_ptr(), 4 * w), mask=(mask.data_ptr(), w), size=(w, h),
                result=res.data_ptr())

    def call(obj=True, **kw):
        a = dict(base, **kw)
        flat = []
        for k in ("disp_cur", "disp_prev", "flow", "mask"):
            flat += [C.c_void_p(a[k][0]), a[k][1]]
        rc = lib.cart_dense_ego_refine(dense()._h if obj else None, C.byref(cam), rel, C.byref(p), *flat, *a["size"], C.c_void_p(a["result"]), None)
        return rc, lib.cart_last_error(None).decode()

    bad = [(dict(obj=False), "bad arguments"), (dict(result=None), "result"), (dict(result=res.data_ptr() + 4), "result must be 8-byte aligned"),
           (dict(size=(1243, h)), "exceeds"), (dict(size=(w, 521)), "exceeds"), (dict(size=(0, h)), "width")]
    for k, elem in (("disp_cur", 2), ("disp_prev", 2), ("flow", 4), ("mask", 1)):
        ptr, step = base[k]
        if k != "mask":
            bad.append(({k: (None, step)}, k))
        if elem > 1:
            bad.append(({k: (ptr + 1, step)}, k))
            bad.append(({k: (ptr, step + 1)}, k))
        bad.append(({k: (ptr, step - elem)}, k + "_step"))
        bad.append((dict(result=ptr + step * (h - 1)), f"result and {k} must not overlap"))
    for kw, word in bad:
        rc, err = call(**kw)
        assert rc != 0 and word in err, (kw, err)
    torch.cuda.synchronize()
    assert bool((res == 77.0).all())               # no refused call touched the output
    rc, err = call(mask=(None, 0))
    assert rc == 0, err
    torch.cuda.synchronize()
    assert not bool((res[:17] == 77.0).any()) and bool((res[17:] == 77.0).all())


def test_lifecycle():
    from cartslam import DenseEgo, Engine
    w, h = 64, 12
    cam, dc, dp, fl = T.smooth_scene(w, h, T.TRUE_REL)
    p = D.params(min_inliers=6)
    exp = D.refine(cam, p, T.START_REL, dc, dp, fl)
    eng = Engine(64, 32, num_disparities=0, paths=0)
    obj = DenseEgo(eng, w, h)
    eng.close()                                    # the object keeps its device, not its engine
    same(record(run(obj, cam, p, T.START_REL, dc, dp, fl)), exp)
    torch = _torch()
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = [run(obj, cam, p, T.START_REL, dc, dp, fl, stream=streams[k % 3]) for k in range(6)]    # back to back on one object
    for out in outs:
        same(record(out), exp)
    obj.close()
    obj.close()                                    # idempotent
    with DenseEgo(engine(), w, h) as o2:
        same(record(run(o2, cam, p, T.START_REL, dc, dp, fl)), exp)
    assert o2._h is None


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------
def test_dense_ego_module_in_the_frame_loop(tmp_path):
    """The dense_ego host module over 3 synthetic frames: <id>_dense_ego.bin (the device record, then the chained pose) against the
    restatement with the acceptance rule and np_ego's chain; a plane_map with "pose_key": "dense_ego" against np_planemap fed those poses;
    a plane_map without the key against np_planemap fed ego_motion's, as before."""
    import json
    import os

    import np_ego as E
    import np_planemap as PM
    import oracle_lib as O
    from test_gpu_matches import noise_frame, noise_world
    from test_gpu_planemap import check_dump
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n, w, h = 3, 320, 96
    world = noise_world(79)
    images = [noise_frame(world, f) for f in range(n)]
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for cam in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, cam))
    for f, (l, r) in enumerate(images):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    static = {"type": "static", "horizontal_range_min": 6, "horizontal_range_max": 18, "vertical_range_min": -5, "vertical_range_max": 6}
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    grid = dict(cells_x=64, cells_z=64, cell_size=1.0, max_depth=40.0, max_lateral=30.0)
    mp = dict(flow_threshold=1.5, disparity_threshold=0.5, radius=1, support_percent=40)
    dp = dict(flow_threshold=1.5, disparity_threshold=0.75, disparity_weight=0.5, iterations=3, stride=2, min_inliers=500)
    head = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
            {"type": "optflow", "search_radius": 4}, {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion"),
            {"type": "disparity_planeseg", "parameter_provider": static}, dict(keys, type="motion_seg", **mp)]
    cam = M.camera(**keys)
    pm_params = PM.params(cell_size=1.0, max_depth=40.0, max_lateral=30.0)
    estimates = 0
    for use_motion in (True, False):
        d = os.path.join(tmp, "dump%d" % use_motion)
        os.makedirs(d)
        modules = head + [dict(keys, type="dense_ego", use_motion=use_motion, **dp)] + ([dict(keys, type="plane_map", pose_key="dense_ego", **grid)] if use_motion else [dict(keys, type="plane_map", **grid)])
        r = run_exe(src, modules, tmp, ("--dump", d))
        assert r.returncode == 0, r.stderr
        ref_map = PM.Map(PM.camera(**keys), 64, 64, pm_params)
        pose, disps = list(E.POSE_IDENTITY), []
        for f in range(n):
            l, rr = images[f]
            ed = O.disparity_module(l, rr, 64, 8, 4, radius=2, iterations=1)
            ep = O.classify(O.plane_derivative(ed)[0], (6, 18, -5, 6, 12, 0))
            disps.append(ed)
            ego = np.fromfile(os.path.join(d, f"{f + 1}_ego_motion.bin"), np.uint8)
            ego_res, ego_pose = ego[:120].view(E.RESULT_DTYPE), ego[120:].view(np.float64)
            raw = open(os.path.join(d, f"{f + 1}_dense_ego.bin"), "rb").read()
            assert len(raw) == 136 + 96
            got, got_pose = np.frombuffer(raw, D.RESULT_DTYPE, 1), np.frombuffer(raw, np.float64, 12, 136)
            rel0 = D.join(ego_res["R"][0].tolist(), ego_res["t"][0].tolist())
            chained = ego_res.copy()
            if f == 0 or int(ego_res["status"][0]) == 0:
                exp = np.zeros(1, D.RESULT_DTYPE)
                exp["R"][0], exp["t"][0] = ego_res["R"][0], ego_res["t"][0]
            else:
                flow = O.block_flow(l, images[f - 1][0], 4, 2)
                mask = M.segment(cam, M.params(**mp), rel0, ed, disps[f - 1], flow)["labels"] if use_motion else None
                exp = D.refine(cam, D.params(**dp), rel0, ed, disps[f - 1], flow, mask)
                if use_motion and exp["status"][0] == 1 and exp["n_initial"][0] >= 500 and (mask == 1).sum() > 0:     # a real refinement, a real mask
                    estimates += 1
                rel = D.accept(exp, rel0)
                chained["R"][0], chained["t"][0] = D.split(rel)
            same(got, exp)
            pose = E.chain(pose, chained)
            assert got_pose.tobytes() == np.array(pose, np.float64).tobytes(), f"frame {f + 1}: the chained pose"
            ref_map.update(ed, ep, pose if use_motion else ego_pose)
            check_dump(os.path.join(d, f"{f + 1}_plane_map.bin"), ref_map, 3, 50)
    assert estimates >= 1
    # configuration errors name their key and fail at creation
    for bad, word in ((dict(type="dense_ego"), "fx"), (dict(keys, type="dense_ego", stride=17), "stride"), (dict(keys, type="dense_ego", iterations=-1), "iterations"),
                      (dict(keys, type="dense_ego", min_inliers=5), "min_inliers"), (dict(keys, type="dense_ego", disparity_weight=-1.0), "disparity_weight"),
                      (dict(keys, type="dense_ego", flow_threshold=0.0), "flow_threshold"), (dict(keys, type="dense_ego", disparity_threshold=0.0), "disparity_threshold"),
                      (dict(keys, type="dense_ego", min_disparity=0.0), "min_disparity")):
        r = run_exe(src, head + [bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    r = run_exe(src, head[:6] + [dict(keys, type="dense_ego", use_motion=True)], tmp)
    assert r.returncode != 0 and 'requires "motion"' in r.stderr, r.stderr
    r = run_exe(src, head + [dict(keys, type="plane_map", pose_key="dense_ego", **grid)], tmp)
    assert r.returncode != 0 and 'requires "dense_ego"' in r.stderr, r.stderr

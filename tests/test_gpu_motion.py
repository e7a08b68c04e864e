"""GPU tests of the motion segmentation (spec S25): cart_motion_segment against the numpy restatement tests/np_motion.py,
byte for byte on pitched buffers, and the motion_seg host module in the C++ frame loop.  Beside every byte comparison stands a numeric
premise on the restatement (labels and gates that must occur), so that no comparison passes on an empty case."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import np_motion as M
import test_motion_spec as S

pytestmark = pytest.mark.gpu

CAM = S.CAM
SHAPES = [(5, 3), (67, 5), (130, 33), (257, 17)]


def _torch():
    import torch
    return torch


_ENGINE = []


def engine():
    from cartslam import Engine
    if not _ENGINE:
        _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's (see __graft_entry__.build)
        _ENGINE.append(Engine(64, 32, num_disparities=0, paths=0))
    return _ENGINE[0]


def cam_tuple(cam):
    return tuple(cam[k] for k in ("fx", "fy", "cx", "cy", "baseline"))


def pitched(a, extra, fill):
    """A device tensor of `a` ([h, w] or [h, w, c]) whose rows are `extra` pixels longer than the image, the slack holding `fill`."""
    torch = _torch()
    full = np.full((a.shape[0], a.shape[1] + extra) + a.shape[2:], fill, a.dtype)
    full[:, :a.shape[1]] = a
    return torch.from_numpy(full).cuda()[:, :a.shape[1]]


def run(cam, p, rel, dc, dp, fl, planes=None, residual=True, stream=None):
    """cart_motion_segment through cartslam.motion_segment on pitched inputs whose slack would pass every gate -> host arrays."""
    torch = _torch()
    from cartslam import motion_params, motion_segment
    args = (pitched(dc, 3, 256), pitched(dp, 5, 256), pitched(fl, 2, 0))
    pl = pitched(planes, 7, 1) if planes is not None else None
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        out = motion_segment(engine(), cam_tuple(cam), rel, *args, params=motion_params(**p), planes=pl, residual=residual, raw=True)
    return out


def same(out, ref, residual=True, planes=True):
    _torch().cuda.synchronize()
    assert (out.residual is not None) == residual and (out.planes_static is not None) == planes
    for key in ("raw", "labels") + (("residual",) if residual else ()) + (("planes_static",) if planes else ()):
        got = getattr(out, key).cpu().numpy()
        assert got.dtype == ref[key].dtype and got.shape == ref[key].shape, key
        assert got.tobytes() == ref[key].tobytes(), f"{key}: {int((got != ref[key]).sum())} values differ"


def check(cam, p, rel, dc, dp, fl, planes=None, residual=True):
    ref = M.segment(cam, p, rel, dc, dp, fl, planes)
    same(run(cam, p, rel, dc, dp, fl, planes, residual), ref, residual, planes is not None)
    return ref


@pytest.mark.parametrize("radius", [0, 1, 4])
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_and_radii_on_pitched_buffers(w, h, radius):
    """Every output at sizes below, at and above one block / one tile, with a window larger than the image at (5, 3)."""
    dc, dp, fl, planes = S.random_frame(1 if (w, h) == (5, 3) else 7 * w + h, w, h)   # seed 1: 5 STATIC, 2 MOVING, 8 UNKNOWN pixels at (5, 3)
    ref = check(CAM, M.params(radius=radius, support_percent=40), M.REL_IDENTITY, dc, dp, fl, planes)
    S.premises(ref)
    if w > 5:
        assert ((ref["labels"] != ref["raw"]).sum() > 0) == (radius > 0)
    assert (ref["planes_static"] != planes).sum() == ((ref["labels"] == 1) & (planes != 2)).sum()


@pytest.mark.parametrize("w,h", SHAPES[1:])
def test_large_random_flows_and_a_yawed_pose(w, h):
    """A gather from anywhere in the previous image, flows that leave it, and a yawed rel with negative translations."""
    dc, dp, fl, planes = S.random_frame(11 * w + h, w, h, big_flow=True)
    rel = S.yaw_rel(-0.3, (-0.01, -0.005, -0.1))     # 1.3 pixels of yaw, a third of a pixel of t_x, 0.2 of disparity
    ref = check(CAM, M.params(radius=2), rel, dc, dp, fl, planes)
    S.premises(ref)
    moved = (np.abs(fl.astype(np.int64) >> 5).max(axis=2) > 8) & (ref["gate"] == 0)
    assert moved.sum() > 10                                                  # known pixels that read far from themselves
    ref = check(CAM, M.params(radius=1), S.yaw_rel(170.0, (0.5, -0.2, -1.0)), dc, dp, fl)      # nearly every point behind the camera
    assert (ref["gate"] == 4).sum() > w * h // 4


def test_flows_leave_the_image_on_every_side():
    w, h = 67, 9
    dc, dp, _ = S.flat(h, w, 256, 256)
    for fx, fy in ((33, 0), (-1, 0), (0, 64), (0, -33), (95, 40), (-70, -1), (33, -1), (-1, 32)):   # sides and corners; -1 >> 5 = -1
        fl = np.zeros((h, w, 2), np.int16)
        fl[..., 0], fl[..., 1] = fx, fy
        ref = check(CAM, M.params(radius=0), M.REL_IDENTITY, dc, dp, fl)
        sx, sy = fx >> 5, fy >> 5
        assert (ref["gate"] == 2).sum() == w * h - (w - abs(sx)) * (h - abs(sy)) > 0, (fx, fy)
        assert (ref["raw"] != M.UNKNOWN).sum() == (w - abs(sx)) * (h - abs(sy)) > 0


@pytest.mark.parametrize("case", S.threshold_cases(), ids=lambda c: c[0])
def test_threshold_edges(case):
    _, cam, p, rel, dc, dp, fl, label, record = case
    ref = check(cam, p, rel, dc, dp, fl)
    assert (ref["raw"] == label).all()
    if record is not None:
        assert (ref["residual"] == np.array(record, np.int16)).all()


def test_points_behind_the_camera():
    dc, dp, fl = S.flat(9, 67, 256, 256)
    assert (check(CAM, M.params(), S.rel_t(tz=-8.0), dc, dp, fl)["gate"] == 4).all()           # q.z = 0
    assert (check(CAM, M.params(), S.rel_t(tz=-7.0), dc, dp, fl)["raw"] == M.MOVING).all()     # q.z = 1


@pytest.mark.parametrize("pattern", ["checkerboard", "columns", "rows", "blocks"])
def test_raw_patterns_through_the_filter(pattern):
    """The disparity step of 2 pixels makes a pixel MOVING exactly where the pattern is set: the filter sees the pattern as its raw image."""
    w, h = 130, 33
    y, x = np.indices((h, w))
    on = {"checkerboard": (x + y) % 2, "columns": x % 2, "rows": y % 3 == 0, "blocks": ((x // 5) + (y // 3)) % 2}[pattern].astype(bool)
    dc, dp, fl = S.flat(h, w, 256, 256)
    dc[on] = 288
    dc[::7, ::11] = -32768
    moving = 0
    for radius, percent in ((1, 30), (2, 34), (4, 30), (1, 60)):
        ref = check(CAM, M.params(radius=radius, support_percent=percent), M.REL_IDENTITY, dc, dp, fl)
        assert ((ref["raw"] == M.MOVING) == (on & (dc != -32768))).all() and (ref["labels"] != ref["raw"]).sum() > 0
        assert (ref["labels"] == M.UNKNOWN).sum() == (dc == -32768).sum() > 0
        moving += int((ref["labels"] == M.MOVING).sum())
    assert moving > 0


def test_optional_outputs_and_host_arrays():
    from cartslam import motion_params, motion_segment
    dc, dp, fl, planes = S.random_frame(3, 130, 33)
    p = M.params(radius=2)
    ref = M.segment(CAM, p, M.REL_IDENTITY, dc, dp, fl, planes)
    S.premises(ref)
    same(run(CAM, p, M.REL_IDENTITY, dc, dp, fl, None, residual=False), ref, residual=False, planes=False)
    same(run(CAM, p, M.REL_IDENTITY, dc, dp, fl, planes, residual=False), ref, residual=False, planes=True)
    same(run(CAM, p, M.REL_IDENTITY, dc, dp, fl, None, residual=True), ref, residual=True, planes=False)
    out = motion_segment(engine(), cam_tuple(CAM), M.REL_IDENTITY, dc, dp, fl, params=motion_params(**p), planes=planes)   # numpy in, numpy out
    for key in ("residual", "raw", "labels", "planes_static"):
        assert isinstance(getattr(out, key), np.ndarray) and getattr(out, key).tobytes() == ref[key].tobytes(), key
    assert motion_segment(engine(), cam_tuple(CAM), M.REL_IDENTITY, dc, dp, fl).labels.tobytes() == M.segment(CAM, M.params(), M.REL_IDENTITY, dc, dp, fl)["labels"].tobytes()


def corridor_frame():
    """synth.road_corridor_motion at 1242 x 375: a forward step of 0.5 m with a block that moves with the camera."""
    from cartslam import synth
    cam = M.camera(721.5, 721.5, 609.5, 172.85, 0.54)
    return (cam,) + tuple(synth.road_corridor_motion(1242, 375, *cam_tuple(cam)))


_CORRIDOR = []


def corridor():
    if not _CORRIDOR:
        cam, rel, dc, dp, fl, planes, block = corridor_frame()
        _CORRIDOR.append((cam, rel, dc, dp, fl, planes, block, M.segment(cam, M.params(), rel, dc, dp, fl, planes)))
    return _CORRIDOR[0]


def test_full_size_corridor_with_a_moving_block_and_two_streams():
    torch = _torch()
    cam, rel, dc, dp, fl, planes, block, ref = corridor()
    inside = ref["labels"][block]
    outside = ref["labels"].copy()
    outside[block] = M.UNKNOWN
    assert (inside == M.MOVING).mean() > 0.95 and (outside == M.STATIC).sum() > 100000 and (outside == M.MOVING).sum() < (outside == M.STATIC).sum() // 4
    S.premises(ref)
    same(run(cam, M.params(), rel, dc, dp, fl, planes), ref)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = [run(cam, M.params(), rel, dc, dp, fl, planes, stream=s) for s in (a, b, a, b)]     # side by side, no shared state
    for out in outs:
        same(out, ref)


def test_bad_arguments_touch_no_output():
    torch = _torch()
    from cartslam import EngineError, _lib, motion_params, motion_segment
    lib = _lib.load()
    w, h = 130, 9
    dc, dp, fl, planes = (torch.from_numpy(a).cuda() for a in S.random_frame(1, w, h))
    res = torch.full((h, w, 4), 77, dtype=torch.int16, device="cuda")
    raw, labels, static = (torch.full((h, w), 77, dtype=torch.uint8, device="cuda") for _ in range(3))
    cam, p, rel = _lib.EgoCamera(*cam_tuple(CAM)), motion_params(), (C.c_double * 12)(*M.REL_IDENTITY)
    base = dict(disp_cur=(dc.data_ptr(), 2 * w), disp_prev=(dp.data_ptr(), 2 * w), flow=(fl.data_ptr(), 4 * w), size=(w, h), residual=(res.data_ptr(), 8 * w),
                raw=(raw.data_ptr(), w), labels=(labels.data_ptr(), w), planes=(planes.data_ptr(), w), planes_static=(static.data_ptr(), w))

    def call(eng=True, **kw):
        a = dict(base, **kw)
        flat = []
        for k in ("disp_cur", "disp_prev", "flow", "size", "residual", "raw", "labels", "planes", "planes_static"):
            flat += [C.c_void_p(a[k][0]) if k != "size" else a[k][0], a[k][1]]
        rc = lib.cart_motion_segment(engine()._h if eng else None, C.byref(cam), rel, C.byref(p), *flat, None)
        return rc, lib.cart_last_error(None).decode()

    bad = [(dict(eng=False), "bad arguments")]
    for k, elem in (("disp_cur", 2), ("disp_prev", 2), ("flow", 4), ("residual", 8), ("raw", 1), ("labels", 1), ("planes", 1), ("planes_static", 1)):
        ptr, step = base[k]
        if k != "residual":
            bad.append(({k: (None, step)}, k if k not in ("planes", "planes_static") else "planes"))
        if elem > 1:
            bad.append(({k: (ptr + 1, step)}, k))
            bad.append(({k: (ptr, step + 1)}, k))
        bad.append(({k: (ptr, step - elem)}, k + "_step"))
    bad += [(dict(size=(0, h)), "width"), (dict(size=(w, 16385)), "height"), (dict(planes_static=base["planes"]), "overlap"),
            (dict(planes_static=(planes.data_ptr() + w * (h - 1), w)), "overlap"), (dict(labels=base["raw"]), "overlap"),
            # no output may lie on another output or on an input
            (dict(raw=(res.data_ptr(), w)), "residual and raw must not overlap"), (dict(labels=base["planes_static"]), "labels and planes_static must not overlap"),
            (dict(labels=base["planes"]), "planes and labels must not overlap"), (dict(raw=(dp.data_ptr(), w)), "disp_prev and raw must not overlap"),
            (dict(residual=(dc.data_ptr(), 8 * w)), "disp_cur and residual must not overlap"), (dict(planes_static=(fl.data_ptr(), w)), "flow and planes_static must not overlap"),
            (dict(labels=(dc.data_ptr() + 2 * w * h - 1, w)), "disp_cur and labels must not overlap")]
    for kw, word in bad:
        rc, err = call(**kw)
        assert rc != 0 and word in err, (kw, err)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (res, raw, labels, static))     # no refused call touched an output
    rc, err = call()
    assert rc == 0, err
    torch.cuda.synchronize()
    assert not bool((labels == 77).any()) and not bool((static == 77).any())
    with pytest.raises(EngineError, match="rel"):
        motion_segment(engine(), cam_tuple(CAM), [float("nan")] * 12, dc, dp, fl, raw=True)
    with pytest.raises(EngineError, match="radius"):
        motion_segment(engine(), cam_tuple(CAM), M.REL_IDENTITY, dc, dp, fl, params=motion_params(radius=5), raw=True)
    with pytest.raises(EngineError):
        motion_segment(engine(), cam_tuple(CAM), M.REL_IDENTITY, dc.cpu(), dp, fl, raw=True)
    with pytest.raises(EngineError, match="flow"):
        motion_segment(engine(), cam_tuple(CAM), M.REL_IDENTITY, dc, dp, fl[:, :, :1], raw=True)


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------
def read_motion(path, w, h):
    raw = open(path, "rb").read()
    assert len(raw) == 8 + w * h * 10, path
    assert np.frombuffer(raw, "<i4", 2).tolist() == [w, h]
    return dict(labels=np.frombuffer(raw, np.uint8, w * h, 8).reshape(h, w), raw=np.frombuffer(raw, np.uint8, w * h, 8 + w * h).reshape(h, w),
                residual=np.frombuffer(raw, np.int16, w * h * 4, 8 + 2 * w * h).reshape(h, w, 4))


def test_motion_seg_module_in_the_frame_loop(tmp_path):
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
    modules = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
               {"type": "optflow", "search_radius": 4}, {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion"),
               {"type": "disparity_planeseg", "parameter_provider": static}, dict(keys, type="motion_seg", planes=True, **mp),
               dict(keys, type="plane_map", planes_key="planes_static", **grid)]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, modules, tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    cam = M.camera(**keys)
    ref_map = PM.Map(PM.camera(**keys), 64, 64, PM.params(cell_size=1.0, max_depth=40.0, max_lateral=30.0))
    disps, estimates = [], 0
    for f in range(n):
        l, rr = images[f]
        ed = O.disparity_module(l, rr, 64, 8, 4, radius=2, iterations=1)
        ep = O.classify(O.plane_derivative(ed)[0], (6, 18, -5, 6, 12, 0))
        disps.append(ed)
        ego = np.fromfile(os.path.join(d, f"{f + 1}_ego_motion.bin"), np.float64)
        status = int(np.frombuffer(ego[13:14].tobytes(), "<i4")[0])
        got = read_motion(os.path.join(d, f"{f + 1}_motion.bin"), w, h)
        comps = np.fromfile(os.path.join(d, f"{f + 1}_motion_components.bin"), np.int32).reshape(h, w)
        count = int(np.fromfile(os.path.join(d, f"{f + 1}_motion_component_count.bin"), np.int32)[0])
        if f == 0 or status == 0:
            assert f > 0 or status == 0
            exp = M.unknown_frame(h, w, ep)
            assert (comps == -1).all() and count == 0
        else:
            estimates += 1
            flow = O.block_flow(l, images[f - 1][0], 4, 2)
            assert np.fromfile(os.path.join(d, f"{f + 1}_optflow.bin"), np.int16).tobytes() == flow.tobytes()
            rel = np.concatenate([ego[0:9].reshape(3, 3), ego[9:12].reshape(3, 1)], axis=1).reshape(12)
            exp = M.segment(cam, M.params(**mp), rel, ed, disps[f - 1], flow, ep)
            assert (exp["raw"] == M.STATIC).sum() > w * h // 4 and (exp["gate"] > 0).sum() > 0     # a static world, mostly recognised as such
            eids, en = O.ccl(exp["labels"])
            assert (comps == eids).all() and count == en
        for key in ("labels", "raw", "residual"):
            assert got[key].tobytes() == exp[key].tobytes(), f"frame {f + 1}: {key}"
        assert np.fromfile(os.path.join(d, f"{f + 1}_planes_static.bin"), np.uint8).tobytes() == exp["planes_static"].tobytes(), f"frame {f + 1}: planes_static"
        ref_map.update(ed, exp["planes_static"], ego[15:])
        check_dump(os.path.join(d, f"{f + 1}_plane_map.bin"), ref_map, 3, 50)
    assert estimates >= 1
    # configuration errors name their key
    head = modules[:6]
    for bad, word in ((dict(type="motion_seg"), "fx"), (dict(keys, type="motion_seg", radius=5), "radius"), (dict(keys, type="motion_seg", support_percent=0), "support_percent"),
                      (dict(keys, type="motion_seg", flow_threshold=0.0), "flow_threshold"), (dict(keys, type="motion_seg", disparity_threshold=-1.0), "disparity_threshold"),
                      (dict(keys, type="motion_seg", min_disparity=0.0), "min_disparity"), (dict(keys, type="motion_seg", baseline=0.0), "baseline")):
        r = run_exe(src, head + [bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    r = run_exe(src, head + [dict(keys, type="plane_map", planes_key="no_such_image", **grid)], tmp)
    assert r.returncode != 0 and 'requires "no_such_image"' in r.stderr, r.stderr
    r = run_exe(src, head[:5] + [dict(keys, type="motion_seg", planes=True)], tmp)
    assert r.returncode != 0 and 'requires "planes"' in r.stderr, r.stderr

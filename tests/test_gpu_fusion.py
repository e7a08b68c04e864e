"""GPU tests of the temporal disparity fusion (spec S28): cart_fusion_update against the numpy restatement
tests/np_fusion.py, byte for byte on pitched buffers that start at a byte offset, and the temporal_fusion host module in the C++ frame
loop.  Beside every byte comparison stands a numeric premise on the restatement (source classes that must occur), so that no comparison
passes on an empty case."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import np_fusion as F
import test_fusion_spec as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 3), (64, 3), (65, 3), (257, 9), (130, 70)]   # width x height
SENTINEL = 77


def _torch():
    import torch
    return torch


_STATE = {}


def engine():
    from cartslam import Engine
    if "engine" not in _STATE:
        _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's (see __graft_entry__.build)
        _STATE["engine"] = Engine(64, 32, num_disparities=0, paths=0)
    return _STATE["engine"]


def fusion():
    """One object for frames of up to 257 x 70, shared by the tests: every call must leave its z-buffer and counters all zero."""
    from cartslam import DisparityFusion
    if "fusion" not in _STATE:
        _STATE["fusion"] = DisparityFusion(engine(), 257, 70)
    return _STATE["fusion"]


def cam_for(w, h):
    return F.camera(fx=256.0, fy=256.0, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, baseline=0.5)


def cam_tuple(cam):
    return tuple(cam[k] for k in ("fx", "fy", "cx", "cy", "baseline"))


def pitched(a, extra, fill, offset):
    """A device tensor of the image `a` whose rows are `extra` pixels longer than the image and whose first pixel lies `offset` pixels
    into its allocation, the slack holding `fill`."""
    torch = _torch()
    h, w = a.shape
    flat = np.full(offset + h * (w + extra), fill, a.dtype)
    rows = flat[offset:].reshape(h, w + extra)
    rows[:, :w] = a
    return torch.from_numpy(flat).cuda()[offset:].view(h, w + extra)[:, :w]


def ptr_step(t):
    return (C.c_void_p(t.data_ptr()), t.stride(0) * t.element_size()) if t is not None else (None, 0)


def call(obj, cam, p, rel, dc, pd=None, pa=None, mp=None, mc=None, fused=None, age=None, source=None, counts=None, size=None, stream=None):
    """cart_fusion_update on device tensors (or (pointer, step) pairs) as they are -> (rc, message)."""
    from cartslam import _lib, fusion_params
    torch = _torch()
    lib = _lib.load()
    flat = []
    for t in (dc, pd, pa, mp, mc):
        flat += list(t if isinstance(t, tuple) else ptr_step(t))
    flat += list(size if size is not None else (int(dc.shape[1]), int(dc.shape[0])))
    for t in (fused, age, source):
        flat += list(t if isinstance(t, tuple) else ptr_step(t))
    cnt = counts if not isinstance(counts, torch.Tensor) else C.c_void_p(counts.data_ptr())
    host_rel = (C.c_double * 12)(*[float(v) for v in rel]) if rel is not None else None
    sp = C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)
    rc = lib.cart_fusion_update(obj._h if obj is not None else None, C.byref(_lib.EgoCamera(*cam_tuple(cam))), host_rel, C.byref(fusion_params(**p)), *flat, cnt, sp)
    return rc, lib.cart_last_error(None).decode()


def run(cam, p, rel, dc, prev=None, mask_prev=None, mask_cur=None, source=True, counts=True, obj=None, stream=None):
    """One call on pitched, offset inputs and outputs whose slack would pass every gate -> (host arrays, the output tensors' parents)."""
    torch = _torch()
    h, w = dc.shape
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        ins = dict(dc=pitched(dc, 3, 256, 1), pd=pitched(prev[0], 5, 256, 3) if prev else None, pa=pitched(prev[1], 2, 200, 3) if prev else None,
                   mp=pitched(mask_prev, 1, 0, 5) if mask_prev is not None else None, mc=pitched(mask_cur, 4, 0, 7) if mask_cur is not None else None)
        outs = dict(fused=pitched(np.full((h, w), SENTINEL, np.int16), 3, SENTINEL, 1), age=pitched(np.full((h, w), SENTINEL, np.uint8), 6, SENTINEL, 3),
                    source=pitched(np.full((h, w), SENTINEL, np.uint8), 1, SENTINEL, 1) if source else None,
                    counts=torch.full((7,), SENTINEL, dtype=torch.int32, device="cuda")[1:6] if counts else None)
    rc, err = call(obj or fusion(), cam, p, rel, stream=stream, **ins, **outs)
    assert rc == 0, err
    return outs


def same(outs, ref):
    torch = _torch()
    torch.cuda.synchronize()
    for name in ("fused", "age", "source", "counts"):
        t = outs[name]
        if t is None:
            continue
        got = t.cpu().numpy()
        assert got.dtype == ref[name].dtype and got.shape == ref[name].shape, name
        assert got.tobytes() == ref[name].tobytes(), f"{name}: {int((got != ref[name]).sum())} values differ"
        base = t._base if t._base is not None else t                 # the slack of the pitched output and the words around counts: untouched
        whole = base.cpu().numpy().reshape(-1)
        assert int((whole != SENTINEL).sum()) <= int((got != SENTINEL).sum()), f"{name}: bytes outside the image were written"


def check(cam, p, rel, dc, prev=None, mask_prev=None, mask_cur=None, **kw):
    ref = F.update(cam, F.params(**p), rel, dc, prev, mask_prev, mask_cur)
    same(run(cam, p, rel, dc, prev, mask_prev, mask_cur, **kw), ref)
    return ref


STEP_AND_YAW = S.yaw_rel(1.5, (0.02, -0.01, -0.3))     # a forward step and a yaw: the targets change rows and columns


@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_on_pitched_offset_buffers(w, h):
    """Every output at sizes below, at and above one wave, one block and one strip, with both masks, under the identity and under a pose that
    moves the targets, and without a previous frame."""
    dc, pd, pa, mp, mc = S.random_frame(7 * w + h, w, h)
    cam = cam_for(w, h)
    ref = check(cam, {}, F.REL_IDENTITY, dc, (pd, pa), mp, mc)
    if w * h >= 189:
        S.premises(ref)
    ref = check(cam, {}, STEP_AND_YAW, dc, (pd, pa), mp, mc)
    if w * h >= 189:
        S.premises(ref)
        assert (ref["zbuf"] != F.splat(cam, F.params(), F.REL_IDENTITY, pd, pa, mp)).sum() > w * h // 8      # the pose did move the targets
    ref = check(cam, {}, None, dc)
    assert ref["counts"][[2, 3, 4]].sum() == 0
    check(cam, {}, STEP_AND_YAW, dc, (pd, pa))                         # no masks


def big():
    """The 130 x 70 case of the tests below, built once."""
    if "big" not in _STATE:
        _STATE["big"] = (cam_for(130, 70),) + S.random_frame(130 * 70, 130, 70)
    return _STATE["big"]


def test_identity_reproduces_the_previous_image():
    cam, dc, pd, pa, mp, mc = big()
    hole = np.full(dc.shape, F.INVALID, np.int16)
    ref = check(cam, dict(min_age=1), F.REL_IDENTITY, hole, (pd, pa))
    src = (pa >= 1) & (pd != F.INVALID) & (pd >= 16)
    assert (ref["fused"][src] == pd[src]).all() and ref["counts"][F.PREDICTED] == src.sum() > 4000


def test_every_target_outside_the_image_and_behind_the_camera():
    cam, dc, pd, pa, mp, mc = big()
    for rel in (S.rel_t(tx=1e3), S.rel_t(ty=-1e6), S.rel_t(tz=-12.0), S.yaw_rel(170.0)):
        ref = check(cam, {}, rel, dc, (pd, pa))
        assert (ref["zbuf"] == 0).all() and ref["counts"][[2, 3, 4]].sum() == 0


def test_maximum_contention_every_source_on_one_pixel():
    """R = 0, t = (0, 0, 1) sends all 9100 pixels' sources to (cx, cy) = (64.5, 34.5): four target pixels take every maximum."""
    cam, dc, pd, pa, mp, mc = big()
    z, writes = F.splat(cam, F.params(), S.REL_COLLAPSE, pd, pa, want_targets=True)
    assert (z != 0).sum() == 4 and writes > 4 * 5000 and len(set(z[z != 0].tolist())) == 1
    check(cam, {}, S.REL_COLLAPSE, dc, (pd, pa))
    check(cam, {}, S.REL_COLLAPSE, dc, (pd, pa), mp, mc)


@pytest.mark.parametrize("name,values", [("splat_radius", (0.5, 0.96875)), ("max_weight", (1, 255)), ("min_age", (1, 255)), ("agree_threshold", (0.0625, 3.0)),
                                         ("min_disparity", (0.0625, 17.0))])
def test_parameters_off_their_defaults(name, values):
    cam, dc, pd, pa, mp, mc = big()
    refs = [check(cam, {name: v}, STEP_AND_YAW, dc, (pd, pa), mp, mc) for v in values]
    which = "zbuf" if name in ("splat_radius", "min_disparity") else "fused" if name in ("max_weight", "agree_threshold") else "source"
    assert (refs[0][which] != refs[1][which]).sum() > 50                 # the parameter is felt
    default = F.update(cam, F.params(), STEP_AND_YAW, dc, (pd, pa), mp, mc)
    assert any((r[which] != default[which]).sum() > 20 for r in refs)


def test_optional_outputs_and_the_python_class():
    from cartslam import DisparityFusion, fusion_params
    cam, dc, pd, pa, mp, mc = big()
    ref = F.update(cam, F.params(), STEP_AND_YAW, dc, (pd, pa), mp, mc)
    same(run(cam, {}, STEP_AND_YAW, dc, (pd, pa), mp, mc, source=False), ref)
    same(run(cam, {}, STEP_AND_YAW, dc, (pd, pa), mp, mc, counts=False), ref)
    same(run(cam, {}, STEP_AND_YAW, dc, (pd, pa), mp, mc, source=False, counts=False), ref)
    same(run(cam, {}, STEP_AND_YAW, dc, (pd, pa), mp, mc), ref)              # the counters were left zero by the calls that did not count
    out = fusion().update(cam_tuple(cam), STEP_AND_YAW, dc, (pd, pa), mp, mc)   # numpy in, numpy out
    for got, name in zip(out, ("fused", "age", "source", "counts")):
        assert isinstance(got, np.ndarray) and got.dtype == ref[name].dtype and got.tobytes() == ref[name].tobytes(), name
    assert fusion().update(cam_tuple(cam), None, dc, source=False)[2] is None
    with DisparityFusion(engine(), 130, 70) as small:
        got = small.update(cam_tuple(cam), STEP_AND_YAW, dc, (pd, pa), params=fusion_params(min_age=1))
        assert got[0].tobytes() == F.update(cam, F.params(min_age=1), STEP_AND_YAW, dc, (pd, pa))["fused"].tobytes()
    assert small._h is None


def test_back_to_back_calls_and_a_second_object_on_another_stream():
    """Two calls on one object with nothing in between: the second finds the z-buffer and the counters the first one left all zero, at a
    smaller size too.  A second object on another stream runs beside them."""
    torch = _torch()
    from cartslam import DisparityFusion
    cam, dc, pd, pa, mp, mc = big()
    other = DisparityFusion(engine(), 130, 70)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ref_a = F.update(cam, F.params(), STEP_AND_YAW, dc, (pd, pa), mp, mc)
    ref_b = F.update(cam, F.params(), S.REL_COLLAPSE, dc, (pd, pa))
    small = (cam_for(63, 3),) + S.random_frame(11, 63, 3)
    ref_c = F.update(small[0], F.params(), F.REL_IDENTITY, small[1], (small[2], small[3]))
    outs = [run(cam, {}, STEP_AND_YAW, dc, (pd, pa), mp, mc), run(cam, {}, S.REL_COLLAPSE, dc, (pd, pa), obj=other, stream=side),
            run(cam, {}, S.REL_COLLAPSE, dc, (pd, pa)), run(small[0], {}, F.REL_IDENTITY, small[1], (small[2], small[3])),
            run(cam, {}, STEP_AND_YAW, dc, (pd, pa), mp, mc, obj=other, stream=side), run(cam, {}, STEP_AND_YAW, dc, (pd, pa), mp, mc)]
    for out, ref in zip(outs, (ref_a, ref_b, ref_b, ref_c, ref_a, ref_a)):
        same(out, ref)
    other.close()


def test_three_frame_chain_feeds_on_the_device_outputs():
    """Frames 2 and 3 take the fused and age tensors of the call before as they lie on the device."""
    torch = _torch()
    cam, w, h = cam_for(130, 70), 130, 70
    rng = np.random.default_rng(28)
    y, x = np.indices((h, w))
    truth = (200 + 2 * y + (x > 70) * 90).astype(np.int16)               # a slanted surface with a depth step
    prev_dev, prev_ref, seen = None, None, np.zeros(5, np.int64)
    for f, rel in enumerate((None, S.yaw_rel(0.4, (0.01, 0.0, -0.2)), S.yaw_rel(-0.3, (0.0, 0.005, -0.25)))):
        d = (truth + rng.integers(-4, 5, (h, w))).astype(np.int16)
        d[rng.random((h, w)) < 0.15] = F.INVALID
        ref = F.update(cam, F.params(), rel, d, prev_ref)
        fused, age, source, counts = fusion().update(cam_tuple(cam), rel, torch.from_numpy(d).cuda(), prev_dev, raw=True)
        same(dict(fused=fused, age=age, source=source, counts=counts), ref)
        prev_dev, prev_ref = (fused, age), (ref["fused"], ref["age"])
        seen += ref["counts"]
    assert (seen[1:] > 100).all() and int(prev_ref[1].max()) == 3         # every class along the chain, and pixels confirmed in all three frames


def test_bad_arguments_touch_no_output():
    torch = _torch()
    from cartslam import DisparityFusion, EngineError, fusion_params
    w, h = 130, 9
    cam = cam_for(w, h)
    # one allocation in a known order, so that a misplaced output meets the buffer the case names before any other
    arena = torch.zeros(16 * 4096, dtype=torch.uint8, device="cuda")

    def carve(k, dtype, shape):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return arena[4096 * k:4096 * k + n].view(dtype).view(shape)
    dc, pd = carve(0, torch.int16, (h, w)), carve(1, torch.int16, (h, w))
    pa, mp, mc = (carve(k, torch.uint8, (h, w)) for k in (2, 3, 4))
    for t, a in zip((dc, pd, pa, mp, mc), S.random_frame(1, w, h)):
        t.copy_(torch.from_numpy(a))
    fused, age, source, counts = carve(5, torch.int16, (h, w)), carve(6, torch.uint8, (h, w)), carve(7, torch.uint8, (h, w)), carve(8, torch.int32, (5,))
    for t in (fused, age, source, counts):
        t.fill_(SENTINEL)
    obj = DisparityFusion(engine(), 130, 9)
    base = dict(dc=dc, pd=pd, pa=pa, mp=mp, mc=mc, fused=fused, age=age, source=source, counts=counts)
    names = dict(dc="disp_cur", pd="prev_disp", pa="prev_age", mp="mask_prev", mc="mask_cur", fused="fused", age="age", source="source")

    def refused(word, obj_=obj, rel=F.REL_IDENTITY, size=None, **kw):
        rc, err = call(obj_, cam, {}, rel, size=size or (w, h), **dict(base, **kw))
        assert rc != 0 and word in err, (kw, err)

    refused("bad arguments", obj_=None)
    refused("exceeds the object's 130 x 9", size=(131, 9))
    refused("exceeds the object's 130 x 9", size=(130, 10))
    refused("width", size=(0, 9))
    refused("rel is NULL", rel=None)
    for k in ("dc", "fused", "age"):
        refused(names[k] + " is NULL", **{k: None})
    refused("prev_disp and prev_age", pd=None)
    refused("prev_disp and prev_age", pa=None)
    for k, elem in (("dc", 2), ("pd", 2), ("pa", 1), ("mp", 1), ("mc", 1), ("fused", 2), ("age", 1), ("source", 1)):
        ptr, step = base[k].data_ptr(), w * elem
        if elem > 1:
            refused(names[k] + " and its step must be 2-byte aligned", **{k: (C.c_void_p(ptr + 1), step)})
            refused(names[k] + " and its step must be 2-byte aligned", **{k: (C.c_void_p(ptr), step + 1)})
        refused(names[k] + "_step is below the row size", **{k: (C.c_void_p(ptr), step - elem)})
    refused("counts must be 4-byte aligned", counts=C.c_void_p(counts.data_ptr() + 2))
    # no output may lie on another output or on an input: the pair is named
    refused("disp_cur and fused must not overlap", fused=dc)
    refused("prev_disp and fused must not overlap", fused=pd)
    refused("prev_age and age must not overlap", age=pa)
    refused("mask_prev and source must not overlap", source=mp)
    refused("mask_cur and age must not overlap", age=(C.c_void_p(mc.data_ptr() + w * (h - 1)), w))
    refused("fused and age must not overlap", age=(C.c_void_p(fused.data_ptr() + 2 * w * h - 1), w))
    refused("age and source must not overlap", source=age)
    refused("fused and counts must not overlap", counts=C.c_void_p(fused.data_ptr() + 4))
    refused("disp_cur and counts must not overlap", counts=C.c_void_p(dc.data_ptr() + 2 * w * h - 4))
    refused("source and counts must not overlap", counts=C.c_void_p(source.data_ptr()))
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (fused, age, source, counts))     # no refused call touched an output
    rc, err = call(obj, cam, {}, None, **dict(base, pd=None, pa=None))                   # mask_prev without a previous frame is not read
    assert rc == 0, err
    rc, err = call(obj, cam, {}, F.REL_IDENTITY, **base)
    assert rc == 0, err
    torch.cuda.synchronize()
    ref = F.update(cam, F.params(), F.REL_IDENTITY, *(t.cpu().numpy() for t in (dc,)), prev=(pd.cpu().numpy(), pa.cpu().numpy()), mask_prev=mp.cpu().numpy(),
                   mask_cur=mc.cpu().numpy())
    assert fused.cpu().numpy().tobytes() == ref["fused"].tobytes() and counts.cpu().numpy().tobytes() == ref["counts"].tobytes()
    with pytest.raises(EngineError, match="rel"):
        obj.update(cam_tuple(cam), [float("nan")] * 12, dc, (pd, pa), raw=True)
    with pytest.raises(EngineError, match="splat_radius"):
        obj.update(cam_tuple(cam), F.REL_IDENTITY, dc, params=fusion_params(splat_radius=1.0), raw=True)
    with pytest.raises(EngineError, match="prev"):
        obj.update(cam_tuple(cam), F.REL_IDENTITY, dc, (pd, None), raw=True)
    with pytest.raises(EngineError, match="mask_cur"):
        obj.update(cam_tuple(cam), F.REL_IDENTITY, dc, mask_cur=mc[:, :8], raw=True)
    with pytest.raises(EngineError, match="max_width"):
        DisparityFusion(engine(), 0, 9)
    eng2 = __import__("cartslam").Engine(64, 32, num_disparities=0, paths=0)
    late = DisparityFusion(eng2, 16, 8)
    eng2.close()
    late.close()                                                           # destroy is valid after the engine
    obj.close()


# ---- the C++ frame loop ------------------------------------------------------------------------------------------------------------
def read_fused(path, w, h):
    raw = open(path, "rb").read()
    assert len(raw) == 8 + w * h * 4 + 20, path
    assert np.frombuffer(raw, "<i4", 2).tolist() == [w, h]
    return dict(fused=np.frombuffer(raw, np.int16, w * h, 8).reshape(h, w), age=np.frombuffer(raw, np.uint8, w * h, 8 + 2 * w * h).reshape(h, w),
                source=np.frombuffer(raw, np.uint8, w * h, 8 + 3 * w * h).reshape(h, w), counts=np.frombuffer(raw, np.int32, 5, 8 + 4 * w * h))


def test_temporal_fusion_module_in_the_frame_loop(tmp_path):
    """cart_slam_amd over four synthetic frames against the chain of restatements np_ego -> np_fusion -> np_planemap: temporal_fusion feeding
    plane_map through disparity_key, then temporal_fusion with the labels of motion_seg as its masks."""
    import np_ego as E
    import np_motion as NM
    import np_planemap as PM
    import oracle_lib as O
    from test_gpu_ego import restated_frames
    from test_gpu_matches import noise_frame, noise_world
    from test_gpu_planemap import check_dump
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
    grid = dict(cells_x=64, cells_z=64, cell_size=1.0, max_depth=40.0, max_lateral=30.0)
    fp = dict(agree_threshold=0.75, max_weight=3, min_age=1)
    mp = dict(flow_threshold=1.5, disparity_threshold=0.5, radius=1, support_percent=40)
    head = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1}, {"type": "optflow", "search_radius": 4},
            {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion"), {"type": "disparity_planeseg", "parameter_provider": static}]
    # the restatement chain, once for both runs
    ecam, fcam = E.camera(**keys), F.camera(**keys)
    feats, stereo, temporal = restated_frames(images, 5000)
    lms = [E.triangulate(ecam, feats[f][0][0], feats[f][1][0], stereo[f]) for f in range(n)]
    disps, planes, egos, poses, pose = [], [], [], [], list(E.POSE_IDENTITY)
    for f in range(n):
        l, rr = images[f]
        disps.append(O.disparity_module(l, rr, 64, 8, 4, radius=2, iterations=1))
        planes.append(O.classify(O.plane_derivative(disps[f])[0], (6, 18, -5, 6, 12, 0)))
        res = E.estimate(ecam, E.params(), lms[f], feats[f][0][0], lms[max(f - 1, 0)], temporal[f], 0, f + 1)[0]
        pose = E.chain(pose, res)
        egos.append(res)
        poses.append(list(pose))
    rels = [np.concatenate([e["R"][0].reshape(3, 3), e["t"][0].reshape(3, 1)], axis=1).reshape(12) for e in egos]
    carried = [f > 0 and int(egos[f]["status"][0]) != 0 for f in range(n)]
    assert sum(carried) >= 2

    # run A: temporal_fusion, and plane_map voting with the fused image
    d = os.path.join(tmp, "dump_a")
    os.makedirs(d)
    r = run_exe(src, head + [dict(keys, type="temporal_fusion", **fp), dict(keys, type="plane_map", disparity_key="disparity_fused", **grid)], tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    ref_map = PM.Map(PM.camera(**keys), 64, 64, PM.params(cell_size=1.0, max_depth=40.0, max_lateral=30.0))
    prev, seen = None, np.zeros(5, np.int64)
    for f in range(n):
        ego = open(os.path.join(d, f"{f + 1}_ego_motion.bin"), "rb").read()
        assert ego[:120] == egos[f].tobytes() and ego[120:] == np.array(poses[f], np.float64).tobytes(), f"frame {f + 1}: ego_motion"
        ref = F.update(fcam, F.params(**fp), rels[f], disps[f], prev if carried[f] else None)
        got = read_fused(os.path.join(d, f"{f + 1}_disparity_fused.bin"), w, h)
        for name in ("fused", "age", "source", "counts"):
            assert got[name].tobytes() == ref[name].tobytes(), f"frame {f + 1}: {name}"
        assert np.fromfile(os.path.join(d, f"{f + 1}_disparity.bin"), np.int16).tobytes() == disps[f].tobytes()      # the input is what it is without the module
        ref_map.update(ref["fused"], planes[f], poses[f])
        check_dump(os.path.join(d, f"{f + 1}_plane_map.bin"), ref_map, 3, 50)
        prev = (ref["fused"], ref["age"])
        seen += ref["counts"]
    assert seen[F.AGREED] > w * h // 4 and seen[F.PREDICTED] > 0 and (prev[0] != disps[-1]).sum() > 100      # the fusion did something, and the map saw it

    # run B: the labels of motion_seg as mask_cur and, from the frame before, as mask_prev
    d = os.path.join(tmp, "dump_b")
    os.makedirs(d)
    r = run_exe(src, head + [dict(keys, type="motion_seg", **mp), dict(keys, type="temporal_fusion", use_motion=True, **fp)], tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    prev, labels, masked = None, [], 0
    for f in range(n):
        if carried[f]:
            flow = O.block_flow(images[f][0], images[f - 1][0], 4, 2)
            labels.append(NM.segment(NM.camera(**keys), NM.params(**mp), rels[f], disps[f], disps[f - 1], flow)["labels"])
        else:
            labels.append(NM.unknown_frame(h, w)["labels"])
        ref = F.update(fcam, F.params(**fp), rels[f], disps[f], prev if carried[f] else None, labels[f - 1] if carried[f] else None, labels[f])
        got = read_fused(os.path.join(d, f"{f + 1}_disparity_fused.bin"), w, h)
        for name in ("fused", "age", "source", "counts"):
            assert got[name].tobytes() == ref[name].tobytes(), f"use_motion, frame {f + 1}: {name}"
        if carried[f]:
            masked += int((ref["source"] != F.update(fcam, F.params(**fp), rels[f], disps[f], prev)["source"]).sum())
        prev = (ref["fused"], ref["age"])
    assert masked > 0                                                     # the masks changed the outcome somewhere

    # configuration errors name their key
    for bad, word in ((dict(type="temporal_fusion"), "fx"), (dict(keys, type="temporal_fusion", splat_radius=1.0), "splat_radius"),
                      (dict(keys, type="temporal_fusion", max_weight=0), "max_weight"), (dict(keys, type="temporal_fusion", min_age=256), "min_age"),
                      (dict(keys, type="temporal_fusion", agree_threshold=0.0), "agree_threshold"), (dict(keys, type="temporal_fusion", min_disparity=-1.0), "min_disparity")):
        r = run_exe(src, head + [bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    r = run_exe(src, head + [dict(keys, type="temporal_fusion", use_motion=True)], tmp)
    assert r.returncode != 0 and 'requires "motion"' in r.stderr, r.stderr
    r = run_exe(src, head + [dict(keys, type="temporal_fusion", pose_key="dense_ego")], tmp)
    assert r.returncode != 0 and 'requires "dense_ego"' in r.stderr, r.stderr
    r = run_exe(src, head + [dict(keys, type="plane_map", disparity_key="disparity_fused", **grid)], tmp)
    assert r.returncode != 0 and 'requires "disparity_fused"' in r.stderr, r.stderr

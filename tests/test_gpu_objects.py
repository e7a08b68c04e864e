"""GPU tests of the moving-object tracks (spec S31): cart_object_tracker_update against the numpy restatement
tests/np_objects.py, byte for byte on pitched buffers, and the moving_objects host module in the C++ frame loop.  Beside every byte
comparison stands a numeric premise on the restatement (objects, points, flow points and gate rejections that must occur), so that no
comparison passes on an empty case."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import np_motion as M
import np_objects as OB
import test_motion_spec as S
import test_objects_spec as T
from test_gpu_motion import cam_tuple, engine, pitched

pytestmark = pytest.mark.gpu

CAM = T.CAM
POSE = S.yaw_rel(25.0, (3.0, -1.0, 7.0))
SHAPES = [(5, 3), (67, 5), (130, 33), (257, 17), (300, 70)]


def _torch():
    import torch
    return torch


class Pair:
    """A device tracker and its restated twin, fed the same frames."""

    def __init__(self, max_w, max_h, max_objects=16, max_tracks=8):
        from cartslam import ObjectTracker
        engine()
        self.dev = ObjectTracker(engine(), max_w, max_h, max_objects, max_tracks)
        self.ref = OB.Tracker(max_objects, max_tracks)

    def run(self, cam, p, rel, pose, ids, table, n, dc, dp, fl, stream=None, objects=True):
        """One frame on pitched inputs whose slack holds the first object's id and disparities that pass every gate -> (device result, restated result)."""
        torch = _torch()
        from cartslam import object_params
        ref = self.ref.update(cam, p, rel, pose, ids, table, n, dc, dp, fl)
        moving = table[:max(min(n, len(table)), 0)]
        slack_id = int(moving[moving[:, 1] == 1][0, 0]) if (moving[:, 1] == 1).any() else 0
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            args = (pitched(ids, 3, slack_id), torch.from_numpy(np.ascontiguousarray(table)).cuda(), torch.tensor([n], dtype=torch.int32).cuda(),
                    pitched(dc, 3, 256), pitched(dp, 5, 256), pitched(fl, 2, 0))
        out = self.dev.update(cam_tuple(cam), rel, pose, *args, params=object_params(**p), raw=True, stream=stream)
        return out, ref

    def close(self):
        self.dev.close()


def same(out, ref):
    _torch().cuda.synchronize()
    got = (out.objects.cpu().numpy().view(OB.OBJECT_DTYPE), out.tracks.cpu().numpy().view(OB.TRACK_DTYPE), out.counts.cpu().numpy())
    assert got[2].tolist() == ref["counts"].tolist(), dict(zip(OB.COUNTS, zip(got[2].tolist(), ref["counts"].tolist())))
    for name, a, b in (("objects", got[0], ref["objects"]), ("tracks", got[1], ref["tracks"])):
        assert a.shape == b.shape, name
        if a.tobytes() != b.tobytes():
            k = int(np.flatnonzero([a[i].tobytes() != b[i].tobytes() for i in range(len(a))])[0])
            raise AssertionError(f"{name}[{k}] differs:\n device {a[k]}\n spec   {b[k]}")
    return ref


def check(cam, p, rel, pose, ids, table, n, dc, dp, fl, max_objects=16, max_tracks=8, frames=1):
    """`frames` times the same frame through a fresh pair (the second time every valid object is a match or a miss of its own track)."""
    h, w = dc.shape
    pair = Pair(w, h, max_objects, max_tracks)
    try:
        for _ in range(frames):
            ref = same(*pair.run(cam, p, rel, pose, ids, table, n, dc, dp, fl))
    finally:
        pair.close()
    return ref


@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_on_pitched_buffers(w, h):
    """Below, at and above one block, one wave and one row strip, with random components, disparities around the band's edges and flows of
    both signs; twice, so that the second frame matches tracks."""
    small = (w, h) == (5, 3)
    p = OB.params(**dict(T.RANDOM_PARAMS, min_area=2 if small else 8, min_points=1 if small else 4, gate=1.0))
    seed = 7 * w + h
    while True:   # the first seed whose frame has an object with points (decided on the restatement alone)
        ids, table, n, dc, dp, fl = T.random_case(seed, w, h, cells=(3, 2) if small else (13, 7))
        probe = OB.measure(CAM, p, OB.IDENTITY, POSE, ids, table, n, dc, dp, fl, 16)
        if probe[0]["valid"].sum() > 0:
            break
        seed += 1
    ref = check(CAM, p, OB.IDENTITY, POSE, ids, table, n, dc, dp, fl, frames=2)
    assert ref["counts"][3] > 0 and ref["counts"][7] > 0
    if w >= 130:
        T.premises(ref["info"])
        assert ref["counts"][4] > 0 and ref["objects"]["has_velocity"].sum() > 0
    if w == 300:
        assert ref["counts"][1] > 16 == ref["counts"][2] and ref["counts"][6] > 0     # more objects than records, more valid ones than track slots


def test_large_flows_and_a_yawed_pose():
    w, h = 130, 33
    ids, table, n, dc, dp, fl = T.random_case(11 * w + h, w, h, big_flow=True)
    p = OB.params(**dict(T.RANDOM_PARAMS, max_speed=2.0))
    ref = check(CAM, p, S.yaw_rel(-0.3, (-0.01, -0.005, -0.1)), POSE, ids, table, n, dc, dp, fl)
    T.premises(ref["info"])
    ref = check(CAM, p, S.yaw_rel(170.0, (0.5, -0.2, -1.0)), POSE, ids, table, n, dc, dp, fl)      # nearly every point behind the camera
    assert ref["info"]["gate234"] > ref["info"]["points"] // 2 and ref["counts"][3] > 0


def whole_image_case(w, h, seed=3):
    dc, dp, fl, _ = S.random_frame(seed, w, h)
    ids, table, n = T.components(h, w, [(np.ones((h, w), bool), 1)])
    return ids, table, n, dc, dp, fl


def test_one_component_covering_the_whole_image():
    """Every pixel adds to one histogram and one accumulator: the most contention a destination can get."""
    w, h = 300, 70
    ref = check(CAM, OB.params(disparity_band=1.0, max_speed=0.3), OB.IDENTITY, POSE, *whole_image_case(w, h))
    o = ref["objects"][0]
    assert ref["counts"][:4].tolist() == [1, 1, 1, 1] and o["area"] == w * h and o["n_hist"] > w * h // 2 and o["n_points"] > w * h // 4 and o["n_flow"] > 1000
    assert (o["x0"], o["y0"], o["x1"], o["y1"]) == (0, 0, w - 1, h - 1)
    T.premises(ref["info"])
    # a flat image: one bin, one run per wave and strip
    dc, dp, fl = S.flat(h, w, 512, 512, flow=(32, 0))
    ids, table, n = T.components(h, w, [(np.ones((h, w), bool), 1)])
    ref = check(CAM, OB.params(), OB.IDENTITY, POSE, ids, table, n, dc, dp, fl)
    assert ref["objects"][0]["n_points"] == w * h and ref["objects"][0]["n_flow"] == (w - 1) * h


def test_two_components_interleaved_column_by_column():
    """Neighbouring lanes never share an object, so every run is one lane wide."""
    w, h = 130, 33
    dc, dp, fl, _ = S.random_frame(5, w, h)
    x = np.indices((h, w))[1]
    ids, table, n = T.components(h, w, [(x % 2 == 0, 1), (x % 2 == 1, 1)])
    ref = check(CAM, OB.params(disparity_band=1.0, max_speed=0.3), OB.IDENTITY, POSE, ids, table, n, dc, dp, fl)
    assert ref["objects"]["component"][:2].tolist() == [0, 1] and (ref["objects"]["n_points"][:2] > 500).all() and (ref["objects"]["n_flow"][:2] > 100).all()
    assert (ref["objects"]["x0"][:2].tolist(), ref["objects"]["x1"][:2].tolist()) == ([0, 1], [w - 2, w - 1])
    T.premises(ref["info"])


def test_an_object_wider_than_a_block_and_taller_than_a_strip_beside_others():
    w, h = 300, 70
    dc, dp, fl, _ = S.random_frame(9, w, h)
    regions = [(T.rect(h, w, 10, 3, 290, 60), 1), (T.rect(h, w, 0, 0, 299, 1), 0), (T.rect(h, w, 0, 3, 8, 69), 1), (T.rect(h, w, 20, 62, 280, 69), 1),
               (T.rect(h, w, 292, 3, 299, 69), 1)]
    ids, table, n = T.components(h, w, regions)
    ref = check(CAM, OB.params(disparity_band=1.0, max_speed=0.3), OB.IDENTITY, POSE, ids, table, n, dc, dp, fl)
    assert ref["counts"][:4].tolist() == [5, 4, 4, 4]
    big = ref["objects"][1]
    assert big["area"] == 281 * 58 and (big["x0"], big["y0"], big["x1"], big["y1"]) == (10, 3, 290, 60) and big["n_flow"] > 1000
    T.premises(ref["info"])


def test_an_object_with_every_disparity_invalid():
    w, h = 130, 33
    dc, dp, fl, _ = S.random_frame(13, w, h)
    a, b = T.rect(h, w, 5, 2, 70, 20), T.rect(h, w, 80, 5, 120, 30)
    dc[a] = -32768
    dc[3, 6] = 15
    ids, table, n = T.components(h, w, [(a, 1), (b, 1)])
    ref = check(CAM, OB.params(), OB.IDENTITY, POSE, ids, table, n, dc, dp, fl, frames=2)
    o = ref["objects"][0]
    assert (o["median_bin"], o["n_hist"], o["n_points"], o["valid"], o["x1"], o["y1"]) == (-1, 0, 0, 0, -1, -1) and ref["objects"][1]["valid"] == 1
    assert ref["counts"].tolist() == [2, 2, 2, 1, 1, 0, 0, 1]


def test_more_selected_components_than_objects_and_a_truncated_table():
    w, h = 257, 17
    ids, table, n, dc, dp, fl = T.random_case(21, w, h)
    p = OB.params(**T.RANDOM_PARAMS)
    ref = check(CAM, p, OB.IDENTITY, POSE, ids, table, n, dc, dp, fl, max_objects=4, max_tracks=2)
    assert ref["counts"][1] > 4 == ref["counts"][2] and ref["counts"][6] > 0
    # n_components > max_components: the walk ends with the table, and the pixels of the roots without an entry belong to no object
    full = OB.measure(CAM, p, OB.IDENTITY, POSE, ids, table, n, dc, dp, fl, 16)
    short = np.ascontiguousarray(table[:9])
    ref = check(CAM, p, OB.IDENTITY, POSE, ids, short, n, dc, dp, fl)
    assert n > 9 and ref["counts"][0] == 9 and 0 < ref["counts"][1] < full[1] and ref["info"]["pixels"] < full[3]["pixels"]
    # a count below the table's rows: the filler rows past it would be selected, and are not walked
    ref = check(CAM, p, OB.IDENTITY, POSE, ids, table, 5, dc, dp, fl)
    assert ref["counts"][0] == 5 and ref["counts"][1] == OB.select(table, 5, p, 16)[1] < full[1]
    ref = check(CAM, p, OB.IDENTITY, POSE, ids, table, -1, dc, dp, fl)
    assert ref["counts"].tolist() == [0] * 8


def gpu_components(labels, max_components=4096):
    """cart_plane_ccl_table on a label image -> (ids, table, count) as host arrays: the input the tracker has in the pipeline."""
    torch = _torch()
    ids, table, n = engine_for(labels.shape).plane_ccl_table(torch.from_numpy(labels).cuda(), max_components)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), table.cpu().numpy().reshape(max_components, 7), int(n.cpu().numpy()[0])


_ENGINES = {}


def engine_for(shape):
    from cartslam import Engine
    engine()
    if shape not in _ENGINES:
        _ENGINES[shape] = Engine(shape[1], shape[0], num_disparities=0, paths=0)
    return _ENGINES[shape]


def test_corridor_with_a_band_of_wrong_flow():
    """synth.road_corridor_motion at 320 x 96: the block that moves with the camera is an object with a velocity near the camera's step;
    the band whose flow is 200 pixels off forms a component whose points carry no flow, because |f| is far above max_speed."""
    from cartslam import synth
    cam = M.camera(721.5 * 320 / 1242, 721.5 * 320 / 1242, 160.0, 44.0, 0.54)
    rel, dc, dp, fl, planes, block = synth.road_corridor_motion(320, 96, *cam_tuple(cam))
    labels = M.segment(cam, M.params(), rel, dc, dp, fl)["labels"]
    ids, table, n = gpu_components(labels)
    exp_table, exp_n = OB.component_table(labels, ids, 4096)
    assert n == exp_n and (table[:n] == exp_table[:n]).all()
    table[n:] = 0                                                     # the rows past the count are undefined: pin them for the restatement
    ref = check(cam, OB.params(), rel, POSE, ids, table, n, dc, dp, fl, max_objects=32)
    objs = ref["objects"][:ref["counts"][2]]
    band = objs[(objs["y0"] >= 96 - 35 - 2) & (objs["y1"] <= 96 - 26 + 2) & (objs["x0"] >= 198) & (objs["valid"] == 1) & (objs["has_velocity"] == 0)]   # the filter's radius is 2
    assert len(band) >= 1 and band["n_points"].max() >= 16 and ref["info"]["speed"] > 100
    car = objs[(objs["x0"] >= 2 * 320 // 5 - 2) & (objs["x1"] <= 2 * 320 // 5 + 320 // 9 + 2) & (objs["has_velocity"] == 1)]
    assert len(car) == 1 and car[0]["median_bin"] == 24 and car[0]["n_flow"] > 300


def test_full_size_frame_and_two_trackers_on_two_streams():
    torch = _torch()
    from test_gpu_motion import corridor
    cam, rel, dc, dp, fl, planes, block, seg = corridor()
    ids, table, n = gpu_components(seg["labels"])
    table[n:] = 0
    h, w = dc.shape
    p = OB.params(max_speed=0.75)   # the block moves with the camera: |f| = the step of 0.5 m; the band's 200 pixels of wrong flow are 0.8 m and more on the near road
    a, b = Pair(w, h, 64, 32), Pair(w, h, 64, 32)
    try:
        ref = same(*a.run(cam, p, rel, POSE, ids, table, n, dc, dp, fl))
        assert ref["counts"][2] >= 2 and ref["counts"][3] >= 2 and ref["info"]["points"] > 5000 and ref["info"]["flow"] > 5000 and ref["info"]["speed"] > 1000
        assert ref["info"]["band"] > 1000 and sorted(ref["objects"]["has_velocity"][:2].tolist()) == [0, 1]
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        outs = []
        for k in range(2):                                            # side by side: a's second and third frame, b's first and second
            outs.append(a.run(cam, p, rel, POSE, ids, table, n, dc, dp, fl, stream=sa))
            outs.append(b.run(cam, p, rel, POSE, ids, table, n, dc, dp, fl, stream=sb))
        for out, exp in outs:
            same(out, exp)
        assert outs[-1][1]["counts"][4] > 0 and outs[0][1]["tracks"].tobytes() != outs[1][1]["tracks"].tobytes()
    finally:
        a.close()
        b.close()


def sequence_frame(x0, present=True, d=512):
    """32 x 16: a 6 x 6 square at column x0 with disparity d / 16 that came from one pixel further left, or no component at all."""
    h, w = 16, 32
    sq = T.rect(h, w, x0, 4, x0 + 5, 9)
    ids, table, n = T.components(h, w, [(sq, 1)] if present else [(T.rect(h, w, 0, 0, 3, 3), 0)])
    dc, dp, fl = S.flat(h, w, 256, 256)
    dc[sq] = d
    dp[T.rect(h, w, x0 - 1, 4, x0 + 4, 9)] = d
    fl[sq, 0] = 32
    return ids, table, n, dc, dp, fl


def test_a_sequence_with_a_birth_a_miss_a_death_and_a_reset():
    p = OB.params(min_area=16, max_missed=1, min_age=2, gain_percent=50)
    pair = Pair(32, 16, 4, 4)
    try:
        steps = [(sequence_frame(8), [1, 1, 1, 1, 0, 1, 0, 1]), (sequence_frame(9), [1, 1, 1, 1, 1, 0, 0, 1]), (sequence_frame(9, False), [1, 0, 0, 0, 0, 0, 0, 1]),
                 (sequence_frame(11), [1, 1, 1, 1, 1, 0, 0, 1]), (sequence_frame(9, False), [1, 0, 0, 0, 0, 0, 0, 1]), (sequence_frame(9, False), [1, 0, 0, 0, 0, 0, 0, 0]),
                 (sequence_frame(20), [1, 1, 1, 1, 0, 1, 0, 1])]
        states = []
        for frame, counts in steps:
            ref = same(*pair.run(CAM, p, OB.IDENTITY, OB.IDENTITY, *frame))
            assert ref["counts"].tolist() == counts
            states.append(ref["tracks"][0].copy())
        assert [int(t["id"]) for t in states] == [1, 1, 1, 1, 1, 0, 2] and [int(t["state"]) for t in states] == [1, 2, 2, 2, 2, 0, 1]
        assert [int(t["missed"]) for t in states] == [0, 0, 1, 0, 1, 0, 0] and [int(t["age"]) for t in states] == [1, 2, 2, 3, 3, 0, 1]
        assert states[2]["position"][0] == states[1]["position"][0] + states[1]["velocity"][0]       # the miss coasts
        # reset: every slot free, ids from 1 again
        pair.dev.reset()
        pair.ref.reset()
        ref = same(*pair.run(CAM, p, OB.IDENTITY, OB.IDENTITY, *sequence_frame(8)))
        assert ref["tracks"][0]["id"] == 1 and ref["counts"].tolist() == [1, 1, 1, 1, 0, 1, 0, 1]
        # objects_out = NULL: the tracks and counts come all the same
        torch = _torch()
        from cartslam import _lib, object_params
        ids, table, n, dc, dp, fl = sequence_frame(9)
        exp = pair.ref.update(CAM, p, OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl)
        t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (ids, table, np.array([n], np.int32), dc, dp, fl)]
        tracks, counts = torch.zeros(4 * 12, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
        cam, op, ident = _lib.EgoCamera(*cam_tuple(CAM)), object_params(**p), (C.c_double * 12)(*OB.IDENTITY)
        rc = _lib.load().cart_object_tracker_update(pair.dev._h, C.byref(cam), ident, ident, C.byref(op), t[0].data_ptr(), 4 * 32, t[1].data_ptr(), 64, t[2].data_ptr(),
                                                    t[3].data_ptr(), 2 * 32, t[4].data_ptr(), 2 * 32, t[5].data_ptr(), 4 * 32, 32, 16, None, tracks.data_ptr(),
                                                    counts.data_ptr(), None)
        assert rc == 0, _lib.load().cart_last_error(None).decode()
        torch.cuda.synchronize()
        assert tracks.cpu().numpy().tobytes() == exp["tracks"].tobytes() and counts.cpu().numpy().tolist() == exp["counts"].tolist() == [1, 1, 1, 1, 1, 0, 0, 1]
    finally:
        pair.close()


def test_host_arrays_defaults_and_the_lifecycle():
    from cartslam import Engine, EngineError, ObjectTracker
    engine()
    ids, table, n, dc, dp, fl = T.hand_case()
    with ObjectTracker(engine(), 16, 8) as tr:
        out = tr.update(cam_tuple(CAM), OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl)     # numpy in, numpy out, the default parameters: min_area 64 > 16
        assert out.objects.dtype == OB.OBJECT_DTYPE and out.tracks.dtype == OB.TRACK_DTYPE and out.objects.shape == (64,) and out.tracks.shape == (64,)
        assert out.counts.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and out.tracks.tobytes() == OB.free_tracks(64).tobytes()
        with pytest.raises(EngineError, match="exceeds the object's 16 x 8"):
            tr.update(cam_tuple(CAM), OB.IDENTITY, OB.IDENTITY, *T.random_case(1, 23, 9))
        with pytest.raises(EngineError, match="pose"):
            tr.update(cam_tuple(CAM), OB.IDENTITY, [float("nan")] * 12, ids, table, n, dc, dp, fl)
        with pytest.raises(EngineError, match="flow"):
            tr.update(cam_tuple(CAM), OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl[:, :, :1])
    assert tr._h is None
    with pytest.raises(Exception):
        tr.update(cam_tuple(CAM), OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl)           # a closed object
    tr.close()                                                                                   # twice is once
    # destroy after the engine
    eng = Engine(16, 8, num_disparities=0, paths=0)
    tr = ObjectTracker(eng, 16, 8, 2, 2)
    eng.close()
    tr.close()
    with pytest.raises(EngineError, match="max_objects"):
        ObjectTracker(engine(), 16, 8, 257, 2)


def test_bad_arguments_touch_no_output_and_no_track():
    torch = _torch()
    from cartslam import _lib, object_params
    lib = _lib.load()
    p = OB.params(min_area=16)
    pair = Pair(32, 16, 4, 4)
    try:
        same(*pair.run(CAM, p, OB.IDENTITY, OB.IDENTITY, *sequence_frame(8)))               # one live track to lose
        ids, table, n, dc, dp, fl = sequence_frame(9)
        w, h = 32, 16
        t = dict(zip(("ids", "table", "n_components", "disp_cur", "disp_prev", "flow"), (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (ids, table, np.array([n], np.int32), dc, dp, fl))))
        objects, tracks = torch.full((4 * 24,), 77.0, dtype=torch.float64, device="cuda"), torch.full((4 * 12,), 77.0, dtype=torch.float64, device="cuda")
        counts = torch.full((8,), 77, dtype=torch.int32, device="cuda")
        cam, ident = _lib.EgoCamera(*cam_tuple(CAM)), (C.c_double * 12)(*OB.IDENTITY)
        base = dict(ids=(t["ids"].data_ptr(), 4 * w), table=t["table"].data_ptr(), max_components=64, n_components=t["n_components"].data_ptr(),
                    disp_cur=(t["disp_cur"].data_ptr(), 2 * w), disp_prev=(t["disp_prev"].data_ptr(), 2 * w), flow=(t["flow"].data_ptr(), 4 * w), size=(w, h),
                    objects_out=objects.data_ptr(), tracks_out=tracks.data_ptr(), counts_out=counts.data_ptr())

        def call(obj=True, params=None, **kw):
            a = dict(base, **kw)
            flat = []
            for k in ("ids", "table", "max_components", "n_components", "disp_cur", "disp_prev", "flow", "size", "objects_out", "tracks_out", "counts_out"):
                v = a[k]
                if k in ("max_components",):
                    flat.append(v)
                elif k == "size":
                    flat += list(v)
                elif isinstance(v, tuple):
                    flat += [C.c_void_p(v[0]), v[1]]
                else:
                    flat.append(C.c_void_p(v))
            rc = lib.cart_object_tracker_update(pair.dev._h if obj else None, C.byref(cam), ident, ident, C.byref(object_params(**(params or p))), *flat, None)
            return rc, lib.cart_last_error(None).decode()

        bad = [(dict(obj=False), "bad arguments"), (dict(size=(33, 16)), "exceeds the object's 32 x 16"), (dict(size=(32, 17)), "exceeds"), (dict(size=(0, 16)), "width"),
               (dict(params=dict(p, gate=0.0)), "gate"), (dict(max_components=0), "max_components")]
        for k, elem in (("ids", 4), ("disp_cur", 2), ("disp_prev", 2), ("flow", 4)):
            ptr, step = base[k]
            bad += [({k: (None, step)}, k + " is NULL"), ({k: (ptr + 1, step)}, k + " and its step must be"), ({k: (ptr, step + 1)}, k + " and its step must be"),
                    ({k: (ptr, step - elem)}, k + "_step is below the row size")]
        for k, elem in (("table", 4), ("n_components", 4), ("tracks_out", 8), ("counts_out", 4)):
            bad += [({k: None}, k + " is NULL"), ({k: base[k] + 1}, f"{k} must be {elem}-byte aligned")]
        bad += [(dict(objects_out=base["objects_out"] + 4), "objects_out must be 8-byte aligned"), (dict(tracks_out=base["tracks_out"] + 4), "tracks_out must be 8-byte aligned"),
                # no output may lie on another output or on an input
                (dict(tracks_out=base["objects_out"]), "objects_out and tracks_out must not overlap"), (dict(counts_out=base["tracks_out"] + 4 * 96 - 4), "tracks_out and counts_out must not overlap"),
                (dict(counts_out=base["objects_out"]), "objects_out and counts_out must not overlap"), (dict(counts_out=base["ids"][0]), "ids and counts_out must not overlap"),
                (dict(counts_out=base["table"] + 28 * 63), "table and counts_out must not overlap"), (dict(counts_out=base["n_components"]), "n_components and counts_out must not overlap"),
                (dict(counts_out=base["disp_cur"][0] + 2 * w * h - 4), "disp_cur and counts_out must not overlap"), (dict(counts_out=base["disp_prev"][0]), "disp_prev and counts_out must not overlap"),
                (dict(counts_out=base["flow"][0]), "flow and counts_out must not overlap")]
        for kw, word in bad:
            rc, err = call(**kw)
            assert rc != 0 and word in err, (kw, err)
        torch.cuda.synchronize()
        assert bool((objects == 77.0).all()) and bool((tracks == 77.0).all()) and bool((counts == 77).all())     # no refused call touched an output
        rc, err = call()                                                                     # ... or a track: the next frame matches the track of the first
        assert rc == 0, err
        torch.cuda.synchronize()
        exp = pair.ref.update(CAM, p, OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl)
        assert exp["counts"].tolist() == [1, 1, 1, 1, 1, 0, 0, 1] == counts.cpu().numpy().tolist()
        assert tracks.cpu().numpy().tobytes() == exp["tracks"].tobytes() and objects.cpu().numpy().tobytes() == exp["objects"].tobytes()
    finally:
        pair.close()


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------
def read_moving_objects(path):
    raw = open(path, "rb").read()
    counts = np.frombuffer(raw, "<i4", 8)
    n_obj, n_live = int(counts[2]), int(counts[7])
    assert len(raw) == 32 + 192 * n_obj + 96 * n_live, path
    return counts, np.frombuffer(raw, OB.OBJECT_DTYPE, n_obj, 32), np.frombuffer(raw, OB.TRACK_DTYPE, n_live, 32 + 192 * n_obj)


def test_moving_objects_module_in_the_frame_loop(tmp_path):
    """The dump of every frame equals the restatement fed with that frame's dumped inputs (components, table, count, disparities, flow,
    poses), the tracker carried from frame to frame and dropped where the module drops it."""
    from test_gpu_matches import noise_frame, noise_world
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n, w, h = 4, 320, 96
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
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    mp = dict(flow_threshold=1.0, disparity_threshold=0.25, radius=1, support_percent=40)      # tight thresholds: the static world's noise gives MOVING specks
    op = dict(min_area=6, min_points=3, max_speed=1.0, gate=1.5, min_age=2, max_missed=1, gain_percent=30, disparity_band=1.5, min_disparity=2.0)
    modules = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
               {"type": "optflow", "search_radius": 4}, {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion"),
               dict(keys, type="motion_seg", **mp), dict(keys, type="moving_objects", max_objects=32, max_tracks=16, **op)]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, modules, tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    cam, p = M.camera(**keys), OB.params(**op)
    ref = OB.Tracker(32, 16)
    estimates = objects = valid = matched = 0
    for f in range(n):
        ego = np.fromfile(os.path.join(d, f"{f + 1}_ego_motion.bin"), np.float64)
        status = int(np.frombuffer(ego[13:14].tobytes(), "<i4")[0])
        counts, objs, tracks = read_moving_objects(os.path.join(d, f"{f + 1}_moving_objects.bin"))
        if f == 0 or status == 0:
            ref.reset()
            assert counts.tolist() == [0] * 8 and len(objs) == 0 and len(tracks) == 0
            continue
        estimates += 1
        load = lambda name, dtype, frame=f + 1: np.fromfile(os.path.join(d, f"{frame}_{name}.bin"), dtype)   # noqa: E731
        rel = np.concatenate([ego[0:9].reshape(3, 3), ego[9:12].reshape(3, 1)], axis=1).reshape(12)
        exp = ref.update(cam, p, rel, ego[15:], load("motion_components", np.int32).reshape(h, w), load("motion_component_table", np.int32).reshape(4096, 7),
                         int(load("motion_component_count", np.int32)[0]), load("disparity", np.int16).reshape(h, w), load("disparity", np.int16, f).reshape(h, w),
                         load("optflow", np.int16).reshape(h, w, 2))
        assert counts.tolist() == exp["counts"].tolist(), f"frame {f + 1}"
        assert objs.tobytes() == exp["objects"][:counts[2]].tobytes(), f"frame {f + 1}: objects"
        assert tracks.tobytes() == exp["tracks"][exp["tracks"]["state"] != 0].tobytes(), f"frame {f + 1}: tracks"
        objects, valid, matched = objects + int(counts[2]), valid + int(counts[3]), matched + int(counts[4])
    print(f"{estimates} frames with an estimate: {objects} objects, {valid} valid, {matched} matched")
    assert estimates >= 2 and objects >= 1 and valid >= 1
    # configuration errors name their key
    head = modules[:6]
    for bad, word in ((dict(type="moving_objects"), "fx"), (dict(keys, type="moving_objects", gate=0.0), "gate"), (dict(keys, type="moving_objects", disparity_band=0.25), "disparity_band"),
                      (dict(keys, type="moving_objects", min_age=0), "min_age"), (dict(keys, type="moving_objects", max_objects=257), "max_objects"),
                      (dict(keys, type="moving_objects", pose_key="pose_graph"), "pose_graph")):
        r = run_exe(src, head + [bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    r = run_exe(src, modules[:5] + [dict(keys, type="motion_seg", components=False), dict(keys, type="moving_objects")], tmp)
    assert r.returncode != 0 and 'requires "motion_components"' in r.stderr, r.stderr
    r = run_exe(src, head + [dict(keys, type="moving_objects", pose_key="dense_ego")], tmp)
    assert r.returncode != 0 and 'requires "dense_ego"' in r.stderr, r.stderr

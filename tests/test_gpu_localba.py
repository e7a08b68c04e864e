"""GPU tests of the windowed bundle adjustment (spec S32): after every push and every optimise the poses, the frame ids,
every point slot, track_of, the counts and the result record equal the numpy restatement (tests/np_localba.py) byte for byte -- over the
keypoint counts, windows, table sizes and active-point counts at which each kernel can go wrong, the object's state in call order, the
failed pivot and the argument checks.

The kernels as built: the compactions of a push run in one workgroup of 1024 threads (rounds of 1024 slots / features); the sums over
the point slots run in workgroups of 256 lanes = S23's virtual lanes, so 255 / 256 / 257 / 513 active points are the edges."""
import ctypes as C

import numpy as np
import pytest

import np_ego as E
import np_localba as B
import test_localba_spec as S

pytestmark = pytest.mark.gpu


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


def make(max_features, window, max_points, eng=None):
    from cartslam import LocalBA
    return LocalBA(eng or engine(), max_features, window, max_points), B.Window(max_features, window, max_points)


def c_params(p):
    from cartslam import local_ba_params
    return local_ba_params(**p)


def same_state(ba, win):
    poses, ids = ba.poses()
    want, want_ids = win.poses()
    assert ba.size() == (win.frames(), win.max_points)
    assert ids.tobytes() == want_ids.tobytes(), (ids, want_ids)
    assert poses.tobytes() == want.tobytes(), f"poses: largest difference {np.abs(poses - want).max()}"
    pts, wpts = ba.points(), win.points()
    assert pts.tobytes() == wpts.tobytes(), f"points: {int((pts != wpts).any(axis=1).sum())} slots differ, largest difference {np.abs(pts - wpts).max()}"
    assert ba.track_of().tobytes() == win.track_of.tobytes()


def push_both(ba, win, cam, p, fid, f):
    got = ba.push(cam_tuple(cam), fid, f["odom"], f["kpL"], f["kpR"], f["stereo"], f["temporal"], params=c_params(p))
    want = win.push(cam, p, fid, f["odom"], f["kpL"], f["kpR"], f["stereo"], f["temporal"])
    assert got.tobytes() == want.tobytes(), (got, want)
    same_state(ba, win)
    return want


def optimize_both(ba, win, cam, p):
    got = ba.optimize(cam_tuple(cam), params=c_params(p))
    with np.errstate(all="ignore"):
        want = win.optimize(cam, p)
    assert got.tobytes() == want.tobytes(), (got, want)
    same_state(ba, win)
    return want[0]


def run(frames, window, max_points, p=None, cam=S.CAM, max_features=None, optimise="last"):
    """Pushes the frames into a device object and the restatement side by side; optimise = "each", "last", None, or the number of the
    first push that is followed by one."""
    p = p or B.params()
    ba, win = make(max_features or max(len(f["kpL"]) for f in frames) + 1, window, max_points)
    counts, res = [], None
    for k, f in enumerate(frames):
        counts.append(push_both(ba, win, cam, p, k + 1, f))
        if optimise == "each" or (optimise == "last" and k + 1 == len(frames)) or (isinstance(optimise, int) and k + 1 >= optimise):
            res = optimize_both(ba, win, cam, p)
    ba.close()
    return counts, res, win


DRIVE = {}


def drive(n_frames=11, n_points=1400):
    """One synthetic drive shared by the tests that cut it to size (never modified)."""
    if (n_frames, n_points) not in DRIVE:
        DRIVE[n_frames, n_points] = B.drive(41, n_frames, n_points, S.CAM, step=0.3, yaw_deg=1.0)
    return DRIVE[n_frames, n_points]


# ---- keypoint counts, windows, the sequence past the ring's size --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65, 257, 1000])
def test_keypoint_counts(n):
    """max_features one above the count; the premise: the drive's frames hold at least n keypoints each (1000 only: at least 900)."""
    frames = S.truncate(drive()[:4], n)
    assert min(len(f["kpL"]) for f in frames) >= min(n, 900)
    counts, res, _ = run(frames, 3, 2048, max_features=max(len(f["kpL"]) for f in frames) + 1)
    assert counts[-1][0] == len(frames[-1]["kpL"]) and res["status"] == 1
    if n >= 65:
        assert res["n_points_active"] > 0 and res["cost_after"] < res["cost_before"]


@pytest.mark.parametrize("window", [2, 3, 8, 16])
def test_window_sizes_past_the_ring(window):
    """W + 3 pushes with an optimise after each (window 16: after each from the 14th on, which keeps the restatement's share of the test
    to a few seconds): the ring wraps, frames leave, their points are freed and the slots reused."""
    frames = S.truncate(B.drive(42 + window, window + 3, 260, S.CAM, step=0.8, yaw_deg=3.0), 120)
    counts, res, win = run(frames, window, 512, optimise="each" if window < 16 else 14)
    assert sum(int(c[5]) for c in counts) > 0 and counts[-1][7] == window      # points were freed; the ring is full
    assert res["status"] == 1 and res["n_frames"] == window
    n_obs = win.n_obs[win.state != 0]
    assert n_obs.max() == window and (n_obs == 2).any()                         # a point seen in every frame and one seen twice


def test_more_births_than_slots():
    frames = S.truncate(drive()[:3], 150)
    counts, res, win = run(frames, 3, 64, optimise="each")
    assert counts[0][3] == 64 and counts[0][4] > 0 and counts[0][6] == 64       # born, dropped, live
    assert (win.track_of[:150] == -1).any()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_active_point_counts(n):
    """Exactly n points, every one seen by every frame: the edges of the 256 virtual lanes."""
    frames = S.rigid(n, 3, seed=50 + n)
    p = B.params(min_frame_observations=1)
    counts, res, _ = run(frames, 3, 576, p=p)
    assert res["n_points_active"] == n and res["n_observations"] == 3 * n
    assert res["status"] == (0 if n == 1 else 1)                                # one point cannot fix the poses: the restatement's pivot fails


# ---- the edge cases of a step -----------------------------------------------------------------------------------------------------------
def test_a_held_frame():
    frames = S.starved(S.truncate(drive()[:4], 200), 3, keep=3)
    _, res, _ = run(frames, 4, 1024, p=B.params(iterations=2))
    assert res["status"] == 1 and res["n_held"] == 2                            # the newest frame, in both steps


@pytest.mark.parametrize("yaw, status", [(100.0, 1), (80.0, 0)])
def test_observations_behind_the_camera(yaw, status):
    """Frame 2's pose is turned by `yaw` degrees, so a share of its observations has q.z <= 0.  The restatement decides the outcome: at
    100 degrees the steps go through, at 80 degrees a pivot of the 18 x 18 reduced system is not > 0 and nothing moves."""
    frames = S.turned(S.truncate(drive()[:4], 200), 2, yaw)
    _, res, win = run(frames, 4, 1024)
    act = win.active(B.params())
    seen = sum(int(((win.obs["valid"][:, s] != 0) & act).sum()) for s in range(4))
    assert res["status"] == status and 0 < res["n_observations"] < seen


@pytest.mark.parametrize("p", [dict(iterations=0), dict(iterations=16), dict(damping=1e-3), dict(huber=0.5, min_observations=3)], ids=str)
def test_parameters(p):
    frames = S.truncate(drive()[:5], 300)
    _, res, _ = run(frames, 5, 1024, p=B.params(**p))
    assert res["status"] == 1 and res["iterations"] == B.params(**p)["iterations"]
    assert (res["cost_after"] == res["cost_before"]) == (p.get("iterations") == 0)


def test_a_failed_pivot_moves_nothing():
    """tests/test_localba_spec.py confirms the premise on the restatement: two frames that share one point meet a pivot that is not > 0."""
    frames, p = S.degenerate()
    ba, win = make(8, 2, 64)
    for k, f in enumerate(frames):
        push_both(ba, win, S.CAM, p, k + 1, f)
    before = (ba.poses()[0].tobytes(), ba.points().tobytes())
    res = optimize_both(ba, win, S.CAM, p)
    assert res["status"] == 0 and res["cost_after"] == res["cost_before"] and (ba.poses()[0].tobytes(), ba.points().tobytes()) == before
    ba.close()


def test_slack_rows_are_never_read():
    """Device lists longer than their counts, with rows past the counts that would pass every gate."""
    torch = _torch()
    frames = S.truncate(drive()[:3], 100)
    cap = 160
    ba, win = make(cap, 3, 512)
    p = B.params()
    for k, f in enumerate(frames):
        n = len(f["kpL"])
        kl, kr = np.zeros((cap, 7), np.float32), np.zeros((cap, 7), np.float32)
        kl[:n], kr[:n] = f["kpL"].view(np.float32).reshape(n, 7), f["kpR"].view(np.float32).reshape(n, 7)
        kl[n:, 0], kl[n:, 1], kr[n:, 0], kr[n:, 1] = 100.0, 50.0, 90.0, 50.0                      # a disparity of 10 pixels
        st, te = np.zeros((cap, 4), np.int32), np.zeros((cap, 4), np.int32)
        st[:len(f["stereo"])] = f["stereo"].view(np.int32).reshape(-1, 4)
        te[:len(f["temporal"])] = f["temporal"].view(np.int32).reshape(-1, 4)
        st[len(f["stereo"]):, 0] = st[len(f["stereo"]):, 1] = np.arange(len(f["stereo"]), cap)    # matches onto the slack keypoints
        te[len(f["temporal"]):, 0] = te[len(f["temporal"]):, 1] = np.arange(len(f["temporal"]), cap)
        dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
        cnt = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")   # noqa: E731
        got = ba.push(cam_tuple(S.CAM), k + 1, f["odom"], dev(kl), dev(kr), dev(st), dev(te), cnt(n), cnt(len(f["stereo"])), cnt(len(f["temporal"])), params=c_params(p))
        want = win.push(S.CAM, p, k + 1, f["odom"], f["kpL"], f["kpR"], f["stereo"], f["temporal"])
        assert got.tobytes() == want.tobytes()
        same_state(ba, win)
    optimize_both(ba, win, S.CAM, p)
    ba.close()


# ---- the object's state in call order ----------------------------------------------------------------------------------------------------
def test_two_objects_on_two_streams():
    torch = _torch()
    fa, fb = S.truncate(drive()[:4], 180), S.truncate(drive()[4:8], 140)
    p = B.params()
    (ba1, w1), (ba2, w2) = make(200, 3, 512), make(200, 4, 256)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    raw = []
    for k in range(4):
        for ba, st, f in ((ba1, s1, fa[k]), (ba2, s2, fb[k])):
            with torch.cuda.stream(st):
                ba.push(cam_tuple(S.CAM), k + 1, f["odom"], f["kpL"], f["kpR"], f["stereo"], f["temporal"], params=c_params(p), raw=True)
                raw.append(ba.optimize(cam_tuple(S.CAM), params=c_params(p), raw=True))
    with torch.cuda.stream(s2):             # the other stream: ordered behind the object's last call
        raw.append(ba1.optimize(cam_tuple(S.CAM), params=c_params(p), raw=True))
    want = []
    for k in range(4):
        for w, f in ((w1, fa[k]), (w2, fb[k])):
            w.push(S.CAM, p, k + 1, f["odom"], f["kpL"], f["kpR"], f["stereo"], f["temporal"])
            want.append(w.optimize(S.CAM, p))
    want.append(w1.optimize(S.CAM, p))
    torch.cuda.synchronize()
    for g, w in zip(raw, want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    same_state(ba1, w1)
    same_state(ba2, w2)
    ba1.close()
    ba2.close()


def test_clear_and_reuse():
    frames = S.truncate(drive()[:5], 150)
    p = B.params()
    ba, win = make(151, 3, 256)
    for k, f in enumerate(frames[:4]):
        push_both(ba, win, S.CAM, p, k + 1, f)
    optimize_both(ba, win, S.CAM, p)
    ba.clear()
    win.clear()
    same_state(ba, win)
    assert ba.size() == (0, 256) and not ba.points().any() and (ba.track_of() == -1).all()
    res = optimize_both(ba, win, S.CAM, p)                                       # an empty window: nothing to do
    assert res["status"] == 1 and res["n_frames"] == 0
    c = push_both(ba, win, S.CAM, p, 9, frames[4])                               # the first push after a clear ignores its temporal list
    assert len(frames[4]["temporal"]) > 0 and c[2] == 0 and c[3] == c[1]
    res = optimize_both(ba, win, S.CAM, p)                                       # one frame: nothing moves
    assert res["status"] == 1 and res["n_frames"] == 1 and res["n_points_active"] == 0
    ba.close()


def test_lifecycle():
    from cartslam import Engine, EngineError, LocalBA, local_ba_params
    other = Engine(64, 32, num_disparities=0, paths=0)
    ba, win = make(64, 2, 64, eng=other)
    frames = S.truncate(drive()[:2], 60)
    p = B.params()
    push_both(ba, win, S.CAM, p, 1, frames[0])
    other.close()                                                               # the object outlives its engine
    push_both(ba, win, S.CAM, p, 2, frames[1])
    optimize_both(ba, win, S.CAM, p)
    ba.close()
    assert ba._h is None
    ba.close()                                                                  # closing twice is harmless
    with pytest.raises(EngineError, match="ba is NULL"):                        # a closed object refuses every call by name
        ba.size()
    with pytest.raises(EngineError, match="ba is NULL"):
        ba.optimize(cam_tuple(S.CAM))
    for args, word in (((0, 8, 64), "max_features"), ((8, 1, 64), "window"), ((8, 17, 64), "window"), ((8, 8, 63), "max_points"), ((8, 8, 65537), "max_points")):
        with pytest.raises(EngineError, match=word):
            LocalBA(engine(), *args)
    with LocalBA(engine(), 8, 2, 64) as ba:
        with pytest.raises(EngineError, match="iterations"):
            ba.optimize(cam_tuple(S.CAM), params=local_ba_params(iterations=17))
        with pytest.raises(EngineError, match="huber"):
            ba.optimize(cam_tuple(S.CAM), huber=0.0)
    assert ba._h is None


def test_bad_arguments_name_the_argument_and_touch_nothing():
    torch = _torch()
    from cartslam import EgoCamera, local_ba_params
    frames = S.truncate(drive()[:3], 100)
    p = B.params()
    ba, win = make(128, 3, 256)
    for k, f in enumerate(frames[:2]):
        push_both(ba, win, S.CAM, p, k + 1, f)
    lib = ba._lib
    err = lambda: lib.cart_last_error(None).decode()   # noqa: E731
    cp, cam = local_ba_params(), EgoCamera(*cam_tuple(S.CAM))
    pose = (C.c_double * 12)(*frames[2]["odom"])
    buf = torch.zeros(128 * 7, dtype=torch.float32, device="cuda")
    ints = torch.full((128 * 4 + 16,), -7, dtype=torch.int32, device="cuda")
    one = torch.tensor([5], dtype=torch.int32, device="cuda")
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731

    def push(params=cp, camera=cam, pose_=pose, handle=None, kl=vp(buf), kr=vp(buf), lc=vp(one), sm=vp(ints), sc=vp(one), tm=vp(ints), tc=vp(one), out=None):
        return lib.cart_local_ba_push(ba._h if handle is None else handle, C.byref(camera) if camera else None, C.byref(params) if params else None, 3,
                                      pose_, kl, kr, lc, sm, sc, tm, tc, out, None)
    bad_cam = EgoCamera(0.0, 300.0, 1.0, 1.0, 0.5)
    bad_pose = (C.c_double * 12)(*([float("nan")] + list(frames[2]["odom"])[1:]))
    cases = [(dict(params=None), "params is NULL"), (dict(params=local_ba_params(min_disparity=0.0)), "min_disparity"), (dict(params=local_ba_params(damping=-1.0)), "damping"),
             (dict(params=local_ba_params(min_observations=0)), "min_observations"), (dict(params=local_ba_params(min_frame_observations=-1)), "min_frame_observations"),
             (dict(camera=None), "camera is NULL"), (dict(camera=bad_cam), "fx"), (dict(pose_=None), "pose is NULL"), (dict(pose_=bad_pose), "pose[0]"),
             (dict(handle=C.c_void_p(None)), "ba is NULL"), (dict(kl=None), "kpL is NULL"), (dict(kr=None), "kpR is NULL"), (dict(lc=None), "left_count is NULL"),
             (dict(sm=None), "stereo_matches is NULL"), (dict(sc=None), "stereo_count is NULL"), (dict(tm=None), "temporal_matches is NULL"),
             (dict(tc=None), "temporal_count is NULL"), (dict(kl=vp(buf, 2)), "kpL must be 4-byte aligned"), (dict(out=vp(ints, 2)), "counts_out must be 4-byte aligned"),
             (dict(out=vp(ints, 16)), "stereo_matches and counts_out must not overlap"), (dict(out=vp(one)), "left_count and counts_out must not overlap")]
    for kw, word in cases:
        assert push(**kw) != 0 and word in err(), (word, err())
    res = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    assert lib.cart_local_ba_optimize(ba._h, C.byref(cam), None, vp(res), None) != 0 and "params is NULL" in err()
    assert lib.cart_local_ba_optimize(ba._h, None, C.byref(cp), vp(res), None) != 0 and "camera is NULL" in err()
    assert lib.cart_local_ba_optimize(None, C.byref(cam), C.byref(cp), vp(res), None) != 0 and "ba is NULL" in err()
    assert lib.cart_local_ba_optimize(ba._h, C.byref(cam), C.byref(cp), vp(res, 4), None) != 0 and "result must be 8-byte aligned" in err()
    assert lib.cart_local_ba_poses(ba._h, None, None, None) != 0 and "out is NULL" in err()
    assert lib.cart_local_ba_poses(ba._h, vp(res, 4), None, None) != 0 and "out must be 8-byte aligned" in err()
    big = torch.zeros(3 * 12 + 3, dtype=torch.float64, device="cuda")
    assert lib.cart_local_ba_poses(ba._h, vp(big), vp(big, 8 * 35), None) != 0 and "out and ids_out must not overlap" in err()
    assert lib.cart_local_ba_points(ba._h, None, None) != 0 and "out is NULL" in err()
    assert lib.cart_local_ba_track_of(ba._h, vp(ints, 2), None) != 0 and "out must be 4-byte aligned" in err()
    assert lib.cart_local_ba_clear(None, None) != 0 and "ba is NULL" in err()
    assert lib.cart_local_ba_size(None, None, None) != 0 and "ba is NULL" in err()
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == -7.0).all() and (ints.cpu().numpy() == -7).all()
    same_state(ba, win)                                                          # nothing moved, and the object is still usable
    push_both(ba, win, S.CAM, p, 3, frames[2])
    optimize_both(ba, win, S.CAM, p)
    ba.close()


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------------------
def test_local_ba_module_in_the_frame_loop(tmp_path):
    """[orb_features, orb_matches, ego_motion, local_ba] over six frames of the block-noise scene of tests/test_gpu_matches.py (the camera
    moves by (0.25, 1/12, 0) m per frame): every frame's dump equals the restatement of the module fed with that frame's dumped inputs --
    the keypoints, the two match lists and ego_motion's result and pose.  window = 3, so frames leave the ring from frame 4 on."""
    import json
    import os
    from test_gpu_matches import noise_frame, noise_world
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n, W = 6, 3
    world = noise_world(79)
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for cam in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, cam))
    for f in range(n):
        l, r = noise_frame(world, f)
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    cam = E.camera(**keys)
    front = [{"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion")]
    runs = {"defaults": dict(window=W, max_points=4096), "keys": dict(window=W, max_points=512, interval=2, iterations=2, huber=1.5, damping=1e-6, min_observations=3,
                                                                      min_frame_observations=4, min_disparity=2.0)}
    for name, cfg in runs.items():
        d = os.path.join(tmp, "dump_" + name)
        os.makedirs(d)
        r = run_exe(src, front + [dict(keys, type="local_ba", **cfg)], tmp, ("--dump", d))
        assert r.returncode == 0, r.stderr
        frames = []
        for fid in range(1, n + 1):
            ego = open(os.path.join(d, f"{fid}_ego_motion.bin"), "rb").read()
            res = np.frombuffer(ego[:120], E.RESULT_DTYPE)
            frames.append(dict(kpL=np.fromfile(os.path.join(d, f"{fid}_features_left_keypoints.bin"), E.KEYPOINT_DTYPE),
                               kpR=np.fromfile(os.path.join(d, f"{fid}_features_right_keypoints.bin"), E.KEYPOINT_DTYPE),
                               stereo=np.fromfile(os.path.join(d, f"{fid}_feature_matches_stereo.bin"), E.MATCH_DTYPE),
                               temporal=np.fromfile(os.path.join(d, f"{fid}_feature_matches_temporal.bin"), E.MATCH_DTYPE),
                               status=int(res["status"][0]), pose=np.frombuffer(ego[120:], np.float64), R=res["R"][0], t=res["t"][0]))
        assert [f["status"] for f in frames] == [0] + [1] * (n - 1) and min(len(f["temporal"]) for f in frames[1:]) > 50
        want = B.module(cam, frames, 5000, **cfg)
        for fid in range(1, n + 1):
            rec, pose, ids, poses, R, t = want[fid - 1]
            got = open(os.path.join(d, f"{fid}_local_ba.bin"), "rb").read()
            assert len(got) == 80 + 96 + 8 * W + 96 * W + 96
            assert got[:80] == rec.tobytes(), f"{name} frame {fid}: {np.frombuffer(got[:80], B.MODULE_DTYPE)} != {rec}"
            assert got[80:176] == np.asarray(pose, np.float64).tobytes(), f"{name} frame {fid}: pose"
            assert got[176:176 + 8 * W] == ids.tobytes() and got[176 + 8 * W:176 + 104 * W] == poses.tobytes(), f"{name} frame {fid}: window"
            assert got[176 + 104 * W:] == np.array(list(R) + list(t), np.float64).tobytes(), f"{name} frame {fid}: relative pose"
            assert int(rec["counts"][0][7]) == min(fid, W) and int(rec["optimised"][0]) == int(fid > 1 and fid % cfg.get("interval", 1) == 0)
        last = want[n - 1][0][0]
        assert last["optimised"] == 1 and last["result"]["status"] == 1 and last["result"]["n_points_active"] > 50 and last["counts"][5] > 0
        assert sum(int(w[0]["taken"][0]) for w in want) >= 1
    # creation-time checks: the dependencies and an out-of-range key with the library's message
    r = run_exe(src, front[:2] + [dict(keys, type="local_ba")], tmp)
    assert r.returncode != 0 and 'requires "ego_motion"' in r.stderr
    r = run_exe(src, front + [dict(type="local_ba")], tmp)
    assert r.returncode != 0 and "fx" in r.stderr
    for key, bad in (("window", 1), ("window", 17), ("max_points", 63), ("iterations", 17), ("huber", 0), ("damping", -1.0), ("min_disparity", 0), ("min_observations", 0),
                     ("min_frame_observations", -1), ("interval", 0), ("pose_key", "pose_graph")):
        r = run_exe(src, front + [dict(keys, type="local_ba", **{key: bad})], tmp)
        assert r.returncode != 0 and key in r.stderr, (key, r.stderr)

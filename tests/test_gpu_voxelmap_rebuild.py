"""GPU tests of spec S35, rebuilding the TSDF volume from stored keyframes: cart_voxel_map_rebuild through
cartslam.VoxelMap.rebuild and the C ABI against the numpy restatement tests/np_voxelmap_rebuild.py, byte for byte (the volume, the origin,
`used` and `counts`), the equivalence with clear + sequential integrates on the device, the calls that continue on a rebuilt map, queued
calls on one and two streams, the refusals, and the voxel_map host module with "rebuild" in the C++ frame loop.  Beside every byte comparison
stands a numeric premise on the restatement, so that no comparison passes on an empty case."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import np_voxelmap as V
import np_voxelmap_rebuild as R
import test_voxelmap_spec as S
from test_gpu_voxelmap import SENTINEL, SMALL, cam_for, cam_tuple, engine, frame_for, integrate, pitched, raycast, same_ray, same_volume

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def make_map(shape, p):
    from cartslam import VoxelMap, voxel_map_params
    return VoxelMap(engine(), *shape, voxel_map_params(**p))


def fill(frames, capacity=None):
    """frames = [(id, disp, plane)] into a PlaneStore and its restatement, through pitched rows whose slack would pass every gate."""
    from cartslam import PlaneStore
    h, w = frames[0][1].shape
    store, ref = PlaneStore(engine(), w, h, capacity or len(frames)), R.Store(w, h, capacity or len(frames))
    for fid, disp, plane in frames:
        store.insert(fid, pitched(disp, 3, 256, 1), pitched(plane, 5, 0, 3), raw=True)
        ref.insert(fid, disp, plane)
    return store, ref


def frames_for(n, w, h, seed=0, depth=1.5):
    """[(id, disp, plane)]: test_voxelmap_spec.small_frame's wall with a step, holes and sub-minimum pixels; the plane holds 0, 2 and a block of 1."""
    cam = cam_for(w, h)
    return [(100 + k, *frame_for(seed + 7 * k, w, h, cam, depth=depth)) for k in range(n)]


def rebuild_call(obj, store, cam, ids, poses, window, use_mask=0, counts=None, used=None, stream=None):
    """cart_voxel_map_rebuild as it is -> (rc, message)."""
    from cartslam import _lib
    lib = _lib.load()
    flat = [float(v) for pose in poses for v in pose]
    sp = C.c_void_p((stream if stream is not None else _torch().cuda.current_stream()).cuda_stream)
    rc = lib.cart_voxel_map_rebuild(obj._h if obj is not None else None, store._h if store is not None else None, C.byref(_lib.EgoCamera(*cam_tuple(cam))),
                                    (C.c_uint64 * max(len(ids), 1))(*ids), (C.c_double * max(len(flat), 1))(*flat), len(ids),
                                    (C.c_double * 12)(*[float(v) for v in window]) if window is not None else None, use_mask,
                                    C.byref(used) if used is not None else None, C.c_void_p(counts.data_ptr()) if counts is not None else None, sp)
    return rc, lib.cart_last_error(None).decode()


def rebuild(obj, store, cam, ids, poses, window, use_mask=False, counts=True, stream=None):
    """One rebuild -> (used, the counts tensor inside sentinel words, or None)."""
    torch = _torch()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        n = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")[1:3] if counts else None
    used = C.c_int(-1)
    rc, err = rebuild_call(obj, store, cam, ids, poses, window, 1 if use_mask else 0, n, used, stream)
    assert rc == 0, err
    return used.value, n


def same_counts(n, ref):
    _torch().cuda.synchronize()
    assert n.cpu().numpy().tolist() == ref.tolist(), (n.cpu().numpy(), ref)
    assert (n._base.cpu().numpy()[[0, 3]] == SENTINEL).all()


def check_rebuild(shape, p, size, frames, ids, poses, window, use_mask, capacity=None, counts=True, prior=None):
    """The device and the restatement rebuild the same list; the volume, the origin, `used` and the counts must agree.  `prior` = a
    (pose, disp) integrated first, so that the rebuild runs over content and a window of another place.  -> the restatement and its results."""
    cam = cam_for(*size)
    store, sref = fill(frames, capacity)
    ref = R.Map(*shape, V.params(**p))
    with make_map(shape, p) as obj:
        if prior is not None:
            integrate(obj, cam, prior[0], prior[1], counts=False)
            ref.integrate(cam, prior[0], prior[1])
        used, n = rebuild(obj, store, cam, ids, poses, window, use_mask, counts)
        origin, rused, rn = ref.rebuild(sref, ids, poses, window, cam, use_mask)
        assert used == rused
        if counts:
            same_counts(n, rn)
        same_volume(obj, ref)
        assert obj.window()[0] == origin
    store.close()
    return ref, rused, rn


# poses whose own windows differ from one another on the small volumes (look-ahead 1 m, 2 m cubes)
POSES = [S.pose_t(), S.yaw_pose(9.0, (0.3, 0.0, 0.25)), S.pose_t(tz=1.0), S.yaw_pose(-14.0, (-1.0, 0.05, 0.5)), S.pose_t(tx=0.2, ty=-0.1, tz=0.1)]

CASES = {
    # name: (volume, image, entries, use_mask, params, window pose)
    "cube_empty_list": ((16, 16, 16), (40, 24), 0, False, SMALL, POSES[3]),
    "cube_one_entry_masked": ((16, 16, 16), (40, 24), 1, True, SMALL, POSES[0]),
    "cube_three_entries": ((16, 16, 16), (67, 19), 3, False, SMALL, POSES[1]),
    "wide_three_entries_masked": ((72, 16, 24), (67, 19), 3, True, dict(SMALL, lookahead=1.5), POSES[0]),
    "wide_five_entries": ((72, 16, 24), (40, 24), 5, False, dict(SMALL, lookahead=1.5), POSES[4]),
    "flat_five_entries_weight_cap": ((64, 32, 16), (40, 24), 5, False, dict(SMALL, max_weight=2), POSES[0]),
    "flat_three_entries_masked": ((64, 32, 16), (67, 19), 3, True, SMALL, POSES[2]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_byte_exact_against_the_restatement(name):
    """72 is no multiple of 64 and above it (two workgroups along x, the second with eight lanes in); 24 is no multiple of 16 (a build of the
    kernel with 16 slices per workgroup, the integrate's depth, has a partial workgroup there); the origins have negative components, so the
    toroidal offsets are non-zero; the masks hold the value 1."""
    shape, size, entries, use_mask, p, window = CASES[name]
    frames = frames_for(entries or 1, *size, seed=len(name))
    assert all((f[2] == V.MOVING).any() and (f[2] != V.MOVING).any() for f in frames)
    poses = POSES[:entries]
    prior = (S.pose_t(tz=3.0), frames[0][1])                                  # content and a window that the rebuild must leave no trace of
    ref, used, n = check_rebuild(shape, p, size, frames, [f[0] for f in frames][:entries], poses, window, use_mask, prior=prior)
    assert used == entries and min(ref.origin) < 0 and any(o % s for o, s in zip(ref.origin, shape)), ref.origin
    if entries:
        assert len({V.window_origin(q, ref.p, shape) for q in poses + [window]}) > (1 if entries > 1 else 0)
        assert n[0] > 50 and 0 < n[1] < n[0], n                               # voxels were updated, some inside the truncation band, some in free space
        top = int(ref.read()[0]["weight"].max())
        assert top == 2 if p.get("max_weight") == 2 else top >= min(entries, 3), top   # voxels that several entries saw; capped where the cap is 2
    else:
        assert not ref.read()[0]["weight"].any() and n.tolist() == [0, 0]
    if use_mask:                                                              # the mask matters: without it more voxels are updated
        other, sref = R.Map(*shape, V.params(**p)), R.Store(size[0], size[1], len(frames))
        for f in frames:
            sref.insert(*f)
        assert other.rebuild(sref, [f[0] for f in frames][:entries], poses, window, cam_for(*size))[2][0] > n[0]


def test_evicted_and_repeated_ids_and_counts_null():
    frames = frames_for(3, 67, 19, seed=5)
    ids = [100, 101, 999, 102, 101]                                           # 100 was evicted (capacity 2, three inserts), 999 never existed, 101 twice
    ref, used, n = check_rebuild((16, 16, 16), SMALL, (67, 19), frames, ids, POSES, POSES[0], True, capacity=2)
    assert used == 3 and ref.read()[0]["weight"].max() >= 2 and n[0] > 50
    ref2, used2, _ = check_rebuild((72, 16, 24), dict(SMALL, lookahead=1.5), (67, 19), frames, ids, POSES, POSES[1], False, capacity=2, counts=False)
    assert used2 == 3 and ref2.read()[0]["weight"].max() >= 2
    # nothing known: an empty valid window at the new origin
    ref3, used3, n3 = check_rebuild((16, 16, 16), SMALL, (67, 19), frames, [7, 8], POSES[:2], S.pose_t(tx=9.0, tz=-30.0), False, prior=(POSES[0], frames[0][1]))
    assert used3 == 0 and n3.tolist() == [0, 0] and ref3.origin == (64, -8, -240)
    # through the Python class: the origin, used and the counts as host values
    store, sref = fill(frames, 2)
    cam = cam_for(67, 19)
    with make_map((16, 16, 16), SMALL) as obj:
        got = obj.rebuild(store, ids, POSES, POSES[0], cam_tuple(cam), use_mask=True)
        assert got[0] == ref.origin and got[1] == 3 and got[2].dtype == np.int64 and got[2].tolist() == n.tolist()
        assert obj.rebuild(store, [], np.zeros((0, 12)), POSES[2], cam_tuple(cam), counts=False) == (V.window_origin(POSES[2], ref.p, (16, 16, 16)), 0, None)
    store.close()


def test_equivalence_with_clear_and_sequential_integrates_on_the_device():
    """Poses that share the rebuild's window (asserted on the restatement): the rebuilt volume equals clear + one integrate per entry, byte
    for byte, and the counts are the sums of the integrates' counts.  Both sides are the device's."""
    shape, size = (72, 16, 24), (67, 19)
    p = dict(SMALL, lookahead=1.5, max_weight=3)
    cam = cam_for(*size)
    frames = frames_for(5, *size, seed=3)
    poses = [S.yaw_pose(1.5 * k, (0.01 * k, 0.005 * k, 0.02 * k)) for k in range(5)]
    assert len({V.window_origin(q, V.params(**p), shape) for q in poses}) == 1
    store, _ = fill(frames)
    with make_map(shape, p) as a, make_map(shape, p) as b:
        integrate(b, cam, S.pose_t(tz=5.0), frames[0][1], counts=False)       # b holds something else first
        b.clear()
        total = np.zeros(2, np.int64)
        for (_, disp, plane), pose in zip(frames, poses):
            total += integrate(b, cam, pose, disp, plane).cpu().numpy().astype(np.int64)
        used, n = rebuild(a, store, cam, [f[0] for f in frames], poses, poses[2], use_mask=True)
        same_counts(n, total)
        (va, oa), (vb, ob) = a.read(), b.read()
        assert used == 5 and oa == ob and va.tobytes() == vb.tobytes(), f"{int((va != vb).sum())} voxels differ"
        assert va["weight"].max() == 3 and total[1] > 100
    store.close()


def test_integrate_raycast_and_tracking_continue_on_a_rebuilt_map():
    import np_modeltrack as T
    from test_gpu_modeltrack import MODEL_SIZE, START, TRACK, model_frames, record, run, same, tracker
    w, h = MODEL_SIZE
    cam = cam_for(w, h)
    shape, p = (16, 16, 24), SMALL
    built = model_frames(3)
    frames = [(k, d, np.zeros((h, w), np.uint8)) for k, (_, d, _) in enumerate(built)]
    poses = [pose for pose, _, _ in built]
    store, sref = fill(frames)
    ref = R.Map(*shape, V.params(**p))
    with make_map(shape, p) as obj:
        used, n = rebuild(obj, store, cam, [0, 1, 2], poses, poses[-1])
        _, rused, rn = ref.rebuild(sref, [0, 1, 2], poses, poses[-1], cam)
        assert used == rused == 3
        same_counts(n, rn)
        same_volume(obj, ref)
        # the model is tracked against, as after any integrate
        disp, mask = frame_for(9, w, h, cam)
        tp = T.params(**TRACK)
        exp = T.refine(ref, cam, tp, START, disp, mask)
        assert exp["status"][0] == 1 and exp["n_inliers"][0] > 100
        same(record(run(tracker(), obj, cam, tp, START, disp, mask)), exp)
        # a raycast of the rebuilt model
        rr = ref.raycast(cam, poses[-1], w, h)
        assert rr["counts"][V.HIT] > 1000
        same_ray(raycast(obj, cam, poses[-1], w, h), rr)
        # an integrate that moves the window by 8 voxels on z and on x: what entered is emptied, what stayed is the rebuilt content
        moved = S.pose_t(tx=1.0, tz=1.0)
        before = ref.origin
        nd = integrate(obj, cam, moved, disp, mask)
        rnd = ref.integrate(cam, moved, disp, mask)
        assert ref.origin == (before[0] + 8, before[1], before[2] + 8) and rnd[0] > 100
        assert nd.cpu().numpy().tolist() == rnd.tolist()
        same_volume(obj, ref)
        assert (ref.read()[0]["weight"] >= 3).any()                           # rebuilt voxels survived the move and took the new frame
        same_ray(raycast(obj, cam, moved, w, h), ref.raycast(cam, moved, w, h))
    store.close()


def test_back_to_back_rebuilds_and_two_streams():
    torch = _torch()
    shape, size, p = (72, 16, 24), (67, 19), dict(SMALL, lookahead=1.5)
    cam = cam_for(*size)
    frames = frames_for(4, *size, seed=11)
    store, sref = fill(frames)
    ids = [f[0] for f in frames]
    first, second = POSES[:4], [S.yaw_pose(-6.0 * k, (-0.1 * k, 0.0, 0.2 * k)) for k in range(4)]
    ref, ref2 = R.Map(*shape, V.params(**p)), R.Map(*shape, V.params(**p))
    with make_map(shape, p) as m, make_map(shape, p) as m2:
        torch.cuda.synchronize()
        _, n1 = rebuild(m, store, cam, ids, first, first[0])                  # queued back to back, nothing between them: the second call's
        _, n2 = rebuild(m, store, cam, ids[::-1], second, second[3], use_mask=True)   # records must not reach the first call's kernel
        rn1 = ref.rebuild(sref, ids, first, first[0], cam)[2]
        rn2 = ref.rebuild(sref, ids[::-1], second, second[3], cam, True)[2]
        same_counts(n1, rn1)
        same_counts(n2, rn2)
        same_volume(m, ref)
        _, n1 = rebuild(m, store, cam, ids, first, first[0])                  # one store, two maps, no synchronisation
        _, n2 = rebuild(m2, store, cam, ids[::-1], second, second[3])
        ref.rebuild(sref, ids, first, first[0], cam)
        ref2.rebuild(sref, ids[::-1], second, second[3], cam)
        same_volume(m, ref)
        same_volume(m2, ref2)
        # an insert on one stream, the rebuild on another: the rebuild sees the inserted frame; an insert after it waits for it
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        newer = frame_for(99, *size, cam)
        with torch.cuda.stream(b):
            d, l = pitched(newer[0], 3, 256, 1), pitched(newer[1], 5, 0, 3)
        torch.cuda.synchronize()
        with torch.cuda.stream(b):
            store.insert(500, d, l, raw=True)                                 # evicts frame 100 (slot 0)
        used, n3 = rebuild(m, store, cam, [500, 100, 101], first[:3], first[1], use_mask=True, stream=a)
        with torch.cuda.stream(b):
            store.insert(501, d, l, raw=True)                                 # evicts frame 101, which the rebuild in flight reads
        sref.insert(500, *newer)
        assert used == 2 == ref.rebuild(sref, [500, 100, 101], first[:3], first[1], cam, True)[1]
        same_counts(n3, ref.rebuild(sref, [500, 100, 101], first[:3], first[1], cam, True)[2])
        same_volume(m, ref)
    store.close()


def test_bad_arguments_touch_nothing():
    torch = _torch()
    from cartslam import EngineError, PlaneStore
    shape, size, p = (16, 16, 16), (40, 24), SMALL
    cam = cam_for(*size)
    frames = frames_for(2, *size)
    store, sref = fill(frames)
    ref = R.Map(*shape, V.params(**p))
    ids, poses = [100, 101], POSES[:2]
    with make_map(shape, p) as obj:
        integrate(obj, cam, POSES[0], frames[0][1], counts=False)
        ref.integrate(cam, POSES[0], frames[0][1])
        counts = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
        used = C.c_int(-7)
        nan1 = [list(q) for q in poses]
        nan1[1][7] = math.nan
        far = list(POSES[0])
        far[11] = 2e6
        bad_cam = dict(cam, fx=0.0)
        cases = [(dict(ids=[1] * 4097, poses=[POSES[0]] * 4097), "count"), (dict(use_mask=2), "use_mask"), (dict(cam=bad_cam), "fx"), (dict(window=None), "window_pose"),
                 (dict(window=far), "window_pose[11]"), (dict(poses=nan1), "poses[1][7]"), (dict(obj=None), "map is NULL"), (dict(store=None), "store is NULL"),
                 (dict(counts=counts.view(torch.int8)[4:]), "counts must be 8-byte aligned")]
        for kw, word in cases:
            args = dict(obj=obj, store=store, cam=cam, ids=ids, poses=poses, window=POSES[1], use_mask=0, counts=counts[1:3], used=used)
            args.update(kw)
            rc, text = rebuild_call(**args)
            assert rc != 0 and word in text, (word, text)
        torch.cuda.synchronize()
        assert used.value == -7 and (counts.cpu().numpy() == SENTINEL).all()
        same_volume(obj, ref)                                                 # the volume and the origin are where the integrate left them
        with pytest.raises(EngineError, match="12 numbers"):
            obj.rebuild(store, ids, [POSES[0]], POSES[0], cam_tuple(cam))
        with pytest.raises(EngineError, match="PlaneStore"):
            obj.rebuild(obj, ids, poses, POSES[0], cam_tuple(cam))
        closed = PlaneStore(engine(), 40, 24, 1)
        closed.close()
        with pytest.raises(EngineError):
            obj.rebuild(closed, ids, poses, POSES[0], cam_tuple(cam))
        same_volume(obj, ref)
        used_ok, n = rebuild(obj, store, cam, ids, poses, POSES[1])           # and the valid call goes through
        assert used_ok == 2
        same_counts(n, ref.rebuild(sref, ids, poses, POSES[1], cam)[2])
        same_volume(obj, ref)
    store.close()


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------------------
def test_voxel_map_module_rebuilds_when_the_pose_graph_optimised(tmp_path):
    """test_gpu_planemap_rebuild's synthetic loop (keyframes 2, 4, 6; frame 6 closes the loop) with the voxel_map module behind pose_graph:
    frames 1 to 5 equal the per-frame integrates, frame 6 equals the restatement's rebuild of keyframes 2, 4, 6 through np_posegraph's node
    estimates in the window of frame 6's corrected pose, and only frame 6 writes the rebuild record.  Without "rebuild" the module dumps
    the chain of integrates and no rebuild record."""
    import json
    import np_posegraph as G
    import oracle_lib as O
    import test_place_spec as L
    from test_gpu_voxelmap import read_dump
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    images, _, _, _, ego, records = L.loop_sequence()
    n, w, h = len(images), 320, 96
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for side in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, side))
    for f, (l, r) in enumerate(images):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    # test_gpu_voxelmap's frame loop: a textured plane 25 m away, half-metre voxels
    vp = dict(voxel_size=0.5, min_disparity=3.5, max_depth=40.0, truncation=1.0, march_step=0.5, lookahead=16.0, max_weight=3)
    shape = dict(cells_x=64, cells_y=16, cells_z=64)
    front = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
             {"type": "orb_features"}, {"type": "orb_matches"}, dict(L.LOOP_KEYS, type="ego_motion"), dict(L.LOOP_KEYS, type="loop_closure", **L.LOOP_CONFIG)]
    graph_keys = dict(keyframe_interval=L.LOOP_CONFIG["keyframe_interval"], max_nodes=8, max_loops=2)
    voxel_map = dict(L.LOOP_KEYS, type="voxel_map", pose_key="pose_graph", rebuild=True, store_capacity=4, **shape, **vp)
    want = G.module([pose for _, pose in ego], records, **graph_keys)
    assert [int(rec["node"][0]) for rec, _, _ in want] == [-1, 0, -1, 1, -1, 2] and [nodes is not None for _, _, nodes in want] == [False] * 5 + [True]
    cam = V.camera(**L.LOOP_KEYS)
    disps = {}
    for f in range(n):
        k = L.LOOP_ORDER[f]
        if k not in disps:
            disps[k] = O.disparity_module(images[f][0], images[f][1], 64, 8, 4, radius=2, iterations=1)

    def run(module, name):
        d = os.path.join(tmp, name)
        os.makedirs(d)
        r = run_exe(src, front + [dict(graph_keys, type="pose_graph"), module], tmp, ("--dump", d), env={"CARTSLAM_VOXEL_MAP_SNAPSHOT": "1"})
        assert r.returncode == 0, r.stderr
        return d

    def same_frame(d, f, ref, counts, rays):
        got = read_dump(os.path.join(d, f"{f + 1}_voxel_map.bin"), w, h)
        assert got["origin"] == ref.origin and got["cells"] == (64, 16, 64), f"frame {f + 1}: window"
        assert got["counts"].tolist() == [int(v) for v in counts] and got["rays"].tobytes() == rays["counts"].tobytes(), f"frame {f + 1}: counts"
        assert got["disp"].tobytes() == rays["disp"].tobytes() and got["status"].tobytes() == rays["status"].tobytes(), f"frame {f + 1}: model"
        assert open(os.path.join(d, f"{f + 1}_voxel_map_voxels.bin"), "rb").read() == ref.read()[0].tobytes(), f"frame {f + 1}: voxels"

    d = run(voxel_map, "dump")
    ref, store = R.Map(64, 16, 64, V.params(**vp)), R.Store(w, h, 4)
    for f in range(n):
        disp = disps[L.LOOP_ORDER[f]]
        rec, pose, nodes = want[f]
        if int(rec["node"][0]) >= 0:
            store.insert(f + 1, disp, np.zeros((h, w), np.uint8))
        path = os.path.join(d, f"{f + 1}_voxel_map_rebuild.bin")
        if nodes is None:
            counts = ref.integrate(cam, pose, disp)
            assert not os.path.exists(path), path
        else:
            _, used, counts = ref.rebuild(store, [2, 4, 6], nodes, pose, cam)
            assert used == 3 and counts[1] > 1000 and int(ref.read()[0]["weight"].max()) == 3
            raw = open(path, "rb").read()
            assert np.frombuffer(raw[:8], "<i4").tolist() == [3, 3] and np.frombuffer(raw[8:], "<u8").tolist() == [2, 4, 6]
        same_frame(d, f, ref, counts, ref.raycast(cam, pose, w, h))
    rebuilt = ref.read()[0].tobytes()

    d = run({k: v for k, v in voxel_map.items() if k not in ("rebuild", "store_capacity")}, "dump_plain")
    ref = V.Map(64, 16, 64, V.params(**vp))
    for f in range(n):
        rec, pose, nodes = want[f]
        counts = ref.integrate(cam, pose, disps[L.LOOP_ORDER[f]])
        same_frame(d, f, ref, counts, ref.raycast(cam, pose, w, h))
        assert not os.path.exists(os.path.join(d, f"{f + 1}_voxel_map_rebuild.bin"))
    assert ref.read()[0].tobytes() != rebuilt                                 # the rebuild made a difference

    # "rebuild" needs the corrected trajectory and no tracking: any other configuration fails at creation, naming the key
    for bad, word in ((dict(voxel_map, pose_key="ego_motion"), "rebuild"), (dict(voxel_map, store_capacity=0), "store_capacity"), (dict(voxel_map, track=True), "track")):
        r = run_exe(src, front + [dict(graph_keys, type="pose_graph"), bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    r = run_exe(src, front + [voxel_map], tmp)                                # without the pose_graph module
    assert r.returncode != 0 and 'requires "pose_graph' in r.stderr, r.stderr

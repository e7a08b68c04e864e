"""GPU tests of spec S30, rebuilding the plane map from stored keyframes: cart_plane_store_* and cart_plane_map_rebuild
through cartslam.PlaneStore / PlaneMap.rebuild against the numpy restatement tests/np_planemap_rebuild.py, byte for byte, and the plane_map
host module with "rebuild" in the C++ frame loop."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import np_planemap as M
import np_planemap_rebuild as R
from test_gpu_planemap import CAM, cam_tuple, engine, make_map, pitched, pose_at, random_frame, yaw_pose

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def make_store(w, h, capacity, eng=None):
    from cartslam import PlaneStore
    return PlaneStore(eng or engine(), w, h, capacity)


def wall_frame(seed, w, h):
    """test_gpu_planemap.random_frame plus one all-wall row and one all-wall COLUMN (Z = 6 m): the column's run stays open across the 8-row groups."""
    disp, planes = random_frame(seed, w, h)
    disp[h // 2, :] = 400
    disp[:, w // 3], planes[:, w // 3] = 400, 1
    return disp, planes


def same(m, ref, what="", thresholds=((3, 50),)):
    cells, origin = m.read()
    assert origin == ref.origin == m.window()[:2] and m.window()[2], what
    assert cells.tobytes() == ref.cells.tobytes(), f"{what}: {int((cells != ref.cells).sum())} cells differ"
    for mv, pc in thresholds:
        assert m.classify(mv, pc).tobytes() == ref.classify(mv, pc).tobytes(), f"{what}: classes ({mv}, {pc})"


def fill(frames, w, h, capacity, eng=None):
    """frames = [(id, disp, planes)] into a store and its restatement, through pitched rows whose slack would vote if read."""
    store, ref = make_store(w, h, capacity, eng), R.Store(w, h, capacity)
    for fid, disp, planes in frames:
        store.insert(fid, pitched(disp, 6), pitched(planes, 5), raw=True)
        ref.insert(fid, disp, planes)
    assert store.size() == ref.size()
    return store, ref


def check_rebuild(cam, nx, nz, p, frames, ids, poses, window_pose, capacity=8, expect_used=None):
    h, w = frames[0][1].shape
    store, sref = fill(frames, w, h, capacity)
    m, ref = make_map(cam, nx, nz, p), M.Map(cam, nx, nz, p)
    try:
        origin, used = m.rebuild(store, ids, poses, window_pose)
        assert used == R.rebuild(ref, sref, ids, poses, window_pose) and origin == ref.origin
        if expect_used is not None:
            assert used == expect_used
        same(m, ref)
    finally:
        m.close()
        store.close()
    return ref


POSES = [yaw_pose(0.0), yaw_pose(30.0, (0.3, 0.0, -0.7)), yaw_pose(-20.0, (-1.1, 0.05, 0.9)), yaw_pose(75.0, (0.8, -0.1, 0.2)), yaw_pose(170.0, (2.0, 0.0, 3.5))]


@pytest.mark.parametrize("w,h", [(67, 5), (130, 9), (256, 16), (130, 131), (67, 259)])   # the last two: more than one tall strip and no multiple of 8, 32, 64 or 128
@pytest.mark.parametrize("entries", [1, 2, 5])
def test_kernel_edges_with_pitched_rows(w, h, entries):
    frames = [(100 + k, *wall_frame(w * h + k, w, h)) for k in range(entries)]
    ref = check_rebuild(CAM, 64, 48, M.params(), frames, [f[0] for f in frames], POSES[:entries], POSES[entries - 1], expect_used=entries)
    total = int(ref.cells["horizontal"].sum()) + int(ref.cells["vertical"].sum())
    assert w * h // 8 < total and (entries < 5 or total < entries * w * h * 2 // 3)      # votes land, and with the far poses some leave the window


@pytest.mark.parametrize("label", [0, 1])
def test_maximal_contention_counts_every_pixel(label):
    disp, planes = np.full((16, 256), 200, np.int16), np.full((16, 256), label, np.uint8)
    frames = [(k, disp, planes) for k in range(5)]
    ref = check_rebuild(CAM, 32, 32, M.params(cell_size=64.0), frames, list(range(5)), [pose_at(tx=20.0)] * 5, pose_at(tx=20.0), expect_used=5)
    field = "vertical" if label else "horizontal"
    assert int(ref.cells[field][16, 16]) == 5 * 4096 and int(ref.cells[field].sum()) == 5 * 4096


def test_ring_wrap_around_duplicated_and_unknown_ids():
    w, h = 130, 9
    frames = [(k, *wall_frame(10 + k, w, h)) for k in range(5)]
    check_rebuild(CAM, 64, 48, M.params(), frames, [0, 1, 2, 3, 4], POSES, POSES[0], capacity=2, expect_used=2)
    check_rebuild(CAM, 64, 48, M.params(), frames[:2], [1, 999, 1, 0], POSES[:4], POSES[1], expect_used=3)   # 1 votes twice, 999 is skipped
    check_rebuild(CAM, 64, 48, M.params(), frames[:2], [7, 8], POSES[:2], pose_at(tx=9.0), expect_used=0)     # nothing known: an empty window there
    ref = check_rebuild(CAM, 64, 48, M.params(), frames[:2], [], np.zeros((0, 12)), pose_at(tx=9.0, tz=-30.0), expect_used=0)
    assert ref.origin == (0, -144) and ref.cells.tobytes() == M.empty_cells(48, 64).tobytes()
    # a repeated id names its latest insertion; clear forgets everything
    store, sref = fill([(3, *frames[0][1:]), (3, *frames[1][1:])], w, h, 4)
    m, ref = make_map(CAM, 64, 48), M.Map(CAM, 64, 48)
    assert m.rebuild(store, [3], [POSES[0]], POSES[0])[1] == R.rebuild(ref, sref, [3], [POSES[0]], POSES[0]) == 1
    same(m, ref, "repeated id")
    only_second = M.Map(CAM, 64, 48)
    only_second.update(*frames[1][1:], POSES[0])
    assert ref.cells.tobytes() == only_second.cells.tobytes()
    assert store.contains(3) and not store.contains(4) and store.size() == (2, 4)
    store.clear()
    assert store.size() == (0, 4) and not store.contains(3) and m.rebuild(store, [3], [POSES[0]], POSES[0])[1] == 0
    m.close()
    store.close()


def test_rebuild_over_existing_content_and_continuing_after_it():
    w, h = 130, 9
    frames = [(k, *wall_frame(30 + k, w, h)) for k in range(3)]
    good = [yaw_pose(5.0 * k, (0.2 * k, 0.0, 0.4 * k)) for k in range(3)]
    drifted = [yaw_pose(5.0 * k + 4.0, (0.2 * k + 1.3, 0.0, 0.4 * k - 2.2)) for k in range(3)]
    store, sref = fill(frames, w, h, 4)
    m, ref = make_map(CAM, 64, 48), M.Map(CAM, 64, 48)
    for (_, disp, planes), pose in zip(frames, drifted):                # the live map, with the drift
        m.update(disp, planes, pose)
        ref.update(disp, planes, pose)
    same(m, ref, "live")
    drifted_bytes = ref.cells.tobytes()
    assert m.rebuild(store, [0, 1, 2], good, good[2])[1] == R.rebuild(ref, sref, [0, 1, 2], good, good[2]) == 3
    same(m, ref, "rebuilt")
    clean = M.Map(CAM, 64, 48)                                          # nothing of the old content survives: the bytes are those of the good poses alone
    for (_, disp, planes), pose in zip(frames, good):
        clean.update(disp, planes, pose)
    assert clean.origin == ref.origin and ref.cells.tobytes() == clean.cells.tobytes() != drifted_bytes
    for k, pose in enumerate((yaw_pose(12.0, (4.3, 0.0, 0.3)), yaw_pose(15.0, (4.4, 0.0, 4.4)), good[0])):   # window-moving updates continue on it
        m.update(*frames[k][1:], pose)
        ref.update(*frames[k][1:], pose)
        same(m, ref, f"update {k} after the rebuild")
    assert ref.origin == (-32, -32)
    m.close()
    store.close()


def test_back_to_back_rebuilds_and_two_streams():
    torch = _torch()
    w, h = 256, 16
    frames = [(k, *wall_frame(60 + k, w, h)) for k in range(4)]
    store, sref = fill(frames, w, h, 4)
    first, second = POSES[:4], [yaw_pose(-9.0 * k, (-0.2 * k, 0.0, 0.3 * k)) for k in range(4)]
    m, ref = make_map(CAM, 64, 48), M.Map(CAM, 64, 48)
    torch.cuda.synchronize()
    m.rebuild(store, [0, 1, 2, 3], first, first[0])                      # queued back to back, nothing between them: the second call's
    m.rebuild(store, [3, 2, 1, 0], second, second[3])                    # records must not reach the first call's kernel
    R.rebuild(ref, sref, [3, 2, 1, 0], second, second[3])
    same(m, ref, "the second of two rebuilds")
    m2, ref2 = make_map(CAM, 64, 48), M.Map(CAM, 64, 48)
    m.rebuild(store, [0, 1, 2, 3], first, first[0])
    m2.rebuild(store, [3, 2, 1, 0], second, second[3])                   # one store, two maps, no synchronisation
    R.rebuild(ref, sref, [0, 1, 2, 3], first, first[0])
    R.rebuild(ref2, sref, [3, 2, 1, 0], second, second[3])
    same(m, ref, "map 1 of two")
    same(m2, ref2, "map 2 of two")
    # rebuild and insert on two streams: the insert that follows the rebuild must wait for it, the rebuild that follows the insert sees it
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    newer = wall_frame(99, w, h)
    d, l = torch.from_numpy(newer[0]).cuda(), torch.from_numpy(newer[1]).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        m.rebuild(store, [0, 1, 2, 3], first, first[0])
    with torch.cuda.stream(b):
        store.insert(4, d, l, raw=True)                                  # evicts frame 0 (slot 0)
    with torch.cuda.stream(a):
        m2.rebuild(store, [4, 1, 0], second[:3], second[0])
    R.rebuild(ref, sref, [0, 1, 2, 3], first, first[0])
    sref.insert(4, *newer)
    assert R.rebuild(ref2, sref, [4, 1, 0], second[:3], second[0]) == 2
    same(m, ref, "rebuild before the insert")
    same(m2, ref2, "rebuild after the insert")
    for o in (m, m2, store):
        o.close()


def test_lifecycle():
    torch = _torch()
    from cartslam import Engine, EngineError
    w, h = 130, 9
    disp, planes = wall_frame(2, w, h)
    sref, ref = R.Store(w, h, 2), M.Map(CAM, 64, 48)
    sref.insert(1, disp, planes)
    R.rebuild(ref, sref, [1], [POSES[1]], POSES[1])
    other = Engine(64, 32, num_disparities=0, paths=0)                   # both closed after their engine
    store, m = make_store(w, h, 2, eng=other), make_map(CAM, 64, 48, eng=other)
    store.insert(1, disp, planes)
    other.close()
    assert m.rebuild(store, [1], [POSES[1]], POSES[1]) == (ref.origin, 1)
    assert m.read()[0].tobytes() == ref.cells.tobytes()
    store.close()
    store.close()
    for call in (lambda: store.insert(2, disp, planes), lambda: store.contains(1), store.size, store.clear, lambda: m.rebuild(store, [1], [POSES[1]], POSES[1])):
        with pytest.raises(EngineError):
            call()
    assert m.read()[0].tobytes() == ref.cells.tobytes()                  # the refused rebuild touched nothing
    live = make_store(w, h, 2)
    m.close()
    with pytest.raises(EngineError):
        m.rebuild(live, [1], [POSES[1]], POSES[1])
    live.close()
    d, l = torch.from_numpy(disp).cuda(), torch.from_numpy(planes).cuda()

    def cycle(n):
        for _ in range(n):
            s, o = make_store(w, h, 16), make_map(CAM, 512, 512)
            s.insert(1, d, l, raw=True)
            o.rebuild(s, [1], [POSES[0]], POSES[0])
            o.close()
            s.close()
        torch.cuda.synchronize()
    cycle(3)
    free0 = torch.cuda.mem_get_info()[0]
    cycle(20)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"plane store leak: {(free0 - free1) >> 20} MiB over 20 create/insert/rebuild/close cycles"


def test_bad_arguments():
    torch = _torch()
    from cartslam import EngineError, PlaneStore, _lib
    lib = _lib.load()
    err = lambda: lib.cart_last_error(None).decode()   # noqa: E731
    with pytest.raises(EngineError, match="capacity"):
        PlaneStore(engine(), 130, 9, 0)
    with pytest.raises(EngineError, match="width"):
        PlaneStore(engine(), 0, 9, 4)
    w, h = 130, 9
    store, m = make_store(w, h, 2), make_map(CAM, 64, 48)
    disp, planes = (torch.from_numpy(a).cuda() for a in wall_frame(1, w, h))

    def insert(d=disp.data_ptr(), ds=260, p=planes.data_ptr(), ps=130, iw=w, ih=h):
        return lib.cart_plane_store_insert(store._h, 5, C.c_void_p(d), ds, C.c_void_p(p), ps, iw, ih, None), err()

    for kw, word in ((dict(d=None), "NULL"), (dict(p=None), "NULL"), (dict(d=disp.data_ptr() + 1), "aligned"), (dict(ds=261), "aligned"), (dict(ds=258), "disparity_step"),
                     (dict(ps=129), "planes_step"), (dict(iw=0), "width"), (dict(ih=20000), "height"), (dict(iw=128, ds=256, ps=128), "must equal the store's W x H"),
                     (dict(ih=8), "must equal the store's W x H")):
        rc, text = insert(**kw)
        assert rc != 0 and word in text, (kw, text)
    assert store.size() == (0, 2) and not store.contains(5)                # no refused insert touched the store
    assert lib.cart_plane_store_contains(store._h, 5, None) != 0 and "slot" in err()
    store.insert(5, disp, planes, raw=True)
    cam = _lib.EgoCamera(*cam_tuple(CAM))
    ids, window = (C.c_uint64 * 2)(5, 5), (C.c_double * 12)(*M.POSE_IDENTITY)

    def rebuild(count=2, poses=None, window_pose=window, id_list=ids, mh=m._h, sh=store._h, camera=cam):
        flat = (C.c_double * 24)(*(poses if poses is not None else list(M.POSE_IDENTITY) * 2))
        return lib.cart_plane_map_rebuild(mh, sh, C.byref(camera), id_list, flat, count, window_pose, None, None), err()

    nan1 = list(M.POSE_IDENTITY) * 2
    nan1[12 + 7] = math.nan
    for kw, word in ((dict(count=-1), "count"), (dict(count=4097), "count"), (dict(poses=nan1), "poses[1]"), (dict(window_pose=None), "window_pose"),
                     (dict(id_list=None), "ids"), (dict(mh=None), "map is NULL"), (dict(sh=None), "store is NULL"),
                     (dict(camera=_lib.EgoCamera(300.0, 0.0, 80.0, 8.0, 0.5)), "fy")):
        rc, text = rebuild(**kw)
        assert rc != 0 and word in text, (kw, text)
    with pytest.raises(EngineError, match="12 numbers"):
        m.rebuild(store, [5, 5], [M.POSE_IDENTITY], M.POSE_IDENTITY)
    with pytest.raises(EngineError, match="PlaneStore"):
        m.rebuild(m, [5], [M.POSE_IDENTITY], M.POSE_IDENTITY)
    assert m.window() == (0, 0, False)                                     # no refused call touched the map
    assert rebuild()[0] == 0 and m.window() == (-32, -32, True)
    m.close()
    store.close()


def test_full_size_frame():
    from cartslam import synth
    kitti = M.camera(721.5, 721.5, 609.5, 172.85, 0.54)
    disp, planes = synth.road_corridor(1242, 375, *cam_tuple(kitti))
    poses = [M.POSE_IDENTITY, yaw_pose(4.0, (0.3, -0.02, 1.1)), yaw_pose(9.0, (0.9, -0.03, 4.2))]
    ref = check_rebuild(kitti, 512, 512, M.params(), [(k, disp, planes) for k in range(3)], [0, 1, 2], poses, poses[2], capacity=3, expect_used=3)
    assert ref.origin == (-256, -240)                                      # the last pose moved the window: the earlier frames vote into it all the same
    assert int(ref.cells["vertical"].max()) > 5000 and int((ref.cells["horizontal"] > 0).sum()) > 1500   # wall cells take whole columns


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------------------
def test_plane_map_module_rebuilds_when_the_pose_graph_optimised(tmp_path):
    """test_gpu_posegraph.test_pose_graph_module_frame_loop's configuration with "rebuild": true (keyframes 2, 4, 6; frame 6 closes the loop):
    frames 1 to 5 equal the per-frame map, frame 6 equals the restatement's rebuild of keyframes 2, 4, 6 through np_posegraph's node estimates
    in the window of frame 6's corrected pose, and only frame 6 writes the rebuild record."""
    import json
    import np_posegraph as G
    import oracle_lib as O
    import test_place_spec as L
    from test_gpu_planemap import check_dump
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    images, _, _, _, ego, records = L.loop_sequence()
    n = len(images)
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for cam in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, cam))
    for f, (l, r) in enumerate(images):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    static = {"type": "static", "horizontal_range_min": 6, "horizontal_range_max": 18, "vertical_range_min": -5, "vertical_range_max": 6}
    grid = dict(cells_x=64, cells_z=64, cell_size=1.0, max_depth=40.0, max_lateral=30.0)
    front = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
             {"type": "disparity_planeseg", "parameter_provider": static},
             {"type": "orb_features"}, {"type": "orb_matches"}, dict(L.LOOP_KEYS, type="ego_motion"), dict(L.LOOP_KEYS, type="loop_closure", **L.LOOP_CONFIG)]
    graph_keys = dict(keyframe_interval=L.LOOP_CONFIG["keyframe_interval"], max_nodes=8, max_loops=2)
    plane_map = dict(L.LOOP_KEYS, type="plane_map", pose_key="pose_graph", rebuild=True, store_capacity=4, **grid)
    modules = front + [dict(graph_keys, type="pose_graph"), plane_map]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, modules, tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    want = G.module([pose for _, pose in ego], records, **graph_keys)
    assert [int(rec["node"][0]) for rec, _, _ in want] == [-1, 0, -1, 1, -1, 2] and [nodes is not None for _, _, nodes in want] == [False] * 5 + [True]
    p = M.params(cell_size=1.0, max_depth=40.0, max_lateral=30.0)
    cam = M.camera(**L.LOOP_KEYS)
    ref = M.Map(cam, 64, 64, p)
    store, planes = None, {}
    for f in range(n):
        k = L.LOOP_ORDER[f]
        if k not in planes:
            ed = O.disparity_module(images[f][0], images[f][1], 64, 8, 4, radius=2, iterations=1)
            planes[k] = (ed, O.classify(O.plane_derivative(ed)[0], (6, 18, -5, 6, 12, 0)))
        rec, pose, nodes = want[f]
        if int(rec["node"][0]) >= 0:
            store = store or R.Store(planes[k][0].shape[1], planes[k][0].shape[0], 4)
            store.insert(f + 1, *planes[k])
        path = os.path.join(d, f"{f + 1}_plane_map_rebuild.bin")
        if nodes is None:
            ref.update(planes[k][0], planes[k][1], pose)
            assert not os.path.exists(path), path
        else:
            assert R.rebuild(ref, store, [2, 4, 6], nodes, pose) == 3
            raw = open(path, "rb").read()
            assert np.frombuffer(raw[:8], "<i4").tolist() == [3, 3] and np.frombuffer(raw[8:], "<u8").tolist() == [2, 4, 6]
        check_dump(os.path.join(d, f"{f + 1}_plane_map.bin"), ref, 3, 50)
    assert int(ref.cells["horizontal"].sum()) + int(ref.cells["vertical"].sum()) > 1000
    # "rebuild" needs the corrected trajectory: any other pose source fails at creation, naming the key
    pose_file = os.path.join(tmp, "poses.txt")
    open(pose_file, "w").write(" ".join(repr(float(v)) for v in M.POSE_IDENTITY) + "\n")
    for bad in (dict(plane_map, pose_key="ego_motion"), dict(plane_map, pose_file=pose_file), dict(plane_map, store_capacity=0)):
        r = run_exe(src, front + [dict(graph_keys, type="pose_graph"), bad], tmp)
        assert r.returncode != 0 and ("store_capacity" if bad.get("store_capacity") == 0 else "rebuild") in r.stderr, (bad, r.stderr)
    r = run_exe(src, front + [plane_map], tmp)                             # without the pose_graph module
    assert r.returncode != 0 and 'requires "pose_graph' in r.stderr, r.stderr

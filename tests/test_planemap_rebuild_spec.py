"""CPU tests of spec S30, rebuilding the plane map from stored keyframes: the restatement tests/np_planemap_rebuild.py
against the hand-worked case of the spec and against sequential np_planemap.Map.update calls, the ring and its id table, and the parts
of the C ABI that need no GPU (exports, argument checks that come before any device call)."""
import ctypes as C
import math

import numpy as np

import np_planemap as M
import np_planemap_rebuild as R

CAM = M.camera(fx=300.0, fy=300.0, cx=80.0, cy=8.0, baseline=0.5)   # fx * baseline = 150: s = 200 is Z = 12 exactly


def pose_at(tx=0.0, ty=0.0, tz=0.0):
    p = list(M.POSE_IDENTITY)
    p[3], p[7], p[11] = tx, ty, tz
    return p


def yaw_pose(deg, t=(0.0, 0.0, 0.0)):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [c, 0.0, s, t[0], 0.0, 1.0, 0.0, t[1], -s, 0.0, c, t[2]]


def random_frame(seed, w, h):
    rng = np.random.default_rng(seed)
    disp = rng.integers(300, 1400, (h, w)).astype(np.int16)
    disp[rng.random((h, w)) < 0.05] = -32768
    return disp, rng.integers(0, 3, (h, w)).astype(np.uint8)


def test_hand_worked_case():
    disp, planes = np.full((9, 160), 200, np.int16), np.ones((9, 160), np.uint8)
    live = M.Map(CAM, 64, 128)
    live.update(disp, planes, pose_at(tz=0.0))
    live.update(disp, planes, pose_at(tz=1.0))                       # the drift: the same wall, one metre further
    assert live.origin == (-32, -64)
    rows = live.cells["vertical"].astype(np.int64).sum(axis=1)
    assert rows[112] == 1440 and rows[116] == 1440 and rows.sum() == 2880   # the wall appears twice
    store = R.Store(160, 9, 4)
    store.insert(10, disp, planes)
    store.insert(20, disp, planes)
    m = M.Map(CAM, 64, 128)
    assert R.rebuild(m, store, [10, 20], [M.POSE_IDENTITY, M.POSE_IDENTITY], pose_at(tz=1.0)) == 2
    assert m.origin == (-32, -64)
    v = m.cells["vertical"].astype(np.int64)
    assert v[112].sum() == 2880 == v.sum() and v.max() == 126
    assert np.flatnonzero(v[112]).tolist() == list(range(19, 45))
    twice = M.Map(CAM, 64, 128)
    twice.update(disp, planes, M.POSE_IDENTITY)
    twice.update(disp, planes, M.POSE_IDENTITY)
    assert twice.origin == m.origin and twice.cells.tobytes() == m.cells.tobytes()


def test_rebuild_equals_sequential_updates_when_every_pose_shares_the_window():
    w, h = 130, 9
    frames = [random_frame(k, w, h) for k in range(4)]
    poses = [yaw_pose(7.0 * k, (0.3 * k, -0.01 * k, 0.5 * k)) for k in range(4)]   # |t| < 4 cells of 0.25: one window
    p = M.params(height_quantum=0.1)
    seq = M.Map(CAM, 64, 48, p)
    store = R.Store(w, h, 8)
    for k, ((d, l), pose) in enumerate(zip(frames, poses)):
        seq.update(d, l, pose)
        store.insert(100 + k, d, l)
    assert len({(M.window_origin(q[3], 0.25, 64), M.window_origin(q[11], 0.25, 48)) for q in poses}) == 1
    m = M.Map(CAM, 64, 48, p)
    m.update(*frames[0], pose_at(tx=50.0))                              # old content elsewhere: nothing of it survives
    assert R.rebuild(m, store, [100, 101, 102, 103], poses, poses[-1]) == 4
    assert m.origin == seq.origin and m.cells.tobytes() == seq.cells.tobytes()
    assert int(m.cells["horizontal"].sum()) + int(m.cells["vertical"].sum()) > 1000
    m2 = M.Map(CAM, 64, 48, p)                                          # exact in any order
    assert R.rebuild(m2, store, [103, 101, 100, 102], [poses[3], poses[1], poses[0], poses[2]], poses[0]) == 4
    assert m2.cells.tobytes() == seq.cells.tobytes()
    m.update(*frames[1], yaw_pose(3.0, (4.3, 0.0, -4.2)))                # and the map goes on like any other
    seq.update(*frames[1], yaw_pose(3.0, (4.3, 0.0, -4.2)))
    assert m.origin == seq.origin == (-16, -48) and m.cells.tobytes() == seq.cells.tobytes()


def test_ring_eviction_and_newest_first_lookup():
    w, h = 16, 4
    frames = [random_frame(50 + k, w, h) for k in range(5)]
    store = R.Store(w, h, 2)
    assert store.size() == (0, 2) and not store.contains(0)
    for k, (d, l) in enumerate(frames):
        store.insert(k, d, l)
    assert store.size() == (2, 2) and [store.contains(k) for k in range(5)] == [False, False, False, True, True]
    assert store.slot_of(3) == 1 and store.slot_of(4) == 0            # insertion n lives in slot n mod capacity
    store.insert(3, *frames[0])                                        # a repeated id names its latest insertion
    assert store.slot_of(3) == 1 and store.frames[1][0].tobytes() == frames[0][0].tobytes() and store.contains(4)
    store = R.Store(w, h, 3)
    store.insert(7, *frames[0])
    store.insert(7, *frames[1])
    assert store.slot_of(7) == 1 and store.size() == (2, 3)
    store.clear()
    assert store.size() == (0, 3) and not store.contains(7)
    store.insert(9, *frames[2])
    assert store.slot_of(9) == 0


def test_duplicated_ids_unknown_ids_and_count_zero():
    disp, planes = np.full((9, 160), 200, np.int16), np.ones((9, 160), np.uint8)
    store = R.Store(160, 9, 2)
    store.insert(5, disp, planes)
    m = M.Map(CAM, 64, 128)
    assert R.rebuild(m, store, [5, 77, 5], [M.POSE_IDENTITY] * 3, M.POSE_IDENTITY) == 2    # 77 was never inserted
    assert int(m.cells["vertical"].sum()) == 2 * 1440 and int(m.cells["vertical"].max()) == 126
    assert R.rebuild(m, store, [], np.zeros((0, 12)), pose_at(tx=40.0, tz=-8.1)) == 0
    assert m.origin == (M.window_origin(40.0, 0.25, 64), M.window_origin(-8.1, 0.25, 128)) == (128, -112)
    assert m.cells.tobytes() == M.empty_cells(128, 64).tobytes()
    m.update(disp, planes, pose_at(tx=40.0, tz=-8.1))                  # valid with that origin: an update continues on it
    assert m.origin == (128, -112) and int(m.cells["vertical"].sum()) == 1440


# ---- the built library, without a GPU ----------------------------------------------------------------------------------------

def _lib():
    from cartslam import _lib as L
    return L, L.load()


def _err(lib):
    return lib.cart_last_error(None).decode()


def test_symbols_and_exports():
    L, lib = _lib()
    for name in ("cart_plane_store_create", "cart_plane_store_destroy", "cart_plane_store_clear", "cart_plane_store_size", "cart_plane_store_insert",
                 "cart_plane_store_contains", "cart_plane_map_rebuild"):
        assert hasattr(lib, name) and name in L.PROTOTYPES, name
    import cartslam
    assert hasattr(cartslam, "PlaneStore") and hasattr(cartslam.PlaneMap, "rebuild")
    for method in ("insert", "contains", "size", "clear", "close"):
        assert hasattr(cartslam.PlaneStore, method)


def test_store_create_refuses_bad_sizes_naming_them():
    L, lib = _lib()
    out = C.c_void_p()
    for w, h, cap, word in ((0, 9, 4, "width"), (160, 16385, 4, "height"), (160, 9, 0, "capacity must be in [1, 1024]"), (160, 9, 1025, "capacity must be in [1, 1024]")):
        assert lib.cart_plane_store_create(None, w, h, cap, C.byref(out)) != 0 and word in _err(lib), (w, h, cap)
    assert lib.cart_plane_store_create(None, 160, 9, 1024, C.byref(out)) != 0 and not out.value and "capacity" not in _err(lib)   # valid but the engine
    assert lib.cart_plane_store_insert(None, 1, None, 0, None, 0, 0, 9, None) != 0 and "width" in _err(lib)
    assert lib.cart_plane_store_insert(None, 1, None, 0, None, 0, 160, 9, None) != 0 and "store" in _err(lib)
    slot, n = C.c_int(0), C.c_int(0)
    assert lib.cart_plane_store_contains(None, 1, C.byref(slot)) != 0 and "store" in _err(lib)
    assert lib.cart_plane_store_size(None, C.byref(n), C.byref(n)) != 0 and "store" in _err(lib)
    assert lib.cart_plane_store_clear(None) != 0 and "store" in _err(lib)
    lib.cart_plane_store_destroy(None)


def test_rebuild_refuses_bad_arguments_naming_them_before_any_device_call():
    L, lib = _lib()
    cam = L.EgoCamera(300.0, 300.0, 80.0, 8.0, 0.5)
    window = (C.c_double * 12)(*M.POSE_IDENTITY)
    ids = (C.c_uint64 * 3)(1, 2, 3)
    used = C.c_int(-5)

    def rebuild(count=3, camera=cam, poses=None, window_pose=window, id_list=ids, m=None, s=None):
        flat = (C.c_double * 36)(*(poses if poses is not None else list(M.POSE_IDENTITY) * 3))
        return lib.cart_plane_map_rebuild(m, s, C.byref(camera), id_list, flat, count, window_pose, C.byref(used), None)

    for count in (-1, 4097):
        assert rebuild(count=count) != 0 and "count must be in [0, 4096]" in _err(lib)
    bad = list(M.POSE_IDENTITY) * 3
    bad[12 + 5] = math.nan
    assert rebuild(poses=bad) != 0 and "poses[1]" in _err(lib)
    bad = list(M.POSE_IDENTITY) * 3
    bad[24 + 3] = 2e6
    assert rebuild(poses=bad) != 0 and "poses[2]" in _err(lib)
    assert rebuild(count=1, poses=bad) != 0 and "map" in _err(lib)    # only the first `count` poses are looked at
    nan_window = (C.c_double * 12)(*([math.nan] + list(M.POSE_IDENTITY)[1:]))
    assert rebuild(window_pose=nan_window) != 0 and "window_pose" in _err(lib)
    assert rebuild(window_pose=None) != 0 and "window_pose" in _err(lib)
    assert rebuild(camera=L.EgoCamera(0.0, 300.0, 80.0, 8.0, 0.5)) != 0 and "fx" in _err(lib)
    assert rebuild(id_list=None) != 0 and "ids" in _err(lib)
    assert lib.cart_plane_map_rebuild(None, None, C.byref(cam), ids, None, 3, window, None, None) != 0 and "poses" in _err(lib)
    assert rebuild() != 0 and "map is NULL" in _err(lib)                # everything valid gets as far as the missing map ...
    assert rebuild(count=0, id_list=None) != 0 and "map is NULL" in _err(lib)
    fake = C.c_void_p(1)                                                 # ... and with a map, as far as the missing store (not dereferenced)
    assert rebuild(m=fake) != 0 and "store is NULL" in _err(lib)
    assert used.value == -5

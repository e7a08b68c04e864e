"""CPU tests of spec S35, rebuilding the TSDF volume from stored keyframes, on the numpy restatement
tests/np_voxelmap_rebuild.py alone: the hand-worked voxel, the equivalence clause (clear + one integrate per used entry where every entry's
own window is the rebuild's), the list order as part of the spec, skipped and repeated ids, an empty list, the correction of a drifted
volume on the accuracy scene of 7.15, and the library's host-side checks (no GPU: validation comes before any device call).
tests/test_gpu_voxelmap_rebuild.py runs the device against the same restatement."""
import ctypes as C

import numpy as np
import pytest

import np_voxelmap as V
import np_voxelmap_rebuild as R
import test_voxelmap_spec as S

INV = V.INVALID


def store_of(frames, capacity=None):
    """frames = [(id, disp, plane or None)] -> R.Store; a missing plane is stored as zeros."""
    h, w = frames[0][1].shape
    store = R.Store(w, h, capacity or len(frames))
    for fid, disp, plane in frames:
        store.insert(fid, disp, plane if plane is not None else np.zeros((h, w), np.uint8))
    return store


def sequential(shape, p, cam, entries):
    """cart_voxel_map_clear, then one integrate per entry (pose, disp, mask).  -> (the map, the origin after every integrate, the summed counts)."""
    m = V.Map(*shape, p)
    origins, counts = [], np.zeros(2, np.int64)
    for pose, disp, mask in entries:
        counts += m.integrate(cam, pose, disp, mask).astype(np.int64)
        origins.append(m.origin)
    return m, origins, counts


def same_maps(a, b):
    (va, oa), (vb, ob) = a.read(), b.read()
    assert tuple(oa) == tuple(ob) and va.tobytes() == vb.tobytes(), f"{int((va != vb).sum())} voxels differ"


def test_hand_worked_voxel():
    """S33's own case (test_voxelmap_spec.test_hand_worked_voxel): identity pose, fx = fy = 256, cx = 8, cy = 4, baseline 0.5, constant
    disparity 64 px, 0.25 m voxels; voxel (0, 0, 7) has obs = 15420.  The frame listed twice, both at the identity, leaves (15420, 2)."""
    disp = np.full((48, 48), 64 * 16, np.int16)
    m = R.Map(32, 32, 64, V.params(voxel_size=0.25))
    origin, used, counts = m.rebuild(store_of([(9, disp, None)]), [9, 9], [V.POSE_IDENTITY] * 2, V.POSE_IDENTITY, S.CAM)
    assert origin == (-16, -16, 0) and used == 2
    vox, o = m.read()
    assert tuple(vox[7 - o[2], 0 - o[1], 0 - o[0]]) == (15420, 2)
    two, _, n = sequential((32, 32, 64), V.params(voxel_size=0.25), S.CAM, [(V.POSE_IDENTITY, disp, None)] * 2)
    same_maps(m, two)
    assert counts.tolist() == n.tolist() and counts[0] > 0


def corridor_frames(n, seed=11, w=160, h=64):
    """The frames of test_voxelmap_spec.corridor_run: road_corridor with +-1/4 px noise and 10 % fresh holes per frame.  -> (truth, [disp])."""
    from cartslam import synth
    truth, _ = synth.road_corridor(w, h, *[S.ACC_CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline")])
    rng = np.random.default_rng(seed)
    ok = truth != INV
    frames = []
    for _ in range(n):
        d = truth.copy()
        d[ok] += rng.integers(-4, 5, int(ok.sum())).astype(np.int16)
        d[ok & (rng.random((h, w)) < 0.10)] = INV
        frames.append(d)
    return truth, frames


def test_equivalence_with_clear_and_sequential_integrates_on_the_corridor():
    """The equivalence clause: every entry's own pose yields the rebuild's window origin (asserted first), so the rebuilt volume is the one
    that clear + one integrate per entry leaves, and the counts are the sums.  The mask plane is used: a block of MOVING pixels."""
    _, frames = corridor_frames(4)
    poses = [S.pose_t(tx=0.01 * k, tz=0.02 * k) for k in range(4)]
    mask = np.zeros((64, 160), np.uint8)
    mask[30:50, 20:60] = V.MOVING
    seq, origins, n = sequential(S.ACC_SHAPE, V.params(), S.ACC_CAM, [(poses[k], frames[k], mask) for k in range(4)])
    assert len(set(origins)) == 1
    m = R.Map(*S.ACC_SHAPE)
    origin, used, counts = m.rebuild(store_of([(k + 1, frames[k], mask) for k in range(4)]), [1, 2, 3, 4], poses, poses[3], S.ACC_CAM, use_mask=True)
    assert origin == origins[0] and used == 4 and counts.tolist() == n.tolist()
    same_maps(m, seq)
    unmasked = R.Map(*S.ACC_SHAPE)
    assert unmasked.rebuild(store_of([(k + 1, frames[k], mask) for k in range(4)]), [1, 2, 3, 4], poses, poses[3], S.ACC_CAM)[2][0] > counts[0]


def order_case():
    """max_weight = 2, three frames of constant disparity 20, 21.5 and 23.25 px on the small volume, one window.  -> (store, poses, params)"""
    frames = [(k + 1, np.full((10, 24), s, np.int16), None) for k, s in enumerate((320, 344, 372))]
    return store_of(frames), [S.pose_t()] * 3, V.params(max_weight=2, **S.SMALL)


def test_the_list_order_is_part_of_the_spec():
    """With three entries the weight is 0, 1, 2 when they arrive, so the last step is still a true mean: the two orders differ by the
    rounding of the intermediate mean alone (t2 = floor((a + b + 1) / 2) carries half a unit into the last division where a + b is odd).
    The surfaces lie at 0.6, 0.558 and 0.516 m, inside each other's truncation band, so the voxels between them hold three different obs."""
    store, poses, p = order_case()
    a, b = R.Map(16, 16, 24, p), R.Map(16, 16, 24, p)
    ra, rb = a.rebuild(store, [1, 2, 3], poses, poses[0], S.SMALL_CAM), b.rebuild(store, [3, 2, 1], poses, poses[0], S.SMALL_CAM)
    assert ra[0] == rb[0] and ra[1] == rb[1] == 3 and ra[2].tolist() == rb[2].tolist()
    (va, _), (vb, _) = a.read(), b.read()
    assert (va["weight"] == vb["weight"]).all() and va["weight"].max() == 2
    differ = int((va["tsdf"] != vb["tsdf"]).sum())
    print("voxels that differ between the two orders:", differ)
    assert differ > 0 and np.abs(va["tsdf"].astype(int) - vb["tsdf"].astype(int)).max() == 1
    # a fourth entry meets the cap: the mean becomes an exponential one and the orders differ by far more than a rounding
    ids = [1, 2, 3, 3]
    a.rebuild(store, ids, poses + poses[:1], poses[0], S.SMALL_CAM)
    b.rebuild(store, ids[::-1], poses + poses[:1], poses[0], S.SMALL_CAM)
    assert np.abs(a.read()[0]["tsdf"].astype(int) - b.read()[0]["tsdf"].astype(int)).max() > 100


def test_skipped_ids_a_repeated_id_and_an_empty_list():
    frames = [(k, *S.small_frame(40 + k)) for k in range(3)]
    p = V.params(**S.SMALL)
    poses = [S.pose_t(), S.yaw_pose(7.0, (0.05, -0.02, 0.1)), S.yaw_pose(-11.0, (0.1, 0.0, 0.3))]
    store = store_of(frames, capacity=2)                                      # frame 0 is evicted
    assert [store.slot_of(k) for k in (0, 1, 2, 7)] == [-1, 1, 0, -1]
    m = R.Map(16, 16, 24, p)
    origin, used, counts = m.rebuild(store, [0, 1, 7, 2], poses + [poses[0]], poses[1], S.SMALL_CAM, use_mask=True)
    assert used == 2 and origin == V.window_origin(poses[1], p, (16, 16, 24))
    only = R.Map(16, 16, 24, p)
    assert only.rebuild(store, [1, 2], [poses[1], poses[0]], poses[1], S.SMALL_CAM, use_mask=True)[2].tolist() == counts.tolist()
    same_maps(m, only)                                                        # the skipped entries left no trace; entry 2 went through the pose listed with it
    # an id listed twice is integrated twice
    twice = R.Map(16, 16, 24, p)
    assert twice.rebuild(store, [1, 1], [poses[0]] * 2, poses[0], S.SMALL_CAM)[1] == 2
    seq, _, n = sequential((16, 16, 24), p, S.SMALL_CAM, [(poses[0], frames[1][1], None)] * 2)
    same_maps(twice, seq)
    assert twice.read()[0]["weight"].max() == 2
    # a repeated id names its latest insertion
    store.insert(1, *frames[0][1:])
    latest = R.Map(16, 16, 24, p)
    latest.rebuild(store, [1], [poses[0]], poses[0], S.SMALL_CAM)
    same_maps(latest, sequential((16, 16, 24), p, S.SMALL_CAM, [(poses[0], frames[0][1], None)])[0])
    # count = 0, and nothing known: an empty valid window at the new origin, over whatever the map held
    for ids in ([], [7, 8]):
        origin, used, counts = latest.rebuild(store, ids, [poses[0]] * len(ids), S.pose_t(tx=9.0, tz=-30.0), S.SMALL_CAM)
        assert used == 0 and counts.tolist() == [0, 0] and origin == latest.origin == (64, -8, -240)
        vox, o = latest.read()
        assert tuple(o) == origin and not vox["tsdf"].any() and not vox["weight"].any()
    # the map continues as after any integrate: the next integrate moves the window from the rebuild's origin
    latest.integrate(S.SMALL_CAM, S.pose_t(tx=9.0, tz=-29.0), frames[1][1])
    assert latest.origin == (64, -8, -232)


def test_entries_are_integrated_into_the_fixed_window_not_their_own():
    """Poses whose own windows differ from the rebuild's: the window stays where window_pose puts it, and a voxel outside it does not exist."""
    frames = [(k, *S.small_frame(70 + k, masked=False)) for k in range(3)]
    p = V.params(**S.SMALL)
    poses = [S.pose_t(), S.pose_t(tz=1.0), S.pose_t(tx=-1.0, tz=0.5)]
    assert len({V.window_origin(q, p, (16, 16, 24)) for q in poses}) == 3
    m = R.Map(16, 16, 24, p)
    origin, used, counts = m.rebuild(store_of(frames), [0, 1, 2], poses, poses[1], S.SMALL_CAM)
    assert origin == (-8, -8, 8) == m.origin and used == 3
    seq, origins, n = sequential((16, 16, 24), p, S.SMALL_CAM, [(poses[k], frames[k][1], None) for k in range(3)])
    assert 0 < counts[0] < n[0] and m.read()[0]["weight"].max() >= 2         # fewer voxels than in the windows of their own, and some seen twice


# ---- the correction itself ----------------------------------------------------------------------------------------------------------
# measured on the restatement at seed 11: rms error in px at the HIT pixels of the raycast from the last true pose
CORRECTION = dict(drifted=0.7785, rebuilt=0.0480)


def correction_run(n=12, step=0.25):
    """Twelve corridor frames along a forward path, integrated at poses with an accumulating drift (3 cm to the side and 0.4 degrees of yaw
    per frame), then rebuilt from the same frames at the true poses.  -> the rms error of both raycasts from the last true pose."""
    truth, frames = corridor_frames(n)
    true = [S.pose_t(tz=step * k) for k in range(n)]
    drifted = [S.yaw_pose(0.4 * k, (0.03 * k, 0.0, step * k)) for k in range(n)]
    ok = truth != INV

    def rms(m):
        r = m.raycast(S.ACC_CAM, true[-1], 160, 64)
        hit = (r["status"] == V.HIT) & ok
        return float(np.sqrt(((((r["disp"].astype(np.float64) - truth) / 16.0)[hit]) ** 2).mean())), int(hit.sum())

    m = R.Map(*S.ACC_SHAPE)
    for pose, d in zip(drifted, frames):
        m.integrate(S.ACC_CAM, pose, d)
    before = rms(m)
    _, used, _ = m.rebuild(store_of([(k, d, None) for k, d in enumerate(frames)]), list(range(n)), true, true[-1], S.ACC_CAM)
    assert used == n
    return dict(drifted=before[0], rebuilt=rms(m)[0], hits=(before[1], rms(m)[1]))


def test_a_rebuild_at_the_true_poses_removes_the_drift():
    """Measured values: see CORRECTION and DESIGN.md 7.17.  The bound on the rebuilt figure sits at twice the measured distance to the ideal
    (0 px), 7.15's convention, and the rebuilt figure lies below the drifted one."""
    got = correction_run()
    print(got)
    assert got["hits"][1] > 3000
    assert got["rebuilt"] <= 2 * CORRECTION["rebuilt"]
    assert got["rebuilt"] < got["drifted"]


# ---- the library's host side --------------------------------------------------------------------------------------------------------
def rebuild_error(count=2, use_mask=0, cam=S.CAM, poses=None, window=V.POSE_IDENTITY, ids=(1, 2)):
    """cart_voxel_map_rebuild without objects: a valid configuration gets as far as the missing map."""
    from cartslam import _lib
    lib = _lib.load()
    c = C.byref(_lib.EgoCamera(*[cam[k] for k in ("fx", "fy", "cx", "cy", "baseline")])) if cam is not None else None
    flat = list(V.POSE_IDENTITY) * 2 if poses is None else poses
    rc = lib.cart_voxel_map_rebuild(None, None, c, (C.c_uint64 * 2)(*ids) if ids is not None else None, (C.c_double * len(flat))(*flat) if flat else None, count,
                                    (C.c_double * 12)(*window) if window is not None else None, use_mask, None, None, None)
    assert rc != 0
    return lib.cart_last_error(None).decode()


def test_argument_checks_without_an_object():
    from cartslam import VoxelMap, _lib
    assert "cart_voxel_map_rebuild" in _lib.PROTOTYPES and hasattr(VoxelMap, "rebuild")
    assert rebuild_error() == "map is NULL" and rebuild_error(count=0, ids=None, poses=[]) == "map is NULL"
    for kw, word in ((dict(count=-1), "count"), (dict(count=4097), "count"), (dict(use_mask=2), "use_mask"), (dict(use_mask=-1), "use_mask"), (dict(cam=None), "camera"),
                     (dict(cam=dict(S.CAM, fy=0.0)), "fy"), (dict(window=None), "window_pose is NULL"), (dict(ids=None), "ids is NULL"), (dict(poses=[]), "poses is NULL")):
        assert word in rebuild_error(**kw), kw
    bad = list(V.POSE_IDENTITY) * 2
    bad[12 + 7] = float("nan")
    assert "poses[1][7]" in rebuild_error(poses=bad)
    w = list(V.POSE_IDENTITY)
    w[3] = 2e6
    assert "window_pose[3]" in rebuild_error(window=w)
    # the order: count and use_mask, the camera, window_pose, the entries' poses, the map
    assert "count" in rebuild_error(count=-1, use_mask=2, cam=None) and "use_mask" in rebuild_error(use_mask=2, cam=None)
    assert "camera" in rebuild_error(cam=None, window=None) and "window_pose" in rebuild_error(window=None, poses=bad)

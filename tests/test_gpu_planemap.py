"""GPU tests of the world-frame plane map (spec S24): cart_plane_map_* through cartslam.PlaneMap against the numpy
restatement tests/np_planemap.py, byte for byte, and the plane_map host module in the C++ frame loop.  Written without a GPU in reach: the
numeric premises asserted beside the byte comparisons were checked against the restatement alone; the comparisons themselves have not run."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import np_planemap as M

pytestmark = pytest.mark.gpu

CAM = M.camera(fx=300.0, fy=300.0, cx=80.0, cy=8.0, baseline=0.5)     # fx * baseline = 150: s = 200 is Z = 12 exactly
NEAR = M.camera(fx=30.0, fy=30.0, cx=33.0, cy=2.0, baseline=0.5)      # one pixel is 5 cm at Z = 1.5


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


def make_map(cam, nx, nz, p=None, eng=None):
    from cartslam import PlaneMap, plane_map_params
    return PlaneMap(eng or engine(), cam_tuple(cam), nx, nz, plane_map_params(**(p or M.params())))


def pitched(a, extra):
    """A device tensor of `a` whose rows are `extra` elements longer than the image, the slack filled with values that would vote."""
    torch = _torch()
    h, w = a.shape
    full = np.full((h, w + extra), 1 if a.dtype == np.uint8 else 200, a.dtype)
    full[:, :w] = a
    return torch.from_numpy(full).cuda()[:, :w]


def pose_at(tx=0.0, ty=0.0, tz=0.0):
    p = list(M.POSE_IDENTITY)
    p[3], p[7], p[11] = tx, ty, tz
    return p


def yaw_pose(deg, t=(0.0, 0.0, 0.0)):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [c, 0.0, s, t[0], 0.0, 1.0, 0.0, t[1], -s, 0.0, c, t[2]]


def random_frame(seed, w, h, lo=300, hi=1400):
    rng = np.random.default_rng(seed)
    disp = rng.integers(lo, hi, (h, w)).astype(np.int16)
    disp[rng.random((h, w)) < 0.05] = -32768
    return disp, rng.integers(0, 3, (h, w)).astype(np.uint8)


def check(cam, nx, nz, p, frames, extra=(3, 5), thresholds=((3, 50),)):
    """frames = [(disp, planes, pose)] voted in order into one map and one restatement: the origin, the cells and the classes agree
    after every frame.  -> the restatement."""
    m, ref = make_map(cam, nx, nz, p), M.Map(cam, nx, nz, p)
    try:
        for k, (disp, planes, pose) in enumerate(frames):
            got_origin = m.update(pitched(disp, extra[0] * 2), pitched(planes, extra[1]), pose, raw=True)
            exp_origin = ref.update(disp, planes, pose)
            cells, origin = m.read()
            assert got_origin == exp_origin == origin == m.window()[:2], f"frame {k}"
            assert cells.tobytes() == ref.cells.tobytes(), f"frame {k}: {int((cells != ref.cells).sum())} cells differ"
            for mv, pc in thresholds:
                assert m.classify(mv, pc).tobytes() == ref.classify(mv, pc).tobytes(), f"frame {k}: classes ({mv}, {pc})"
    finally:
        m.close()
    return ref


@pytest.mark.parametrize("w,h", [(67, 5), (130, 9), (256, 16)])
def test_kernel_edges_with_pitched_rows(w, h):
    disp, planes = random_frame(w * h, w, h)
    disp[h // 2, :] = 200                                      # one wall row among the noise: long runs next to runs of one
    ref = check(CAM, 64, 48, M.params(), [(disp, planes, M.POSE_IDENTITY), (disp, planes, yaw_pose(30.0, (0.3, 0.0, -0.7)))])
    assert int(ref.cells["horizontal"].sum()) + int(ref.cells["vertical"].sum()) > w * h // 2


@pytest.mark.parametrize("label", [0, 1])
def test_maximal_contention_counts_every_pixel(label):
    disp, planes = np.full((16, 256), 200, np.int16), np.full((16, 256), label, np.uint8)
    ref = check(CAM, 32, 32, M.params(cell_size=64.0), [(disp, planes, pose_at(tx=20.0))])   # Xw in [14.9, 25.1], Zw = 12: cell (0, 0)
    field = "vertical" if label else "horizontal"
    assert int(ref.cells[field][16, 16]) == 4096 and int(ref.cells[field].sum()) == 4096


@pytest.mark.parametrize("pattern", ["pixels", "rows", "columns"])
def test_shortest_runs_with_alternating_labels(pattern):
    h, w = 16, 256
    y, x = np.indices((h, w))
    planes = ({"pixels": x + y, "rows": y, "columns": x}[pattern] % 2).astype(np.uint8)
    disp = np.full((h, w), 200, np.int16)
    disp[:, 100:140] = 640                                     # a nearer block: other cells in the middle of the rows
    ref = check(CAM, 64, 64, M.params(), [(disp, planes, M.POSE_IDENTITY)])
    assert int(ref.cells["horizontal"].sum()) == int(ref.cells["vertical"].sum()) > 0


@pytest.mark.parametrize("w,h", [(67, 9), (256, 16)])
def test_every_pixel_in_its_own_cell(w, h):
    y, x = np.indices((h, w))
    disp, planes = (160 + 2 * y).astype(np.int16), ((x + y) % 2).astype(np.uint8)   # Z = 15 / (10 + y / 8): 2 cm per row, 5 cm per column
    ref = check(NEAR, 512, 512, M.params(cell_size=0.01), [(disp, planes, M.POSE_IDENTITY)])
    n = ref.cells["horizontal"].astype(np.int64) + ref.cells["vertical"]
    assert n.max() == 1 and n.sum() >= min(w, 67) * h          # nothing merges; columns beyond +- 2.56 m fall outside the window


def test_ignored_labels_invalid_disparities_and_votes_outside_the_window():
    disp, planes = random_frame(5, 130, 9)
    planes[0, :] = 2
    planes[1, ::2] = 7
    planes[2, :] = 255
    disp[3, :] = -32768
    disp[4, :] = 0
    disp[5, :] = -16
    disp[6, :] = 100                                           # Z = 24 > max_depth
    ref = check(CAM, 32, 32, M.params(), [(disp, planes, M.POSE_IDENTITY), (disp, planes, pose_at(tx=-7.9, tz=-3.0))])   # most votes leave +- 4 m
    total = int(ref.cells["horizontal"].sum()) + int(ref.cells["vertical"].sum())
    assert 0 < total < 2 * 130 * 2


def test_gate_boundaries():
    disp, planes = np.full((9, 160), 200, np.int16), np.ones((9, 160), np.uint8)
    disp[1::2] = 199                                           # d = 12.4375, Z = 12.06
    for p, rows, cols in ((M.params(min_disparity=12.5), 5, 160), (M.params(min_disparity=12.4375), 9, 160), (M.params(max_depth=12.0), 5, 160),
                          (M.params(max_depth=150.0 / 12.4375), 9, 160), (M.params(max_lateral=2.0), 9, None)):
        ref = check(CAM, 128, 128, p, [(disp, planes, M.POSE_IDENTITY)])
        if cols is not None:
            assert int(ref.cells["vertical"].sum()) == rows * cols, p
        else:   # X = (x - 80) Z / 300: at Z = 12 exactly +-2 for x = 30 and 130 (101 columns); at Z = 12.06 x = 31..129 (99 columns)
            assert int(ref.cells["vertical"].sum()) == 5 * 101 + 4 * 99


def test_poses_yaw_90_and_negative_translations():
    disp, planes = np.full((9, 160), 400, np.int16), np.ones((9, 160), np.uint8)    # Z = 6
    ref = check(CAM, 64, 64, M.params(), [(disp, planes, yaw_pose(90.0))])
    assert int(ref.cells["vertical"][:, 24 - ref.origin[0]].sum()) == 9 * 160       # camera Z became world X
    disp, planes = random_frame(6, 130, 9)
    check(CAM, 64, 48, M.params(cell_size=0.5, height_quantum=0.1),
          [(disp, planes, yaw_pose(-37.0, (-5.1, -0.2, -2.6))), (disp, planes, yaw_pose(200.0, (-1e5 - 0.3, 40.0, -77.7)))])


def test_window_moves_and_clear():
    nx, nz, cs = 64, 48, 0.25
    steps = [(0, 0), (0, 0), (16, 0), (-16, 0), (nx - 16, 0), (0, nz - 16), (0, -16), (16, 16), (-16, 16), (nx, 0), (0, 0), (16, -nz - 16), (-32, -16)]
    frames, cx, cz = [], 0, 0
    for k, (dx, dz) in enumerate(steps):
        cx, cz = cx + dx, cz + dz
        disp, planes = random_frame(100 + k, 130, 9)
        frames.append((disp, planes, yaw_pose(25.0 * k, (cx * cs + 0.1, 0.0, cz * cs + 0.2))))
    ref = check(CAM, nx, nz, M.params(cell_size=cs), frames)
    assert ref.origin == (16 * ((cx - nx // 2) // 16), 16 * ((cz - nz // 2) // 16)) == (64, -64)
    # clear: the next update starts an empty window
    m, ref = make_map(CAM, nx, nz), M.Map(CAM, nx, nz)
    for disp, planes, pose in frames[:2]:
        m.update(disp, planes, pose)
    m.clear()
    assert m.window() == (0, 0, False) and m.read()[0].tobytes() == M.empty_cells(nz, nx).tobytes() and (m.classify() == 2).all()
    m.update(*frames[2])
    ref.update(*frames[2])
    assert m.read()[0].tobytes() == ref.cells.tobytes() and m.window() == (*ref.origin, True)
    m.close()


def test_classes_on_and_off_the_thresholds():
    y, x = np.indices((16, 256))
    disp, planes = np.full((16, 256), 200, np.int16), (y % 3 == 0).astype(np.uint8)   # 6 of 16 rows vertical: 37.5 % in every hit cell
    ref = check(CAM, 128, 128, M.params(), [(disp, planes, M.POSE_IDENTITY)], thresholds=((1, 37), (1, 38), (16, 37), (17, 37), (96, 37), (97, 37), (112, 37), (113, 37), (1, 100), (1, 1)))
    row = ref.cells[48 - ref.origin[1]]
    assert set(np.unique(row["horizontal"] + row["vertical"])) == {0, 16, 80, 96, 112}   # cells 1, 5, 6 and 7 pixels wide
    assert set(np.unique(ref.classify(1, 37))) == {1, 2} and set(np.unique(ref.classify(1, 38))) == {0, 2}
    assert set(np.unique(ref.classify(97, 37))) == {1, 2} and (ref.classify(113, 37) == 2).all()


def test_full_size_frame_repeats_and_two_streams():
    torch = _torch()
    from cartslam import synth
    kitti = M.camera(721.5, 721.5, 609.5, 172.85, 0.54)
    disp, planes = synth.road_corridor(1242, 375, *cam_tuple(kitti))
    poses = [M.POSE_IDENTITY, yaw_pose(4.0, (0.3, -0.02, 1.1)), yaw_pose(9.0, (0.9, -0.03, 4.2))]
    ref = check(kitti, 512, 512, M.params(), [(disp, planes, p) for p in poses])
    assert int(ref.cells["vertical"].max()) > 5000 and int((ref.cells["horizontal"] > 0).sum()) > 1500   # wall cells take whole columns
    expect = ref.cells.tobytes()
    d, l = torch.from_numpy(disp).cuda(), torch.from_numpy(planes).cuda()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    maps = [make_map(kitti, 512, 512) for _ in range(3)]
    for p in poses:                      # map 0 alternates between two streams, maps 1 and 2 run side by side on one each
        for m, s in ((maps[0], a if p is poses[1] else b), (maps[1], a), (maps[2], b)):
            with torch.cuda.stream(s):
                m.update(d, l, p, raw=True)
    for m in maps:
        assert m.read()[0].tobytes() == expect
        assert m.read()[0].tobytes() == expect
        m.close()


def test_bad_arguments():
    torch = _torch()
    from cartslam import EngineError, PlaneMap, _lib, plane_map_params
    lib = _lib.load()
    with pytest.raises(EngineError, match="cells_x"):
        PlaneMap(engine(), cam_tuple(CAM), 48 + 8, 64)
    with pytest.raises(EngineError, match="height_quantum"):
        PlaneMap(engine(), cam_tuple(CAM), 64, 64, plane_map_params(height_quantum=0.0))
    m = make_map(CAM, 64, 48)
    disp, planes = (torch.from_numpy(a).cuda() for a in random_frame(1, 130, 9))
    pose = (C.c_double * 12)(*M.POSE_IDENTITY)
    cam = _lib.EgoCamera(*cam_tuple(CAM))

    def update(d=disp.data_ptr(), ds=260, p=planes.data_ptr(), ps=130, w=130, h=9):
        rc = lib.cart_plane_map_update(m._h, C.byref(cam), pose, C.c_void_p(d), ds, C.c_void_p(p), ps, w, h, None)
        return rc, lib.cart_last_error(None).decode()

    for kw, word in ((dict(d=None), "NULL"), (dict(p=None), "NULL"), (dict(d=disp.data_ptr() + 1), "aligned"), (dict(ds=261), "aligned"), (dict(ds=258), "disparity_step"),
                     (dict(ps=129), "planes_step"), (dict(w=0), "width"), (dict(h=20000), "height")):
        rc, err = update(**kw)
        assert rc != 0 and word in err, (kw, err)
    with pytest.raises(EngineError, match="pose"):
        m.update(disp, planes, [math.nan] * 12, raw=True)
    with pytest.raises(EngineError):
        m.update(disp.cpu(), planes, M.POSE_IDENTITY, raw=True)
    for mv, pc, word in ((0, 50, "min_votes"), (3, 0, "obstacle_percent"), (3, 101, "obstacle_percent")):
        with pytest.raises(EngineError, match=word):
            m.classify(mv, pc)
    out = torch.empty((48, 64), dtype=torch.uint8, device="cuda")
    assert lib.cart_plane_map_classify(m._h, 3, 50, None, 64, None) != 0 and lib.cart_plane_map_classify(m._h, 3, 50, C.c_void_p(out.data_ptr()), 63, None) != 0
    assert lib.cart_plane_map_read(m._h, None, None, None, None) != 0
    assert m.window() == (0, 0, False)                         # no refused call touched the map
    m.close()


def test_lifecycle():
    torch = _torch()
    from cartslam import Engine, EngineError
    disp, planes = random_frame(2, 130, 9)
    ref = M.Map(CAM, 64, 48)
    ref.update(disp, planes, M.POSE_IDENTITY)
    m = make_map(CAM, 64, 48)
    m.update(disp, planes, M.POSE_IDENTITY)
    m.close()
    m.close()
    for call in (lambda: m.update(disp, planes, M.POSE_IDENTITY), m.read, m.classify, m.clear, m.window):
        with pytest.raises(EngineError):
            call()
    other = Engine(64, 32, num_disparities=0, paths=0)         # closed after its engine
    m = make_map(CAM, 64, 48, eng=other)
    m.update(disp, planes, M.POSE_IDENTITY)
    other.close()
    assert m.read()[0].tobytes() == ref.cells.tobytes()
    m.close()
    d, l = torch.from_numpy(disp).cuda(), torch.from_numpy(planes).cuda()

    def cycle(n):
        for _ in range(n):
            o = make_map(CAM, 512, 512)
            o.update(d, l, M.POSE_IDENTITY, raw=True)
            o.classify(raw=True)
            o.close()
        torch.cuda.synchronize()
    cycle(3)
    free0 = torch.cuda.mem_get_info()[0]
    cycle(20)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"plane map leak: {(free0 - free1) >> 20} MiB over 20 create/use/close cycles"


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------
HEADER = np.dtype([("ox", "<i8"), ("oz", "<i8"), ("nx", "<i4"), ("nz", "<i4"), ("cell_size", "<f8")])


def check_dump(path, ref, min_votes, percent):
    raw = open(path, "rb").read()
    nx, nz = ref.nx, ref.nz
    assert len(raw) == HEADER.itemsize + nx * nz * 16 + nx * nz, path
    head = np.frombuffer(raw, HEADER, 1)[0]
    assert (int(head["ox"]), int(head["oz"])) == ref.origin and (int(head["nx"]), int(head["nz"])) == (nx, nz) and float(head["cell_size"]) == ref.p["cell_size"]
    assert raw[HEADER.itemsize:HEADER.itemsize + nx * nz * 16] == ref.cells.tobytes(), path + ": cells"
    assert raw[HEADER.itemsize + nx * nz * 16:] == ref.classify(min_votes, percent).tobytes(), path + ": classes"


def test_plane_map_module_with_a_pose_file(tmp_path):
    import oracle_lib as O
    from test_host import make_dataset, run_exe
    tmp = str(tmp_path)
    n, w, h = 3, 160, 64
    src, frames = make_dataset(tmp, n, w, h)
    poses = [yaw_pose(3.0 * f, (0.35 * f, -0.01 * f, 8.3 * f)) for f in range(n)]     # frame 2 moves the window by 16 rows
    pose_file = os.path.join(tmp, "poses.txt")
    with open(pose_file, "w") as fh:
        for p in poses[:2]:
            fh.write(" ".join(repr(float(v)) for v in p) + "\n")
        fh.write("1 0 0\n")                                    # frame 3: a short line is no pose
    static = {"type": "static", "horizontal_range_min": 6, "horizontal_range_max": 18, "vertical_range_min": -5, "vertical_range_max": 6}
    keys = dict(fx=300.0, fy=300.0, cx=80.0, cy=20.0, baseline=0.1)       # disparities of about 5 pixels: 6 m
    extra = dict(cells_x=64, cells_z=48, cell_size=0.5, max_depth=30.0, min_disparity=4.0, height_quantum=0.1, min_votes=2, obstacle_percent=40)
    modules = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
               {"type": "disparity_planeseg", "parameter_provider": static},
               dict(keys, type="plane_map", pose_file=pose_file, **extra)]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, modules, tmp, ("--dump", d))
    assert r.returncode == 2 and "no pose for frame 3" in r.stderr, r.stderr     # frames 1 and 2 ran, frame 3 failed with a message
    cam = M.camera(**keys)
    ref = M.Map(cam, 64, 48, M.params(cell_size=0.5, max_depth=30.0, min_disparity=4.0, height_quantum=0.1))
    for f in range(2):
        l, rr = frames[f]
        ed = O.disparity_module(l, rr, 64, 8, 4, radius=2, iterations=1)
        ep = O.classify(O.plane_derivative(ed)[0], (6, 18, -5, 6, 12, 0))
        ref.update(ed, ep, poses[f])
        assert int(ref.cells["horizontal"].sum()) + int(ref.cells["vertical"].sum()) > 3000 * (f + 1) and ref.origin == (-32, -32 + 16 * f)
        check_dump(os.path.join(d, f"{f + 1}_plane_map.bin"), ref, 2, 40)
    assert not os.path.exists(os.path.join(d, "3_plane_map.bin"))
    # configuration errors name their key
    for bad, word in ((dict(keys, type="plane_map", pose_file=pose_file, cells_x=40), "cells_x"), (dict(type="plane_map", pose_file=pose_file), "fx"),
                      (dict(keys, type="plane_map", pose_file=pose_file, cell_size=0.001), "cell_size"),
                      (dict(keys, type="plane_map", pose_file=pose_file, obstacle_percent=0), "obstacle_percent"),
                      (dict(keys, type="plane_map", pose_file=os.path.join(tmp, "missing.txt")), "pose_file")):
        r = run_exe(src, modules[:2] + [bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    r = run_exe(src, modules[:2] + [dict(keys, type="plane_map")], tmp)
    assert r.returncode != 0 and 'requires "ego_motion"' in r.stderr


def test_plane_map_module_takes_the_pose_of_ego_motion(tmp_path):
    import json
    import oracle_lib as O
    from test_gpu_matches import noise_frame, noise_world
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n = 2
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
    modules = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
               {"type": "disparity_planeseg", "parameter_provider": static},
               {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion"), dict(keys, type="plane_map", **grid)]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, modules, tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    ref = M.Map(M.camera(**keys), 64, 64, M.params(cell_size=1.0, max_depth=40.0, max_lateral=30.0))
    for f in range(n):
        l, rr = images[f]
        ed = O.disparity_module(l, rr, 64, 8, 4, radius=2, iterations=1)
        ep = O.classify(O.plane_derivative(ed)[0], (6, 18, -5, 6, 12, 0))
        pose = np.fromfile(os.path.join(d, f"{f + 1}_ego_motion.bin"), np.float64)[15:]     # the pose the same run reports
        assert len(pose) == 12 and (f == 0) == (pose.tolist() == list(M.POSE_IDENTITY))
        ref.update(ed, ep, pose)
        check_dump(os.path.join(d, f"{f + 1}_plane_map.bin"), ref, 3, 50)
    assert int(ref.cells["horizontal"].sum()) + int(ref.cells["vertical"].sum()) > 1000

"""CPU tests of the plane map spec S24: the numpy restatement tests/np_planemap.py against expectations worked out
by hand or by a scalar Python loop that shares no code with it, and the parts of the C ABI that need no GPU (exports, layouts,
defaults, argument checks that come before any device call)."""
import ctypes as C
import math

import numpy as np

import np_planemap as M

W, H = 160, 48
CAM = M.camera(fx=300.0, fy=300.0, cx=80.0, cy=8.0, baseline=0.5)   # fx * baseline = 150


def pose_at(tx=0.0, ty=0.0, tz=0.0):
    p = list(M.POSE_IDENTITY)
    p[3], p[7], p[11] = tx, ty, tz
    return p


def yaw_pose(deg, t=(0.0, 0.0, 0.0)):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return [c, 0.0, s, t[0], 0.0, 1.0, 0.0, t[1], -s, 0.0, c, t[2]]


def wall(depth_s16):
    return np.full((H, W), depth_s16, np.int16), np.ones((H, W), np.uint8)


def scalar_votes(cam, p, pose, disp, planes):
    """S24 pixel by pixel in Python floats (IEEE doubles, one rounding per operation) -> {(gx, gz): [h, v, y_min, y_max]} over ALL cells."""
    cells = {}
    for y in range(disp.shape[0]):
        for x in range(disp.shape[1]):
            l, s = int(planes[y, x]), int(disp[y, x])
            if l not in (0, 1) or s == -32768:
                continue
            d = s / 16.0
            if not d >= p["min_disparity"]:
                continue
            Z = (cam["fx"] * cam["baseline"]) / d
            if not Z <= p["max_depth"]:
                continue
            X = ((x - cam["cx"]) * Z) / cam["fx"]
            if not -p["max_lateral"] <= X <= p["max_lateral"]:
                continue
            Y = ((y - cam["cy"]) * Z) / cam["fy"]
            pw = [((pose[4 * r] * X + pose[4 * r + 1] * Y) + pose[4 * r + 2] * Z) + pose[4 * r + 3] for r in range(3)]
            key = (math.floor(pw[0] / p["cell_size"]), math.floor(pw[2] / p["cell_size"]))
            c = cells.setdefault(key, [0, 0, M.INT32_MAX, M.INT32_MIN])
            c[l] += 1
            if l == 1:
                q = int(min(max(math.floor(pw[1] / p["height_quantum"]), -2 ** 30), 2 ** 30))
                c[2], c[3] = min(c[2], q), max(c[3], q)
    return cells


def windowed(cells_by_abs, origin, nx, nz):
    out = M.empty_cells(nz, nx)
    for (gx, gz), c in cells_by_abs.items():
        if origin[0] <= gx < origin[0] + nx and origin[1] <= gz < origin[1] + nz:
            out[gz - origin[1], gx - origin[0]] = tuple(c)
    return out


def test_window_origin_uses_floor_division():
    assert M.window_origin(0.0, 0.25, 32) == -16 and M.window_origin(0.0, 0.25, 512) == -256
    assert M.window_origin(-0.1, 0.25, 32) == -32          # c = -1: 16 * floor(-17 / 16), truncation would give -16
    assert M.window_origin(3.99, 0.25, 32) == -16 and M.window_origin(4.0, 0.25, 32) == 0   # c = 15 | 16
    assert M.window_origin(-4.0, 0.25, 32) == -32 and M.window_origin(-4.01, 0.25, 32) == -48
    assert M.window_origin(1e6, 0.01, 4096) == 10 ** 8 - 2048


def test_ground_votes_are_horizontal_only():
    # a ground plane 1.5 m under the camera: y - cy = fy 1.5 / Z, d = fx b / Z = (y - cy) / 3, rounded to the disparity grid
    y = np.arange(H)[:, None] + np.zeros((1, W), np.int64)
    disp = np.round(16.0 * (y - CAM["cy"]) / 3.0).astype(np.int16)
    planes = np.zeros((H, W), np.uint8)
    m = M.Map(CAM, 256, 256)            # 20 m of depth are 80 cells: all of them inside [-128, 128)
    assert m.update(disp, planes, M.POSE_IDENTITY) == (-128, -128)
    cells, _ = m.read()
    expect = scalar_votes(CAM, m.p, M.POSE_IDENTITY, disp, planes)
    accepted = sum(c[0] for c in expect.values())
    assert accepted > 1000 and int(cells["horizontal"].sum()) == accepted        # Z <= 20 and |X| <= 10 leave the lower rows
    assert int(cells["vertical"].sum()) == 0 and (cells["y_min"] == M.INT32_MAX).all() and (cells["y_max"] == M.INT32_MIN).all()
    assert cells.tobytes() == windowed(expect, (-128, -128), 256, 256).tobytes()


def test_wall_lands_in_its_row_with_its_quantised_extent():
    disp, planes = wall(200)            # d = 12.5, Z = 150 / 12.5 = 12 exactly
    m = M.Map(CAM, 128, 128)
    m.update(disp, planes, M.POSE_IDENTITY)
    cells, (ox, oz) = m.read()
    row = math.floor(12 / 0.25) - oz
    assert int(cells["vertical"][row].sum()) == W * H and int(cells["vertical"].sum()) == W * H and int(cells["horizontal"].sum()) == 0
    hit = cells["vertical"][row] > 0
    # every column of the image spans all rows, so every hit cell has the whole wall's extent: Y = (y - 8) * 12 / 300, q = floor(Y / 0.05)
    qs = [math.floor((((yy - 8.0) * 12.0) / 300.0) / 0.05) for yy in range(H)]
    assert min(qs) == -7 and max(qs) == 31
    assert (cells["y_min"][row][hit] == -7).all() and (cells["y_max"][row][hit] == 31).all()
    # floor, not truncation, for negative world X: x = 74..79 -> X in [-0.24, -0.04] -> cell -1; x = 80..86 -> cell 0
    assert int(cells["vertical"][row, -1 - ox]) == 6 * H and int(cells["vertical"][row, 0 - ox]) == 7 * H
    assert hit.sum() == 13 + 13 and hit[-13 - ox] and hit[12 - ox] and not hit[-14 - ox] and not hit[13 - ox]   # X in [-3.2, 3.16]


def test_advancing_camera_keeps_absolute_cells_and_forgets_what_leaves():
    nx, nz = 32, 128
    m = M.Map(CAM, nx, nz)
    frames = [(wall(200), pose_at(tz=0.0)), (wall(300), pose_at(tz=4.0)), (wall(600), pose_at(tz=8.0))]   # Z = 12, 8, 4: the wall stays at world Z = 12
    total = {}
    for k, ((disp, planes), pose) in enumerate(frames):
        assert m.update(disp, planes, pose) == (-16, -64 + 16 * k)
        for key, c in scalar_votes(CAM, m.p, pose, disp, planes).items():
            t = total.setdefault(key, [0, 0, M.INT32_MAX, M.INT32_MIN])
            t[0], t[1], t[2], t[3] = t[0] + c[0], t[1] + c[1], min(t[2], c[2]), max(t[3], c[3])
    assert {gz for _, gz in total} == {48}
    cells, origin = m.read()
    assert origin == (-16, -32) and int(cells["vertical"][48 + 32].sum()) == 3 * W * H == int(cells["vertical"].sum())
    assert cells.tobytes() == windowed(total, origin, nx, nz).tobytes()
    # a step of 16 cells to the right: the columns [-16, 0) leave; stepping back brings them in empty, the columns [0, 16) are kept
    nothing = np.full((H, W), -32768, np.int16)
    assert m.update(nothing, planes, pose_at(tx=4.0, tz=8.0)) == (0, -32)
    assert m.update(nothing, planes, pose_at(tx=0.0, tz=8.0)) == (-16, -32)
    cells, origin = m.read()
    kept = {k: v for k, v in total.items() if k[0] >= 0}
    assert len(kept) < len(total) and cells.tobytes() == windowed(kept, origin, nx, nz).tobytes()
    assert int(cells["vertical"][:, :16].sum()) == 0 and int(cells["vertical"][:, 16:].sum()) > 0
    # a move of a whole window empties everything
    m.update(nothing, planes, pose_at(tx=0.0, tz=8.0 + 0.25 * nz))
    assert m.read()[0].tobytes() == M.empty_cells(nz, nx).tobytes()


def test_restatement_equals_the_scalar_loop_under_yaw_and_negative_translation():
    rng = np.random.default_rng(24)
    disp = rng.integers(100, 700, (H, W)).astype(np.int16)
    disp[rng.random((H, W)) < 0.1] = -32768
    planes = rng.integers(0, 3, (H, W)).astype(np.uint8)
    planes[0, :5] = 7
    for pose in (yaw_pose(90.0, (-3.3, 0.7, -12.9)), yaw_pose(-37.0, (5.1, -0.2, 2.6))):
        m = M.Map(CAM, 64, 48, M.params(cell_size=0.5, height_quantum=0.1))
        origin = m.update(disp, planes, pose)
        expect = scalar_votes(CAM, m.p, pose, disp, planes)
        cells = m.read()[0]
        assert int(cells["horizontal"].sum()) + int(cells["vertical"].sum()) > 500
        assert cells.tobytes() == windowed(expect, origin, 64, 48).tobytes()
    # yaw 90 degrees: camera Z becomes world X
    m = M.Map(CAM, 64, 64)
    d, p = wall(400)                    # Z = 6
    m.update(d, p, yaw_pose(90.0))
    cells, (ox, oz) = m.read()
    col = cells["vertical"][:, math.floor(6 / 0.25) - ox]
    assert int(col.sum()) == W * H == int(cells["vertical"].sum())


def test_classes_at_the_thresholds():
    c = M.empty_cells(1, 8)
    c["horizontal"] = [0, 2, 3, 1, 2, 51, 50, 2 ** 32 - 1]
    c["vertical"] = [0, 0, 0, 1, 1, 49, 50, 2 ** 32 - 1]
    assert M.classify(c, 3, 50).tolist() == [[2, 2, 0, 2, 0, 0, 1, 1]]       # n < 3 unknown; 49 % free; 50 % obstacle; no 32-bit wrap
    assert M.classify(c, 2, 34).tolist() == [[2, 0, 0, 1, 0, 1, 1, 1]]       # 1 of 3 = 33.3 % < 34 %
    assert M.classify(c, 2, 33).tolist() == [[2, 0, 0, 1, 1, 1, 1, 1]]
    assert M.classify(c, 1, 100).tolist() == [[2, 0, 0, 0, 0, 0, 0, 0]]


# ---- the built library, without a GPU ----------------------------------------------------------------------------------------

def _lib():
    from cartslam import _lib as L
    return L, L.load()


def _err(lib):
    return lib.cart_last_error(None).decode()


def test_symbols_layouts_and_defaults():
    L, lib = _lib()
    for name in ("default_params", "create", "destroy", "clear", "update", "window", "read", "classify"):
        assert hasattr(lib, "cart_plane_map_" + name) and "cart_plane_map_" + name in L.PROTOTYPES
    assert C.sizeof(L.PlaneMapParams) == 40 and C.sizeof(L.PlaneMapCell) == 16
    from cartslam import PLANE_MAP_CELL_DTYPE, plane_map_params
    assert PLANE_MAP_CELL_DTYPE == M.CELL_DTYPE and PLANE_MAP_CELL_DTYPE.itemsize == 16
    p = plane_map_params()
    assert {n: getattr(p, n) for n, _ in L.PlaneMapParams._fields_} == M.DEFAULTS
    assert plane_map_params(cell_size=0.5).cell_size == 0.5


def test_create_refuses_bad_cells_and_params_naming_them():
    L, lib = _lib()
    from cartslam import plane_map_params
    out = C.c_void_p()
    good = plane_map_params()
    for cx, cz, name in ((16, 64, "cells_x"), (40, 64, "cells_x"), (4112, 64, "cells_x"), (64, 0, "cells_z"), (64, 8192, "cells_z"), (64, 33, "cells_z")):
        assert lib.cart_plane_map_create(None, cx, cz, C.byref(good), C.byref(out)) != 0 and name in _err(lib), (cx, cz)
    bad = [("cell_size", 0.009), ("cell_size", math.nan), ("min_disparity", 0.0), ("min_disparity", math.inf), ("max_depth", -1.0),
           ("max_lateral", 0.0), ("max_lateral", math.nan), ("height_quantum", 0.0009), ("height_quantum", math.inf)]
    for field, value in bad:
        assert lib.cart_plane_map_create(None, 64, 64, C.byref(plane_map_params(**{field: value})), C.byref(out)) != 0 and field in _err(lib), (field, value)
    assert lib.cart_plane_map_create(None, 64, 64, None, C.byref(out)) != 0 and "params" in _err(lib)
    assert lib.cart_plane_map_create(None, 64, 64, C.byref(good), C.byref(out)) != 0 and not out.value   # everything valid but the engine


def test_update_refuses_a_bad_camera_or_pose_naming_it():
    L, lib = _lib()
    cam = L.EgoCamera(300.0, 300.0, 80.0, 8.0, 0.5)

    def update(camera, pose):
        arr = (C.c_double * 12)(*pose) if pose is not None else None
        return lib.cart_plane_map_update(None, C.byref(camera), arr, None, 0, None, 0, W, H, None)

    for k, value in ((0, 2.5), (5, math.nan), (10, -2.01), (3, 1.5e6), (7, -math.inf), (11, math.nan)):
        pose = list(M.POSE_IDENTITY)
        pose[k] = value
        assert update(cam, pose) != 0 and f"pose[{k}]" in _err(lib), k
    assert update(cam, None) != 0 and "pose" in _err(lib)
    assert update(L.EgoCamera(0.0, 300.0, 80.0, 8.0, 0.5), M.POSE_IDENTITY) != 0 and "fx" in _err(lib)
    assert update(L.EgoCamera(300.0, 300.0, 80.0, 8.0, -1.0), M.POSE_IDENTITY) != 0 and "baseline" in _err(lib)
    assert update(cam, M.POSE_IDENTITY) != 0 and "map" in _err(lib)      # a valid camera and pose get as far as the missing map
    assert lib.cart_plane_map_update(None, C.byref(cam), (C.c_double * 12)(*M.POSE_IDENTITY), None, 0, None, 0, 0, H, None) != 0 and "width" in _err(lib)

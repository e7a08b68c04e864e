"""GPU tests of the colour companion of the TSDF voxel map (spec S37): cart_voxel_color_integrate / _render / _vertices /
_read / _write against the numpy restatement tests/np_voxelcolor.py, byte for byte, on pitched buffers that start at a byte offset with
sentinel bytes around them, and the voxel_map host module with "color": true in the C++ frame loop.  Beside every byte comparison stands a
numeric premise on the restatement (voxels coloured per frame, voxels of weight >= 2 in a chain, pixels and vertices with a colour), so that
no comparison passes on an empty case.

The kernels as built: the integrate's workgroup owns 64 x 4 x 16 voxels (the volumes below have 1 to 3 of them along z and one with a partly
filled last one along x: 24), a lane walks 4 slices at a time; the render's wave owns an 8 x 8 pixel tile; a vertex has a lane."""
import ctypes as C

import numpy as np
import pytest

import np_voxelcolor as K
import np_voxelmap as V
import np_voxelmesh as M
import test_voxelmap_spec as S
from test_gpu_voxelmap import SENTINEL, SHAPES, SMALL, VOLUMES, WINDOW_CASES, _common, _torch, cam_for, counts_ptr, engine, frame_for, integrate, pitched, ptr_step, raycast

pytestmark = pytest.mark.gpu


def image_for(seed, w, h, channels):
    rng = np.random.default_rng(5000 + seed)
    return rng.integers(0, 256, (h, w, 3) if channels == 3 else (h, w), dtype=np.uint8)


class Rows:
    """h rows of `row` bytes, `row + extra` apart, the first `offset` bytes into a uint8 allocation that holds `fill` everywhere else."""

    def __init__(self, h, row, extra, offset, fill=SENTINEL, data=None, stream=None):
        torch = _torch()
        self.h, self.row, self.step, self.offset = h, row, row + extra, offset
        flat = np.full(offset + h * self.step + 5, fill, np.uint8)
        self.inside = np.zeros(len(flat), bool)
        for y in range(h):
            self.inside[offset + y * self.step: offset + y * self.step + row] = True
        if data is not None:
            flat[self.inside] = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            self.t = torch.from_numpy(flat).cuda()

    def arg(self):
        return C.c_void_p(self.t.data_ptr() + self.offset), self.step

    def split(self):
        """-> (the rows' bytes [h, row], every other byte of the allocation)"""
        flat = self.t.cpu().numpy()
        return flat[self.inside].reshape(self.h, self.row), flat[~self.inside]


def color_integrate_call(col, obj, cam, pose, disp, image, channels, mask=None, counts=None, size=None, stream=None):
    """cart_voxel_color_integrate on device tensors or (pointer, step) pairs as they are -> (rc, message)."""
    lib, c, P, sp = _common(cam, pose, stream)
    w, h = size if size is not None else (int(disp.shape[1]), int(disp.shape[0]))
    rc = lib.cart_voxel_color_integrate(col._h if col is not None else None, obj._h if obj is not None else None, c, P, *ptr_step(disp), *ptr_step(image), channels,
                                        w, h, *ptr_step(mask), counts_ptr(counts), sp)
    return rc, lib.cart_last_error(None).decode()


def color_integrate(col, obj, cam, pose, disp, image, mask=None, counts=True, stream=None):
    """One colour integrate on pitched, offset inputs whose slack would pass every gate and paint white; a three-channel image gets a step
    that is no multiple of 3.  -> the counts tensor (inside sentinel words) or None."""
    torch = _torch()
    channels = 3 if image.ndim == 3 else 1
    h, w = disp.shape
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d = pitched(disp, 3, 256, 1)
        m = pitched(mask, 5, 0, 3) if mask is not None else None
        n = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")[1:3] if counts else None
    im = Rows(h, channels * w, 4 if (channels * w + 4) % 3 else 5, 2, fill=255, data=image, stream=stream)
    assert channels == 1 or im.step % 3
    rc, err = color_integrate_call(col, obj, cam, pose, d, im.arg(), channels, m, n, stream=stream)
    assert rc == 0, err
    return n


def color_render_call(col, cam, pose, disp, size, image, alpha=(None, 0), counts=None, stream=None):
    lib, c, P, sp = _common(cam, pose, stream)
    rc = lib.cart_voxel_color_render(col._h if col is not None else None, c, P, *ptr_step(disp), size[0], size[1], *image, *alpha, counts_ptr(counts), sp)
    return rc, lib.cart_last_error(None).decode()


def color_render(col, cam, pose, disp, alpha=True, counts=True, stream=None):
    """disp = a device tensor (a raycast's pitched output) or a host array -> dict(image Rows, alpha Rows or None, counts tensor or None)."""
    torch = _torch()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d = disp if isinstance(disp, torch.Tensor) else pitched(np.ascontiguousarray(disp), 3, 256, 1)
        n = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")[1:2] if counts else None
    h, w = int(d.shape[0]), int(d.shape[1])
    outs = dict(image=Rows(h, 3 * w, 4 if (3 * w + 4) % 3 else 5, 1, stream=stream), alpha=Rows(h, w, 6, 5, stream=stream) if alpha else None, counts=n, disp=d)
    rc, err = color_render_call(col, cam, pose, d, (w, h), outs["image"].arg(), outs["alpha"].arg() if alpha else (None, 0), n, stream=stream)
    assert rc == 0, err
    return outs


def same_render(outs, ref):
    _torch().cuda.synchronize()
    h, w = ref["alpha"].shape
    got, slack = outs["image"].split()
    assert got.reshape(h, w, 3).tobytes() == ref["image"].tobytes(), f"image: {int((got.reshape(h, w, 3) != ref['image']).sum())} bytes differ"
    assert (slack == SENTINEL).all(), "image: bytes outside the rows were written"
    if outs["alpha"] is not None:
        got, slack = outs["alpha"].split()
        assert got.tobytes() == ref["alpha"].tobytes(), f"alpha: {int((got != ref['alpha']).sum())} bytes differ"
        assert (slack == SENTINEL).all(), "alpha: bytes outside the rows were written"
    if outs["counts"] is not None:
        words = outs["counts"]._base.cpu().numpy()
        assert words[1] == ref["counts"][0] and (words[[0, 2, 3]] == SENTINEL).all(), (words, ref["counts"])


def same_counts(n, ref):
    _torch().cuda.synchronize()
    words = n._base.cpu().numpy()
    assert words[1:3].tobytes() == ref.tobytes(), (words, ref)
    assert (words[[0, 3]] == SENTINEL).all()


def same_colors(col, ref):
    vox, origin = col.read()
    rv, ro = ref.read()
    assert tuple(origin) == tuple(ro), (origin, ro)
    assert vox.dtype == rv.dtype and vox.shape == rv.shape
    assert vox.tobytes() == rv.tobytes(), f"{int((vox != rv).sum())} colour voxels differ"
    assert col.window() == (tuple(ro), (ref.nx, ref.ny, ref.nz), ref.origin is not None)


def vertices_call(col, vertices, n, max_vertices, origin, colors, stream=None):
    """cart_voxel_color_vertices; vertices / n / colors = tensors or pointers (None = NULL) -> (rc, message)."""
    from cartslam import _lib
    torch = _torch()
    lib = _lib.load()
    p = [C.c_void_p(t.data_ptr()) if isinstance(t, torch.Tensor) else t for t in (vertices, n, colors)]
    o = (C.c_int64 * 3)(*origin) if origin is not None else None
    sp = C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)
    rc = lib.cart_voxel_color_vertices(col._h if col is not None else None, p[0], p[1], max_vertices, o, p[2], sp)
    return rc, lib.cart_last_error(None).decode()


def color_vertices(col, vertices, n, max_vertices, origin, stream=None):
    """-> int32 words [max_vertices + 2] filled with the sentinel, the records one word into the allocation."""
    torch = _torch()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        out = torch.full((max_vertices + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    rc, err = vertices_call(col, vertices, n, max_vertices, origin, C.c_void_p(out.data_ptr() + 4), stream)
    assert rc == 0, err
    return out


def same_vertex_colors(out, ref):
    _torch().cuda.synchronize()
    words = out.cpu().numpy()
    k = len(ref)
    assert words[1:1 + k].tobytes() == ref.tobytes(), f"{int((words[1:1 + k] != ref.view(np.int32)).sum())} vertex colours differ"
    assert words[0] == SENTINEL and (words[1 + k:] == SENTINEL).all(), "words outside the coloured vertices were touched"


def check_mesh_colours(obj, col, ref, cref, least=1):
    """The extracted mesh of the device map, coloured on the same stream with the count read from the mesh's own device counts; against the
    restatement's mesh and colours.  -> vertices with a colour."""
    full = M.extract(ref.tsdf, ref.weight, 1, ref.p["voxel_size"])
    nv = len(full["vertices"])
    cap = nv + 3
    vt, _, n, o = obj.mesh(cap, len(full["quads"]) + 3, min_weight=1, raw=True)
    assert o == (ref.origin or (0, 0, 0))
    exp = cref.colorize(full["vertices"], o)
    same_vertex_colors(color_vertices(col, vt, n[2:3], cap, o), exp)
    assert int(n.cpu()[2]) == nv and (exp["weight"] > 0).sum() >= least, (nv, int((exp["weight"] > 0).sum()))
    return int((exp["weight"] > 0).sum())


def run_chain(shape, p, cam, frames, max_weight=K.DEFAULT_MAX_WEIGHT, mesh_least=1):
    """frames = [(pose, disp, mask, image)] or [(pose, disp, mask, image, camera)] for a frame with a camera of its own.  The device objects
    and the restatement integrate every frame, geometry first; the colour volume, the counts, a render behind the model raycast from the
    frame's pose and the colours of the extracted mesh are compared after each.  Every frame colours at least 30 voxels, and at some frame
    of the chain at least 10 voxels have weight >= 2 (where max_weight allows it).  -> [(counts, voxels of weight >= 2, render, coloured
    vertices)] of the restatement."""
    from cartslam import VoxelColor, VoxelMap, voxel_map_params
    ref = V.Map(*shape, V.params(**p))
    cref = K.Color(ref, max_weight)
    out = []
    with VoxelMap(engine(), *shape, voxel_map_params(**p)) as obj, VoxelColor(engine(), obj, max_weight) as col:
        for frame in frames:
            pose, disp, mask, image = frame[:4]
            fcam = frame[4] if len(frame) > 4 else cam
            integrate(obj, fcam, pose, disp, mask, counts=False)
            ref.integrate(fcam, pose, disp, mask)
            n = color_integrate(col, obj, fcam, pose, disp, image, mask)
            rn = cref.integrate(fcam, pose, disp, image, mask)
            same_counts(n, rn)
            same_colors(col, cref)
            assert rn[0] >= 30, rn
            h, w = disp.shape
            ray = raycast(obj, fcam, pose, w, h, weight=False, status=False, counts=False)      # the model disparity stays on the device
            rr = cref.render(fcam, pose, ref.raycast(fcam, pose, w, h)["disp"])
            same_render(color_render(col, fcam, pose, ray["disp"]), rr)
            out.append((rn, int((cref.weight >= 2).sum()), rr, check_mesh_colours(obj, col, ref, cref, mesh_least)))
    assert max_weight < 2 or max(o[1] for o in out) >= 10, [o[1] for o in out]
    return out


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", VOLUMES)
def test_volumes_gray_and_bgr_with_and_without_the_mask(shape, channels, masked):
    w, h = 63, 24
    cam = cam_for(w, h)
    frames = [(S.pose_t(), *frame_for(7 + k + shape[0], w, h, cam, masked=masked), image_for(k + shape[0], w, h, channels)) for k in range(2)]
    res = run_chain(shape, dict(SMALL, lookahead=0.125 * shape[2] / 2), cam, frames)
    assert res[-1][2]["counts"][0] > 0 and res[-1][3] > 0                     # pixels and vertices with a colour


@pytest.mark.parametrize("w,h", SHAPES)
def test_image_shapes_on_pitched_offset_buffers(w, h):
    """As test_gpu_voxelmap's test of the shapes: two frames of 130 x 70 come first (gray, then B, G, R), the frame of the shape under test is
    integrated into their volume (B, G, R: 3 w + 4 or 5 bytes a row, no multiple of 3) and rendered from it."""
    cam, wide = cam_for(w, h), cam_for(130, 70)
    frames = [(S.pose_t(0.0625, 0.0625, 0.0), *frame_for(900 + k, 130, 70, wide, masked=False), image_for(900 + k, 130, 70, 1 + 2 * k), wide) for k in range(2)]
    frames.append((S.pose_t(0.0625, 0.0625, 0.0625), *frame_for(10 * w + h, w, h, cam, masked=w * h >= 64), image_for(10 * w + h, w, h, 3)))
    res = run_chain((16, 16, 16), SMALL, cam, frames)
    assert res[-1][2]["counts"][0] > 0, res[-1][2]["counts"]


@pytest.mark.parametrize("name", ["forward", "jump", "lateral_and_vertical", "turned_180"])
def test_window_cases(name):
    """Negative origins, storage wrap, slabs that enter on every axis and jumps that empty everything.  Every pose of the case gives two
    frames (a wall 1.5 m ahead moves with the camera, so one frame a pose would colour no voxel twice): gray then B, G, R.  After the first
    frame at a new origin a voxel of weight >= 2 is one that stayed and kept its colour."""
    poses, lookahead, depth, origins_ok = WINDOW_CASES[name]
    w, h = 40, 24
    cam = cam_for(w, h)
    p = dict(SMALL, lookahead=lookahead, max_depth=max(3.0, depth + 1.0))
    frames = [(pose, *frame_for(3 * len(name) + 2 * k + rep, w, h, cam, depth=depth, masked=k % 2 == 0), image_for(2 * k + rep, w, h, 1 + 2 * rep))
              for k, pose in enumerate(poses) for rep in range(2)]
    ref = V.Map(16, 16, 16, V.params(**p))
    cref = K.Color(ref)
    origins, kept = [], []
    for pose, disp, mask, image in frames:
        ref.integrate(cam, pose, disp, mask)
        cref.integrate(cam, pose, disp, image, mask)
        origins.append(cref.origin)
        kept.append(len(origins) > 1 and origins[-1] != origins[-2] and int((cref.weight >= 2).sum()) > 0)
    assert origins_ok(origins[::2]), origins
    assert name == "jump" or any(kept), kept                                  # a move after which voxels that stayed still had their colour
    run_chain((16, 16, 16), p, cam, frames, mesh_least=0)


@pytest.mark.parametrize("max_weight,top", [(1, 1), (2, 2)])
def test_weight_cap(max_weight, top):
    w, h = 40, 24
    cam = cam_for(w, h)
    frames = [(S.pose_t(), *frame_for(50 + k, w, h, cam, masked=False), image_for(50 + k, w, h, 3)) for k in range(4)]
    res = run_chain((16, 16, 16), SMALL, cam, frames, max_weight=max_weight)
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    cref = K.Color(ref, max_weight)
    seen = []
    for pose, disp, mask, image in frames:
        ref.integrate(cam, pose, disp, mask)
        cref.integrate(cam, pose, disp, image, mask)
        seen.append(cref.read()[0].copy())
    assert seen[-1]["weight"].max() == top and (seen[-1]["b"] != seen[-2]["b"]).sum() > 10    # capped, and still averaging
    assert res[-1][0][1] < res[-1][0][0]                                      # the last frame met voxels that had a colour


def test_map_clear_rebuild_and_write_then_a_colour_integrate():
    """The colour volume follows whatever origin the map has at the next colour integrate, by the move rule; a map without a window refuses."""
    from cartslam import PlaneStore, VoxelColor, VoxelMap, voxel_map_params
    w, h = 63, 24
    cam = cam_for(w, h)
    frame = lambda k: (*frame_for(80 + k, w, h, cam, masked=False), image_for(80 + k, w, h, 3))   # noqa: E731
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    cref = K.Color(ref)
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as obj, VoxelColor(engine(), obj) as col, PlaneStore(engine(), w, h, 2) as store:
        def both(k, pose, geometry=True):
            disp, mask, image = frame(k)
            if geometry:
                integrate(obj, cam, pose, disp, mask, counts=False)
                ref.integrate(cam, pose, disp, mask)
            same_counts(color_integrate(col, obj, cam, pose, disp, image, mask), cref.integrate(cam, pose, disp, image, mask))
            same_colors(col, cref)

        both(0, S.pose_t())
        both(1, S.pose_t())
        assert (cref.weight >= 2).sum() >= 10
        # clear: the map has no window, the colour integrate is refused and changes nothing; the map's next window lies 8 voxels on
        obj.clear()
        disp, mask, image = frame(2)
        n = _torch().full((4,), SENTINEL, dtype=_torch().int32, device="cuda")
        im = Rows(h, 3 * w, 4, 0, data=image)
        rc, err = color_integrate_call(col, obj, cam, S.pose_t(), pitched(disp, 3, 256, 1), im.arg(), 3, None, n[1:3])
        assert rc != 0 and err == "the map has no window"
        _torch().cuda.synchronize()
        assert bool((n == SENTINEL).all())
        same_colors(col, cref)
        ref.clear()
        both(2, S.pose_t(tz=1.0))
        assert cref.origin[2] == 8 and (cref.weight >= 2).sum() >= 10          # what stayed kept its colour and was coloured again
        # rebuild: a fresh window one slab back, from the store's frame; nothing of the colours is rebuilt, the overlap stays
        disp, mask, image = frame(3)
        store.insert(5, disp, np.zeros((h, w), np.uint8))
        origin, used, _ = obj.rebuild(store, [5], [S.pose_t()], S.pose_t(), cam_tuple_of(cam))
        assert used == 1 and origin == V.window_origin(S.pose_t(), ref.p, (16, 16, 16)) and origin[2] == 0
        ref.origin = origin                                                   # the colour restatement reads nothing else of the map
        kept = int((cref.weight > 0).sum())
        both(3, S.pose_t(), geometry=False)
        assert cref.origin == origin and 0 < kept
        # write: the map's window jumps by more than N; every colour is emptied
        vox, _ = obj.read()
        far = (origin[0] + 32, origin[1], origin[2] - 16)
        obj.write(vox, far)
        ref.origin = far
        both(4, S.pose_t(tx=4.0, tz=-2.0), geometry=False)
        assert cref.origin == far and cref.weight.max() == 1 and (cref.weight > 0).sum() >= 30


def cam_tuple_of(cam):
    return tuple(cam[k] for k in ("fx", "fy", "cx", "cy", "baseline"))


def random_colours(seed, shape, empty=0.3):
    """-> VOXEL_RGB_DTYPE [nz, ny, nx]: random bytes, weights over the whole range, a share of empty words."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    vox = np.frombuffer(rng.integers(0, 256, 4 * nx * ny * nz, dtype=np.uint8).tobytes(), K.VOXEL_RGB_DTYPE).reshape(nz, ny, nx).copy()
    vox.view(np.uint32)[rng.random((nz, ny, nx)) < empty] = 0
    return vox


def probe_vertices(seed, shape, voxel_size, n=600):
    """Vertex records all over the window and up to two voxels beyond every face, some exactly on voxel-centre planes and on the window's
    faces, two with a NaN and an infinity.  -> MESH_VERTEX_DTYPE [n]"""
    rng = np.random.default_rng(seed)
    v = np.zeros(n, M.MESH_VERTEX_DTYPE)
    for a in range(3):
        v["position"][:, a] = (rng.random(n) * (shape[a] + 4) - 2).astype(np.float32) * np.float32(voxel_size)
    on = rng.random(n) < 0.3                                                  # (k + 0.5) voxel_size: a = k exactly, at the first and the last corner too
    for a in range(3):
        k = rng.integers(-1, shape[a] + 1, n).astype(np.float64)
        v["position"][:, a] = np.where(on, ((k + 0.5) * voxel_size).astype(np.float32), v["position"][:, a])
    v["position"][0] = (np.nan, 0.5, 0.5)
    v["position"][1] = (0.5, np.inf, 0.5)
    v["position"][2] = (0.0625, 0.0625, 0.0625)                               # the window's first corner: a = 0
    v["position"][3] = [(s - 1.5) * voxel_size for s in shape]                # the last i0 with both corners inside
    v["position"][4] = [(s - 0.5) * voxel_size for s in shape]                # one beyond it
    return v


@pytest.mark.parametrize("shape", VOLUMES)
def test_written_volumes_render_and_colorize(shape):
    """Random colour volumes through cart_voxel_color_write at toroidal origins: write then read gives the bytes back; a render behind a
    synthetic disparity whose points cover the window and its surroundings; vertices in, on and beyond the window's faces, with the mesh
    origin another than the window's, and a count below and above the capacity."""
    from cartslam import VoxelColor, VoxelMap
    torch = _torch()
    w, h = 63, 24
    cam = cam_for(w, h)
    origin = (-8, 40, -56)
    with VoxelMap(engine(), *shape) as obj, VoxelColor(engine(), obj, 7) as col:
        cref = K.Color(V.Map(*shape), 7)
        for seed, o in ((1, origin), (2, (0, 0, 0))):
            vox = random_colours(seed + shape[0], shape)
            col.write(vox, o)
            cref.write(vox, o)
            same_colors(col, cref)
            # a camera in the middle of the window looking along z, then along -x
            centre = [(o[a] + shape[a] / 2) * 0.125 for a in range(3)]
            for pose in (S.pose_t(centre[0], centre[1], centre[2] - 0.5), [0.0, 0.0, -1.0, centre[0] + 0.4, 0.0, 1.0, 0.0, centre[1], 1.0, 0.0, 0.0, centre[2]]):
                rng = np.random.default_rng(seed)
                disp = rng.integers(-3, 2000, (h, w)).astype(np.int16)        # 0 and negative values, and depths from 0.25 m to far outside
                disp[rng.random((h, w)) < 0.1] = V.INVALID
                rr = cref.render(cam, pose, disp)
                assert rr["counts"][0] > 100 and (rr["alpha"] == 0).sum() > 100, rr["counts"]
                same_render(color_render(col, cam, pose, disp), rr)
                same_render(color_render(col, cam, pose, disp, alpha=False, counts=False), rr)
            v = probe_vertices(seed, shape, 0.125)
            vt = torch.from_numpy(v.view(np.float32).reshape(-1, 6).copy()).cuda()
            for mesh_origin, count, cap in ((o, len(v), len(v)), ((o[0] + 8, o[1], o[2] - 8), len(v), len(v)), (o, 100, len(v)), (o, len(v) + 50, 250), (o, 0, 16), (o, -3, 16)):
                nt = torch.tensor([SENTINEL, count, SENTINEL], dtype=torch.int32).cuda()
                exp = cref.colorize(v, mesh_origin, n=count, max_vertices=cap)
                assert len(exp) == max(0, min(count, cap)) and (count < 100 or (count // 20 < (exp["weight"] > 0).sum() < len(exp) - count // 20))
                same_vertex_colors(color_vertices(col, vt, nt[1:2], cap, mesh_origin), exp)
        same_colors(col, cref)                                                # the read-outs changed nothing


def test_no_window_gives_zeros():
    from cartslam import VoxelColor, VoxelMap
    torch = _torch()
    w, h = 40, 24
    cam = cam_for(w, h)
    disp, _ = frame_for(4, w, h, cam, masked=False)
    v = probe_vertices(3, (16, 16, 16), 0.125, n=70)
    vt = torch.from_numpy(v.view(np.float32).reshape(-1, 6).copy()).cuda()
    nt = torch.tensor([70], dtype=torch.int32).cuda()
    with VoxelMap(engine(), 16, 16, 16) as obj, VoxelColor(engine(), obj) as col:
        cref = K.Color(V.Map(16, 16, 16))
        for _ in range(2):
            same_colors(col, cref)                                            # every voxel empty, origin (0, 0, 0), not valid
            rr = cref.render(cam, S.pose_t(), disp)
            assert rr["counts"][0] == 0 and not rr["image"].any()
            same_render(color_render(col, cam, S.pose_t(), disp), rr)
            same_vertex_colors(color_vertices(col, vt, nt, 70, (0, 0, 0)), np.zeros(70, K.VOXEL_RGB_DTYPE))
            vox = random_colours(9, (16, 16, 16), empty=0.0)
            col.write(vox, (0, 0, 0))
            assert col.render(cam_tuple_of(cam), S.pose_t(tx=1.0, ty=1.0), disp)[2][0] > 0
            col.clear()                                                       # and again after clear


def test_queued_calls_on_one_stream_and_on_two():
    """Integrates, renders and vertex colourings queued without a synchronisation, on the current stream and on a second one: only the
    object's own ordering keeps a read-out from seeing the next frame's colours."""
    from cartslam import VoxelColor, VoxelMap, voxel_map_params
    torch = _torch()
    w, h = 63, 24
    cam = cam_for(w, h)
    frames = [(S.pose_t(tz=0.125 * k), *frame_for(40 + k, w, h, cam, masked=False), image_for(40 + k, w, h, 3)) for k in range(4)]
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    cref = K.Color(ref)
    v = probe_vertices(5, (16, 16, 16), 0.125, n=2000)                        # the coloured band is thin: about 3 % of them get a colour
    side = torch.cuda.Stream()
    queued = []
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as obj, VoxelColor(engine(), obj) as col:
        vt = torch.from_numpy(v.view(np.float32).reshape(-1, 6).copy()).cuda()
        nt = torch.tensor([2000], dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        for k, (pose, disp, mask, image) in enumerate(frames):
            stream = side if k % 2 else None
            integrate(obj, cam, pose, disp, mask, counts=False)
            ref.integrate(cam, pose, disp, mask)
            n = color_integrate(col, obj, cam, pose, disp, image, mask, stream=stream)
            rn = cref.integrate(cam, pose, disp, image, mask)
            model = ref.raycast(cam, pose, w, h)["disp"]
            other = None if k % 2 else side                                   # the read-outs on the other stream than the integrate
            queued.append((n, rn, color_render(col, cam, pose, model, stream=other), cref.render(cam, pose, model),
                           color_vertices(col, vt, nt, 2000, cref.origin, stream=stream), cref.colorize(v, cref.origin)))
        torch.cuda.synchronize()
        for n, rn, outs, rr, colours, exp in queued:
            same_counts(n, rn)
            same_render(outs, rr)
            same_vertex_colors(colours, exp)
        same_colors(col, cref)
    assert queued[-1][3]["counts"][0] > 50 and (queued[-1][5]["weight"] > 0).sum() > 10 and (cref.weight >= 2).sum() >= 10
    assert queued[1][3]["image"].tobytes() != queued[2][3]["image"].tobytes()


def test_the_python_class(tmp_path):
    from cartslam import VOXEL_RGB_DTYPE, EngineError, VoxelColor, VoxelMap, voxel_map_params, write_ply
    torch = _torch()
    w, h = 63, 24
    cam = cam_for(w, h)
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    cref = K.Color(ref, 5)
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as obj, VoxelColor(engine(), obj, max_weight=5) as col:
        assert col.window() == ((0, 0, 0), (16, 16, 16), False) and col.max_weight == 5
        with pytest.raises(EngineError, match="no window"):
            col.integrate(cam_tuple_of(cam), S.pose_t(), *frame_for(8, w, h, cam, masked=False)[:1], image_for(8, w, h, 1))
        for k, channels in enumerate((1, 3, 3)):
            disp, mask = frame_for(8 + k, w, h, cam)
            image = image_for(8 + k, w, h, channels)
            obj.integrate(cam_tuple_of(cam), S.pose_t(), disp, mask, counts=False)
            ref.integrate(cam, S.pose_t(), disp, mask)
            rn = cref.integrate(cam, S.pose_t(), disp, image, mask)
            if k < 2:                                                         # host arrays in, host arrays out
                n = col.integrate(cam_tuple_of(cam), S.pose_t(), disp, image, mask)
                assert n.dtype == np.int32 and n.tobytes() == rn.tobytes()
            else:                                                             # device tensors, a stream of its own, raw
                n = col.integrate(cam_tuple_of(cam), S.pose_t(), torch.from_numpy(disp).cuda(), torch.from_numpy(image).cuda(), torch.from_numpy(mask).cuda(),
                                  raw=True, stream=torch.cuda.Stream())
                assert isinstance(n, torch.Tensor) and n.is_cuda
                torch.cuda.synchronize()
                assert n.cpu().numpy().tobytes() == rn.tobytes()
        vox, origin = col.read()
        assert vox.dtype == VOXEL_RGB_DTYPE and vox.tobytes() == cref.read()[0].tobytes() and origin == cref.origin and (vox["weight"] >= 2).sum() >= 10
        dm = obj.raycast(cam_tuple_of(cam), S.pose_t(), w, h)[0]
        rr = cref.render(cam, S.pose_t(), dm)
        image, alpha, n = col.render(cam_tuple_of(cam), S.pose_t(), dm)
        assert image.tobytes() == rr["image"].tobytes() and alpha.tobytes() == rr["alpha"].tobytes() and n.tobytes() == rr["counts"].tobytes() and n[0] > 50
        image, alpha, n = col.render(cam_tuple_of(cam), S.pose_t(), torch.from_numpy(dm).cuda(), alpha=False, counts=False, stream=torch.cuda.Stream())
        assert image.tobytes() == rr["image"].tobytes() and alpha is None and n is None
        vertices, quads, counts, o = obj.mesh(4000, 4000)
        exp = cref.colorize(vertices, o)
        colours = col.colorize(vertices, None, o)
        assert colours.dtype == VOXEL_RGB_DTYPE and colours.tobytes() == exp.tobytes() and (exp["weight"] > 0).sum() > 10
        vt, qt, nt, o = obj.mesh(4000, 4000, raw=True)
        assert col.colorize(vt, nt, o, stream=torch.cuda.Stream()).tobytes() == exp.tobytes()
        raw = col.colorize(vt, nt, o, raw=True)
        assert raw.is_cuda and tuple(raw.shape) == (4000, 4) and raw[:len(exp)].cpu().numpy().tobytes() == exp.tobytes()
        path = str(tmp_path / "mesh.ply")
        write_ply(path, vertices, quads, o, 0.125, colors=colours)
        assert open(path, "rb").read().endswith(np.frombuffer(quads.tobytes(), "<i4").reshape(-1, 4)[-1].tobytes()) and b"property uchar alpha" in open(path, "rb").read()
        col.write(vox, (8, 8, 8))
        assert col.window()[0] == (8, 8, 8) and col.read()[0].tobytes() == vox.tobytes()
        with pytest.raises(EngineError, match="cells_z"):
            col.write(vox[:8], (0, 0, 0))
        with pytest.raises(EngineError, match="origin3\\[1\\]"):
            col.write(vox, (0, 12, 0))
        with pytest.raises(EngineError, match="image"):
            col.integrate(cam_tuple_of(cam), S.pose_t(), disp, image[:5], mask)
        assert col.window()[0] == (8, 8, 8)                                   # the refused calls changed nothing
        col.clear()
        assert col.window() == ((0, 0, 0), (16, 16, 16), False) and not col.read()[0].view(np.uint32).any()
        with pytest.raises(EngineError, match="max_weight"):
            VoxelColor(engine(), obj, 256)
        with VoxelMap(engine(), 24, 16, 16, voxel_map_params(**SMALL)) as wide:
            wide.integrate(cam_tuple_of(cam), S.pose_t(), disp, mask, counts=False)
            col._map = wide
            with pytest.raises(EngineError, match="shape"):
                col.integrate(cam_tuple_of(cam), S.pose_t(), disp, image, mask)
            col._map = obj


def test_bad_arguments_touch_no_output():
    from cartslam import VoxelColor, VoxelMap, _lib, voxel_map_params
    torch = _torch()
    lib = _lib.load()
    w, h = 63, 24
    cam = cam_for(w, h)
    disp, mask = frame_for(8, w, h, cam)
    image = image_for(8, w, h, 3)
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    cref = K.Color(ref)
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as obj, VoxelColor(engine(), obj) as col:
        integrate(obj, cam, S.pose_t(), disp, mask, counts=False)
        ref.integrate(cam, S.pose_t(), disp, mask)
        color_integrate(col, obj, cam, S.pose_t(), disp, image, mask)
        cref.integrate(cam, S.pose_t(), disp, image, mask)
        d, m = pitched(disp, 3, 256, 1), pitched(mask, 5, 0, 3)
        im = Rows(h, 3 * w, 4, 0, data=image)
        n = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
        good = dict(col_=col, obj_=obj, cam_=cam, pose=S.pose_t(), disp=d, image=im.arg(), channels=3, mask=m, counts=n[1:3], size=None)

        def refused(word, **kw):
            a = dict(good, **kw)
            rc, err = color_integrate_call(a["col_"], a["obj_"], a["cam_"], a["pose"], a["disp"], a["image"], a["channels"], a["mask"], a["counts"], a["size"])
            assert rc != 0 and word in err, (kw, err)

        dp, ip = d.data_ptr(), im.arg()[0].value
        refused("channels", channels=2, col_=None, obj_=None)
        refused("fx", cam_=dict(cam, fx=0.0))
        refused("pose[3]", pose=[float("nan") if k == 3 else v for k, v in enumerate(S.pose_t())])
        refused("width", size=(0, h))
        refused("color is NULL", col_=None)
        refused("map is NULL", obj_=None)
        refused("disp is NULL", disp=(None, 0), size=(w, h))
        refused("image is NULL", image=(None, 0))
        refused("disp and its step must be 2-byte aligned", disp=(C.c_void_p(dp + 1), 2 * (w + 3)), size=(w, h))
        refused("disp_step is below the row size", disp=(C.c_void_p(dp), 2 * w - 2), size=(w, h))
        refused("image_step is below the row size", image=(C.c_void_p(ip), 3 * w - 1))
        refused("mask_step is below the row size", mask=(C.c_void_p(m.data_ptr()), w - 1))
        refused("counts must be 4-byte aligned", counts=C.c_void_p(n.data_ptr() + 2))
        refused("disp and counts must not overlap", counts=C.c_void_p((dp + 3) // 4 * 4))
        refused("image and counts must not overlap", counts=C.c_void_p(ip + 4))
        refused("mask and counts must not overlap", counts=C.c_void_p((m.data_ptr() + 3) // 4 * 4))
        # render
        image_out, alpha_out = Rows(h, 3 * w, 4, 1), Rows(h, w, 6, 5)
        rgood = dict(col_=col, cam_=cam, pose=S.pose_t(), disp=d, size=(w, h), image=image_out.arg(), alpha=alpha_out.arg(), counts=n[1:2])

        def render_refused(word, **kw):
            a = dict(rgood, **kw)
            rc, err = color_render_call(a["col_"], a["cam_"], a["pose"], a["disp"], a["size"], a["image"], a["alpha"], a["counts"])
            assert rc != 0 and word in err, (kw, err)

        op, ap = image_out.arg()[0].value, alpha_out.arg()[0].value
        render_refused("baseline", cam_=dict(cam, baseline=-1.0))
        render_refused("pose is NULL", pose=None)
        render_refused("height", size=(w, 0))
        render_refused("color is NULL", col_=None)
        render_refused("disp is NULL", disp=(None, 0))
        render_refused("image_bgr is NULL", image=(None, 0))
        render_refused("image_bgr_step is below the row size", image=(C.c_void_p(op), 3 * w - 1))
        render_refused("alpha_step is below the row size", alpha=(C.c_void_p(ap), w - 1))
        render_refused("counts must be 4-byte aligned", counts=C.c_void_p(n.data_ptr() + 1))
        render_refused("disp and image_bgr must not overlap", image=(C.c_void_p(dp + 2), 3 * w + 4))
        render_refused("disp and alpha must not overlap", alpha=(C.c_void_p(dp + 2 * (w + 3) * h - 10), w))
        render_refused("image_bgr and alpha must not overlap", alpha=(C.c_void_p(op + 7), w + 6))
        render_refused("image_bgr and counts must not overlap", counts=C.c_void_p((op + 3) // 4 * 4))
        render_refused("alpha and counts must not overlap", counts=C.c_void_p((ap + 3) // 4 * 4))
        # vertices
        v = probe_vertices(5, (16, 16, 16), 0.125, n=64)
        vt = torch.from_numpy(v.view(np.float32).reshape(-1, 6).copy()).cuda()
        nt = torch.tensor([64], dtype=torch.int32).cuda()
        colours = torch.full((66,), SENTINEL, dtype=torch.int32, device="cuda")
        vgood = dict(col_=col, vertices=vt, n=nt, max_vertices=64, origin=(0, 0, 0), colors=C.c_void_p(colours.data_ptr() + 4))

        def vertices_refused(word, **kw):
            a = dict(vgood, **kw)
            rc, err = vertices_call(a["col_"], a["vertices"], a["n"], a["max_vertices"], a["origin"], a["colors"])
            assert rc != 0 and word in err, (kw, err)

        vertices_refused("max_vertices", max_vertices=0)
        vertices_refused("max_vertices", max_vertices=(1 << 26) + 1)
        vertices_refused("origin3 is NULL", origin=None)
        vertices_refused("origin3[2]", origin=(0, 0, -(1 << 27) - 1))
        vertices_refused("color is NULL", col_=None)
        vertices_refused("vertices is NULL", vertices=None)
        vertices_refused("n_vertices is NULL", n=None)
        vertices_refused("colors is NULL", colors=None)
        vertices_refused("vertices must be 4-byte aligned", vertices=C.c_void_p(vt.data_ptr() + 2))
        vertices_refused("n_vertices must be 4-byte aligned", n=C.c_void_p(nt.data_ptr() + 1))
        vertices_refused("colors must be 4-byte aligned", colors=C.c_void_p(colours.data_ptr() + 3))
        vertices_refused("vertices and colors must not overlap", colors=C.c_void_p(vt.data_ptr() + 24 * 64 - 4))
        vertices_refused("n_vertices and colors must not overlap", colors=C.c_void_p(nt.data_ptr()))
        # the host entry points
        o = (C.c_int64 * 3)(0, 0, 0)
        assert lib.cart_voxel_color_write(col._h, None, o, None) != 0 and lib.cart_last_error(None).decode() == "host_voxels is NULL"
        assert lib.cart_voxel_color_read(col._h, None, o, None) != 0 and lib.cart_last_error(None).decode() == "host_voxels is NULL"
        assert lib.cart_voxel_color_window(col._h, o, None, None) != 0 and lib.cart_last_error(None).decode() == "shape3 is NULL"
        out = C.c_void_p()
        assert lib.cart_voxel_color_create(engine()._h, None, 64, C.byref(out)) != 0 and lib.cart_last_error(None).decode() == "map is NULL" and not out.value
        torch.cuda.synchronize()
        assert bool((n == SENTINEL).all()) and bool((colours == SENTINEL).all())
        for rows in (image_out, alpha_out):
            body, slack = rows.split()
            assert (body == SENTINEL).all() and (slack == SENTINEL).all()      # no refused call touched an output
        same_colors(col, cref)                                                # nor the volume or its window
        assert cref.weight.sum() >= 30


# ---- the C++ frame loop ------------------------------------------------------------------------------------------------------------
def read_colour_dump(path, w, h):
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, "<i4", 6)
    assert head[4:].tolist() == [w, h] and len(raw) == 24 + 4 * w * h, path
    return dict(integrated=int(head[0]), counts=head[1:3], rendered=int(head[3]), image=np.frombuffer(raw, np.uint8, 3 * w * h, 24).reshape(h, w, 3),
                alpha=np.frombuffer(raw, np.uint8, w * h, 24 + 3 * w * h).reshape(h, w))


def test_voxel_map_module_with_colour(tmp_path):
    """cart_slam_amd over four synthetic frames (the scene and the head of test_gpu_voxelmesh's module test) with "color": true, the raycast
    and "mesh_interval": 2.  The restatement is fed what the run itself dumped for every frame (the disparity, ego_motion's pose, the map's
    window) and the left image: the colour counts, the colour voxels (through the snapshot switch), image_model and its alpha behind the
    dumped model disparity, and the colours of the dumped mesh's vertices are its, byte for byte.  With "color": false the module dumps
    what it dumped before, byte for byte."""
    import json
    import os
    from test_gpu_matches import noise_frame, noise_world
    from test_gpu_voxelmap import read_dump
    from test_gpu_voxelmesh import read_mesh_dump
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
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    vp = dict(voxel_size=0.5, min_disparity=3.5, max_depth=40.0, truncation=1.0, march_step=0.5, lookahead=16.0, max_weight=3)
    shape = dict(cells_x=64, cells_y=16, cells_z=64)
    head = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
            {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion")]
    module = dict(keys, type="voxel_map", mesh=True, mesh_interval=2, **shape, **vp)

    def run(name, **extra):
        d = os.path.join(tmp, name)
        os.makedirs(d)
        r = run_exe(src, head + [dict(module, **extra)], tmp, ("--dump", d), env={"CARTSLAM_VOXEL_MAP_SNAPSHOT": "1"})
        assert r.returncode == 0, r.stderr
        return d, {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if "voxel_m" in f or "voxel_c" in f}

    d, got = run("colour", color=True, color_max_weight=2)
    vcam = V.camera(**keys)
    ref = V.Map(64, 16, 64, V.params(**vp))
    cref = K.Color(ref, 2)
    seen, coloured_vertices = 0, 0
    for f in range(1, n + 1):
        disp = np.fromfile(os.path.join(d, f"{f}_disparity.bin"), np.int16).reshape(h, w)
        pose = np.frombuffer(open(os.path.join(d, f"{f}_ego_motion.bin"), "rb").read(), "<f8", 12, 120).tolist()
        vm = read_dump(os.path.join(d, f"{f}_voxel_map.bin"), w, h)
        ref.origin = vm["origin"]                                             # the colour restatement reads nothing else of the map
        rn = cref.integrate(vcam, pose, disp, images[f - 1][0])
        vc = read_colour_dump(os.path.join(d, f"{f}_voxel_color.bin"), w, h)
        assert vc["integrated"] == 1 and vc["counts"].tobytes() == rn.tobytes() and rn[0] == vm["counts"][1] > 1000, (f, vc["counts"], rn, vm["counts"])
        raw = got[f"{f}_voxel_color_voxels.bin"]
        assert tuple(np.frombuffer(raw, "<i8", 3).tolist()) == cref.origin and raw[24:] == cref.read()[0].tobytes(), f"frame {f}: colour voxels"
        rr = cref.render(vcam, pose, vm["disp"])
        assert vc["image"].tobytes() == rr["image"].tobytes() and vc["alpha"].tobytes() == rr["alpha"].tobytes() and vc["rendered"] == rr["counts"][0], f"frame {f}: image_model"
        seen += int(rr["counts"][0])
        name = f"{f}_voxel_mesh_colors.bin"
        assert (name in got) == (f % 2 == 0) == (f"{f}_voxel_mesh.bin" in got), sorted(got)
        if f % 2 == 0:
            mesh = read_mesh_dump(os.path.join(d, f"{f}_voxel_mesh.bin"))
            exp = cref.colorize(mesh["vertices"], mesh["origin"])
            assert np.frombuffer(got[name], "<i4", 1)[0] == len(exp) > 200 and got[name][4:] == exp.tobytes(), f"frame {f}: mesh colours"
            coloured_vertices += int((exp["weight"] > 0).sum())
    assert seen > w * h and coloured_vertices > 200 and (cref.weight == 2).sum() > 1000     # the plane 25 m away has the frames' texture

    # without "color": the files of before, with the bytes of the run above
    d, plain = run("plain")
    assert sorted(plain) == sorted(f for f in got if "voxel_c" not in f and "voxel_mesh_colors" not in f) and len(plain) == 2 * n + n // 2
    assert all(plain[f] == got[f] for f in plain)
    r = run_exe(src, head + [dict(module, color=True, color_max_weight=0)], tmp)
    assert r.returncode != 0 and "color_max_weight" in r.stderr, r.stderr

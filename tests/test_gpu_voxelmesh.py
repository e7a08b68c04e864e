"""GPU tests of the surface mesh of the TSDF volume (spec S36): cart_voxel_map_mesh against the numpy restatement
tests/np_voxelmesh.py, byte for byte over vertices, quads, counts and origin, on output buffers that start one word into their allocation
with sentinel words around them; cart_voxel_map_write, which puts the volumes under the kernels.  Beside every byte comparison stands a
numeric premise on the restatement (vertices and quads found), so that no comparison passes on an empty case.

The kernels as built: a thread owns one window voxel in linear order, a workgroup 1024 of them (kMeshBlock); the scan is one workgroup of
1024 threads (kMeshScanThreads), each over a run of consecutive workgroups: the volumes below have 4, 15, 27, 32 and 1088 workgroups (runs
of two, the last threads without one), the 24 x 24 x 24 volume of the spheres 13 and a half."""
import ctypes as C

import numpy as np
import pytest

import np_voxelmap as V
import np_voxelmesh as M
import test_voxelmap_spec as S
import test_voxelmesh_spec as MS
from test_gpu_voxelmap import SENTINEL, SMALL, _torch, cam_for, engine, frame_for, integrate, raycast, same_ray, same_volume

pytestmark = pytest.mark.gpu

VOLUMES = [(16, 16, 16), (24, 16, 40), (72, 16, 24), (64, 32, 16), (136, 64, 128)]
ORIGIN = (-8, 40, -56)                                                        # a non-zero toroidal offset on every axis of every volume above


class Out:
    """The three outputs of one call: int32 words filled with the sentinel, the records one word into the allocation (4-byte aligned only)."""

    def __init__(self, max_vertices, max_quads, stream=None):
        torch = _torch()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            self.v = torch.full((6 * max_vertices + 2,), SENTINEL, dtype=torch.int32, device="cuda")
            self.q = torch.full((4 * max_quads + 2,), SENTINEL, dtype=torch.int32, device="cuda")
            self.n = torch.full((6,), SENTINEL, dtype=torch.int32, device="cuda")
        self.max_vertices, self.max_quads, self.origin = max_vertices, max_quads, None

    def pointers(self):
        return C.c_void_p(self.v.data_ptr() + 4), C.c_void_p(self.q.data_ptr() + 4), C.c_void_p(self.n.data_ptr() + 4)


def mesh_call(obj, min_weight, out, stream=None, vertices=0, quads=0, counts=0, max_vertices=None, max_quads=None):
    """cart_voxel_map_mesh -> (rc, message); vertices / quads / counts replace the pointer of `out` when given (None = NULL)."""
    from cartslam import _lib
    torch = _torch()
    lib = _lib.load()
    pv, pq, pn = out.pointers()
    pv, pq, pn = (pv if vertices == 0 else vertices), (pq if quads == 0 else quads), (pn if counts == 0 else counts)
    o = (C.c_int64 * 3)(7, 7, 7)
    sp = C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)
    rc = lib.cart_voxel_map_mesh(obj._h if obj is not None else None, min_weight, pv, out.max_vertices if max_vertices is None else max_vertices, pq,
                                 out.max_quads if max_quads is None else max_quads, pn, o, sp)
    out.origin = tuple(o)
    return rc, lib.cart_last_error(None).decode()


def mesh(obj, min_weight, max_vertices, max_quads, stream=None):
    out = Out(max_vertices, max_quads, stream)
    rc, err = mesh_call(obj, min_weight, out, stream)
    assert rc == 0, err
    return out


def same_mesh(out, ref, origin):
    """Every word of the three allocations: the written records equal the restatement's, everything else still holds the sentinel."""
    _torch().cuda.synchronize()
    n = out.n.cpu().numpy()
    assert n[1:5].tobytes() == ref["counts"].tobytes(), (n[1:5], ref["counts"])
    assert n[0] == SENTINEL and n[5] == SENTINEL
    assert out.origin == tuple(origin), (out.origin, origin)
    for words, records, per in ((out.v.cpu().numpy(), ref["vertices"], 6), (out.q.cpu().numpy(), ref["quads"], 4)):
        k = per * len(records)
        assert words[1:1 + k].tobytes() == records.tobytes(), f"{int((words[1:1 + k] != np.frombuffer(records.tobytes(), np.int32)).sum())} words differ"
        assert words[0] == SENTINEL and (words[1 + k:] == SENTINEL).all(), "words outside the written records were touched"


def write_volume(obj, tsdf, weight, origin):
    vox = MS.voxels_of(tsdf, weight)
    obj.write(vox, origin)
    back, o = obj.read()
    assert o == tuple(origin) and back.tobytes() == vox.tobytes()             # write then read: the same bytes and origin
    assert obj.window() == (tuple(origin), (obj.cells_x, obj.cells_y, obj.cells_z), True)


def check(obj, tsdf, weight, origin, min_weight, own=1, least=(50, 10), caps=None):
    """One extraction against the restatement; min_weight 0 stands for the map's own (`own`).  -> the restatement's counts."""
    full = M.extract(tsdf, weight, min_weight or own, obj.params.voxel_size)
    assert full["counts"][0] >= least[0] and full["counts"][1] >= least[1], full["counts"]
    caps = caps or (int(full["counts"][0]) + 3, int(full["counts"][1]) + 3)
    ref = M.extract(tsdf, weight, min_weight or own, obj.params.voxel_size, *caps) if caps else full
    same_mesh(mesh(obj, min_weight, *caps), ref, origin)
    return full["counts"]


@pytest.mark.parametrize("shape", VOLUMES)
def test_random_volumes_through_write(shape):
    from cartslam import VoxelMap, voxel_map_params
    big = shape[0] * shape[1] * shape[2] > 100000
    cells = (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
    with VoxelMap(engine(), *shape, voxel_map_params(min_weight=2)) as obj:
        tsdf, weight = MS.random_volume(shape[0] + 1, shape, unknown=1.0 / 16)
        write_volume(obj, tsdf, weight, ORIGIN)
        n = check(obj, tsdf, weight, ORIGIN, 1, least=(cells // 4, cells // 40))
        assert n[0] < cells * 3 // 4                                          # about 0.6 of the cells are known
        tsdf, weight = MS.random_volume(shape[0] + 2, shape)                  # fully known: nearly every cell is active
        write_volume(obj, tsdf, weight, (0, 0, 0))
        n = check(obj, tsdf, weight, (0, 0, 0), 1, least=(cells * 9 // 10, cells))
        if not big:
            tsdf, weight = MS.random_volume(shape[0] + 3, shape, weights=True)
            write_volume(obj, tsdf, weight, (ORIGIN[2], ORIGIN[0], ORIGIN[1]))
            n1 = check(obj, tsdf, weight, (ORIGIN[2], ORIGIN[0], ORIGIN[1]), 1, least=(cells // 2, cells // 10))
            n2 = check(obj, tsdf, weight, (ORIGIN[2], ORIGIN[0], ORIGIN[1]), 0, own=2, least=(cells // 3, cells // 20))   # the map's own min_weight
            assert n2[0] < n1[0] and n2[1] < n1[1]


@pytest.mark.parametrize("radius,centre,hollow", [MS.SPHERES[0], MS.SPHERES[3]])
def test_sphere_through_write(radius, centre, hollow):
    from cartslam import VoxelMap
    tsdf, weight = MS.sphere_volume(radius, centre, hollow)
    with VoxelMap(engine(), 24, 24, 24) as obj:
        write_volume(obj, tsdf, weight, (16, -16, 8))
        n = check(obj, tsdf, weight, (16, -16, 8), 0, least=(200, 200))
        assert n[0] - 2 * n[1] + n[1] == 2                                    # closed: V - E + F with E = 2 F


def test_integrated_frames_and_a_window_that_moved():
    """Three frames of small_frame at 40 x 24 on the small volume; the window moves by 8 on z before the third.  The prototype of the rule
    found 34 to 98 vertices and 16 to 57 quads on such frames."""
    from cartslam import VoxelMap, voxel_map_params
    w, h = 40, 24
    cam = cam_for(w, h)
    poses = [S.pose_t(tz=0.5 * k) for k in range(3)]
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    origins = []
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as obj:
        for k, pose in enumerate(poses):
            disp, mask = frame_for(70 + k, w, h, cam, masked=False)
            integrate(obj, cam, pose, disp, mask)
            ref.integrate(cam, pose, disp, mask)
            origins.append(ref.origin)
            # measured on the restatement: 15 vertices and no quad after the first frame (one observation does not close a cell ring), then
            # 58 / 29 and 66 / 26; nothing is known at min_weight 2 before a voxel was seen twice from the same window
            check(obj, ref.tsdf, ref.weight, ref.origin, 0, least=(34, 16) if k else (10, 0))
        same_volume(obj, ref)                                                 # the extraction changed nothing
    assert origins[2][2] == origins[1][2] + 8 == origins[0][2] + 8, origins


def test_truncation_keeps_the_prefix_and_the_sentinel():
    from cartslam import VoxelMap
    tsdf, weight = MS.random_volume(5, (24, 16, 40), unknown=1.0 / 16)
    with VoxelMap(engine(), 24, 16, 40) as obj:
        write_volume(obj, tsdf, weight, ORIGIN)
        nv, nq = check(obj, tsdf, weight, ORIGIN, 0)[:2]
        for caps in ((int(nv) // 3, int(nq) // 2), (1, 1), (int(nv), 7), (300, int(nq))):
            check(obj, tsdf, weight, ORIGIN, 0, caps=caps)


def test_write_then_raycast_and_integrate_continue():
    from cartslam import VoxelMap, voxel_map_params
    w, h = 63, 24
    cam = cam_for(w, h)
    frames = [(S.pose_t(tz=0.125 * k), *frame_for(40 + k, w, h, cam, masked=False)) for k in range(3)]
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    for pose, disp, _ in frames[:2]:
        ref.integrate(cam, pose, disp)
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as obj:
        write_volume(obj, ref.tsdf, ref.weight, ref.origin)
        rr = ref.raycast(cam, frames[1][0], w, h)
        assert rr["counts"][V.HIT] > 0
        same_ray(raycast(obj, cam, frames[1][0], w, h), rr)
        integrate(obj, cam, frames[2][0], frames[2][1])                       # continues as after any integrate
        rn = ref.integrate(cam, frames[2][0], frames[2][1])
        assert rn[1] > 0
        same_volume(obj, ref)
        obj.clear()
        write_volume(obj, ref.tsdf, ref.weight, (ref.origin[0] + 8, ref.origin[1], ref.origin[2] - 16))   # after clear, elsewhere
        check(obj, ref.tsdf, ref.weight, (ref.origin[0] + 8, ref.origin[1], ref.origin[2] - 16), 0, least=(20, 8))


def test_no_window_gives_zero_counts():
    from cartslam import VoxelMap
    tsdf, weight = MS.random_volume(6)
    with VoxelMap(engine(), 16, 16, 16) as obj:
        empty = dict(vertices=np.zeros(0, M.MESH_VERTEX_DTYPE), quads=np.zeros(0, M.MESH_QUAD_DTYPE), counts=np.zeros(4, np.int32))
        same_mesh(mesh(obj, 0, 50, 50), empty, (0, 0, 0))
        write_volume(obj, tsdf, weight, ORIGIN)
        check(obj, tsdf, weight, ORIGIN, 0)
        obj.clear()
        same_mesh(mesh(obj, 0, 50, 50), empty, (0, 0, 0))


def test_queued_calls_on_one_stream_and_on_two():
    """The calls of one map share its workspace: nothing but the object's own ordering keeps the second from overwriting the first's."""
    from cartslam import VoxelMap
    torch = _torch()
    tsdf, weight = MS.random_volume(7, (64, 32, 16), weights=True)
    refs = {mw: M.extract(tsdf, weight, mw, 0.125) for mw in (1, 2)}
    assert refs[2]["counts"][1] > 1000 and refs[1]["counts"][0] > refs[2]["counts"][0] + 1000            # the two calls' results differ widely
    caps = (int(refs[1]["counts"][0]), int(refs[1]["counts"][1]))
    side = torch.cuda.Stream()
    with VoxelMap(engine(), 64, 32, 16) as obj:
        write_volume(obj, tsdf, weight, ORIGIN)
        outs = [(mw, mesh(obj, mw, *caps, stream=stream)) for mw, stream in ((1, None), (2, None), (1, side), (2, None), (1, None), (2, side), (1, side))]
        torch.cuda.synchronize()
        for mw, out in outs:
            same_mesh(out, refs[mw], ORIGIN)


def test_the_python_class():
    from cartslam import MESH_QUAD_DTYPE, MESH_VERTEX_DTYPE, EngineError, VoxelMap
    torch = _torch()
    tsdf, weight = MS.random_volume(8, unknown=1.0 / 16)
    ref = M.extract(tsdf, weight, 1, 0.125)
    assert ref["counts"][1] > 10
    with VoxelMap(engine(), 16, 16, 16) as obj:
        obj.write(MS.voxels_of(tsdf, weight), ORIGIN)
        v, q, n, o = obj.mesh(4000, 4000)
        assert v.dtype == MESH_VERTEX_DTYPE and q.dtype == MESH_QUAD_DTYPE and n.dtype == np.int32 and o == ORIGIN
        assert v.tobytes() == ref["vertices"].tobytes() and q.tobytes() == ref["quads"].tobytes() and n.tobytes() == ref["counts"].tobytes()
        v, q, n, o = obj.mesh(100, 4000, min_weight=1, stream=torch.cuda.Stream())
        assert len(v) == 100 and v.tobytes() == ref["vertices"][:100].tobytes() and n.tolist() == [len(ref["vertices"]), len(q), 100, len(q)]
        vt, qt, nt, o = obj.mesh(4000, 4000, raw=True)
        assert vt.is_cuda and tuple(vt.shape) == (4000, 6) and tuple(qt.shape) == (4000, 4) and nt.cpu().numpy().tobytes() == ref["counts"].tobytes()
        assert vt[:100].cpu().numpy().tobytes() == ref["vertices"][:100].tobytes()
        with pytest.raises(EngineError, match="max_quads"):
            obj.mesh(10, 0)
        with pytest.raises(EngineError, match="min_weight"):
            obj.mesh(10, 10, min_weight=70000)
        with pytest.raises(EngineError, match="cells_z"):
            obj.write(MS.voxels_of(tsdf, weight)[:8], ORIGIN)
        with pytest.raises(EngineError, match="origin3\\[1\\]"):
            obj.write(MS.voxels_of(tsdf, weight), (0, 12, 0))
        assert obj.window()[0] == ORIGIN                                      # the refused calls changed nothing


def test_bad_arguments_touch_no_output():
    from cartslam import VoxelMap, _lib
    torch = _torch()
    lib = _lib.load()
    tsdf, weight = MS.random_volume(9)
    ref = M.extract(tsdf, weight, 1, 0.125, 4000, 5000)
    assert ref["counts"][1] > 4000
    out = Out(4000, 5000)
    pv, pq, pn = [p.value for p in out.pointers()]
    with VoxelMap(engine(), 16, 16, 16) as obj:
        write_volume(obj, tsdf, weight, ORIGIN)

        def refused(word, obj_=obj, min_weight=0, **kw):
            rc, err = mesh_call(obj_, min_weight, out, **kw)
            assert rc != 0 and word in err, (kw, err)

        refused("map is NULL", obj_=None)
        refused("min_weight", min_weight=-1)
        refused("max_vertices", max_vertices=0)
        refused("max_quads", max_quads=(1 << 26) + 1)
        refused("vertices is NULL", vertices=None)
        refused("quads is NULL", quads=None)
        refused("counts is NULL", counts=None)
        refused("vertices must be 4-byte aligned", vertices=C.c_void_p(pv + 2))
        refused("quads must be 4-byte aligned", quads=C.c_void_p(pq + 1))
        refused("counts must be 4-byte aligned", counts=C.c_void_p(pn + 3))
        refused("vertices and quads must not overlap", quads=C.c_void_p(pv + 24 * 4000 - 4))
        refused("vertices and quads must not overlap", vertices=C.c_void_p(pq + 16 * 5000 - 4), max_vertices=1)
        refused("vertices and counts must not overlap", counts=C.c_void_p(pv))
        refused("quads and counts must not overlap", counts=C.c_void_p(pq + 16 * 5000 - 16))
        o = (C.c_int64 * 3)(0, 0, 0)
        assert lib.cart_voxel_map_write(obj._h, None, o, None) != 0 and lib.cart_last_error(None).decode() == "host_voxels is NULL"
        torch.cuda.synchronize()
        for t in (out.v, out.q, out.n):
            assert bool((t == SENTINEL).all())                                # no refused call touched an output
        assert obj.window()[0] == ORIGIN
        rc, err = mesh_call(obj, 0, out)
        assert rc == 0, err
        same_mesh(out, ref, ORIGIN)


# ---- the C++ frame loop ------------------------------------------------------------------------------------------------------------
def read_mesh_dump(path):
    raw = open(path, "rb").read()
    out = dict(origin=tuple(np.frombuffer(raw, "<i8", 3).tolist()), voxel_size=float(np.frombuffer(raw, "<f8", 1, 24)[0]), counts=np.frombuffer(raw, "<i4", 4, 32))
    nv, nq = int(out["counts"][2]), int(out["counts"][3])
    assert len(raw) == 48 + 24 * nv + 16 * nq, path
    out["vertices"] = np.frombuffer(raw, M.MESH_VERTEX_DTYPE, nv, 48)
    out["quads"] = np.frombuffer(raw, M.MESH_QUAD_DTYPE, nq, 48 + 24 * nv)
    return out


def test_voxel_map_module_extracts_every_second_frame(tmp_path):
    """cart_slam_amd over four synthetic frames (the scene and the head of test_gpu_voxelmap's module test) with "mesh": true and
    "mesh_interval": 2: frames 2 and 4 dump a mesh that equals the restatement's extraction of the same frame's dumped voxels, frames 1 and
    3 dump none; a capacity below the found counts truncates; without "mesh" the module dumps what it dumped before, byte for byte."""
    import json
    import os
    from test_gpu_matches import noise_frame, noise_world
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n = 4
    world = noise_world(79)
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for side in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, side))
    for f in range(n):
        l, r = noise_frame(world, f)
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    vp = dict(voxel_size=0.5, min_disparity=3.5, max_depth=40.0, truncation=1.0, march_step=0.5, lookahead=16.0, max_weight=3)
    shape = dict(cells_x=64, cells_y=16, cells_z=64)
    head = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
            {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion")]
    module = dict(keys, type="voxel_map", raycast=False, **shape, **vp)

    def run(name, **extra):
        d = os.path.join(tmp, name)
        os.makedirs(d)
        r = run_exe(src, head + [dict(module, **extra)], tmp, ("--dump", d), env={"CARTSLAM_VOXEL_MAP_SNAPSHOT": "1"})
        assert r.returncode == 0, r.stderr
        return d, {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if "voxel_m" in f}

    d, with_mesh = run("mesh", mesh=True, mesh_interval=2)
    found = []
    for f in range(1, n + 1):
        name = f"{f}_voxel_mesh.bin"
        assert (name in with_mesh) == (f % 2 == 0), sorted(with_mesh)
        if f % 2:
            continue
        vox = np.frombuffer(with_mesh[f"{f}_voxel_map_voxels.bin"], V.VOXEL_DTYPE).reshape(64, 16, 64)
        origin = tuple(np.frombuffer(with_mesh[f"{f}_voxel_map.bin"], "<i8", 3).tolist())
        ref = M.extract(vox["tsdf"], vox["weight"], 1, 0.5, 1 << 20, 1 << 20)
        got = read_mesh_dump(os.path.join(d, name))
        assert got["origin"] == origin and got["voxel_size"] == 0.5, f"frame {f}: window"
        assert got["counts"].tobytes() == ref["counts"].tobytes(), (f, got["counts"], ref["counts"])
        assert got["vertices"].tobytes() == ref["vertices"].tobytes() and got["quads"].tobytes() == ref["quads"].tobytes(), f"frame {f}: records"
        found.append(ref["counts"])
    assert all(c[0] > 200 and c[1] > 100 for c in found), found               # the plane 25 m away is a surface of the model

    # capacities below the found counts, min_weight 2, every frame: the written prefix
    d, cut = run("cut", mesh=True, mesh_interval=1, mesh_max_vertices=150, mesh_max_quads=70, mesh_min_weight=2)
    vox = np.frombuffer(cut["4_voxel_map_voxels.bin"], V.VOXEL_DTYPE).reshape(64, 16, 64)
    ref = M.extract(vox["tsdf"], vox["weight"], 2, 0.5, 150, 70)
    got = read_mesh_dump(os.path.join(d, "4_voxel_mesh.bin"))
    assert ref["counts"][0] > 150 and ref["counts"][1] > 70 and got["counts"].tobytes() == ref["counts"].tobytes(), (got["counts"], ref["counts"])
    assert got["vertices"].tobytes() == ref["vertices"].tobytes() and got["quads"].tobytes() == ref["quads"].tobytes()
    assert all(f"{f}_voxel_mesh.bin" in cut for f in range(1, n + 1))

    # without "mesh": the files of before, with the bytes of the run above
    d, plain = run("plain")
    assert sorted(plain) == sorted(f for f in with_mesh if "voxel_mesh" not in f) and len(plain) == 2 * n
    assert all(plain[f] == with_mesh[f] for f in plain)

    # configuration errors name their key
    for bad, word in ((dict(mesh=True, mesh_interval=0), "mesh_interval"), (dict(mesh=True, mesh_max_vertices=0), "mesh_max_vertices"),
                      (dict(mesh=True, mesh_max_quads=0), "mesh_max_quads"), (dict(mesh=True, mesh_min_weight=-1), "mesh_min_weight")):
        r = run_exe(src, head + [dict(module, **bad)], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)

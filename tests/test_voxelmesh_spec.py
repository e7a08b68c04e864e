"""CPU tests of spec S36, the surface mesh of the TSDF volume by naive surface nets: the numpy restatement
tests/np_voxelmesh.py against a scalar twin written here (a pure-Python loop over cells and voxels in Python floats and integers), the
hand-worked case, closed spheres, the accuracy of the spec on the synthetic corridor against the analytic scene, truncation, write_ply and
the library's host-side checks (no GPU: validation comes before any device call).  tests/test_gpu_voxelmesh.py runs the device against
the restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import np_voxelmap as V
import np_voxelmesh as M
import test_voxelmap_spec as S


# ---- the scalar twin ----------------------------------------------------------------------------------------------------------------
def scalar_extract(tsdf, weight, mw, vs):
    """Spec S36 one cell and one voxel edge at a time.  -> (vertices [(position, normal)] as Python floats, quads [[4 indices]])."""
    nz, ny, nx = tsdf.shape
    t = lambda x, y, z: int(tsdf[z, y, x])
    known, index, verts = {}, {}, []
    for cz in range(nz - 1):
        for cy in range(ny - 1):
            for cx in range(nx - 1):
                corners = [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
                known[(cx, cy, cz)] = all(int(weight[cz + dz, cy + dy, cx + dx]) >= mw for dx, dy, dz in corners)
                inside = [t(cx + dx, cy + dy, cz + dz) <= 0 for dx, dy, dz in corners]
                if not known[(cx, cy, cz)] or all(inside) or not any(inside):
                    continue
                T = {d: t(cx + d[0], cy + d[1], cz + d[2]) for d in corners}
                s, n = [0.0, 0.0, 0.0], 0
                for axis in range(3):
                    for p, q in ((0, 0), (1, 0), (0, 1), (1, 1)):
                        a = [p, q]
                        a.insert(axis, 0)
                        b = list(a)
                        b[axis] = 1
                        ta, tb = T[tuple(a)], T[tuple(b)]
                        if (ta <= 0) == (tb <= 0):
                            continue
                        f = float(ta) / float(ta - tb)
                        for k in range(3):
                            s[k] = s[k] + (f if k == axis else float(a[k]))
                        n += 1
                l = [s[k] / float(n) for k in range(3)]
                pos = [((float(c) + 0.5) + l[k]) * vs for k, c in enumerate((cx, cy, cz))]
                # voxel_value's gradient (S34) with t[dy][dz][dx]
                d = {(dy, dz): float(T[(1, dy, dz)] - T[(0, dy, dz)]) for dy in (0, 1) for dz in (0, 1)}
                c = {(dy, dz): float(T[(0, dy, dz)]) + l[0] * d[(dy, dz)] for dy in (0, 1) for dz in (0, 1)}
                h0, h1 = c[(1, 0)] - c[(0, 0)], c[(1, 1)] - c[(0, 1)]
                e0, e1 = c[(0, 0)] + l[1] * h0, c[(0, 1)] + l[1] * h1
                gz = e1 - e0
                gy = h0 + l[2] * (h1 - h0)
                a0, a1 = d[(0, 0)] + l[1] * (d[(1, 0)] - d[(0, 0)]), d[(0, 1)] + l[1] * (d[(1, 1)] - d[(0, 1)])
                gx = a0 + l[2] * (a1 - a0)
                n2 = (gx * gx + gy * gy) + gz * gz
                normal = [g / math.sqrt(n2) for g in (gx, gy, gz)] if n2 > 0.0 else [0.0, 0.0, 0.0]
                index[(cx, cy, cz)] = len(verts)
                verts.append((pos, normal))
    quads = []
    around = {0: ((0, -1, -1), (0, 0, -1), (0, 0, 0), (0, -1, 0)), 1: ((-1, 0, -1), (-1, 0, 0), (0, 0, 0), (0, 0, -1)),
              2: ((-1, -1, 0), (0, -1, 0), (0, 0, 0), (-1, 0, 0))}
    for k in range(nz - 1):                                                   # voxels in cell-index order: only a cell's origin voxel can emit
        for j in range(ny - 1):
            for i in range(nx - 1):
                for axis in range(3):
                    up = [i, j, k]
                    up[axis] += 1
                    lower_in = t(i, j, k) <= 0
                    if lower_in == (t(*up) <= 0):
                        continue
                    cells = [(i + o[0], j + o[1], k + o[2]) for o in around[axis]]
                    if not all(known.get(cell, False) for cell in cells):      # a cell that does not exist is not in the dict
                        continue
                    v = [index[cell] for cell in cells]
                    quads.append(v if lower_in else v[::-1])
    return verts, quads


def same_as_scalar(tsdf, weight, mw, vs=0.125):
    got = M.extract(tsdf, weight, mw, vs)
    verts, quads = scalar_extract(tsdf, weight, mw, vs)
    ref_v = np.zeros(len(verts), M.MESH_VERTEX_DTYPE)
    for k, (p, n) in enumerate(verts):
        ref_v["position"][k], ref_v["normal"][k] = np.array(p, np.float64).astype(np.float32), np.array(n, np.float64).astype(np.float32)
    ref_q = np.array(quads, np.int32).reshape(-1, 4)
    assert got["counts"].tolist() == [len(verts), len(quads), len(verts), len(quads)]
    assert got["vertices"].tobytes() == ref_v.tobytes() and got["quads"]["v"].tobytes() == ref_q.tobytes()
    return got


def random_volume(seed, shape=(16, 16, 16), unknown=0.0, weights=None):
    """Uniformly random tsdf over the whole int16 range; unknown = the share of voxels of weight 0; weights = True for random weights in
    0..3, the two low ones at 1 / 32 each: at min_weight 1 and 2 about 3 / 4 and 3 / 5 of the cells stay known (uniform weights would leave
    one cell in ten, and one in 250)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    tsdf = rng.integers(-32767, 32768, (nz, ny, nx)).astype(np.int16)
    if weights is not None:
        weight = rng.choice(4, (nz, ny, nx), p=[1 / 32, 1 / 32, 15 / 32, 15 / 32]).astype(np.uint16)
    else:
        weight = np.ones((nz, ny, nx), np.uint16)
        weight[rng.random((nz, ny, nx)) < unknown] = 0
    return tsdf, weight


def sphere_volume(radius, centre, hollow, shape=(24, 24, 24)):
    """tsdf = round(clip((|x - c| - r) / 2 voxels) 32767) at the voxel centres x = index + 0.5, all weights 1; hollow flips the sign."""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz) + 0.5, np.arange(ny) + 0.5, np.arange(nx) + 0.5, indexing="ij")
    dist = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    f = np.clip((dist - radius) / 2.0, -1.0, 1.0)
    tsdf = np.round((-f if hollow else f) * 32767.0).astype(np.int16)
    return tsdf, np.ones((nz, ny, nx), np.uint16)


def voxels_of(tsdf, weight):
    v = np.zeros(tsdf.shape, V.VOXEL_DTYPE)
    v["tsdf"], v["weight"] = tsdf, weight
    return v


@pytest.mark.parametrize("seed,unknown,weights,mw", [(1, 0.0, None, 1), (2, 1.0 / 16, None, 1), (3, 0.0, True, 1), (4, 0.0, True, 2)])
def test_vectorised_restatement_equals_the_scalar_loop(seed, unknown, weights, mw):
    tsdf, weight = random_volume(seed, unknown=unknown, weights=weights)
    got = same_as_scalar(tsdf, weight, mw)
    assert got["counts"][0] > 100 and got["counts"][1] > 20, got["counts"]
    if unknown or weights:
        assert got["counts"][0] < 15 ** 3 - 100                               # unknown cells left their mark


def test_a_random_known_volume_reaches_all_256_corner_configurations():
    tsdf, weight = random_volume(1)
    inside = tsdf <= 0
    code = np.zeros((15, 15, 15), np.int64)
    for bit, d in enumerate([(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]):
        code |= M.corner(inside, d).astype(np.int64) << bit
    assert len(np.unique(code)) == 256
    got = M.extract(tsdf, weight, 1, 0.125)
    assert got["counts"][0] == int(((code != 0) & (code != 255)).sum()) > 3300   # nearly every cell is active


def test_hand_worked_example():
    tsdf = np.full((16, 16, 16), 16384, np.int16)
    tsdf[8:] = -16384
    got = same_as_scalar(tsdf, np.ones((16, 16, 16), np.uint16), 1)
    assert got["counts"].tolist() == [225, 196, 225, 196]
    v, q = got["vertices"], got["quads"]["v"]
    cy, cx = np.mgrid[0:15, 0:15]
    exp = np.stack([(cx.reshape(-1) + 1) / 8.0, (cy.reshape(-1) + 1) / 8.0, np.ones(225)], axis=1).astype(np.float32)
    assert v["position"].tobytes() == exp.tobytes()
    assert (v["normal"] == np.array([0, 0, -1], np.float32)).all()
    assert got["active"][7].all() and got["active"].sum() == 225
    # the z-edges at i, j = 1..14, voxel k = 7 outside: reversed, (i-1,j), (i,j), (i,j-1), (i-1,j-1)
    j, i = [a.reshape(-1) for a in np.mgrid[1:15, 1:15]]
    cell = lambda a, b: b * 15 + a
    assert q.tobytes() == np.stack([cell(i - 1, j), cell(i, j), cell(i, j - 1), cell(i - 1, j - 1)], axis=1).astype(np.int32).tobytes()
    p = v["position"].astype(np.float64)
    cross = np.cross(p[q[:, 2]] - p[q[:, 0]], p[q[:, 3]] - p[q[:, 1]])
    assert (cross[:, 2] < 0).all() and (cross[:, :2] == 0).all()              # towards -z: the free side


SPHERES = [(4.1, (11.3, 12.6, 11.9), False), (4.1, (12.2, 11.4, 12.7), True), (6.3, (11.7, 12.2, 12.4), False), (6.3, (12.45, 11.8, 11.55), True)]


@pytest.mark.parametrize("radius,centre,hollow", SPHERES)
def test_spheres_are_closed_and_accurate(radius, centre, hollow):
    """The prototype of the rule measured 0.089 voxel and cos 0.9885 at the worst; the bounds are the issue's."""
    tsdf, weight = sphere_volume(radius, centre, hollow)
    got = M.extract(tsdf, weight, 1, 1.0)                                     # voxel_size 1: positions in voxels
    v, q = got["vertices"], got["quads"]["v"].astype(np.int64)
    assert len(v) > 200 and len(q) > 200
    edges = np.sort(np.stack([q, np.roll(q, -1, axis=1)], axis=2).reshape(-1, 2), axis=1)
    uniq, count = np.unique(edges, axis=0, return_counts=True)
    assert (count == 2).all()                                                 # closed: every mesh edge belongs to exactly two quads
    assert len(np.unique(q)) == len(v) and len(v) - len(uniq) + len(q) == 2   # V - E + F = 2
    p = v["position"].astype(np.float64) - np.array(centre)
    r = np.sqrt((p ** 2).sum(axis=1))
    free = -1.0 if hollow else 1.0                                            # free space: outside a ball, inside a hollow
    cos = free * (v["normal"].astype(np.float64) * p).sum(axis=1) / r
    print(radius, hollow, "distance", np.abs(r - radius).max(), "cos", cos.min())
    assert np.abs(r - radius).max() <= 0.15
    assert cos.min() >= 0.98
    P = v["position"].astype(np.float64)
    cross = np.cross(P[q[:, 2]] - P[q[:, 0]], P[q[:, 3]] - P[q[:, 1]])
    mid = P[q].mean(axis=1) - np.array(centre)
    assert (free * (cross * mid).sum(axis=1) > 0).all()                      # every quad's diagonal cross product points to free space


def test_truncation_writes_the_prefix():
    tsdf, weight = random_volume(2, unknown=1.0 / 16)
    full = M.extract(tsdf, weight, 1, 0.125)
    nv, nq = int(full["counts"][0]), int(full["counts"][1])
    cut = M.extract(tsdf, weight, 1, 0.125, max_vertices=nv // 3, max_quads=nq // 2)
    assert cut["counts"].tolist() == [nv, nq, nv // 3, nq // 2]
    assert cut["vertices"].tobytes() == full["vertices"][:nv // 3].tobytes() and cut["quads"].tobytes() == full["quads"][:nq // 2].tobytes()
    assert cut["quads"]["v"].max() >= nv // 3                                  # a quad may name a vertex that was not written
    same = M.extract(tsdf, weight, 1, 0.125, max_vertices=nv, max_quads=nq)
    assert same["counts"].tolist() == [nv, nq, nv, nq]


# ---- accuracy of the spec on the corridor -------------------------------------------------------------------------------------------
def corridor_map(step, seed=11, frames=6, w=160, h=64):
    """The frames of test_voxelmap_spec.corridor_run, integrated into its volume -> the np_voxelmap.Map after the last frame."""
    from cartslam import synth
    truth, _ = synth.road_corridor(w, h, *[S.ACC_CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline")])
    rng = np.random.default_rng(seed)
    ok = truth != V.INVALID
    m = V.Map(*S.ACC_SHAPE)
    for k in range(frames):
        d = truth.copy()
        d[ok] += rng.integers(-4, 5, int(ok.sum())).astype(np.int16)
        d[ok & (rng.random((h, w)) < 0.10)] = V.INVALID
        m.integrate(S.ACC_CAM, S.pose_t(tz=step * k), d)
    return m


# forward step (m per frame) -> measured on the restatement at seed 11 (14152 / 14681 / 16651 vertices, 13686 / 14168 / 15960 quads): rms and largest distance of a vertex to the nearest
# analytic surface of synth.road_corridor (ground Y = 1.65 m, walls X = -4 and +4 m), in voxels of 0.125 m
MESH_ACCURACY = {0.0: (0.4098, 2.0712), 0.25: (0.3935, 1.8580), 0.5: (0.4039, 1.8841)}


@pytest.mark.parametrize("step", sorted(MESH_ACCURACY))
def test_accuracy_on_the_corridor(step):
    """Measured values: see MESH_ACCURACY and DESIGN.md 7.18.  The reference is the analytic scene, not the code under test.  Each bound sits
    at twice the measured distance, so that the measured value lies half-way between the bound and zero, as 7.15 does."""
    m = corridor_map(step)
    got = M.extract(m.tsdf, m.weight, 1, V.DEFAULTS["voxel_size"])
    assert got["counts"][0] > 5000 and got["counts"][1] > 4000, got["counts"]
    p = M.world_positions(got["vertices"], m.origin, V.DEFAULTS["voxel_size"])
    dist = np.minimum(np.minimum(np.abs(p[:, 1] - 1.65), np.abs(p[:, 0] - 4.0)), np.abs(p[:, 0] + 4.0)) / V.DEFAULTS["voxel_size"]
    rms, worst = float(np.sqrt((dist ** 2).mean())), float(dist.max())
    print(step, got["counts"].tolist(), "rms", rms, "max", worst)
    assert rms <= 2 * MESH_ACCURACY[step][0]
    assert worst <= 2 * MESH_ACCURACY[step][1]


# ---- the library's host side --------------------------------------------------------------------------------------------------------
def _lib():
    from cartslam import _lib
    return _lib, _lib.load()


def test_layout_defaults_and_exports():
    import inspect
    from cartslam import MESH_QUAD_DTYPE, MESH_VERTEX_DTYPE, MeshQuad, MeshVertex, VoxelMap, write_ply  # noqa: F401
    L, lib = _lib()
    assert C.sizeof(MeshVertex) == 24 and MeshVertex.normal.offset == 12 and C.sizeof(MeshQuad) == 16
    assert MESH_VERTEX_DTYPE.itemsize == 24 and MESH_VERTEX_DTYPE.fields["normal"][1] == 12 and MESH_QUAD_DTYPE.itemsize == 16
    assert MESH_VERTEX_DTYPE == M.MESH_VERTEX_DTYPE and MESH_QUAD_DTYPE == M.MESH_QUAD_DTYPE
    for name in ("mesh", "write"):
        assert hasattr(lib, "cart_voxel_map_" + name) and "cart_voxel_map_" + name in L.PROTOTYPES and hasattr(VoxelMap, name)
    sig = inspect.signature(VoxelMap.mesh).parameters
    assert list(sig) == ["self", "max_vertices", "max_quads", "min_weight", "raw", "stream"]
    assert (sig["min_weight"].default, sig["raw"].default, sig["stream"].default) == (0, False, None)


def mesh_error(min_weight=0, max_vertices=8, max_quads=8):
    L, lib = _lib()
    assert lib.cart_voxel_map_mesh(None, min_weight, None, max_vertices, None, max_quads, None, None, None) != 0
    return lib.cart_last_error(None).decode()


def write_error(origin=(0, 0, 0)):
    L, lib = _lib()
    o = (C.c_int64 * 3)(*origin) if origin is not None else None
    assert lib.cart_voxel_map_write(None, None, o, None) != 0
    return lib.cart_last_error(None).decode()


def test_mesh_checks_its_numbers_before_the_object():
    assert mesh_error() == "map is NULL"                                      # valid numbers get as far as the missing map
    assert mesh_error(65535, 1 << 26, 1 << 26) == "map is NULL" and mesh_error(1, 1, 1) == "map is NULL"
    for bad in (-1, 65536):
        assert "min_weight" in mesh_error(min_weight=bad)
    for bad in (0, -5, (1 << 26) + 1):
        assert "max_vertices" in mesh_error(max_vertices=bad) and "max_quads" in mesh_error(max_quads=bad)
    # the order: min_weight, max_vertices, max_quads, the object
    assert "min_weight" in mesh_error(-1, 0, 0) and "max_vertices" in mesh_error(0, 0, 0) and "max_quads" in mesh_error(0, 1, 0)


def test_write_checks_the_origin_before_the_object():
    assert write_error() == "map is NULL"
    assert write_error((-8, 16, 1 << 27)) == "map is NULL" and write_error((-(1 << 27), 0, 0)) == "map is NULL"
    assert write_error(None) == "origin3 is NULL"
    for k, bad in ((0, 4), (1, -7), (2, 1), (0, (1 << 27) + 8), (2, -(1 << 27) - 8)):
        o = [0, 0, 0]
        o[k] = bad
        assert f"origin3[{k}]" in write_error(o), o


# ---- write_ply ----------------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """A reader for what write_ply promises: binary little-endian, float vertex properties, one uchar-counted int list per face."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements, props = [], {}
    for line in lines[2:]:
        words = line.split()
        if words[:1] == ["element"]:
            elements.append((words[1], int(words[2])))
            props[words[1]] = []
        elif words[:1] == ["property"]:
            props[elements[-1][0]].append(words[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    assert props["vertex"] == [["float", c] for c in ("x", "y", "z", "nx", "ny", "nz")] and props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    nv, nf = elements[0][1], elements[1][1]
    vertices = np.frombuffer(raw, "<f4", 6 * nv, end).reshape(nv, 6)
    faces, at = [], end + 24 * nv
    for _ in range(nf):
        k = raw[at]
        faces.append(np.frombuffer(raw, "<i4", k, at + 1).tolist())
        at += 1 + 4 * k
    assert at == len(raw)
    return vertices, faces


def test_write_ply_round_trips(tmp_path):
    from cartslam import write_ply
    tsdf, weight = sphere_volume(4.1, (11.3, 12.6, 11.9), False)
    got = M.extract(tsdf, weight, 1, 0.125)
    origin = (-4000000, 8, 1 << 27)                                           # far origins: the shift happens in fp64 before the conversion
    path = str(tmp_path / "mesh.ply")
    write_ply(path, got["vertices"], got["quads"], origin, 0.125)
    vertices, faces = read_ply(path)
    assert len(vertices) == len(got["vertices"]) > 200 and len(faces) == len(got["quads"]) > 200
    assert vertices[:, :3].tobytes() == M.world_positions(got["vertices"], origin, 0.125).astype(np.float32).tobytes()
    assert vertices[:, 3:].tobytes() == got["vertices"]["normal"].tobytes()
    assert faces == got["quads"]["v"].tolist()
    write_ply(path, got["vertices"][:0], got["quads"][:0], (0, 0, 0), 0.125)  # an empty mesh is a valid file
    vertices, faces = read_ply(path)
    assert len(vertices) == 0 and faces == []

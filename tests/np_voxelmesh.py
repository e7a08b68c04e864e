"""numpy restatement of spec S36: the surface of the TSDF volume as an indexed quad mesh by naive surface nets.  Written
from the spec, not from the kernels: whole-volume array arithmetic in the spec's operation order (every numpy ufunc rounds once, there is no
fused multiply-add), a boolean-mask compaction in C order for the two output orders.  Works on window-order arrays [nz, ny, nx]."""
import numpy as np

MESH_VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3)])
MESH_QUAD_DTYPE = np.dtype([("v", "<i4", 4)])
# the twelve cell edges in the spec's order as (axis, lower corner (dx, dy, dz)): x-edges over (dy, dz), y-edges over (dx, dz), z-edges
# over (dx, dy), each over (0,0), (1,0), (0,1), (1,1)
PAIRS = ((0, 0), (1, 0), (0, 1), (1, 1))
EDGES = [(0, (0, p, q)) for p, q in PAIRS] + [(1, (p, 0, q)) for p, q in PAIRS] + [(2, (p, q, 0)) for p, q in PAIRS]
# the four cells around the edge that leaves voxel (i, j, k) along each axis, as offsets (di, dj, dk), in the spec's order
AROUND = {0: ((0, -1, -1), (0, 0, -1), (0, 0, 0), (0, -1, 0)),
          1: ((-1, 0, -1), (-1, 0, 0), (0, 0, 0), (0, 0, -1)),
          2: ((-1, -1, 0), (0, -1, 0), (0, 0, 0), (-1, 0, 0))}


def corner(a, d):
    """The [nz - 1, ny - 1, nx - 1] array of every cell's corner d = (dx, dy, dz) of the voxel array a."""
    nz, ny, nx = a.shape
    return a[d[2]:nz - 1 + d[2], d[1]:ny - 1 + d[1], d[0]:nx - 1 + d[0]]


def gradient(t, fr):
    """voxel_value's gradient (S34): t[(dx, dy, dz)] = corner tsdf arrays (int64), fr = [fr_x, fr_y, fr_z] -> (gx, gy, gz)."""
    D = {(dy, dz): (t[(1, dy, dz)] - t[(0, dy, dz)]).astype(np.float64) for dy in (0, 1) for dz in (0, 1)}
    c = {(dy, dz): t[(0, dy, dz)].astype(np.float64) + fr[0] * D[(dy, dz)] for dy in (0, 1) for dz in (0, 1)}
    h0, h1 = c[(1, 0)] - c[(0, 0)], c[(1, 1)] - c[(0, 1)]
    e0, e1 = c[(0, 0)] + fr[1] * h0, c[(0, 1)] + fr[1] * h1
    gz = e1 - e0
    gy = h0 + fr[2] * (h1 - h0)
    a0, a1 = D[(0, 0)] + fr[1] * (D[(1, 0)] - D[(0, 0)]), D[(0, 1)] + fr[1] * (D[(1, 1)] - D[(0, 1)])
    gx = a0 + fr[2] * (a1 - a0)
    return gx, gy, gz


def extract(tsdf, weight, min_weight, voxel_size, max_vertices=1 << 26, max_quads=1 << 26):
    """tsdf, weight = integer arrays [nz, ny, nx] in window order; min_weight >= 1 (the caller resolves 0 to the map's own).
    -> dict(vertices MESH_VERTEX_DTYPE [written], quads MESH_QUAD_DTYPE [written], counts int32 [4] = vertices found, quads found, vertices
    written, quads written, active = bool [nz - 1, ny - 1, nx - 1], index = the cells' vertex indices (-1 where a cell is not active))."""
    t, w = np.asarray(tsdf).astype(np.int64), np.asarray(weight).astype(np.int64)
    nz, ny, nx = t.shape
    vs = np.float64(voxel_size)
    ds = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    T = {d: corner(t, d) for d in ds}
    inside = {d: T[d] <= 0 for d in ds}
    known = np.ones((nz - 1, ny - 1, nx - 1), bool)
    n_inside = np.zeros(known.shape, np.int64)
    for d in ds:
        known &= corner(w, d) >= min_weight
        n_inside += inside[d]
    active = known & (n_inside > 0) & (n_inside < 8)
    # vertices
    s = [np.zeros(known.shape), np.zeros(known.shape), np.zeros(known.shape)]
    n = np.zeros(known.shape, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, a in EDGES:
            b = tuple(a[k] + (1 if k == axis else 0) for k in range(3))
            cross = inside[a] != inside[b]
            f = T[a].astype(np.float64) / (T[a] - T[b]).astype(np.float64)
            for k in range(3):
                s[k] = np.where(cross, s[k] + (f if k == axis else np.float64(a[k])), s[k])
            n += cross
        l = [s[k] / n.astype(np.float64) for k in range(3)]
        cz, cy, cx = np.meshgrid(np.arange(nz - 1, dtype=np.float64), np.arange(ny - 1, dtype=np.float64), np.arange(nx - 1, dtype=np.float64), indexing="ij")
        p = [((c + 0.5) + l[k]) * vs for k, c in enumerate((cx, cy, cz))]
        g = gradient(T, l)
        n2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        root = np.sqrt(n2)
        normal = [np.where(n2 > 0.0, g[k] / root, 0.0) for k in range(3)]
    found_v = int(active.sum())
    vertices = np.zeros(found_v, MESH_VERTEX_DTYPE)
    for k in range(3):
        vertices["position"][:, k] = p[k][active].astype(np.float32)            # boolean masks compact in C order: ascending cell index
        vertices["normal"][:, k] = normal[k][active].astype(np.float32)
    index = np.full(known.shape, -1, np.int64)
    index[active] = np.arange(found_v)
    # quads: per voxel (i, j, k) that is a cell's origin corner, per axis
    emit = np.zeros(known.shape + (3,), bool)
    rec = np.zeros(known.shape + (3, 4), np.int64)
    for axis in range(3):
        up = tuple(1 if k == axis else 0 for k in range(3))
        cross = inside[(0, 0, 0)] != inside[up]
        lo = [1 if any(o[k] < 0 for o in AROUND[axis]) else 0 for k in range(3)]          # the first voxel index with all four cells
        sub = (slice(lo[2], None), slice(lo[1], None), slice(lo[0], None))
        ok = cross[sub].copy()
        for c, o in enumerate(AROUND[axis]):
            sl = tuple(slice(lo[k] + o[k], known.shape[2 - k] + o[k]) for k in (2, 1, 0))
            ok &= known[sl]
            rec[sub + (axis, c)] = index[sl]
        emit[sub + (axis,)] = ok
    forward = inside[(0, 0, 0)][..., None, None]
    rec = np.where(forward, rec, rec[..., ::-1])
    quads = np.zeros(int(emit.sum()), MESH_QUAD_DTYPE)
    quads["v"] = rec[emit]                                                       # C order over (cell index, axis)
    found_q = len(quads)
    wv, wq = min(found_v, int(max_vertices)), min(found_q, int(max_quads))
    return dict(vertices=vertices[:wv], quads=quads[:wq], counts=np.array([found_v, found_q, wv, wq], np.int32), active=active, index=index)


def world_positions(vertices, origin, voxel_size):
    """o_a voxel_size + p_a in fp64 -> float64 [n, 3]."""
    return np.array([int(c) for c in origin], np.float64) * np.float64(voxel_size) + vertices["position"].astype(np.float64)

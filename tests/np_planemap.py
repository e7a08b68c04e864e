"""numpy restatement of spec S24: the world-frame bird's-eye plane map.  Written from the spec, not from the
kernels: whole-image array arithmetic in the spec's operation order (every numpy ufunc rounds once, there is no fused multiply-add),
votes by np.add.at / np.minimum.at / np.maximum.at over window cells, and a window that is rebuilt by copying the overlap of the old
one into a fresh empty array."""
import numpy as np

CELL_DTYPE = np.dtype([("horizontal", "<u4"), ("vertical", "<u4"), ("y_min", "<i4"), ("y_max", "<i4")])
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
INVALID = -32768
DEFAULTS = dict(cell_size=0.25, min_disparity=1.0, max_depth=20.0, max_lateral=10.0, height_quantum=0.05)
POSE_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise ValueError(k)
        p[k] = float(v)
    return p


def camera(fx, fy, cx, cy, baseline):
    return dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), baseline=float(baseline))


def empty_cells(nz, nx):
    c = np.zeros((nz, nx), CELL_DTYPE)
    c["y_min"], c["y_max"] = INT32_MAX, INT32_MIN
    return c


def window_origin(t, cell_size, n):
    """o = 16 floor_div(floor(t / cell_size) - n / 2, 16) in Python integers (floor division)."""
    c = int(np.floor(np.float64(t) / np.float64(cell_size)))
    return 16 * ((c - n // 2) // 16)


def votes(cam, p, pose, disp, planes):
    """The accepted pixels of one frame -> (gx, gz) as float64 absolute cells, label, q (int64; meaningful for label 1)."""
    P = np.asarray(pose, np.float64).reshape(12)
    s = np.asarray(disp).astype(np.int64)
    l = np.asarray(planes).astype(np.int64)
    h, w = s.shape
    y, x = np.mgrid[0:h, 0:w]
    ok = ((l == 0) | (l == 1)) & (s != INVALID)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = s.astype(np.float64) / 16.0
        ok &= d >= p["min_disparity"]
        Z = (np.float64(cam["fx"]) * np.float64(cam["baseline"])) / d
        ok &= Z <= p["max_depth"]
        X = ((x.astype(np.float64) - cam["cx"]) * Z) / cam["fx"]
        ok &= (X >= -p["max_lateral"]) & (X <= p["max_lateral"])
        Y = ((y.astype(np.float64) - cam["cy"]) * Z) / cam["fy"]
        X, Y, Z, l = X[ok], Y[ok], Z[ok], l[ok]
        pw = [((P[4 * r] * X + P[4 * r + 1] * Y) + P[4 * r + 2] * Z) + P[4 * r + 3] for r in range(3)]
        gx, gz = np.floor(pw[0] / p["cell_size"]), np.floor(pw[2] / p["cell_size"])
        q = np.clip(np.floor(pw[1] / p["height_quantum"]), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    return gx, gz, l, q


class Map:
    """cart_plane_map restated: cells in window order [nz, nx], origin (ox, oz) or None before the first update."""

    def __init__(self, cam, nx, nz, p=None):
        self.cam, self.nx, self.nz, self.p = cam, int(nx), int(nz), p if p is not None else params()
        self.clear()

    def clear(self):
        self.origin = None
        self.cells = empty_cells(self.nz, self.nx)

    def update(self, disp, planes, pose):
        P = np.asarray(pose, np.float64).reshape(12)
        ox, oz = window_origin(P[3], self.p["cell_size"], self.nx), window_origin(P[11], self.p["cell_size"], self.nz)
        fresh = empty_cells(self.nz, self.nx)
        if self.origin is not None:   # copy the overlap of the old window; everything else stays empty
            pox, poz = self.origin
            x0, x1 = max(ox, pox), min(ox + self.nx, pox + self.nx)
            z0, z1 = max(oz, poz), min(oz + self.nz, poz + self.nz)
            if x0 < x1 and z0 < z1:
                fresh[z0 - oz:z1 - oz, x0 - ox:x1 - ox] = self.cells[z0 - poz:z1 - poz, x0 - pox:x1 - pox]
        self.cells, self.origin = fresh, (ox, oz)
        gx, gz, l, q = votes(self.cam, self.p, P, disp, planes)
        inside = (gx >= ox) & (gx < ox + self.nx) & (gz >= oz) & (gz < oz + self.nz)
        cx, cz = (gx[inside] - ox).astype(np.int64), (gz[inside] - oz).astype(np.int64)
        l, q = l[inside], q[inside]
        hcount, vcount = np.zeros((self.nz, self.nx), np.int64), np.zeros((self.nz, self.nx), np.int64)
        np.add.at(hcount, (cz[l == 0], cx[l == 0]), 1)
        np.add.at(vcount, (cz[l == 1], cx[l == 1]), 1)
        lo, hi = self.cells["y_min"].astype(np.int64), self.cells["y_max"].astype(np.int64)
        np.minimum.at(lo, (cz[l == 1], cx[l == 1]), q[l == 1])
        np.maximum.at(hi, (cz[l == 1], cx[l == 1]), q[l == 1])
        self.cells["horizontal"] = ((self.cells["horizontal"].astype(np.int64) + hcount) & 0xFFFFFFFF).astype(np.uint32)
        self.cells["vertical"] = ((self.cells["vertical"].astype(np.int64) + vcount) & 0xFFFFFFFF).astype(np.uint32)
        self.cells["y_min"], self.cells["y_max"] = lo.astype(np.int32), hi.astype(np.int32)
        return self.origin

    def read(self):
        return self.cells.copy(), (self.origin if self.origin is not None else (0, 0))

    def classify(self, min_votes=3, obstacle_percent=50):
        return classify(self.cells, min_votes, obstacle_percent)


def classify(cells, min_votes, obstacle_percent):
    """u8 [nz, nx]: 2 where n = h + v < min_votes, else 1 where 100 v >= percent n, else 0 (Python-width integers via uint64: n < 2^33)."""
    h, v = cells["horizontal"].astype(np.uint64), cells["vertical"].astype(np.uint64)
    n = h + v
    out = np.where(v * np.uint64(100) >= np.uint64(obstacle_percent) * n, 1, 0).astype(np.uint8)
    out[n < np.uint64(min_votes)] = 2
    return out

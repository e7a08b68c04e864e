"""numpy restatement of spec S33: the rolling TSDF voxel map and its model raycast.  Written from the spec, not from
the kernels: whole-volume / whole-image array arithmetic in the spec's operation order (every numpy ufunc rounds once, there is no fused
multiply-add), Python integers for the window, int64 for the running average.  The volume is kept in window order [nz, ny, nx]; a window
move copies the overlap of the old window into a fresh empty array (the device stores toroidally and copies nothing: equality is on the
window-order contents)."""
import numpy as np

VOXEL_DTYPE = np.dtype([("tsdf", "<i2"), ("weight", "<u2")])
INVALID = -32768
NONE, HIT, INSIDE = 0, 1, 2
MOVING = 1
# build-owned, untuned
DEFAULTS = dict(voxel_size=0.125, min_disparity=1.0, min_depth=0.5, max_depth=16.0, truncation=0.25, disparity_sigma=0.5, lookahead=8.0,
                march_step=0.125, max_weight=64, min_weight=1)
POSE_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise ValueError(k)
        p[k] = int(v) if k in ("max_weight", "min_weight") else float(v)
    return p


def camera(fx, fy, cx, cy, baseline):
    return dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), baseline=float(baseline))


def window_origin(pose, p, shape):
    """o_a = 8 floor_div(floor((t_a + lookahead P[4a + 2]) / voxel_size) - N_a / 2, 8) in Python integers; shape = (nx, ny, nz)."""
    P = np.asarray(pose, np.float64).reshape(12)
    out = []
    for a, n in enumerate(shape):
        c = int(np.floor((P[4 * a + 3] + np.float64(p["lookahead"]) * P[4 * a + 2]) / np.float64(p["voxel_size"])))
        out.append(8 * ((c - n // 2) // 8))
    return tuple(out)


def march_steps(p):
    return int(np.floor((np.float64(p["max_depth"]) - np.float64(p["min_depth"])) / np.float64(p["march_step"])))


class Map:
    """cart_voxel_map restated: voxels in window order [nz, ny, nx], origin (ox, oy, oz) or None before the first integrate."""

    def __init__(self, nx, ny, nz, p=None):
        self.nx, self.ny, self.nz, self.p = int(nx), int(ny), int(nz), p if p is not None else params()
        self.clear()

    def clear(self):
        self.origin = None
        self.tsdf = np.zeros((self.nz, self.ny, self.nx), np.int64)
        self.weight = np.zeros((self.nz, self.ny, self.nx), np.int64)

    def read(self):
        v = np.zeros((self.nz, self.ny, self.nx), VOXEL_DTYPE)
        v["tsdf"], v["weight"] = self.tsdf, self.weight
        return v, (self.origin if self.origin is not None else (0, 0, 0))

    def _move(self, o):
        t, w = np.zeros_like(self.tsdf), np.zeros_like(self.weight)
        if self.origin is not None:
            lo = [max(o[a], self.origin[a]) for a in range(3)]
            hi = [min(o[a] + n, self.origin[a] + n) for a, n in enumerate((self.nx, self.ny, self.nz))]
            if all(lo[a] < hi[a] for a in range(3)):
                new = tuple(slice(lo[a] - o[a], hi[a] - o[a]) for a in (2, 1, 0))
                old = tuple(slice(lo[a] - self.origin[a], hi[a] - self.origin[a]) for a in (2, 1, 0))
                t[new], w[new] = self.tsdf[old], self.weight[old]
        self.tsdf, self.weight, self.origin = t, w, tuple(o)

    def integrate(self, cam, pose, disp, mask=None):
        """One frame.  -> counts int32 [2]: voxels updated, of them with f < 1."""
        p = self.p
        P = np.asarray(pose, np.float64).reshape(12)
        s_img = np.asarray(disp).astype(np.int64)
        h, w = s_img.shape
        self._move(window_origin(P, p, (self.nx, self.ny, self.nz)))
        ox, oy, oz = self.origin
        fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        fxb = fx * np.float64(cam["baseline"])
        vs = np.float64(p["voxel_size"])
        gz, gy, gx = np.meshgrid(np.arange(oz, oz + self.nz, dtype=np.float64), np.arange(oy, oy + self.ny, dtype=np.float64),
                                 np.arange(ox, ox + self.nx, dtype=np.float64), indexing="ij")
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            d0, d1, d2 = (gx + 0.5) * vs - P[3], (gy + 0.5) * vs - P[7], (gz + 0.5) * vs - P[11]
            q = [(P[c] * d0 + P[4 + c] * d1) + P[8 + c] * d2 for c in range(3)]
            ok = q[2] >= p["min_depth"]
            u = (fx * q[0]) / q[2] + cx
            v = (fy * q[1]) / q[2] + cy
            xd, yd = np.floor(u + 0.5), np.floor(v + 0.5)
            ok &= (xd >= 0.0) & (xd <= float(w - 1)) & (yd >= 0.0) & (yd <= float(h - 1))        # a NaN fails
            x, y = np.where(ok, xd, 0.0).astype(np.int64), np.where(ok, yd, 0.0).astype(np.int64)
            s = s_img[y, x]
            ok &= s != INVALID
            d = s.astype(np.float64) / 16.0
            ok &= d >= p["min_disparity"]
            Z = fxb / d
            ok &= Z <= p["max_depth"]
            if mask is not None:
                ok &= np.asarray(mask)[y, x] != MOVING
            tr = np.float64(p["truncation"]) + np.float64(p["disparity_sigma"]) * ((Z * Z) / fxb)
            sdf = Z - q[2]
            ok &= sdf >= -tr
            f = sdf / tr
            near = ok & (f < 1.0)
            f = np.where(f > 1.0, 1.0, f)
            obs = np.where(ok, np.floor(f * 32767.0 + 0.5), 0.0).astype(np.int64)
        t, wt = self.tsdf, self.weight
        tn = (2 * (wt * t + obs) + (wt + 1)) // (2 * (wt + 1))                                  # numpy's // is floor division
        self.tsdf = np.where(ok, tn, t)
        self.weight = np.where(ok, np.minimum(wt + 1, p["max_weight"]), wt)
        return np.array([ok.sum(), near.sum()], np.int32)

    def raycast(self, cam, pose, width, height):
        """-> dict(disp int16 [h, w], weight uint16, status uint8, counts int32 [3] = NONE, HIT, INSIDE).  Reads the volume only."""
        p = self.p
        P = np.asarray(pose, np.float64).reshape(12)
        h, w = int(height), int(width)
        fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        fxb = fx * np.float64(cam["baseline"])
        vs, step = np.float64(p["voxel_size"]), np.float64(p["march_step"])
        y, x = np.mgrid[0:h, 0:w]
        xf, yf = x.astype(np.float64), y.astype(np.float64)
        disp = np.full((h, w), INVALID, np.int16)
        weight = np.zeros((h, w), np.uint16)
        status = np.zeros((h, w), np.uint8)
        if self.origin is not None:
            o = [float(v) for v in self.origin]
            n = (self.nx, self.ny, self.nz)
            live = np.ones((h, w), bool)
            have_prev = np.zeros((h, w), bool)
            Fp, zp = np.zeros((h, w)), np.zeros((h, w))
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                for k in range(march_steps(p) + 1):
                    if not live.any():
                        break
                    z = np.float64(p["min_depth"]) + np.float64(k) * step
                    X, Y = ((xf - cx) * z) / fx, ((yf - cy) * z) / fy
                    pw = [((P[4 * r] * X + P[4 * r + 1] * Y) + P[4 * r + 2] * z) + P[4 * r + 3] for r in range(3)]
                    a = [c / vs - 0.5 for c in pw]
                    i0 = [np.floor(c) for c in a]
                    fr = [a[c] - i0[c] for c in range(3)]
                    known = live.copy()
                    for c in range(3):
                        known &= (i0[c] >= o[c]) & (i0[c] <= o[c] + float(n[c] - 2))              # both corners inside; a NaN fails
                    r = [np.where(known, i0[c] - o[c], 0.0).astype(np.int64) for c in range(3)]
                    T = {(dz, dy, dx): self.tsdf[r[2] + dz, r[1] + dy, r[0] + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
                    wmin = np.full((h, w), 65535, np.int64)
                    for key in T:
                        wmin = np.minimum(wmin, self.weight[r[2] + key[0], r[1] + key[1], r[0] + key[2]])
                    known &= wmin >= p["min_weight"]
                    cc = {(dy, dz): T[(dz, dy, 0)].astype(np.float64) + fr[0] * (T[(dz, dy, 1)] - T[(dz, dy, 0)]).astype(np.float64) for dy in (0, 1) for dz in (0, 1)}
                    e0 = cc[(0, 0)] + fr[1] * (cc[(1, 0)] - cc[(0, 0)])
                    e1 = cc[(0, 1)] + fr[1] * (cc[(1, 1)] - cc[(0, 1)])
                    F = e0 + fr[2] * (e1 - e0)
                    neg = known & (F <= 0.0)
                    hit = neg & have_prev                                                       # F_p > 0 by construction
                    zs = zp + (step * Fp) / (Fp - F)
                    swd = np.floor((fxb / zs) * 16.0 + 0.5)
                    good = hit & (swd >= 1.0) & (swd <= 32767.0)
                    disp[good] = swd[good].astype(np.int16)
                    weight[good] = wmin[good].astype(np.uint16)
                    status[good] = HIT
                    status[neg & ~have_prev] = INSIDE
                    live &= ~neg
                    pos = known & (F > 0.0)
                    have_prev = pos                                                             # an unknown sample forgets the previous one
                    Fp, zp = np.where(pos, F, Fp), np.where(pos, z, zp)
        counts = np.array([(status == k).sum() for k in (NONE, HIT, INSIDE)], np.int32)
        return dict(disp=disp, weight=weight, status=status, counts=counts)

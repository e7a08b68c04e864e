"""numpy restatement of spec S37: colour for the TSDF voxel map.  Written from the spec, not from the kernels: whole-volume /
whole-image array arithmetic in the spec's operation order (every numpy ufunc rounds once, there is no fused multiply-add), int64 for the
running averages and the sample sums.  `Color` wraps an np_voxelmap.Map for the origin and the parameters; the colour volume is kept in
window order [nz, ny, nx] and a window move copies the overlap into a fresh empty array, as np_voxelmap does.  Every operation exists twice:
vectorised, and as a scalar loop in Python floats and integers (`*_scalar`), which tests/test_voxelcolor_spec.py holds against each other."""
import math

import numpy as np

import np_voxelmap as V

VOXEL_RGB_DTYPE = np.dtype([("b", "u1"), ("g", "u1"), ("r", "u1"), ("weight", "u1")])
CHANNELS = ("b", "g", "r")
INVALID = V.INVALID
MOVING = V.MOVING
DEFAULT_MAX_WEIGHT = 64   # build-owned, untuned


def bgr_of(image):
    """uint8 [h, w] or [h, w, 3] -> int64 [h, w, 3]: b = g = r for one channel."""
    im = np.asarray(image)
    assert im.dtype == np.uint8 and (im.ndim == 2 or (im.ndim == 3 and im.shape[2] == 3))
    return (np.repeat(im[:, :, None], 3, axis=2) if im.ndim == 2 else im).astype(np.int64)


class Color:
    """cart_voxel_color restated: c = int64 [nz, ny, nx, 3] (b, g, r) and weight = int64 [nz, ny, nx] in window order, origin (ox, oy, oz) or
    None before the first integrate / write."""

    def __init__(self, vmap, max_weight=DEFAULT_MAX_WEIGHT):
        assert 1 <= int(max_weight) <= 255
        self.map, self.max_weight = vmap, int(max_weight)
        self.nx, self.ny, self.nz, self.p = vmap.nx, vmap.ny, vmap.nz, vmap.p
        self.clear()

    def clear(self):
        self.origin = None
        self.c = np.zeros((self.nz, self.ny, self.nx, 3), np.int64)
        self.weight = np.zeros((self.nz, self.ny, self.nx), np.int64)

    def read(self):
        v = np.zeros((self.nz, self.ny, self.nx), VOXEL_RGB_DTYPE)
        for k, name in enumerate(CHANNELS):
            v[name] = self.c[..., k]
        v["weight"] = self.weight
        return v, (self.origin if self.origin is not None else (0, 0, 0))

    def write(self, voxels, origin):
        v = np.asarray(voxels, VOXEL_RGB_DTYPE).reshape(self.nz, self.ny, self.nx)
        self.c = np.stack([v[name].astype(np.int64) for name in CHANNELS], axis=3)
        self.weight = v["weight"].astype(np.int64)
        self.origin = tuple(int(o) for o in origin)

    def _move(self, o):
        """S33's move rule on the colour volume: the overlap of the old and the new window stays, everything else is empty."""
        c, w = np.zeros_like(self.c), np.zeros_like(self.weight)
        if self.origin is not None:
            lo = [max(o[a], self.origin[a]) for a in range(3)]
            hi = [min(o[a] + n, self.origin[a] + n) for a, n in enumerate((self.nx, self.ny, self.nz))]
            if all(lo[a] < hi[a] for a in range(3)):
                new = tuple(slice(lo[a] - o[a], hi[a] - o[a]) for a in (2, 1, 0))
                old = tuple(slice(lo[a] - self.origin[a], hi[a] - self.origin[a]) for a in (2, 1, 0))
                c[new], w[new] = self.c[old], self.weight[old]
        self.c, self.weight, self.origin = c, w, tuple(o)

    def _follow(self):
        if self.map.origin is None:
            raise ValueError("the map has no window")
        self._move(self.map.origin)

    # ---- integrate ----------------------------------------------------------------------------------------------------------------
    def passing(self, cam, pose, disp, mask=None):
        """Gates 1 - 5 of S33 and f < 1 at the colour window -> (ok bool [nz, ny, nx], x, y int64: the pixel, 0 where not ok)."""
        p = self.p
        P = np.asarray(pose, np.float64).reshape(12)
        s_img = np.asarray(disp).astype(np.int64)
        h, w = s_img.shape
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
            ok &= f < 1.0                                                                      # the unclamped f
        return ok, np.where(ok, x, 0), np.where(ok, y, 0)

    def integrate(self, cam, pose, disp, image, mask=None):
        """One frame, after the map's integrate of it.  -> counts int32 [2]: voxels coloured, of them with w = 0 before."""
        self._follow()
        ok, x, y = self.passing(cam, pose, disp, mask)
        obs = bgr_of(image)[y, x]                                                              # [nz, ny, nx, 3]
        w = self.weight
        cn = (2 * (w[..., None] * self.c + obs) + (w[..., None] + 1)) // (2 * (w[..., None] + 1))
        fresh = ok & (w == 0)
        self.c = np.where(ok[..., None], cn, self.c)
        self.weight = np.where(ok, np.minimum(w + 1, self.max_weight), w)
        return np.array([ok.sum(), fresh.sum()], np.int32)

    def integrate_scalar(self, cam, pose, disp, image, mask=None):
        """The same, voxel by voxel in Python floats and integers."""
        self._follow()
        p = self.p
        P = [float(v) for v in np.asarray(pose, np.float64).reshape(12)]
        s_img, im = np.asarray(disp), np.asarray(image)
        h, w = s_img.shape
        ox, oy, oz = self.origin
        fx, fy, cx, cy, bl = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
        fxb = fx * bl
        vs = float(p["voxel_size"])
        coloured = fresh = 0
        for rz in range(self.nz):
            for ry in range(self.ny):
                for rx in range(self.nx):
                    d0, d1, d2 = (float(ox + rx) + 0.5) * vs - P[3], (float(oy + ry) + 0.5) * vs - P[7], (float(oz + rz) + 0.5) * vs - P[11]
                    qx = (P[0] * d0 + P[4] * d1) + P[8] * d2
                    qy = (P[1] * d0 + P[5] * d1) + P[9] * d2
                    qz = (P[2] * d0 + P[6] * d1) + P[10] * d2
                    if not qz >= p["min_depth"]:
                        continue
                    xd, yd = math.floor((fx * qx) / qz + cx + 0.5), math.floor((fy * qy) / qz + cy + 0.5)
                    if not (0 <= xd <= w - 1 and 0 <= yd <= h - 1):
                        continue
                    s = int(s_img[yd, xd])
                    if s == INVALID:
                        continue
                    d = float(s) / 16.0
                    if not d >= p["min_disparity"]:
                        continue
                    Z = fxb / d
                    if not Z <= p["max_depth"] or (mask is not None and int(mask[yd, xd]) == MOVING):
                        continue
                    tr = float(p["truncation"]) + float(p["disparity_sigma"]) * ((Z * Z) / fxb)
                    sdf = Z - qz
                    if not sdf >= -tr or not sdf / tr < 1.0:
                        continue
                    wt = int(self.weight[rz, ry, rx])
                    for k in range(3):
                        obs = int(im[yd, xd]) if im.ndim == 2 else int(im[yd, xd, k])
                        self.c[rz, ry, rx, k] = (2 * (wt * int(self.c[rz, ry, rx, k]) + obs) + (wt + 1)) // (2 * (wt + 1))
                    self.weight[rz, ry, rx] = min(wt + 1, self.max_weight)
                    coloured, fresh = coloured + 1, fresh + (wt == 0)
        return np.array([coloured, fresh], np.int32)

    # ---- the sample rule ------------------------------------------------------------------------------------------------------------
    def sample(self, ix, iy, iz):
        """ix, iy, iz = float64 arrays of one shape: the absolute index of the lowest of the eight corners.  -> VOXEL_RGB_DTYPE array of
        that shape, the weight field holding alpha."""
        ix, iy, iz = (np.asarray(v, np.float64) for v in (ix, iy, iz))
        out = np.zeros(ix.shape, VOXEL_RGB_DTYPE)
        if self.origin is None:
            return out
        i0 = (ix, iy, iz)
        n = (self.nx, self.ny, self.nz)
        inside = np.ones(ix.shape, bool)
        with np.errstate(invalid="ignore"):
            for a in range(3):
                inside &= (i0[a] >= float(self.origin[a])) & (i0[a] <= float(self.origin[a]) + float(n[a] - 2))   # both corners inside; a NaN fails
            r = [np.where(inside, i0[a] - float(self.origin[a]), 0.0).astype(np.int64) for a in range(3)]
        W = np.zeros(ix.shape, np.int64)
        S = np.zeros(ix.shape + (3,), np.int64)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    wk = self.weight[r[2] + dz, r[1] + dy, r[0] + dx]
                    W += wk
                    S += wk[..., None] * self.c[r[2] + dz, r[1] + dy, r[0] + dx]
        good = inside & (W > 0)
        den = np.where(good, 2 * W, 1)
        for k, name in enumerate(CHANNELS):
            out[name] = np.where(good, (2 * S[..., k] + W) // den, 0)
        out["weight"] = np.where(good, np.minimum(W, 255), 0)
        return out

    def sample_scalar(self, ix, iy, iz):
        """One sample in Python numbers -> (b, g, r, alpha)."""
        if self.origin is None:
            return (0, 0, 0, 0)
        i0, n = (float(ix), float(iy), float(iz)), (self.nx, self.ny, self.nz)
        for a in range(3):
            if not (i0[a] >= float(self.origin[a]) and i0[a] <= float(self.origin[a]) + float(n[a] - 2)):
                return (0, 0, 0, 0)
        r = [int(i0[a] - float(self.origin[a])) for a in range(3)]
        W, S = 0, [0, 0, 0]
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    wk = int(self.weight[r[2] + dz, r[1] + dy, r[0] + dx])
                    W += wk
                    for k in range(3):
                        S[k] += wk * int(self.c[r[2] + dz, r[1] + dy, r[0] + dx, k])
        if W == 0:
            return (0, 0, 0, 0)
        return tuple((2 * S[k] + W) // (2 * W) for k in range(3)) + (min(W, 255),)

    # ---- the two read-outs --------------------------------------------------------------------------------------------------------------
    def colorize(self, vertices, origin, n=None, max_vertices=None):
        """vertices = MESH_VERTEX_DTYPE records with their mesh origin; the first min(n, max_vertices) are coloured (default: all).
        -> VOXEL_RGB_DTYPE [that count]."""
        v = np.asarray(vertices).reshape(-1)
        count = len(v) if n is None else max(0, min(int(n), len(v) if max_vertices is None else int(max_vertices)))
        vs = np.float64(self.p["voxel_size"])
        pos = v["position"][:count].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            i0 = [np.float64(int(origin[a])) + np.floor(pos[:, a] / vs - 0.5) for a in range(3)]
        return self.sample(*i0)

    def colorize_scalar(self, vertices, origin):
        v = np.asarray(vertices).reshape(-1)
        vs = float(self.p["voxel_size"])
        out = np.zeros(len(v), VOXEL_RGB_DTYPE)
        for k in range(len(v)):
            i0 = [float(int(origin[a])) + math.floor(float(v["position"][k][a]) / vs - 0.5) for a in range(3)]
            out[k] = self.sample_scalar(*i0)
        return out

    def render(self, cam, pose, disp):
        """-> dict(image uint8 [h, w, 3], alpha uint8 [h, w], counts int32 [1] = pixels with alpha > 0).  Reads the volume only."""
        P = np.asarray(pose, np.float64).reshape(12)
        s = np.asarray(disp).astype(np.int64)
        h, w = s.shape
        fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        fxb = fx * np.float64(cam["baseline"])
        vs = np.float64(self.p["voxel_size"])
        y, x = np.mgrid[0:h, 0:w]
        ok = (s != INVALID) & (s >= 1)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            d = np.where(ok, s, 16).astype(np.float64) / 16.0
            Z = fxb / d
            X, Y = ((x.astype(np.float64) - cx) * Z) / fx, ((y.astype(np.float64) - cy) * Z) / fy
            pw = [((P[4 * r] * X + P[4 * r + 1] * Y) + P[4 * r + 2] * Z) + P[4 * r + 3] for r in range(3)]
            i0 = [np.floor(c / vs - 0.5) for c in pw]
        c = self.sample(*i0)
        image = np.zeros((h, w, 3), np.uint8)
        for k, name in enumerate(CHANNELS):
            image[..., k] = np.where(ok, c[name], 0)
        alpha = np.where(ok, c["weight"], 0).astype(np.uint8)
        return dict(image=image, alpha=alpha, counts=np.array([(alpha > 0).sum()], np.int32))

    def render_scalar(self, cam, pose, disp):
        P = [float(v) for v in np.asarray(pose, np.float64).reshape(12)]
        s_img = np.asarray(disp)
        h, w = s_img.shape
        fx, fy, cx, cy, bl = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
        vs = float(self.p["voxel_size"])
        image, alpha = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8)
        for y in range(h):
            for x in range(w):
                s = int(s_img[y, x])
                if s == INVALID or s < 1:
                    continue
                Z = (fx * bl) / (float(s) / 16.0)
                X, Y = ((float(x) - cx) * Z) / fx, ((float(y) - cy) * Z) / fy
                pw = [((P[4 * r] * X + P[4 * r + 1] * Y) + P[4 * r + 2] * Z) + P[4 * r + 3] for r in range(3)]
                b, g, r, al = self.sample_scalar(*[math.floor(c / vs - 0.5) for c in pw])
                image[y, x], alpha[y, x] = (b, g, r), al
        return dict(image=image, alpha=alpha, counts=np.array([(alpha > 0).sum()], np.int32))

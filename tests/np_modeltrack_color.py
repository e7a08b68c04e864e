"""numpy restatement of spec S38: colour-aided frame-to-model tracking, S34's geometric term plus a photometric term read
from the colour companion of the volume (S37).  Written from the spec on top of np_modeltrack (the pixel gates, the eight-corner sample
with its gradient, the solve), np_voxelcolor.Color (the colour volume) and np_dense_ego's two-level lane order, extended to 29 sums and to
two additions per pixel: a lane adds a pixel's geometric terms, then its photometric terms, then goes on to its next column.
scalar_pixel() and scalar_evaluate() are the same spec one pixel at a time in Python floats for cross-checking the vectorised form."""
import math

import numpy as np

import np_modeltrack as T
from np_dense_ego import LANES, _scalar_butterfly, butterfly, join, rms_of, split  # noqa: F401
from np_ego import apply_update, solve6

INVALID = T.INVALID
NSUMS = 29                   # S34's 28, then the sum of rc rc
# build-owned, untuned
DEFAULTS = dict(photo_weight=64.0, photo_gate=0.25, color_min_weight=1)
RESULT_DTYPE = np.dtype(T.RESULT_DTYPE.descr + [("rms_photo_initial", "<f8"), ("rms_photo", "<f8"), ("cost_initial", "<f8"), ("cost", "<f8"),
                                                ("n_photo_initial", "<i4"), ("n_photo", "<i4")])   # cart_model_track_color_result, 176 bytes


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise ValueError(k)
        p[k] = int(v) if k == "color_min_weight" else float(v)
    return p


class Luminance:
    """The colour object seen as np_modeltrack.sample sees a Map: `tsdf` holds t = b + 2 g + r of every voxel (0 .. 1020), `weight` the
    colour weight, under the colour object's own grid and origin, with min_weight = color_min_weight."""

    def __init__(self, color, cp):
        self.origin = color.origin
        self.nx, self.ny, self.nz = color.nx, color.ny, color.nz
        self.tsdf = color.c[..., 0] + 2 * color.c[..., 1] + color.c[..., 2]
        self.weight = color.weight
        self.p = dict(voxel_size=color.p["voxel_size"], min_weight=cp["color_min_weight"])


def observed(image):
    """uint8 [h, w] or [h, w, 3] (B, G, R) -> int64 [h, w]: L_obs = b + 2 g + r."""
    im = np.asarray(image)
    assert im.dtype == np.uint8 and (im.ndim == 2 or (im.ndim == 3 and im.shape[2] == 3))
    im = im.astype(np.int64)
    return 4 * im if im.ndim == 2 else im[..., 0] + 2 * im[..., 1] + im[..., 2]


# ---- one pixel's terms at a pose ----------------------------------------------------------------------------------------------
def terms(m, color, cam, p, cp, R, t, disp, image, mask=None):
    """-> (candidate, geometric inlier, photometric inlier [nj, ni] bool, geometric values [28, nj, ni], photometric values [29, nj, ni]:
    entry 27 of the photometric values is unused, entry 28 is rc rc)."""
    cand, inl, vals = T.terms(m, cam, p, R, t, disp, mask)
    pin = np.zeros(inl.shape, bool)
    cvals = np.zeros((NSUMS,) + inl.shape)
    lam = np.float64(cp["photo_weight"])
    if not lam > 0.0:
        return cand, inl, pin, vals, cvals
    s = p["stride"]
    s_full = np.asarray(disp).astype(np.int64)
    h, w = s_full.shape
    y, x = np.mgrid[0:h:s, 0:w:s]
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    fxb = fx * np.float64(cam["baseline"])
    with np.errstate(all="ignore"):
        Z = fxb / (s_full[y, x].astype(np.float64) / 16.0)
        X = ((x.astype(np.float64) - cx) * Z) / fx
        Y = ((y.astype(np.float64) - cy) * Z) / fy
        pw = [((R[3 * r] * X + R[3 * r + 1] * Y) + R[3 * r + 2] * Z) + t[r] for r in range(3)]
        known, Cv, gx, gy, gz = T.sample(Luminance(color, cp), pw, inl)
        rc = (Cv - observed(image)[y, x].astype(np.float64)) / 1020.0
        pin = known & (np.abs(rc) < cp["photo_gate"])
        gs = np.float64(1020.0) * np.float64(m.p["voxel_size"])
        G = [gx / gs, gy / gs, gz / gs]
        J = [pw[1] * G[2] - pw[2] * G[1], pw[2] * G[0] - pw[0] * G[2], pw[0] * G[1] - pw[1] * G[0], G[0], G[1], G[2]]
        out = [(lam * J[i]) * J[j] for i in range(6) for j in range(i, 6)]
        out += [(lam * J[i]) * rc for i in range(6)]
        out += [np.zeros(inl.shape), rc * rc]
    return cand, inl, pin, vals, np.stack([np.broadcast_to(v, inl.shape) for v in out])


def lane_sums2(gv, gok, cv, cok):
    """The row level: lane l walks its columns l, l + 256, ... in ascending order and adds, per column, the geometric terms of an inlier to
    sums 0 .. 27 and then the photometric terms of a photometric inlier to sums 0 .. 26 and 28; then the butterfly.  -> [NSUMS, nj]."""
    nj, ni = gok.shape
    v = np.zeros((NSUMS, nj, LANES), np.float64)
    with np.errstate(all="ignore"):
        for c0 in range(0, ni, LANES):
            mg, mc = gok[:, c0:c0 + LANES], cok[:, c0:c0 + LANES]
            k = mg.shape[-1]
            v[:28, :, :k] = np.where(mg, v[:28, :, :k] + np.where(mg, gv[:, :, c0:c0 + LANES], 0.0), v[:28, :, :k])
            for sl in (slice(0, 27), slice(28, 29)):
                v[sl, :, :k] = np.where(mc, v[sl, :, :k] + np.where(mc, cv[sl, :, c0:c0 + LANES], 0.0), v[sl, :, :k])
    return butterfly(v)


def image_level(rows):
    """rows [NSUMS, nj] -> [NSUMS]: lane l adds the partials of rows l, l + 256, ... in ascending order, then the butterfly."""
    nj = rows.shape[-1]
    v = np.zeros((rows.shape[0], LANES), np.float64)
    with np.errstate(all="ignore"):
        for c0 in range(0, nj, LANES):
            k = min(LANES, nj - c0)
            v[:, :k] = v[:, :k] + rows[:, c0:c0 + k]
    return butterfly(v)


def evaluate(m, color, cam, p, cp, R, t, disp, image, mask=None):
    """-> (inliers, candidates, photometric inliers, the NSUMS sums as Python floats) at the pose (R, t)."""
    cand, inl, pin, gv, cv = terms(m, color, cam, p, cp, R, t, disp, image, mask)
    s = [float(v) for v in image_level(lane_sums2(gv, inl, cv, pin))]
    return int(inl.sum()), int(cand.sum()), int(pin.sum()), s


def cost_of(e2, n, e2c, nphoto, lam):
    den = float(n) + lam * float(nphoto)
    return math.sqrt((e2 + lam * e2c) / den) if den != 0.0 else 0.0


# ---- the whole call -----------------------------------------------------------------------------------------------------------
def refine(m, color, cam, p, cp, pose0, disp, image, mask=None, evaluate=evaluate):
    """cart_model_track_refine_color restated -> RESULT_DTYPE [1].  The state machine is S34's: iterations + 1 evaluations, of which the
    last one at a pose gives the final counts and errors."""
    R, t = split(pose0)
    lam = float(cp["photo_weight"])
    res = np.zeros(1, RESULT_DTYPE)
    steps = 0
    for ev in range(p["iterations"] + 1):
        n, nc, nph, s = evaluate(m, color, cam, p, cp, R, t, disp, image, mask)
        if ev == 0:
            res["n_initial"], res["rms_initial"] = n, rms_of(s[27], n)
            res["n_photo_initial"], res["rms_photo_initial"], res["cost_initial"] = nph, rms_of(s[28], nph), cost_of(s[27], n, s[28], nph, lam)
        if ev == p["iterations"] or n < p["min_inliers"]:
            break
        H = [[0.0] * 6 for _ in range(6)]
        k = 0
        for i in range(6):
            for j in range(i, 6):
                H[i][j] = s[k]
                k += 1
        for i in range(6):
            H[i][i] = H[i][i] + p["damping"] * float(n)
        delta = solve6(H, s[21:27])
        if delta is None:
            break
        R, t = apply_update(R, t, delta)
        steps += 1
    res["R"][0], res["t"][0] = R, t
    res["n_candidates"], res["n_inliers"], res["rms"], res["steps"], res["status"] = nc, n, rms_of(s[27], n), steps, 1 if steps > 0 else 0
    res["n_photo"], res["rms_photo"], res["cost"] = nph, rms_of(s[28], nph), cost_of(s[27], n, s[28], nph, lam)
    return res


def accept(res, pose0, p):
    """The consumer's rule -> (taken, the 12 doubles of the pose to use): the refined one iff status == 1, every number of the record is
    finite, cost <= cost_initial and n_inliers >= min_inliers; otherwise pose0."""
    r = res.reshape(-1)[0]
    pose = join([float(v) for v in r["R"]], [float(v) for v in r["t"]])
    nums = pose + [float(r[k]) for k in ("rms_initial", "rms", "rms_photo_initial", "rms_photo", "cost_initial", "cost")]
    if int(r["status"]) == 1 and all(math.isfinite(v) for v in nums) and float(r["cost"]) <= float(r["cost_initial"]) and int(r["n_inliers"]) >= p["min_inliers"]:
        return True, pose
    return False, [float(v) for v in np.asarray(pose0, np.float64).reshape(12)]


# ---- the same spec, one pixel at a time in Python floats ----------------------------------------------------------------------
def scalar_observed(image, x, y):
    px = image[y][x]
    return 4 * int(px) if np.ndim(px) == 0 else int(px[0]) + 2 * int(px[1]) + int(px[2])


def scalar_pixel(m, color, cam, p, cp, R, t, disp, image, mask, x, y):
    """-> None for a pixel that is no candidate, else (inlier, the 28 geometric values or None, the NSUMS photometric values or None)."""
    got = T.scalar_pixel(m, cam, p, R, t, disp, mask, x, y)
    if got is None or not got[0]:
        return None if got is None else (False, None, None)
    lam = float(cp["photo_weight"])
    if not lam > 0.0:
        return True, got[1], None
    fx, fy, cx, cy, base = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
    Z = (fx * base) / (int(disp[y][x]) / 16.0)
    X = ((float(x) - cx) * Z) / fx
    Y = ((float(y) - cy) * Z) / fy
    pw = [((R[3 * r] * X + R[3 * r + 1] * Y) + R[3 * r + 2] * Z) + t[r] for r in range(3)]
    smp = T.scalar_sample(Luminance(color, cp), *pw)
    if smp is None:
        return True, got[1], None
    Cv, gx, gy, gz = smp[:4]
    rc = (Cv - float(scalar_observed(image, x, y))) / 1020.0
    if not abs(rc) < cp["photo_gate"]:
        return True, got[1], None
    gs = 1020.0 * m.p["voxel_size"]
    G = [gx / gs, gy / gs, gz / gs]
    J = [pw[1] * G[2] - pw[2] * G[1], pw[2] * G[0] - pw[0] * G[2], pw[0] * G[1] - pw[1] * G[0], G[0], G[1], G[2]]
    vals = [(lam * J[i]) * J[j] for i in range(6) for j in range(i, 6)]
    vals += [(lam * J[i]) * rc for i in range(6)]
    vals += [0.0, rc * rc]
    return True, got[1], vals


def scalar_evaluate(m, color, cam, p, cp, R, t, disp, image, mask=None):
    """-> (inliers, candidates, photometric inliers, the NSUMS sums) by the two-level lane order, one pixel at a time."""
    h, w = np.asarray(disp).shape
    s = p["stride"]
    ni, nj = (w + s - 1) // s, (h + s - 1) // s
    count = ncand = nphoto = 0
    rows = []
    for j in range(nj):
        v = [[0.0] * LANES for _ in range(NSUMS)]
        for i in range(ni):
            got = scalar_pixel(m, color, cam, p, cp, R, t, disp, image, mask, i * s, j * s)
            if got is None:
                continue
            ncand += 1
            if not got[0]:
                continue
            count += 1
            for k in range(28):
                v[k][i % LANES] = v[k][i % LANES] + got[1][k]
            if got[2] is not None:
                nphoto += 1
                for k in list(range(27)) + [28]:
                    v[k][i % LANES] = v[k][i % LANES] + got[2][k]
        rows.append([_scalar_butterfly(v[k]) for k in range(NSUMS)])
    out = []
    for k in range(NSUMS):
        v = [0.0] * LANES
        for j in range(nj):
            v[j % LANES] = v[j % LANES] + rows[j][k]
        out.append(_scalar_butterfly(v))
    return count, ncand, nphoto, out

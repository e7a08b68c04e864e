"""numpy restatement of spec S26: dense Gauss-Newton refinement of the relative pose over all static pixels, from this
frame's disparity, the previous frame's and the flow between them.  Written from the spec, not from the kernels: whole-image array
arithmetic in the spec's operation order (every numpy ufunc rounds once, there is no fused multiply-add), every sum in the two-level
lane order written out (numpy's own `sum` is pairwise and is never used on floating point).  scalar_evaluate() is the same spec as a
pure-Python loop over pixels in Python floats for cross-checking the vectorised form.  The solve and the pose update are S23's."""
import math

import numpy as np

from np_ego import apply_update, solve6
from np_motion import INVALID, _div, camera  # noqa: F401  (camera: the same dict as S25's)

LANES = 256
MOVING = 1
NSUMS = 28                   # 21 upper entries of H (row-major, i <= j), the 6 of g, e2
DEFAULTS = dict(min_disparity=1.0, flow_threshold=2.0, disparity_threshold=1.0, disparity_weight=1.0, iterations=4, stride=1, min_inliers=1024)
RESULT_DTYPE = np.dtype([("R", "<f8", 9), ("t", "<f8", 3), ("rms_initial", "<f8"), ("rms", "<f8"), ("status", "<i4"), ("n_candidates", "<i4"),
                         ("n_initial", "<i4"), ("n_inliers", "<i4"), ("steps", "<i4"), ("reserved", "<i4")])   # cart_dense_ego_result, 136 bytes


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise ValueError(k)
        p[k] = int(v) if k in ("iterations", "stride", "min_inliers") else float(v)
    return p


def split(rel):
    """3 x 4 (R | t) in row order -> (R [9], t [3]) as Python floats."""
    r = [float(v) for v in np.asarray(rel, np.float64).reshape(12)]
    return [r[4 * i + c] for i in range(3) for c in range(3)], [r[3], r[7], r[11]]


def join(R, t):
    return [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]


# ---- the pose-independent part: the sample grid and gates 1-3 of S25 plus the mask -------------------------------------------
def candidates(cam, p, disp_cur, disp_prev, flow, mask=None):
    """-> dict of [nj, ni] arrays on the sample grid: x, y (float64), dc, xp, yp (float64), dp, cand (bool)."""
    s = p["stride"]
    sc_full = np.asarray(disp_cur).astype(np.int64)
    h, w = sc_full.shape
    y, x = np.mgrid[0:h:s, 0:w:s]
    sc = sc_full[y, x]
    fl = np.asarray(flow).astype(np.int64)[y, x]
    dc = sc.astype(np.float64) / 16.0
    cand = (sc != INVALID) & (dc >= p["min_disparity"])
    xp, yp = x - (fl[..., 0] >> 5), y - (fl[..., 1] >> 5)                   # numpy's >> on signed integers is arithmetic
    cand &= (xp >= 0) & (xp < w) & (yp >= 0) & (yp < h)
    sp = np.asarray(disp_prev).astype(np.int64)[np.clip(yp, 0, h - 1), np.clip(xp, 0, w - 1)]
    dp = sp.astype(np.float64) / 16.0
    cand &= (sp != INVALID) & (dp >= p["min_disparity"])
    if mask is not None:
        cand &= np.asarray(mask)[y, x] != MOVING
    return dict(x=x.astype(np.float64), y=y.astype(np.float64), dc=dc, xp=xp.astype(np.float64), yp=yp.astype(np.float64), dp=dp, cand=cand)


# ---- one pixel's terms at a pose ----------------------------------------------------------------------------------------------
def terms(cam, p, R, t, c):
    """-> (contributing [nj, ni] bool, values [NSUMS, nj, ni]); entries of pixels that do not contribute are meaningless."""
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    fxb = fx * np.float64(cam["baseline"])
    wd = np.float64(p["disparity_weight"])
    with np.errstate(all="ignore"):
        Zp = fxb / c["dp"]
        Xp = ((c["xp"] - cx) * Zp) / fx
        Yp = ((c["yp"] - cy) * Zp) / fy
        qx, qy, qz = (((R[3 * r] * Xp + R[3 * r + 1] * Yp) + R[3 * r + 2] * Zp) + t[r] for r in range(3))
        eu = ((fx * qx) / qz + cx) - c["x"]
        ev = ((fy * qy) / qz + cy) - c["y"]
        ed = fxb / qz - c["dc"]
        ef = eu * eu + ev * ev
        ok = c["cand"] & (qz > 0) & (ef < p["flow_threshold"] * p["flow_threshold"]) & (ed * ed < p["disparity_threshold"] * p["disparity_threshold"])
        a = fx / qz
        b = -((fx * qx) / (qz * qz))
        cc = fy / qz
        d = -((fy * qy) / (qz * qz))
        g = -(fxb / (qz * qz))
        zero = np.zeros_like(qz)
        Ju = [b * qy, a * qz - b * qx, -(a * qy), a, zero, b]
        Jv = [d * qy - cc * qz, -(d * qx), cc * qx, zero, cc, d]
        Jd = [g * qy, -(g * qx), zero, zero, zero, g]
        vals = [(Ju[i] * Ju[j] + Jv[i] * Jv[j]) + wd * (Jd[i] * Jd[j]) for i in range(6) for j in range(i, 6)]
        vals += [(Ju[i] * eu + Jv[i] * ev) + wd * (Jd[i] * ed) for i in range(6)]
        vals.append(ef + wd * (ed * ed))
    return ok, np.stack(vals)


# ---- the sums -----------------------------------------------------------------------------------------------------------------
def butterfly(v):
    """v[..., l] += v[..., l ^ o] for o = 1, 2, 4 .. 128 (ascending); lane 0's value."""
    lanes = np.arange(LANES)
    o = 1
    with np.errstate(all="ignore"):
        while o < LANES:
            v = v + v[..., lanes ^ o]
            o *= 2
    return v[..., 0]


def lane_sums(vals, ok):
    """vals [..., n], ok [..., n] -> [...]: lane l adds its entries l, l + 256, ... that are ok in ascending order, then the butterfly."""
    n = vals.shape[-1]
    v = np.zeros(vals.shape[:-1] + (LANES,), np.float64)
    with np.errstate(all="ignore"):
        for c0 in range(0, n, LANES):              # one round of all lanes at a time: element-wise, so the order per lane is kept
            m = ok[..., c0:c0 + LANES]
            k = m.shape[-1]
            v[..., :k] = np.where(m, v[..., :k] + np.where(m, vals[..., c0:c0 + LANES], 0.0), v[..., :k])
    return butterfly(v)


def two_level(vals, ok):
    """vals [NSUMS, nj, ni], ok [nj, ni] -> [NSUMS]: the row level, then the image level over the row partials (every row adds its partial)."""
    rows = lane_sums(vals, np.broadcast_to(ok, vals.shape))            # [NSUMS, nj]
    return lane_sums(rows, np.ones(rows.shape, bool))


def evaluate(cam, p, R, t, c):
    """-> (count, H 6 x 6 with the upper entries filled, g [6], sum of e2) at the pose (R, t)."""
    ok, vals = terms(cam, p, R, t, c)
    s = [float(v) for v in two_level(vals, ok)]
    H = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = s[k]
            k += 1
    return int(ok.sum()), H, s[21:27], s[27]


def rms_of(e2sum, n):
    return math.sqrt(e2sum / n) if n else 0.0


# ---- the whole call -----------------------------------------------------------------------------------------------------------
def refine(cam, p, rel0, disp_cur, disp_prev, flow, mask=None, evaluate=evaluate):
    """cart_dense_ego_refine restated -> RESULT_DTYPE [1]."""
    c = candidates(cam, p, disp_cur, disp_prev, flow, mask)
    R, t = split(rel0)
    res = np.zeros(1, RESULT_DTYPE)
    res["n_candidates"] = int(c["cand"].sum())
    n, _, _, e2 = evaluate(cam, p, R, t, c)
    res["n_initial"], res["rms_initial"] = n, rms_of(e2, n)
    steps = 0
    for _ in range(p["iterations"]):
        n, H, g, _ = evaluate(cam, p, R, t, c)
        if n < p["min_inliers"]:
            break
        delta = solve6(H, g)
        if delta is None:
            break
        R, t = apply_update(R, t, delta)
        steps += 1
    n, _, _, e2 = evaluate(cam, p, R, t, c)
    res["R"][0], res["t"][0] = R, t
    res["n_inliers"], res["rms"], res["steps"], res["status"] = n, rms_of(e2, n), steps, 1 if steps > 0 else 0
    return res


def accept(res, rel0):
    """The consumer's rule -> the 12 doubles of the relative pose to use: the refined one iff status == 1, all 12 entries are finite and
    n_inliers >= n_initial; otherwise rel0."""
    r = res.reshape(-1)[0]
    pose = join([float(v) for v in r["R"]], [float(v) for v in r["t"]])
    if int(r["status"]) == 1 and all(math.isfinite(v) for v in pose) and int(r["n_inliers"]) >= int(r["n_initial"]):
        return pose
    return [float(v) for v in np.asarray(rel0, np.float64).reshape(12)]


# ---- the same spec, one pixel at a time in Python floats ----------------------------------------------------------------------
def scalar_pixel(cam, p, R, t, disp_cur, disp_prev, flow, mask, x, y):
    """-> None for a pixel that is no candidate, else (contributes, the NSUMS values or None)."""
    h, w = np.asarray(disp_cur).shape
    fx, fy, cx, cy, base = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
    wd = p["disparity_weight"]
    sc = int(disp_cur[y][x])
    dc = sc / 16.0
    if sc == INVALID or not dc >= p["min_disparity"]:
        return None
    xp, yp = x - (int(flow[y][x][0]) >> 5), y - (int(flow[y][x][1]) >> 5)
    if not (0 <= xp < w and 0 <= yp < h):
        return None
    sp = int(disp_prev[yp][xp])
    dp = sp / 16.0
    if sp == INVALID or not dp >= p["min_disparity"]:
        return None
    if mask is not None and int(mask[y][x]) == MOVING:
        return None
    fxb = fx * base
    Zp = fxb / dp
    Xp = ((float(xp) - cx) * Zp) / fx
    Yp = ((float(yp) - cy) * Zp) / fy
    qx, qy, qz = (((R[3 * r] * Xp + R[3 * r + 1] * Yp) + R[3 * r + 2] * Zp) + t[r] for r in range(3))
    if not qz > 0:
        return False, None
    eu = (_div(fx * qx, qz) + cx) - float(x)
    ev = (_div(fy * qy, qz) + cy) - float(y)
    ed = _div(fxb, qz) - dc
    ef = eu * eu + ev * ev
    if not (ef < p["flow_threshold"] * p["flow_threshold"] and ed * ed < p["disparity_threshold"] * p["disparity_threshold"]):
        return False, None
    a, b = _div(fx, qz), -_div(fx * qx, qz * qz)
    cc, d = _div(fy, qz), -_div(fy * qy, qz * qz)
    g = -_div(fxb, qz * qz)
    Ju = [b * qy, a * qz - b * qx, -(a * qy), a, 0.0, b]
    Jv = [d * qy - cc * qz, -(d * qx), cc * qx, 0.0, cc, d]
    Jd = [g * qy, -(g * qx), 0.0, 0.0, 0.0, g]
    vals = [(Ju[i] * Ju[j] + Jv[i] * Jv[j]) + wd * (Jd[i] * Jd[j]) for i in range(6) for j in range(i, 6)]
    vals += [(Ju[i] * eu + Jv[i] * ev) + wd * (Jd[i] * ed) for i in range(6)]
    vals.append(ef + wd * (ed * ed))
    return True, vals


def _scalar_butterfly(v):
    o = 1
    while o < LANES:
        v = [v[l] + v[l ^ o] for l in range(LANES)]
        o *= 2
    return v[0]


def scalar_evaluate(cam, p, R, t, disp_cur, disp_prev, flow, mask=None, order=None):
    """-> (count, candidates, the NSUMS sums) by the two-level lane order, one pixel at a time.  `order`, a permutation of the sampled
    columns, replaces the ascending walk of a lane's columns (to show that the order matters)."""
    h, w = np.asarray(disp_cur).shape
    s = p["stride"]
    ni, nj = (w + s - 1) // s, (h + s - 1) // s
    cols = list(range(ni)) if order is None else list(order)
    count = ncand = 0
    rows = []
    for j in range(nj):
        v = [[0.0] * LANES for _ in range(NSUMS)]
        for i in cols:
            got = scalar_pixel(cam, p, R, t, disp_cur, disp_prev, flow, mask, i * s, j * s)
            if got is None:
                continue
            ncand += 1
            if got[0]:
                count += 1
                for k in range(NSUMS):
                    v[k][i % LANES] = v[k][i % LANES] + got[1][k]
        rows.append([_scalar_butterfly(v[k]) for k in range(NSUMS)])
    out = []
    for k in range(NSUMS):
        v = [0.0] * LANES
        for j in range(nj):
            v[j % LANES] = v[j % LANES] + rows[j][k]
        out.append(_scalar_butterfly(v))
    return count, ncand, out

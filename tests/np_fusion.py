"""numpy restatement of spec S28: temporal disparity fusion through ego-motion.  Written from the spec, not from the
kernels: whole-image array arithmetic in the spec's operation order (every numpy ufunc rounds once, there is no fused multiply-add), the
z-buffer by np.maximum.at.  scalar_update() is the same spec as a pure-Python loop over pixels in Python floats (IEEE doubles, one
rounding per operation) and Python integers, for cross-checking the vectorised form."""
import math

import numpy as np

INVALID = -32768
NONE, MEASURED, AGREED, REPLACED, PREDICTED = 0, 1, 2, 3, 4
MOVING = 1
DEFAULTS = dict(min_disparity=1.0, agree_threshold=1.0, splat_radius=0.75, max_weight=4, min_age=2)   # build-owned, untuned
REL_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise ValueError(k)
        p[k] = int(v) if k in ("max_weight", "min_age") else float(v)
    return p


def camera(fx, fy, cx, cy, baseline):
    return dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), baseline=float(baseline))


def splat(cam, p, rel, prev_disp, prev_age, mask_prev=None, want_targets=False):
    """The z-buffer of one frame: uint32 [h, w], 0 where no source landed.  want_targets: also the number of (source, target) writes."""
    R = np.asarray(rel, np.float64).reshape(12)
    s = np.asarray(prev_disp).astype(np.int64)
    a = np.asarray(prev_age).astype(np.int64)
    h, w = s.shape
    yp, xp = np.mgrid[0:h, 0:w]
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    r = np.float64(p["splat_radius"])
    dp = s.astype(np.float64) / 16.0
    src = (a >= 1) & (s != INVALID) & (dp >= p["min_disparity"])
    if mask_prev is not None:
        src &= np.asarray(mask_prev) != MOVING
    fxb = fx * np.float64(cam["baseline"])
    z = np.zeros((h, w), np.uint32)
    writes = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Zp = fxb / dp
        Xp = ((xp.astype(np.float64) - cx) * Zp) / fx
        Yp = ((yp.astype(np.float64) - cy) * Zp) / fy
        q = [((R[4 * k] * Xp + R[4 * k + 1] * Yp) + R[4 * k + 2] * Zp) + R[4 * k + 3] for k in range(3)]
        src &= q[2] > 0
        u = (fx * q[0]) / q[2] + cx
        v = (fy * q[1]) / q[2] + cy
        swd = np.floor((fxb / q[2]) * 16.0 + 0.5)
        src &= (swd >= 1.0) & (swd <= 32767.0)                       # a NaN fails both comparisons
        sw = np.where(src, swd, 0.0).astype(np.int64)
        cols = (-np.floor(-(u - r)), np.floor(u + r))                # ceil(a) = -floor(-a)
        rows = (-np.floor(-(v - r)), np.floor(v + r))
        base = ((sw >> 4) << 16) | ((sw & 15) << 8) | a
        for i in range(2):
            xok = (cols[0] <= cols[1]) & (cols[i] >= 0.0) & (cols[i] <= float(w - 1))
            if i == 1:
                xok &= cols[1] != cols[0]                            # once when they are equal
            for j in range(2):
                yok = (rows[0] <= rows[1]) & (rows[j] >= 0.0) & (rows[j] <= float(h - 1))
                if j == 1:
                    yok &= rows[1] != rows[0]
                m = src & xok & yok
                if not m.any():
                    continue
                f = np.floor(16.0 * np.maximum(np.abs(cols[i][m] - u[m]), np.abs(rows[j][m] - v[m])))
                c = 15 - np.minimum(15, f.astype(np.int64))
                key = (base[m] | (c << 12)).astype(np.uint32)
                np.maximum.at(z, (rows[j][m].astype(np.int64), cols[i][m].astype(np.int64)), key)
                writes += int(m.sum())
    return (z, writes) if want_targets else z


def fuse(p, disp_cur, zbuf, mask_cur=None):
    """The table of S28 -> dict(fused int16, age uint8, source uint8, counts int32 [5])."""
    sc = np.asarray(disp_cur).astype(np.int64)
    P = np.asarray(zbuf).astype(np.int64)
    if mask_cur is not None:
        P = np.where(np.asarray(mask_cur) == MOVING, 0, P)
    sw = ((P >> 16) << 4) | ((P >> 8) & 15)
    aw = P & 255
    valid = (sc != INVALID) & (sc.astype(np.float64) / 16.0 >= p["min_disparity"])
    hit = P != 0
    e = (sc - sw).astype(np.float64) / 16.0
    agree = valid & hit & (e * e <= p["agree_threshold"] * p["agree_threshold"])
    wgt = np.minimum(aw, p["max_weight"])
    mean = (wgt * sw + sc + (wgt + 1) // 2) // (wgt + 1)             # every term is positive where it is used: // is C's division
    pred = ~valid & hit & (aw >= p["min_age"])
    source = np.select([agree, valid & hit, valid, pred], [AGREED, REPLACED, MEASURED, PREDICTED], NONE).astype(np.uint8)
    fused = np.select([agree, pred], [mean, sw], sc).astype(np.int16)
    age = np.select([agree, valid, pred], [np.minimum(aw + 1, 255), 1, aw - 1], 0).astype(np.uint8)
    return dict(fused=fused, age=age, source=source, counts=np.bincount(source.reshape(-1), minlength=5).astype(np.int32))


def update(cam, p, rel, disp_cur, prev=None, mask_prev=None, mask_cur=None):
    """cart_fusion_update restated: prev = (fused, age) of the previous call or None -> dict(fused, age, source, counts, zbuf)."""
    h, w = np.asarray(disp_cur).shape
    z = np.zeros((h, w), np.uint32) if prev is None else splat(cam, p, rel, prev[0], prev[1], mask_prev)
    return dict(fuse(p, disp_cur, z, mask_cur), zbuf=z)


# ---- the same spec, one pixel at a time in Python floats and integers --------------------------------------------------------------
def _div(a, b):
    """IEEE division for b = 0 as well (Python raises)."""
    if b != 0.0:
        return a / b
    return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _floor(a):
    return float(math.floor(a)) if math.isfinite(a) else a


def scalar_update(cam, p, rel, disp_cur, prev=None, mask_prev=None, mask_cur=None):
    R = [float(v) for v in np.asarray(rel, np.float64).reshape(12)] if rel is not None else None
    h, w = np.asarray(disp_cur).shape
    fx, fy, cx, cy, b = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
    r = p["splat_radius"]
    z = [[0] * w for _ in range(h)]
    for yp in range(h if prev is not None else 0):
        for xp in range(w):
            ap, sp = int(prev[1][yp][xp]), int(prev[0][yp][xp])
            dp = sp / 16.0
            if ap < 1 or sp == INVALID or not dp >= p["min_disparity"] or (mask_prev is not None and int(mask_prev[yp][xp]) == MOVING):
                continue
            Zp = (fx * b) / dp
            Xp = ((float(xp) - cx) * Zp) / fx
            Yp = ((float(yp) - cy) * Zp) / fy
            q = [((R[4 * k] * Xp + R[4 * k + 1] * Yp) + R[4 * k + 2] * Zp) + R[4 * k + 3] for k in range(3)]
            if not q[2] > 0:
                continue
            u = _div(fx * q[0], q[2]) + cx
            v = _div(fy * q[1], q[2]) + cy
            swd = _floor(_div(fx * b, q[2]) * 16.0 + 0.5)
            if not (swd >= 1.0 and swd <= 32767.0):
                continue
            sw = int(swd)
            x0, x1, y0, y1 = -_floor(-(u - r)), _floor(u + r), -_floor(-(v - r)), _floor(v + r)
            xs = ([x0] if x0 <= x1 else []) + ([x1] if x0 < x1 else [])
            ys = ([y0] if y0 <= y1 else []) + ([y1] if y0 < y1 else [])
            for yt in ys:
                for xt in xs:
                    if not (xt >= 0.0 and xt <= float(w - 1) and yt >= 0.0 and yt <= float(h - 1)):
                        continue
                    c = 15 - min(15, int(math.floor(16.0 * max(abs(xt - u), abs(yt - v)))))
                    key = ((sw >> 4) << 16) | (c << 12) | ((sw & 15) << 8) | ap
                    z[int(yt)][int(xt)] = max(z[int(yt)][int(xt)], key)
    fused, age, source = np.zeros((h, w), np.int16), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            P = 0 if mask_cur is not None and int(mask_cur[y][x]) == MOVING else z[y][x]
            sw, aw, sc = ((P >> 16) << 4) | ((P >> 8) & 15), P & 255, int(disp_cur[y][x])
            valid = sc != INVALID and sc / 16.0 >= p["min_disparity"]
            out = (sc, 0, NONE)
            if valid and P == 0:
                out = (sc, 1, MEASURED)
            elif valid:
                e = float(sc - sw) / 16.0
                if e * e <= p["agree_threshold"] * p["agree_threshold"]:
                    wgt = min(aw, p["max_weight"])
                    out = ((wgt * sw + sc + (wgt + 1) // 2) // (wgt + 1), min(aw + 1, 255), AGREED)
                else:
                    out = (sc, 1, REPLACED)
            elif P != 0 and aw >= p["min_age"]:
                out = (sw, aw - 1, PREDICTED)
            fused[y, x], age[y, x], source[y, x] = out
    return dict(fused=fused, age=age, source=source, counts=np.bincount(source.reshape(-1), minlength=5).astype(np.int32),
                zbuf=np.array(z, np.uint32).reshape(h, w))

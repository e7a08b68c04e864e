"""numpy restatement of spec S25: motion segmentation from flow, disparity and ego-motion.  Written from the spec, not
from the kernels: whole-image array arithmetic in the spec's operation order (every numpy ufunc rounds once, there is no fused
multiply-add), the window counts as sums of shifted, zero-padded images.  scalar_segment() is the same spec as a pure-Python loop over
pixels in Python floats (IEEE doubles, one rounding per operation) for cross-checking the vectorised form."""
import math

import numpy as np

INVALID = -32768
STATIC, MOVING, UNKNOWN = 0, 1, 2
DEFAULTS = dict(min_disparity=1.0, flow_threshold=2.0, disparity_threshold=1.0, radius=2, support_percent=50)
REL_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise ValueError(k)
        p[k] = int(v) if k in ("radius", "support_percent") else float(v)
    return p


def camera(fx, fy, cx, cy, baseline):
    return dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), baseline=float(baseline))


def quantise(e):
    """Q(e) = (int16) clamp(floor(e * 16.0 + 0.5), -32767, 32767); Q(NaN) = -32767 (the clamp's first test is `not v > -32767`)"""
    v = np.floor(np.asarray(e, np.float64) * 16.0 + 0.5)
    return np.clip(np.where(np.isnan(v), -32767.0, v), -32767.0, 32767.0).astype(np.int16)


def residual(cam, p, rel, disp_cur, disp_prev, flow):
    """-> (record int16 [h, w, 4], raw uint8 [h, w], gate uint8 [h, w]: the gate 1..4 that made a pixel UNKNOWN, 0 for a known one)."""
    R = np.asarray(rel, np.float64).reshape(12)
    sc = np.asarray(disp_cur).astype(np.int64)
    spi = np.asarray(disp_prev).astype(np.int64)
    fl = np.asarray(flow).astype(np.int64)
    h, w = sc.shape
    y, x = np.mgrid[0:h, 0:w]
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    gate = np.zeros((h, w), np.uint8)
    dc = sc.astype(np.float64) / 16.0
    gate[(gate == 0) & ~((sc != INVALID) & (dc >= p["min_disparity"]))] = 1
    xp, yp = x - (fl[..., 0] >> 5), y - (fl[..., 1] >> 5)                  # numpy's >> on signed integers is arithmetic
    inside = (xp >= 0) & (xp < w) & (yp >= 0) & (yp < h)
    gate[(gate == 0) & ~inside] = 2
    sp = spi[np.clip(yp, 0, h - 1), np.clip(xp, 0, w - 1)]
    dp = sp.astype(np.float64) / 16.0
    gate[(gate == 0) & ~((sp != INVALID) & (dp >= p["min_disparity"]))] = 3
    fxb = fx * np.float64(cam["baseline"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Zp = fxb / dp
        Xp = ((xp.astype(np.float64) - cx) * Zp) / fx
        Yp = ((yp.astype(np.float64) - cy) * Zp) / fy
        q = [((R[4 * r] * Xp + R[4 * r + 1] * Yp) + R[4 * r + 2] * Zp) + R[4 * r + 3] for r in range(3)]
        gate[(gate == 0) & ~(q[2] > 0)] = 4
        eu = ((fx * q[0]) / q[2] + cx) - x.astype(np.float64)
        ev = ((fy * q[1]) / q[2] + cy) - y.astype(np.float64)
        ed = fxb / q[2] - dc
        moving = (eu * eu + ev * ev > p["flow_threshold"] * p["flow_threshold"]) | (ed * ed > p["disparity_threshold"] * p["disparity_threshold"])
    known = gate == 0
    raw = np.where(known, np.where(moving, MOVING, STATIC), UNKNOWN).astype(np.uint8)
    rec = np.full((h, w, 4), INVALID, np.int16)
    rec[..., 3] = raw
    for c, e in enumerate((eu, ev, ed)):
        rec[..., c][known] = quantise(e[known])
    return rec, raw, gate


def majority(raw, radius, support_percent):
    """The filtered labels: window counts of raw 1 and raw 0 over the (2 radius + 1)^2 window clipped to the image."""
    raw = np.asarray(raw)
    h, w = raw.shape
    r = int(radius)
    nm, ns = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    pm, ps = np.pad((raw == MOVING).astype(np.int64), r), np.pad((raw == STATIC).astype(np.int64), r)   # zero padding = clipping
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            nm += pm[dy:dy + h, dx:dx + w]
            ns += ps[dy:dy + h, dx:dx + w]
    out = np.where(nm * 100 >= int(support_percent) * (nm + ns), MOVING, STATIC).astype(np.uint8)
    out[raw == UNKNOWN] = UNKNOWN
    return out, nm, ns


def segment(cam, p, rel, disp_cur, disp_prev, flow, planes=None):
    """cart_motion_segment restated -> dict(residual, raw, labels, planes_static (None without planes), gate)."""
    rec, raw, gate = residual(cam, p, rel, disp_cur, disp_prev, flow)
    labels = majority(raw, p["radius"], p["support_percent"])[0]
    static = None if planes is None else np.where(labels == MOVING, UNKNOWN, np.asarray(planes)).astype(np.uint8)
    return dict(residual=rec, raw=raw, labels=labels, planes_static=static, gate=gate)


def unknown_frame(h, w, planes=None):
    """What a frame without an estimate publishes: all-UNKNOWN labels, the UNKNOWN record everywhere, planes_static = planes."""
    rec = np.full((h, w, 4), INVALID, np.int16)
    rec[..., 3] = UNKNOWN
    lab = np.full((h, w), UNKNOWN, np.uint8)
    return dict(residual=rec, raw=lab, labels=lab.copy(), planes_static=None if planes is None else np.asarray(planes).astype(np.uint8).copy())


# ---- the same spec, one pixel at a time in Python floats --------------------------------------------------------------------
def _q(e):
    if math.isnan(e):
        return -32767
    v = math.floor(e * 16.0 + 0.5) if math.isfinite(e) else e
    return int(min(max(v, -32767), 32767))


def _div(a, b):
    """IEEE division for b = 0 as well (Python raises)."""
    if b != 0.0:
        return a / b
    return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a) * math.copysign(1.0, b)


def scalar_segment(cam, p, rel, disp_cur, disp_prev, flow, planes=None):
    R = [float(v) for v in np.asarray(rel, np.float64).reshape(12)]
    h, w = np.asarray(disp_cur).shape
    fx, fy, cx, cy, b = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
    rec = np.zeros((h, w, 4), np.int16)
    raw = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            rec[y, x] = (INVALID, INVALID, INVALID, UNKNOWN)
            raw[y, x] = UNKNOWN
            sc = int(disp_cur[y][x])
            dc = sc / 16.0
            if sc == INVALID or not dc >= p["min_disparity"]:
                continue
            xp, yp = x - (int(flow[y][x][0]) >> 5), y - (int(flow[y][x][1]) >> 5)     # Python's >> floors: arithmetic
            if not (0 <= xp < w and 0 <= yp < h):
                continue
            sp = int(disp_prev[yp][xp])
            dp = sp / 16.0
            if sp == INVALID or not dp >= p["min_disparity"]:
                continue
            Zp = (fx * b) / dp
            Xp = ((float(xp) - cx) * Zp) / fx
            Yp = ((float(yp) - cy) * Zp) / fy
            q = [((R[4 * r] * Xp + R[4 * r + 1] * Yp) + R[4 * r + 2] * Zp) + R[4 * r + 3] for r in range(3)]
            if not q[2] > 0:
                continue
            eu = (_div(fx * q[0], q[2]) + cx) - float(x)
            ev = (_div(fy * q[1], q[2]) + cy) - float(y)
            ed = _div(fx * b, q[2]) - dc
            moving = eu * eu + ev * ev > p["flow_threshold"] * p["flow_threshold"] or ed * ed > p["disparity_threshold"] * p["disparity_threshold"]
            raw[y, x] = MOVING if moving else STATIC
            rec[y, x] = (_q(eu), _q(ev), _q(ed), raw[y, x])
    labels = np.full((h, w), UNKNOWN, np.uint8)
    r = p["radius"]
    for y in range(h):
        for x in range(w):
            if raw[y, x] == UNKNOWN:
                continue
            nm = ns = 0
            for yy in range(max(0, y - r), min(h, y + r + 1)):
                for xx in range(max(0, x - r), min(w, x + r + 1)):
                    nm += raw[yy, xx] == MOVING
                    ns += raw[yy, xx] == STATIC
            labels[y, x] = MOVING if nm * 100 >= p["support_percent"] * (nm + ns) else STATIC
    static = None if planes is None else np.where(labels == MOVING, UNKNOWN, np.asarray(planes)).astype(np.uint8)
    return dict(residual=rec, raw=raw, labels=labels, planes_static=static)

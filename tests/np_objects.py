"""numpy restatement of spec S31: moving-object measurements from the motion components and their tracks.  Written
from the spec, not from the kernels: per object, array arithmetic over its pixels in the spec's operation order (every numpy ufunc
rounds once, there is no fused multiply-add), integer sums in int64.  scalar_measure() is the same measurement as a pure-Python loop
over pixels in Python floats (IEEE doubles, one rounding per operation) for cross-checking the vectorised form.  The tracker is one
plain loop in Python floats: it is small and has no vector form."""
import math

import numpy as np

from np_motion import INVALID, _div, camera  # noqa: F401  (camera: the dict every restatement of the warp chain takes)

BINS = 512
MOVING = 1
DEFAULTS = dict(min_disparity=1.0, disparity_band=2.0, max_speed=5.0, gate=2.0, min_area=64, min_points=16, gain_percent=50, max_missed=3, min_age=3)
_INTS = ("min_area", "min_points", "gain_percent", "max_missed", "min_age")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
QP_MAX = 2147483647

OBJECT_DTYPE = np.dtype([("component", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("median_bin", "<i4"), ("n_hist", "<i4"),
                         ("n_points", "<i4"), ("n_flow", "<i4"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("sum", "<i8", 3), ("flow_sum", "<i8", 3),
                         ("centroid", "<f8", 3), ("velocity", "<f8", 3), ("extent", "<f8", 3), ("valid", "<i4"), ("has_velocity", "<i4")])   # cart_object
TRACK_DTYPE = np.dtype([("id", "<u4"), ("state", "<i4"), ("age", "<i4"), ("missed", "<i4"), ("object", "<i4"), ("component", "<i4"),
                        ("position", "<f8", 3), ("velocity", "<f8", 3), ("extent", "<f8", 3)])   # cart_track
assert OBJECT_DTYPE.itemsize == 192 and TRACK_DTYPE.itemsize == 96
COUNTS = ("components", "n_selected", "n_objects", "n_valid", "n_matched", "n_born", "n_dropped", "n_live")


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise ValueError(k)
        p[k] = int(v) if k in _INTS else float(v)
    return p


def qp(v):
    """Qp(v) = (int64) clamp(floor(v * 1024.0 + 0.5), -2147483647, 2147483647); Qp(NaN) = -2147483647 (the clamp's first test is `not v > -2147483647`)"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(np.asarray(v, np.float64) * 1024.0 + 0.5)
    return np.clip(np.where(np.isnan(q), -float(QP_MAX), q), -float(QP_MAX), float(QP_MAX)).astype(np.int64)


def select(table, n_components, p, max_objects):
    """-> (table rows of the objects in order, n_selected, entries walked).  table = int32 [max_components, 7] rows {id, label, area, x0, y0, x1, y1}."""
    table = np.asarray(table).reshape(-1, 7)
    seen = min(max(int(n_components), 0), table.shape[0])
    rows = [k for k in range(seen) if table[k, 1] == MOVING and table[k, 2] >= p["min_area"]]
    return rows[:max_objects], len(rows), seen


def component_table(labels, ids, max_components, fill=(0, 0, 0, 0, 0, 0, 0)):
    """cart_plane_ccl_table's table restated from a label image and its ids -> (int32 [max_components, 7] in ascending id order, the true
    count).  The rows past the count, which the library leaves undefined, hold `fill`."""
    labels, ids = np.asarray(labels), np.asarray(ids)
    roots = np.unique(ids[ids >= 0])
    table = np.empty((max_components, 7), np.int32)
    table[:] = fill
    w = ids.shape[1]
    for k, r in enumerate(roots[:max_components]):
        ys, xs = np.nonzero(ids == r)
        table[k] = (r, labels[r // w, r % w], len(ys), xs.min(), ys.min(), xs.max(), ys.max())
    return table, len(roots)


def median_bin(hist):
    """The smallest bin whose cumulative count is >= (n + 1) >> 1, -1 for an empty histogram -> (B, n)."""
    n = int(np.sum(hist))
    if n == 0:
        return -1, 0
    return int(np.searchsorted(np.cumsum(hist), (n + 1) >> 1, side="left")), n


def band16(p):
    return int(math.floor(p["disparity_band"] * 16.0))


def _derive(o, p, pose):
    """The fp64 fields of one record from its integer sums, in place."""
    P = [float(v) for v in np.asarray(pose, np.float64).reshape(12)]
    n, nf = int(o["n_points"]), int(o["n_flow"])
    o["valid"] = int(n >= p["min_points"])
    o["has_velocity"] = int(o["valid"] and nf >= p["min_points"])
    if o["valid"]:
        c = [(float(int(o["sum"][i])) / 1024.0) / float(n) for i in range(3)]
        o["centroid"] = [((P[4 * r] * c[0] + P[4 * r + 1] * c[1]) + P[4 * r + 2] * c[2]) + P[4 * r + 3] for r in range(3)]
        o["extent"] = [float(int(o["hi"][i]) - int(o["lo"][i])) / 1024.0 for i in range(3)]
    if o["has_velocity"]:
        v = [(float(int(o["flow_sum"][i])) / 1024.0) / float(nf) for i in range(3)]
        o["velocity"] = [(P[4 * r] * v[0] + P[4 * r + 1] * v[1]) + P[4 * r + 2] * v[2] for r in range(3)]


def measure(cam, p, rel, pose, ids, table, n_components, disp_cur, disp_prev, flow, max_objects):
    """Selection, both passes and the derived fields -> (objects OBJECT_DTYPE [max_objects] with the rows past n_objects all zero,
    n_selected, entries walked, info).  info counts what the gates did over all objects: pixels of objects, pixels pass 1 refused,
    pixels the band refused, points, flow points, points refused by gates 2 - 4 and by max_speed."""
    R = np.asarray(rel, np.float64).reshape(12)
    ids = np.asarray(ids)
    table = np.asarray(table).reshape(-1, 7)
    sc_all, sp_all, fl_all = np.asarray(disp_cur).astype(np.int64), np.asarray(disp_prev).astype(np.int64), np.asarray(flow).astype(np.int64)
    h, w = sc_all.shape
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    fxb = fx * np.float64(cam["baseline"])
    rows, n_selected, seen = select(table, n_components, p, max_objects)
    out = np.zeros(max_objects, OBJECT_DTYPE)
    info = dict(pixels=0, gate1=0, band=0, points=0, flow=0, gate234=0, speed=0)
    b16 = band16(p)
    for j, k in enumerate(rows):
        o = out[j]
        o["component"], o["area"] = table[k, 0], table[k, 2]
        o["x0"], o["y0"], o["x1"], o["y1"] = 0, 0, -1, -1
        ys, xs = np.nonzero(ids == table[k, 0]) if 0 <= table[k, 0] < w * h else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        sc = sc_all[ys, xs]
        ok1 = (sc != INVALID) & (sc.astype(np.float64) / 16.0 >= p["min_disparity"])
        B, n_hist = median_bin(np.bincount(np.minimum(sc[ok1] >> 4, BINS - 1), minlength=BINS))
        o["median_bin"], o["n_hist"] = B, n_hist
        pt = ok1 & (np.abs(sc - (16 * B + 8)) <= b16)
        info["pixels"] += len(sc); info["gate1"] += int((~ok1).sum()); info["band"] += int((ok1 & ~pt).sum()); info["points"] += int(pt.sum())
        ys, xs, sc = ys[pt], xs[pt], sc[pt]
        o["n_points"] = len(sc)
        if len(sc):
            Z = fxb / (sc.astype(np.float64) / 16.0)
            P = (((xs.astype(np.float64) - cx) * Z) / fx, ((ys.astype(np.float64) - cy) * Z) / fy, Z)
            Q = [qp(c) for c in P]
            o["sum"], o["lo"], o["hi"] = [q.sum() for q in Q], [q.min() for q in Q], [q.max() for q in Q]
            o["x0"], o["y0"], o["x1"], o["y1"] = xs.min(), ys.min(), xs.max(), ys.max()
            xp, yp = xs - (fl_all[ys, xs, 0] >> 5), ys - (fl_all[ys, xs, 1] >> 5)
            inside = (xp >= 0) & (xp < w) & (yp >= 0) & (yp < h)
            sp = sp_all[np.clip(yp, 0, h - 1), np.clip(xp, 0, w - 1)]
            dp = sp.astype(np.float64) / 16.0
            ok = inside & (sp != INVALID) & (dp >= p["min_disparity"])
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                Zp = fxb / dp
                Xp = ((xp.astype(np.float64) - cx) * Zp) / fx
                Yp = ((yp.astype(np.float64) - cy) * Zp) / fy
                q = [((R[4 * r] * Xp + R[4 * r + 1] * Yp) + R[4 * r + 2] * Zp) + R[4 * r + 3] for r in range(3)]
                ok &= q[2] > 0
                f = [P[i] - q[i] for i in range(3)]
                slow = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] <= p["max_speed"] * p["max_speed"]
            info["gate234"] += int((~ok).sum()); info["speed"] += int((ok & ~slow).sum())
            ok &= slow
            o["n_flow"] = int(ok.sum())
            o["flow_sum"] = [qp(c[ok]).sum() for c in f]
            info["flow"] += int(ok.sum())
        _derive(o, p, pose)
    return out, n_selected, seen, info


# ---- the same measurement, one pixel at a time in Python floats ---------------------------------------------------------------
def _qp(v):
    if math.isnan(v):
        return -QP_MAX
    q = math.floor(v * 1024.0 + 0.5) if math.isfinite(v * 1024.0 + 0.5) else v * 1024.0 + 0.5
    return int(min(max(q, -QP_MAX), QP_MAX))


def scalar_measure(cam, p, rel, pose, ids, table, n_components, disp_cur, disp_prev, flow, max_objects):
    R = [float(v) for v in np.asarray(rel, np.float64).reshape(12)]
    table = np.asarray(table).reshape(-1, 7)
    h, w = np.asarray(disp_cur).shape
    fx, fy, cx, cy, b = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
    rows, n_selected, seen = select(table, n_components, p, max_objects)
    slot = {int(table[k, 0]): j for j, k in enumerate(rows)}
    out = np.zeros(max_objects, OBJECT_DTYPE)
    hist = [[0] * BINS for _ in rows]
    for j, k in enumerate(rows):
        out[j]["component"], out[j]["area"] = table[k, 0], table[k, 2]
        out[j]["x0"], out[j]["y0"], out[j]["x1"], out[j]["y1"] = 0, 0, -1, -1

    def gate1(y, x):
        sc = int(disp_cur[y][x])
        return sc if sc != INVALID and sc / 16.0 >= p["min_disparity"] else None

    for y in range(h):
        for x in range(w):
            j = slot.get(int(ids[y][x]))
            if j is not None and gate1(y, x) is not None:
                hist[j][min(gate1(y, x) >> 4, BINS - 1)] += 1
    acc = []
    for j in range(len(rows)):
        n, cum, B = sum(hist[j]), 0, -1
        if n:
            for B in range(BINS):
                cum += hist[j][B]
                if cum >= (n + 1) >> 1:
                    break
        out[j]["median_bin"], out[j]["n_hist"] = B, n
        acc.append(dict(n=0, nf=0, sum=[0, 0, 0], fsum=[0, 0, 0], lo=[None] * 3, hi=[None] * 3, box=None))
    b16 = band16(p)
    for y in range(h):
        for x in range(w):
            j = slot.get(int(ids[y][x]))
            sc = gate1(y, x) if j is not None else None
            if sc is None or abs(sc - (16 * int(out[j]["median_bin"]) + 8)) > b16:
                continue
            a = acc[j]
            Z = (fx * b) / (sc / 16.0)
            P = (((float(x) - cx) * Z) / fx, ((float(y) - cy) * Z) / fy, Z)
            a["n"] += 1
            for i in range(3):
                q = _qp(P[i])
                a["sum"][i] += q
                a["lo"][i] = q if a["lo"][i] is None else min(a["lo"][i], q)
                a["hi"][i] = q if a["hi"][i] is None else max(a["hi"][i], q)
            a["box"] = (x, y, x, y) if a["box"] is None else (min(a["box"][0], x), min(a["box"][1], y), max(a["box"][2], x), max(a["box"][3], y))
            xp, yp = x - (int(flow[y][x][0]) >> 5), y - (int(flow[y][x][1]) >> 5)
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
            f = [P[i] - q[i] for i in range(3)]
            if not (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] <= p["max_speed"] * p["max_speed"]:
                continue
            a["nf"] += 1
            for i in range(3):
                a["fsum"][i] += _qp(f[i])
    for j, a in enumerate(acc):
        o = out[j]
        o["n_points"], o["n_flow"], o["sum"], o["flow_sum"] = a["n"], a["nf"], a["sum"], a["fsum"]
        if a["n"]:
            o["lo"], o["hi"] = a["lo"], a["hi"]
            o["x0"], o["y0"], o["x1"], o["y1"] = a["box"]
        _derive(o, p, pose)
    return out, n_selected, seen


# ---- the tracks -------------------------------------------------------------------------------------------------------------------
def free_tracks(n):
    t = np.zeros(n, TRACK_DTYPE)
    t["object"], t["component"] = -1, -1
    return t


class Tracker:
    """cart_object_tracker restated: `tracks` holds every slot (state 0 = free), next_id starts at 1."""

    def __init__(self, max_objects, max_tracks):
        self.max_objects, self.max_tracks = int(max_objects), int(max_tracks)
        self.reset()

    def reset(self):
        self.tracks, self.next_id = free_tracks(self.max_tracks), 1

    def associate(self, objects, n_objects, p):
        """Steps 1 - 6 of the spec on the measured objects -> (n_valid, n_matched, n_born, n_dropped, n_live)."""
        T = self.tracks
        valid = [o for o in range(n_objects) if objects[o]["valid"]]
        live = [t for t in range(self.max_tracks) if T[t]["state"] != 0]
        pred = {t: [float(T[t]["position"][i]) + float(T[t]["velocity"][i]) for i in range(3)] for t in live}
        g2 = p["gate"] * p["gate"]
        pairs = {}
        for t in live:
            for o in valid:
                d = [float(objects[o]["centroid"][i]) - pred[t][i] for i in range(3)]
                d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if d2 <= g2:
                    pairs[(t, o)] = d2
        match = {}
        while True:
            best = None
            for (t, o), d2 in sorted(pairs.items()):                 # ascending slot, then ascending object: a strict < keeps the first of a tie
                if t not in match and o not in match.values() and (best is None or d2 < best[0]):
                    best = (d2, t, o)
            if best is None:
                break
            match[best[1]] = best[2]
        g = p["gain_percent"] / 100.0
        for t in live:
            tr = T[t]
            if t in match:
                ob = objects[match[t]]
                for i in range(3):
                    m = float(ob["velocity"][i]) if ob["has_velocity"] else float(ob["centroid"][i]) - float(tr["position"][i])
                    tr["velocity"][i] = float(tr["velocity"][i]) + g * (m - float(tr["velocity"][i]))
                tr["position"], tr["extent"] = ob["centroid"], ob["extent"]
                tr["age"] += 1
                tr["missed"] = 0
                tr["object"], tr["component"] = match[t], ob["component"]
                tr["state"] = 2 if tr["age"] >= p["min_age"] else 1
            else:
                tr["position"] = pred[t]
                tr["missed"] += 1
                tr["object"], tr["component"] = -1, -1
                if tr["missed"] > p["max_missed"]:
                    T[t] = free_tracks(1)[0]
        born = dropped = 0
        for o in valid:
            if o in match.values():
                continue
            free = [t for t in range(self.max_tracks) if T[t]["state"] == 0]
            if not free:
                dropped += 1
                continue
            tr, ob = T[free[0]], objects[o]
            tr["id"], self.next_id = self.next_id, (self.next_id + 1) & 0xFFFFFFFF
            tr["age"], tr["missed"], tr["state"] = 1, 0, 2 if p["min_age"] <= 1 else 1
            tr["object"], tr["component"] = o, ob["component"]
            tr["position"], tr["extent"] = ob["centroid"], ob["extent"]
            tr["velocity"] = ob["velocity"]                          # +0.0 without has_velocity
            born += 1
        return len(valid), len(match), born, dropped, int((T["state"] != 0).sum())

    def update(self, cam, p, rel, pose, ids, table, n_components, disp_cur, disp_prev, flow, measure_fn=None):
        """cart_object_tracker_update restated -> dict(objects, tracks (a copy of every slot), counts int32 [8], info)."""
        res = (measure_fn or measure)(cam, p, rel, pose, ids, table, n_components, disp_cur, disp_prev, flow, self.max_objects)
        objects, n_selected, seen = res[:3]
        n_objects = min(n_selected, self.max_objects)
        tail = self.associate(objects, n_objects, p)
        counts = np.array((seen, n_selected, n_objects) + tail, np.int32)
        return dict(objects=objects, tracks=self.tracks.copy(), counts=counts, info=res[3] if len(res) > 3 else None)

"""CPU restatement of the superpixel plane stages, DESIGN.md S17-S19 (pure numpy / Python, exact fp64).

S17  per-label RANSAC plane          (the reference's segmentPlane / getPlaneFromPoints, src/utils/plane.cpp:56-180)
S18  planecluster host merge         (src/modules/planecluster.cpp:19-177, one OpenMP thread)
S19  planefit assignment loop        (src/modules/planefit.cu:223-445)

Every sum is written in the order the spec fixes: sequential where the reference sums sequentially, and the 64-lane
strided + butterfly order for the refit.  numpy's own `sum` is pairwise and is never used on floating point here.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
THR17 = 0.01            # plane.hpp:7-12
RANSAC_N = 4
ITERS = 100
MIN_POINTS = 16
QERR_SCALE = float(1 << 24)
PRED_PLANEFIT, PRED_PLANECLUSTER = 0, 1


# ---- counter-based generator ----------------------------------------------------------------------------------------
def mix(z):
    """splitmix64 finaliser (mod 2^64)."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def stream(seed, tag, a, b, c):
    return mix(mix(mix(mix((seed ^ tag) & M64) ^ (a & M64)) ^ (b & M64)) ^ (c & M64))


def draw(s, c):
    return mix((s + c) & M64)


def uniform(d, n):
    """uniform index in [0, n) from one draw."""
    return ((d >> 32) * n) >> 32


# ---- per-label points -------------------------------------------------------------------------------------------------
def valid_mask(z, predicate):
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        if predicate == PRED_PLANEFIT:      # IS_VALID_DEPTH, planefit.cu:20
            return np.isfinite(z) & (z <= 40) & (z > 0)
        return ~((z <= 0) | (z > 40))       # planecluster.cpp:35 (NaN passes)


def label_points(labels, xyz, max_label, predicate):
    """-> (counts [L+1,2] int64 (all, invalid), offsets [L+2], points [n,3] float32 in label-major raster order).
    Pixels whose label is above max_label are left out of everything (the device reports them through its status)."""
    lab = np.asarray(labels).astype(np.int64).ravel()
    pts = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    L1 = max_label + 1
    keep = lab < L1
    lab, pts = lab[keep], pts[keep]
    ok = valid_mask(pts[:, 2], predicate)
    counts = np.zeros((L1, 2), np.int64)
    counts[:, 0] = np.bincount(lab, minlength=L1)[:L1]
    counts[:, 1] = np.bincount(lab[~ok], minlength=L1)[:L1]
    order = np.argsort(lab[ok], kind="stable")
    sel = np.nonzero(ok)[0][order]
    npts = np.bincount(lab[ok], minlength=L1)[:L1]
    offsets = np.zeros(L1 + 1, np.int64)
    offsets[1:] = np.cumsum(npts)
    return counts, offsets, pts[sel]


# ---- getPlaneFromPoints -----------------------------------------------------------------------------------------------
def _plane_from_moments(c, m):
    cx, cy, cz = c
    xx, xy, xz, yy, yz, zz = m
    detX = yy * zz - yz * yz
    detY = xx * zz - xz * xz
    detZ = xx * yy - xy * xy
    if detX <= 0 and detY <= 0 and detZ <= 0:
        return (0.0, 0.0, 0.0, 0.0)
    if detX > detY and detX > detZ:
        a, b, cc = detX, xz * yz - xy * zz, xy * yz - xz * yy
    elif detY > detZ:
        a, b, cc = xz * yz - xy * zz, detY, xy * xz - yz * xx
    else:
        a, b, cc = xy * yz - xz * yy, xy * xz - yz * xx, detZ
    inv = 1.0 / math.sqrt((a * a + b * b) + cc * cc)
    a, b, cc = a * inv, b * inv, cc * inv
    d = -((a * cx + b * cy) + cc * cz)
    return (a, b, cc, d)


def plane_sequential(P):
    """getPlaneFromPoints with sequential sums in the given order; P = list of (x, y, z) Python floats."""
    sx = sy = sz = 0.0
    for x, y, z in P:
        sx += x; sy += y; sz += z
    n = float(len(P))
    c = (sx / n, sy / n, sz / n)
    m = [0.0] * 6
    for x, y, z in P:
        rx, ry, rz = x - c[0], y - c[1], z - c[2]
        m[0] += rx * rx; m[1] += rx * ry; m[2] += rx * rz
        m[3] += ry * ry; m[4] += ry * rz; m[5] += rz * rz
    return _plane_from_moments(c, m)


def lane_sum(v):
    """The refit order: lane j of 64 adds v[j], v[j+64], ... in order; then v[j] += v[j^o], o = 32..1; lane 0."""
    v = np.asarray(v, dtype=np.float64)
    rows = (len(v) + 63) // 64
    pad = np.zeros(rows * 64)
    pad[:len(v)] = v
    acc = np.zeros(64)
    for r in range(rows):
        acc = acc + pad[r * 64:(r + 1) * 64]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[idx ^ o]
    return float(acc[0])


def plane_lanes(P):
    """getPlaneFromPoints with the 64-lane sums (S17 refit); P = [n,3] float64."""
    n = float(len(P))
    c = (lane_sum(P[:, 0]) / n, lane_sum(P[:, 1]) / n, lane_sum(P[:, 2]) / n)
    r = P - np.array(c)
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    m = [lane_sum(rx * rx), lane_sum(rx * ry), lane_sum(rx * rz), lane_sum(ry * ry), lane_sum(ry * rz), lane_sum(rz * rz)]
    return _plane_from_moments(c, m)


def dist_vec4(pl, P):
    """|((a*x + b*y) + c*z) + d| (Vec4d::dot order), P = [n,3] float64."""
    a, b, c, d = pl
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(((a * P[:, 0] + b * P[:, 1]) + c * P[:, 2]) + d)


def hypothesis_indices(seed, frame_id, label, h, n):
    s = stream(seed, 1, frame_id, label, h)
    picked, c = [], 0
    while len(picked) < RANSAC_N:
        i = uniform(draw(s, c), n)
        c += 1
        if i not in picked:
            picked.append(i)
    return picked


def ransac_plane(points, seed, frame_id, label, thr=THR17, return_best=False):
    """S17 for one label; points = [n,3] float32 (raster order)."""
    P = np.asarray(points, dtype=np.float32).astype(np.float64)
    n = len(P)
    zero = (0.0, 0.0, 0.0, 0.0)
    if n < MIN_POINTS:
        return (zero, None) if return_best else zero
    thr2 = thr * thr
    hyps, hs = [], []
    for h in range(ITERS):
        pl = plane_sequential([tuple(float(v) for v in P[i]) for i in hypothesis_indices(seed, frame_id, label, h, n)])
        if pl != zero:
            hyps.append(pl)
            hs.append(h)
    best = None    # (count, qerr, h, plane)
    with np.errstate(invalid="ignore", over="ignore"):
        if hyps:
            H = np.array(hyps)
            a, b, c, d = (H[:, k:k + 1] for k in range(4))
            dist = np.abs(((a * P[None, :, 0] + b * P[None, :, 1]) + c * P[None, :, 2]) + d)    # [hyp, point]
            inl = dist < thr
            cnt = inl.sum(axis=1)
            q = np.where(inl, np.floor((dist * dist) / thr2 * QERR_SCALE), 0.0).astype(np.uint64).sum(axis=1)   # integers: any order
            for k in range(len(hyps)):
                if cnt[k] < 1:
                    continue
                if best is None or cnt[k] > best[0] or (cnt[k] == best[0] and int(q[k]) < best[1]):
                    best = (int(cnt[k]), int(q[k]), hs[k], hyps[k])
        if best is None:
            return (zero, None) if return_best else zero
        inl = dist_vec4(best[3], P) < thr
        out = plane_lanes(P[inl])
    return (out, best) if return_best else out


def label_planes(labels, xyz, max_label, predicate, seed, frame_id, thr=THR17):
    """S17 for every label -> (planes [L+1,4] float64, npoints [L+1], counts [L+1,2], offsets, points)."""
    counts, offsets, pts = label_points(labels, xyz, max_label, predicate)
    planes = np.zeros((max_label + 1, 4))
    for l in range(max_label + 1):
        planes[l] = ransac_plane(pts[offsets[l]:offsets[l + 1]], seed, frame_id, l, thr)
    return planes, np.diff(offsets), counts, offsets, pts


# ---- adjacency --------------------------------------------------------------------------------------------------------
def adjacency(labels, max_label):
    """8-neighbour label sets (planecluster.cpp:72-96) as CSR (offsets [L+2], ascending neighbours).  A pair with a label above
    max_label on either side is dropped."""
    lab = np.asarray(labels).astype(np.int64)
    h, w = lab.shape
    L1 = max_label + 1
    pairs = set()
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        a = lab[0:h - dy, max(0, -dx):w - max(0, dx)]
        b = lab[dy:h, max(0, dx):w - max(0, -dx)]
        m = (a != b) & (a < L1) & (b < L1)
        key = np.unique(a[m] * L1 + b[m])
        pairs.update(key.tolist())
        key = np.unique(b[m] * L1 + a[m])
        pairs.update(key.tolist())
    keys = np.array(sorted(pairs), dtype=np.int64)
    src = keys // L1 if len(keys) else np.zeros(0, np.int64)
    offsets = np.zeros(L1 + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(src, minlength=L1)[:L1])
    return offsets, (keys % L1 if len(keys) else np.zeros(0, np.int64))


# ---- S18 planecluster ------------------------------------------------------------------------------------------------
def plane_cluster(planes, offsets, neigh, min_group=32):
    """-> (planes [k,4], assignments [L+1] uint64)."""
    L1 = len(planes)
    zero = [bool((planes[l] == 0).all()) for l in range(L1)]
    st = [None] * L1
    for l in range(L1):
        if zero[l]:
            continue
        a, b, c, d = (float(v) for v in planes[l])
        length = math.sqrt((a * a + b * b) + c * c)
        yaw = math.atan2(b, a)
        pitch = math.atan2(c, length)
        st[l] = (d, math.sin(yaw), math.cos(yaw), math.sin(pitch), math.cos(pitch))
    nb = [neigh[offsets[l]:offsets[l + 1]].tolist() for l in range(L1)]
    out, assign = [], [0] * L1
    for l in range(L1):
        if assign[l] != 0 or zero[l]:
            continue
        s = st[l]
        similar = [l]
        seen = {l}
        frontier = set(nb[l])
        while frontier:
            o = min(frontier)
            frontier.discard(o)
            seen.add(o)
            if zero[o]:
                continue
            t = st[o]
            yawd = abs(s[1] - t[1]) + abs(s[2] - t[2])
            pitchd = abs(s[3] - t[3]) + abs(s[4] - t[4])
            dd = abs(s[0] - t[0])
            if yawd < 0.2 and pitchd < 0.2 and dd < 3:
                cur = assign[o]
                if cur != 0:
                    u = out[cur - 1][1]
                    cy = abs(u[1] - t[1]) + abs(u[2] - t[2])
                    cp = abs(u[3] - t[3]) + abs(u[4] - t[4])
                    if cy + cp + dd < yawd + pitchd + dd:
                        continue
                similar.append(o)
                for q in nb[o]:
                    if q not in seen:
                        frontier.add(q)
        if len(similar) < min_group:
            continue
        out.append((l, s))
        for q in similar:
            assign[q] = len(out)
    P = np.array([planes[l] for l, _ in out], dtype=np.float64).reshape(-1, 4)
    return P, np.array(assign, dtype=np.uint64)


# ---- S19 planefit ----------------------------------------------------------------------------------------------------
FIT_THR = 0.02
FIT_MAX_PLANES = 100


def sample_positions(w, h, seed, frame_id, it, xcount=4, ycount=3):
    """selectRandomSuperpixels(4, 3) (planefit.cu:329-355) with the S19 jitter -> list of (x, y) inside the image."""
    ystep, xstep = h // (ycount + 2), w // (xcount + 2)
    out = []
    if ystep <= 0 or xstep <= 0:
        return out
    s = 0
    y = ystep
    while y < h:
        x = xstep
        while x < w:
            st = stream(seed, 2, frame_id, it, s)
            hx, hy = xstep // 2, ystep // 2
            xo = x - hx + uniform(draw(st, 0), 2 * hx + 1)
            yo = y - hy + uniform(draw(st, 1), 2 * hy + 1)
            s += 1
            if 0 <= xo < w and 0 <= yo < h:
                out.append((xo, yo))
            x += xstep
        y += ystep
    return out


def fit_distance(pl, P):
    """|a*x+b*y+c*z+d| / sqrt(a*a+b*b+c*c) (planefit.cu:34-36); a zero plane gives NaN (0/0)."""
    a, b, c, d = pl
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return np.abs(a * P[:, 0] + b * P[:, 1] + c * P[:, 2] + d) / np.float64(math.sqrt(a * a + b * b + c * c))


def planefit(labels, xyz, max_label, seed, frame_id, planes17=None, trace=None):
    """S19 -> (planes [k,4], assignments [L+1] uint64, iterations run).  trace: a list that receives one dict per iteration:
    "labels" (the sampled labels that gave the local planes, in order), "local" (their number), "votes" (accepting labels of
    the winner; None when <= 3 local planes skipped the iteration), "accepted"."""
    lab = np.asarray(labels)
    h, w = lab.shape
    counts, offsets, pts = label_points(lab, xyz, max_label, PRED_PLANEFIT)
    L1 = max_label + 1
    if planes17 is None:
        planes17 = np.zeros((L1, 4))
        for l in range(L1):
            planes17[l] = ransac_plane(pts[offsets[l]:offsets[l + 1]], seed, frame_id, l)
    P64 = pts.astype(np.float64)
    valid = counts[:, 1] < 0.5 * counts[:, 0]
    npts = np.diff(offsets)
    assign = np.zeros(L1, np.uint64)
    assigned = int(valid.sum())              # planefit.cu:390-396, literally
    planes = []
    it = 0
    while assigned / float(L1) < 0.9 and it < 100:
        i = it
        it += 1
        local, sampled = [], []
        for (x, y) in sample_positions(w, h, seed, frame_id, i):
            l = int(lab[y, x])
            if assign[l] != 0 or not valid[l] or npts[l] < MIN_POINTS:
                continue
            local.append(tuple(float(v) for v in planes17[l]))
            sampled.append(l)
        step = {"labels": sampled, "local": len(local), "votes": None, "accepted": False}
        if trace is not None:
            trace.append(step)
        if len(local) <= 3:
            continue
        acc = np.zeros(len(local), np.int64)
        accepting = [[] for _ in local]
        for l in range(L1):
            if not valid[l] or assign[l] != 0:
                continue
            seg = P64[offsets[l]:offsets[l + 1]]
            for k, pl in enumerate(local):
                inl = int((fit_distance(pl, seg) < FIT_THR).sum())
                if inl > 0.5 * counts[l, 0]:
                    accepting[k].append(l)
                    acc[k] += 1
        best, bc = 0, 0
        for k in range(len(local)):
            if acc[k] > bc:
                best, bc = k, acc[k]
        step["votes"] = len(accepting[best])
        if len(accepting[best]) < 16:
            continue
        step["accepted"] = True
        planes.append(local[best])
        for l in accepting[best]:
            assign[l] = len(planes)
        assigned += len(accepting[best])
    return np.array(planes, dtype=np.float64).reshape(-1, 4), assign, it

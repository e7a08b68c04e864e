"""numpy restatement of spec S34: frame-to-model pose tracking against the TSDF volume of spec S33.  Written from the
spec on top of np_voxelmap.Map, not from the kernels: whole-image array arithmetic in the spec's operation order (every numpy ufunc rounds
once, there is no fused multiply-add), every sum in S26's two-level lane order (np_dense_ego's, reused).  scalar_sample() and
scalar_evaluate() are the same spec one pixel at a time in Python floats for cross-checking the vectorised form.  The solve and the pose
update are S23's."""
import math

import numpy as np

from np_dense_ego import LANES, NSUMS, RESULT_DTYPE, _scalar_butterfly, join, rms_of, split, two_level  # noqa: F401
from np_ego import apply_update, solve6

INVALID = -32768
MOVING = 1
# build-owned, untuned
DEFAULTS = dict(residual_gate=0.9, damping=0.01, iterations=4, stride=1, min_inliers=1024)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise ValueError(k)
        p[k] = int(v) if k in ("iterations", "stride", "min_inliers") else float(v)
    return p


# ---- the eight-corner sample with its gradient ----------------------------------------------------------------------------------
def sample(m, pw, want):
    """m = np_voxelmap.Map, pw = [x, y, z] world arrays, want = bool array -> (known, F, gx, gy, gz); entries that are not known are
    meaningless.  The sampling rule is the raycast's."""
    mp = m.p
    vs = np.float64(mp["voxel_size"])
    known = np.array(want, bool, copy=True)
    if m.origin is None:
        z = np.zeros(known.shape)
        return np.zeros(known.shape, bool), z, z, z, z
    o = [float(v) for v in m.origin]
    n = (m.nx, m.ny, m.nz)
    with np.errstate(all="ignore"):
        a = [c / vs - 0.5 for c in pw]
        i0 = [np.floor(c) for c in a]
        fr = [a[c] - i0[c] for c in range(3)]
        for c in range(3):
            known &= (i0[c] >= o[c]) & (i0[c] <= o[c] + float(n[c] - 2))                           # both corners inside; a NaN fails
        r = [np.where(known, i0[c] - o[c], 0.0).astype(np.int64) for c in range(3)]
        T = {(dz, dy, dx): m.tsdf[r[2] + dz, r[1] + dy, r[0] + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
        wmin = np.full(known.shape, 65535, np.int64)
        for key in T:
            wmin = np.minimum(wmin, m.weight[r[2] + key[0], r[1] + key[1], r[0] + key[2]])
        known &= wmin >= mp["min_weight"]
        D = {(dy, dz): (T[(dz, dy, 1)] - T[(dz, dy, 0)]).astype(np.float64) for dy in (0, 1) for dz in (0, 1)}
        cc = {k: T[(k[1], k[0], 0)].astype(np.float64) + fr[0] * D[k] for k in D}
        h0, h1 = cc[(1, 0)] - cc[(0, 0)], cc[(1, 1)] - cc[(0, 1)]
        e0 = cc[(0, 0)] + fr[1] * h0
        e1 = cc[(0, 1)] + fr[1] * h1
        gz = e1 - e0
        F = e0 + fr[2] * gz
        gy = h0 + fr[2] * (h1 - h0)
        a0 = D[(0, 0)] + fr[1] * (D[(1, 0)] - D[(0, 0)])
        a1 = D[(0, 1)] + fr[1] * (D[(1, 1)] - D[(0, 1)])
        gx = a0 + fr[2] * (a1 - a0)
    return known, F, gx, gy, gz


# ---- one pixel's terms at a pose ----------------------------------------------------------------------------------------------
def terms(m, cam, p, R, t, disp, mask=None):
    """-> (candidate [nj, ni] bool, inlier [nj, ni] bool, values [NSUMS, nj, ni]) on the sample grid at the pose (R, t)."""
    mp = m.p
    s = p["stride"]
    s_full = np.asarray(disp).astype(np.int64)
    h, w = s_full.shape
    y, x = np.mgrid[0:h:s, 0:w:s]
    sc = s_full[y, x]
    fx, fy, cx, cy = (np.float64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    fxb = fx * np.float64(cam["baseline"])
    with np.errstate(all="ignore"):
        d = sc.astype(np.float64) / 16.0
        Z = fxb / d
        ok = (sc != INVALID) & (d >= mp["min_disparity"]) & (Z >= mp["min_depth"]) & (Z <= mp["max_depth"])
        if mask is not None:
            ok &= np.asarray(mask)[y, x] != MOVING
        X = ((x.astype(np.float64) - cx) * Z) / fx
        Y = ((y.astype(np.float64) - cy) * Z) / fy
        pw = [((R[3 * r] * X + R[3 * r + 1] * Y) + R[3 * r + 2] * Z) + t[r] for r in range(3)]
        cand, F, gx, gy, gz = sample(m, pw, ok)
        res = F / 32767.0
        inl = cand & (np.abs(res) < p["residual_gate"])
        gs = np.float64(32767.0) * np.float64(mp["voxel_size"])
        G = [gx / gs, gy / gs, gz / gs]
        J = [pw[1] * G[2] - pw[2] * G[1], pw[2] * G[0] - pw[0] * G[2], pw[0] * G[1] - pw[1] * G[0], G[0], G[1], G[2]]
        vals = [J[i] * J[j] for i in range(6) for j in range(i, 6)]
        vals += [J[i] * res for i in range(6)]
        vals.append(res * res)
    return cand, inl, np.stack([np.broadcast_to(v, inl.shape) for v in vals])


def evaluate(m, cam, p, R, t, disp, mask=None):
    """-> (inliers, candidates, H 6 x 6 with the upper entries filled and undamped, g [6], sum of r r) at the pose (R, t)."""
    cand, inl, vals = terms(m, cam, p, R, t, disp, mask)
    s = [float(v) for v in two_level(vals, inl)]
    H = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = s[k]
            k += 1
    return int(inl.sum()), int(cand.sum()), H, s[21:27], s[27]


# ---- the whole call -----------------------------------------------------------------------------------------------------------
def refine(m, cam, p, pose0, disp, mask=None, evaluate=evaluate):
    """cart_model_track_refine restated -> RESULT_DTYPE [1] (the layout of cart_dense_ego_result)."""
    R, t = split(pose0)
    res = np.zeros(1, RESULT_DTYPE)
    n, _, _, _, e2 = evaluate(m, cam, p, R, t, disp, mask)
    res["n_initial"], res["rms_initial"] = n, rms_of(e2, n)
    steps = 0
    for _ in range(p["iterations"]):
        n, _, H, g, _ = evaluate(m, cam, p, R, t, disp, mask)
        if n < p["min_inliers"]:
            break
        for i in range(6):
            H[i][i] = H[i][i] + p["damping"] * float(n)
        delta = solve6(H, g)
        if delta is None:
            break
        R, t = apply_update(R, t, delta)
        steps += 1
    n, nc, _, _, e2 = evaluate(m, cam, p, R, t, disp, mask)
    res["R"][0], res["t"][0] = R, t
    res["n_candidates"], res["n_inliers"], res["rms"], res["steps"], res["status"] = nc, n, rms_of(e2, n), steps, 1 if steps > 0 else 0
    return res


def accept(res, pose0, p):
    """The consumer's rule -> (taken, the 12 doubles of the pose to use): the refined one iff status == 1, every number of the record is
    finite, rms <= rms_initial and n_inliers >= min_inliers; otherwise pose0."""
    r = res.reshape(-1)[0]
    pose = join([float(v) for v in r["R"]], [float(v) for v in r["t"]])
    nums = pose + [float(r["rms_initial"]), float(r["rms"])]
    if int(r["status"]) == 1 and all(math.isfinite(v) for v in nums) and float(r["rms"]) <= float(r["rms_initial"]) and int(r["n_inliers"]) >= p["min_inliers"]:
        return True, pose
    return False, [float(v) for v in np.asarray(pose0, np.float64).reshape(12)]


# ---- the same spec, one pixel at a time in Python floats ----------------------------------------------------------------------
def scalar_sample(m, px, py, pz):
    """-> None for an unknown sample, else (F, gx, gy, gz, fr [3], t[dz][dy][dx])."""
    if m.origin is None:
        return None
    vs = m.p["voxel_size"]
    a = [px / vs - 0.5, py / vs - 0.5, pz / vs - 0.5]
    if not all(math.isfinite(v) for v in a):
        return None
    i0 = [math.floor(v) for v in a]
    fr = [a[c] - float(i0[c]) for c in range(3)]
    n = (m.nx, m.ny, m.nz)
    for c in range(3):
        if not (m.origin[c] <= i0[c] <= m.origin[c] + n[c] - 2):
            return None
    r = [i0[c] - m.origin[c] for c in range(3)]
    T = [[[int(m.tsdf[r[2] + dz, r[1] + dy, r[0] + dx]) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                if int(m.weight[r[2] + dz, r[1] + dy, r[0] + dx]) < m.p["min_weight"]:
                    return None
    D = [[float(T[dz][dy][1] - T[dz][dy][0]) for dz in (0, 1)] for dy in (0, 1)]       # D[dy][dz]
    c = [[float(T[dz][dy][0]) + fr[0] * D[dy][dz] for dz in (0, 1)] for dy in (0, 1)]  # c[dy][dz]
    e0 = c[0][0] + fr[1] * (c[1][0] - c[0][0])
    e1 = c[0][1] + fr[1] * (c[1][1] - c[0][1])
    F = e0 + fr[2] * (e1 - e0)
    gz = e1 - e0
    h0, h1 = c[1][0] - c[0][0], c[1][1] - c[0][1]
    gy = h0 + fr[2] * (h1 - h0)
    a0 = D[0][0] + fr[1] * (D[1][0] - D[0][0])
    a1 = D[0][1] + fr[1] * (D[1][1] - D[0][1])
    gx = a0 + fr[2] * (a1 - a0)
    return F, gx, gy, gz, fr, T


def scalar_pixel(m, cam, p, R, t, disp, mask, x, y):
    """-> None for a pixel that is no candidate, else (inlier, the NSUMS values or None)."""
    mp = m.p
    fx, fy, cx, cy, base = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "baseline"))
    s = int(disp[y][x])
    d = s / 16.0
    if s == INVALID or not d >= mp["min_disparity"]:
        return None
    Z = (fx * base) / d
    if not (mp["min_depth"] <= Z <= mp["max_depth"]):
        return None
    if mask is not None and int(mask[y][x]) == MOVING:
        return None
    X = ((float(x) - cx) * Z) / fx
    Y = ((float(y) - cy) * Z) / fy
    pw = [((R[3 * r] * X + R[3 * r + 1] * Y) + R[3 * r + 2] * Z) + t[r] for r in range(3)]
    got = scalar_sample(m, *pw)
    if got is None:
        return None
    F, gx, gy, gz = got[:4]
    res = F / 32767.0
    if not abs(res) < p["residual_gate"]:
        return False, None
    gs = 32767.0 * mp["voxel_size"]
    G = [gx / gs, gy / gs, gz / gs]
    J = [pw[1] * G[2] - pw[2] * G[1], pw[2] * G[0] - pw[0] * G[2], pw[0] * G[1] - pw[1] * G[0], G[0], G[1], G[2]]
    vals = [J[i] * J[j] for i in range(6) for j in range(i, 6)]
    vals += [J[i] * res for i in range(6)]
    vals.append(res * res)
    return True, vals


def scalar_evaluate(m, cam, p, R, t, disp, mask=None):
    """-> (inliers, candidates, the NSUMS sums) by the two-level lane order, one pixel at a time."""
    h, w = np.asarray(disp).shape
    s = p["stride"]
    ni, nj = (w + s - 1) // s, (h + s - 1) // s
    count = ncand = 0
    rows = []
    for j in range(nj):
        v = [[0.0] * LANES for _ in range(NSUMS)]
        for i in range(ni):
            got = scalar_pixel(m, cam, p, R, t, disp, mask, i * s, j * s)
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

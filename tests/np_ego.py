"""CPU restatement of the stereo visual odometry stage, DESIGN.md S23 (section 7.5): triangulated landmarks, the correspondence
list, triad hypotheses with their integer scores, the arg-max, the Gauss-Newton refinement and the pose chain.

Every floating-point value is an IEEE double produced by one +, -, *, / or sqrt at a time, in the order written here; every
sum is written out (numpy's own `sum` is pairwise and is never used on floating point).  The generator is S17's
(tests/np_planefit.py)."""
import math

import numpy as np

from np_planefit import draw, stream, uniform

TAG = 3                      # stream tag of the hypothesis draws
MAX_DRAWS = 64               # draws a hypothesis may use to find three distinct indices
DEGENERATE = 1e-12
QERR_SCALE = float(1 << 24)
LANES = 256                  # virtual lanes of the refinement sums
MIN_REFINE = 6               # inliers a Gauss-Newton step needs

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                           ("class_id", "<i4")])
MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4")])
RESULT_DTYPE = np.dtype([("R", "<f8", 9), ("t", "<f8", 3), ("rms", "<f8"), ("status", "<i4"), ("n_correspondences", "<i4"),
                         ("n_inliers", "<i4"), ("best_hypothesis", "<i4")])   # cart_ego_result, 120 bytes
HYP_DTYPE = np.dtype([("qerr", "<u8"), ("count", "<i4"), ("skipped", "<i4")])   # cart_ego_hypothesis

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def camera(fx=300.0, fy=300.0, cx=160.0, cy=48.0, baseline=0.5):
    return dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), baseline=float(baseline))


def params(**over):
    p = dict(min_disparity=1.0, inlier_threshold=2.0, hypotheses=256, refine_iterations=4)
    p.update(over)
    return p


# ---- landmarks ---------------------------------------------------------------------------------------------------------
def triangulate(cam, kpL, kpR, stereo, p=None, capacity=None):
    """-> float64 [len(kpL), 4]: (X, Y, Z, valid) per left keypoint index; a stereo match whose indices lie outside the sets (or,
    with `capacity`, at or beyond it) is ignored."""
    p = p or params()
    fx, fy, cx, cy, b = (cam[k] for k in ("fx", "fy", "cx", "cy", "baseline"))
    nl = len(kpL)
    cap = capacity if capacity is not None else max(nl, len(kpR))
    out = np.zeros((nl, 4), np.float64)
    for m in stereo:
        i, j = int(m["query"]), int(m["train"])
        if not (0 <= i < nl and 0 <= j < cap and j < len(kpR)):
            continue
        xl, yl = float(kpL["x"][i]), float(kpL["y"][i])
        d = xl - float(kpR["x"][j])
        if not d >= p["min_disparity"]:
            continue
        Z = (fx * b) / d
        X = ((xl - cx) * Z) / fx
        Y = ((yl - cy) * Z) / fy
        out[i] = (X, Y, Z, 1.0)
    return out


# ---- correspondences ---------------------------------------------------------------------------------------------------
def correspondences(cur, kp_cur, prev, temporal):
    """Stable compaction of the usable temporal matches -> (a [n,3] previous points, b [n,3] current points, uv [n,2], k [n])."""
    a, b, uv, ks = [], [], [], []
    for k, m in enumerate(temporal):
        i, j = int(m["query"]), int(m["train"])
        if not (0 <= i < len(cur) and 0 <= j < len(prev)):
            continue
        if cur[i, 3] == 1.0 and prev[j, 3] == 1.0:
            a.append(prev[j, :3]); b.append(cur[i, :3])
            uv.append((float(kp_cur["x"][i]), float(kp_cur["y"][i]))); ks.append(k)
    return (np.array(a, np.float64).reshape(-1, 3), np.array(b, np.float64).reshape(-1, 3), np.array(uv, np.float64).reshape(-1, 2),
            np.array(ks, np.int64))


# ---- hypotheses --------------------------------------------------------------------------------------------------------
def sample(seed, frame_id, h, n):
    """Three distinct indices of hypothesis h, or None when MAX_DRAWS draws did not give them."""
    s = stream(seed, TAG, frame_id, h, 0)
    idx = []
    for c in range(MAX_DRAWS):
        v = uniform(draw(s, c), n)
        if v not in idx:
            idx.append(v)
            if len(idx) == 3:
                return idx
    return None


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def triad(p0, p1, p2):
    """Orthonormal frame (e1, e2, e3) of three points, or None when they are coincident or collinear."""
    u1 = tuple(p1[k] - p0[k] for k in range(3))
    u2 = tuple(p2[k] - p0[k] for k in range(3))
    l1 = _dot(u1, u1)
    if l1 <= DEGENERATE:
        return None
    s1 = math.sqrt(l1)
    e1 = tuple(u1[k] / s1 for k in range(3))
    nrm = _cross(e1, u2)
    ln = _dot(nrm, nrm)
    if ln <= DEGENERATE:
        return None
    sn = math.sqrt(ln)
    e3 = tuple(nrm[k] / sn for k in range(3))
    e2 = _cross(e3, e1)
    return e1, e2, e3


def fit_triad(A, B):
    """(R [9] row-major, t [3]) with B_k = R A_k + t for the three sample points, or None (skipped)."""
    A = [tuple(float(v) for v in p) for p in A]
    B = [tuple(float(v) for v in p) for p in B]
    E = triad(*A)
    F = triad(*B)
    if E is None or F is None:
        return None
    e1, e2, e3 = E
    f1, f2, f3 = F
    R = [(f1[r] * e1[c] + f2[r] * e2[c]) + f3[r] * e3[c] for r in range(3) for c in range(3)]
    ca = [((A[0][k] + A[1][k]) + A[2][k]) / 3.0 for k in range(3)]
    cb = [((B[0][k] + B[1][k]) + B[2][k]) / 3.0 for k in range(3)]
    t = [cb[r] - ((R[3 * r] * ca[0] + R[3 * r + 1] * ca[1]) + R[3 * r + 2] * ca[2]) for r in range(3)]
    return R, t


def transform(R, t, a):
    """q = R a + t for points a [n, 3] -> three arrays."""
    return tuple(((R[3 * r] * a[:, 0] + R[3 * r + 1] * a[:, 1]) + R[3 * r + 2] * a[:, 2]) + t[r] for r in range(3))


def residuals(cam, R, t, a, uv, thr):
    """-> (q, eu, ev, e2, inlier) per correspondence; entries of outliers with q.z <= 0 are meaningless."""
    qx, qy, qz = transform(R, t, a)
    front = ~(qz <= 0)
    with np.errstate(all="ignore"):
        eu = ((cam["fx"] * qx) / qz + cam["cx"]) - uv[:, 0]
        ev = ((cam["fy"] * qy) / qz + cam["cy"]) - uv[:, 1]
        e2 = eu * eu + ev * ev
        inl = front & (e2 < thr * thr)
    return (qx, qy, qz), eu, ev, e2, inl


def score(cam, R, t, a, uv, thr):
    """-> (count, qerr): the inliers of one hypothesis and the integer sum of their scaled squared errors."""
    _, _, _, e2, inl = residuals(cam, R, t, a, uv, thr)
    q = np.floor((e2[inl] / (thr * thr)) * QERR_SCALE)
    return int(inl.sum()), int(sum(int(v) for v in q))


def hypotheses(cam, p, a, b, uv, seed, frame_id):
    """-> (table HYP_DTYPE [H], poses: list of (R, t) or None)."""
    H, n = p["hypotheses"], len(a)
    table = np.zeros(H, HYP_DTYPE)
    poses = [None] * H
    for h in range(H):
        idx = sample(seed, frame_id, h, n) if n >= 3 else None
        fit = fit_triad(a[idx], b[idx]) if idx is not None else None
        if fit is None:
            table[h]["skipped"] = 1
            continue
        poses[h] = fit
        c, q = score(cam, fit[0], fit[1], a, uv, p["inlier_threshold"])
        table[h]["count"], table[h]["qerr"] = c, q
    return table, poses


def best_hypothesis(table):
    """max (count, -qerr, -h) over the hypotheses that were not skipped and have count >= 3; -1 without one."""
    best = -1
    for h in range(len(table)):
        if table[h]["skipped"] or table[h]["count"] < 3:
            continue
        if best < 0 or (int(table[h]["count"]), -int(table[h]["qerr"])) > (int(table[best]["count"]), -int(table[best]["qerr"])):
            best = h
    return best


# ---- refinement --------------------------------------------------------------------------------------------------------
def lane_sum(values, mask):
    """Σ values[mask] in the fixed order: virtual lane l adds its entries l, l + 256, ... in ascending order (entries outside
    the mask are skipped), then v[l] += v[l ^ o] for o = 128 .. 1; lane 0's value."""
    v = np.zeros(LANES, np.float64)
    for c0 in range(0, len(values), LANES):        # one round of all lanes at a time: element-wise, so the order per lane is kept
        m = np.asarray(mask[c0:c0 + LANES], bool)
        part = v[:len(m)]
        with np.errstate(all="ignore"):
            v[:len(m)] = np.where(m, part + np.where(m, values[c0:c0 + LANES], 0.0), part)
    lanes = np.arange(LANES)
    o = LANES // 2
    while o:
        v = v + v[lanes ^ o]
        o //= 2
    return float(v[0])


def jacobian(cam, q):
    """Rows of d(eu, ev) / d(omega, upsilon) at q = (qx, qy, qz) arrays -> (Ju [6], Jv [6]) lists of arrays."""
    qx, qy, qz = q
    zero = np.zeros_like(qx)
    with np.errstate(all="ignore"):
        au = cam["fx"] / qz
        bu = -((cam["fx"] * qx) / (qz * qz))
        av = cam["fy"] / qz
        bv = -((cam["fy"] * qy) / (qz * qz))
        Ju = [bu * qy, au * qz - bu * qx, -(au * qy), au, zero, bu]
        Jv = [bv * qy - av * qz, -(bv * qx), av * qx, zero, av, bv]
    return Ju, Jv


def solve6(Hm, g):
    """Unpivoted Cholesky of the symmetric 6 x 6 Hm (upper entries used), right-hand side -g; None at a pivot that is not > 0."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = Hm[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = Hm[j][i]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        s = -g[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def quat_rotation(w3):
    """Rotation matrix [9] of the unit quaternion (1, w3 / 2) / |(1, w3 / 2)|."""
    hx, hy, hz = 0.5 * w3[0], 0.5 * w3[1], 0.5 * w3[2]
    s = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    w, x, y, z = 1.0 / s, hx / s, hy / s, hz / s
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def apply_update(R, t, delta):
    Rq = quat_rotation(delta[:3])
    Rn = [(Rq[3 * r] * R[c] + Rq[3 * r + 1] * R[3 + c]) + Rq[3 * r + 2] * R[6 + c] for r in range(3) for c in range(3)]
    tn = [((Rq[3 * r] * t[0] + Rq[3 * r + 1] * t[1]) + Rq[3 * r + 2] * t[2]) + delta[3 + r] for r in range(3)]
    return Rn, tn


def normal_equations(cam, R, t, a, uv, thr):
    """-> (inlier count, Hm 6 x 6 with the upper entries filled, g [6]) at the pose (R, t)."""
    q, eu, ev, _, inl = residuals(cam, R, t, a, uv, thr)
    Ju, Jv = jacobian(cam, q)
    Hm = [[0.0] * 6 for _ in range(6)]
    g = [0.0] * 6
    with np.errstate(all="ignore"):
        for i in range(6):
            for j in range(i, 6):
                Hm[i][j] = lane_sum(Ju[i] * Ju[j] + Jv[i] * Jv[j], inl)
            g[i] = lane_sum(Ju[i] * eu + Jv[i] * ev, inl)
    return int(inl.sum()), Hm, g


def refine(cam, p, R, t, a, uv):
    thr = p["inlier_threshold"]
    for _ in range(p["refine_iterations"]):
        cnt, Hm, g = normal_equations(cam, R, t, a, uv, thr)
        if cnt < MIN_REFINE:
            break
        delta = solve6(Hm, g)
        if delta is None:
            break
        R, t = apply_update(R, t, delta)
    return R, t


# ---- the whole call ----------------------------------------------------------------------------------------------------
def estimate(cam, p, cur, kp_cur, prev, temporal, seed=0, frame_id=0, capacity=None):
    """-> (result RESULT_DTYPE [1], mask int32 [capacity or len(temporal)], table HYP_DTYPE [H])."""
    a, b, uv, ks = correspondences(cur, kp_cur, prev, temporal)
    table, poses = hypotheses(cam, p, a, b, uv, seed, frame_id)
    res = np.zeros(1, RESULT_DTYPE)
    mask = np.zeros(capacity if capacity is not None else len(temporal), np.int32)
    res["R"][0], res["n_correspondences"], res["best_hypothesis"] = IDENTITY, len(a), -1
    best = best_hypothesis(table)
    if best < 0:
        return res, mask, table
    R, t = refine(cam, p, poses[best][0], poses[best][1], a, uv)
    _, _, _, e2, inl = residuals(cam, R, t, a, uv, p["inlier_threshold"])
    n_in = int(inl.sum())
    res["R"][0], res["t"][0] = R, t
    res["rms"] = math.sqrt(lane_sum(e2, inl) / n_in) if n_in else 0.0
    res["status"], res["n_inliers"], res["best_hypothesis"] = 1, n_in, best
    mask[ks[inl]] = 1
    return res, mask, table


# ---- the pose chain (host side of the ego_motion module) ---------------------------------------------------------------
def chain(pose, res):
    """T_w(t) = T_w(t-1) inv(T_rel), inv = (R^T, -R^T t); pose = 12 doubles, a 3 x 4 in row order.  status 0 keeps the pose."""
    if not int(res["status"][0]):
        return list(pose)
    R, t = [float(v) for v in res["R"][0]], [float(v) for v in res["t"][0]]
    Ri = [R[3 * c + r] for r in range(3) for c in range(3)]
    ti = [-((Ri[3 * r] * t[0] + Ri[3 * r + 1] * t[1]) + Ri[3 * r + 2] * t[2]) for r in range(3)]
    out = [0.0] * 12
    for r in range(3):
        for c in range(3):
            out[4 * r + c] = (pose[4 * r] * Ri[c] + pose[4 * r + 1] * Ri[3 + c]) + pose[4 * r + 2] * Ri[6 + c]
        out[4 * r + 3] = ((pose[4 * r] * ti[0] + pose[4 * r + 1] * ti[1]) + pose[4 * r + 2] * ti[2]) + pose[4 * r + 3]
    return out


POSE_IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]

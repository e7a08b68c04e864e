"""CPU restatement of the ORB feature stage, DESIGN.md S20 (pure numpy / Python integers, exact).

S20 follows the structure and defaults of cv::cuda::ORB::create(5000) as the reference's ImageFeatureDetectorModule
calls it (src/modules/features.cpp:48-66): an image pyramid (scale 1.2, 8 levels), FAST-9 (threshold 20) with 3x3
non-maximum suppression, the Harris score, a per-level top-n_l selection, the intensity-centroid orientation and a
steered BRIEF descriptor of 256 pairs.  Every choice that cv::cuda::ORB leaves to chance (atomic append order, unstable
sorts, fastAtan2) is fixed here; see DESIGN.md §7.2 for the deviations.
"""
import numpy as np

import np_planefit as PF
import oracle_lib as O

N_DEFAULT = 5000           # CARTSLAM_OPTION_KEYPOINTS, features.hpp:11
N_LEVELS = 8
SCALE = 1.2
EDGE = 31                  # edge threshold = patch size
FAST_T = 20
MIN_LEVEL = 2 * EDGE + 1   # a level is built while w_l, h_l >= 63 (non-empty inner region)
RESPONSE_SCALE = 64972990404000000.0   # 25 * 7140^4
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])

# FAST-9 circle of radius 3 as (dx, dy), OpenCV's order
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))

# 2^20 fixed point, rounded half away from zero: boundary rays B_j at (12j + 6) degrees, steering (C_k, S_k) at 12k degrees
BOUNDARY = ((1042832, 109606), (997255, 324028), (908093, 524288), (779244, 701634), (616338, 848316), (426494, 957922),
            (218011, 1025662), (0, 1048576), (-218011, 1025662), (-426494, 957922), (-616338, 848316), (-779244, 701634),
            (-908093, 524288), (-997255, 324028), (-1042832, 109606), (-1042832, -109606), (-997255, -324028),
            (-908093, -524288), (-779244, -701634), (-616338, -848316), (-426494, -957922), (-218011, -1025662),
            (0, -1048576), (218011, -1025662), (426494, -957922), (616338, -848316), (779244, -701634), (908093, -524288),
            (997255, -324028), (1042832, -109606))
STEER = ((1048576, 0), (1025662, 218011), (957922, 426494), (848316, 616338), (701634, 779244), (524288, 908093),
         (324028, 997255), (109606, 1042832), (-109606, 1042832), (-324028, 997255), (-524288, 908093), (-701634, 779244),
         (-848316, 616338), (-957922, 426494), (-1025662, 218011), (-1048576, 0), (-1025662, -218011), (-957922, -426494),
         (-848316, -616338), (-701634, -779244), (-524288, -908093), (-324028, -997255), (-109606, -1042832),
         (109606, -1042832), (324028, -997255), (524288, -908093), (701634, -779244), (848316, -616338),
         (957922, -426494), (1025662, -218011))


# ---- sizes and quotas -------------------------------------------------------------------------------------------------
def level_quotas(n):
    """n_0..n_7 of N = n features (cv::cuda::ORB's nfeaturesPerLevel, with the last level's underflow clipped)."""
    f = 1.0 / SCALE
    f8 = 1.0
    for _ in range(N_LEVELS):
        f8 *= f
    nd = n * (1.0 - f) / (1.0 - f8)
    out, s = [], 0
    for _ in range(N_LEVELS - 1):
        q = min(int(np.rint(nd)), n - s)
        out.append(q)
        s += q
        nd *= f
    out.append(n - s)
    return out


def level_sizes(w, h):
    """-> [(w_l, h_l, s_l)] for all 8 levels (built or not)."""
    out, s = [], 1.0
    for _ in range(N_LEVELS):
        out.append((int(np.rint(w / s)), int(np.rint(h / s)), s))
        s *= SCALE
    return out


def built_levels(w, h):
    n = 0
    for lw, lh, _ in level_sizes(w, h):
        if lw < MIN_LEVEL or lh < MIN_LEVEL:
            break
        n += 1
    return n


def pyramid(img):
    """Level images (uint8) of the built levels; a 3-channel input is converted by S1 gray first."""
    img = np.ascontiguousarray(img, np.uint8)
    g = O.bgr2gray(img) if img.ndim == 3 else img
    h, w = g.shape
    levels = []
    for lw, lh, _ in level_sizes(w, h)[:built_levels(w, h)]:
        g = g if not levels else O.resize_linear(levels[-1], lw, lh)
        levels.append(g)
    return levels


# ---- detection ----------------------------------------------------------------------------------------------------------
def fast_scores(img):
    """FAST-9 score of every candidate pixel (int32 [h, w]); 0 = not a corner or not a candidate."""
    I = img.astype(np.int32)
    h, w = I.shape
    out = np.zeros((h, w), np.int32)
    if w < MIN_LEVEL or h < MIN_LEVEL:
        return out
    ys, xs = slice(EDGE, h - EDGE), slice(EDGE, w - EDGE)
    c = I[ys, xs]
    d = np.stack([I[EDGE + dy:h - EDGE + dy, EDGE + dx:w - EDGE + dx] - c for dx, dy in CIRCLE])
    best = np.full(c.shape, np.iinfo(np.int32).min, np.int32)
    for k in range(16):
        arc = d[[(k + j) & 15 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), -arc.max(0)))
    score = best - 1
    out[ys, xs] = np.where(score >= FAST_T, score, 0)
    return out


def nms(scores):
    """Strict 3x3 non-maximum suppression: mask of corners above each of their 8 neighbours."""
    h, w = scores.shape
    p = np.zeros((h + 2, w + 2), np.int32)
    p[1:-1, 1:-1] = scores
    keep = scores > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= scores > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep


def gradients(img):
    """Ix, Iy of OpenCV ORB's HarrisResponses at every pixel with a full 3x3 neighbourhood (0 on the 1-pixel border)."""
    I = img.astype(np.int64)
    h, w = I.shape
    Ix = np.zeros((h, w), np.int64)
    Iy = np.zeros((h, w), np.int64)
    Ix[1:-1, 1:-1] = (2 * (I[1:-1, 2:] - I[1:-1, :-2]) + (I[:-2, 2:] - I[:-2, :-2]) + (I[2:, 2:] - I[2:, :-2]))
    Iy[1:-1, 1:-1] = (2 * (I[2:, 1:-1] - I[:-2, 1:-1]) + (I[2:, :-2] - I[:-2, :-2]) + (I[2:, 2:] - I[:-2, 2:]))
    return Ix, Iy


def harris(img, ys, xs):
    """R = 25 (ab - c^2) - (a + b)^2 (int64) over the 7x7 window at each (y, x)."""
    Ix, Iy = gradients(img)
    R = np.zeros(len(ys), np.int64)
    a = np.zeros(len(ys), np.int64)
    b = np.zeros(len(ys), np.int64)
    c = np.zeros(len(ys), np.int64)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            gx, gy = Ix[ys + dy, xs + dx], Iy[ys + dy, xs + dx]
            a += gx * gx
            b += gy * gy
            c += gx * gy
    R = 25 * (a * b - c * c) - (a + b) * (a + b)
    return R


def detect_level(img):
    """-> survivors of a level as (R, y, x) arrays, unordered."""
    keep = nms(fast_scores(img))
    ys, xs = np.nonzero(keep)
    return harris(img, ys, xs), ys.astype(np.int64), xs.astype(np.int64)


def select(R, ys, xs, n):
    """The first n survivors under (R descending, y ascending, x ascending)."""
    order = np.lexsort((xs, ys, -R))[:n]
    return R[order], ys[order], xs[order]


# ---- orientation and descriptor -----------------------------------------------------------------------------------------
def patch_offsets():
    """(u, v) of the circular patch of half-size 15, row by row."""
    pts = [(u, v) for v in range(-15, 16) for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1)]
    return np.array(pts, np.int64)


def moments(img, ys, xs):
    off = patch_offsets()
    I = img.astype(np.int64)
    vals = I[np.asarray(ys)[:, None] + off[None, :, 1], np.asarray(xs)[:, None] + off[None, :, 0]]
    return (vals * off[None, :, 0]).sum(1), (vals * off[None, :, 1]).sum(1)


def orientation_bin(m10, m01):
    """The k in 0..29 with cross(B_{k-1}, m) >= 0 and cross(B_k, m) < 0; 0 for m = 0 (int64 arithmetic)."""
    m10 = np.asarray(m10, np.int64)
    m01 = np.asarray(m01, np.int64)
    B = np.array(BOUNDARY, np.int64)
    cr = B[:, 0][None, :] * m01[:, None] - B[:, 1][None, :] * m10[:, None]   # [n, 30]
    hit = (np.roll(cr, 1, axis=1) >= 0) & (cr < 0)
    k = np.argmax(hit, axis=1)
    zero = (m10 == 0) & (m01 == 0)
    assert (hit.sum(1)[~zero] == 1).all()
    return np.where(zero, 0, k)


def pattern():
    """256 pairs (px, py, qx, qy) in [-13, 13], drawn from the S17 counter stream with tag 3."""
    out = []
    for i in range(256):
        a = 0
        while True:
            s = PF.stream(0, 3, i, a, 0)
            idx = [PF.uniform(PF.draw(s, c), 27) for c in range(16)]
            coords = [(sum(idx[4 * t:4 * t + 4]) + 2) // 4 - 13 for t in range(4)]
            if coords[:2] != coords[2:]:
                out.append(coords)
                break
            a += 1
    return np.array(out, np.int64)


def rnd20(v):
    """sgn(v) * ((|v| + 2^19) >> 20)"""
    v = np.asarray(v, np.int64)
    return np.sign(v) * ((np.abs(v) + (1 << 19)) >> 20)


def steered_pattern():
    """[30, 256, 4] pattern rotated by 12k degrees."""
    P = pattern()
    out = np.zeros((30, 256, 4), np.int64)
    for k, (C, S) in enumerate(STEER):
        for t in (0, 2):
            x, y = P[:, t], P[:, t + 1]
            out[k, :, t] = rnd20(x * C - y * S)
            out[k, :, t + 1] = rnd20(x * S + y * C)
    return out


_STEERED = None


def descriptors(img, ys, xs, bins):
    global _STEERED
    if _STEERED is None:
        _STEERED = steered_pattern()
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    sp = _STEERED[np.asarray(bins, np.int64)]          # [n, 256, 4]
    I = img.astype(np.int32)
    p = I[ys[:, None] + sp[:, :, 1], xs[:, None] + sp[:, :, 0]]
    q = I[ys[:, None] + sp[:, :, 3], xs[:, None] + sp[:, :, 2]]
    bits = (p < q).astype(np.uint8).reshape(-1, 32, 8)
    return (bits << np.arange(8, dtype=np.uint8)).sum(2).astype(np.uint8)


# ---- the whole stage ----------------------------------------------------------------------------------------------------
def orb(img, nfeatures=N_DEFAULT, want_levels=False):
    """-> (keypoints structured [n] KEYPOINT_DTYPE, descriptors uint8 [n, 32]) in output order; with want_levels also
    (level images, survivor counts per built level)."""
    levels = pyramid(img)
    h, w = levels[0].shape if levels else np.asarray(img).shape[:2]
    sizes = level_sizes(w, h)
    quotas = level_quotas(nfeatures)
    kps, descs, counts = [], [], []
    for l, L in enumerate(levels):
        R, ys, xs = detect_level(L)
        counts.append(len(R))
        R, ys, xs = select(R, ys, xs, quotas[l])
        m10, m01 = moments(L, ys, xs)
        k = orientation_bin(m10, m01)
        s = np.float32(sizes[l][2])
        kp = np.zeros(len(R), KEYPOINT_DTYPE)
        kp["x"] = xs.astype(np.float32) * s
        kp["y"] = ys.astype(np.float32) * s
        kp["size"] = np.float32(31.0) * s
        kp["angle"] = np.float32(12.0) * k.astype(np.float32)
        kp["response"] = (R.astype(np.float64) / RESPONSE_SCALE).astype(np.float32)
        kp["octave"] = l
        kp["class_id"] = -1
        kps.append(kp)
        descs.append(descriptors(L, ys, xs, k))
    kp = np.concatenate(kps) if kps else np.zeros(0, KEYPOINT_DTYPE)
    de = np.concatenate(descs) if descs else np.zeros((0, 32), np.uint8)
    if want_levels:
        return kp, de, levels, counts
    return kp, de

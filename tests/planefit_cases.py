"""Inputs of the planefit layout tests (test_gpu_planefit_layout.py) with what the restatement (np_planefit.py) says about them.

Everything here is numpy: the GPU tests take the inputs and the expected values from here, and test_planefit_cases.py checks on a CPU
that every case is what its name says (the premises), so that a case cannot turn trivial unnoticed.  Expected values are computed once
per process (functools.lru_cache) and must not be changed by the tests that share them.
"""
import functools

import numpy as np

import np_planefit as N

SIZES = [(67, 37), (130, 33), (257, 37)]      # no width is a multiple of 64: 64-pixel chunks straddle rows; 2, 5 and 10 tiles of 1024 pixels
ZERO = (0.0, 0.0, 0.0, 0.0)


def block_labels(w, h, bs):
    nbx = (w + bs - 1) // bs
    return ((np.arange(h)[:, None] // bs) * nbx + np.arange(w)[None, :] // bs).astype(np.uint16), nbx * ((h + bs - 1) // bs) - 1


# ---- section 1: one scene per size -------------------------------------------------------------------------------------------
def road_wall(w, h, rng, split=0.55, noise=0.002):
    """xyz float64 [h, w, 3]: the road y = 1.6 left of `split`, the wall x = 3 right of it, Gaussian noise."""
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    u0 = int(split * w)
    wall = u >= u0
    xyz = np.zeros((h, w, 3))
    xyz[..., 0] = np.where(wall, 3.0, (u - w / 2) / (w / 8.0))
    xyz[..., 1] = np.where(wall, 1.6 - (h - v) / (h / 3.0), 1.6)
    xyz[..., 2] = np.where(wall, 5.0 + (u - u0) / 4.0, 3.0 + 30.0 * v / h)
    return xyz + rng.normal(0, noise, xyz.shape), wall


@functools.lru_cache(maxsize=None)
def layout_scene(w, h):
    """-> (labels u16, xyz f32, max_label): blocks of 8 (every label with up to 64 points), a third of the regions mostly invalid (so
    that the S19 loop runs), scattered NaN / inf / z <= 0 / z > 40 holes.  Label 1 and the point OFF (valid z, far off both planes) fill
    the input slack of the layout tests: label 1 is used by the image, and reading OFF would move label 1's counts, points and plane."""
    rng = np.random.default_rng(1000 * w + h)
    lab, mx = block_labels(w, h, 8)
    xyz, _ = road_wall(w, h, rng)
    xyz = xyz.astype(np.float32)
    z = xyz[..., 2]
    for val, frac in ((np.nan, 0.03), (np.inf, 0.01), (-np.inf, 0.01), (0.0, 0.01), (-2.0, 0.01), (55.0, 0.02)):
        z[rng.random((h, w)) < frac] = val
    bad = rng.random(mx + 1) < 0.35
    bad[1] = False
    z[bad[lab] & (rng.random((h, w)) < 0.8)] = np.nan
    return lab, xyz, mx


SLACK_LABEL = 1
OFF = (11.0, 11.0, 11.0)      # the xyz slack holds 11.0 throughout: a valid z, 9.4 off the road and 8 off the wall


@functools.lru_cache(maxsize=None)
def layout_expected(w, h, pred, seed=3, frame=5):
    lab, xyz, mx = layout_scene(w, h)
    planes, npts, counts, off, pts = N.label_planes(lab, xyz, mx, pred, seed, frame)
    aoff, anb = N.adjacency(lab, mx)
    out = dict(planes=planes, npts=npts, counts=counts, off=off, pts=pts, aoff=aoff, anb=anb, seed=seed, frame=frame, mx=mx)
    if pred == N.PRED_PLANEFIT:
        trace = []
        out["fit"] = N.planefit(lab, xyz, mx, seed, frame, planes17=planes, trace=trace)
        out["trace"] = trace
    return out


# ---- section 2: label-count boundaries, point-count boundaries, RANSAC inputs -------------------------------------------------
L1_VALUES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2080, 16384]
BW, BH = 130, 33      # the image of sections 2 to 4


@functools.lru_cache(maxsize=None)
def sparse_case(L1):
    """The 130 x 33 image in blocks of 4 x 3 pixels (11 rows of 33 blocks, 12 pixels each: no block reaches 16 points) with the blocks
    mapped onto sparse ids in [0, L1) that always hold 0 and L1 - 1.  With fewer ids than blocks the ids repeat (labels in several pieces).
    With L1 >= 2049 the block rows 4 to 6 hold ids >= 2048 only, except every second block of row 5: those have all their neighbours at
    or above 2048, and the blocks of rows 3 and 7 have neighbours on both sides of 2048.  The label of the first block is painted over
    2 x 40 pixels more, so that one label has a plane."""
    rng = np.random.default_rng(L1)
    by, bx = np.arange(BH)[:, None] // 3, np.arange(BW)[None, :] // 4
    blk = by * 33 + bx
    if L1 >= 2049:
        row, col = np.arange(363) // 33, np.arange(363) % 33
        high = (row >= 4) & (row <= 6) & ~((row == 5) & (col % 2 == 1))
        pool_hi = np.arange(2048, L1 - 1)
        hi = np.concatenate([[L1 - 1], rng.choice(pool_hi, min(len(pool_hi), int(high.sum()) - 1), replace=False)]).astype(np.int64)
        lo = np.concatenate([[0], rng.choice(np.arange(1, 2048), int((~high).sum()) - 1, replace=False)])
        ids = np.zeros(363, np.int64)
        ids[high] = rng.permutation(hi)[np.arange(int(high.sum())) % len(hi)]
        ids[~high] = rng.permutation(lo)
    else:
        n = min(L1, 363)
        inner = rng.choice(np.arange(1, L1 - 1), n - 2, replace=False).tolist() if n > 2 else []
        base = np.array(([0] + inner + [L1 - 1])[:n] if L1 > 1 else [0])
        ids = rng.permutation(base)[np.arange(363) % n]
    lab = ids[blk].astype(np.uint16)
    lab[30:32, 5:45] = lab[0, 0]
    xyz, _ = road_wall(BW, BH, rng)
    return lab, xyz.astype(np.float32), L1 - 1


@functools.lru_cache(maxsize=None)
def sparse_expected(L1, seed=2, frame=9):
    lab, xyz, mx = sparse_case(L1)
    counts, off, pts = N.label_points(lab, xyz, mx, N.PRED_PLANEFIT)
    planes = np.zeros((L1, 4))
    for l in np.nonzero(np.diff(off) >= N.MIN_POINTS)[0]:
        planes[l] = N.ransac_plane(pts[off[l]:off[l + 1]], seed, frame, int(l))
    aoff, anb = N.adjacency(lab, mx)
    return dict(planes=planes, npts=np.diff(off), counts=counts, off=off, pts=pts, aoff=aoff, anb=anb, seed=seed, frame=frame, mx=mx)


POINT_COUNTS = [15, 16, 1023, 1024, 1025]


@functools.lru_cache(maxsize=None)
def point_count_case(n):
    """Label 7 painted over whole rows of the 130-wide image plus a partial row, n + 3 pixels of which 3 are invalid: n valid points.
    The rest of the image is blocks of 4 x 3 (12 points: zero planes) with ids 8..370."""
    rng = np.random.default_rng(n)
    lab = ((np.arange(BH)[:, None] // 3) * 33 + np.arange(BW)[None, :] // 4 + 8).astype(np.uint16)
    flat = lab.reshape(-1)
    flat[BW * 2:BW * 2 + n + 3] = 7
    xyz, _ = road_wall(BW, BH, rng, split=2.0)      # the road alone
    xyz = xyz.astype(np.float32)
    z = xyz.reshape(-1, 3)[:, 2]
    z[BW * 2 + np.array([1, n // 2, n + 1])] = (np.nan, -1.0, 41.0)
    return lab, xyz, 370


@functools.lru_cache(maxsize=None)
def point_count_expected(n, seed=4, frame=2):
    lab, xyz, mx = point_count_case(n)
    counts, off, pts = N.label_points(lab, xyz, mx, N.PRED_PLANEFIT)
    planes = np.zeros((mx + 1, 4))
    planes[7] = N.ransac_plane(pts[off[7]:off[8]], seed, frame, 7)
    return dict(planes=planes, npts=np.diff(off), counts=counts, off=off, pts=pts, seed=seed, frame=frame, mx=mx)


RANSAC_LABELS = dict(identical=3, collinear=5, noisy=6, nonfinite=9, nanz=11)


@functools.lru_cache(maxsize=None)
def ransac_case():
    """130 x 33 in blocks of 10 x 11 (13 x 3 = 39 labels of up to 110 points on the road, noise 0.002), with five labels rewritten:
      identical  every valid point the same point
      collinear  points on one line: every hypothesis is degenerate
      noisy      noise 0.05: under thr = 1e-7 no hypothesis has an inlier (not even its own four points), at 0.01 and 0.05 the inlier sets differ
      nonfinite  a NaN, a +inf and a -inf in x or y beside a valid z
      nanz       NaN z in a quarter of the label: points under PLANECLUSTER, invalid under PLANEFIT"""
    rng = np.random.default_rng(77)
    lab = ((np.arange(BH)[:, None] // 11) * 13 + np.arange(BW)[None, :] // 10).astype(np.uint16)
    xyz, _ = road_wall(BW, BH, rng, split=2.0)
    m = lab == RANSAC_LABELS["identical"]
    xyz[m] = (0.5, 1.6, 7.25)
    m = lab == RANSAC_LABELS["collinear"]
    t = rng.integers(0, 64, int(m.sum())) / 8.0
    xyz[m] = np.stack([t, 2 * t, 1 + t], 1)      # dyadic: exact in float32, the moments of four of them have all determinants <= 0
    m = lab == RANSAC_LABELS["noisy"]
    xyz[m] += rng.normal(0, 0.05, (int(m.sum()), 3))
    xyz = xyz.astype(np.float32)
    ys, xs = np.nonzero(lab == RANSAC_LABELS["nonfinite"])
    xyz[ys[3], xs[3], 0] = np.nan; xyz[ys[17], xs[17], 1] = np.inf; xyz[ys[40], xs[40], 0] = -np.inf
    ys, xs = np.nonzero(lab == RANSAC_LABELS["nanz"])
    xyz[ys[::4], xs[::4], 2] = np.nan
    return lab, xyz, 38


RANSAC_RUNS = [(N.PRED_PLANEFIT, 0.01), (N.PRED_PLANECLUSTER, 0.01), (N.PRED_PLANEFIT, 0.05), (N.PRED_PLANEFIT, 1e-7)]


@functools.lru_cache(maxsize=None)
def ransac_expected(pred, thr, seed=6, frame=3):
    lab, xyz, mx = ransac_case()
    counts, off, pts = N.label_points(lab, xyz, mx, pred)
    planes, best = np.zeros((mx + 1, 4)), {}
    for l in range(mx + 1):
        planes[l], best[l] = N.ransac_plane(pts[off[l]:off[l + 1]], seed, frame, l, thr, return_best=True)
    return dict(planes=planes, best=best, npts=np.diff(off), counts=counts, off=off, pts=pts, seed=seed, frame=frame, mx=mx)


# ---- section 3: labels above max_label ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def above_case():
    """The 130 x 33 layout scene (blocks of 8: ids 0..84) read with max_label 59: the ids 60..84 (the last block row and a half) are out of range."""
    lab, xyz, mx = layout_scene(BW, BH)
    return lab, xyz, 59, mx


@functools.lru_cache(maxsize=None)
def above_expected(seed=1, frame=4):
    lab, xyz, low, mx = above_case()
    planes, npts, counts, off, pts = N.label_planes(lab, xyz, low, N.PRED_PLANEFIT, seed, frame)
    aoff, anb = N.adjacency(lab, low)
    return dict(planes=planes, npts=npts, counts=counts, off=off, pts=pts, aoff=aoff, anb=anb, seed=seed, frame=frame, mx=low)


# ---- section 4: one object, many calls ----------------------------------------------------------------------------------------
REUSE_STEPS = [(16383, N.PRED_PLANEFIT), (63, N.PRED_PLANECLUSTER), (2080, N.PRED_PLANEFIT), (0, N.PRED_PLANECLUSTER)]


@functools.lru_cache(maxsize=None)
def reuse_case(k):
    """Step k of the reuse sequence -> (labels, xyz, max_label, predicate).  16383 and 2080: the sparse images; 63: blocks of 17 x 9 (32 ids)
    mapped onto ids up to 63; 0: one label.  Different images, point counts and label counts every time."""
    mx, pred = REUSE_STEPS[k]
    if mx in (16383, 2080):
        lab, xyz, _ = sparse_case(mx + 1)
        return lab, xyz, mx, pred
    rng = np.random.default_rng(40 + k)
    xyz, _ = road_wall(BW, BH, rng)
    xyz = xyz.astype(np.float32)
    xyz[..., 2][rng.random((BH, BW)) < 0.1] = -1.0      # invalid under both predicates: the point count differs from that of the sparse images
    if mx == 0:
        return np.zeros((BH, BW), np.uint16), xyz, 0, pred
    blk = (np.arange(BH)[:, None] // 9) * 8 + np.arange(BW)[None, :] // 17
    ids = np.concatenate([[0, 63], rng.permutation(np.arange(1, 63))])[:32]
    return rng.permutation(ids)[blk].astype(np.uint16), xyz, 63, pred


@functools.lru_cache(maxsize=None)
def reuse_expected(k):
    lab, xyz, mx, pred = reuse_case(k)
    seed, frame = 10 + k, 20 + k
    planes, npts, counts, off, pts = N.label_planes(lab, xyz, mx, pred, seed, frame)
    aoff, anb = N.adjacency(lab, mx)
    out = dict(planes=planes, npts=npts, counts=counts, off=off, pts=pts, aoff=aoff, anb=anb, seed=seed, frame=frame, mx=mx)
    if pred == N.PRED_PLANEFIT:
        out["fit"] = N.planefit(lab, xyz, mx, seed, frame, planes17=planes)
    return out


# ---- section 5: the S19 loop ----------------------------------------------------------------------------------------------------
def fit_scene(w, h, bs, invalid, seed, third=False, collinear=False, both=False):
    """Two-plane block scene: road and wall (noise 0.002), whole regions invalid (NaN z) with probability `invalid`.
    third = (c, extra): a slanted third plane over block column c and `extra` blocks of the next (all its regions valid); collinear: valid regions (a list of labels) of collinear points: their S17 plane is zero; both: valid regions whose points lie where road
    and wall meet (x = 3, y = 1.6): they accept either plane, so the second plane must skip them once the first one has them."""
    rng = np.random.default_rng(seed)
    lab, mx = block_labels(w, h, bs)
    nbx = (w + bs - 1) // bs
    split = (int(0.55 * nbx) * bs + 0.5) / w      # the wall starts on a block border
    xyz, _ = road_wall(w, h, rng, split=split)
    bad = rng.random(mx + 1) < invalid
    if third:
        v, u = np.mgrid[0:h, 0:w].astype(np.float64)
        c, extra = third      # block column c and the first `extra` blocks of column c + 1
        col = ((lab % nbx) == c) | (((lab % nbx) == c + 1) & (lab // nbx < extra))
        xyz[col] = np.stack([u[col] / w - 2, v[col] / h - 1, 9 + 0.5 * (u[col] / w - 2) + 0.25 * (v[col] / h - 1)], 1) + rng.normal(0, 0.002, (int(col.sum()), 3))
        bad[np.unique(lab[col])] = False
    if collinear:
        for l in collinear:
            m = lab == l
            t = rng.integers(0, 64, int(m.sum())) / 8.0
            xyz[m] = np.stack([t, 2 * t, 1 + t], 1)
            bad[l] = False
    if both:
        for l in both:
            m = lab == l
            k = int(m.sum())
            xyz[m] = np.stack([np.full(k, 3.0), np.full(k, 1.6), rng.uniform(5, 9, k)], 1) + rng.normal(0, 0.002, (k, 3))
            bad[l] = False
    xyz = xyz.astype(np.float32)
    xyz[..., 2][bad[lab]] = np.nan
    return lab, xyz, mx


def accepts(lab, xyz, max_label, plane, label):
    """Would `label` accept `plane` in S19: more than half of its pixels are valid points within 0.02 of it."""
    counts, off, pts = N.label_points(lab, xyz, max_label, N.PRED_PLANEFIT)
    seg = pts[off[label]:off[label + 1]].astype(np.float64)
    return int((N.fit_distance(tuple(float(v) for v in plane), seg) < N.FIT_THR).sum()) > 0.5 * counts[label, 0]


COLLINEAR = (104, 103, 105, 80, 128, 110, 134, 86)      # blocks around the sampling grid's cells (96 x 40, blocks of 4)
BOTH = (30, 60, 100, 140)
# name -> (w, h, block, invalid fraction, generator seed, scene options, fit seed, frame id)
FIT_CASES = {
    "all_valid":        (96, 40, 4, 0.05, 0, {}, 0, 1),                          # >= 90 % valid regions: no iteration
    "one_iteration":    (192, 80, 8, 0.30, 0, {}, 0, 1),                         # one plane, the count passes 90 %: the loop ends after one iteration
    "early_end":        (130, 67, 6, 0.50, 0, {}, 0, 1),                         # two planes, ends after two iterations
    "cap_96":           (96, 40, 4, 0.65, 0, {}, 0, 1),                          # two planes (the second in iteration 9), runs to the cap of 100
    "cap_96_reseeded":  (96, 40, 4, 0.65, 0, {}, 9, 3),                          # the same scene, another seed and frame id
    "cap_192":          (192, 80, 8, 0.65, 0, {}, 0, 1),
    "rejected_12":      (130, 67, 6, 0.65, 1, {"third": (4, 0)}, 1, 1),          # a third plane over 12 regions: its winners are rejected
    "rejected_15":      (130, 67, 6, 0.65, 2, {"third": (4, 3)}, 2, 1),          # 15 regions: one below the bound
    "accepted_16":      (130, 67, 6, 0.65, 0, {"third": (4, 4)}, 0, 1),          # 16 regions: exactly the bound, a third plane
    "collinear":        (96, 40, 4, 0.65, 2, {"collinear": COLLINEAR}, 2, 1),    # sampled labels whose S17 plane is zero
    "both":             (96, 40, 4, 0.65, 0, {"both": BOTH}, 0, 1),              # labels of the first plane that fit the second too
    "few_local":        (96, 40, 8, 0.0, 3, {"only": (1, 13)}, 0, 1),             # two labels have points, under three grid cells: <= 3 local planes in every iteration
}


@functools.lru_cache(maxsize=None)
def fit_case(name):
    w, h, bs, invalid, gen, opts, _, _ = FIT_CASES[name]
    opts = dict(opts)
    only = opts.pop("only", None)
    lab, xyz, mx = fit_scene(w, h, bs, invalid, gen, **opts)
    if only:      # after test_planefit_spec's third scene: every point outside the labels `only` fails the predicate
        xyz[..., 2][~np.isin(lab, only)] = -1.0
    return lab, xyz, mx


@functools.lru_cache(maxsize=None)
def fit_expected(name):
    lab, xyz, mx = fit_case(name)
    seed, frame = FIT_CASES[name][6:]
    planes17, npts, counts, off, pts = N.label_planes(lab, xyz, mx, N.PRED_PLANEFIT, seed, frame)
    trace = []
    P, A, it = N.planefit(lab, xyz, mx, seed, frame, planes17=planes17, trace=trace)
    return dict(planes17=planes17, npts=npts, counts=counts, P=P, A=A, it=it, trace=trace, seed=seed, frame=frame, mx=mx)

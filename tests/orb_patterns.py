"""Input images for the ORB edge tests (test_gpu_orb_edges.py), as plain numpy, with the CPU helpers that state what each image does
to the kernels of csrc/orb_kernels.hip.  test_orb_patterns.py checks every premise with np_orb alone; the GPU tests assert the same
premises again before they compare, so an image that has stopped reaching its branch fails the test instead of passing it.

The selection (orb_select_kernel) orders the survivors of a level by one 96-bit key, larger = earlier:

    bits 95..32   R + 2^54                 (|R| < 2^56)
    bits 31..0    ~(y << 16 | x)

and finds the quota-th largest key by a radix select over eight 12-bit digits, digit 0 the most significant.  A pass runs while more than
SEL_FINISH = 2048 keys share the digits chosen so far; the rest is finished in a 2048-entry LDS buffer.  Digits 0..4 and the upper 4 bits
of digit 5 are R, the lower 8 bits of digit 5 are ~(y >> 8), digit 6 is ~((y & 255) << 4 | x >> 12), digit 7 is ~(x & 4095).

With ONE class of R among more than 2048 survivors, and the threshold inside it (the dot lattice below):
  * digits 0..4 hold one bin each, and so does digit 5 as long as every y is below 256;
  * digit 6 holds one bin per row (x < 4096), so after pass 6 at most one row's keys share the prefix: seven passes, then the finish;
  * digit 7 cannot be reached.  It needs more than 2048 keys that agree in R, in y and in x >> 12, which is more than 2048 survivors of
    the strict 3 x 3 non-maximum suppression in one row within 4096 columns; two survivors are never neighbours, so a row has at most
    2048 of them there.  Nothing tests digit 7.
radix_trace() replays these passes on the CPU from the keys, so that a test can assert how many passes its image takes.
"""
import functools

import numpy as np

import np_orb as N

SEL_FINISH = 2048   # kSelFinish = kSelChunk of orb_kernels.hip
SEL_THREADS = 1024  # kSelThreads
TILE_W, TILE_H = 64, 16   # kOrbTileW, kOrbTileH: the detect kernel's tiles start at x = y = EDGE

RAMPS = {"down": 8, "up": 23, "right": 0, "left": 15}   # direction the background grows in -> orientation bin of every level-0 keypoint


# ---- generators -------------------------------------------------------------------------------------------------------------
def dot_lattice(h, w, p=4, ox=0, oy=0, hi=255, bg=0):
    """`bg` (a scalar or an [h, w] image) with single pixels of value `hi` at [oy::p, ox::p]."""
    img = np.empty((h, w), np.uint8)
    img[...] = bg
    img[oy::p, ox::p] = hi
    return img


def ramp(h, w, direction, steps=40):
    """A background that depends on one coordinate only: `steps` grey levels, growing in `direction`."""
    y, x = (np.arange(h) * steps) // h, (np.arange(w) * steps) // w
    line = {"down": y[:, None], "up": y[::-1, None], "right": x[None, :], "left": x[None, ::-1]}[direction]
    return np.broadcast_to(line, (h, w)).astype(np.uint8)


def ramp_lattice(h, w, direction, ox=0, oy=0):
    return dot_lattice(h, w, 4, ox, oy, 255, ramp(h, w, direction))


def two_class_lattice(h, w, ox, oy, split, low=200):
    """The dot lattice with the dots of rows >= split at `low`: a few large classes of R, the largest (the `low` dots) last in order."""
    img = dot_lattice(h, w, 4, ox, oy)
    part = img[split:]
    part[part == 255] = low
    return img


def plateau_marks(h, w):
    """Where plateau() puts its groups in an [h, w] image with at least two tile columns and three tile rows: (y, x, shape, values),
    shape "h" = a horizontal pair, "v" = a vertical pair, "q" = a 2 x 2 block (values in raster order), "d" = a single dot.
    xs / ys / ys2 = the first column / row of the second tile column / second and third tile row.  Groups keep 5 or more pixels apart, so
    none lies on another's FAST circle (radius 3)."""
    xs, ys, ys2 = N.EDGE + TILE_W, N.EDGE + TILE_H, N.EDGE + 2 * TILE_H
    xl, yl = w - N.EDGE - 1, h - N.EDGE - 1   # the last candidate column and row
    assert xs + 21 <= xl and ys2 + 5 <= yl
    e, a, b = (255, 255), (255, 250), (250, 255)
    return [
        # inside the first tile: equal pairs and block (all dropped), unequal pairs (the larger pixel survives), a dot
        (35, 40, "h", e), (35, 50, "v", e), (35, 60, "q", (255,) * 4), (35, 70, "h", a), (35, 80, "v", b), (40, 88, "d", (255,)),
        # across the column seam xs - 1 | xs, in the first and the second tile row
        (35, xs - 1, "h", e), (ys + 5, xs - 1, "h", a), (ys + 10, xs - 1, "h", b),
        # across the row seam ys - 1 | ys, in the first tile column
        (ys - 1, 40, "v", e), (ys - 1, 50, "v", a), (ys - 1, 60, "v", b),
        # blocks on the corner of four tiles (equal; the largest pixel in the upper left tile) and across the row seam ys2 - 1 | ys2 alone
        (ys - 1, xs - 1, "q", (255,) * 4), (ys2 - 1, xs - 1, "q", (255, 250, 250, 250)), (ys2 - 1, xs + 9, "q", (250, 250, 250, 255)),
        (ys2 - 1, xs - 11, "q", (250, 255, 250, 250)), (ys2 - 1, xs - 21, "q", (250, 250, 255, 250)),
        # across the ends of the candidate region: the pixel outside scores nothing, so the one inside survives
        (ys + 8, N.EDGE - 1, "h", e), (ys + 8, xl, "h", e), (N.EDGE - 1, xs + 10, "v", e), (yl, xs + 10, "v", e),
        # equal pairs on the first and last candidate column and row themselves
        (40, N.EDGE, "v", e), (yl - 1, xl, "v", e), (N.EDGE, xs + 20, "h", e), (yl, 45, "h", e),
    ]


def plateau(h, w, marks=None, bg=0):
    img = np.full((h, w), bg, np.uint8)
    for y, x, shape, v in (plateau_marks(h, w) if marks is None else marks):
        cells = {"d": [(0, 0)], "h": [(0, 0), (0, 1)], "v": [(0, 0), (1, 0)], "q": [(0, 0), (0, 1), (1, 0), (1, 1)]}[shape]
        for (dy, dx), val in zip(cells, v):
            assert img[y + dy, x + dx] == bg, "plateau groups overlap"
            img[y + dy, x + dx] = val
    return img


def gray3(img):
    """[h, w] -> [h, w, 3] with three equal channels (S1 gray gives the image back: the weights sum to 2^14)."""
    return np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2))


# ---- what an image does -----------------------------------------------------------------------------------------------------
def level0(img):
    """-> (R, ys, xs) of the level-0 survivors in the kernel's order of preference (R descending, y, x ascending)."""
    R, ys, xs = N.detect_level(np.ascontiguousarray(img))
    return N.select(R, ys, xs, len(R))


def key_digits(R, ys, xs):
    """The eight 12-bit digits of every 96-bit key, [n, 8] (Python integers: no 64-bit overflow to think about)."""
    out = np.zeros((len(R), 8), np.int64)
    for i, (r, y, x) in enumerate(zip(R.tolist(), ys.tolist(), xs.tolist())):
        key = ((r + (1 << 54)) << 32) | (~((y << 16) | x) & 0xFFFFFFFF)
        assert 0 <= key < 1 << 96
        out[i] = [(key >> (84 - 12 * d)) & 4095 for d in range(8)]
    return out


def radix_trace(R, ys, xs, quota):
    """The radix passes of orb_select_kernel for one level -> dict(passes, bins = non-empty bins of each pass among the keys that still
    match, finish = keys that go to the LDS finish, threshold = index of the quota-th key); passes = 0 and finish = 0 when quota >= c
    (no selection at all), passes = 0 and finish = c when c <= SEL_FINISH."""
    c = len(R)
    if quota >= c:
        return dict(passes=0, bins=[], finish=0, threshold=None)
    dig = key_digits(R, ys, xs)
    match, need, bins = np.ones(c, bool), quota, []
    d = 0
    while d < 8 and match.sum() > SEL_FINISH:
        hist = np.bincount(dig[match, d], minlength=4096)
        above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])   # keys in the bins above each bin
        b = int(np.nonzero((above < need) & (need <= above + hist))[0][0])
        bins.append(int((hist > 0).sum()))
        need -= int(above[b])
        match &= dig[:, d] == b
        d += 1
    order = np.lexsort((xs, ys, -R))
    kept = order[match[order]]          # the matching keys, best first
    return dict(passes=d, bins=bins, finish=int(match.sum()), threshold=int(kept[need - 1]))


def rank_chunks(keep):
    """-> (LDS chunks of the rank stage, records per thread) for `keep` kept records."""
    return -(-keep // SEL_FINISH), -(-keep // SEL_THREADS)


def equal_drops(img):
    """Pixels with a FAST score that strict NMS drops although no neighbour scores MORE: an equal neighbour alone removes them.
    -> set of (y, x)."""
    s = N.fast_scores(np.ascontiguousarray(img))
    h, w = s.shape
    p = np.zeros((h + 2, w + 2), np.int32)
    p[1:-1, 1:-1] = s
    top = np.max([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx], axis=0)
    ys, xs = np.nonzero((s > 0) & ~N.nms(s) & (top == s))
    return set(zip(ys.tolist(), xs.tolist()))


def tile_edges(h, w):
    """-> (columns, rows) that are the first or last of a detect tile or of the candidate region of an [h, w] level."""
    xe, ye = w - N.EDGE, h - N.EDGE
    cols = {x for x0 in range(N.EDGE, xe, TILE_W) for x in (x0, min(x0 + TILE_W, xe) - 1)}
    rows = {y for y0 in range(N.EDGE, ye, TILE_H) for y in (y0, min(y0 + TILE_H, ye) - 1)}
    return cols, rows


# ---- the named images of the tests, each made once, and what np_orb gives for them -------------------------------------------
LATTICE = (200, 400, 1, 2)          # h, w, ox, oy: 2856 level-0 survivors in one class of R
LATTICE_FULL = (190, 318, 1, 2)     # exactly SEL_FINISH
LATTICE_OVER = (190, 322, 1, 2)     # 2080: just above it
LATTICE_BIG = (375, 1242, 1, 2)     # 23010, the one large image
RAMP_SIZE = (128, 160, 1, 2)
SEAM_SIZE = (100, 160)              # two tile columns (the second partial), three tile rows (the last partial)


@functools.lru_cache(maxsize=None)
def image(name):
    """The test images by name; read-only."""
    kind, _, arg = name.partition(":")
    if kind == "lattice":
        img = dot_lattice(*LATTICE[:2], 4, *LATTICE[2:])
    elif kind == "lattice_full":
        img = dot_lattice(*LATTICE_FULL[:2], 4, *LATTICE_FULL[2:])
    elif kind == "lattice_over":
        img = dot_lattice(*LATTICE_OVER[:2], 4, *LATTICE_OVER[2:])
    elif kind == "lattice_big":
        img = dot_lattice(*LATTICE_BIG[:2], 4, *LATTICE_BIG[2:])
    elif kind == "two_class":
        img = two_class_lattice(*LATTICE[:2], *LATTICE[2:], split=60)
    elif kind == "ramp":        # ramp:down ...
        img = ramp_lattice(*RAMP_SIZE[:2], arg, *RAMP_SIZE[2:])
    elif kind == "plain":       # the plain lattice at the ramps' size
        img = dot_lattice(*RAMP_SIZE[:2], 4, *RAMP_SIZE[2:])
    elif kind == "seam":        # seam:<ox><oy>
        img = dot_lattice(*SEAM_SIZE, 4, int(arg[0]), int(arg[1]))
    elif kind == "plateau":
        img = plateau(*SEAM_SIZE)
    elif kind == "flat":        # flat:<h>x<w>
        h, w = (int(v) for v in arg.split("x"))
        img = np.full((h, w), 90, np.uint8)
    else:
        raise KeyError(name)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(name, nfeatures):
    """np_orb.orb of image(name) -> (keypoints, descriptors, survivor counts per built level); read-only."""
    kp, de, _, counts = N.orb(image(name), nfeatures, want_levels=True)
    kp.setflags(write=False)
    de.setflags(write=False)
    return kp, de, tuple(counts)


@functools.lru_cache(maxsize=None)
def survivors(name):
    out = level0(image(name))
    for a in out:
        a.setflags(write=False)
    return out


def selection_facts(name, nfeatures):
    """-> dict(c, classes, quota, keep, trace) of level 0 of image(name) under nfeatures."""
    R, ys, xs = survivors(name)
    quota = N.level_quotas(nfeatures)[0]
    return dict(c=len(R), classes=len(np.unique(R)), quota=quota, keep=min(len(R), quota), trace=radix_trace(R, ys, xs, quota))

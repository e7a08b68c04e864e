"""CPU tests of the ORB edge-test inputs (tests/orb_patterns.py): every premise that test_gpu_orb_edges.py relies on, checked with the numpy
restatement (np_orb) alone, and radix_trace() itself against a plain sort.  No GPU."""
import numpy as np
import pytest

import np_orb as N
import orb_patterns as P


def _moments(name):
    R, ys, xs = P.survivors(name)
    return N.moments(P.image(name), ys, xs)


# ---- the dot lattice ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,count", [("lattice", 2856), ("lattice_full", 2048), ("lattice_over", 2080), ("plain", 384)])
def test_lattice_every_dot_is_one_survivor_in_one_class(name, count):
    img = P.image(name)
    h, w = img.shape
    R, ys, xs = P.survivors(name)
    inside = np.zeros((h, w), bool)
    inside[N.EDGE:h - N.EDGE, N.EDGE:w - N.EDGE] = True
    dots = (img == 255) & inside
    got = np.zeros((h, w), bool)
    got[ys, xs] = True
    assert (got == dots).all(), "the survivors are the dots of the candidate region, all of them and nothing else"
    assert len(R) == count and len(np.unique(R)) == 1
    m10, m01 = _moments(name)
    assert (m10 == 0).all() and (m01 == 0).all()
    assert ys.max() < 256 and xs.max() < 4096      # digit 5 holds one bin, digit 6 one bin per row


def test_lattice_counts_of_other_sizes():
    for (h, w), count in (((190, 330), 2144), ((192, 352), 2304)):
        R, _, _ = P.level0(P.dot_lattice(h, w, 4, 1, 2))
        assert len(R) == count and len(np.unique(R)) == 1


def test_big_lattice():
    R, ys, xs = P.survivors("lattice_big")
    assert len(R) == 23010 and len(np.unique(R)) == 1
    f = P.selection_facts("lattice_big", 65536)
    assert f["quota"] == 14233 < f["c"] and P.rank_chunks(f["keep"]) == (7, 14)
    # 375 rows: y reaches 256, so digit 5 (whose low 8 bits are ~(y >> 8)) splits in two, and digit 6 has one bin per row of that half
    assert f["trace"]["passes"] == 7 and f["trace"]["bins"][:6] == [1, 1, 1, 1, 1, 2] and f["trace"]["finish"] == len(np.unique(xs))


def test_lattice_with_a_background_image():
    bg = P.ramp(64, 80, "right")
    img = P.dot_lattice(64, 80, 4, 3, 1, hi=200, bg=bg)
    assert (img[1::4, 3::4] == 200).all()
    rest = np.ones((64, 80), bool)
    rest[1::4, 3::4] = False
    assert (img[rest] == bg[rest]).all() and bg.min() == 0 and bg.max() == 39 and (np.diff(bg.astype(int), axis=0) == 0).all()


# ---- selection cases ------------------------------------------------------------------------------------------------------------
# 400 x 200, one class of 2856: what each nfeatures of the GPU test does (see the module text of orb_patterns for the derivation)
@pytest.mark.parametrize("n,quota,passes,chunks", [(500, 109, 7, (1, 1)), (5000, 1086, 7, (1, 2)), (12000, 2606, 7, (2, 3)), (65536, 14233, 0, (2, 3))])
def test_selection_cases_of_the_lattice(n, quota, passes, chunks):
    f = P.selection_facts("lattice", n)
    assert (f["c"], f["classes"], f["quota"]) == (2856, 1, quota)
    assert f["keep"] == min(quota, 2856) and P.rank_chunks(f["keep"]) == chunks
    t = f["trace"]
    assert t["passes"] == passes
    if quota < f["c"]:
        R, ys, xs = P.survivors("lattice")
        rows = len(np.unique(ys))
        assert t["bins"] == [1, 1, 1, 1, 1, 1, rows] and t["finish"] == f["c"] // rows == 84     # one row's keys finish in LDS
        assert t["threshold"] == quota - 1                                                      # survivors() is in key order
    else:
        assert t["finish"] == 0                                                                 # keep = c: no threshold is sought


def test_lattice_keys_digit_by_digit():
    R, ys, xs = P.survivors("lattice")
    d = P.key_digits(R, ys, xs)
    assert all(len(np.unique(d[:, k])) == 1 for k in range(6))
    assert (d[:, 6] == (~(ys << 4) & 4095)).all() and len(np.unique(d[:, 6])) == len(np.unique(ys))
    assert (d[:, 7] == (~xs & 4095)).all()
    # digit 5 is the straddling one: 4 bits of R + 2^54 above 8 bits of ~(y >> 8)
    assert (d[:, 5] == ((((R + (1 << 54)) & 15) << 8) | 255)).all()
    # digit 7 would need more than SEL_FINISH keys in one bin of digit 6, i.e. in one row; strict NMS allows (4096 / 2) in 4096 columns
    assert np.bincount(d[:, 6]).max() <= P.SEL_FINISH


def test_sel_finish_boundary():
    full, over = P.selection_facts("lattice_full", 5000), P.selection_facts("lattice_over", 5000)
    assert full["c"] == P.SEL_FINISH and full["classes"] == 1 and full["quota"] == 1086
    assert full["trace"]["passes"] == 0 and full["trace"]["finish"] == P.SEL_FINISH          # no pass, the LDS buffer exactly full
    assert P.SEL_FINISH < over["c"] == 2080 <= 2100 and over["classes"] == 1
    assert over["trace"]["passes"] == 7 and over["trace"]["finish"] == 65


def test_two_class_lattice():
    """The threshold lies in the last and largest class: the pass that separates the classes subtracts the keys above, the deep passes go on."""
    R, ys, xs = P.survivors("two_class")
    u, cnt = np.unique(R, return_counts=True)
    assert len(u) == 4 and cnt[0] == 2184 > P.SEL_FINISH and cnt[1:].sum() == 672
    f = P.selection_facts("two_class", 5000)
    assert 672 < f["quota"] < f["c"] and f["trace"]["passes"] == 7 and f["trace"]["bins"][:2] == [1, 4] and f["trace"]["finish"] == 84
    assert P.selection_facts("two_class", 500)["trace"] == dict(passes=2, bins=[1, 4], finish=504, threshold=108)


def test_radix_trace_finds_the_quota_th_key():
    rng = np.random.default_rng(3)
    for c, classes in ((5000, 2), (3000, 1), (2049, 3), (2048, 1), (70, 5)):
        cells = rng.permutation(300 * 200)[:c]
        ys, xs = 31 + cells // 200, 31 + cells % 200
        R = rng.integers(-(1 << 50), 1 << 50, classes)[rng.integers(0, classes, c)]
        order = np.lexsort((xs, ys, -R))
        for quota in (1, c // 3, c - 1):
            t = P.radix_trace(R, ys, xs, quota)
            assert t["threshold"] == order[quota - 1], (c, classes, quota)
            assert (t["passes"] == 0) == (c <= P.SEL_FINISH) and t["finish"] <= P.SEL_FINISH
        assert P.radix_trace(R, ys, xs, c)["threshold"] is None


# ---- ramps: moments exactly on a ray ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", list(P.RAMPS))
def test_ramp_moments(direction):
    name = "ramp:" + direction
    R, ys, xs = P.survivors(name)
    m10, m01 = _moments(name)
    assert len(R) == 384
    if direction in ("down", "up"):        # 90 / 270 degrees: exactly on boundary ray 7 / 22, which starts bin 8 / 23
        assert (m10 == 0).all() and (np.sign(m01) == (1 if direction == "down" else -1)).all()
        B = np.array(N.BOUNDARY[7 if direction == "down" else 22], np.int64)
        assert (B[0] * m01 - B[1] * m10 == 0).all()
    else:
        assert (m01 == 0).all() and (np.sign(m10) == (1 if direction == "right" else -1)).all()
    assert (N.orientation_bin(m10, m01) == P.RAMPS[direction]).all()
    kp = P.expected(name, 2000)[0]
    k0 = kp[kp["octave"] == 0]
    assert len(k0) == 384 and (k0["angle"] == np.float32(12 * P.RAMPS[direction])).all()


def test_plain_lattice_has_zero_moments_and_bin_0():
    m10, m01 = _moments("plain")
    assert (m10 == 0).all() and (m01 == 0).all()
    kp = P.expected("plain", 2000)[0]
    assert (kp[kp["octave"] == 0]["angle"] == 0).all() and (kp["octave"] == 0).sum() == 384


def test_gray3_converts_back():
    import oracle_lib as O
    img = P.image("ramp:left")
    assert (O.bgr2gray(P.gray3(img)) == img).all()


# ---- seams ---------------------------------------------------------------------------------------------------------------------
def test_seam_lattices_reach_every_tile_edge():
    h, w = P.SEAM_SIZE
    cols, rows = P.tile_edges(h, w)
    assert cols == {31, 94, 95, 128} and rows == {31, 46, 47, 62, 63, 68}      # 2 tile columns (64 + 34), 3 tile rows (16 + 16 + 6)
    seen_c, seen_r = set(), set()
    for ox in range(4):
        for oy in range(4):
            kp = P.expected(f"seam:{ox}{oy}", 5000)[0]
            k0 = kp[kp["octave"] == 0]
            assert len(k0) == P.expected(f"seam:{ox}{oy}", 5000)[2][0] >= 216      # every survivor is kept
            seen_c |= set(k0["x"].astype(int).tolist()) & cols
            seen_r |= set(k0["y"].astype(int).tolist()) & rows
    assert seen_c == cols and seen_r == rows


def test_plateau_drops_equal_neighbours_on_the_seams():
    img = P.image("plateau")
    drops = P.equal_drops(img)
    R, ys, xs = P.survivors("plateau")
    alive = set(zip(ys.tolist(), xs.tolist()))
    assert len(drops) == 24 and not drops & alive
    assert {(35, 40), (35, 41), (35, 50), (36, 50)} <= drops                                   # inside a tile
    assert {(35, 94), (35, 95)} <= drops and {(46, 40), (47, 40)} <= drops                     # across x = 94 | 95, across y = 46 | 47
    assert {(46, 94), (46, 95), (47, 94), (47, 95)} <= drops                                   # on the corner of four tiles
    assert {(40, 31), (41, 31), (67, 128), (68, 128), (31, 115), (31, 116), (68, 45), (68, 46)} <= drops      # first / last candidate column and row
    # the larger pixel of an unequal pair survives on either side of a seam; beside a pixel outside the region the inner one does
    assert {(52, 94), (57, 95), (46, 50), (47, 60), (62, 94), (63, 105), (62, 85), (63, 74)} <= alive
    assert {(55, 31), (55, 128), (31, 105), (68, 105)} <= alive
    assert len(alive) == 15

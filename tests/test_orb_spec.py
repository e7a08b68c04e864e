"""CPU tests of the ORB feature spec and its numpy restatement (tests/np_orb.py): pinned tables,
hand-worked known answers, properties, and the built library's host-side level layout (cart_orb_levels, no GPU)."""
import numpy as np
import pytest

import np_orb as N


# ---- pinned tables ------------------------------------------------------------------------------------------------------
def test_level_quotas_pinned():
    assert N.level_quotas(5000) == [1086, 905, 754, 628, 524, 436, 364, 303]
    assert N.level_quotas(7) == [2, 1, 1, 1, 1, 1, 0, 0]


def test_level_quotas_sum_and_sign_for_every_n():
    for n in range(1, 65537):
        q = N.level_quotas(n)
        assert min(q) >= 0 and sum(q) == n, n


def test_level_sizes_pinned():
    sz = [(w, h) for w, h, _ in N.level_sizes(1242, 375)]
    assert sz == [(1242, 375), (1035, 312), (862, 260), (719, 217), (599, 181), (499, 151), (416, 126), (347, 105)]
    assert N.built_levels(1242, 375) == 8
    assert [(w, h) for w, h, _ in N.level_sizes(320, 96)][:3] == [(320, 96), (267, 80), (222, 67)]
    assert N.built_levels(320, 96) == 3
    assert N.built_levels(62, 200) == 0 and N.built_levels(63, 63) == 1


def test_umax_pinned():
    assert N.UMAX == (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
    assert len(N.patch_offsets()) == 749


def _round_away(v):
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def test_fixed_point_tables_equal_rounded_cos_sin():
    j = np.arange(30)
    bt = np.deg2rad(12.0 * j + 6.0)
    st = np.deg2rad(12.0 * j)
    B = np.stack([_round_away(np.cos(bt) * 2.0 ** 20), _round_away(np.sin(bt) * 2.0 ** 20)], 1)
    S = np.stack([_round_away(np.cos(st) * 2.0 ** 20), _round_away(np.sin(st) * 2.0 ** 20)], 1)
    assert (np.array(N.BOUNDARY) == B).all()
    assert (np.array(N.STEER) == S).all()
    assert (B[15:] == -B[:15]).all() and (S[15:] == -S[:15]).all()


def test_pattern_properties_and_stability():
    P = N.pattern()
    assert P.shape == (256, 4)
    assert (P >= -13).all() and (P <= 13).all()
    assert ((P[:, :2] != P[:, 2:]).any(1)).all()
    assert (N.pattern() == P).all()
    # pinned: a change to the stream, the draw rule or the coordinate rule changes these
    assert P[:4].tolist() == PATTERN_HEAD
    assert int(np.abs(P).sum()) == PATTERN_ABS_SUM
    SP = N.steered_pattern()
    assert (SP[0] == P).all() and (SP[15] == -P).all()
    assert np.abs(SP).max() <= 19


PATTERN_HEAD = [[4, 2, -3, -2], [7, 0, -4, 4], [5, -7, 1, 3], [-10, -1, -2, 6]]
PATTERN_ABS_SUM = 3280


# ---- the built library's host-side layout -------------------------------------------------------------------------------
def test_cart_orb_levels_equals_restatement():
    from cartslam import orb_levels
    for w, h in ((1242, 375), (320, 96), (333, 129), (97, 71), (62, 200), (63, 63), (1, 1), (4096, 2160), (16384, 63)):
        for n in (1, 7, 500, 5000, 20000, 65536):
            built, lv = orb_levels(w, h, n)
            assert built == N.built_levels(w, h), (w, h)
            assert [(a, b) for a, b, _ in lv] == [(a, b) for a, b, _ in N.level_sizes(w, h)], (w, h)
            assert [c for _, _, c in lv] == N.level_quotas(n), n
    from cartslam import EngineError
    for bad in ((0, 10, 10), (10, 0, 10), (10, 10, 0), (10, 10, 65537)):
        with pytest.raises(EngineError):
            orb_levels(*bad)


# ---- known answers ------------------------------------------------------------------------------------------------------
def _ring_image(values, centre=100, size=96):
    """A flat image with the 16 circle pixels around (48, 48) set to `values` (list of 16)."""
    img = np.full((size, size), centre, np.uint8)
    for (dx, dy), v in zip(N.CIRCLE, values):
        img[48 + dy, 48 + dx] = v
    return img


def test_fast_arcs():
    nine = [130] * 9 + [100] * 7
    s = N.fast_scores(_ring_image(nine))
    assert s[48, 48] == 29   # min over the arc of (130 - 100) = 30, minus 1
    eight = [130] * 8 + [100] * 8
    assert N.fast_scores(_ring_image(eight))[48, 48] == 0
    dark = [100] * 3 + [60] * 10 + [100] * 3
    assert N.fast_scores(_ring_image(dark))[48, 48] == 39
    weak = [121] * 16   # every difference 21: score 20, the threshold itself
    assert N.fast_scores(_ring_image(weak))[48, 48] == 20
    flat = [120] * 16   # every difference 20: score 19, not a corner
    assert N.fast_scores(_ring_image(flat))[48, 48] == 0
    mixed = [140, 135, 150, 130, 170, 160, 145, 133, 180] + [100] * 7   # arc minimum 130 -> 29
    assert N.fast_scores(_ring_image(mixed))[48, 48] == 29


def test_fast_straight_edge_is_not_a_corner():
    img = np.full((96, 96), 50, np.uint8)
    img[:, 48:] = 200
    s = N.fast_scores(img)
    assert (s[31:65, 31:65] == 0).all()


def test_nms_drops_equal_neighbours():
    sc = np.zeros((10, 10), np.int32)
    sc[4, 4] = sc[4, 5] = 30
    sc[7, 2] = 25
    keep = N.nms(sc)
    assert not keep[4, 4] and not keep[4, 5] and keep[7, 2]
    sc[4, 5] = 29
    keep = N.nms(sc)
    assert keep[4, 4] and not keep[4, 5]


def test_harris_small_patch_by_hand():
    # a vertical step at x >= 50: Ix = 4 * 40 = 160 at x = 49 and x = 50, Iy = 0 everywhere
    img = np.full((96, 96), 10, np.uint8)
    img[:, 50:] = 50
    # window at (48, 48): columns 45..51 -> x = 49 and 50 carry Ix = 160 on 7 rows each
    a = 2 * 7 * 160 * 160
    R = N.harris(img, [48], [48])[0]
    assert R == 25 * (a * 0 - 0) - (a + 0) ** 2
    # a single bright pixel: gradients around it, worked out exhaustively here
    img = np.zeros((96, 96), np.uint8)
    img[48, 48] = 100
    Ix = {(0, -1): 200, (0, 1): -200, (-1, -1): 100, (1, -1): 100, (-1, 1): -100, (1, 1): -100}   # (dy, dx) -> Ix
    Iy = {(-1, 0): 200, (1, 0): -200, (-1, -1): 100, (-1, 1): 100, (1, -1): -100, (1, 1): -100}
    keys = set(Ix) | set(Iy)
    a = sum(Ix.get(k, 0) ** 2 for k in keys)
    b = sum(Iy.get(k, 0) ** 2 for k in keys)
    c = sum(Ix.get(k, 0) * Iy.get(k, 0) for k in keys)
    assert (a, b, c) == (120000, 120000, 0)
    assert N.harris(img, [48], [48])[0] == 25 * (a * b - c * c) - (a + b) ** 2


def test_orientation_bins_at_centres_and_boundaries():
    B = np.array(N.BOUNDARY, np.int64)
    S = np.array(N.STEER, np.int64)
    k = N.orientation_bin(S[:, 0], S[:, 1])          # direction of bin centre k (moments (m10, m01) = (cos, sin))
    assert (k == np.arange(30)).all()
    kb = N.orientation_bin(B[:, 0], B[:, 1])         # ray B_j starts bin j + 1
    assert (kb == (np.arange(30) + 1) % 30).all()
    assert N.orientation_bin([0], [0])[0] == 0
    assert N.orientation_bin([5], [0])[0] == 0
    assert N.orientation_bin([0], [5])[0] == 8     # 90 degrees lies on ray B_7, which starts bin 8
    assert N.orientation_bin([-5], [0])[0] == 15 and N.orientation_bin([0], [-5])[0] == 23


# ---- properties ---------------------------------------------------------------------------------------------------------
def _brute(img):
    """Per-pixel loops of FAST, NMS and Harris, straight from the spec's words."""
    I = img.astype(np.int64)
    h, w = I.shape
    score = np.zeros((h, w), np.int64)
    for y in range(N.EDGE, h - N.EDGE):
        for x in range(N.EDGE, w - N.EDGE):
            ring = [I[y + dy, x + dx] - I[y, x] for dx, dy in N.CIRCLE]
            best = max(min(sg * ring[(k + j) % 16] for j in range(9)) for k in range(16) for sg in (1, -1)) - 1
            score[y, x] = best if best >= N.FAST_T else 0
    out = []
    for y in range(N.EDGE, h - N.EDGE):
        for x in range(N.EDGE, w - N.EDGE):
            s = score[y, x]
            if s and all(s > score[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx):
                a = b = c = 0
                for v in range(-3, 4):
                    for u in range(-3, 4):
                        yy, xx = y + v, x + u
                        ix = 2 * (I[yy, xx + 1] - I[yy, xx - 1]) + (I[yy - 1, xx + 1] - I[yy - 1, xx - 1]) + (I[yy + 1, xx + 1] - I[yy + 1, xx - 1])
                        iy = 2 * (I[yy + 1, xx] - I[yy - 1, xx]) + (I[yy + 1, xx - 1] - I[yy - 1, xx - 1]) + (I[yy + 1, xx + 1] - I[yy - 1, xx + 1])
                        a += ix * ix; b += iy * iy; c += ix * iy
                out.append((25 * (a * b - c * c) - (a + b) ** 2, y, x))
    return score, sorted(out)


@pytest.mark.parametrize("seed", [0, 1])
def test_brute_force_equals_vectorised(seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (96, 96)).astype(np.uint8)
    if seed:
        img = np.kron(rng.integers(0, 256, (33, 33)), np.ones((3, 3), np.int64))[:96, :96].astype(np.uint8)   # blocky: ties
    score, brute = _brute(img)
    assert (N.fast_scores(img) == score).all()
    R, ys, xs = N.detect_level(img)
    assert len(brute) > 10
    assert sorted(zip(R.tolist(), ys.tolist(), xs.tolist())) == brute


def test_selection_order_is_total():
    R = np.array([5, 7, 7, 7, 1], np.int64)
    ys = np.array([0, 3, 2, 2, 9], np.int64)
    xs = np.array([0, 1, 9, 4, 0], np.int64)
    r, y, x = N.select(R, ys, xs, 4)
    assert list(zip(r, y, x)) == [(7, 2, 4), (7, 2, 9), (7, 3, 1), (5, 0, 0)]


def test_rotation_by_180_degrees():
    rng = np.random.default_rng(5)
    img = np.kron(rng.integers(0, 256, (40, 60)), np.ones((3, 3), np.int64)).astype(np.uint8)
    H, W = img.shape
    rot = img[::-1, ::-1].copy()
    R, ys, xs = N.detect_level(img)
    m10, m01 = N.moments(img, ys, xs)
    ok = (m10 != 0) | (m01 != 0)
    ys, xs, m10, m01 = ys[ok], xs[ok], m10[ok], m01[ok]
    assert len(ys) > 50
    ry, rx = H - 1 - ys, W - 1 - xs
    r10, r01 = N.moments(rot, ry, rx)
    assert (r10 == -m10).all() and (r01 == -m01).all()
    k = N.orientation_bin(m10, m01)
    rk = N.orientation_bin(r10, r01)
    assert ((rk - k) % 30 == 15).all()
    assert (N.descriptors(img, ys, xs, k) == N.descriptors(rot, ry, rx, rk)).all()

    # the rotated image has the same survivors with the same R, mirrored (the stages before the orientation are symmetric)
    R1, y1, x1 = N.detect_level(img)
    R2, y2, x2 = N.detect_level(rot)
    assert sorted(zip(R1.tolist(), y1.tolist(), x1.tolist())) == sorted(zip(R2.tolist(), (H - 1 - y2).tolist(), (W - 1 - x2).tolist()))

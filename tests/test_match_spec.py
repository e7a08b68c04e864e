"""CPU tests of spec S22: the numpy restatement tests/np_match.py against an independent plain-Python double
loop on small sets, case by case through every rule of the spec, and a planted-motion case through the ORB restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import np_match as M
import np_orb as N


def kps(xs, ys=None, octs=None):
    k = np.zeros(len(xs), N.KEYPOINT_DTYPE)
    k["x"] = xs
    k["y"] = 0 if ys is None else ys
    k["octave"] = 0 if octs is None else octs
    return k


def loop_match(qd, td, p, qk=None, tk=None):
    """S22 word by word with Python ints and floats rounded through float32."""
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    pop = lambda a, b: sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))   # noqa: E731

    def adm(i, j):
        if not p["use_gate"]:
            return True
        dx, dy = f32(np.float32(qk["x"][i]) - np.float32(tk["x"][j])), f32(np.float32(qk["y"][i]) - np.float32(tk["y"][j]))
        if math.isnan(dx) or math.isnan(dy):
            return False
        if not (f32(p["dx_min"]) <= dx <= f32(p["dx_max"]) and f32(p["dy_min"]) <= dy <= f32(p["dy_max"])):
            return False
        return p["max_octave_diff"] < 0 or abs(int(qk["octave"][i]) - int(tk["octave"][j])) <= p["max_octave_diff"]

    nq, nt = len(qd), len(td)
    D = [[pop(qd[i], td[j]) for j in range(nt)] for i in range(nq)]
    A = [[adm(i, j) for j in range(nt)] for i in range(nq)]
    i1 = []
    for j in range(nt):
        c = [(D[i][j] * 65536 + i, i) for i in range(nq) if A[i][j]]
        i1.append(min(c)[1] if c else -1)
    fwd, out = [], []
    for i in range(nq):
        c = [(D[i][j] * 65536 + j, j) for j in range(nt) if A[i][j]]
        if not c:
            fwd.append((-1, -1, -1, -1))
            continue
        j1 = min(c)[1]
        d1 = D[i][j1]
        others = [D[i][j] for j in range(nt) if A[i][j] and j != j1]
        d2 = min(others) if others else -1
        back = i1[j1] if p["cross_check"] else -1
        fwd.append((j1, d1, d2, back))
        if d1 <= p["max_distance"] and (p["ratio"] == 0 or d2 < 0 or 100 * d1 < p["ratio"] * d2) and (not p["cross_check"] or back == i):
            out.append((i, j1, d1, d2))
    return np.array(out, np.int32).reshape(-1, 4), np.array(fwd, np.int32).reshape(-1, 4)


def same(qd, td, p, qk=None, tk=None, block=256):
    m, f = M.match(qd, td, p, qk, tk, block=block)
    em, ef = loop_match(qd, td, p, qk, tk)
    assert (f == ef).all(), (f, ef)
    assert (m.view(np.int32).reshape(-1, 4) == em).all(), (m, em)
    return m, f


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32)).astype(np.uint8)


def flip(d, bits):
    """d with the first `bits` bits inverted."""
    o = d.copy()
    for b in range(bits):
        o[b // 8] ^= 1 << (b % 8)
    return o


def test_struct_layouts():
    from cartslam import _lib
    assert C.sizeof(_lib.MatchParams) == 36 and C.sizeof(_lib.Match) == 16
    assert [n for n, _ in _lib.MatchParams._fields_] == ["use_gate", "dx_min", "dx_max", "dy_min", "dy_max", "max_octave_diff", "max_distance",
                                                         "ratio", "cross_check"]
    p = _lib.MatchParams()
    _lib.load().cart_match_default_params(C.byref(p))
    assert {n: getattr(p, n) for n, _ in p._fields_} == M.DEFAULTS


def test_distance_forms_agree():
    rng = np.random.default_rng(0)
    q, t = rand_desc(rng, 300), rand_desc(rng, 257)
    q[0], q[1], t[0], t[1] = 0, 255, 255, 0
    q[2:40] = [flip(t[5], k) for k in range(38)]
    assert (M.distances(q, t) == M.distances_product(q, t)).all()
    assert M.distances(q, t)[0, 0] == 256 and M.distances(q, t)[1, 0] == 0 and M.distances(q, t)[7, 5] == 5


@pytest.mark.parametrize("seed", range(6))
def test_random_sets_every_rule(seed):
    rng = np.random.default_rng(seed)
    nq, nt = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    base = rand_desc(rng, 8)
    pick = lambda n: np.array([flip(base[rng.integers(0, 8)], int(rng.integers(0, 60))) for _ in range(n)])   # noqa: E731
    qd, td = pick(nq), pick(nt)
    qk = kps(rng.integers(0, 40, nq).astype(np.float32) / 2, rng.integers(0, 6, nq).astype(np.float32), rng.integers(0, 4, nq))
    tk = kps(rng.integers(0, 40, nt).astype(np.float32) / 2, rng.integers(0, 6, nt).astype(np.float32), rng.integers(0, 4, nt))
    for p in (M.params(), M.params(cross_check=0), M.params(ratio=0, max_distance=256), M.params(ratio=100, max_distance=20),
              M.params(use_gate=1, dx_min=-3.0, dx_max=6.5, dy_min=-1.0, dy_max=2.0), M.stereo_params(8, 1), M.temporal_params(4, cross_check=0),
              M.params(use_gate=1, dx_min=-100, dx_max=100, dy_min=-100, dy_max=100, max_octave_diff=0, ratio=0)):
        same(qd, td, p, qk, tk, block=7)


def test_duplicates_tie_to_the_lowest_index_in_both_directions():
    rng = np.random.default_rng(1)
    a, b = rand_desc(rng, 2)
    qd = np.array([a, a, b, a])
    td = np.array([b, a, a, b, a])
    m, f = same(qd, td, M.params(ratio=0))
    assert f[:, 0].tolist() == [1, 1, 0, 1] and f[:, 1].tolist() == [0, 0, 0, 0] and f[:, 2].tolist() == [0, 0, 0, 0]
    assert f[:, 3].tolist() == [0, 0, 2, 0]          # i1(1) = 0: the lowest query among the duplicates; i1(0) = 2
    assert m["query"].tolist() == [0, 2] and m["train"].tolist() == [1, 0]
    m, _ = same(qd, td, M.params())                  # d2 == d1 == 0: 100 * 0 < 80 * 0 fails
    assert len(m) == 0


def test_gate_bounds_are_inclusive_and_nan_fails():
    rng = np.random.default_rng(2)
    qd, td = rand_desc(rng, 1), rand_desc(rng, 6)
    qk = kps([10.0], [5.0], [2])
    tk = kps([7.0, 6.75, 12.0, 12.25, 8.0, np.nan], [5.0, 5.0, 5.0, 5.0, 3.5, 5.0], [2, 2, 2, 2, 2, 2])
    p = M.params(use_gate=1, dx_min=-2.0, dx_max=3.0, dy_min=-1.5, dy_max=1.5, cross_check=0, ratio=0, max_distance=256)
    assert M.admissible(qk, tk, p)[0].tolist() == [True, False, True, False, True, False]   # dx = 3, 3.25, -2, -2.25; dy = 1.5; NaN
    same(qd, td, p, qk, tk)
    tk["y"][4] = 3.25
    assert not M.admissible(qk, tk, p)[0, 4]
    qk["y"][0] = np.nan
    m, f = same(qd, td, p, qk, tk)
    assert len(m) == 0 and (f == -1).all()
    # the octave test: |2 - o| <= 1
    qk["y"][0] = 5.0
    tk["octave"] = [0, 1, 2, 3, 4, 2]
    assert M.admissible(qk, tk, M.params(use_gate=1, dx_min=-99, dx_max=99, dy_min=-99, dy_max=99, max_octave_diff=1))[0].tolist() == \
        [False, True, True, True, False, False]


def test_sole_candidate_is_accepted():
    rng = np.random.default_rng(3)
    qd = rand_desc(rng, 3)
    td = np.array([flip(qd[1], 5)])
    m, f = same(qd, td, M.params(max_distance=5))
    assert f[1].tolist() == [0, 5, -1, 1] and m.tolist() == [(1, 0, 5, -1)]
    # a gate that leaves one admissible train descriptor out of three
    td3 = np.array([flip(qd[0], 1), flip(qd[0], 9), flip(qd[0], 2)])
    qk, tk = kps([50.0, 0, 0]), kps([80.0, 45.0, 90.0])
    m, f = same(qd[:1], td3, M.params(use_gate=1, dx_min=0.0, dx_max=10.0, dy_min=0.0, dy_max=0.0), qk[:1], tk)
    assert f[0].tolist() == [1, 9, -1, 0] and m.tolist() == [(0, 1, 9, -1)]


def test_ratio_boundary():
    rng = np.random.default_rng(4)
    q = rand_desc(rng, 1)
    p = M.params(ratio=80, cross_check=0)
    m, f = same(q, np.array([flip(q[0], 40), flip(q[0], 50)]), p)     # 100 * 40 == 80 * 50: rejected
    assert f[0].tolist() == [0, 40, 50, -1] and len(m) == 0
    m, f = same(q, np.array([flip(q[0], 39), flip(q[0], 50)]), p)     # one bit less: accepted
    assert m.tolist() == [(0, 0, 39, 50)]
    m, _ = same(q, np.array([flip(q[0], 40), flip(q[0], 50)]), M.params(ratio=0, cross_check=0))
    assert len(m) == 1


def test_max_distance_boundary():
    rng = np.random.default_rng(5)
    q = rand_desc(rng, 1)
    t = np.array([flip(q[0], 30)])
    assert len(same(q, t, M.params(max_distance=30))[0]) == 1
    assert len(same(q, t, M.params(max_distance=29))[0]) == 0
    assert len(same(q, 255 - q, M.params(max_distance=256))[0]) == 1   # every bit differs


def test_cross_check_removes_exactly_the_non_mutual_pairs():
    rng = np.random.default_rng(6)
    t = rand_desc(rng, 3)
    qd = np.array([flip(t[0], 2), flip(t[0], 1), flip(t[1], 3), flip(t[2], 4), flip(t[2], 4)])
    m0, f0 = same(qd, t, M.params(cross_check=0, ratio=0))
    m1, f1 = same(qd, t, M.params(cross_check=1, ratio=0))
    assert m0["query"].tolist() == [0, 1, 2, 3, 4] and m0["train"].tolist() == [0, 0, 1, 2, 2]
    assert m1["query"].tolist() == [1, 2, 3]              # query 0 loses train 0 to query 1, query 4 ties with 3 and loses
    assert (f0[:, :3] == f1[:, :3]).all() and (f0[:, 3] == -1).all() and f1[:, 3].tolist() == [1, 1, 2, 3, 3]
    mutual = [r for r in m0.tolist() if f1[r[0], 3] == r[0]]
    assert m1.tolist() == mutual


def test_empty_sets():
    rng = np.random.default_rng(7)
    d = rand_desc(rng, 4)
    none = np.zeros((0, 32), np.uint8)
    for p in (M.params(), M.stereo_params()):
        k4, k0 = kps([1.0] * 4), kps([])
        m, f = same(none, d, p, k0, k4)
        assert len(m) == 0 and f.shape == (0, 4)
        m, f = same(d, none, p, k4, k0)
        assert len(m) == 0 and (f == -1).all() and f.shape == (4, 4)
        m, f = same(none, none, p, k0, k0)
        assert len(m) == 0 and f.shape == (0, 4)


def test_planted_motion_through_the_orb_restatement():
    """Two crops of one noise image, offset by (dx, dy): a keypoint pair of level 0 with identical descriptors is the same image
    point, so its offset is exactly (dx, dy).  Structural: no share of the matches is asserted."""
    dx, dy = 7, 3
    img = np.kron(np.random.default_rng(8).integers(0, 256, (70, 100)), np.ones((2, 2), np.int64)).astype(np.uint8)
    a, b = img[dy:dy + 120, dx:dx + 180], img[:120, :180]          # a(x, y) = b(x + dx, y + dy)
    (ka, da), (kb, db) = N.orb(a, 300)[:2], N.orb(b, 300)[:2]
    m, _ = M.match(da, db, M.params())
    exact = [r for r in m if r["distance"] == 0 and ka["octave"][r["query"]] == 0 and kb["octave"][r["train"]] == 0]
    assert len(exact) >= 1
    for r in exact:
        assert kb["x"][r["train"]] - ka["x"][r["query"]] == dx and kb["y"][r["train"]] - ka["y"][r["query"]] == dy

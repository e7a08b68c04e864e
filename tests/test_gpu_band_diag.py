"""GPU parity tests (-m gpu) of the banded WTA's second recomputed path (CART_OPT_BAND_DIAG, default on): under plan "band_up" wta_band_kernel
rebuilds the up-right diagonal {dx = +1, dy = -1} (the oracle's path 7) inside its tile of 64 columns x K rows -- the predecessor bytes travel
from lane group to lane group through LDS -- and reads from that path's slab only the row under each band and the column left of each tile.
What the aggregation launch writes, the plan names and describe_plan do not change.  Every comparison here is bit-exact.

The engine accepts images from 16 x 8 pixels up (cart_engine_create): the band-edge heights below 8 (1, K - 1 for K <= 8, K and K + 1 for K = 4)
cannot be run, and test_heights_below_the_smallest_image_are_refused asserts that they are refused.  Every width asked for (17 .. 129) is accepted."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from cartslam import _lib, synth
from test_gpu_parity import dev, make_engine, torch_cuda  # noqa: F401  (torch_cuda: fixture)

pytestmark = pytest.mark.gpu
D, P = 128, 8
BAND_ROWS = (4, 8, 16)
UR = 7                       # the oracle's path index of direction (+1, -1)
PENALTIES = ((10, 120), (29, 224))   # the second lets a path cost (a state byte handed through LDS) pass 151, the most the defaults reach
WIDTHS = (17, 63, 64, 65, 129)       # a one-wave partial tile, a tile one short, a full tile, two tiles (the second one column), three tiles
OPT_BAND_DIAG = 9


def heights(k):
    """the band-edge heights the engine accepts, and 33 rows for every K (2 K + 1 at K = 16): the height whose paths are long enough for bytes above 151"""
    return sorted({h for h in (1, k - 1, k, k + 1, 2 * k + 1) if h >= 8} | {33})


def frames(w, h, n, seed):
    """n distinct frames of a scene with true matches: the cost of a wrong disparity then climbs by its matching cost on every step of a path
    until P2 caps it, so under P2 = 224 the paths of the 33-row image pass 151 (a 9-row image cannot)."""
    return synth.make_batch(n, w, h, D, 0, seed=seed)


def oracle_maps(l, r, md, p1, p2, uniq=12, drop=(), twice=()):
    """the oracle's (WTA left, WTA right, disparity, the slab of path 7) of one pair; drop / twice: path indices left out of / counted twice in the sum"""
    cl, cr = O.census(l), O.census(r)
    S = np.zeros(l.shape + (D,), np.uint16)
    ur = None
    for i in range(P):
        Lp = O.aggregate_path(cl, cr, D, md, p1, p2, *O.path_dir(i))
        if i == UR:
            ur = Lp
        S += Lp.astype(np.uint16) * np.uint16((i not in drop) + (i in twice))
    wl, wr = O.wta(S, uniq)
    return wl, wr, O.lr_check_range(O.median3x3(wl), O.median3x3(wr), l, md), ur


@functools.lru_cache(maxsize=None)
def edge_reference(w, h, pen):
    """computed once per shape and penalties, shared by the three K; never modified"""
    p1, p2 = pen
    ls, rs = frames(w, h, 2, 1000 * w + h)
    exp = [oracle_maps(ls[f], rs[f], 0, p1, p2) for f in range(2)]
    for f in range(2):
        assert (exp[f][2] == O.disparity_module(ls[f], rs[f], D, P, 0, p1=p1, p2=p2)).all()   # the stages above are the oracle's module
    return ls, rs, exp


def run_maps(eng, L, R, n):
    d = eng.compute_disparity(L, R).cpu().numpy()
    return d, [eng.debug_read(32, frame_slot=f).copy() for f in range(n)], [eng.debug_read(33, frame_slot=f).copy() for f in range(n)]


def assert_same(a, b, what):
    assert (a[0] == b[0]).all(), f"{what}: {int((a[0] != b[0]).sum())} disparities differ"
    for f in range(len(a[1])):
        assert (a[1][f] == b[1][f]).all(), f"{what}: frame {f} wta left, {int((a[1][f] != b[1][f]).sum())} differ"
        assert (a[2][f] == b[2][f]).all(), f"{what}: frame {f} wta right, {int((a[2][f] != b[2][f]).sum())} differ"


def assert_oracle(got, exp, what):
    for f, (wl, wr, d, _) in enumerate(exp):
        assert (got[1][f] == wl).all(), f"{what}: frame {f} wta left against the oracle, {int((got[1][f] != wl).sum())} differ"
        assert (got[2][f] == wr).all(), f"{what}: frame {f} wta right against the oracle, {int((got[2][f] != wr).sum())} differ"
        assert (got[0][f] == d).all(), f"{what}: frame {f} disparity against the oracle"


def assert_diag_runs(eng, n, per_launch=None):
    """a silent fall-back to another plan or to the option's other value would pass every comparison"""
    assert eng.describe_plan(n) == {"frames_per_launch": per_launch or n, "plan": "band_up", "slabs_written": 7}
    assert eng.get_option(OPT_BAND_DIAG) == 1


# ------------------------------------------------------------------ 1. tile and band edges
@pytest.mark.parametrize("pen", PENALTIES)
@pytest.mark.parametrize("k", BAND_ROWS)
@pytest.mark.parametrize("w", WIDTHS)
def test_tile_and_band_edges(torch_cuda, w, k, pen):
    """every height of the K that the engine accepts: two distinct frames, the option on against the oracle, against the option off and against plan slabs"""
    torch = torch_cuda
    above = 0
    for h in heights(k):
        ls, rs, exp = edge_reference(w, h, pen)
        above += sum(int((e[3] > 151).sum()) for e in exp)
        L, R = dev(torch, ls), dev(torch, rs)
        eng = make_engine(w, h, D, P, 0, inflight=2, plan="band_up", p1=pen[0], p2=pen[1])
        eng.set_band_rows(k)
        assert_diag_runs(eng, 2)
        on = run_maps(eng, L, R, 2)
        assert_oracle(on, exp, f"{w}x{h} K={k} {pen}")
        eng.set_band_diag(False)
        assert eng.get_option(OPT_BAND_DIAG) == 0 and eng.describe_plan(2)["plan"] == "band_up"
        assert_same(run_maps(eng, L, R, 2), on, f"{w}x{h} K={k} {pen}: option off")
        eng.set_band_diag(True)
        eng.set_plan("slabs")
        assert eng.describe_plan(2)["plan"] == "slabs"
        assert_same(run_maps(eng, L, R, 2), on, f"{w}x{h} K={k} {pen}: plan slabs")
        eng.close()
    if pen[1] == 224:
        assert above > 0, "P2 = 224: no byte of path 7 above 151, the most the default penalties can reach"


def test_heights_below_the_smallest_image_are_refused(torch_cuda):
    from cartslam import EngineError
    for h in sorted({h for k in BAND_ROWS for h in (1, k - 1, k, k + 1, 2 * k + 1) if h < 8}):
        with pytest.raises(EngineError):
            make_engine(64, h, D, P, 0)


# ------------------------------------------------------------------ 2. a scene in which the diagonal decides
def test_the_diagonal_decides(torch_cuda):
    """The oracle's disparity of this pair changes when path 7 alone is left out of the cost sum, and when it is counted twice (checked here on the
    CPU): an implementation that drops or double-counts the rebuilt path cannot give the oracle's bits."""
    torch = torch_cuda
    w, h, md = 150, 41, 4   # three tiles (the last of 22 columns), six bands at K = 8 (the bottom one a single row)
    ls, rs = synth.make_batch(2, w, h, D, md, seed=4242)
    exp = [oracle_maps(ls[f], rs[f], md, 10, 120) for f in range(2)]
    for f in range(2):
        for variant in ({"drop": (UR,)}, {"twice": (UR,)}):
            wl, wr, d, _ = oracle_maps(ls[f], rs[f], md, 10, 120, **variant)
            assert (wl != exp[f][0]).any() and (d != exp[f][2]).any(), f"frame {f}: path 7 does not decide anything here ({variant})"
    L, R = dev(torch, ls), dev(torch, rs)
    eng = make_engine(w, h, D, P, md, inflight=2, plan="band_up")
    for k in BAND_ROWS:
        eng.set_band_rows(k)
        assert_diag_runs(eng, 2)
        assert_oracle(run_maps(eng, L, R, 2), exp, f"K={k}")
    eng.close()


# ------------------------------------------------------------------ 3. launch shapes
@pytest.mark.parametrize("n", [8, 3])
def test_launch_shapes(torch_cuda, n):
    """one launch of 8 distinct frames (XCD-decoded grid of the aggregation launch, plain horizontal scans) and one of 3 (split scans): every frame
    against the oracle"""
    torch = torch_cuda
    w, h, md = 201, 45, 4
    ls, rs = synth.make_batch(n, w, h, D, md, seed=60 + n)
    exp = [oracle_maps(ls[f], rs[f], md, 10, 120) for f in range(n)]
    assert all((exp[0][0] != exp[f][0]).any() for f in range(1, n)), "the frames are not distinct"
    eng = make_engine(w, h, D, P, md, inflight=n, plan="band_up")
    assert_diag_runs(eng, n)
    assert_oracle(run_maps(eng, dev(torch, ls), dev(torch, rs), n), exp, f"{n} frames")
    eng.close()


# ------------------------------------------------------------------ 4. the option
def test_option_alternates_on_one_engine(torch_cuda):
    torch = torch_cuda
    w, h, n, md = 201, 45, 4, 4
    ls, rs = synth.make_batch(n, w, h, D, md, seed=77)
    L, R = dev(torch, ls), dev(torch, rs)
    eng = make_engine(w, h, D, P, md, inflight=n)   # AUTO: 4 frames take band_up
    assert_diag_runs(eng, n)
    ref = run_maps(eng, L, R, n)
    assert_oracle(ref, [oracle_maps(ls[f], rs[f], md, 10, 120) for f in range(n)], "default")
    for on in (False, True, False, True):
        eng.set_band_diag(on)
        assert eng.get_option(OPT_BAND_DIAG) == int(on) and eng.describe_plan(n)["plan"] == "band_up"
        assert_same(run_maps(eng, L, R, n), ref, f"option {'on' if on else 'off'}")
    eng.set_band_rows(8, probe=True)   # with the probe the option is ignored: all 8 slabs are read
    eng.set_plan("band_up")
    assert eng.describe_plan(n) == {"frames_per_launch": n, "plan": "band_up", "slabs_written": 8}
    assert_same(run_maps(eng, L, R, n), ref, "probe")
    eng.close()


def test_option_on_an_engine_without_the_plan(torch_cuda):
    """a D = 64 engine accepts the option, keeps it and still answers slabs"""
    torch = torch_cuda
    assert _lib.OPT_BAND_DIAG == OPT_BAND_DIAG
    w, h, n = 200, 40, 4
    ls, rs = synth.make_batch(n, w, h, 64, 4, seed=9)
    eng = make_engine(w, h, 64, 8, 4, inflight=n, plan="band_up")
    assert eng.get_option(OPT_BAND_DIAG) == 1
    for on in (False, True):
        eng.set_band_diag(on)
        assert eng.get_option(OPT_BAND_DIAG) == int(on)
        assert eng.describe_plan(n) == {"frames_per_launch": n, "plan": "slabs", "slabs_written": 8}
        got = eng.compute_disparity(dev(torch, ls), dev(torch, rs)).cpu().numpy()
        assert (got[0] == O.disparity_module(ls[0], rs[0], 64, 8, 4)).all()
    from cartslam import EngineError
    with pytest.raises(EngineError):
        eng._check(eng._lib.cart_engine_set_option(eng._h, OPT_BAND_DIAG, 2), "cart_engine_set_option")
    eng.close()

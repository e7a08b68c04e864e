"""cart_optical_flow_pyramid (spec S21) on the GPU: bit-exact against the numpy restatement (np_flow), level by
level through cart_flow_debug_level -- images, then flows -- and then the S10.5 result; both paths of the refinement kernel
(previous features staged in LDS / gathered from global memory) give those bits.

The 1242x375 case (L = 4, R = 4, r = 2) is not in this file: the restatement takes 5 s to 25 s of CPU time at that size, more than a
test here may.  profiles/tools/flow_pyramid_full_size.py runs it (every level and the result bit-exact on both paths:
profiles/flow_pyramid.txt)."""
import threading

import numpy as np
import pytest

import np_flow as F
import oracle_lib as O
from cartslam import Engine, EngineError, synth
from test_flow_pyramid_spec import SHIFT_FLOOR, SHIFT_PARAMS, exact_share, shift_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gray(a):
    return a if a.ndim == 2 else O.bgr2gray(a)


def synth_pair(w, h, seed, ch=1, step=1):
    cur, _, _ = synth.make_pair(w, h, 64, 4, seed=seed, frame=step, channels=ch)
    prev, _, _ = synth.make_pair(w, h, 64, 4, seed=seed, frame=0, channels=ch)   # the scene moves 2 px per frame
    return cur, prev


def noise_pair(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)


def check(torch, eng, cur, prev, pitched=False, **p):
    """One call on each path of the refinement kernel against the restatement, level by level.  -> the expected level flows."""
    exp, ec, ep, ef = F.pyramid_flow(gray(cur), gray(prev), want_levels=True, **p)
    dc, dp = dev(torch, cur), dev(torch, prev)
    if pitched:   # rows 5 pixels longer than the image
        pad = (0, 5) if cur.ndim == 2 else (0, 0, 0, 5)
        dc = torch.nn.functional.pad(dc, pad)[:, :cur.shape[1]]
        dp = torch.nn.functional.pad(dp, pad)[:, :cur.shape[1]]
        assert not dc.is_contiguous()
    for gather in (False, True):
        eng.set_flow_gather(gather)
        got = eng.optical_flow_pyramid(dc, dp, levels=p["levels"], radius=p["radius"], refine_radius=p["refine_radius"], block=p["block"],
                                       median=bool(p["median"])).cpu().numpy()
        for l in range(len(ef)):
            assert (eng.flow_debug_level(l, 0) == ec[l]).all(), ("cur image", l)
            assert (eng.flow_debug_level(l, 1) == ep[l]).all(), ("prev image", l)
        for l in range(len(ef) - 1, -1, -1):   # coarsest first: a finer level inherits a coarser one's error
            gl = eng.flow_debug_level(l, 2)
            assert (gl == ef[l]).all(), ("flow", l, "gather" if gather else "auto", int((gl != ef[l]).any(axis=-1).sum()))
        with pytest.raises(EngineError):
            eng.flow_debug_level(len(ef), 2)   # a level that call did not build
        assert (got == exp).all()
    eng.set_flow_gather(False)
    return ef


CASES = [
    # name, w, h, channels, pitched, levels, R, r, B, levels used
    ("gray", 200, 80, 1, False, 3, 4, 2, 2, 3),
    ("bgr_pitched_odd", 131, 53, 3, True, 4, 4, 2, 2, 2),
    ("level0_only", 64, 16, 1, False, 4, 4, 2, 2, 1),
    ("wide_radii", 333, 41, 1, False, 3, 16, 4, 3, 2),   # 84 x 11 would be too low for a level: two levels, the coarse one 167 x 21
    ("narrow_coarse", 47, 33, 1, False, 2, 2, 1, 1, 2),  # level 1 is 24 x 17: narrower than a refinement tile, the smallest a level gets
    ("r3", 90, 40, 1, True, 2, 3, 3, 2, 2),
]


@pytest.mark.parametrize("median", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_levels_and_flow_match_the_restatement(torch_cuda, case, median):
    _, w, h, ch, pitched, levels, R, r, B, used = case
    assert len(F.level_sizes(w, h, levels)) == used
    eng = Engine(w, h, num_disparities=0, paths=0, max_inflight=2)
    cur, prev = synth_pair(w, h, 70 + w, ch)
    ef = check(torch_cuda, eng, cur, prev, pitched, levels=levels, radius=R, refine_radius=r, block=B, median=median)
    assert any((f != 0).any() for f in ef)
    flat = np.full(cur.shape, 77, np.uint8)
    got = eng.optical_flow_pyramid(dev(torch_cuda, flat), dev(torch_cuda, flat), levels, R, r, B, bool(median)).cpu().numpy()
    assert (got == 0).all()
    eng.close()


@pytest.mark.parametrize("median", [1, 0])
def test_garbage_priors_take_the_gather_path(torch_cuda, median):
    """Two independent noise images: the coarse winners are arbitrary, so without the median the priors of a 32 x 8 tile spread
    over more previous-frame positions than the kernel stages (4096 features) and those tiles gather."""
    w, h = 96, 64
    eng = Engine(w, h, num_disparities=0, paths=0, max_inflight=2)
    cur, prev = noise_pair(w, h, 5)
    ef = check(torch_cuda, eng, cur, prev, levels=3, radius=16, refine_radius=2, block=2, median=median)
    if not median:   # the staged window of every level-0 tile, from the restatement's level-1 flow
        over = 0
        for ty in range(0, h // 2, 4):
            for tx in range(0, w // 2, 16):
                pr = 2 * ef[1].astype(np.int64)[ty:ty + 4, tx:tx + 16]
                pw = 32 + 8 + int(pr[..., 0].max() - pr[..., 0].min()); ph = 8 + 8 + int(pr[..., 1].max() - pr[..., 1].min())
                over += pw * ph > 4096
        assert over >= 8, over
    eng.close()


@pytest.mark.parametrize("median", [1, 0])
def test_discontinuous_priors(torch_cuda, median):
    """Frames 0 and 8 of one synthetic sequence: the boxes move 16 px against the background."""
    w, h = 256, 96
    eng = Engine(w, h, num_disparities=0, paths=0, max_inflight=2)
    cur, prev = synth_pair(w, h, 4242, step=8)
    ef = check(torch_cuda, eng, cur, prev, levels=3, radius=4, refine_radius=2, block=2, median=median)
    assert len({tuple(v) for v in ef[0].reshape(-1, 2)[::7]}) > 2   # more than one motion
    eng.close()


def test_single_level_equals_optical_flow_and_the_oracle(torch_cuda):
    torch = torch_cuda
    for (w, h, R, B, ch) in ((200, 80, 6, 2, 1), (131, 53, 4, 1, 3)):
        eng = Engine(w, h, num_disparities=0, paths=0, max_inflight=2)
        cur, prev = synth_pair(w, h, 50 + w, ch)
        got = eng.optical_flow_pyramid(dev(torch, cur), dev(torch, prev), levels=1, radius=R, block=B, median=False).cpu().numpy()
        assert (eng.flow_debug_level(0, 2).astype(np.int32) * 32 == got).all()
        assert (got == eng.optical_flow(dev(torch, cur), dev(torch, prev), R, B).cpu().numpy()).all()
        assert (got == O.block_flow(gray(cur), gray(prev), R, B)).all()
        eng.close()


def test_large_shift(torch_cuda):
    cur, prev = shift_pair()
    eng = Engine(cur.shape[1], cur.shape[0], num_disparities=0, paths=0, max_inflight=2)
    p = SHIFT_PARAMS
    got = eng.optical_flow_pyramid(dev(torch_cuda, cur), dev(torch_cuda, prev), p["levels"], p["radius"], p["refine_radius"], p["block"],
                                   bool(p["median"])).cpu().numpy()
    share = exact_share(got)
    print("share", share)
    assert share >= SHIFT_FLOOR
    assert exact_share(eng.optical_flow(dev(torch_cuda, cur), dev(torch_cuda, prev), 16, 2).cpu().numpy()) < 0.05
    eng.close()


def test_argument_errors_raise(torch_cuda):
    torch = torch_cuda
    w, h = 96, 48
    eng = Engine(w, h, num_disparities=0, paths=0, max_inflight=2)
    with pytest.raises(EngineError):
        eng.flow_debug_level(0, 2)   # no call yet
    cur, prev = (dev(torch, a) for a in synth_pair(w, h, 3))
    for bad in (dict(levels=0), dict(levels=7), dict(radius=0), dict(radius=17), dict(refine_radius=0), dict(refine_radius=5), dict(block=0),
                dict(block=4)):
        with pytest.raises(EngineError):
            eng.optical_flow_pyramid(cur, prev, **bad)
    with pytest.raises(EngineError):
        eng.optical_flow_pyramid(cur[:, :90], prev[:, :90])   # not the engine's size
    lib, fp = eng._lib, __import__("cartslam")._lib.FlowParams(4, 4, 2, 2, 2)   # median = 2; then NULL pointers and short steps
    import ctypes as C
    out = torch.empty((h, w, 2), dtype=torch.int16, device="cuda")
    args = lambda **k: [k.get("e", eng._h), k.get("cur", cur.data_ptr()), k.get("cs", w), prev.data_ptr(), w, 1, k.get("fp", C.byref(fp)),
                        k.get("out", out.data_ptr()), k.get("os", w * 4), None]
    assert lib.cart_optical_flow_pyramid(*args()) != 0 and b"median" in lib.cart_last_error(eng._h)
    fp.median = 1
    for k in (dict(cur=None), dict(out=None), dict(fp=None), dict(cs=w - 1), dict(os=w * 4 - 4), dict(os=w * 4 + 2), dict(e=None)):
        assert lib.cart_optical_flow_pyramid(*args(**k)) != 0, k
    assert lib.cart_optical_flow_pyramid(*args()) == 0
    torch.cuda.synchronize()
    buf = np.empty((h, w), np.uint8)
    assert lib.cart_flow_debug_level(eng._h, 0, 3, buf.ctypes.data, buf.nbytes) != 0
    assert lib.cart_flow_debug_level(eng._h, 0, 0, buf.ctypes.data, buf.nbytes - 1) != 0
    assert lib.cart_flow_debug_level(eng._h, 0, 0, buf.ctypes.data, buf.nbytes) == 0
    eng.close()


def test_two_threads_equal_two_serial_calls(torch_cuda):
    torch = torch_cuda
    w, h = 200, 80
    eng = Engine(w, h, num_disparities=0, paths=0, max_inflight=2)
    pairs = [synth_pair(w, h, 900 + i) for i in range(2)]
    serial = [eng.optical_flow_pyramid(dev(torch, c), dev(torch, p), levels=3).cpu().numpy() for c, p in pairs]
    results, levels, errors = [None] * 2, [None] * 2, []

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _ in range(3):
                    out = eng.optical_flow_pyramid(dev(torch, pairs[i][0]), dev(torch, pairs[i][1]), levels=3)
                s.synchronize()
            results[i] = out.cpu().numpy()
            levels[i] = eng.flow_debug_level(1, 2)   # this thread's call, not the other's
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert (results[i] == serial[i]).all(), f"thread {i}"
        want = F.pyramid_flow(pairs[i][0], pairs[i][1], levels=3, want_levels=True)[3][1]
        assert (levels[i] == want).all(), f"thread {i} level 1"
    eng.close()

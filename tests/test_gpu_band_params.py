"""GPU parity tests (-m gpu) of launch plan "band_up" off its defaults.  test_gpu_band_plan.py runs the plan at P1 = 10, P2 = 120, uniqueness 12
and reads no slab back.  Here, always against the CPU oracle and bit for bit:

  * engine parameters: a seeded sweep over size / min_disparity / P1 / P2 / uniqueness / smoothing / channels / scene / frames per call, and the
    corners of the accepted range -- P2 = 224 makes path costs reach 255, the whole byte a checkpoint cell holds;
  * the checkpoint rows themselves (debug_read of the "up" slab), the other seven slabs of the CKPT launch, and the rows the launch must leave alone;
  * launches that are a multiple of 8 DISTINCT frames at full size (XCD placement: frames x and x + 8 share an XCD);
  * the two most lopsided images the engine accepts;
  * the other entry points: compute_disparity_multi, several host threads on one engine, the two-stream StereoPipeline under AUTO.

Every case that is meant to run the plan asserts describe_plan(n)["plan"] == "band_up": a fall-back to SLABS would pass every comparison."""
import threading

import numpy as np
import pytest

import oracle_lib as O
from cartslam import synth
from test_gpu_band_plan import BAND_ROWS, D, P, assert_same, run_maps
from test_gpu_parity import dev, make_engine, torch_cuda  # noqa: F401  (torch_cuda: fixture)

pytestmark = pytest.mark.gpu
UP = 1   # the oracle's path index of direction (0, -1): debug_read(16 + UP) is the slab that holds the checkpoint rows
BAND = {"frames_per_launch": None, "plan": "band_up", "slabs_written": 7}


def assert_band(eng, n, per_launch=None):
    assert eng.describe_plan(n) == dict(BAND, frames_per_launch=per_launch or n), eng.describe_plan(n)


def images(rng, kind, n, w, h, md, ch, seed):
    """n frames: kind "noise" = independent uniform bytes left and right (no structure, many ties and invalid pixels), else a synth scene"""
    if kind == "noise":
        shape = (n, h, w) if ch == 1 else (n, h, w, 3)
        return rng.integers(0, 256, shape).astype(np.uint8), rng.integers(0, 256, shape).astype(np.uint8)
    return synth.make_batch(n, w, h, D, md, seed=seed, channels=ch, scene=kind)


def oracle(l, r, md, p1, p2, uniq, radius, iters):
    return O.disparity_module(l, r, D, P, md, p1=p1, p2=p2, uniq=uniq, radius=radius, iterations=iters)


def checkpoint_rows(h, k):
    return np.arange(k, h, k)


def up_slab(l, r, md, p1, p2):
    g = (O.bgr2gray(l), O.bgr2gray(r)) if l.ndim == 3 else (l, r)
    return O.aggregate_path(O.census(g[0]), O.census(g[1]), D, md, p1, p2, 0, -1)


# ------------------------------------------------------------------ 1. engine parameters
SWEEP_SEED = 20261016


def sweep_cases():
    """(w, h, md, p1, p2, uniq, radius, iters, channels, frames, kind): shaped like test_randomized_configurations, restricted to D = 128 / 8 paths.
    Sizes, penalties, smoothing and channels are drawn; min_disparity and uniqueness walk through their lists (22 cases meet every value three times
    or more, in changing pairs).  P1 is drawn from the range a caller would use (0..29) in even cases and from everything the
    engine accepts (0..224) in odd ones; P2 from P1..224.  Frames per call 2..5 (fewer than 8 frames: the aggregation launch runs its split
    horizontal scans), and the last four cases 8 and 9 (plain scans; 8 also turns XCD placement on).
    The interpolation stage keeps a value v (disparity x 16) only if 16 min_disparity < v < width (oracle S9), so on a narrow image or with a large
    min_disparity it leaves nothing but invalid pixels: smoothing is switched off where fewer than 12 disparity levels would pass it,
    width < 16 (min_disparity + 12), under uniqueness 99 / 100, which leave too few pixels for it to work on, and on noise images, whose
    disparities are spread over all of D.  Widths start at min_disparity + 32: in a narrower image no candidate lies inside the right image and
    both WTA maps are constant (the 97-wide corner below is the narrow case with content)."""
    rng = np.random.default_rng(SWEEP_SEED)
    cases = []
    for i in range(22):
        md = (0, 1, 4, 17, 64)[i % 5]
        w = max(int(rng.integers(16, 421)), md + 32); h = int(rng.integers(8, 131))
        kind = "noise" if i % 3 == 2 else synth.SCENES[(i // 3 + i % 3) % len(synth.SCENES)]
        p1 = int(rng.integers(0, 30 if i % 2 == 0 else 225)); p2 = int(rng.integers(p1, 225))
        uniq = (12, 0, 99, 5, 100, 50)[(i + i // 6) % 6]   # shifted by one every round: noise images (i % 3 == 2) meet every value
        radius = int(rng.choice([-1, 1, 2, 3])); iters = int(rng.choice([1, 2, 5]))
        if w < 16 * (md + 12) or uniq >= 99 or kind == "noise":
            radius = -1
        ch = int(rng.choice([1, 3]))
        n = int(rng.integers(2, 6)) if i < 18 else (8, 9)[i % 2]
        cases.append((w, h, md, p1, p2, uniq, radius, iters, ch, n, kind))
    return cases


SWEEP = sweep_cases()


def sweep_reference(case):
    """the case's frames and, per frame, the oracle's (WTA left, WTA right, disparity after smoothing).  Guards on the reference alone, so that a
    re-seeded sweep cannot go vacuous unnoticed: the pair of WTA maps, which depends on every parameter but the smoothing, differs between the
    first two frames (on an image narrower than min_disparity the left map alone is constant); the disparity image before smoothing has valid
    pixels and differs between them; and where the case smooths, the smoothed image keeps valid pixels."""
    w, h, md, p1, p2, uniq, radius, iters, ch, n, kind = SWEEP[case]
    ls, rs = images(np.random.default_rng(7000 + case), kind, n, w, h, md, ch, seed=2000 + case)
    exp, raw = [], []
    for f in range(n):
        l, r = (O.bgr2gray(ls[f]), O.bgr2gray(rs[f])) if ch == 3 else (ls[f], rs[f])
        _, wl, wr, d = oracle_stages(l, r, md, p1, p2, uniq)
        raw.append(d)
        if radius > 0 and iters > 0:
            d = O.interpolate(d, radius, iters, md * 16, w)
        assert (d == oracle(ls[f], rs[f], md, p1, p2, uniq, radius, iters)).all()   # the stages above are the oracle's module
        exp.append((wl, wr, d))
    assert (exp[0][0] != exp[1][0]).any() or (exp[0][1] != exp[1][1]).any(), f"case {case}: the oracle's WTA maps do not differ between frames"
    assert (raw[0] != (md - 1) * 16).any() and (raw[0] != raw[1]).any(), f"case {case}: nothing to compare in the oracle's disparity"
    assert (exp[0][2] != -32768).any() and (exp[0][2] != exp[1][2]).any(), f"case {case}: nothing left to compare after smoothing"
    return ls, rs, exp


@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_band_up_randomized_parameters(torch_cuda, case):
    """every frame, every K: both WTA maps and the disparity against the oracle"""
    torch = torch_cuda
    w, h, md, p1, p2, uniq, radius, iters, ch, n, kind = SWEEP[case]
    ls, rs, exp = sweep_reference(case)
    eng = make_engine(w, h, D, P, md, radius=radius, iters=iters, inflight=n, plan="band_up", p1=p1, p2=p2, uniqueness_ratio=uniq)
    L, R = dev(torch, ls), dev(torch, rs)
    for k in BAND_ROWS:
        eng.set_band_rows(k)
        assert_band(eng, n)
        got = run_maps(eng, L, R, n)
        for f in range(n):
            what = f"case {case} {SWEEP[case]}, K={k}, frame {f}"
            assert (got[1][f] == exp[f][0]).all(), f"{what}: wta left, {int((got[1][f] != exp[f][0]).sum())} pixels differ"
            assert (got[2][f] == exp[f][1]).all(), f"{what}: wta right, {int((got[2][f] != exp[f][1]).sum())} pixels differ"
            assert (got[0][f] == exp[f][2]).all(), f"{what}: {int((got[0][f] != exp[f][2]).sum())} disparities differ"
    eng.close()


# (name, w, h, md, p1, p2, uniq, scene, smoothing radius): the corners of what cart_engine_create accepts.  P2 = 224: a path cost may reach
# 31 + 224 = 255.  The narrow image runs without smoothing: the interpolation stage drops every disparity >= the image width, i.e. all of them.
CORNERS = [
    ("p_0_0", 330, 75, 4, 0, 0, 12, "road", 2),
    ("p_0_224", 330, 75, 4, 0, 224, 12, "stripes", 2),
    ("p_29_224", 330, 75, 4, 29, 224, 12, "photometric", 2),
    ("p_224_224", 330, 75, 4, 224, 224, 12, "road", 2),
    ("uniq_0", 330, 75, 4, 10, 120, 0, "stripes", 2),
    ("uniq_100", 330, 75, 4, 10, 120, 100, "photometric", 2),
    ("md_64_narrow", 97, 75, 64, 10, 120, 12, "road", -1),   # narrower than D: every right feature partly out of range
]


def corner_reference(corner, n):
    """the corner's frames, the oracle's disparities, and the guards that hold on the reference alone: the corner's parameters change the
    oracle's output on these images (against P1 = 10, P2 = 120, uniqueness 12, min_disparity 4) and leave valid pixels, and with P2 = 224 the oracle's "up" costs
    hold the value 255 on a checkpoint row of every K"""
    name, w, h, md, p1, p2, uniq, scene, radius = corner
    ls, rs = synth.make_batch(n, w, h, D, md, seed=31, scene=scene)
    exp = [oracle(ls[f], rs[f], md, p1, p2, uniq, radius, 1) for f in range(n)]
    assert (exp[0] != oracle(ls[0], rs[0], 4, 10, 120, 12, radius, 1)).any(), f"{name}: the oracle gives the default parameters' output: a vacuous case"
    assert (exp[0] != -32768).any() and (exp[0] != exp[1]).any(), f"{name}: nothing to compare in the oracle's output"
    if p2 == 224:
        up = up_slab(ls[0], rs[0], md, p1, p2)
        for k in BAND_ROWS:
            assert (up[checkpoint_rows(h, k)] == 255).any(), f"{name}: no checkpoint cell of K={k} holds 255"
    return ls, rs, exp


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("corner", CORNERS, ids=[c[0] for c in CORNERS])
def test_band_up_parameter_corners(torch_cuda, corner, n):
    """3 frames: split horizontal scans; 8 frames: plain scans and XCD placement.  Disparities against the oracle, WTA maps against SLABS."""
    torch = torch_cuda
    name, w, h, md, p1, p2, uniq, scene, radius = corner
    ls, rs, exp = corner_reference(corner, n)
    L, R = dev(torch, ls), dev(torch, rs)
    eng = make_engine(w, h, D, P, md, radius=radius, iters=1, inflight=n, plan="slabs", p1=p1, p2=p2, uniqueness_ratio=uniq)
    ref = run_maps(eng, L, R, n)
    for f in range(n):
        assert (ref[0][f] == exp[f]).all(), f"{name}: slabs, frame {f} against the oracle"
    eng.set_plan("band_up")
    for k in BAND_ROWS:
        eng.set_band_rows(k)
        assert_band(eng, n)
        assert_same(run_maps(eng, L, R, n), ref, f"{name} n={n} K={k}")
    eng.close()


# ------------------------------------------------------------------ 2. the checkpoint rows, read back
def oracle_stages(l, r, md, p1, p2, uniq=12):
    """-> (the 8 path slabs, WTA left, WTA right, disparity before interpolation) of one gray frame"""
    cl, cr = O.census(l), O.census(r)
    slabs = [O.aggregate_path(cl, cr, D, md, p1, p2, *O.path_dir(i)) for i in range(P)]
    S = np.zeros(slabs[0].shape, np.uint16)
    for s in slabs:
        S += s
    wl, wr = O.wta(S, uniq)
    return slabs, wl, wr, O.lr_check_range(O.median3x3(wl), O.median3x3(wr), l, md)


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("p1,p2", [(10, 120), (29, 224)])
@pytest.mark.parametrize("k", BAND_ROWS)
def test_checkpoint_rows_against_the_oracle(torch_cuda, k, p1, p2, n):
    """After a BAND_UP call the "up" slab holds the oracle's costs on the rows y % K == 0, y > 0, cell for cell, and the other seven slabs are the
    oracle's in full (the CKPT instantiation of aggregate_kernel is a kernel body of its own for every direction) -- heights with h % K in
    {0, 1, K - 1}, widths that are no multiple of 64, 3 frames (split horizontal scans) and 8 (plain scans, XCD placement), every frame."""
    torch = torch_cuda
    assert O.path_dir(UP) == (0, -1)
    for w, h in ((150, 48), (201, 49), (77, 48 + k - 1)):
        ls, rs = synth.make_batch(n, w, h, D, 4, seed=900 + w + k, scene="photometric" if p2 == 224 else "road")
        eng = make_engine(w, h, D, P, 4, inflight=n, plan="band_up", p1=p1, p2=p2)
        eng.set_band_rows(k)
        assert_band(eng, n)
        disp = eng.compute_disparity(dev(torch, ls), dev(torch, rs)).cpu().numpy()
        ys = checkpoint_rows(h, k)
        assert len(ys) >= 2
        above = 0
        for f in range(n):
            slabs, wl, wr, exp = oracle_stages(ls[f], rs[f], 4, p1, p2)
            for i in range(P):
                got = eng.debug_read(16 + i, frame_slot=f)
                if i == UP:
                    assert (got[ys] == slabs[i][ys]).all(), f"{w}x{h} frame {f}: {int((got[ys] != slabs[i][ys]).sum())} checkpoint cells differ"
                else:
                    assert (got == slabs[i]).all(), f"{w}x{h} frame {f} path {i}: {int((got != slabs[i]).sum())} cells differ"
            assert (eng.debug_read(32, frame_slot=f) == wl).all(), f"{w}x{h} frame {f} wta left"
            assert (eng.debug_read(33, frame_slot=f) == wr).all(), f"{w}x{h} frame {f} wta right"
            assert (disp[f] == exp).all(), f"{w}x{h} frame {f} disparity"
            above += int((slabs[UP][ys] > 151).sum())
        assert above > 0 or p2 != 224, "P2 = 224: no checkpoint cell above 151, the most the default penalties can reach"
        eng.close()


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("k", BAND_ROWS)
def test_band_up_writes_the_checkpoint_rows_only(torch_cuda, k, n):
    """the other rows of the "up" slab "keep whatever an earlier launch left".  SLABS on images A, then BAND_UP on images B in the same
    slots: row 0 and the rows between the checkpoints still hold A's "up" costs, the checkpoint rows hold B's -- what slabs_written == 7 says."""
    torch = torch_cuda
    w, h = 330, 75
    la, ra = synth.make_batch(n, w, h, D, 4, seed=1)
    lb, rb = synth.make_batch(n, w, h, D, 4, seed=2, scene="stripes")
    ys = checkpoint_rows(h, k)
    rest = np.setdiff1d(np.arange(h), ys)
    assert rest[0] == 0
    eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=n, plan="slabs")
    eng.compute_disparity(dev(torch, la), dev(torch, ra))
    ups_a = [eng.debug_read(16 + UP, frame_slot=f).copy() for f in range(n)]
    eng.set_plan("band_up"); eng.set_band_rows(k)
    assert_band(eng, n)
    got_d = eng.compute_disparity(dev(torch, lb), dev(torch, rb)).cpu().numpy()
    for f in range(n):
        ua, ub = up_slab(la[f], ra[f], 4, 10, 120), up_slab(lb[f], rb[f], 4, 10, 120)
        assert (ua[ys] != ub[ys]).any() and (ua[rest] != ub[rest]).any()   # else a store too many or too few could not show
        assert (ups_a[f] == ua).all(), f"frame {f}: slabs on A"
        got = eng.debug_read(16 + UP, frame_slot=f)
        assert (got[ys] == ub[ys]).all(), f"frame {f}: {int((got[ys] != ub[ys]).sum())} checkpoint cells are not B's"
        assert (got[rest] == ua[rest]).all(), f"frame {f}: {int((got[rest] != ua[rest]).sum())} cells off the checkpoint rows were written"
        assert (got_d[f] == oracle(lb[f], rb[f], 4, 10, 120, 12, 2, 1)).all(), f"frame {f}: disparity of B"
    eng.close()


# ------------------------------------------------------------------ 3. distinct frames in a launch that is a multiple of 8, full size
def test_sixteen_distinct_frames_at_full_size(torch_cuda):
    """1242 x 375: 8 x census_elems is 5.3 MiB of the 8 MiB up to which a launch of 8 k frames is decoded per XCD (xcd_placement), so frames x and
    x + 8 run on one XCD -- and here they are different images.  Frames 0, 7, 8, 15 against the oracle, all 16 against SLABS (disparity and both
    WTA maps), K = 8 (the default) and K = 4 (most checkpoint rows)."""
    torch = torch_cuda
    w, h, n = 1242, 375, 16
    ls, rs = synth.make_batch(n, w, h, D, 4, seed=616)
    L, R = dev(torch, ls), dev(torch, rs)
    eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=n, plan="slabs")
    ref = run_maps(eng, L, R, n)
    exp = {f: O.disparity_module(ls[f], rs[f], D, P, 4, radius=2, iterations=1) for f in (0, 7, 8, 15)}
    for f, e in exp.items():
        assert (ref[0][f] == e).all(), f"slabs, frame {f} against the oracle"
    assert (exp[0] != exp[8]).any() and (exp[7] != exp[15]).any()
    for x in range(8):   # the oracle-checked SLABS output stands in for the oracle on the other pairs (x, x + 8)
        assert (ls[x] != ls[x + 8]).any() and (ref[0][x] != ref[0][x + 8]).any() and (ref[1][x] != ref[1][x + 8]).any(), x
    eng.set_plan("band_up")
    for k in (8, 4):
        eng.set_band_rows(k)
        assert_band(eng, n)
        got = run_maps(eng, L, R, n)
        assert_same(got, ref, f"K={k}")
        for f, e in exp.items():
            assert (got[0][f] == e).all(), f"K={k}, frame {f} against the oracle"
    eng.close()


# ------------------------------------------------------------------ 4. the most lopsided images
@pytest.mark.parametrize("w,h,radius", [(16384, 8, 2), (16, 2000, -1)])
def test_band_up_extreme_shapes(torch_cuda, w, h, radius):
    """16384 x 8: 256 tiles in a row, two bands at K = 4 and one at K = 8 / 16 (no checkpoint row is ever read).  16 x 2000: one tile whose
    waves 2-7 lie past the image in every column, 500 / 250 / 125 bands; without smoothing, because the interpolation stage drops every disparity
    >= the image width and would leave nothing but invalid pixels to compare.  A batch of three distinct frames and a single frame, images as in
    test_extreme_shapes."""
    torch = torch_cuda
    rng = np.random.default_rng(w * 31 + h)
    base = rng.integers(0, 256, (3, h, w + 40)).astype(np.uint8)
    ls, rs = np.ascontiguousarray(base[:, :, 20:20 + w]), np.ascontiguousarray(base[:, :, 27:27 + w])
    exp = [O.disparity_module(ls[f], rs[f], D, P, 4, radius=radius, iterations=1) for f in range(3)]
    assert (exp[0] != exp[1]).any() and (exp[0] != -32768).any()
    L, R = dev(torch, ls), dev(torch, rs)
    eng = make_engine(w, h, D, P, 4, radius=radius, iters=1, inflight=3, plan="slabs")
    ref = run_maps(eng, L, R, 3)
    eng.set_plan("band_up")
    for k in BAND_ROWS:
        eng.set_band_rows(k)
        assert_band(eng, 3); assert_band(eng, 1)
        got = run_maps(eng, L, R, 3)
        assert_same(got, ref, f"K={k}")
        for f in range(3):
            assert (got[0][f] == exp[f]).all(), f"K={k}, frame {f}: {int((got[0][f] != exp[f]).sum())} pixels differ"
        assert (eng.compute_disparity(L[2], R[2]).cpu().numpy() == exp[2]).all(), f"K={k}, one frame"
    eng.close()


# ------------------------------------------------------------------ 5. the other ways in
def test_multi_entry_point_band_then_slabs(torch_cuda):
    """compute_disparity_multi with 19 separately allocated, row-padded frames, shuffled in memory, under AUTO: launches of 16 (BAND_UP) and 3 (SLABS)
    inside one call.  Equal to the batch entry point on every frame and to the oracle on both sides of the launch boundary."""
    torch = torch_cuda
    w, h, n = 320, 96, 19
    ls, rs = synth.make_batch(n, w, h, D, 4, seed=1919)
    eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=n)
    assert_band(eng, 16)
    assert eng.describe_plan(n)["frames_per_launch"] == 16
    assert eng.describe_plan(3) == {"frames_per_launch": 3, "plan": "slabs", "slabs_written": 8}
    L, R = dev(torch, ls), dev(torch, rs)
    want = eng.compute_disparity(L, R).cpu().numpy()
    order = np.random.default_rng(5).permutation(n)
    store = {int(f): (torch.nn.functional.pad(L[f], (0, 24)), torch.nn.functional.pad(R[f], (0, 40)),
                      torch.full((h, w + 8), -7, dtype=torch.int16, device="cuda")) for f in order}
    lefts = [store[f][0][:, :w] for f in range(n)]; rights = [store[f][1][:, :w] for f in range(n)]; outs = [store[f][2][:, :w] for f in range(n)]
    eng.compute_disparity_multi(lefts, rights, outs)
    torch.cuda.synchronize()
    for f in range(n):
        assert np.array_equal(outs[f].cpu().numpy(), want[f]), f
        assert (store[f][2][:, w:] == -7).all()   # nothing written past the row
    for f in (0, 15, 16, 18):
        assert (want[f] == O.disparity_module(ls[f], rs[f], D, P, 4, radius=2, iterations=1)).all(), f"frame {f} against the oracle"
    assert all((want[f] != want[f + 1]).any() for f in range(n - 1))
    eng.close()


def test_concurrent_host_threads_band_up(torch_cuda):
    """Eight host threads, each on its own stream, share one engine of 8 slots under forced BAND_UP; each calls three times with its own 4
    frames.  The slots form two ranges of 4, so calls of different streams run side by side and the checkpoint rows of one land in the slabs
    next to the other's."""
    torch = torch_cuda
    w, h, nt, nf = 256, 80, 8, 4
    eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=8, plan="band_up")
    assert_band(eng, nf)
    batches = [synth.make_batch(nf, w, h, D, 4, seed=300 + i, first_frame=5 * i, scene=synth.SCENES[i % len(synth.SCENES)]) for i in range(nt)]
    expected = [[O.disparity_module(ls[f], rs[f], D, P, 4, radius=2, iterations=1) for f in range(nf)] for ls, rs in batches]
    assert all((expected[i][0] != expected[(i + 1) % nt][0]).any() for i in range(nt))
    results, errors = [[] for _ in range(nt)], []

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                l, r = dev(torch, batches[i][0]), dev(torch, batches[i][1])
                outs = [eng.compute_disparity(l, r) for _ in range(3)]
                s.synchronize()
            results[i] = [o.cpu().numpy() for o in outs]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(nt)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(nt):
        assert len(results[i]) == 3
        for c, out in enumerate(results[i]):
            for f in range(nf):
                assert (out[f] == expected[i][f]).all(), f"thread {i}, call {c}, frame {f}: {int((out[f] != expected[i][f]).sum())} pixels differ"
    eng.close()


def test_two_stream_pipeline_under_auto(torch_cuda):
    """StereoPipeline(overlap=True) at D = 128 / 8 paths in batches of 8: AUTO runs BAND_UP while the side stream works on the previous batch's
    planes.  Every output equals the one-stream pipeline's, every disparity the oracle's."""
    torch = torch_cuda
    from cartslam.pipeline import StereoPipeline
    w, h, B, nb = 330, 120, 8, 3
    frames = [synth.make_batch(B, w, h, D, 4, seed=88, first_frame=B * k, scene=("road", "pole", "photometric")[k]) for k in range(nb)]
    batches = [(dev(torch, ls), dev(torch, rs)) for ls, rs in frames]
    torch.cuda.synchronize()
    results = {}
    for mode in ("one_stream", "side"):
        eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=2 * B)
        assert_band(eng, B)
        pipe = StereoPipeline(eng, provider="histogram_peak", update_interval=3, reset_interval=2, with_ccl=True, overlap=mode == "side")
        assert (pipe.side is not None) == (mode == "side")
        outs = [pipe.process_batch(l, r) for l, r in batches]
        torch.cuda.synchronize()
        results[mode] = [{k: o[k].cpu().numpy() for k in ("disparity", "planes", "ids", "n_components", "components", "params")} for o in outs]
        eng.close()
    for b, (one, side) in enumerate(zip(results["one_stream"], results["side"])):
        for key in one:
            if key == "components":   # rows past a frame's component count are not written
                for f in range(B):
                    nc = min(int(one["n_components"][f]), one[key].shape[1])
                    assert np.array_equal(one[key][f, :nc], side[key][f, :nc]), (b, key, f)
            else:
                assert np.array_equal(one[key], side[key]), (b, key)
        for f in range(B):
            exp = O.disparity_module(frames[b][0][f], frames[b][1][f], D, P, 4, radius=2, iterations=1)
            assert (side["disparity"][f] == exp).all(), f"batch {b}, frame {f} against the oracle"
    assert not np.array_equal(results["side"][0]["disparity"], results["side"][1]["disparity"])

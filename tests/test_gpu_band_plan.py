"""GPU parity tests (-m gpu) of launch plan "band_up": the aggregation launch stores the "up" path on every K-th row only (checkpoints, in
place in its slab) and wta_band_kernel recomputes the path inside tiles of 64 columns x K rows.  Like every plan it must give the bits of
plan "slabs" and of the CPU oracle on every output.

The engine accepts images from 16 x 8 pixels up (cart_engine_create), so the band-edge heights below 8 and the widths below 16 cannot be run:
for those the tests assert that the engine refuses the size, which is what a caller sees.

This file runs the plan at the default penalties and uniqueness ratio.  test_gpu_band_params.py beside it covers the rest: P1 / P2 / uniqueness /
min_disparity over the accepted range (path costs up to 255 in a checkpoint byte), the checkpoint rows and the other seven slabs read back against
the oracle and the rows the launch must not write, 16 distinct frames in one launch at full size, the 16384 x 8 and 16 x 2000 images, and the
compute_disparity_multi / host threads / two-stream pipeline entry points; test_gpu_parity.py runs the plan wherever it loops over the launch
plans at D = 128 with 8 paths (full-size scenes, KITTI frame sizes, the 4099-wide image, 8 distinct frames per launch, the S8 / S7 variants)."""
import numpy as np
import pytest

import oracle_lib as O
from cartslam import synth
from test_gpu_parity import dev, make_engine, torch_cuda  # noqa: F401  (torch_cuda: fixture)

pytestmark = pytest.mark.gpu
D, P = 128, 8
BAND_ROWS = (4, 8, 16)   # every K that is built (CART_OPT_BAND_ROWS)


def run_maps(eng, L, R, n):
    """disparity + the WTA's left / right maps of every frame slot of one call"""
    d = eng.compute_disparity(L, R).cpu().numpy()
    return d, [eng.debug_read(32, frame_slot=f).copy() for f in range(n)], [eng.debug_read(33, frame_slot=f).copy() for f in range(n)]


def assert_same(a, b, what):
    assert (a[0] == b[0]).all(), f"{what}: {int((a[0] != b[0]).sum())} disparities differ"
    for f in range(len(a[1])):
        assert (a[1][f] == b[1][f]).all(), f"{what}: frame {f} wta left"
        assert (a[2][f] == b[2][f]).all(), f"{what}: frame {f} wta right"


def band_vs_slabs(torch, w, h, md, n=2, ks=BAND_ROWS, seed=5, oracle_frames=(0,)):
    """forced band_up with every K against forced slabs (disparity after post / interpolate, both WTA maps) and against the oracle"""
    ls, rs = synth.make_batch(n, w, h, D, md, seed=seed)
    L, R = dev(torch, ls), dev(torch, rs)
    eng = make_engine(w, h, D, P, md, radius=2, iters=1, inflight=n, plan="slabs")
    ref = run_maps(eng, L, R, n)
    for f in oracle_frames:
        assert (ref[0][f] == O.disparity_module(ls[f], rs[f], D, P, md, radius=2, iterations=1)).all(), f"slabs, frame {f} against the oracle"
    eng.set_plan("band_up")
    for k in ks:
        eng.set_band_rows(k)
        assert eng.describe_plan(n) == {"frames_per_launch": n, "plan": "band_up", "slabs_written": 7}
        assert_same(run_maps(eng, L, R, n), ref, f"{w}x{h} md={md} K={k}")
    eng.close()


def test_band_up_at_the_bench_size(torch_cuda):
    """What bench.py runs: 1242x375, D=128, 8 paths, 16 frames per launch, post + interpolation on top; two distinct frames against the oracle."""
    torch = torch_cuda
    w, h, n = 1242, 375, 16
    ls, rs = synth.make_batch(2, w, h, D, 4, seed=31)
    ls, rs = np.concatenate([ls] * 8), np.concatenate([rs] * 8)
    L, R = dev(torch, ls), dev(torch, rs)
    eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=n, plan="slabs")
    ref = run_maps(eng, L, R, n)
    eng.set_plan("band_up")
    assert eng.describe_plan(n) == {"frames_per_launch": n, "plan": "band_up", "slabs_written": 7}
    assert_same(run_maps(eng, L, R, n), ref, "default K")
    for k in BAND_ROWS:
        eng.set_band_rows(k)
        assert_same(run_maps(eng, L, R, n), ref, f"K={k}")
    eng.close()
    for f in (0, 1):
        assert (ref[0][f] == O.disparity_module(ls[f], rs[f], D, P, 4, radius=2, iterations=1)).all(), f"frame {f} against the oracle"
    assert (ref[0][0] == ref[0][2]).all() and (ref[0][0] != ref[0][1]).any()


def edge_heights():
    hs = {37}   # a prime height
    for k in BAND_ROWS:
        hs |= {1, k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1}   # k + 1, 2k + 1: a bottom band of one row = the checkpoint row is the image's last row
    return sorted(hs)


@pytest.mark.parametrize("md", [0, 4])
@pytest.mark.parametrize("h", edge_heights())
def test_band_edges_in_height(torch_cuda, h, md):
    from cartslam import EngineError
    if h < 8:   # below the engine's smallest image: refused at creation
        with pytest.raises(EngineError):
            make_engine(200, h, D, P, md)
        return
    band_vs_slabs(torch_cuda, 200, h, md, seed=100 + h)


@pytest.mark.parametrize("md", [0, 4])
@pytest.mark.parametrize("w", [1, 63, 64, 65, 1243])
def test_band_edges_in_width(torch_cuda, w, md):
    """one tile minus a column, one tile, one tile plus a column, and a full-size width that is no multiple of anything (20 tiles, the last of 27 columns)"""
    from cartslam import EngineError
    if w < 16:
        with pytest.raises(EngineError):
            make_engine(w, 21, D, P, md)
        return
    band_vs_slabs(torch_cuda, w, 21, md, seed=200 + w)


def test_band_up_bgr_pitched(torch_cuda):
    """BGR input, non-tight pitches of inputs and output, a batch of frames"""
    torch = torch_cuda
    w, h, n = 190, 70, 3
    ls, rs = synth.make_batch(n, w, h, D, 4, seed=77, channels=3)
    lbuf = torch.zeros((n, h + 3, w + 11, 3), dtype=torch.uint8, device="cuda")
    rbuf = torch.zeros((n, h + 1, w + 5, 3), dtype=torch.uint8, device="cuda")
    lv, rv = lbuf[:, :h, :w], rbuf[:, :h, :w]
    lv.copy_(dev(torch, ls)); rv.copy_(dev(torch, rs))
    eng = make_engine(w, h, D, P, 4, radius=2, iters=2, inflight=4, plan="band_up")
    for k in BAND_ROWS:
        eng.set_band_rows(k)
        assert eng.describe_plan(n)["plan"] == "band_up"
        obuf = torch.full((n, h + 2, w + 6), 12345, dtype=torch.int16, device="cuda")
        eng.compute_disparity(lv, rv, out=obuf[:, :h, :w])
        got = obuf.cpu().numpy()
        for f in range(n):
            assert (got[f, :h, :w] == O.disparity_module(ls[f], rs[f], D, P, 4, radius=2, iterations=2)).all(), f"K={k}, frame {f}"
        assert (got[:, h:, :] == 12345).all() and (got[:, :, w:] == 12345).all(), "wrote outside the image"
    eng.close()


@pytest.mark.parametrize("Dx,Px", [(128, 4), (64, 8), (256, 8)])
def test_band_up_is_for_d128_with_8_paths(torch_cuda, Dx, Px):
    """The banded WTA exists for D = 128 with 8 paths: any other engine answers SLABS when the plan is asked for, and computes the oracle's bits."""
    torch = torch_cuda
    w, h, n = 200, 40, 4
    ls, rs = synth.make_batch(n, w, h, Dx, 4, seed=9)
    eng = make_engine(w, h, Dx, Px, 4, radius=2, iters=1, inflight=n, plan="band_up")
    assert eng.describe_plan(n) == {"frames_per_launch": n, "plan": "slabs", "slabs_written": Px}
    got = eng.compute_disparity(dev(torch, ls), dev(torch, rs)).cpu().numpy()
    eng.close()
    assert (got[0] == O.disparity_module(ls[0], rs[0], Dx, Px, 4, radius=2, iterations=1)).all()


def test_describe_plan_and_auto(torch_cuda):
    """The forced plan, what AUTO picks at D = 128, and the AUTO answers the other tests pin."""
    w, h = 1242, 375
    eng = make_engine(w, h, D, P, 4, inflight=2)
    eng.set_plan("band_up")
    assert eng.describe_plan(16) == {"frames_per_launch": 16, "plan": "band_up", "slabs_written": 7}
    eng.set_plan("auto")
    assert eng.describe_plan(16) == {"frames_per_launch": 16, "plan": "band_up", "slabs_written": 7}
    for n in (4, 6, 8, 12, 40):   # every measured launch size; 40 frames run as launches of 16
        assert eng.describe_plan(n)["plan"] == "band_up", n
    for n in (1, 2, 3):
        assert eng.describe_plan(n) == {"frames_per_launch": n, "plan": "slabs", "slabs_written": 8}
    eng.set_spec_variants(s5_top2=True)   # the S5 variant lives in the two-kernel WTA
    for plan in ("auto", "band_up"):
        eng.set_plan(plan)
        assert eng.describe_plan(16)["plan"] == "slabs"
    eng.set_spec_variants()
    eng.set_plan("band_up", 8)   # a forced plan's minimum launch size
    assert eng.describe_plan(4)["plan"] == "slabs" and eng.describe_plan(8)["plan"] == "band_up"
    eng.close()
    for (Dx, Px, n, want) in [(64, 4, 16, "slabs"), (64, 8, 16, "slabs"), (128, 4, 16, "slabs"), (256, 4, 16, "fused_up"), (256, 4, 2, "slabs"), (256, 8, 16, "fused_up")]:
        eng = make_engine(w, h, Dx, Px, 4, inflight=2)
        assert eng.describe_plan(n)["plan"] == want, (Dx, Px, n)
        eng.close()
    eng = make_engine(1920, 1080, 256, 8, 4, inflight=2)
    assert eng.describe_plan(4)["plan"] == "fused_up"
    eng.close()


def test_band_up_across_slot_groups_and_placement_tuning(torch_cuda):
    """One call of max_inflight frames in launches of 12: the slab workspace is groups of 16 + 8 slots, so the second launch takes its slabs
    from two groups (SlabTable); and every slot gives the same bits before and after cart_engine_tune_placement, which times the plan's own
    launches."""
    torch = torch_cuda
    w, h, n = 1242, 375, 24
    ls, rs = synth.make_batch(n, w, h, D, 4, scene="stripes")
    L, R = dev(torch, ls), dev(torch, rs)
    eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=n, plan="slabs")
    eng.set_chunk_frames(12)
    ref = run_maps(eng, L, R, n)
    eng.set_plan("band_up")
    assert eng.describe_plan(n) == {"frames_per_launch": 12, "plan": "band_up", "slabs_written": 7}
    assert_same(run_maps(eng, L, R, n), ref, "before tuning")
    first, kept = eng.tune_placement(12, 3, max_extra_bytes=None)
    assert first > 0 and 0 < kept <= first
    assert_same(run_maps(eng, L, R, n), ref, "after tuning")
    eng.set_plan("slabs")
    assert_same(run_maps(eng, L, R, n), ref, "slabs after tuning")
    eng.close()
    assert (ref[0][5] == O.disparity_module(ls[5], rs[5], D, P, 4, radius=2, iterations=1)).all()
    assert any((ref[0][0] != ref[0][k]).any() for k in range(1, n))


@pytest.mark.parametrize("order", ["slabs_first", "band_first"])
def test_stale_rows_in_the_up_slab(torch_cuda, order):
    """The checkpoint rows live in place in the "up" slab, between whatever an earlier launch left there: full rows of a SLABS run on other
    images, or checkpoint rows of a band_up run with another K on other images.  Neither may show in the result."""
    torch = torch_cuda
    w, h, n = 330, 75, 2
    la, ra = synth.make_batch(n, w, h, D, 4, seed=1)
    lb, rb = synth.make_batch(n, w, h, D, 4, seed=2, scene="stripes")
    A, B = (dev(torch, la), dev(torch, ra)), (dev(torch, lb), dev(torch, rb))
    ref_eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=n, plan="slabs")
    ref_a, ref_b = run_maps(ref_eng, *A, n), run_maps(ref_eng, *B, n)
    ref_eng.close()
    assert (ref_a[0] != ref_b[0]).any()
    assert (ref_b[0][0] == O.disparity_module(lb[0], rb[0], D, P, 4, radius=2, iterations=1)).all()
    eng = make_engine(w, h, D, P, 4, radius=2, iters=1, inflight=n)
    if order == "slabs_first":
        eng.set_plan("slabs")
        assert_same(run_maps(eng, *A, n), ref_a, "slabs on A")
        for k in BAND_ROWS:   # over a SLABS run's full rows, then over the previous K's checkpoints
            eng.set_plan("band_up"); eng.set_band_rows(k)
            assert_same(run_maps(eng, *B, n), ref_b, f"band_up K={k} on B after A")
            eng.set_plan("slabs")
            assert_same(run_maps(eng, *A, n), ref_a, f"slabs on A after band_up K={k}")
    else:
        eng.set_plan("band_up")
        for k, (imgs, ref) in zip((16, 4, 8, 16), ((A, ref_a), (B, ref_b), (A, ref_a), (B, ref_b))):   # a fresh workspace first
            eng.set_band_rows(k)
            assert_same(run_maps(eng, *imgs, n), ref, f"band_up K={k}")
        eng.set_plan("slabs")
        assert_same(run_maps(eng, *B, n), ref_b, "slabs on B after band_up")
        eng.set_plan("band_up"); eng.set_band_rows(8)
        assert_same(run_maps(eng, *A, n), ref_a, "band_up K=8 on A after slabs on B")
    eng.close()

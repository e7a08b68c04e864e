"""Spec S21, the coarse-to-fine census flow, without a GPU: its numpy restatement (np_flow) against the S15
oracle it is anchored to, the level sizes of the C ABI, and what the pyramid is for -- a shift beyond the single-level reach."""
import numpy as np
import pytest

import np_flow as F
import oracle_lib as O
from cartslam import synth
from cartslam.engine import flow_pyramid_levels

# The large-shift case (shared with tests/test_gpu_flow_pyramid.py): (u, v) = (21, -9) at L = 3, R = 4, r = 2 (reach 22).
SHIFT_U, SHIFT_V = 21, -9
SHIFT_PARAMS = dict(levels=3, radius=4, refine_radius=2, block=2, median=1)
SHIFT_FLOOR = 0.962   # share of exact vectors 32 px from every border; the restatement gives 0.98226, the floor is 0.02 below


def shift_pair():
    """cur(p) = prev(p - (u, v)): the flow of every pixel is (u, v)."""
    prev, _, _ = synth.make_pair(256, 128, 64, 4, seed=7)
    return np.roll(prev, (SHIFT_V, SHIFT_U), axis=(0, 1)), prev


def exact_share(flow):
    inner = flow[32:-32, 32:-32]
    return float(((inner[..., 0] == 32 * SHIFT_U) & (inner[..., 1] == 32 * SHIFT_V)).mean())


@pytest.mark.parametrize("w,h,R,B", [(96, 64, 3, 2), (131, 53, 5, 1)])
def test_single_level_equals_the_s15_oracle(w, h, R, B):
    cur, _, _ = synth.make_pair(w, h, 64, 4, seed=11 + w, frame=1)
    prev, _, _ = synth.make_pair(w, h, 64, 4, seed=11 + w, frame=0)
    got = F.pyramid_flow(cur, prev, levels=1, radius=R, refine_radius=2, block=B, median=0)
    exp = O.block_flow(cur, prev, R, B)
    assert (got == exp).all() and (exp != 0).any()


@pytest.mark.parametrize("w,h,levels,used", [(1242, 375, 6, 5), (131, 53, 4, 2), (64, 16, 4, 1), (47, 31, 4, 2), (1242, 375, 1, 1)])
def test_level_sizes_equal_the_c_abi(w, h, levels, used):
    sizes = F.level_sizes(w, h, levels)
    assert flow_pyramid_levels(w, h, levels) == sizes
    assert len(sizes) == used and sizes[0] == (w, h)
    for (aw, ah), (bw, bh) in zip(sizes, sizes[1:]):
        assert (bw, bh) == ((aw + 1) >> 1, (ah + 1) >> 1) and bw >= 24 and bh >= 16
    assert [im.shape for im in F.pyramid(np.zeros((h, w), np.uint8), levels)] == [(lh, lw) for lw, lh in sizes]


def test_level_sizes_reject_bad_arguments():
    from cartslam.engine import EngineError
    for args in ((0, 10, 2), (10, 10, 0), (10, 10, 7)):
        with pytest.raises(EngineError):
            flow_pyramid_levels(*args)


def test_downsample_rounds_and_clamps():
    img = np.array([[0, 1, 255], [2, 3, 255], [9, 9, 7]], np.uint8)
    assert (F.downsample(img) == np.array([[(0 + 1 + 2 + 3 + 2) >> 2, 255], [9, 7]], np.uint8)).all()


def test_large_shift_needs_the_pyramid():
    cur, prev = shift_pair()
    share = exact_share(F.pyramid_flow(cur, prev, **SHIFT_PARAMS))
    print("pyramid share", share)
    assert share >= SHIFT_FLOOR
    single = exact_share(O.block_flow(cur, prev, 16, 2))   # the widest single-level search there is
    print("single-level share", single)
    assert single < 0.05

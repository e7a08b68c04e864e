"""The "optflow" module's pyramid keys through the frame loop (cart_slam_amd --dump): with "pyramid_levels" > 1 the dumped flow
of every frame equals the restatement of spec S21 (np_flow); without the key it is the single-level S15 flow, as before."""
import os

import numpy as np
import pytest

import np_flow as F
import oracle_lib as O
from test_host import load, make_dataset, run_exe


@pytest.mark.gpu
def test_optflow_pyramid_frame_loop(tmp_path):
    w, h, n = 320, 96, 4
    grays = None
    for name, module, want in (
            ("pyramid", {"type": "optflow", "search_radius": 4, "pyramid_levels": 3}, lambda c, p: F.pyramid_flow(c, p, 3, 4, 2, 2, 1)),
            ("keys", {"type": "optflow", "search_radius": 3, "block_radius": 1, "pyramid_levels": 2, "refine_radius": 1, "median": False},
             lambda c, p: F.pyramid_flow(c, p, 2, 3, 1, 1, 0)),
            ("single", {"type": "optflow", "search_radius": 4}, lambda c, p: O.block_flow(c, p, 4, 2))):
        tmp = str(tmp_path / name)
        os.makedirs(os.path.join(tmp, "dump"))
        src, frames = make_dataset(tmp, n, w, h, channels=3)
        grays = grays or [O.bgr2gray(l) for l, _ in frames]
        r = run_exe(src, [module], tmp, ("--dump", os.path.join(tmp, "dump")))
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(os.path.join(tmp, "dump", "1_optflow.bin"))   # no flow for the first frame
        for f in range(1, n):
            got = load(tmp, f + 1, "optflow", np.int16, (h, w, 2))
            assert (got == want(grays[f], grays[f - 1])).all(), f"{name}: optflow frame {f + 1}"
            assert (got != 0).any()
    for bad, msg in (({"pyramid_levels": 7}, "pyramid_levels must be in [1, 6]"), ({"pyramid_levels": 2, "refine_radius": 5}, "refine_radius must be in [1, 4]")):
        r = run_exe(src, [dict({"type": "optflow"}, **bad)], tmp)
        assert r.returncode != 0 and msg in r.stderr

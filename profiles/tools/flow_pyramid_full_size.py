"""cart_optical_flow_pyramid at 1242x375 (L = 4, R = 4, r = 2, B = 2, median on) against the numpy restatement of spec S21, level by level, on both
paths of the refinement kernel.  Kept out of the test suite: the restatement takes 5 s to 25 s of CPU time at this size."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch
import np_flow as F
from cartslam import Engine, synth
w, h = 1242, 375
cur = synth.make_pair(w, h, 128, 4, seed=9, frame=1)[0]; prev = synth.make_pair(w, h, 128, 4, seed=9, frame=0)[0]
t = time.time(); exp, ec, ep, ef = F.pyramid_flow(cur, prev, 4, 4, 2, 2, 1, want_levels=True); print("restatement s", time.time() - t)
eng = Engine(w, h, num_disparities=0, paths=0, max_inflight=2)
for gather in (False, True):
    eng.set_flow_gather(gather)
    got = eng.optical_flow_pyramid(torch.from_numpy(cur).cuda(), torch.from_numpy(prev).cuda(), 4, 4, 2, 2, True).cpu().numpy()
    for l in range(4):
        print("gather", gather, "level", l, "images", bool((eng.flow_debug_level(l, 0) == ec[l]).all() and (eng.flow_debug_level(l, 1) == ep[l]).all()),
              "flow mismatches", int((eng.flow_debug_level(l, 2) != ef[l]).any(axis=-1).sum()))
    print("gather", gather, "final mismatches", int((got != exp).any(axis=-1).sum()), "nonzero", int((got != 0).any(axis=-1).sum()))

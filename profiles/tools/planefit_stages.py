"""Device time of the superpixel plane stages at 1242x375 / block 12: relaxed superpixels of a synthetic
pair, a piecewise planar xyz image with invalid patches (planefit's loop runs) or without (>= 90 % valid regions: the loop
does not run).  Prints the per-call time of each entry point (torch events, mean of REPS calls after a warm-up); run it
under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
torch.zeros(1, device="cuda")
from cartslam import Engine, PlaneFit, Superpixels, plane_cluster, synth
from test_gpu_planefit import scene
import time

REPS = int(os.environ.get("REPS", 20))
w, h, bs = 1242, 375, 12
eng = Engine(w, h, num_disparities=0, paths=0)
l, _, _ = synth.make_pair(w, h, 64, 4, seed=7, channels=3)
sp = Superpixels(eng, block_size=bs, disparity_weight=0.0)
lab = sp.relax(torch.from_numpy(l).cuda(), None, 8)
mx = sp.max_label
pf = PlaneFit(eng, mx)


def timed(fn):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        out = fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS, out


print(f"{w}x{h} block {bs}: {mx + 1} labels, {REPS} calls each")
for name, holes in (("invalid patches (loop runs)", True), ("no holes (>= 90 % valid regions, loop idle)", False)):
    xyz = torch.from_numpy(scene(w, h, 3, holes=holes)).cuda()
    t_lp, _ = timed(lambda: pf.label_planes(lab, xyz, mx, 0, seed=1, frame_id=1))
    t_fit, (P, A, launches) = timed(lambda: pf.fit(lab, seed=1, frame_id=1))
    t_lpc, (p17, _, _) = timed(lambda: pf.label_planes(lab, xyz, mx, 1, seed=1, frame_id=1))
    t_adj, (off, nb) = timed(lambda: pf.adjacency(lab, mx))
    p17, off, nb = p17.cpu().numpy(), off.cpu().numpy(), nb.cpu().numpy()
    t0 = time.perf_counter()
    for _ in range(REPS):
        cP, cA = plane_cluster(p17, off, nb)
    t_merge = (time.perf_counter() - t0) / REPS * 1e3
    print(f"  {name}: label_planes(planefit) {t_lp:.3f} ms, fit {t_fit:.3f} ms ({launches} launches, {len(P)} planes), "
          f"label_planes(planecluster) {t_lpc:.3f} ms, adjacency {t_adj:.3f} ms, host merge {t_merge:.3f} ms ({len(cP)} planes)")
    print(f"    planefit device total {t_lp + t_fit:.3f} ms, planecluster device total {t_lpc + t_adj:.3f} ms")
pf.close(); sp.close(); eng.close()

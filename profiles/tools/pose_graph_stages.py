"""Device time of the pose-graph optimisation: ms per cart_pose_graph_optimize (default 4 Gauss-Newton steps) at
(nodes, loops) = (64, 1), (256, 8), (1024, 64) on the ring scenario of tests/test_posegraph_spec.py (noisy chained odometry, loop edges
from the truth), with torch events, --rounds alternating rounds of --iters runs per case after a warm-up; median and range over the
rounds.  The kernel has no data-dependent loop and no early exit, so repeated calls on the same graph cost the same as the first; the
first call's result record is printed (cost before and after) so that the timed work is an optimisation that converged.  The yardstick
is what a keyframe already costs: cart_place_query at 5000 x 256, 3.75 ms (profiles/place.txt).  `--trace` runs one short round (for one
`rocprofv3 --kernel-trace --stats -- python pose_graph_stages.py --trace` run of its own, which gives the per-kernel times)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd"), os.path.join(ROOT, "tests")]
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--cases", default="64x1,256x8,1024x64")
ap.add_argument("--iterations", type=int, default=4)
args = ap.parse_args()
YARDSTICK_MS = 3.75

import torch
torch.zeros(1, device="cuda")
from cartslam import Engine, PoseGraph
import test_posegraph_spec as S

eng = Engine(64, 32, num_disparities=0, paths=0)
cases = {}
for spec in args.cases.split(","):
    n, nl = (int(v) for v in spec.split("x"))
    loops = [((7 * k) % (n // 2), n - 1 - (5 * k) % (n // 2 - 1)) for k in range(nl)]
    _, odom, edges = S.ring(n, loops, seed=29)
    pg = PoseGraph(eng, n, max(nl, 1))
    for p in odom:
        pg.add_node(p, S.W_ROT, S.W_TRANS)
    for e in edges:
        pg.add_loop(*e, S.W_ROT, S.W_TRANS)
    first = pg.optimize(args.iterations)[0]
    if first["status"] != 1 or not first["cost_after"] < first["cost_before"]:
        sys.exit(f"{spec}: the optimisation did not converge: {first}")
    print(f"{spec}: first call: cost {first['cost_before']:.6g} -> {first['cost_after']:.6g} in {args.iterations} steps", flush=True)
    pg.optimize(args.iterations, raw=True)
    torch.cuda.synchronize()
    cases[spec] = pg

rounds, iters = (1, 2) if args.trace else (args.rounds, args.iters)
ms = {name: [] for name in cases}
for _ in range(rounds):
    for name, pg in cases.items():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            pg.optimize(args.iterations, raw=True)
        e.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(e) / iters)
for name, v in ms.items():
    t = float(np.median(v))
    print(f"{name} (nodes x loops), {args.iterations} steps: {t:.4f} ms per cart_pose_graph_optimize (min {min(v):.4f}, max {max(v):.4f}; {rounds} rounds of {iters}); "
          f"{t / YARDSTICK_MS:.2f} x the 3.75 ms of cart_place_query at 5000 x 256", flush=True)

"""Device time per call at KITTI size: cart_optical_flow (R = 8, 16) against cart_optical_flow_pyramid (L = 3, 4; R = 4, r = 2;
median on / off; refinement staged per tile or forced to gather).  The configurations alternate inside each of several rounds,
so that drift of the shared machine shows as spread between the rounds, not as a difference between configurations.
--once runs every configuration a few times and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import torch
from cartslam import Engine, synth

w, h = 1242, 375
eng = Engine(w, h, num_disparities=0, paths=0, max_inflight=2)
cur = torch.from_numpy(synth.make_pair(w, h, 128, 4, seed=9, frame=1)[0]).cuda()
prev = torch.from_numpy(synth.make_pair(w, h, 128, 4, seed=9, frame=0)[0]).cuda()


def single(R):
    return lambda: eng.optical_flow(cur, prev, R, 2)


def pyramid(L, median, gather=False):
    def call():
        eng.set_flow_gather(gather)
        eng.optical_flow_pyramid(cur, prev, levels=L, radius=4, refine_radius=2, block=2, median=median)
    return call


CONFIGS = [("optical_flow R=8  B=2 (reach  8)", single(8)), ("optical_flow R=16 B=2 (reach 16)", single(16)),
           ("pyramid L=3 median on  (reach 22)", pyramid(3, True)), ("pyramid L=3 median off (reach 22)", pyramid(3, False)),
           ("pyramid L=4 median on  (reach 46)", pyramid(4, True)), ("pyramid L=4 median off (reach 46)", pyramid(4, False)),
           ("pyramid L=4 median on, gather only", pyramid(4, True, True))]
if "--once" in sys.argv:
    for _, call in CONFIGS:
        for _ in range(5):
            call()
    torch.cuda.synchronize()
    sys.exit(0)
ROUNDS, CALLS = 5, 200
for _, call in CONFIGS:   # warm-up: code objects, the workspaces of the first call
    for _ in range(10):
        call()
torch.cuda.synchronize()
ms = {name: [] for name, _ in CONFIGS}
for _ in range(ROUNDS):
    for name, call in CONFIGS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            call()
        e1.record(); torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / CALLS)
base = sorted(ms[CONFIGS[1][0]])[ROUNDS // 2]
print(f"{w}x{h}, {ROUNDS} rounds of {CALLS} calls, device events; ms per call: median [min .. max], ratio to optical_flow R=16")
for name, _ in CONFIGS:
    v = sorted(ms[name])
    print(f"{name}: {v[ROUNDS // 2]:.3f} [{v[0]:.3f} .. {v[-1]:.3f}]  x{v[ROUNDS // 2] / base:.2f}")

"""Device time of the temporal disparity fusion: ms per cart_fusion_update (splat + fuse, with the source image and the
counts), per call on a frame without a predecessor (the fuse kernel alone) and per call of the two yardsticks on the same frame in the same
session -- cart_motion_segment at radius 0 without the residual record (the same loads and divisions per pixel, no atomics) and
cart_plane_map_update with the window still (atomics) -- with torch events, --rounds alternating rounds of --iters calls per case after a
warm-up.  The frame is synth.road_corridor at 1242x375 seen again after a forward step of 0.5 m, 2 % holes in both disparity images, every
previous pixel at age 3.  Buffers are allocated once, so a figure is the launch sequence alone.  The splat kernel's A/B (CART_FUSION_MERGE,
csrc/engine_internal.h) is a second build of the library: run the tool once per library (CART_ENGINE_LIB names the other one) and compare the
cart_fusion_update lines; --label tags the output.  `--trace` runs only the first round (for one `rocprofv3 --kernel-trace --stats -- python
fusion_stages.py --trace` run of its own, which gives the per-kernel times)."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np
from cartslam import synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--label", default="")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
W, H, N = 1242, 375, 512
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import DisparityFusion, EgoCamera, Engine, PlaneMap, fusion_params, motion_params

eng = Engine(W, H, num_disparities=0, paths=0)
obj = DisparityFusion(eng, W, H)
pm = PlaneMap(eng, CAMERA, N, N)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
rel_host, dc_host, dp_host, fl_host, planes_host, _ = synth.road_corridor_motion(W, H, *CAMERA, step=0.5)
truth, _ = synth.road_corridor(W, H, *CAMERA)
rng = np.random.default_rng(28)
cur_host, prev_host = truth.copy(), truth.copy()
cur_host[rng.random((H, W)) < 0.02] = -32768
prev_host[rng.random((H, W)) < 0.02] = -32768
cur, prev, dc, dp, fl, planes = (torch.from_numpy(a).cuda() for a in (cur_host, prev_host, dc_host, dp_host, fl_host, planes_host))
prev_age = torch.full((H, W), 3, dtype=torch.uint8, device="cuda")
fused = torch.empty((H, W), dtype=torch.int16, device="cuda")
age, source, raw, labels = (torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(4))
counts = torch.zeros(5, dtype=torch.int32, device="cuda")
cam = EgoCamera(*CAMERA)
rel = (C.c_double * 12)(*rel_host)
FP, MP = fusion_params(), motion_params(radius=0)


def update(carry):
    def call():
        if lib.cart_fusion_update(obj._h, C.byref(cam), rel, C.byref(FP), vp(cur), 2 * W, vp(prev) if carry else None, 2 * W, vp(prev_age) if carry else None, W,
                                  None, 0, None, 0, W, H, vp(fused), 2 * W, vp(age), W, vp(source), W, vp(counts), stream) != 0:
            sys.exit("cart_fusion_update: " + lib.cart_last_error(None).decode())
    return call


def segment():
    if lib.cart_motion_segment(eng._h, C.byref(cam), rel, C.byref(MP), vp(dc), 2 * W, vp(dp), 2 * W, vp(fl), 4 * W, W, H, None, 0, vp(raw), W, vp(labels), W,
                               None, 0, None, 0, stream) != 0:
        sys.exit("cart_motion_segment: " + lib.cart_last_error(None).decode())


def vote():
    pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    if lib.cart_plane_map_update(pm._h, C.byref(pm.camera), pose, vp(cur), 2 * W, vp(planes), W, W, H, stream) != 0:
        sys.exit("cart_plane_map_update: " + lib.cart_last_error(None).decode())


tag = f" [{args.label}]" if args.label else ""
cases = {"cart_fusion_update, splat + fuse" + tag: update(True), "cart_fusion_update without a previous frame (fuse alone)" + tag: update(False),
         "cart_motion_segment radius 0, no residual": segment, "cart_plane_map_update, window still": vote}
for name, call in cases.items():
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    if name.startswith("cart_fusion"):
        print(f"{name}: counts (none, measured, agreed, replaced, predicted) = {counts.cpu().tolist()}", flush=True)
rounds = 1 if args.trace else args.rounds
ms = {name: [] for name in cases}
for _ in range(rounds):
    for name, call in cases.items():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            call()
        e.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(e) / args.iters)
for name, v in ms.items():
    print(f"{name}: {np.median(v):.4f} ms per call (min {min(v):.4f}, max {max(v):.4f}; {rounds} rounds of {args.iters})", flush=True)
names = list(cases)
both = np.median(ms[names[2]]) + np.median(ms[names[3]])
print(f"{names[0]}: {np.median(ms[names[0]]) / both:.2f} x the two yardsticks together ({both:.4f} ms)", flush=True)
pm.close()
obj.close()
eng.close()

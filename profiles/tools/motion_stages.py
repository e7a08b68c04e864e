"""Device time of the motion segmentation: ms per cart_motion_segment with and without the residual output at radius 0,
2 and 4, and per call of the two yardsticks on the same frame -- cart_reproject_depth (similar bytes, no fp64 division) and
cart_plane_map_update (five to six fp64 divisions per pixel plus atomics) -- with torch events, --rounds alternating rounds of --iters
calls per case after a warm-up.  The frame is synth.road_corridor_motion at 1242x375.  Buffers are allocated once, so a figure is the
launch sequence alone.  `--trace` runs only the first round (for one `rocprofv3 --kernel-trace --stats -- python motion_stages.py
--trace` run of its own, which gives the per-kernel times)."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np
from cartslam import synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
W, H, N = 1242, 375, 512
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import EgoCamera, Engine, PlaneMap, motion_params

eng = Engine(W, H, num_disparities=0, paths=0)
pm = PlaneMap(eng, CAMERA, N, N)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
rel_host, dc_host, dp_host, fl_host, planes_host, _ = synth.road_corridor_motion(W, H, *CAMERA)
dc, dp, fl, planes = (torch.from_numpy(a).cuda() for a in (dc_host, dp_host, fl_host, planes_host))
res = torch.empty((H, W, 4), dtype=torch.int16, device="cuda")
raw, labels, static = (torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(3))
xyz = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
classes = torch.empty((N, N), dtype=torch.uint8, device="cuda")
fx, fy, cx, cy, b = CAMERA
Q = (C.c_float * 16)(1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 0, fx, 0, 0, -1 / b, 0)
cam = EgoCamera(*CAMERA)
rel = (C.c_double * 12)(*rel_host)
pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def segment(radius, residual):
    p = motion_params(radius=radius)

    def call():
        if lib.cart_motion_segment(eng._h, C.byref(cam), rel, C.byref(p), vp(dc), 2 * W, vp(dp), 2 * W, vp(fl), 4 * W, W, H, vp(res if residual else None),
                                   8 * W if residual else 0, vp(raw), W, vp(labels), W, vp(planes), W, vp(static), W, stream) != 0:
            sys.exit("cart_motion_segment: " + lib.cart_last_error(None).decode())
    return call


def reproject():
    if lib.cart_reproject_depth(eng._h, 1, vp(dc), 2 * W, 0, Q, vp(xyz), xyz.stride(0) * 4, 0, stream) != 0:
        sys.exit("cart_reproject_depth: " + lib.cart_last_error(eng._h).decode())


def update():
    if lib.cart_plane_map_update(pm._h, C.byref(pm.camera), pose, vp(dc), 2 * W, vp(planes), W, W, H, stream) != 0:
        sys.exit("cart_plane_map_update: " + lib.cart_last_error(eng._h).decode())


cases = {f"cart_motion_segment radius {r}, {'with' if residual else 'no'} residual": segment(r, residual) for r in (0, 2, 4) for residual in (True, False)}
cases["cart_reproject_depth of the same frame"] = reproject
cases["cart_plane_map_update of the same frame, window still"] = update
for call in cases.values():
    for _ in range(10):
        call()
torch.cuda.synchronize()
print(f"frame {W}x{H}: raw labels {np.bincount(raw.cpu().numpy().ravel(), minlength=3).tolist()}, filtered (radius 4) "
      f"{np.bincount(labels.cpu().numpy().ravel(), minlength=3).tolist()}", flush=True)
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
for ref in list(cases)[-2:]:
    for name in list(cases)[:-2]:
        print(f"{name}: {np.median(ms[name]) / np.median(ms[ref]):.2f} x {ref.split(' ')[0]} (the whole call, not one kernel: --trace separates the kernels)", flush=True)
pm.close()
eng.close()

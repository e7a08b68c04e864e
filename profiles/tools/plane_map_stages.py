"""Device time of the world-frame plane map: ms per cart_plane_map_update with the window still and with the window
moving by 16 cells on both axes every call, per cart_plane_map_classify, and per cart_reproject_depth of the same frame (the yardstick:
it reads the same disparity image and writes 12 B per pixel without atomics), with torch events, --rounds alternating rounds of
--iters calls per case after a warm-up.  The frame is a synthetic 1242x375 street corridor (ground + two walls, synth.road_corridor)
voted into a 512x512 grid of 0.25 m cells.  Buffers are allocated once, so a figure is the launch sequence alone.  `--trace` runs only
the first round (for one `rocprofv3 --kernel-trace --stats -- python plane_map_stages.py --trace` run of its own, which gives the
per-kernel times)."""
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
from cartslam import Engine, PlaneMap

eng = Engine(W, H, num_disparities=0, paths=0)
pm = PlaneMap(eng, CAMERA, N, N)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
disp_host, planes_host = synth.road_corridor(W, H, *CAMERA)
disp, planes = torch.from_numpy(disp_host).cuda(), torch.from_numpy(planes_host).cuda()
classes = torch.empty((N, N), dtype=torch.uint8, device="cuda")
xyz = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
fx, fy, cx, cy, b = CAMERA
Q = (C.c_float * 16)(1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 0, fx, 0, 0, -1 / b, 0)
moves = [0]


def update(step):
    def call():
        moves[0] += step
        t = 4.0 * (moves[0] % 64)          # 16 cells of 0.25 m per call on both axes, back to the start every 64 calls
        pose = (C.c_double * 12)(1, 0, 0, t, 0, 1, 0, 0, 0, 0, 1, t)
        if lib.cart_plane_map_update(pm._h, C.byref(pm.camera), pose, vp(disp), disp.stride(0) * 2, vp(planes), planes.stride(0), W, H, stream) != 0:
            sys.exit("cart_plane_map_update: " + lib.cart_last_error(eng._h).decode())
    return call


def classify():
    if lib.cart_plane_map_classify(pm._h, 3, 50, vp(classes), N, stream) != 0:
        sys.exit("cart_plane_map_classify: " + lib.cart_last_error(eng._h).decode())


def reproject():
    if lib.cart_reproject_depth(eng._h, 1, vp(disp), disp.stride(0) * 2, 0, Q, vp(xyz), xyz.stride(0) * 4, 0, stream) != 0:
        sys.exit("cart_reproject_depth: " + lib.cart_last_error(eng._h).decode())


cases = {"cart_plane_map_update, window still": update(0), "cart_plane_map_update, window moving 16 cells on both axes": update(1),
         "cart_plane_map_classify 512x512": classify, "cart_reproject_depth of the same frame": reproject}
for call in cases.values():
    for _ in range(10):
        call()
torch.cuda.synchronize()
cells, _ = pm.read()
n_h, n_v = int(cells["horizontal"].sum()), int(cells["vertical"].sum())
print(f"frame {W}x{H}: labels {np.bincount(planes_host.ravel(), minlength=3).tolist()}; map after the warm-up: {n_h} horizontal and {n_v} vertical votes in "
      f"{int(((cells['horizontal'] > 0) | (cells['vertical'] > 0)).sum())} cells", flush=True)
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
ref = np.median(ms["cart_reproject_depth of the same frame"])
for name in list(cases)[:2]:
    print(f"{name}: {np.median(ms[name]) / ref:.2f} x cart_reproject_depth", flush=True)
pm.close()
eng.close()

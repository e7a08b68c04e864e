"""Device time of the moving-object tracks: ms per cart_object_tracker_update on the 1242x375 corridor frame, and per call
of the yardstick, the existing code that makes its input on the same frame -- cart_motion_segment and cart_plane_ccl_table, one after the
other -- with torch events, --rounds alternating rounds of --iters calls per case after a warm-up.  The frame is
synth.road_corridor_motion at 1242x375; its labels, ids and table come from the library itself.  Buffers are allocated once, so a figure
is the launch sequence alone.  `--trace` runs only the first round (for one `rocprofv3 --kernel-trace --stats -- python object_stages.py
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
W, H, ROWS, MAX_OBJECTS, MAX_TRACKS = 1242, 375, 4096, 64, 64
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import OBJECT_DTYPE, EgoCamera, Engine, ObjectTracker, motion_params, object_params

eng = Engine(W, H, num_disparities=0, paths=0)
tracker = ObjectTracker(eng, W, H, MAX_OBJECTS, MAX_TRACKS)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
rel_host, dc_host, dp_host, fl_host, _, _ = synth.road_corridor_motion(W, H, *CAMERA)
dc, dp, fl = (torch.from_numpy(a).cuda() for a in (dc_host, dp_host, fl_host))
raw, labels = (torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(2))
ids = torch.empty((H, W), dtype=torch.int32, device="cuda")
table = torch.empty((ROWS, 7), dtype=torch.int32, device="cuda")
count = torch.empty(1, dtype=torch.int32, device="cuda")
objects = torch.empty(MAX_OBJECTS * 24, dtype=torch.float64, device="cuda")
tracks = torch.empty(MAX_TRACKS * 12, dtype=torch.float64, device="cuda")
counts = torch.empty(8, dtype=torch.int32, device="cuda")
cam = EgoCamera(*CAMERA)
rel = (C.c_double * 12)(*rel_host)
pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
mp, op = motion_params(), object_params()


def segment():
    if lib.cart_motion_segment(eng._h, C.byref(cam), rel, C.byref(mp), vp(dc), 2 * W, vp(dp), 2 * W, vp(fl), 4 * W, W, H, None, 0, vp(raw), W, vp(labels), W, None, 0,
                               None, 0, stream) != 0:
        sys.exit("cart_motion_segment: " + lib.cart_last_error(None).decode())


def components():
    if lib.cart_plane_ccl_table(eng._h, 1, vp(labels), W, 0, vp(ids), 4 * W, 0, vp(table), ROWS, vp(count), stream) != 0:
        sys.exit("cart_plane_ccl_table: " + lib.cart_last_error(eng._h).decode())


def both():
    segment()
    components()


def update():
    if lib.cart_object_tracker_update(tracker._h, C.byref(cam), rel, pose, C.byref(op), vp(ids), 4 * W, vp(table), ROWS, vp(count), vp(dc), 2 * W, vp(dp), 2 * W, vp(fl),
                                      4 * W, W, H, vp(objects), vp(tracks), vp(counts), stream) != 0:
        sys.exit("cart_object_tracker_update: " + lib.cart_last_error(None).decode())


cases = {"cart_object_tracker_update": update, "cart_motion_segment": segment, "cart_plane_ccl_table": components,
         "cart_motion_segment + cart_plane_ccl_table": both}
both()
for call in cases.values():
    for _ in range(10):
        call()
torch.cuda.synchronize()
got = objects.cpu().numpy().view(OBJECT_DTYPE)[:int(counts[2])]
print(f"frame {W}x{H}: {int(count[0])} components, counts {counts.cpu().numpy().tolist()}, points per object {got['n_points'].tolist()}, "
      f"flow points {got['n_flow'].tolist()}", flush=True)
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
ref = "cart_motion_segment + cart_plane_ccl_table"
print(f"cart_object_tracker_update: {np.median(ms['cart_object_tracker_update']) / np.median(ms[ref]):.2f} x ({ref}) (the whole call, not one kernel: "
      "--trace separates the kernels)", flush=True)
tracker.close()
eng.close()

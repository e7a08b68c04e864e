"""Device time of the colour companion of the TSDF volume, each call beside the existing call it stands next to on the same
frame: cart_voxel_color_integrate (gray and B, G, R) against cart_voxel_map_integrate with the window still, cart_voxel_color_render against
cart_voxel_map_raycast, cart_voxel_color_vertices against cart_voxel_map_mesh; ms per call with torch events, --rounds alternating rounds of
--iters calls per case after a warm-up, median with range.  The volume is the module's default 256 x 64 x 256 voxels of 0.125 m at the
default parameters, filled by --frames frames of synth.road_corridor at 1242x375 with 2 % holes, 0.25 m apart, every frame with an image of
random bytes.  Buffers are allocated once, so a figure is the launch sequence alone.  Also printed: the voxels a frame colours, the pixels
of the model image with a colour and the vertices coloured.  With --no-counts the integrates and the render run without their counters
(no atomics, no tickets)."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np
from cartslam import synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=6)
ap.add_argument("--no-counts", action="store_true")
args = ap.parse_args()
W, H = 1242, 375
NX, NY, NZ = 256, 64, 256
CAP = 1 << 20
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import EgoCamera, Engine, VoxelColor, VoxelMap

eng = Engine(W, H, num_disparities=0, paths=0)
vm = VoxelMap(eng, NX, NY, NZ)
vc = VoxelColor(eng, vm)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
truth, _ = synth.road_corridor(W, H, *CAMERA)
rng = np.random.default_rng(37)
cam = EgoCamera(*CAMERA)
vcounts = torch.zeros(2, dtype=torch.int32, device="cuda")
rcounts = torch.zeros(3, dtype=torch.int32, device="cuda")
mcounts = torch.zeros(4, dtype=torch.int32, device="cuda")
ccounts = torch.zeros(2, dtype=torch.int32, device="cuda")
pcounts = torch.zeros(1, dtype=torch.int32, device="cuda")
model, weight = (torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(2))
status = torch.empty((H, W), dtype=torch.uint8, device="cuda")
vertices = torch.empty((CAP, 6), dtype=torch.float32, device="cuda")
quads = torch.empty((CAP, 4), dtype=torch.int32, device="cuda")
colors = torch.empty((CAP, 4), dtype=torch.uint8, device="cuda")
gray = torch.from_numpy(rng.integers(0, 256, (H, W), dtype=np.uint8)).cuda()
bgr = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
image_model = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
alpha = torch.empty((H, W), dtype=torch.uint8, device="cuda")
origin = (C.c_int64 * 3)()
last = [0.0]
cur = None
counted = not args.no_counts


def check(rc, what):
    if rc != 0:
        sys.exit(what + ": " + lib.cart_last_error(None).decode())


def pose_now():
    return (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, last[0])


def integrate():
    check(lib.cart_voxel_map_integrate(vm._h, C.byref(cam), pose_now(), vp(cur), 2 * W, W, H, None, 0, vp(vcounts) if counted else None, stream), "cart_voxel_map_integrate")


def color_gray():
    check(lib.cart_voxel_color_integrate(vc._h, vm._h, C.byref(cam), pose_now(), vp(cur), 2 * W, vp(gray), W, 1, W, H, None, 0, vp(ccounts) if counted else None, stream),
          "cart_voxel_color_integrate")


def color_bgr():
    check(lib.cart_voxel_color_integrate(vc._h, vm._h, C.byref(cam), pose_now(), vp(cur), 2 * W, vp(bgr), 3 * W, 3, W, H, None, 0, vp(ccounts) if counted else None, stream),
          "cart_voxel_color_integrate")


def raycast():
    check(lib.cart_voxel_map_raycast(vm._h, C.byref(cam), pose_now(), W, H, vp(model), 2 * W, vp(weight), 2 * W, vp(status), W, vp(rcounts), stream), "cart_voxel_map_raycast")


def render():
    check(lib.cart_voxel_color_render(vc._h, C.byref(cam), pose_now(), vp(model), 2 * W, W, H, vp(image_model), 3 * W, vp(alpha), W, vp(pcounts) if counted else None, stream),
          "cart_voxel_color_render")


def mesh():
    check(lib.cart_voxel_map_mesh(vm._h, 0, vp(vertices), CAP, vp(quads), CAP, vp(mcounts), origin, stream), "cart_voxel_map_mesh")


def colorize():
    check(lib.cart_voxel_color_vertices(vc._h, vp(vertices), C.c_void_p(mcounts.data_ptr() + 8), CAP, origin, vp(colors), stream), "cart_voxel_color_vertices")


for k in range(args.frames):
    frame = truth.copy()
    frame[rng.random((H, W)) < 0.02] = -32768
    cur = torch.from_numpy(frame).cuda()
    last[0] = 0.25 * k
    integrate()
    (color_bgr if k % 2 else color_gray)()
raycast()
mesh()
render()
colorize()
torch.cuda.synchronize()
print(f"after {args.frames} frames: " + (f"a frame colours {ccounts.cpu().tolist()[0]} voxels (cart_voxel_map_integrate updates {vcounts.cpu().tolist()[0]}); " if counted else "") +
      f"{int((alpha > 0).sum())} of {int((status == 1).sum())} HIT pixels have a colour; {mcounts.cpu().tolist()[2]} vertices, "
      f"{int((colors[:int(mcounts.cpu()[2]), 3] > 0).sum())} with a colour" + ("" if counted else "; timed without counters"), flush=True)

cases = {"cart_voxel_map_integrate, window still": integrate, "cart_voxel_color_integrate, gray": color_gray, "cart_voxel_color_integrate, BGR": color_bgr,
         "cart_voxel_map_raycast": raycast, "cart_voxel_color_render": render, "cart_voxel_map_mesh": mesh, "cart_voxel_color_vertices": colorize}
for call in cases.values():
    for _ in range(5):
        call()
torch.cuda.synchronize()
ms = {name: [] for name in cases}
for _ in range(args.rounds):
    for name, call in cases.items():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            call()
        e.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(e) / args.iters)
for name, v in ms.items():
    print(f"{name}: {np.median(v):.4f} ms per call (min {min(v):.4f}, max {max(v):.4f}; {args.rounds} rounds of {args.iters})", flush=True)
for new, yardstick in (("cart_voxel_color_integrate, gray", "cart_voxel_map_integrate, window still"), ("cart_voxel_color_integrate, BGR", "cart_voxel_map_integrate, window still"),
                       ("cart_voxel_color_render", "cart_voxel_map_raycast"), ("cart_voxel_color_vertices", "cart_voxel_map_mesh")):
    print(f"{new}: {np.median(ms[new]) / np.median(ms[yardstick]):.2f} x {yardstick}", flush=True)
vc.close()
vm.close()
eng.close()

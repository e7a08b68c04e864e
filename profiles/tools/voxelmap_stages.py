"""Device time of the rolling TSDF voxel map: ms per cart_voxel_map_integrate with the window still, per
cart_voxel_map_integrate with the window moving 8 voxels along z on every call (one clear launch of an 8-voxel slab, then the integrate),
per cart_voxel_map_raycast (with the weight and status images and the counts), and per call of the two yardsticks on the same frame in the
same session -- cart_fusion_update (splat + fuse) and cart_plane_map_update with the window still -- with torch events, --rounds
alternating rounds of --iters calls per case after a warm-up.  The frame is synth.road_corridor at 1242x375 with 2 % holes, the volume the
module's default 256 x 64 x 256 voxels of 0.125 m at the default parameters.  Buffers are allocated once, so a figure is the launch
sequence alone.  Also printed: the voxels updated per call and the bytes per second the integrate achieves on them (one 4-byte read and one
4-byte write per updated voxel, and one 2-byte image read per voxel that reaches gate 3, counted as updated voxels too: a lower bound).
`--trace` runs only the first round (for one `rocprofv3 --kernel-trace --stats -- python voxelmap_stages.py --trace` run of its own, which
gives the per-kernel times)."""
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
NX, NY, NZ = 256, 64, 256
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import DisparityFusion, EgoCamera, Engine, PlaneMap, VoxelMap, fusion_params

eng = Engine(W, H, num_disparities=0, paths=0)
vm = VoxelMap(eng, NX, NY, NZ)
fu = DisparityFusion(eng, W, H)
pm = PlaneMap(eng, CAMERA, N, N)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
truth, planes_host = synth.road_corridor(W, H, *CAMERA)
rng = np.random.default_rng(33)
cur_host, prev_host = truth.copy(), truth.copy()
cur_host[rng.random((H, W)) < 0.02] = -32768
prev_host[rng.random((H, W)) < 0.02] = -32768
cur, prev, planes = (torch.from_numpy(a).cuda() for a in (cur_host, prev_host, planes_host))
prev_age = torch.full((H, W), 3, dtype=torch.uint8, device="cuda")
fused, model, weight = (torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(3))
age, source, status = (torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(3))
counts = torch.zeros(5, dtype=torch.int32, device="cuda")
vcounts = torch.zeros(2, dtype=torch.int32, device="cuda")
rcounts = torch.zeros(3, dtype=torch.int32, device="cuda")
cam = EgoCamera(*CAMERA)
FP = fusion_params()
identity = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
rel = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.5)
forward = [0.0]


def integrate(step):
    def call():
        forward[0] += step
        pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, forward[0])
        if lib.cart_voxel_map_integrate(vm._h, C.byref(cam), pose, vp(cur), 2 * W, W, H, None, 0, vp(vcounts), stream) != 0:
            sys.exit("cart_voxel_map_integrate: " + lib.cart_last_error(None).decode())
    return call


def raycast():
    pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, forward[0])
    if lib.cart_voxel_map_raycast(vm._h, C.byref(cam), pose, W, H, vp(model), 2 * W, vp(weight), 2 * W, vp(status), W, vp(rcounts), stream) != 0:
        sys.exit("cart_voxel_map_raycast: " + lib.cart_last_error(None).decode())


def fuse():
    if lib.cart_fusion_update(fu._h, C.byref(cam), rel, C.byref(FP), vp(cur), 2 * W, vp(prev), 2 * W, vp(prev_age), W, None, 0, None, 0, W, H, vp(fused), 2 * W,
                              vp(age), W, vp(source), W, vp(counts), stream) != 0:
        sys.exit("cart_fusion_update: " + lib.cart_last_error(None).decode())


def vote():
    if lib.cart_plane_map_update(pm._h, C.byref(pm.camera), identity, vp(cur), 2 * W, vp(planes), W, W, H, stream) != 0:
        sys.exit("cart_plane_map_update: " + lib.cart_last_error(None).decode())


tag = f" [{args.label}]" if args.label else ""
cases = {"cart_voxel_map_integrate, window still" + tag: integrate(0.0), "cart_voxel_map_integrate, window moving 8 voxels per call" + tag: integrate(1.0),
         "cart_voxel_map_raycast" + tag: raycast, "cart_fusion_update, splat + fuse": fuse, "cart_plane_map_update, window still": vote}
updated = {}
for name, call in cases.items():
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    if name.startswith("cart_voxel_map_integrate"):
        updated[name] = vcounts.cpu().tolist()
        print(f"{name}: counts (voxels updated, of them with f < 1) = {updated[name]}", flush=True)
    if name.startswith("cart_voxel_map_raycast"):
        print(f"{name}: counts (none, hit, inside) = {rcounts.cpu().tolist()} of {W * H} rays", flush=True)
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
both = np.median(ms[names[3]]) + np.median(ms[names[4]])
for name in names[:3]:
    print(f"{name}: {np.median(ms[name]) / both:.2f} x the two yardsticks together ({both:.4f} ms)", flush=True)
for name, (n, _) in updated.items():
    sec = np.median(ms[name]) * 1e-3
    print(f"{name}: {n} voxels updated per call, {n / sec / 1e9:.2f} G voxels/s, at least {10 * n / sec / 1e9:.1f} GB/s on the volume and the image "
          f"({NX * NY * NZ / sec / 1e9:.1f} G voxels/s visited)", flush=True)
pm.close()
fu.close()
vm.close()
eng.close()

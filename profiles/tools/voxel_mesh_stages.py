"""Device time of the surface mesh extraction from the TSDF volume: ms per cart_voxel_map_mesh and, in the same session on
the same volume, per cart_voxel_map_raycast of one 1242x375 frame, per cart_voxel_map_integrate with the window still, and per
Engine.copy_narrow of as many bytes as the mesh call moves (the volume read once, the workspace written and read as the passes do, the
outputs written), with torch events, --rounds alternating rounds of --iters calls per case after a warm-up.  The volume is the module's
default 256 x 64 x 256 voxels of 0.125 m at the default parameters, filled by --frames frames of synth.road_corridor at 1242x375 with 2 %
holes, 0.25 m apart.  Buffers are allocated once, so a figure is the launch sequence alone.  Also printed: the vertices and quads found.
`--trace` runs only the first round of the mesh call (for one `rocprofv3 --kernel-trace --stats -- python voxel_mesh_stages.py --trace` run
of its own, which gives the per-kernel times)."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np
from cartslam import synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=6)
ap.add_argument("--label", default="")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
W, H = 1242, 375
NX, NY, NZ = 256, 64, 256
CAP = 1 << 20
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import EgoCamera, Engine, VoxelMap

eng = Engine(W, H, num_disparities=0, paths=0)
vm = VoxelMap(eng, NX, NY, NZ)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
truth, _ = synth.road_corridor(W, H, *CAMERA)
rng = np.random.default_rng(33)
cam = EgoCamera(*CAMERA)
vcounts = torch.zeros(2, dtype=torch.int32, device="cuda")
rcounts = torch.zeros(3, dtype=torch.int32, device="cuda")
mcounts = torch.zeros(4, dtype=torch.int32, device="cuda")
model, weight = (torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(2))
status = torch.empty((H, W), dtype=torch.uint8, device="cuda")
vertices = torch.empty((CAP, 6), dtype=torch.float32, device="cuda")
quads = torch.empty((CAP, 4), dtype=torch.int32, device="cuda")
last = [0.0]
cur = None
for k in range(args.frames):
    frame = truth.copy()
    frame[rng.random((H, W)) < 0.02] = -32768
    cur = torch.from_numpy(frame).cuda()
    last[0] = 0.25 * k
    pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, last[0])
    if lib.cart_voxel_map_integrate(vm._h, C.byref(cam), pose, vp(cur), 2 * W, W, H, None, 0, vp(vcounts), stream) != 0:
        sys.exit("cart_voxel_map_integrate: " + lib.cart_last_error(None).decode())
torch.cuda.synchronize()


def pose_now():
    return (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, last[0])


def mesh():
    if lib.cart_voxel_map_mesh(vm._h, 0, vp(vertices), CAP, vp(quads), CAP, vp(mcounts), None, stream) != 0:
        sys.exit("cart_voxel_map_mesh: " + lib.cart_last_error(None).decode())


def raycast():
    if lib.cart_voxel_map_raycast(vm._h, C.byref(cam), pose_now(), W, H, vp(model), 2 * W, vp(weight), 2 * W, vp(status), W, vp(rcounts), stream) != 0:
        sys.exit("cart_voxel_map_raycast: " + lib.cart_last_error(None).decode())


def integrate():
    if lib.cart_voxel_map_integrate(vm._h, C.byref(cam), pose_now(), vp(cur), 2 * W, W, H, None, 0, vp(vcounts), stream) != 0:
        sys.exit("cart_voxel_map_integrate: " + lib.cart_last_error(None).decode())


mesh()
torch.cuda.synchronize()
found = mcounts.cpu().tolist()
print(f"cart_voxel_map_mesh: counts (vertices found, quads found, vertices written, quads written) = {found} after {args.frames} frames", flush=True)
voxels = NX * NY * NZ
# the call's own bytes: the volume read once by mesh_classify (the second read by mesh_vertices touches active cells only); the cell words
# written once and read by mesh_count, mesh_vertices and mesh_quads; the outputs
moved = 4 * voxels + 4 * 4 * voxels + 24 * found[2] + 16 * found[3]
src = torch.empty(moved // 4, dtype=torch.int32, device="cuda")
dst = torch.empty_like(src)


def copy():
    eng.copy_narrow(dst, src)


tag = f" [{args.label}]" if args.label else ""
cases = {"cart_voxel_map_mesh" + tag: mesh}
if not args.trace:
    cases.update({"cart_voxel_map_raycast": raycast, "cart_voxel_map_integrate, window still": integrate, f"copy_narrow of {moved} bytes": copy})
for call in cases.values():
    for _ in range(5):
        call()
torch.cuda.synchronize()
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
if not args.trace:
    names = list(cases)
    m = np.median(ms[names[0]])
    for name in names[1:]:
        print(f"{names[0]}: {m / np.median(ms[name]):.2f} x {name}", flush=True)
    print(f"copy_narrow: {2 * moved / (np.median(ms[names[3]]) * 1e-3) / 1e9:.1f} GB/s read + written; the mesh call moves its {moved} bytes at "
          f"{moved / (m * 1e-3) / 1e9:.1f} GB/s", flush=True)
vm.close()
eng.close()

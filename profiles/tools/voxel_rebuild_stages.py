"""Device time of the rebuild of the TSDF volume from stored keyframes: ms per cart_voxel_map_rebuild of N = 16, 64 and 256
stored frames, against existing code on the same inputs in the same session -- cart_voxel_map_clear plus N calls of cart_voxel_map_integrate,
and cart_plane_map_rebuild of the same N entries (the sibling rebuild, S30) -- with torch events, --rounds alternating rounds after a
warm-up, median with range.  The frames are synth.road_corridor at 1242x375 with 2 % fresh holes each, the volume the module's default
256 x 64 x 256 voxels of 0.125 m at the default parameters.  Two paths:
  still    N poses over half a metre forward, so that every pose's own window is the rebuild's: the integrate loop computes the same volume
           (the equivalence clause of S35; the tool checks the counts of the two against each other) -- the like-for-like comparison;
  forward  N poses 0.25 m apart (64 m at N = 256) with the window at the last: what a rebuild after a loop meets; most keyframes do not
           see most of the window.  The integrate loop moves its window with every pose there and computes another volume: its time is
           printed as what the module would otherwise spend, not as an equal.
`--label` tags the rebuild's lines (the A/B builds of voxel_rebuild_kernels.hip: CART_ENGINE_LIB names the library); `--only-rebuild` leaves
the yardsticks out (for those builds); `--trace` runs one round only (for one `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np
from cartslam import synth

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--label", default="")
ap.add_argument("--only-rebuild", action="store_true")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
W, H, CELLS = 1242, 375, 512
NX, NY, NZ = 256, 64, 256
SIZES = (16, 64, 256)
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import EgoCamera, Engine, PlaneMap, PlaneStore, VoxelMap

eng = Engine(W, H, num_disparities=0, paths=0)
vm, loop_vm = VoxelMap(eng, NX, NY, NZ), VoxelMap(eng, NX, NY, NZ)
pm = PlaneMap(eng, CAMERA, CELLS, CELLS)
store = PlaneStore(eng, W, H, max(SIZES))
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
truth, planes_host = synth.road_corridor(W, H, *CAMERA)
rng = np.random.default_rng(35)
planes = torch.from_numpy(planes_host).cuda()
frames = []
for k in range(max(SIZES)):
    d = truth.copy()
    d[rng.random((H, W)) < 0.02] = -32768
    frames.append(torch.from_numpy(d).cuda())
    store.insert(k, frames[-1], planes, raw=True)
cam = EgoCamera(*CAMERA)
counts = torch.zeros(2, dtype=torch.int64, device="cuda")
vcounts = torch.zeros(2, dtype=torch.int32, device="cuda")
used = C.c_int(0)


def path(n, kind):
    step = 0.5 / n if kind == "still" else 0.25
    return [[1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, step * k] for k in range(n)]


def packed(poses):
    flat = [v for p in poses for v in p]
    return (C.c_uint64 * len(poses))(*range(len(poses))), (C.c_double * len(flat))(*flat), (C.c_double * 12)(*poses[-1])


def rebuild(n, kind):
    ids, flat, window = packed(path(n, kind))

    def call():
        if lib.cart_voxel_map_rebuild(vm._h, store._h, C.byref(cam), ids, flat, n, window, 0, C.byref(used), vp(counts), stream) != 0:
            sys.exit("cart_voxel_map_rebuild: " + lib.cart_last_error(None).decode())
    return call


def integrate_loop(n, kind):
    poses = [(C.c_double * 12)(*p) for p in path(n, kind)]

    def call():
        lib.cart_voxel_map_clear(loop_vm._h)
        for k in range(n):
            if lib.cart_voxel_map_integrate(loop_vm._h, C.byref(cam), poses[k], vp(frames[k]), 2 * W, W, H, None, 0, vp(vcounts), stream) != 0:
                sys.exit("cart_voxel_map_integrate: " + lib.cart_last_error(None).decode())
    return call


def plane_rebuild(n, kind):
    ids, flat, window = packed(path(n, kind))

    def call():
        if lib.cart_plane_map_rebuild(pm._h, store._h, C.byref(pm.camera), ids, flat, n, window, C.byref(used), stream) != 0:
            sys.exit("cart_plane_map_rebuild: " + lib.cart_last_error(None).decode())
    return call


tag = f" [{args.label}]" if args.label else ""
cases = {}
for n in SIZES:
    for kind in ("still", "forward"):
        cases[f"cart_voxel_map_rebuild, N = {n}, {kind}{tag}"] = (rebuild(n, kind), max(2, 256 // n))
        if not args.only_rebuild:
            cases[f"clear + {n} x cart_voxel_map_integrate, {kind}"] = (integrate_loop(n, kind), max(1, 64 // n))
    if not args.only_rebuild:
        cases[f"cart_plane_map_rebuild, N = {n}, forward"] = (plane_rebuild(n, "forward"), max(2, 256 // n))
for name, (call, _) in cases.items():   # the warm-up, and what each case computes
    call()
    call()
    torch.cuda.synchronize()
    if name.startswith("cart_voxel_map_rebuild"):
        print(f"{name}: used {used.value}, counts (voxel updates, of them with f < 1) = {counts.cpu().tolist()}", flush=True)
if not args.only_rebuild:   # the equivalence clause on the still path: the two volumes are one
    for n in SIZES:
        rebuild(n, "still")()
        integrate_loop(n, "still")()
        a, b = vm.read(), loop_vm.read()
        print(f"N = {n}, still: rebuild and integrate loop give the same volume: {a[1] == b[1] and a[0].tobytes() == b[0].tobytes()}", flush=True)
rounds = 1 if args.trace else args.rounds
ms = {name: [] for name in cases}
for _ in range(rounds):
    for name, (call, iters) in cases.items():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            call()
        e.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(e) / iters)
for name, v in ms.items():
    print(f"{name}: {np.median(v):.4f} ms per call (min {min(v):.4f}, max {max(v):.4f}; {rounds} rounds of {cases[name][1]})", flush=True)
if not args.only_rebuild:
    for n in SIZES:
        for kind in ("still", "forward"):
            r, l = np.median(ms[f"cart_voxel_map_rebuild, N = {n}, {kind}{tag}"]), np.median(ms[f"clear + {n} x cart_voxel_map_integrate, {kind}"])
            print(f"N = {n}, {kind}: the rebuild takes {r / l:.2f} x the integrate loop ({l / n:.4f} ms per integrate)", flush=True)
for o in (store, pm, loop_vm, vm, eng):
    o.close()

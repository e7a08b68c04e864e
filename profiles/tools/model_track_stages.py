"""Device time of the frame-to-model pose tracking: ms per cart_model_track_refine at stride 1, 2 and 4 (4 iterations: five
evaluations, ten launches) and, beside it on the same frame in the same session, per cart_dense_ego_refine at the same strides (the code it
is modelled on) and per cart_voxel_map_raycast (the other reader of the volume), with torch events, --rounds alternating rounds of --iters
calls per case after a warm-up.  The frame is synth.road_corridor_motion at 1242x375; the volume is the module's default 256 x 64 x 256
voxels of 0.125 m at the default parameters after six integrates of that frame, 0.25 m forward each (the corridor looks the same from
every forward position); the tracked pose starts (1, 0, 2) cm off the sixth.  Buffers are allocated once, so a figure is the launch
sequence alone.  `--trace` runs only the first round (for one `rocprofv3 --kernel-trace --stats -- python model_track_stages.py --trace`
run of its own, which gives the per-kernel times)."""
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
W, H = 1242, 375
NX, NY, NZ = 256, 64, 256
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import DENSE_EGO_RESULT_DTYPE, MODEL_TRACK_RESULT_DTYPE, DenseEgo, EgoCamera, Engine, ModelTrack, VoxelMap, dense_ego_params, model_track_params

eng = Engine(W, H, num_disparities=0, paths=0)
vm = VoxelMap(eng, NX, NY, NZ)
mt = ModelTrack(eng, W, H)
de = DenseEgo(eng, W, H)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
rel_host, dc_host, dp_host, fl_host, _, _ = synth.road_corridor_motion(W, H, *CAMERA)
dc, dp, fl = (torch.from_numpy(a).cuda() for a in (dc_host, dp_host, fl_host))
model, weight = (torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(2))
status = torch.empty((H, W), dtype=torch.uint8, device="cuda")
rcounts = torch.zeros(3, dtype=torch.int32, device="cuda")
result = torch.empty(MODEL_TRACK_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device="cuda")
dense_result = torch.empty(DENSE_EGO_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device="cuda")
cam = EgoCamera(*CAMERA)
for k in range(6):
    pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.25 * k)
    if lib.cart_voxel_map_integrate(vm._h, C.byref(cam), pose, vp(dc), 2 * W, W, H, None, 0, None, stream) != 0:
        sys.exit("cart_voxel_map_integrate: " + lib.cart_last_error(None).decode())
last = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1.25)
pose0 = (C.c_double * 12)(1, 0, 0, 0.01, 0, 1, 0, 0, 0, 0, 1, 1.27)
start = [float(v) for v in rel_host]
start[3] += 0.01
start[11] += 0.02
rel0 = (C.c_double * 12)(*start)


def track(stride):
    p = model_track_params(stride=stride)

    def call():
        if lib.cart_model_track_refine(mt._h, vm._h, C.byref(cam), pose0, C.byref(p), vp(dc), 2 * W, None, 0, W, H, vp(result), stream) != 0:
            sys.exit("cart_model_track_refine: " + lib.cart_last_error(None).decode())
    return call


def dense(stride):
    p = dense_ego_params(stride=stride)

    def call():
        if lib.cart_dense_ego_refine(de._h, C.byref(cam), rel0, C.byref(p), vp(dc), 2 * W, vp(dp), 2 * W, vp(fl), 4 * W, None, 0, W, H, vp(dense_result), stream) != 0:
            sys.exit("cart_dense_ego_refine: " + lib.cart_last_error(None).decode())
    return call


def raycast():
    if lib.cart_voxel_map_raycast(vm._h, C.byref(cam), last, W, H, vp(model), 2 * W, vp(weight), 2 * W, vp(status), W, vp(rcounts), stream) != 0:
        sys.exit("cart_voxel_map_raycast: " + lib.cart_last_error(None).decode())


cases = {}
for s in (1, 2, 4):
    cases[f"cart_model_track_refine stride {s}, 4 iterations"] = track(s)
    cases[f"cart_dense_ego_refine stride {s}, 4 iterations"] = dense(s)
cases["cart_voxel_map_raycast"] = raycast
for name, call in cases.items():
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    if name.startswith("cart_model_track") or name.startswith("cart_dense"):
        r = (result if name.startswith("cart_model") else dense_result).cpu().numpy().view(MODEL_TRACK_RESULT_DTYPE)[0]
        print(f"{name}: status {r['status']}, steps {r['steps']}, candidates {r['n_candidates']}, inliers {r['n_initial']} -> {r['n_inliers']}, "
              f"rms {r['rms_initial']:.4f} -> {r['rms']:.4f}", flush=True)
    else:
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
ray = np.median(ms["cart_voxel_map_raycast"])
for s in (1, 2, 4):
    t, d = np.median(ms[f"cart_model_track_refine stride {s}, 4 iterations"]), np.median(ms[f"cart_dense_ego_refine stride {s}, 4 iterations"])
    print(f"stride {s}: cart_model_track_refine is {t / d:.2f} x cart_dense_ego_refine and {t / ray:.2f} x cart_voxel_map_raycast (whole calls: --trace separates the kernels)", flush=True)
de.close()
mt.close()
vm.close()
eng.close()

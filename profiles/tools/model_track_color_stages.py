"""Device time of the colour-aided frame-to-model tracking: ms per cart_model_track_refine_color at stride 1, 2 and 4
(4 iterations: five evaluations, ten launches) and, beside it on the same frame in the same session, per cart_model_track_refine (the
yardstick) and per cart_model_track_refine_color with photo_weight = 0 (the same kernels without the image and the colour volume), with
torch events, --rounds alternating rounds of --iters calls per case after a warm-up.  The frame is synth.road_corridor_motion at 1242x375
with a smooth paint of the world point behind every pixel; the volume is the module's default 256 x 64 x 256 voxels of 0.125 m and its
colour companion at the default parameters after six integrates of that frame, 0.25 m forward each; the tracked pose starts (1, 0, 2) cm
off the sixth.  Buffers are allocated once, so a figure is the launch sequence alone.  `--trace` runs only the first round (for one
`rocprofv3 --kernel-trace --stats -- python model_track_color_stages.py --trace` run of its own, which gives the per-kernel times)."""
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
from cartslam import MODEL_TRACK_COLOR_RESULT_DTYPE, MODEL_TRACK_RESULT_DTYPE, EgoCamera, Engine, ModelTrack, VoxelColor, VoxelMap, model_track_color_params, model_track_params

eng = Engine(W, H, num_disparities=0, paths=0)
vm = VoxelMap(eng, NX, NY, NZ)
vc = VoxelColor(eng, vm)
mt = ModelTrack(eng, W, H)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
_, dc_host, _, _, _, _ = synth.road_corridor_motion(W, H, *CAMERA)
dc = torch.from_numpy(dc_host).cuda()


def paint(tz):
    """B, G, R levels that vary smoothly with the world point behind every pixel of the frame seen from (0, 0, tz)."""
    fx, fy, cx, cy, base = CAMERA
    ok = dc_host > 0
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Z = np.where(ok, fx * base / (np.where(ok, dc_host, 16) / 16.0), 0.0)
    X, Y, Z = (x - cx) * Z / fx, (y - cy) * Z / fy, Z + tz
    levels = [128 + 100 * np.sin(0.8 * X + 0.5 * Z), 128 + 100 * np.sin(1.1 * Y + 0.7 * Z), 128 + 100 * np.sin(0.9 * Z)]
    return np.where(ok[..., None], np.stack([np.floor(v + 0.5) for v in levels], axis=2), 0).astype(np.uint8)


result = torch.empty(MODEL_TRACK_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device="cuda")
color_result = torch.empty(MODEL_TRACK_COLOR_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device="cuda")
cam = EgoCamera(*CAMERA)
for k in range(6):
    pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.25 * k)
    im = torch.from_numpy(paint(0.25 * k)).cuda()
    if lib.cart_voxel_map_integrate(vm._h, C.byref(cam), pose, vp(dc), 2 * W, W, H, None, 0, None, stream) != 0:
        sys.exit("cart_voxel_map_integrate: " + lib.cart_last_error(None).decode())
    if lib.cart_voxel_color_integrate(vc._h, vm._h, C.byref(cam), pose, vp(dc), 2 * W, vp(im), 3 * W, 3, W, H, None, 0, None, stream) != 0:
        sys.exit("cart_voxel_color_integrate: " + lib.cart_last_error(None).decode())
    torch.cuda.synchronize()
image = torch.from_numpy(paint(1.25)).cuda()
pose0 = (C.c_double * 12)(1, 0, 0, 0.01, 0, 1, 0, 0, 0, 0, 1, 1.27)


def track(stride):
    p = model_track_params(stride=stride)

    def call():
        if lib.cart_model_track_refine(mt._h, vm._h, C.byref(cam), pose0, C.byref(p), vp(dc), 2 * W, None, 0, W, H, vp(result), stream) != 0:
            sys.exit("cart_model_track_refine: " + lib.cart_last_error(None).decode())
    return call


def track_color(stride, weight):
    p, cp = model_track_params(stride=stride), model_track_color_params(photo_weight=weight)

    def call():
        if lib.cart_model_track_refine_color(mt._h, vm._h, vc._h, C.byref(cam), pose0, C.byref(p), C.byref(cp), vp(dc), 2 * W, vp(image), 3 * W, 3, None, 0, W, H,
                                             vp(color_result), stream) != 0:
            sys.exit("cart_model_track_refine_color: " + lib.cart_last_error(None).decode())
    return call


cases = {}
for s in (1, 2, 4):
    cases[f"cart_model_track_refine stride {s}, 4 iterations"] = track(s)
    cases[f"cart_model_track_refine_color stride {s}, 4 iterations"] = track_color(s, 64.0)
    cases[f"cart_model_track_refine_color photo_weight 0 stride {s}, 4 iterations"] = track_color(s, 0.0)
for name, call in cases.items():
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    if "color" in name:
        r = color_result.cpu().numpy().view(MODEL_TRACK_COLOR_RESULT_DTYPE)[0]
        print(f"{name}: status {r['status']}, steps {r['steps']}, candidates {r['n_candidates']}, inliers {r['n_initial']} -> {r['n_inliers']}, photometric "
              f"{r['n_photo_initial']} -> {r['n_photo']}, rms {r['rms_initial']:.4f} -> {r['rms']:.4f}, photometric rms {r['rms_photo_initial']:.4f} -> {r['rms_photo']:.4f}, "
              f"cost {r['cost_initial']:.4f} -> {r['cost']:.4f}, t = ({r['t'][0]:.4f}, {r['t'][1]:.4f}, {r['t'][2]:.4f})", flush=True)
    else:
        r = result.cpu().numpy().view(MODEL_TRACK_RESULT_DTYPE)[0]
        print(f"{name}: status {r['status']}, steps {r['steps']}, candidates {r['n_candidates']}, inliers {r['n_initial']} -> {r['n_inliers']}, "
              f"rms {r['rms_initial']:.4f} -> {r['rms']:.4f}, t = ({r['t'][0]:.4f}, {r['t'][1]:.4f}, {r['t'][2]:.4f})", flush=True)
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
for s in (1, 2, 4):
    t = np.median(ms[f"cart_model_track_refine stride {s}, 4 iterations"])
    c, z = np.median(ms[f"cart_model_track_refine_color stride {s}, 4 iterations"]), np.median(ms[f"cart_model_track_refine_color photo_weight 0 stride {s}, 4 iterations"])
    print(f"stride {s}: cart_model_track_refine_color is {c / t:.2f} x cart_model_track_refine, and {z / t:.2f} x with photo_weight 0 (whole calls: --trace separates the kernels)", flush=True)
mt.close()
vc.close()
vm.close()
eng.close()

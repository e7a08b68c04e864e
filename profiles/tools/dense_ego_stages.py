"""Device time of the dense ego-motion refinement: ms per cart_dense_ego_refine at stride 1, 2 and 4 (4 iterations: five
evaluations, ten launches) and per call of the two yardsticks -- cart_motion_segment at radius 0 without the residual record on the same
frame, whose residual kernel reads the same bytes through the same gates with about a fifth of the arithmetic of one evaluation, and
cart_ego_estimate (256 hypotheses, 4 refinements) on 5000 points under the same camera and a like motion, 30 % of them mismatched (the
set-up of ego_stages.py: the corridor frame has no images to take ORB features from) -- with torch events, --rounds alternating rounds of --iters calls per case after a warm-up.  The frame is synth.road_corridor_motion at 1242x375 with
the true pose moved by (1, 0, 2) cm.  Buffers are allocated once, so a figure is the launch sequence alone.  `--trace` runs only the first
round (for one `rocprofv3 --kernel-trace --stats -- python dense_ego_stages.py --trace` run of its own, which gives the per-kernel times)."""
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
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import DENSE_EGO_RESULT_DTYPE, DenseEgo, EgoCamera, EgoMotion, Engine, dense_ego_params, motion_params
from cartslam.engine import ego_params

eng = Engine(W, H, num_disparities=0, paths=0)
obj = DenseEgo(eng, W, H)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
rel_host, dc_host, dp_host, fl_host, planes_host, _ = synth.road_corridor_motion(W, H, *CAMERA)
dc, dp, fl = (torch.from_numpy(a).cuda() for a in (dc_host, dp_host, fl_host))
raw, labels = (torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(2))
result = torch.empty(DENSE_EGO_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device="cuda")
cam = EgoCamera(*CAMERA)
rel = (C.c_double * 12)(*rel_host)
start = [float(v) for v in rel_host]
start[3] += 0.01
start[11] += 0.02
rel0 = (C.c_double * 12)(*start)


def refine(stride):
    p = dense_ego_params(stride=stride)

    def call():
        if lib.cart_dense_ego_refine(obj._h, C.byref(cam), rel0, C.byref(p), vp(dc), 2 * W, vp(dp), 2 * W, vp(fl), 4 * W, vp(labels), W, W, H, vp(result),
                                     stream) != 0:
            sys.exit("cart_dense_ego_refine: " + lib.cart_last_error(None).decode())
    return call


def segment():
    p = motion_params(radius=0)
    if lib.cart_motion_segment(eng._h, C.byref(cam), rel0, C.byref(p), vp(dc), 2 * W, vp(dp), 2 * W, vp(fl), 4 * W, W, H, None, 0, vp(raw), W, vp(labels), W,
                               None, 0, None, 0, stream) != 0:
        sys.exit("cart_motion_segment: " + lib.cart_last_error(None).decode())


# ---- cart_ego_estimate: 5000 random points under a known motion, every temporal match usable, 30 % pair a point with a wrong one
N = 5000
ego = EgoMotion(eng, CAMERA, N)
EP = ego_params()
rng = np.random.default_rng(1)
fx, fy, cx, cy, b = CAMERA
Z = rng.uniform(4, 60, N)
Pw = np.stack([rng.uniform(-0.8, 0.8, N) * Z, rng.uniform(-0.2, 0.2, N) * Z, Z], 1)
Qw = Pw + [0.0, 0.0, -0.5]


def keypoints(X, right):
    k = np.zeros((N, 7), np.float32)
    k[:, 0] = np.round((fx * X[:, 0] / X[:, 2] + cx - (fx * b / X[:, 2] if right else 0)) * 4) / 4
    k[:, 1] = np.round((fy * X[:, 1] / X[:, 2] + cy) * 4) / 4
    return torch.from_numpy(k).cuda()


ident = np.zeros((N, 4), np.int32)
ident[:, 0] = ident[:, 1] = np.arange(N)
temporal = ident.copy()
wrong = rng.random(N) < 0.3
temporal[wrong, 1] = rng.integers(0, N, int(wrong.sum()))
full = torch.tensor([N], dtype=torch.int32, device="cuda")
st_dev, tm_dev = torch.from_numpy(ident).cuda(), torch.from_numpy(temporal).cuda()
lm = [torch.zeros((N, 4), dtype=torch.float64, device="cuda") for _ in range(2)]
kq = keypoints(Qw, False)
ego_result = torch.zeros(15, dtype=torch.float64, device="cuda")
for X, out in ((Pw, lm[0]), (Qw, lm[1])):
    if lib.cart_ego_triangulate(ego._h, C.byref(ego.camera), C.byref(EP), vp(keypoints(X, False)), vp(keypoints(X, True)), vp(full), vp(st_dev), vp(full), vp(out),
                                stream) != 0:
        sys.exit("cart_ego_triangulate: " + lib.cart_last_error(None).decode())


def estimate():
    if lib.cart_ego_estimate(ego._h, C.byref(ego.camera), C.byref(EP), vp(lm[1]), vp(kq), vp(lm[0]), vp(tm_dev), vp(full), 0, 1, vp(ego_result), None, stream) != 0:
        sys.exit("cart_ego_estimate: " + lib.cart_last_error(None).decode())


segment()   # the mask of the refinement: the labels at rel0
cases = {f"cart_dense_ego_refine stride {s}, 4 iterations": refine(s) for s in (1, 2, 4)}
cases["cart_motion_segment radius 0, no residual, of the same frame"] = segment
cases["cart_ego_estimate, 5000 points, 256 hypotheses, 4 refinements"] = estimate
for name, call in cases.items():
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    if name.startswith("cart_dense"):
        r = result.cpu().numpy().view(DENSE_EGO_RESULT_DTYPE)[0]
        print(f"{name}: status {r['status']}, steps {r['steps']}, candidates {r['n_candidates']}, inliers {r['n_initial']} -> {r['n_inliers']}, "
              f"rms {r['rms_initial']:.4f} -> {r['rms']:.4f}", flush=True)
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
        print(f"{name}: {np.median(ms[name]) / np.median(ms[ref]):.2f} x {ref.split(',')[0].split(' ')[0]} (the whole call, not one kernel: --trace separates the kernels)", flush=True)
ego.close()
obj.close()
eng.close()

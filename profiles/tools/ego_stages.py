"""Device time of the stereo visual odometry stage: ms per cart_ego_triangulate and per cart_ego_estimate with
torch events, --rounds alternating rounds of --iters calls per case after a warm-up, beside cart_orb_detect of the same pair timed
in the same run (the yardstick).  Cases: a 5000-match random scene (5000 correspondences, 256 hypotheses) and the features and
matches the synthetic 1242x375 gray pairs of two frames actually yield under the modules' presets.  Buffers are allocated once, so
a figure is the launch sequence alone.  `--trace` runs only the first round (for one `rocprofv3 --kernel-trace --stats -- python
ego_stages.py --trace` run of its own, which gives the per-kernel times)."""
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
W, H, N = 1242, 375, 5000

import torch
torch.zeros(1, device="cuda")
from cartslam import EgoMotion, Engine, OrbFeatures, OrbMatcher
from cartslam.engine import ego_params, match_params

eng = Engine(W, H, num_disparities=0, paths=0)
orb, matcher = OrbFeatures(eng, W, H, nfeatures=N), OrbMatcher(eng, N)
ego = EgoMotion(eng, (721.5, 721.5, 609.6, 172.9, 0.54), N)   # KITTI-like intrinsics
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
P = ego_params()
STEREO = match_params(use_gate=1, dx_min=0.0, dx_max=256.0, dy_min=-2.0, dy_max=2.0, max_octave_diff=1)
TEMPORAL = match_params(use_gate=1, dx_min=-128.0, dx_max=128.0, dy_min=-128.0, dy_max=128.0, max_octave_diff=1)
result = torch.zeros(15, dtype=torch.float64, device="cuda")
mask = torch.zeros(N, dtype=torch.int32, device="cuda")


def triangulate_call(kl, kr, nl, st, ns, lm):
    def call():
        if lib.cart_ego_triangulate(ego._h, C.byref(ego.camera), C.byref(P), vp(kl), vp(kr), vp(nl), vp(st), vp(ns), vp(lm), stream) != 0:
            sys.exit("cart_ego_triangulate: " + lib.cart_last_error(eng._h).decode())
    return call


def estimate_call(cur, kl, prev, tm, nt, p=P):
    def call():
        if lib.cart_ego_estimate(ego._h, C.byref(ego.camera), C.byref(p), vp(cur), vp(kl), vp(prev), vp(tm), vp(nt), 0, 1, vp(result), vp(mask), stream) != 0:
            sys.exit("cart_ego_estimate: " + lib.cart_last_error(eng._h).decode())
    return call


def detect(l, r):
    """cart_orb_detect of a pair into buffers of its own -> (call, [(kp, desc, count)] left and right)."""
    tl, tr = torch.from_numpy(np.ascontiguousarray(l)).cuda(), torch.from_numpy(np.ascontiguousarray(r)).cuda()
    kp = torch.zeros((2, N, 7), dtype=torch.float32, device="cuda")
    de = torch.zeros((2, N, 32), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    imgs, steps = (C.c_void_p * 2)(tl.data_ptr(), tr.data_ptr()), (C.c_size_t * 2)(tl.stride(0), tr.stride(0))
    kps, des = (C.c_void_p * 2)(kp[0].data_ptr(), kp[1].data_ptr()), (C.c_void_p * 2)(de[0].data_ptr(), de[1].data_ptr())

    def call():
        if lib.cart_orb_detect(orb._h, 2, imgs, steps, 1, W, H, kps, des, None, vp(counts), stream) != 0:
            sys.exit("cart_orb_detect: " + lib.cart_last_error(eng._h).decode())
    call.keep = (tl, tr)
    call()
    return call, [(kp[i], de[i], counts[i:i + 1]) for i in range(2)]


def match(p, q, t):
    out = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    if lib.cart_matcher_match(matcher._h, C.byref(p), vp(q[1]), 32, vp(q[0]), vp(q[2]), vp(t[1]), 32, vp(t[0]), vp(t[2]), vp(out), vp(n), None, stream) != 0:
        sys.exit("cart_matcher_match: " + lib.cart_last_error(eng._h).decode())
    return out, n


cases = {}
# ---- 5000 random points under a known motion: every temporal match is usable, 30 % pair a point with a wrong one
rng = np.random.default_rng(1)
fx, fy, cx, cy, b = 721.5, 721.5, 609.6, 172.9, 0.54
Z = rng.uniform(4, 60, N)
Pw = np.stack([rng.uniform(-0.8, 0.8, N) * Z, rng.uniform(-0.2, 0.2, N) * Z, Z], 1)
Qw = Pw + [0.05, -0.02, -0.9]


def keypoints(X, right):
    k = np.zeros((N, 7), np.float32)
    k[:, 0] = np.round((fx * X[:, 0] / X[:, 2] + cx - (fx * b / X[:, 2] if right else 0)) * 4) / 4
    k[:, 1] = np.round((fy * X[:, 1] / X[:, 2] + cy) * 4) / 4
    return torch.from_numpy(k).cuda()


ident = np.zeros((N, 4), np.int32)
ident[:, 0] = ident[:, 1] = np.arange(N)
temporal = ident.copy()
bad = rng.random(N) < 0.3
temporal[bad, 1] = rng.integers(0, N, int(bad.sum()))
full = torch.tensor([N], dtype=torch.int32, device="cuda")
st_dev, tm_dev = torch.from_numpy(ident).cuda(), torch.from_numpy(temporal).cuda()
lm = [torch.zeros((N, 4), dtype=torch.float64, device="cuda") for _ in range(4)]
kq = keypoints(Qw, False)
tri_prev = triangulate_call(keypoints(Pw, False), keypoints(Pw, True), full, st_dev, full, lm[0])
tri_cur = triangulate_call(kq, keypoints(Qw, True), full, st_dev, full, lm[1])
tri_prev(); tri_cur()
cases["random 5000: cart_ego_triangulate"] = tri_cur
cases["random 5000: cart_ego_estimate, 256 hypotheses, 4 refinements"] = estimate_call(lm[1], kq, lm[0], tm_dev, full)
cases["random 5000: cart_ego_estimate, 256 hypotheses, no refinement"] = estimate_call(lm[1], kq, lm[0], tm_dev, full, ego_params(refine_iterations=0))
cases["random 5000: cart_ego_estimate, 1024 hypotheses, 4 refinements"] = estimate_call(lm[1], kq, lm[0], tm_dev, full, ego_params(hypotheses=1024))
# ---- what the synthetic gray pairs of two frames yield
f0, f1 = (synth.make_pair(W, H, 128, 4, seed=7, frame=f, channels=1)[:2] for f in (0, 1))
det1, (l1, r1) = detect(*f1)
_, (l0, r0) = detect(*f0)
s1, ns1 = match(STEREO, l1, r1)
s0, ns0 = match(STEREO, l0, r0)
tm, nt = match(TEMPORAL, l1, l0)
tri0 = triangulate_call(l0[0], r0[0], l0[2], s0, ns0, lm[2])
tri1 = triangulate_call(l1[0], r1[0], l1[2], s1, ns1, lm[3])
tri0(); tri1()
est = estimate_call(lm[3], l1[0], lm[2], tm, nt)
est()
torch.cuda.synchronize()
res = result.cpu().numpy()
sizes = f"{int(l1[2].item())} keypoints, {int(ns1.item())} stereo and {int(nt.item())} temporal matches, {res[13:14].view(np.int32)[1]} correspondences"
cases["synthetic gray: cart_orb_detect of the pair"] = det1
cases[f"synthetic gray: cart_ego_triangulate ({sizes})"] = tri1
cases["synthetic gray: cart_ego_estimate"] = est

for call in cases.values():
    for _ in range(10):
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
for o in (orb, matcher, ego, eng):
    o.close()

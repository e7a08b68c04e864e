"""Device time of the ORB descriptor matcher: ms per cart_matcher_match with torch events, --rounds alternating
rounds of --iters calls per case after a warm-up, beside cart_orb_detect of the same pair timed in the same run (the
yardstick).  Cases: 5000 x 5000 random descriptors with the gate off and on, and the features the synthetic 1242x375 gray and
BGR pairs actually yield under the module's stereo and temporal presets.  Buffers are allocated once, so a figure is the launch
sequence alone.  `--trace` runs only the first round (for one `rocprofv3 --kernel-trace --stats -- python match_stages.py
--trace` run of its own); `--throughput` runs the C++ frame loop with and without the orb_matches module instead (frames/s as
in orb_throughput.py)."""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np
from cartslam import synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--throughput", action="store_true")
args = ap.parse_args()
W, H, N = 1242, 375, 5000

if args.throughput:
    EXE = os.path.join(ROOT, "cart-slam_amd", "build", "cart_slam_amd")
    tmp = tempfile.mkdtemp(dir="/tmp")
    d = os.path.join(tmp, "ds", "sequences", "00"); os.makedirs(d + "/image_2"); os.makedirs(d + "/image_3")
    NF, NF0 = int(os.environ.get("N", 480)), int(os.environ.get("N0", 96))
    base = [synth.make_pair(W, H, 128, 4, frame=f, channels=3) for f in range(4)]
    for f in range(NF):
        l, r, _ = base[f % 4]
        for cam, img in ((2, l), (3, r)):
            if f >= 4:
                os.link(f"{d}/image_{cam}/{f % 4:06d}.ppm", f"{d}/image_{cam}/{f:06d}.ppm")
                continue
            with open(f"{d}/image_{cam}/{f:06d}.ppm", "wb") as fh:
                fh.write(b"P6\n1242 375\n255\n"); fh.write(img.tobytes())
    json.dump({"type": "kitti", "path": os.path.join(tmp, "ds"), "sequence": 0}, open(tmp + "/src.json", "w"))
    DISP = {"type": "disparity", "smoothing_radius": 3, "smoothing_iterations": 4}
    ORB, MAT = {"type": "orb_features"}, {"type": "orb_matches"}
    for name, mods in (("[disparity, orb_features]", [DISP, ORB]), ("[disparity, orb_features, orb_matches]", [DISP, ORB, MAT]),
                       ("[orb_features]", [ORB]), ("[orb_features, orb_matches]", [ORB, MAT])):
        json.dump(mods, open(tmp + "/mod.json", "w"))
        ts, out = [], ""
        for n in (NF0, NF):
            t0 = time.perf_counter()
            r = subprocess.run([EXE, tmp + "/src.json", tmp + "/mod.json", "--frames", str(n)], capture_output=True, text=True, timeout=300)
            ts.append(time.perf_counter() - t0)
            if r.returncode != 0:
                sys.exit(f"{name}: rc {r.returncode}\n{r.stderr[-2000:]}")
            out = r.stdout.strip()
        print(f"{name}: {(NF - NF0) / (ts[1] - ts[0]):.0f} frames/s  ({out})", flush=True)
    sys.exit(0)

import torch
torch.zeros(1, device="cuda")
from cartslam import Engine, OrbFeatures, OrbMatcher
from cartslam.engine import match_params

eng = Engine(W, H, num_disparities=0, paths=0)
orb, matcher = OrbFeatures(eng, W, H, nfeatures=N), OrbMatcher(eng, N)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
matches = torch.empty((N, 4), dtype=torch.int32, device="cuda")
n_matches = torch.zeros(1, dtype=torch.int32, device="cuda")
STEREO = match_params(use_gate=1, dx_min=0.0, dx_max=256.0, dy_min=-2.0, dy_max=2.0, max_octave_diff=1)
TEMPORAL = match_params(use_gate=1, dx_min=-128.0, dx_max=128.0, dy_min=-128.0, dy_max=128.0, max_octave_diff=1)


def match_call(p, q, t):
    """q / t = (keypoints [N, 7], descriptors [N, 32], count [1]) on the device."""
    def call():
        if lib.cart_matcher_match(matcher._h, C.byref(p), vp(q[1]), 32, vp(q[0]), vp(q[2]), vp(t[1]), 32, vp(t[0]), vp(t[2]), vp(matches), vp(n_matches),
                                  None, stream) != 0:
            sys.exit("cart_matcher_match: " + lib.cart_last_error(eng._h).decode())
    return call


def detect(l, r):
    """cart_orb_detect of a pair into buffers of its own -> (call, [(kp, desc, count)] left and right)."""
    tl, tr = torch.from_numpy(np.ascontiguousarray(l)).cuda(), torch.from_numpy(np.ascontiguousarray(r)).cuda()
    kp = torch.zeros((2, N, 7), dtype=torch.float32, device="cuda")
    de = torch.zeros((2, N, 32), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    ch = 1 if tl.dim() == 2 else 3
    imgs, steps = (C.c_void_p * 2)(tl.data_ptr(), tr.data_ptr()), (C.c_size_t * 2)(tl.stride(0), tr.stride(0))
    kps, des = (C.c_void_p * 2)(kp[0].data_ptr(), kp[1].data_ptr()), (C.c_void_p * 2)(de[0].data_ptr(), de[1].data_ptr())

    def call():
        if lib.cart_orb_detect(orb._h, 2, imgs, steps, ch, W, H, kps, des, None, vp(counts), stream) != 0:
            sys.exit("cart_orb_detect: " + lib.cart_last_error(eng._h).decode())
    call.keep = (tl, tr)
    call()
    return call, [(kp[i], de[i], counts[i:i + 1]) for i in range(2)]


rng = np.random.default_rng(1)


def random_set():
    k = torch.zeros((N, 7), dtype=torch.float32, device="cuda")
    k[:, 0] = torch.from_numpy(rng.integers(0, 4 * W, N).astype(np.float32) / 4).cuda()
    k[:, 1] = torch.from_numpy(rng.integers(0, 4 * H, N).astype(np.float32) / 4).cuda()
    return k, torch.from_numpy(rng.integers(0, 256, (N, 32)).astype(np.uint8)).cuda(), torch.tensor([N], dtype=torch.int32, device="cuda")


cases = {}
rq, rt = random_set(), random_set()
cases["5000 x 5000 random, gate off"] = match_call(match_params(), rq, rt)
cases["5000 x 5000 random, gate off, no cross-check"] = match_call(match_params(cross_check=0), rq, rt)
cases["5000 x 5000 random, temporal preset"] = match_call(TEMPORAL, rq, rt)
cases["5000 x 5000 random, stereo preset"] = match_call(STEREO, rq, rt)
sizes = {}
for name, ch in (("synthetic gray", 1), ("synthetic BGR", 3)):
    f0, f1 = (synth.make_pair(W, H, 128, 4, seed=7, frame=f, channels=ch)[:2] for f in (0, 1))
    det1, (l1, r1) = detect(*f1)
    _, (l0, _) = detect(*f0)
    torch.cuda.synchronize()
    sizes[name] = (int(l1[2].item()), int(r1[2].item()), int(l0[2].item()))
    cases[f"{name}: cart_orb_detect of the pair"] = det1
    cases[f"{name}: stereo match {sizes[name][0]} x {sizes[name][1]}"] = match_call(STEREO, l1, r1)
    cases[f"{name}: temporal match {sizes[name][0]} x {sizes[name][2]}"] = match_call(TEMPORAL, l1, l0)
    cases[f"{name}: stereo match, gate off"] = match_call(match_params(), l1, r1)

for call in cases.values():
    for _ in range(10):
        call()
torch.cuda.synchronize()
rounds = 1 if args.trace else args.rounds
ms = {name: [] for name in cases}
for _ in range(rounds):
    for name, call in cases.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            call()
        b.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(b) / args.iters)
for name, v in ms.items():
    print(f"{name}: {np.median(v):.4f} ms per call (min {min(v):.4f}, max {max(v):.4f}; {rounds} rounds of {args.iters})", flush=True)
orb.close()
matcher.close()
eng.close()

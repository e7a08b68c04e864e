"""Device time of the windowed bundle adjustment: ms per cart_local_ba_push and per cart_local_ba_optimize at window 8 with
torch events, --rounds alternating rounds of --iters calls per case after a warm-up, beside the calls that make the pose this stage
refines, timed on the same frames in the same run (the yardstick): cart_ego_triangulate + cart_ego_estimate.  The frames are a synthetic
drive (tests/np_localba.py, drive) walked forwards and backwards without end, so every push continues the tracks of the one before; all
lists are on the device before the first timed call, so a figure is the launch sequence alone.  An optimise changes the estimates but not
the work: the iteration count is fixed and there is no early exit.  `--trace` runs only the first round (for one `rocprofv3 --kernel-trace
--stats -- python localba_stages.py --trace` run of its own, which gives the per-kernel times)."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import np_ego as E
import np_localba as B

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--points", type=int, default=900)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
WINDOW, MAX_POINTS = 8, 8192

import torch
torch.zeros(1, device="cuda")
from cartslam import EgoCamera, EgoMotion, Engine, LocalBA, local_ba_params
from cartslam.engine import ego_params

CAM = E.camera(cx=160.0, cy=96.0)
cam_tuple = tuple(CAM[k] for k in ("fx", "fy", "cx", "cy", "baseline"))
drive = B.drive(1, args.frames, args.points, CAM)
N = max(len(f["kpL"]) for f in drive) + 1
eng = Engine(64, 32, num_disparities=0, paths=0)
ba, ego = LocalBA(eng, N, WINDOW, MAX_POINTS), EgoMotion(eng, cam_tuple, N)
camera = EgoCamera(*cam_tuple)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
P, PE = local_ba_params(), ego_params()


def rows(a, width, dtype):
    full = np.zeros((N, width), dtype)
    full[:len(a)] = a.view(dtype).reshape(-1, width)
    return torch.from_numpy(full).cuda()


def count(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def backwards(nxt):
    """The temporal list of a frame that follows the frame after it: the next frame's list with its two ends swapped, in query order."""
    m = np.zeros(len(nxt), E.MATCH_DTYPE)
    m["query"], m["train"] = nxt["train"], nxt["query"]
    return m[np.argsort(m["query"], kind="stable")]


dev = []
for k, f in enumerate(drive):
    back = backwards(drive[k + 1]["temporal"]) if k + 1 < len(drive) else f["temporal"][:0]
    dev.append(dict(pose=(C.c_double * 12)(*f["odom"]), kl=rows(f["kpL"], 7, np.float32), kr=rows(f["kpR"], 7, np.float32), nl=count(len(f["kpL"])),
                    st=rows(f["stereo"], 4, np.int32), ns=count(len(f["stereo"])), fwd=(rows(f["temporal"], 4, np.int32), count(len(f["temporal"]))),
                    back=(rows(back, 4, np.int32), count(len(back))), lm=torch.zeros((N, 4), dtype=torch.float64, device="cuda")))
counts = torch.zeros(8, dtype=torch.int32, device="cuda")
result = torch.zeros(5, dtype=torch.float64, device="cuda")
ego_result = torch.zeros(15, dtype=torch.float64, device="cuda")
walk = {"at": 0, "step": 1, "n": 0}


def advance():
    """-> (the frame to push, its temporal list against the frame pushed before)."""
    k, step = walk["at"], walk["step"]
    f = dev[k]
    tm = f["fwd"] if step > 0 else f["back"]
    if not 0 <= k + step < len(dev):
        walk["step"] = step = -step
    walk["at"] = k + step
    walk["n"] += 1
    return f, tm


def push():
    f, (tm, nt) = advance()
    if lib.cart_local_ba_push(ba._h, C.byref(camera), C.byref(P), walk["n"], f["pose"], vp(f["kl"]), vp(f["kr"]), vp(f["nl"]), vp(f["st"]), vp(f["ns"]), vp(tm),
                              vp(nt), vp(counts), stream) != 0:
        sys.exit("cart_local_ba_push: " + lib.cart_last_error(eng._h).decode())


def optimize():
    if lib.cart_local_ba_optimize(ba._h, C.byref(camera), C.byref(P), vp(result), stream) != 0:
        sys.exit("cart_local_ba_optimize: " + lib.cart_last_error(eng._h).decode())


def push_then_optimize():
    push()
    optimize()


def ego_pair(k=[1]):
    """What makes the pose of one frame: the frame's landmarks, then the estimate against the previous frame's."""
    cur, prev = dev[k[0]], dev[k[0] - 1]
    k[0] = k[0] + 1 if k[0] + 1 < len(dev) else 1
    if lib.cart_ego_triangulate(ego._h, C.byref(ego.camera), C.byref(PE), vp(cur["kl"]), vp(cur["kr"]), vp(cur["nl"]), vp(cur["st"]), vp(cur["ns"]), vp(cur["lm"]), stream) != 0:
        sys.exit("cart_ego_triangulate: " + lib.cart_last_error(eng._h).decode())
    tm, nt = cur["fwd"]
    if lib.cart_ego_estimate(ego._h, C.byref(ego.camera), C.byref(PE), vp(cur["lm"]), vp(cur["kl"]), vp(prev["lm"]), vp(tm), vp(nt), 0, k[0], vp(ego_result), None, stream) != 0:
        sys.exit("cart_ego_estimate: " + lib.cart_last_error(eng._h).decode())


# every landmark table once, so that the yardstick's "previous" tables hold that frame's landmarks
for f in dev:
    lib.cart_ego_triangulate(ego._h, C.byref(ego.camera), C.byref(PE), vp(f["kl"]), vp(f["kr"]), vp(f["nl"]), vp(f["st"]), vp(f["ns"]), vp(f["lm"]), stream)
cases = {"cart_local_ba_push": push, "cart_local_ba_optimize (4 steps)": optimize, "push + optimize, as the module runs them": push_then_optimize,
         "yardstick: cart_ego_triangulate + cart_ego_estimate": ego_pair}
for _ in range(2 * WINDOW):
    push()
for call in cases.values():
    for _ in range(10):
        call()
torch.cuda.synchronize()
rounds = 1 if args.trace else args.rounds
ms = {name: [] for name in cases}
sizes = []
for _ in range(rounds):
    for name, call in cases.items():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            call()
        e.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(e) / args.iters)
    optimize()
    torch.cuda.synchronize()
    r, c = result.cpu().numpy().view(B.RESULT_DTYPE)[0], counts.cpu().numpy()
    sizes.append((int(c[0]), int(c[6]), int(r["n_points_active"]), int(r["n_observations"]), int(r["status"])))
print(f"window {WINDOW}, max_points {MAX_POINTS}, max_features {N}; after each round (keypoints of the last push, live points, active points, observations, status): {sizes}")
for name, v in ms.items():
    print(f"{name}: {np.median(v):.4f} ms per call (min {min(v):.4f}, max {max(v):.4f}; {rounds} rounds of {args.iters})", flush=True)
base = np.median(ms["yardstick: cart_ego_triangulate + cart_ego_estimate"])
for name in list(cases)[:3]:
    print(f"{name} / yardstick: {np.median(ms[name]) / base:.2f}")
for o in (ba, ego, eng):
    o.close()

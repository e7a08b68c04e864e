"""Device time of rebuilding the plane map from stored keyframes: ms per frame of one cart_plane_map_rebuild over N
stored frames against the yardstick, N sequential cart_plane_map_update calls of the same frames and poses into a fixed window, for
N = 16, 64 and 256; and ms per cart_plane_store_insert against cart_reproject_depth of the same image.  Torch events, a warm-up,
--rounds alternating rounds, median and range.  The frame is the synthetic 1242x375 street corridor (synth.road_corridor) in N device
copies (the updates read N distinct images, as the rebuild does), voted into a 512x512 grid of 0.25 m cells; the poses lie on a closed
circle of 1.8 m radius that revisits its start and stays inside one window, so both paths must leave the same bytes, which is checked.
`--trace` runs the warm-up and one round only (for one `rocprofv3 --kernel-trace --stats -- python plane_map_rebuild_stages.py --trace`
run of its own, which gives the per-kernel rows).  CART_ENGINE_LIB selects another build of the library (the kRevoteStrip candidates)."""
import argparse, ctypes as C, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np
from cartslam import synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, nargs="+", default=[16, 64, 256])
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
W, H, N = 1242, 375, 512
CAMERA = (721.5, 721.5, 609.5, 172.85, 0.54)   # KITTI-like intrinsics

import torch
torch.zeros(1, device="cuda")
from cartslam import Engine, PlaneMap, PlaneStore

eng = Engine(W, H, num_disparities=0, paths=0)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
disp_host, planes_host = synth.road_corridor(W, H, *CAMERA)
most = max(args.frames)
disp = torch.from_numpy(disp_host).cuda().unsqueeze(0).repeat(most, 1, 1).contiguous()
planes = torch.from_numpy(planes_host).cuda().unsqueeze(0).repeat(most, 1, 1).contiguous()
xyz = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
fx, fy, cx, cy, b = CAMERA
Q = (C.c_float * 16)(1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 0, fx, 0, 0, -1 / b, 0)
store = PlaneStore(eng, W, H, most)
for k in range(most):
    store.insert(k, disp[k], planes[k], raw=True)


def loop_poses(n):
    """n poses on a circle through (2, 0.2) .. back to the start, heading along the tangent: every translation stays in [0.2, 3.8]^2, one window."""
    out = []
    for k in range(n):
        a = 2.0 * math.pi * k / n
        c, s = math.cos(a), math.sin(a)
        out.append([c, 0.0, s, 2.0 + 1.8 * s, 0.0, 1.0, 0.0, 0.0, -s, 0.0, c, 2.0 - 1.8 * c])
    return out


def fail(what):
    sys.exit(what + ": " + lib.cart_last_error(eng._h).decode())


def make_cases(n):
    poses = loop_poses(n)
    flat = (C.c_double * (12 * n))(*[v for p in poses for v in p])
    each = [(C.c_double * 12)(*p) for p in poses]
    ids = (C.c_uint64 * n)(*range(n))
    seq, reb = PlaneMap(eng, CAMERA, N, N), PlaneMap(eng, CAMERA, N, N)

    def sequential():
        lib.cart_plane_map_clear(seq._h)
        for k in range(n):
            if lib.cart_plane_map_update(seq._h, C.byref(seq.camera), each[k], vp(disp[k]), W * 2, vp(planes[k]), W, W, H, stream) != 0:
                fail("cart_plane_map_update")

    def rebuild():
        if lib.cart_plane_map_rebuild(reb._h, store._h, C.byref(reb.camera), ids, flat, n, each[n - 1], None, stream) != 0:
            fail("cart_plane_map_rebuild")

    return seq, reb, sequential, rebuild


def insert():
    if lib.cart_plane_store_insert(store._h, 0, vp(disp[0]), W * 2, vp(planes[0]), W, W, H, stream) != 0:
        fail("cart_plane_store_insert")


def reproject():
    if lib.cart_reproject_depth(eng._h, 1, vp(disp[0]), W * 2, 0, Q, vp(xyz), xyz.stride(0) * 4, 0, stream) != 0:
        fail("cart_reproject_depth")


def timed(call, iters):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        call()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters


rounds = 1 if args.trace else args.rounds
for n in args.frames:
    seq, reb, sequential, rebuild = make_cases(n)
    for call in (sequential, rebuild):
        call()
    torch.cuda.synchronize()
    a, b2 = seq.read(), reb.read()
    if a[1] != b2[1] or a[0].tobytes() != b2[0].tobytes():
        sys.exit(f"N = {n}: the rebuilt map differs from the sequential one")
    cells = a[0]
    print(f"N = {n}: {int(cells['horizontal'].sum())} horizontal and {int(cells['vertical'].sum())} vertical votes in "
          f"{int(((cells['horizontal'] > 0) | (cells['vertical'] > 0)).sum())} cells, largest cell {int(cells['vertical'].max())}; both paths byte-equal", flush=True)
    ms = {"sequential": [], "rebuild": []}
    for _ in range(rounds):
        ms["sequential"].append(timed(sequential, args.iters) / n)
        ms["rebuild"].append(timed(rebuild, args.iters) / n)
    for name, label in (("sequential", f"{n} x cart_plane_map_update"), ("rebuild", f"cart_plane_map_rebuild of {n}")):
        v = ms[name]
        print(f"N = {n}: {label}: {np.median(v):.4f} ms per frame (min {min(v):.4f}, max {max(v):.4f}; {rounds} rounds of {args.iters})", flush=True)
    print(f"N = {n}: rebuild / sequential per frame = {np.median(ms['rebuild']) / np.median(ms['sequential']):.3f}; one rebuild = {np.median(ms['rebuild']) * n:.3f} ms", flush=True)
    seq.close()
    reb.close()
ms = {"cart_plane_store_insert": [], "cart_reproject_depth of the same frame": []}
for call in (insert, reproject):
    for _ in range(10):
        call()
torch.cuda.synchronize()
for _ in range(rounds):
    ms["cart_plane_store_insert"].append(timed(insert, 100))
    ms["cart_reproject_depth of the same frame"].append(timed(reproject, 100))
for name, v in ms.items():
    print(f"{name}: {np.median(v):.4f} ms per call (min {min(v):.4f}, max {max(v):.4f}; {rounds} rounds of 100)", flush=True)
print(f"cart_plane_store_insert: {np.median(ms['cart_plane_store_insert']) / np.median(ms['cart_reproject_depth of the same frame']):.2f} x cart_reproject_depth", flush=True)
store.close()
eng.close()

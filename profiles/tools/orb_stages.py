"""Device time of the ORB feature stage at 1242x375: one cart_orb_detect for a stereo pair, timed with torch
events (mean of --iters calls after a warm-up) on three inputs: a synthetic KITTI-like pair (BGR), a gray pair, and 2x2
block noise (every level over its quota: the selection's worst case).  Output buffers are allocated once, so the figure is
the launch sequence alone; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np
import torch
torch.zeros(1, device="cuda")
from cartslam import Engine, OrbFeatures, synth

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--nfeatures", type=int, default=5000)
args = ap.parse_args()
w, h, N = 1242, 375, args.nfeatures
eng = Engine(w, h, num_disparities=0, paths=0)
orb = OrbFeatures(eng, w, h, nfeatures=N)
lib = eng._lib
kp = torch.empty((2, N, 7), dtype=torch.float32, device="cuda")
de = torch.empty((2, N, 32), dtype=torch.uint8, device="cuda")
counts = torch.zeros(2, dtype=torch.int32, device="cuda")


def noise(seed):
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 256, (h // 2 + 1, w // 2 + 1)), np.ones((2, 2), np.int64))[:h, :w].astype(np.uint8)


inputs = {"synthetic BGR pair": synth.make_pair(w, h, 64, 4, seed=7, channels=3)[:2],
          "synthetic gray pair": synth.make_pair(w, h, 64, 4, seed=7, channels=1)[:2],
          "2x2 block noise pair": (noise(1), noise(2))}
for name, (l, r) in inputs.items():
    tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
    ch = 1 if tl.dim() == 2 else 3
    imgs = (C.c_void_p * 2)(tl.data_ptr(), tr.data_ptr())
    steps = (C.c_size_t * 2)(tl.stride(0), tr.stride(0))
    kps = (C.c_void_p * 2)(kp[0].data_ptr(), kp[1].data_ptr())
    des = (C.c_void_p * 2)(de[0].data_ptr(), de[1].data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        if lib.cart_orb_detect(orb._h, 2, imgs, steps, ch, w, h, kps, des, None, C.c_void_p(counts.data_ptr()), stream) != 0:
            sys.exit("cart_orb_detect: " + lib.cart_last_error(eng._h).decode())

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        call()
    b.record()
    torch.cuda.synchronize()
    c = counts.cpu().tolist()
    print(f"{w}x{h} N={N} {name}: {a.elapsed_time(b) / args.iters:.4f} ms per pair ({c[0]} + {c[1]} keypoints, {args.iters} calls)")
orb.close()
eng.close()

"""Frames/s of [disparity, orb_features] beside [disparity] in the C++ frame loop (cart_slam_amd, <= 12 frames in flight) at
1242x375, BGR synthetic frames.  Steady state: wall time of N frames minus that of N0 frames.  Disparity at the reference's
defaults with smoothing 3/4, as in planefit_throughput.py."""
import json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
from cartslam import synth
EXE = os.path.join(ROOT, "cart-slam_amd", "build", "cart_slam_amd")
tmp = tempfile.mkdtemp(dir="/tmp")
d = os.path.join(tmp, "ds", "sequences", "00"); os.makedirs(d + "/image_2"); os.makedirs(d + "/image_3")
N, N0 = int(os.environ.get("N", 480)), int(os.environ.get("N0", 96))
base = [synth.make_pair(1242, 375, 128, 4, frame=f, channels=3) for f in range(4)]
for f in range(N):
    l, r, _ = base[f % 4]
    for cam, img in ((2, l), (3, r)):
        if f >= 4:
            os.link(f"{d}/image_{cam}/{f % 4:06d}.ppm", f"{d}/image_{cam}/{f:06d}.ppm")
            continue
        with open(f"{d}/image_{cam}/{f:06d}.ppm", "wb") as fh:
            fh.write(b"P6\n1242 375\n255\n"); fh.write(img.tobytes())
json.dump({"type": "kitti", "path": os.path.join(tmp, "ds"), "sequence": 0}, open(tmp + "/src.json", "w"))
DISP = {"type": "disparity", "smoothing_radius": 3, "smoothing_iterations": 4}
for name, mods in (("[disparity]", [DISP]), ("[disparity, orb_features]", [DISP, {"type": "orb_features"}]),
                   ("[orb_features]", [{"type": "orb_features"}])):
    json.dump(mods, open(tmp + "/mod.json", "w"))
    ts, out = [], ""
    for n in (N0, N):
        t0 = time.perf_counter()
        r = subprocess.run([EXE, tmp + "/src.json", tmp + "/mod.json", "--frames", str(n)], capture_output=True, text=True, timeout=600)
        ts.append(time.perf_counter() - t0)
        if r.returncode != 0:
            sys.exit(f"{name}: rc {r.returncode}\n{r.stderr[-2000:]}")
        out = r.stdout.strip()
    print(f"{name}: {(N - N0) / (ts[1] - ts[0]):.0f} frames/s  ({out})")

"""A/B of CART_OPT_BAND_DIAG inside one process (profiles/band_diag.txt sections 2 and 3): plan band_up at 1242x375, D=128, 8 paths, the option
off / on alternating, ROUNDS rounds x CALLS calls per configuration and launch size, the first call after a switch dropped, placement search off.

  python3 profiles/tools/band_diag_ab.py run [n_frames ...]      the calls themselves; prints ms per compute call (device events) per round
  python3 profiles/tools/band_diag_ab.py trace DIR [n_frames ...] reads the *_kernel_trace.csv rocprofv3 left under DIR for such a run and prints the
                                                                 band kernel's and the aggregation kernel's time per round (dispatch order)
  python3 profiles/tools/band_diag_ab.py counters DIR            medians per kernel of a *_counter_collection.csv (one counter per pass)
Run it plainly, under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 ... run`, or under `rocprofv3 --pmc COUNTER ...`."""
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "cart-slam_amd"))
ROUNDS, CALLS = int(os.environ.get("AB_ROUNDS", 4)), int(os.environ.get("AB_CALLS", 8))   # (the counter passes run 1 x 4)
W, H, D, P = 1242, 375, 128, 8


def sizes(argv):
    return [int(a) for a in argv] or [16]


def run(ns, rounds=ROUNDS, calls=CALLS):
    import torch
    from cartslam import Engine, synth
    for n in ns:
        ls, rs = synth.make_batch(n, W, H, D, 4, seed=3)
        L, R = torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda()
        eng = Engine(W, H, num_disparities=D, paths=P, min_disparity=4, smoothing_radius=2, smoothing_iterations=1, max_inflight=n)
        eng.set_plan("band_up")
        assert eng.describe_plan(n) == {"frames_per_launch": n, "plan": "band_up", "slabs_written": 7}
        out = {0: [], 1: []}
        ref = None
        for _ in range(rounds):
            for on in (0, 1):
                eng.set_band_diag(bool(on))
                assert eng.get_option(9) == on
                ms = []
                for c in range(calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    d = eng.compute_disparity(L, R)
                    e1.record()
                    e1.synchronize()
                    if c:
                        ms.append(e0.elapsed_time(e1))
                out[on].append(round(statistics.median(ms), 4))
                if ref is None:
                    ref = d.clone()
                assert bool((d == ref).all()), "the two kernels differ"
        eng.close()
        print(f"== n_frames {n}: ms per compute call (device events), median of {calls - 1} calls per round")
        print("off", out[0])
        print("on ", out[1])
        sys.stdout.flush()


def trace(d, ns, rounds=ROUNDS, calls=CALLS):
    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    band = [(r["Kernel_Name"], dur(r)) for r in rows if "wta_band_kernel" in r["Kernel_Name"]]
    agg = [dur(r) for r in rows if "aggregate_kernel" in r["Kernel_Name"]]
    assert len(band) == len(agg) == len(ns) * rounds * 2 * calls, (len(band), len(agg))
    i = 0
    for n in ns:
        res = {}
        for _ in range(rounds):
            for on in (0, 1):
                names = {k for k, _ in band[i:i + calls]}
                assert len(names) == 1, names
                key = names.pop().split("(")[0]
                res.setdefault(key, ([], []))
                res[key][0].append(round(statistics.median(t for _, t in band[i + 1:i + calls]), 4))
                res[key][1].append(round(statistics.median(agg[i + 1:i + calls]), 4))
                i += calls
        print(f"== n_frames {n}: kernel trace, ms, median of {calls - 1} launches per round")
        for key, (wt, ag) in res.items():
            print(f"{key[-44:]:44s} wta {wt} median {statistics.median(wt):.4f} | aggregate {ag}")


def counters(d):
    vals = {}
    for p in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(p)):
            if "wta_band_kernel" in r["Kernel_Name"] or "aggregate_kernel" in r["Kernel_Name"]:
                vals.setdefault((r["Kernel_Name"].split("(")[0], r["Counter_Name"]), []).append(float(r["Counter_Value"]))
    for (k, c), v in sorted(vals.items()):
        print(f"{k[-48:]:48s} {c:12s} launches {len(v):3d} median {statistics.median(v):14.1f}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sizes(sys.argv[2:]))
    elif sys.argv[1] == "trace":
        trace(sys.argv[2], sizes(sys.argv[3:]))
    else:
        counters(sys.argv[2])

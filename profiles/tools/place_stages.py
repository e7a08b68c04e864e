"""Device time of the place recognition query: ms per cart_place_query against K stored frames, and per run of the
yardstick -- what a user does without the stage: K calls of cart_matcher_match (gate off, cross_check 0, the same max_distance and ratio)
against K separate train sets, whose K match counts are the scores -- with torch events, --rounds alternating rounds of --iters runs per
case after a warm-up.  Cases: 5000 features x K = 16, 64, 256 and 800 features (a synthetic pair's yield) x K = 64, every object made for
5000 features.  The descriptors are random bytes (the kernels have no data-dependent branch); the stored frames of a case are the train
sets of its yardstick, and the two must count the same votes.  Buffers are allocated once, so a figure is the launch sequence alone.
`--trace` runs one short round (for one `rocprofv3 --kernel-trace --stats -- python place_stages.py --trace` run of its own, which gives the
per-kernel times).  CART_ENGINE_LIB selects another build of the library (the one- against two-queries-per-lane A/B of 7.9:
make HIPFLAGS="... -DCART_PLACE_QUERIES_PER_LANE=2" OUT=<dir>)."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "cart-slam_amd")]
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--cases", default="5000x16,5000x64,5000x256,800x64")
args = ap.parse_args()
MF = 5000

import torch
torch.zeros(1, device="cuda")
from cartslam import Engine, OrbMatcher, PlaceDB, place_params
from cartslam.engine import match_params

eng = Engine(64, 32, num_disparities=0, paths=0)
lib = eng._lib
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
matcher = OrbMatcher(eng, MF)
MP = match_params(use_gate=0, cross_check=0)
PP = place_params(min_gap=0, min_score=0)
gen = torch.Generator(device="cuda").manual_seed(27)
matches = torch.empty((MF, 4), dtype=torch.int32, device="cuda")
kp = torch.zeros((MF, 7), dtype=torch.float32, device="cuda")


def make_case(n, K):
    train = torch.randint(0, 256, (K, MF, 32), dtype=torch.uint8, device="cuda", generator=gen)
    query = train[K // 2].clone()
    flip = torch.randint(0, 256, (MF, 32), dtype=torch.uint8, device="cuda", generator=gen) & torch.randint(0, 256, (MF, 32), dtype=torch.uint8, device="cuda", generator=gen) \
        & torch.randint(0, 256, (MF, 32), dtype=torch.uint8, device="cuda", generator=gen)
    query ^= flip                                       # about 32 of 256 bits away from frame K / 2: that slot collects votes, the others next to none
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    db = PlaceDB(eng, MF, K)
    for k in range(K):
        if lib.cart_place_insert(db._h, vp(train[k]), 32, vp(kp), None, vp(count), k, None, stream) != 0:
            sys.exit("cart_place_insert: " + lib.cart_last_error(None).decode())
    counts = torch.zeros(K, dtype=torch.int32, device="cuda")
    scores = torch.zeros(K, dtype=torch.int32, device="cuda")
    cand = torch.zeros((PP.max_candidates, 2), dtype=torch.int64, device="cuda")
    ncand = torch.zeros(1, dtype=torch.int32, device="cuda")

    each = [(vp(train[k]), vp(counts[k:k + 1])) for k in range(K)]   # the addresses once: the loop below is the K calls alone
    q, c, m, mp = vp(query), vp(count), vp(matches), C.byref(MP)

    def yardstick():
        for t, out in each:
            if lib.cart_matcher_match(matcher._h, mp, q, 32, None, c, t, 32, None, c, m, out, None, stream) != 0:
                sys.exit("cart_matcher_match: " + lib.cart_last_error(None).decode())

    def place():
        if lib.cart_place_query(db._h, C.byref(PP), vp(query), 32, vp(count), 1 << 40, vp(scores), vp(cand), vp(ncand), stream) != 0:
            sys.exit("cart_place_query: " + lib.cart_last_error(None).decode())
    return yardstick, place, counts, scores, (db, train, query, count, counts, scores, cand, ncand)   # every buffer a call writes stays allocated


cases, keep = {}, []
for spec in args.cases.split(","):
    n, K = (int(v) for v in spec.split("x"))
    y, p, counts, scores, hold = make_case(n, K)
    keep.append(hold)
    for _ in range(2):
        y()
        p()
    torch.cuda.synchronize()
    cases[f"{n} features x {K} frames: {K} x cart_matcher_match"] = y
    cases[f"{n} features x {K} frames: cart_place_query"] = p


def verify(when):
    """the two must count the same votes, before the timing and after it"""
    for spec, hold in zip(args.cases.split(","), keep):
        n, K = (int(v) for v in spec.split("x"))
        c, s = hold[4].cpu().numpy(), hold[5].cpu().numpy()
        if (c != s).any() or int(hold[3].item()) != n:
            sys.exit(f"{spec} {when}: the query's scores differ from the yardstick's counts: {s[:8]} != {c[:8]}")
        print(f"{spec} {when}: scores equal the {K} match counts (best slot {int(s.argmax())} with {int(s.max())} votes of {n}, median {int(np.median(s))})", flush=True)


verify("before the timing")
rounds, iters = (1, 2) if args.trace else (args.rounds, args.iters)
ms = {name: [] for name in cases}
for _ in range(rounds):
    for name, call in cases.items():
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            call()
        e.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(e) / iters)
verify("after the timing")
for name, v in ms.items():
    print(f"{name}: {np.median(v):.4f} ms per run (min {min(v):.4f}, max {max(v):.4f}; {rounds} rounds of {iters})", flush=True)
names = list(cases)
for y, p in zip(names[0::2], names[1::2]):
    n, K = (int(v) for v in (p.split(" ")[0], p.split(" ")[3]))
    t = np.median(ms[p])
    print(f"{p}: {np.median(ms[y]) / t:.2f} x faster than the yardstick; {n * K * n / t / 1e6:.1f} G descriptor pairs per second", flush=True)

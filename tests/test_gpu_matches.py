"""GPU tests of the ORB descriptor matcher (spec S22): cart_matcher_match's match list, count and forward table
equal the numpy restatement (tests/np_match.py) bit for bit, and the "orb_matches" module through the C++ frame loop equals
the restatement fed with the restated features (tests/np_orb.py) of every frame.

The kernels as built: match_pairs has 128 rows per workgroup and stages 128 columns in LDS at a time (kMatchRows, kMatchTile);
a column chunk is one tile up to max_features = 8192 and 8 tiles = 1024 columns at 65536 (at most 64 chunks); match_merge has
256 rows per workgroup; match_select compacts 1024 queries per round."""
import ctypes as C
import os

import numpy as np
import pytest

import np_match as M
import np_orb as N

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


_ENGINE = []


def engine():
    from cartslam import Engine
    if not _ENGINE:
        _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's (see __graft_entry__.build)
        _ENGINE.append(Engine(64, 32, num_disparities=0, paths=0))
    return _ENGINE[0]


def mp(p):
    from cartslam.engine import match_params
    return match_params(**p)


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32)).astype(np.uint8)


def flip_bits(rng, d, k):
    """d [32] with k distinct random bits inverted."""
    o = d.copy()
    for b in rng.choice(256, k, replace=False):
        o[b // 8] ^= 1 << (b % 8)
    return o


def related_sets(rng, nq, nt):
    """Train = random descriptors; every second query is a train descriptor with 0..80 bits flipped, the rest are random."""
    td = rand_desc(rng, nt)
    qd = rand_desc(rng, nq)
    if nt:
        for i in range(0, nq, 2):
            qd[i] = flip_bits(rng, td[rng.integers(0, nt)], int(rng.integers(0, 81)))
    return qd, td


def rand_kps(rng, n, w=64, h=8, octaves=4):
    k = np.zeros(n, N.KEYPOINT_DTYPE)
    k["x"] = rng.integers(0, 4 * w, n).astype(np.float32) / 4
    k["y"] = rng.integers(0, 4 * h, n).astype(np.float32) / 4
    k["octave"] = rng.integers(0, octaves, n)
    return k


def check(matcher, qd, td, p, qk=None, tk=None, expect=None):
    """One call against the restatement: match list, count and forward table, bit for bit."""
    m, f = matcher.match((qk, qd, None), (tk, td, None), mp(p), want_forward=True)
    em, ef = expect if expect is not None else M.match(qd, td, p, qk, tk)
    assert f.shape == ef.shape and (f == ef).all(), f"forward table differs at rows {np.nonzero((f != ef).any(1))[0][:8]}"
    assert len(m) == len(em), f"count {len(m)} != {len(em)}"
    assert m.tobytes() == em.tobytes(), "match list differs"
    return m, f


SIZES = [(0, 0), (0, 65), (1, 0), (1, 1), (2, 1), (63, 64), (64, 65), (65, 63), (257, 2), (2, 257), (257, 257), (1000, 257), (257, 1000),
         (1000, 1000)]


@pytest.fixture(scope="module")
def matcher1000():
    from cartslam import OrbMatcher
    m = OrbMatcher(engine(), 1000)
    yield m
    m.close()


@pytest.mark.parametrize("nq,nt", SIZES)
def test_sizes(matcher1000, nq, nt):
    rng = np.random.default_rng(1000 * nq + nt)
    qd, td = related_sets(rng, nq, nt)
    m, _ = check(matcher1000, qd, td, M.params())
    if min(nq, nt) >= 63:
        assert len(m) > 0
    check(matcher1000, rand_desc(rng, nq), td, M.params(ratio=0, max_distance=256, cross_check=0))   # pure noise: everything accepted


def test_full_size_5000():
    from cartslam import OrbMatcher
    rng = np.random.default_rng(5)
    qd, td = related_sets(rng, 5000, 5000)
    qk, tk = rand_kps(rng, 5000, 1242, 375), rand_kps(rng, 5000, 1242, 375)
    matcher = OrbMatcher(engine(), 5000)
    m, _ = check(matcher, qd, td, M.params())
    assert len(m) > 500
    check(matcher, qd, td, M.temporal_params(400), qk, tk)
    matcher.close()


def test_capacity_65536_with_small_counts():
    """Chunks of 1024 columns: 1100 train descriptors cross a chunk boundary, 300 queries three row blocks."""
    from cartslam import OrbMatcher
    rng = np.random.default_rng(6)
    qd, td = related_sets(rng, 300, 1100)
    matcher = OrbMatcher(engine(), 65536)
    m, _ = check(matcher, qd, td, M.params())
    assert len(m) > 20
    check(matcher, td, qd, M.params(ratio=0))
    matcher.close()


def test_device_counts_below_the_capacity_and_pitched_rows():
    """The rows beyond the device counts hold copies of query descriptors (distance 0: they would win if they were read); the
    descriptor rows are 96 bytes apart."""
    torch = _torch()
    from cartslam import OrbMatcher
    rng = np.random.default_rng(7)
    cap, nq, nt = 400, 150, 201
    qd, td = related_sets(rng, nq, nt)
    qk, tk = rand_kps(rng, nq), rand_kps(rng, nt)
    full = lambda d: np.concatenate([d, np.resize(qd, (cap - len(d), 32))])   # noqa: E731
    fullk = lambda k: np.concatenate([k, np.resize(qk, cap - len(k))])        # noqa: E731

    def pitched(d):
        buf = torch.zeros((cap, 96), dtype=torch.uint8, device="cuda")
        buf[:, :32] = torch.from_numpy(d).cuda()
        return buf[:, :32]

    dev_k = lambda k: torch.from_numpy(k.view(np.float32).reshape(-1, 7)).cuda()   # noqa: E731
    cnt = lambda n: torch.tensor([n], dtype=torch.int32, device="cuda")            # noqa: E731
    matcher = OrbMatcher(engine(), cap)
    for p in (M.params(ratio=0), M.temporal_params(16)):
        q = (dev_k(fullk(qk)), pitched(full(qd)), cnt(nq))
        t = (dev_k(fullk(tk)), pitched(full(td)), cnt(nt))
        assert q[1].stride(0) == 96
        m, f = matcher.match(q, t, mp(p), want_forward=True)
        em, ef = M.match(qd, td, p, qk, tk)
        assert (f == ef).all() and m.tobytes() == em.tobytes()
    # counts outside [0, capacity] are clamped
    m, f = matcher.match((None, pitched(full(qd)), cnt(-3)), (None, pitched(full(td)), cnt(nt)), mp(M.params()), want_forward=True)
    assert len(m) == 0 and f.shape == (0, 4)
    q_all, t_all = full(qd), full(td)
    m, f = matcher.match((None, pitched(q_all), cnt(nq)), (None, pitched(t_all), cnt(cap + 1000)), mp(M.params(ratio=0)), want_forward=True)
    em, ef = M.match(qd, t_all, M.params(ratio=0))
    assert (f == ef).all() and m.tobytes() == em.tobytes()
    matcher.close()


def test_ties_duplicated_and_permuted(matcher1000):
    rng = np.random.default_rng(8)
    qd = rand_desc(rng, 300)
    perm = rng.permutation(600)
    td = np.concatenate([qd, qd])[perm]
    for p in (M.params(ratio=0), M.params(), M.params(ratio=0, cross_check=0)):
        m, f = check(matcher1000, qd, td, p)
        lowest = np.array([min(np.nonzero(perm % 300 == i)[0]) for i in range(300)])
        assert (f[:, 0] == lowest).all() and (f[:, 1] == 0).all() and (f[:, 2] == 0).all()
    # the other direction: the duplicates are queries, the lower one wins the cross-check
    m, f = check(matcher1000, td, qd, M.params(ratio=0))
    assert len(m) == 300 and (m["query"] == np.sort(lowest)).all()


def test_perturbed_copies_recover_the_permutation(matcher1000):
    rng = np.random.default_rng(9)
    n = 810
    qd = rand_desc(rng, n)
    perm = rng.permutation(n)
    k = np.arange(n) % 81                                      # bits flipped in the copy of query perm[j]
    td = np.array([flip_bits(rng, qd[perm[j]], int(k[j])) for j in range(n)])
    inv = np.argsort(perm)
    m, f = check(matcher1000, qd, td, M.params())
    # random 256-bit strings are ~128 +- 8 apart, so the planted copy is every query's best and mutual; S22 accepts it iff d1 <= 64 and
    # 100 d1 < 80 d2
    assert (f[:, 0] == inv).all() and (f[:, 1] == k[inv]).all() and (f[:, 3] == np.arange(n)).all()
    want = np.nonzero((f[:, 1] <= 64) & (100 * f[:, 1] < 80 * f[:, 2]))[0]
    assert (m["query"] == want).all() and (m["train"] == inv[want]).all() and len(want) > 600


PARAM_CASES = {
    "no_cross_check": M.params(cross_check=0),
    "max_distance": M.params(max_distance=20),
    "ratio_off": M.params(ratio=0),
    "ratio_100": M.params(ratio=100),
    "gate": M.params(use_gate=1, dx_min=-3.25, dx_max=7.5, dy_min=-1.0, dy_max=1.75),
    "gate_octave_0": M.params(use_gate=1, dx_min=-1000, dx_max=1000, dy_min=-1000, dy_max=1000, max_octave_diff=0),
    "gate_octave_1": M.params(use_gate=1, dx_min=-1000, dx_max=1000, dy_min=-1000, dy_max=1000, max_octave_diff=1),
    "stereo_preset": M.stereo_params(16, 1),
    "temporal_preset": M.temporal_params(8),
    "together": M.params(use_gate=1, dx_min=-3.25, dx_max=7.5, dy_min=-1.0, dy_max=1.75, max_octave_diff=1, max_distance=40, ratio=65, cross_check=0),
}


@pytest.fixture(scope="module")
def param_sets():
    rng = np.random.default_rng(10)
    qd, td = related_sets(rng, 500, 700)
    qd[1::4] = qd[0::4][:len(qd[1::4])]            # duplicates, so that the cross-check and the ratio test have work
    qk, tk = rand_kps(rng, 500), rand_kps(rng, 700)     # quarter-pixel coordinates: the gate bounds are hit exactly
    qk["x"][7], qk["y"][9], tk["x"][11] = np.nan, np.nan, np.nan
    return qd, td, qk, tk


@pytest.mark.parametrize("case", sorted(PARAM_CASES))
def test_parameters(matcher1000, param_sets, case):
    qd, td, qk, tk = param_sets
    p = PARAM_CASES[case]
    m, f = check(matcher1000, qd, td, p, qk, tk)
    assert len(m) > 0
    if p["use_gate"]:
        dx = qk["x"][:, None] - tk["x"][None, :]
        ok = M.admissible(qk, tk, p)
        if p["dx_max"] < 64:   # the coordinates span [0, 64): position bounds within reach are hit exactly, and those pairs are admissible
            assert (ok & (dx == np.float32(p["dx_min"]))).any() and (ok & (dx == np.float32(p["dx_max"]))).any(), "no pair sits on a gate bound"
        assert (f[[7, 9], 0] == -1).all() and (f[:, 0] != 11).all()     # NaN coordinates are never admissible
        base = M.match(qd, td, M.params(**{k: v for k, v in p.items() if k not in ("use_gate", "dx_min", "dx_max", "dy_min", "dy_max", "max_octave_diff")}))[1]
        assert (f != base).any(), "the gate changed nothing"


# ---- inputs straight from cart_orb_detect ---------------------------------------------------------------------------------
def _detect_raw(orb, imgs):
    """cart_orb_detect into full-capacity buffers on the current stream, with no host synchronisation."""
    torch = _torch()
    n = len(imgs)
    h, w = imgs[0].shape
    kp = torch.zeros((n, orb.nfeatures, 7), dtype=torch.float32, device="cuda")
    de = torch.zeros((n, orb.nfeatures, 32), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])   # noqa: E731
    orb._check(orb._lib.cart_orb_detect(orb._h, n, arr(imgs), (C.c_size_t * n)(*[t.stride(0) for t in imgs]), 1, w, h, arr(list(kp)), arr(list(de)),
                                        None, C.c_void_p(counts.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "cart_orb_detect")
    return [(kp[i], de[i], counts[i:i + 1]) for i in range(n)]


def noise_world(seed, h=104, w=380):
    """2x2 block noise: full of corners at every pyramid level, unlike the smooth synthetic scene."""
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 256, (h // 2, w // 2)), np.ones((2, 2), np.int64)).astype(np.uint8)


def noise_frame(world, f, w=320, h=96, disparity=6):
    """Frame f of a camera that moves 3 pixels right and 1 pixel down per frame: (left, right), the right image `disparity` pixels on."""
    x, y = 4 + 3 * f, 1 + f
    return np.ascontiguousarray(world[y:y + h, x:x + w]), np.ascontiguousarray(world[y:y + h, x + disparity:x + disparity + w])


def test_inputs_from_detect_without_a_host_round_trip():
    torch = _torch()
    from cartslam import OrbFeatures, OrbMatcher, synth
    w, h, nf = 320, 96, 1000
    frames = [synth.make_pair(w, h, 64, 4, seed=77, frame=f)[:2] for f in range(2)]
    noise = [noise_frame(noise_world(78), f) for f in range(2)]
    orb, matcher = OrbFeatures(engine(), w, h, nfeatures=nf), OrbMatcher(engine(), nf)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    cases = {"stereo": ((frames[1][0], frames[1][1]), M.stereo_params()), "temporal": ((frames[1][0], frames[0][0]), M.temporal_params()),
             "noise stereo": ((noise[1][0], noise[1][1]), M.stereo_params()), "noise temporal": ((noise[1][0], noise[0][0]), M.temporal_params())}
    for name, (imgs, p) in cases.items():
        ts = [dev(i) for i in imgs]
        torch.cuda.synchronize()
        q, t = _detect_raw(orb, ts)                            # queued ...
        m, f = matcher.match(q, t, mp(p), want_forward=True)   # ... and consumed on the same stream, the counts read on the device
        (qk, qd), (tk, td) = N.orb(imgs[0], nf), N.orb(imgs[1], nf)
        em, ef = M.match(qd, td, p, qk, tk)
        assert f.shape == ef.shape and (f == ef).all() and m.tobytes() == em.tobytes(), name
        if name.startswith("noise"):   # the smooth synthetic scene has a corner or two; the noise scene fills the lists
            assert len(qk) > 300 and len(em) > 100, name
        # and through the convenience path: OrbFeatures.detect(raw=True) outputs as they come
        (k0, d0), (k1, d1) = orb.detect(*ts, raw=True)
        m2 = matcher.match((k0, d0, None), (k1, d1, None), mp(p))
        assert m2.tobytes() == em.tobytes(), name
    orb.close()
    matcher.close()


def test_repeats_and_shared_matcher(matcher1000):
    """Two calls give identical bytes; one matcher used for sets of different sizes in sequence (no stale partials or column minima)."""
    rng = np.random.default_rng(11)
    big, small = related_sets(rng, 900, 1000), related_sets(rng, 70, 130)
    a = matcher1000.match((None, big[0], None), (None, big[1], None), want_forward=True)
    b = matcher1000.match((None, big[0], None), (None, big[1], None), want_forward=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for qd, td in (small, big, (small[0], big[1]), (big[0], small[1]), small):
        check(matcher1000, qd, td, M.params(ratio=0))


def test_bad_arguments():
    torch = _torch()
    from cartslam import EngineError, OrbMatcher
    eng = engine()
    for n in (0, -1, 65537):
        with pytest.raises(EngineError):
            OrbMatcher(eng, n)
    matcher = OrbMatcher(eng, 64)
    d = rand_desc(np.random.default_rng(1), 10)
    k = rand_kps(np.random.default_rng(1), 10)
    for bad in (dict(ratio=101), dict(ratio=-1), dict(max_distance=257), dict(max_distance=-1), dict(use_gate=2), dict(cross_check=2)):
        with pytest.raises(EngineError):
            matcher.match((k, d, None), (k, d, None), mp(M.params(**bad)))
    with pytest.raises(EngineError):
        matcher.match((None, d, None), (k, d, None), mp(M.params(use_gate=1)))     # a gate without keypoints
    with pytest.raises(EngineError):
        matcher.match((None, d, 11), (None, d, None))                              # count above the rows
    with pytest.raises(EngineError):
        matcher.match((None, d[:, :31], None), (None, d, None))
    with pytest.raises(EngineError):                                               # a device count needs full-capacity buffers
        matcher.match((None, d, torch.tensor([5], dtype=torch.int32, device="cuda")), (None, d, None))
    # the C ABI itself: descriptor steps below 32
    t = torch.zeros((64, 32), dtype=torch.uint8, device="cuda")
    c = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    p = mp(M.params())
    vp = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    for qs, ts in ((31, 32), (32, 0)):
        assert matcher._lib.cart_matcher_match(matcher._h, C.byref(p), vp(t), qs, None, vp(c), vp(t), ts, None, vp(c), vp(out), vp(c), None, None) != 0
    assert len(matcher.match((k, d, None), (k, d, None), mp(M.params(ratio=0)))) == 10   # still usable
    matcher.close()


# ---- lifecycle (as tests/test_gpu_device_objects.py for the other objects) -------------------------------------------------
def test_lifecycle_and_streams():
    torch = _torch()
    from cartslam import Engine, EngineError, OrbMatcher
    eng = engine()
    rng = np.random.default_rng(12)
    sets = [related_sets(rng, 300, 260), related_sets(rng, 120, 333)]
    dev = [tuple(torch.from_numpy(d).cuda() for d in s) for s in sets]

    def call(matcher, s):
        """cart_matcher_match on the current stream without the download OrbMatcher.match ends with."""
        qd, td = dev[s]
        out = torch.zeros((matcher.max_features, 4), dtype=torch.int32, device="cuda")
        n = torch.zeros(1, dtype=torch.int32, device="cuda")
        cq, ct = (torch.tensor([len(d)], dtype=torch.int32, device="cuda") for d in (qd, td))
        p = mp(M.params(ratio=0))
        vp = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        matcher._check(matcher._lib.cart_matcher_match(matcher._h, C.byref(p), vp(qd), 32, None, vp(cq), vp(td), 32, None, vp(ct), vp(out), vp(n), None,
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "cart_matcher_match")
        return [out, n, cq, ct]

    def run(streams):
        matcher = OrbMatcher(eng, 400)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            o = call(matcher, 0)
        with torch.cuda.stream(streams[1]):
            o += call(matcher, 1)
        torch.cuda.synchronize()
        matcher.close()
        n0, n1 = int(o[1].item()), int(o[5].item())
        return o[0][:n0].cpu().numpy(), o[4][:n1].cpu().numpy()

    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    same, two = run((a, a)), run((a, b))
    for s, (x, y) in enumerate(zip(same, two)):
        assert x.tobytes() == y.tobytes() and x.tobytes() == M.match(*sets[s], M.params(ratio=0))[0].tobytes()
    # close, double close, use after close
    matcher = OrbMatcher(eng, 400)
    assert len(matcher.match((None, sets[0][0], None), (None, sets[0][1], None))) > 0
    matcher.close()
    matcher.close()
    with pytest.raises(EngineError):
        matcher.match((None, sets[0][0], None), (None, sets[0][1], None))
    # closed after its engine
    other = Engine(64, 32, num_disparities=0, paths=0)
    matcher = OrbMatcher(other, 400)
    call(matcher, 0)
    other.close()
    matcher.close()

    def cycle(n):
        for _ in range(n):
            o = OrbMatcher(eng, 5000)
            call(o, 0)
            o.close()
        torch.cuda.synchronize()
    cycle(3)
    free0 = torch.cuda.mem_get_info()[0]
    cycle(20)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"matcher leak: {(free0 - free1) >> 20} MiB over 20 create/use/close cycles"


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------
def _dumped(d, fid, which):
    return np.fromfile(os.path.join(d, f"{fid}_feature_matches_{which}.bin"), M.MATCH_DTYPE)


def test_matches_module_frame_loop(tmp_path):
    import json
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n = 3
    world = noise_world(79)
    frames = [noise_frame(world, f) for f in range(n)]   # 320 x 96; the layout of test_host.make_dataset with a scene full of corners
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for cam in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, cam))
    for f, (l, r) in enumerate(frames):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    feats = [(N.orb(l, 5000), N.orb(r, 5000)) for l, r in frames]   # ((kp, desc) left, (kp, desc) right) per frame, restated once
    stereo = [M.match(fl[1], fr[1], M.stereo_params(), fl[0], fr[0])[0] for fl, fr in feats]
    temporal = [np.zeros(0, M.MATCH_DTYPE)] + [M.match(feats[f][0][1], feats[f - 1][0][1], M.temporal_params(), feats[f][0][0], feats[f - 1][0][0])[0]
                                               for f in range(1, n)]
    assert min(len(s) for s in stereo) > 100 and min(len(t) for t in temporal[1:]) > 100
    narrow = dict(max_disparity=40, max_dy=1, search_radius=6, ratio=90, max_distance=50, cross_check=False)
    lists = {"both": [{"type": "orb_features"}, {"type": "orb_matches"}],
             "no_temporal": [{"type": "orb_features"}, {"type": "orb_matches", "temporal": False}],
             "with_disparity_and_keys": [{"type": "disparity", "num_disparities": 128, "smoothing_radius": 2, "smoothing_iterations": 1},
                                         {"type": "orb_features"}, dict(narrow, type="orb_matches")]}
    for name, mods in lists.items():
        d = os.path.join(tmp, "dump_" + name)
        os.makedirs(d)
        r = run_exe(src, mods, tmp, ("--dump", d))
        assert r.returncode == 0, r.stderr
        for fid in range(1, n + 1):
            es, et = stereo[fid - 1], temporal[fid - 1]
            if name == "with_disparity_and_keys":
                p = dict(max_distance=50, ratio=90, cross_check=0)
                fl, fr = feats[fid - 1]
                es = M.match(fl[1], fr[1], M.stereo_params(40, 1, **p), fl[0], fr[0])[0]
                if fid > 1:
                    et = M.match(fl[1], feats[fid - 2][0][1], M.temporal_params(6, **p), fl[0], feats[fid - 2][0][0])[0]
            if name == "no_temporal":
                et = et[:0]
            assert _dumped(d, fid, "stereo").tobytes() == es.tobytes(), f"{name} frame {fid}: stereo"
            assert _dumped(d, fid, "temporal").tobytes() == et.tobytes(), f"{name} frame {fid}: temporal"
        assert os.path.getsize(os.path.join(d, "1_feature_matches_temporal.bin")) == 0
        kp = np.fromfile(os.path.join(d, "2_features_left_keypoints.bin"), N.KEYPOINT_DTYPE)      # the features dump is unchanged
        assert kp.tobytes() == feats[1][0][0].tobytes()
    r = run_exe(src, [{"type": "orb_matches"}], tmp)
    assert r.returncode != 0 and 'requires "features"' in r.stderr
    r = run_exe(src, [{"type": "orb_features"}, {"type": "orb_matches", "ratio": 101}], tmp)
    assert r.returncode != 0 and "ratio" in r.stderr

"""GPU tests of the stereo visual odometry stage (spec S23): the landmarks, every field of the result, the inlier
mask and the per-hypothesis table of cart_ego_triangulate / cart_ego_estimate equal the numpy restatement (tests/np_ego.py) bit
for bit, and the "ego_motion" module through the C++ frame loop equals the restatement fed with the restated features and matches.

The kernels as built: ego_score has 64 hypotheses per workgroup and tiles of 256 correspondences; ego_compact handles 1024
temporal matches per round; ego_refine is one workgroup of 256 threads = the 256 virtual lanes of the S23 sums."""
import ctypes as C
import os

import numpy as np
import pytest

import np_ego as E
import np_match as M
import np_orb as N

pytestmark = pytest.mark.gpu

CAM = E.camera(fx=300.0, fy=300.0, cx=160.0, cy=48.0, baseline=0.5)


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


def ep(p):
    from cartslam.engine import ego_params
    return ego_params(**p)


def cam_tuple(cam=CAM):
    return tuple(cam[k] for k in ("fx", "fy", "cx", "cy", "baseline"))


def make_ego(cap, cam=CAM):
    from cartslam import EgoMotion
    return EgoMotion(engine(), cam_tuple(cam), cap)


def rotation(axis, deg):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def matches(q, t):
    m = np.zeros(len(q), E.MATCH_DTYPE)
    m["query"], m["train"] = q, t
    m["distance"], m["second"] = 10, 40
    return m


def frames(seed, nk, usable="all", outliers=0.3, n_pts=None):
    """A rigid scene seen from two poses with quarter-pixel keypoints.  -> dict: kp of the four images (index = a permutation of
    the point id, different per frame), the stereo match lists of both frames and `nk` temporal matches of which a fraction
    `outliers` pairs a point with a wrong one.  usable: "all" = every point has a stereo match in both frames, "half" = every
    second point of the current frame has none, "none" = the previous frame has none at all."""
    rng = np.random.default_rng(seed)
    n = n_pts or max(nk, 8)
    Z = rng.uniform(4, 30, n)
    P = np.stack([rng.uniform(-0.45, 0.45, n) * Z, rng.uniform(-0.12, 0.12, n) * Z, Z], 1)
    R, t = rotation(rng.normal(size=3), 2.0), rng.normal(size=3) * 0.35
    Q = P @ R.T + t
    out = {}
    for name, X in (("prev", P), ("cur", Q)):
        perm_l, perm_r = rng.permutation(n), rng.permutation(n)     # keypoint index of point id, left and right
        kl, kr = np.zeros(n, E.KEYPOINT_DTYPE), np.zeros(n, E.KEYPOINT_DTYPE)
        u, v = CAM["fx"] * X[:, 0] / X[:, 2] + CAM["cx"], CAM["fy"] * X[:, 1] / X[:, 2] + CAM["cy"]
        d = CAM["fx"] * CAM["baseline"] / X[:, 2]
        kl["x"][perm_l], kl["y"][perm_l] = np.round(u * 4) / 4, np.round(v * 4) / 4
        kr["x"][perm_r], kr["y"][perm_r] = np.round((u - d) * 4) / 4, np.round(v * 4) / 4
        ids = np.arange(n)
        if name == "cur" and usable == "half":
            ids = ids[::2]
        if name == "prev" and usable == "none":
            ids = ids[:0]
        order = np.argsort(perm_l[ids], kind="stable")               # ascending query, as the matcher writes
        out[name] = dict(kl=kl, kr=kr, stereo=matches(perm_l[ids][order], perm_r[ids][order]), perm_l=perm_l)
    ids = rng.choice(n, nk, replace=False)
    other = ids.copy()
    bad = rng.random(nk) < outliers
    other[bad] = rng.integers(0, n, int(bad.sum()))
    order = np.argsort(out["cur"]["perm_l"][ids], kind="stable")
    out["temporal"] = matches(out["cur"]["perm_l"][ids][order], out["prev"]["perm_l"][other][order])
    return out


def check(ego, cur_lm, cur_kp, prev_lm, temporal, p, seed=0, frame_id=0, cam=CAM):
    """One estimate call against the restatement: result, mask and hypothesis table, bit for bit."""
    res, mask = ego.estimate(cur_lm, cur_kp, prev_lm, temporal, seed=seed, frame_id=frame_id, params=ep(p), want_mask=True)
    table = ego.debug_hypotheses()
    eres, emask, etable = E.estimate(cam, p, cur_lm, cur_kp, prev_lm, temporal, seed, frame_id, capacity=ego.max_features)
    assert table.tobytes() == etable.tobytes(), f"hypothesis table differs at {np.nonzero(table != etable)[0][:8]}"
    for f in E.RESULT_DTYPE.names:
        assert res[f].tobytes() == eres[f].tobytes(), f"result field {f}: {res[f]} != {eres[f]}"
    assert res.tobytes() == eres.tobytes()
    assert mask.dtype == np.int32 and mask.shape == emask.shape and (mask == emask).all(), "inlier mask differs"
    return eres, emask, etable


def check_frames(ego, fr, p, seed=0, frame_id=0):
    lm = {}
    for name in ("prev", "cur"):
        f = fr[name]
        lm[name] = ego.triangulate(f["kl"], f["kr"], f["stereo"], params=ep(p))
        exp = E.triangulate(CAM, f["kl"], f["kr"], f["stereo"], p)
        assert lm[name].tobytes() == exp.tobytes(), f"{name} landmarks differ"
    return check(ego, lm["cur"], fr["cur"]["kl"], lm["prev"], fr["temporal"], p, seed, frame_id)


@pytest.fixture(scope="module")
def ego1000():
    g = make_ego(1000)
    yield g
    g.close()


@pytest.fixture(scope="module")
def ego5000():
    g = make_ego(5000)
    yield g
    g.close()


@pytest.mark.parametrize("nk", [0, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("usable", ["all", "half", "none"])
def test_counts_and_usable_fractions(ego1000, nk, usable):
    res, mask, table = check_frames(ego1000, frames(1000 + nk, nk, usable), E.params(hypotheses=64), seed=nk, frame_id=3)
    n = int(res["n_correspondences"][0])
    assert n == (nk if usable == "all" else 0 if usable == "none" else n) and (usable != "half" or nk < 4 or 0 < n < nk)
    assert int(res["status"][0]) == (1 if n >= 4 else int(res["status"][0]))
    if n >= 63:
        assert int(res["n_inliers"][0]) > n // 2 and float(res["rms"][0]) < 1.0 and mask.sum() == int(res["n_inliers"][0])
    if n < 3:
        assert int(res["status"][0]) == 0 and table["skipped"].all()


@pytest.mark.parametrize("hyp", [1, 64, 65, 256])
@pytest.mark.parametrize("it", [0, 1, 4])
def test_hypotheses_and_refine_iterations(ego1000, hyp, it):
    res, _, table = check_frames(ego1000, frames(7, 300), E.params(hypotheses=hyp, refine_iterations=it), seed=5, frame_id=hyp)
    assert len(table) == hyp and (hyp == 1 or int(res["status"][0]) == 1)


def test_capacity_5000_with_small_counts(ego5000):
    for nk in (5, 70, 300):
        res, _, _ = check_frames(ego5000, frames(20 + nk, nk), E.params())
        assert int(res["status"][0]) == 1


def test_full_size_5000(ego5000):
    res, mask, _ = check_frames(ego5000, frames(31, 5000), E.params(), seed=9, frame_id=77)
    assert int(res["n_correspondences"][0]) == 5000 and int(res["n_inliers"][0]) > 3000 and int(res["status"][0]) == 1


def test_non_default_parameters(ego1000):
    fr = frames(41, 400)
    base = check_frames(ego1000, fr, E.params())[0]
    seen = {base.tobytes()}
    for p, seed, fid in ((E.params(inlier_threshold=0.75), 0, 0), (E.params(min_disparity=8.25), 0, 0), (E.params(), 123456789012345, 0),
                         (E.params(), 0, 4000000000123), (E.params(inlier_threshold=5.5, min_disparity=4.0, hypotheses=100, refine_iterations=16), 3, 4)):
        res = check_frames(ego1000, fr, p, seed, fid)[0]
        assert int(res["status"][0]) == 1
        seen.add(res.tobytes())
    assert len(seen) == 6, "a parameter changed nothing"


def test_triangulation_rejects_small_and_nan_disparities(ego1000):
    rng = np.random.default_rng(51)
    n = 300
    kl, kr = np.zeros(n, E.KEYPOINT_DTYPE), np.zeros(n, E.KEYPOINT_DTYPE)
    kl["x"], kl["y"] = rng.integers(0, 1280, n) / 4, rng.integers(0, 384, n) / 4
    q = np.union1d(rng.choice(n, 200, replace=False), [5, 9, 12])                 # ascending and distinct, as the matcher writes
    st = matches(q, rng.permutation(n)[:len(q)])
    disp = rng.integers(-8, 40, len(q)) / 4                                        # -2 .. 9.75 in quarter pixels
    disp[20:26] = [1.0, 0.75, 2.5, 2.25, 1.25, 2.75]                               # on, just below and just above both thresholds
    kr["x"][st["train"]], kr["y"][st["train"]] = kl["x"][q] - disp, kl["y"][q]
    kl["x"][5], kr["x"][st["train"][q == 9]], kl["y"][12] = np.nan, np.nan, 17.25
    for md in (1.0, 2.5):
        got = ego1000.triangulate(kl, kr, st, params=ep(E.params(min_disparity=md)))
        exp = E.triangulate(CAM, kl, kr, st, E.params(min_disparity=md))
        assert got.tobytes() == exp.tobytes()
        d = kl["x"][st["query"]].astype(np.float64) - kr["x"][st["train"]].astype(np.float64)
        assert (d == md).any() and (d < md).any() and (exp[st["query"][d == md], 3] == 1).all() and (exp[st["query"][d < md], 3] == 0).all()
        assert (exp[[5, 9], 3] == 0).all() and 50 < exp[:, 3].sum() < len(q) - 10
    # matches with indices outside the sets are ignored, a device count below the rows hides the tail
    st2 = np.concatenate([st[:50], matches([-1, n, 3, 4], [0, 0, -1, 1000])])
    got = ego1000.triangulate(kl, kr, st2, left_count=n)
    assert got.tobytes() == E.triangulate(CAM, kl, kr, st2, capacity=1000).tobytes()
    got = ego1000.triangulate(kl, kr, st, left_count=100, stereo_count=60)
    assert got.shape == (100, 4) and got.tobytes() == E.triangulate(CAM, kl[:100], kr, st[:60], capacity=1000).tobytes()


def landmarks(P):
    return np.concatenate([np.asarray(P, np.float64), np.ones((len(P), 1))], 1)


def project(P):
    k = np.zeros(len(P), E.KEYPOINT_DTYPE)
    with np.errstate(all="ignore"):
        k["x"], k["y"] = CAM["fx"] * P[:, 0] / P[:, 2] + CAM["cx"], CAM["fy"] * P[:, 1] / P[:, 2] + CAM["cy"]
    return k


def test_degenerate_samples_are_skipped(ego1000):
    rng = np.random.default_rng(61)
    n = 200
    ident = matches(np.arange(n), np.arange(n))
    # all points on one line: every hypothesis is skipped, status 0
    s = rng.uniform(0, 10, n)
    line = np.stack([0.3 * s - 1, 0.1 * s, 5 + s], 1)
    res, _, table = check(ego1000, landmarks(line + [0.1, 0, 0.2]), project(line + [0.1, 0, 0.2]), landmarks(line), ident, E.params(hypotheses=64))
    assert table["skipped"].all() and int(res["status"][0]) == 0 and int(res["n_correspondences"][0]) == n
    # all points coincident
    dot = np.tile([[1.0, 0.5, 9.0]], (n, 1))
    res, _, table = check(ego1000, landmarks(dot), project(dot), landmarks(dot), ident, E.params(hypotheses=64))
    assert table["skipped"].all() and int(res["status"][0]) == 0
    # 70 % of the points are copies of one point, the rest are in general position: some hypotheses are skipped, a pose is found
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1, 1, n), rng.uniform(5, 20, n)], 1)
    P[rng.random(n) < 0.7] = P[0]
    Q = P @ rotation([0.2, 1, 0.1], 1.5).T + [0.2, -0.05, 0.3]
    res, _, table = check(ego1000, landmarks(Q), project(Q), landmarks(P), ident, E.params())
    assert 0 < table["skipped"].sum() < len(table) and int(res["status"][0]) == 1 and int(res["n_inliers"][0]) == n


def test_points_behind_the_camera(ego1000):
    rng = np.random.default_rng(62)
    n = 300
    P = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0.5, 6, n)], 1)
    Q = P @ rotation([0, 1, 0], 3.0).T + [0.1, 0.0, -2.0]            # a third of the points end up behind the camera
    kp = project(np.where(Q[:, 2:3] > 0, Q, [0.0, 0.0, 1.0]))
    res, mask, _ = check(ego1000, landmarks(Q), kp, landmarks(P), matches(np.arange(n), np.arange(n)), E.params())
    behind = Q[:, 2] <= 0
    assert 50 < behind.sum() < 200 and int(res["status"][0]) == 1 and not mask[:n][behind].any() and mask[:n][~behind].all()


def test_refinement_stops_below_six_inliers(ego1000):
    fr = frames(63, 5, outliers=0)
    r4 = check_frames(ego1000, fr, E.params(refine_iterations=4), seed=2)[0]
    r0 = check_frames(ego1000, fr, E.params(refine_iterations=0), seed=2)[0]
    assert int(r4["status"][0]) == 1 and 3 <= int(r4["n_inliers"][0]) < 6 and r4.tobytes() == r0.tobytes()
    fr = frames(64, 6, outliers=0)     # six inliers: the step is taken
    r4 = check_frames(ego1000, fr, E.params(refine_iterations=4, inlier_threshold=4.0), seed=2)[0]
    r0 = check_frames(ego1000, fr, E.params(refine_iterations=0, inlier_threshold=4.0), seed=2)[0]
    assert int(r0["n_inliers"][0]) == 6 and r4["R"].tobytes() != r0["R"].tobytes()


def test_repeats_and_shared_object(ego1000):
    """Two calls give identical bytes; one object used for lists of different sizes in sequence (no stale table or list entries)."""
    big, small = frames(71, 900), frames(72, 40)
    a = check_frames(ego1000, big, E.params())
    b = check_frames(ego1000, big, E.params())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for fr, p in ((small, E.params(hypotheses=7)), (big, E.params(hypotheses=300)), (small, E.params())):
        check_frames(ego1000, fr, p)


# ---- inputs straight from cart_orb_detect and cart_matcher_match -----------------------------------------------------------
def _match_raw(matcher, q, t, p):
    """cart_matcher_match on the current stream into full-capacity buffers, with no host synchronisation."""
    torch = _torch()
    from cartslam.engine import match_params
    out = torch.zeros((matcher.max_features, 4), dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    mp = match_params(**p)
    vp = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    matcher._check(matcher._lib.cart_matcher_match(matcher._h, C.byref(mp), vp(q[1]), 32, vp(q[0]), vp(q[2]), vp(t[1]), 32, vp(t[0]), vp(t[2]), vp(out), vp(n),
                                                   None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "cart_matcher_match")
    return out, n


def restated_frames(images, nf):
    """Per frame: ((kp, desc) left, (kp, desc) right), stereo matches, temporal matches, from the restatements of S20 and S22."""
    feats = [(N.orb(l, nf), N.orb(r, nf)) for l, r in images]
    stereo = [M.match(fl[1], fr[1], M.stereo_params(), fl[0], fr[0])[0] for fl, fr in feats]
    temporal = [np.zeros(0, M.MATCH_DTYPE)] + [M.match(feats[f][0][1], feats[f - 1][0][1], M.temporal_params(), feats[f][0][0], feats[f - 1][0][0])[0]
                                               for f in range(1, len(images))]
    return feats, stereo, temporal


def test_inputs_from_detect_and_match_without_a_host_round_trip():
    torch = _torch()
    from cartslam import OrbFeatures, OrbMatcher
    from test_gpu_matches import _detect_raw, noise_frame, noise_world
    w, h, nf = 320, 96, 1000
    images = [noise_frame(noise_world(78), f) for f in range(2)]
    orb, matcher, ego = OrbFeatures(engine(), w, h, nfeatures=nf), OrbMatcher(engine(), nf), make_ego(nf)
    dev = [[torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in pair] for pair in images]
    torch.cuda.synchronize()
    sides = [_detect_raw(orb, pair) for pair in dev]                       # queued ...
    lms = []
    for left, right in sides:                                              # ... and consumed on the same stream, every count read on the device
        st, ns = _match_raw(matcher, left, right, M.stereo_params())
        lms.append(ego.triangulate(left[0], right[0], st, left_count=left[2], stereo_count=ns, raw=True))
    tm, nt = _match_raw(matcher, sides[1][0], sides[0][0], M.temporal_params())
    res, mask = ego.estimate(lms[1], sides[1][0][0], lms[0], tm, temporal_count=nt, seed=4, frame_id=2, want_mask=True, raw=True)
    table = ego.debug_hypotheses()
    feats, stereo, temporal = restated_frames(images, nf)
    elm = [E.triangulate(CAM, feats[f][0][0], feats[f][1][0], stereo[f]) for f in range(2)]
    for f in range(2):
        assert lms[f][:len(elm[f])].cpu().numpy().tobytes() == elm[f].tobytes(), f"frame {f} landmarks"
    eres, emask, etable = E.estimate(CAM, E.params(), elm[1], feats[1][0][0], elm[0], temporal[1], 4, 2, capacity=nf)
    assert len(temporal[1]) > 100 and int(eres["status"][0]) == 1 and int(eres["n_inliers"][0]) > 50
    assert res.cpu().numpy().tobytes() == eres.tobytes() and (mask.cpu().numpy() == emask).all() and table.tobytes() == etable.tobytes()
    for o in (orb, matcher, ego):
        o.close()


def test_bad_arguments():
    torch = _torch()
    from cartslam import EgoMotion, EngineError
    eng = engine()
    for n in (0, -1, 65537):
        with pytest.raises(EngineError):
            EgoMotion(eng, cam_tuple(), n)
    ego = make_ego(64)
    fr = frames(81, 20)
    lm = E.triangulate(CAM, fr["cur"]["kl"], fr["cur"]["kr"], fr["cur"]["stereo"])
    for bad in (dict(hypotheses=0), dict(hypotheses=1025), dict(refine_iterations=-1), dict(refine_iterations=17), dict(inlier_threshold=0.0),
                dict(inlier_threshold=float("nan")), dict(min_disparity=0.0), dict(min_disparity=-1.0)):
        with pytest.raises(EngineError, match=next(iter(bad))):
            ego.estimate(lm, fr["cur"]["kl"], lm, fr["temporal"], params=ep(E.params(**bad)))
        with pytest.raises(EngineError, match=next(iter(bad))):
            ego.triangulate(fr["cur"]["kl"], fr["cur"]["kr"], fr["cur"]["stereo"], params=ep(E.params(**bad)))
    for k, v in (("fx", 0.0), ("fy", -1.0), ("baseline", 0.0), ("cx", float("inf")), ("cy", float("nan")), ("fx", float("nan"))):
        bad_ego = EgoMotion(eng, cam_tuple(dict(CAM, **{k: v})), 64)
        with pytest.raises(EngineError, match=k):
            bad_ego.triangulate(fr["cur"]["kl"], fr["cur"]["kr"], fr["cur"]["stereo"])
        bad_ego.close()
    with pytest.raises(EngineError):
        ego.triangulate(np.zeros(65, E.KEYPOINT_DTYPE), fr["cur"]["kr"], fr["cur"]["stereo"])   # more rows than the capacity
    with pytest.raises(EngineError):
        ego.debug_hypotheses()                                                                  # no estimate call yet
    # the C ABI itself: NULL and misaligned pointers are refused before any device call
    buf = torch.zeros(64 * 8, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    p, cam = ep(E.params()), ego.camera
    vp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)   # noqa: E731
    lib = ego._lib
    assert lib.cart_ego_triangulate(ego._h, C.byref(cam), C.byref(p), vp(buf), vp(buf), vp(cnt), vp(buf), vp(cnt), None, None) != 0
    assert lib.cart_ego_triangulate(ego._h, C.byref(cam), C.byref(p), vp(buf), vp(buf), vp(cnt), vp(buf), vp(cnt), vp(buf, 4), None) != 0
    assert lib.cart_ego_triangulate(ego._h, None, C.byref(p), vp(buf), vp(buf), vp(cnt), vp(buf), vp(cnt), vp(buf), None) != 0
    assert lib.cart_ego_estimate(ego._h, C.byref(cam), C.byref(p), vp(buf), vp(buf), vp(buf), vp(buf), vp(cnt), 0, 0, None, None, None) != 0
    assert lib.cart_ego_estimate(ego._h, C.byref(cam), C.byref(p), vp(buf), vp(buf), vp(buf), vp(buf), vp(cnt), 0, 0, vp(buf, 4), None, None) != 0
    assert lib.cart_ego_estimate(ego._h, C.byref(cam), C.byref(p), vp(buf), vp(buf), vp(buf), vp(buf), vp(cnt, 2), 0, 0, vp(buf), None, None) != 0
    assert int(ego.estimate(lm, fr["cur"]["kl"], lm, fr["temporal"])["n_correspondences"][0]) == 20   # still usable
    ego.close()


# ---- lifecycle (as tests/test_gpu_matches.py::test_lifecycle_and_streams for the matcher) ----------------------------------
def test_lifecycle_and_streams():
    torch = _torch()
    from cartslam import Engine, EngineError
    eng = engine()
    cases = [frames(91, 300), frames(92, 120)]
    lms = [[E.triangulate(CAM, fr[n]["kl"], fr[n]["kr"], fr[n]["stereo"]) for n in ("cur", "prev")] for fr in cases]
    expect = [E.estimate(CAM, E.params(), lms[s][0], cases[s]["cur"]["kl"], lms[s][1], cases[s]["temporal"], 1, s, capacity=400)[0] for s in range(2)]

    def call(ego, s):
        """triangulate + estimate on the current stream without the downloads."""
        fr = cases[s]
        lm = [ego.triangulate(fr[n]["kl"], fr[n]["kr"], fr[n]["stereo"], raw=True) for n in ("cur", "prev")]
        return ego.estimate(lm[0], fr["cur"]["kl"], lm[1], fr["temporal"], seed=1, frame_id=s, raw=True)

    def run(streams):
        ego = make_ego(400)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            a = call(ego, 0)
        with torch.cuda.stream(streams[1]):
            b = call(ego, 1)
        torch.cuda.synchronize()
        ego.close()
        return a.cpu().numpy().tobytes(), b.cpu().numpy().tobytes()

    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    same, two = run((a, a)), run((a, b))
    for s in range(2):
        assert same[s] == two[s] == expect[s].tobytes()
    # close, double close, use after close
    ego = make_ego(400)
    call(ego, 0)
    ego.close()
    ego.close()
    with pytest.raises(EngineError):
        call(ego, 0)
    # closed after its engine
    from cartslam import EgoMotion
    other = Engine(64, 32, num_disparities=0, paths=0)
    ego = EgoMotion(other, cam_tuple(), 400)
    call(ego, 0)
    other.close()
    ego.close()

    def cycle(n):
        for _ in range(n):
            o = make_ego(5000)
            o.estimate(lms[0][0], cases[0]["cur"]["kl"], lms[0][1], cases[0]["temporal"], raw=True)
            o.close()
        torch.cuda.synchronize()
    cycle(3)
    free0 = torch.cuda.mem_get_info()[0]
    cycle(20)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"ego leak: {(free0 - free1) >> 20} MiB over 20 create/use/close cycles"


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------
# the restated t of frames 2 and 3 of the noise scene against the true (-0.25, -1/12, 0): worst component error 0.0342 m (frame 3, both
# parameter sets; whole-pixel keypoints of a plane 25 m away, where one pixel is 8 cm); the bound is twice that
FRAME_T_BOUND = 0.0683


def test_ego_motion_module_frame_loop(tmp_path):
    import json
    from test_gpu_matches import noise_frame, noise_world
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n = 3
    world = noise_world(79)
    images = [noise_frame(world, f) for f in range(n)]
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for cam in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, cam))
    for f, (l, r) in enumerate(images):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    feats, stereo, temporal = restated_frames(images, 5000)
    lms = [E.triangulate(CAM, feats[f][0][0], feats[f][1][0], stereo[f]) for f in range(n)]
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    runs = {"defaults": (dict(keys), E.params(), 0),
            "keys": (dict(keys, seed=11, hypotheses=64, refine_iterations=2, inlier_threshold=1.5, min_disparity=2.0),
                     E.params(hypotheses=64, refine_iterations=2, inlier_threshold=1.5, min_disparity=2.0), 11)}
    for name, (cfg, p, seed) in runs.items():
        d = os.path.join(tmp, "dump_" + name)
        os.makedirs(d)
        r = run_exe(src, [{"type": "orb_features"}, {"type": "orb_matches"}, dict(cfg, type="ego_motion")], tmp, ("--dump", d))
        assert r.returncode == 0, r.stderr
        lm = lms if p["min_disparity"] == 1.0 else [E.triangulate(CAM, feats[f][0][0], feats[f][1][0], stereo[f], p) for f in range(n)]
        pose = list(E.POSE_IDENTITY)
        for fid in range(1, n + 1):
            if fid == 1:
                res = E.estimate(CAM, p, lm[0], feats[0][0][0], lm[0], temporal[0], seed, fid)[0]
            else:
                res = E.estimate(CAM, p, lm[fid - 1], feats[fid - 1][0][0], lm[fid - 2], temporal[fid - 1], seed, fid)[0]
            pose = E.chain(pose, res)
            got = open(os.path.join(d, f"{fid}_ego_motion.bin"), "rb").read()
            assert len(got) == 120 + 96
            assert got[:120] == res.tobytes(), f"{name} frame {fid}: result {np.frombuffer(got[:120], E.RESULT_DTYPE)} != {res}"
            assert got[120:] == np.array(pose, np.float64).tobytes(), f"{name} frame {fid}: pose"
            if fid == 1:
                assert int(res["status"][0]) == 0 and tuple(res["R"][0]) == E.IDENTITY and not res["t"][0].any() and pose == E.POSE_IDENTITY
            else:
                assert int(res["status"][0]) == 1
                err = np.abs(res["t"][0] - [-0.25, -1.0 / 12.0, 0.0]).max()
                print(f"{name} frame {fid}: t = {res['t'][0]}, worst component error {err:.5f} m, inliers {int(res['n_inliers'][0])}")
                assert err < FRAME_T_BOUND
            # the dumps of the modules before it are what they are without it
            for which, exp in (("stereo", stereo[fid - 1]), ("temporal", temporal[fid - 1])):
                assert np.fromfile(os.path.join(d, f"{fid}_feature_matches_{which}.bin"), M.MATCH_DTYPE).tobytes() == exp.tobytes()
            assert np.fromfile(os.path.join(d, f"{fid}_features_left_keypoints.bin"), N.KEYPOINT_DTYPE).tobytes() == feats[fid - 1][0][0].tobytes()
    r = run_exe(src, [{"type": "orb_features"}, dict(keys, type="ego_motion")], tmp)
    assert r.returncode != 0 and 'requires "feature_matches"' in r.stderr
    r = run_exe(src, [{"type": "orb_features"}, {"type": "orb_matches"}, {"type": "ego_motion"}], tmp)
    assert r.returncode != 0 and "fx" in r.stderr
    r = run_exe(src, [{"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion", hypotheses=0)], tmp)
    assert r.returncode != 0 and "hypotheses" in r.stderr

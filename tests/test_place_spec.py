"""CPU tests of spec S27, place recognition over a ring of stored ORB frames: the numpy restatement tests/np_place.py
against a plain double loop and hand-worked cases (the vote rule's edges, eligibility, the ring, the candidate order), and the library's
host-side checks (no GPU: what is checked before the object).  The checks that need an object (pointers, alignment, overlap) are in
tests/test_gpu_place.py, which also runs the cases built here on the device."""
import ctypes as C

import numpy as np
import pytest

import np_place as P


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32)).astype(np.uint8)


def flip_bits(rng, d, k):
    """d [32] with k distinct random bits inverted: Hamming distance k from d."""
    o = d.copy()
    for b in rng.choice(256, k, replace=False):
        o[b // 8] ^= 1 << (b % 8)
    return o


def loop_score(qd, td, p):
    """The score of one stored set in plain loops over bits of Python ints."""
    score = 0
    for q in qd:
        keys = sorted((bin(int.from_bytes(bytes(q), "little") ^ int.from_bytes(bytes(t), "little")).count("1"), j) for j, t in enumerate(td))
        if not keys:
            continue
        d1 = keys[0][0]
        d2 = keys[1][0] if len(keys) > 1 else -1
        if d1 <= p["max_distance"] and (p["ratio"] == 0 or d2 < 0 or 100 * d1 < p["ratio"] * d2):
            score += 1
    return score


def stored_frames(rng, base, specs, noise=20):
    """One stored set per spec = [(rows of base copied, bits flipped in each)], followed by `noise` unrelated rows."""
    out = []
    for spec in specs:
        rows = [flip_bits(rng, base[i], k) for n, k in spec for i in rng.choice(len(base), n, replace=False)]
        out.append(np.array(rows + list(rand_desc(rng, noise)), np.uint8).reshape(-1, 32))
    return out


def test_restatement_equals_the_double_loop():
    rng = np.random.default_rng(27)
    base = rand_desc(rng, 60)
    sets = stored_frames(rng, base, [[(30, 10)], [(20, 60), (10, 70)], [(5, 0)], []], noise=7)
    for p in (P.params(), P.params(ratio=0), P.params(max_distance=61, ratio=95), P.params(max_distance=256, ratio=100)):
        ring = P.Ring(100, 4)
        for f, s in enumerate(sets):
            ring.insert(s, f)
        got = ring.scores(base, 1000, p)
        assert got.tolist() == [loop_score(base, s, p) for s in sets]
    assert len(set(P.Ring(100, 4).scores(base, 0, P.params()).tolist())) == 1   # nothing stored: all -1


def one_query_score(q, train, **fields):
    ring = P.Ring(16, 1)
    ring.insert(np.array(train, np.uint8).reshape(-1, 32), 0)
    return int(ring.scores(q.reshape(1, 32), 100, P.params(**fields))[0])


def test_vote_rule_edges():
    rng = np.random.default_rng(1)
    q = rand_desc(rng, 1)[0]
    # max_distance with one stored feature (d2 = -1: the ratio test does not apply)
    assert one_query_score(q, [flip_bits(rng, q, 64)]) == 1
    assert one_query_score(q, [flip_bits(rng, q, 65)]) == 0
    assert one_query_score(q, [flip_bits(rng, q, 65)], max_distance=65) == 1
    assert one_query_score(q, [flip_bits(rng, q, 0)], max_distance=0) == 1 and one_query_score(q, [flip_bits(rng, q, 1)], max_distance=0) == 0
    # the ratio test is strict: 100 * 40 = 80 * 50 does not vote, 100 * 39 < 80 * 50 does
    assert one_query_score(q, [flip_bits(rng, q, 40), flip_bits(rng, q, 50)]) == 0
    assert one_query_score(q, [flip_bits(rng, q, 50), flip_bits(rng, q, 39)]) == 1
    assert one_query_score(q, [flip_bits(rng, q, 40), flip_bits(rng, q, 50)], ratio=0) == 1
    assert one_query_score(q, [flip_bits(rng, q, 40), flip_bits(rng, q, 50)], ratio=81) == 1
    same = flip_bits(rng, q, 12)
    assert one_query_score(q, [same, same]) == 0 and one_query_score(q, [same, same], ratio=0) == 1      # d2 may equal d1
    assert one_query_score(q, [q, q], ratio=100) == 0 and one_query_score(q, [q, flip_bits(rng, q, 1)], ratio=1) == 1   # 0 < d2 only


def test_empty_slot_and_empty_query():
    rng = np.random.default_rng(2)
    ring = P.Ring(16, 3)
    ring.insert(np.zeros((0, 32), np.uint8), 7)
    ring.insert(rand_desc(rng, 5), 8, count=0)        # a count of 0 empties the set too
    q = rand_desc(rng, 4)
    scores, cand = ring.query(q, 100, P.params())
    assert scores.tolist() == [0, 0, -1] and len(cand) == 0
    scores, cand = ring.query(q, 100, P.params(min_score=0))
    assert cand.tolist() == [(0, 0, 7), (1, 0, 8)]
    scores, cand = ring.query(q[:0], 100, P.params(min_score=0))
    assert scores.tolist() == [0, 0, -1] and len(cand) == 2


def test_min_gap_and_the_uint64_wrap():
    rng = np.random.default_rng(3)
    d = rand_desc(rng, 3)
    ring = P.Ring(16, 4)
    for fid in (10, 11, (1 << 64) - 10, 0):
        ring.insert(d, fid)
    assert ring.scores(d, 60, P.params(ratio=0)).tolist() == [3, -1, -1, 3]             # 10 + 50 <= 60 exactly met, 11 + 50 one short
    assert ring.scores(d, 61, P.params(ratio=0)).tolist() == [3, 3, -1, 3]
    assert ring.scores(d, (1 << 64) - 1, P.params(ratio=0, min_gap=9)).tolist() == [3, 3, 3, 3]
    assert ring.scores(d, (1 << 64) - 1, P.params(ratio=0, min_gap=10)).tolist() == [3, 3, -1, 3]      # the sum wraps to 0: not eligible
    assert ring.scores(d, 5, P.params(ratio=0, min_gap=20)).tolist() == [-1, -1, -1, -1]    # every sum lies ahead of frame 5 or wraps
    assert ring.scores(d, 9, P.params(ratio=0, min_gap=(1 << 64) - 1)).tolist() == [-1, -1, -1, -1]   # 10 + (2^64 - 1) wraps to 9 <= 9
    assert ring.scores(d, (1 << 64) - 1, P.params(ratio=0, min_gap=(1 << 64) - 1)).tolist() == [-1, -1, -1, 3]
    assert ring.scores(d, 0, P.params(ratio=0, min_gap=0)).tolist() == [-1, -1, -1, 3]


def test_ring_overwrite():
    rng = np.random.default_rng(4)
    cap = 3
    sets = [rand_desc(rng, 4) for _ in range(cap + 2)]
    ring = P.Ring(16, cap)
    assert [ring.insert(s, 100 + f) for f, s in enumerate(sets)] == [0, 1, 2, 0, 1]
    assert [s["frame_id"] for s in ring.slots] == [103, 104, 102]
    for f, s in enumerate(sets):
        scores, cand = ring.query(s, 1000, P.params(ratio=0, max_distance=0, min_score=4))
        where = {3: 0, 4: 1, 2: 2}.get(f)          # sets 0 and 1 were replaced
        assert scores.tolist() == [4 if k == where else 0 for k in range(cap)]
        assert cand.tolist() == ([(where, 4, 100 + f)] if where is not None else [])
    ring.clear()
    assert ring.insert(sets[0], 5) == 0 and ring.scores(sets[0], 1000, P.params()).tolist() == [4, -1, -1]


def tie_case():
    """Five stored frames: slots 0 and 3 hold the same set (score 6) under frame ids 9 and 4, slots 1 and 4 the same set AND the same
    frame id (score 3), slot 2 scores 5.  -> (query, [(set, frame id)])."""
    rng = np.random.default_rng(5)
    q = rand_desc(rng, 8)
    six, three, five = q[:6].copy(), q[2:5].copy(), q[3:8].copy()
    return q, [(six, 9), (three, 6), (five, 7), (six, 4), (three, 6)]


def test_candidate_order_and_max_candidates():
    q, frames = tie_case()
    ring = P.Ring(16, 5)
    for s, fid in frames:
        ring.insert(s, fid)
    p = dict(ratio=0, max_distance=0, min_gap=0)
    scores, cand = ring.query(q, 100, P.params(min_score=1, max_candidates=16, **p))
    assert scores.tolist() == [6, 3, 5, 6, 3]
    assert cand.tolist() == [(3, 6, 4), (0, 6, 9), (2, 5, 7), (1, 3, 6), (4, 3, 6)]      # score desc, frame id asc, slot asc
    for m in (1, 2, 4, 5, 6):
        assert ring.query(q, 100, P.params(min_score=1, max_candidates=m, **p))[1].tolist() == cand.tolist()[:m]
    assert ring.query(q, 100, P.params(min_score=5, max_candidates=16, **p))[1].tolist() == cand.tolist()[:3]
    assert ring.query(q, 100, P.params(min_score=7, **p))[1].tolist() == []
    assert ring.query(q, 6, P.params(min_score=1, max_candidates=16, **p))[1].tolist() == [(3, 6, 4), (1, 3, 6), (4, 3, 6)]   # ids 7 and 9 lie ahead


# ---- the library's host side --------------------------------------------------------------------------------------------------
def lib_error(p=None, params_null=False):
    from cartslam import _lib, place_params
    lib = _lib.load()
    pp = place_params(**(p or {}))
    rc = lib.cart_place_query(None, None if params_null else C.byref(pp), None, 0, None, 0, None, None, None, None)
    assert rc != 0
    return lib.cart_last_error(None).decode()


def test_defaults_and_layout():
    from cartslam import PLACE_CANDIDATE_DTYPE, PlaceCandidate, PlaceParams, _lib, place_params
    assert C.sizeof(PlaceParams) == 24 and PlaceParams.min_gap.offset == 16
    assert C.sizeof(PlaceCandidate) == 16 == PLACE_CANDIDATE_DTYPE.itemsize and PLACE_CANDIDATE_DTYPE == P.CANDIDATE_DTYPE
    assert [(n, PLACE_CANDIDATE_DTYPE.fields[n][1]) for n in PLACE_CANDIDATE_DTYPE.names] == [(n, getattr(PlaceCandidate, n).offset) for n, _ in PlaceCandidate._fields_]
    p = place_params()
    assert {k: getattr(p, k) for k in P.DEFAULTS} == P.DEFAULTS
    assert place_params(min_gap=(1 << 64) - 1).min_gap == (1 << 64) - 1
    with pytest.raises(ValueError):
        place_params(cross_check=1)
    _lib.load().cart_place_default_params(None)   # a NULL pointer is ignored
    assert P.LOOP_DTYPE.itemsize == 336 and P.LOOP_DTYPE.fields["relative"][1] == 24 and P.LOOP_DTYPE.fields["pose_loop"][1] == 240


def test_argument_checks_without_an_object():
    from cartslam import _lib
    assert lib_error() == "bad arguments"                                       # a valid configuration gets as far as the missing object
    assert lib_error(dict(max_distance=0, ratio=0, min_score=0, max_candidates=1, min_gap=0)) == "bad arguments"
    assert lib_error(dict(max_distance=256, ratio=100, min_score=65536, max_candidates=16, min_gap=(1 << 64) - 1)) == "bad arguments"
    assert "params" in lib_error(params_null=True)
    for key, bad in (("max_distance", -1), ("max_distance", 257), ("ratio", -1), ("ratio", 101), ("min_score", -1), ("min_score", 65537),
                     ("max_candidates", 0), ("max_candidates", 17)):
        assert key in lib_error({key: bad}), (key, bad)
    assert "max_distance" in lib_error(dict(max_distance=300, max_candidates=0))     # in the order of the fields
    lib = _lib.load()
    out = C.c_void_p()
    for args, word in (((None, 0, 4), "max_features"), ((None, 65537, 4), "max_features"), ((None, 8, 0), "capacity"), ((None, 8, 1025), "capacity"),
                       ((None, 0, 0), "max_features"), ((None, 1, 1), "bad arguments"), ((None, 65536, 1024), "bad arguments")):
        assert lib.cart_place_create(*args, C.byref(out)) != 0 and word in lib.cart_last_error(None).decode()
        assert out.value is None
    # every call refuses a NULL object before it looks at anything else
    slot = C.c_int32(-7)
    assert lib.cart_place_insert(None, None, 0, None, None, None, 0, C.byref(slot), None) != 0 and lib.cart_last_error(None).decode() == "bad arguments"
    assert slot.value == -7
    assert lib.cart_place_clear(None, None) != 0 and lib.cart_last_error(None).decode() == "bad arguments"
    ptrs = [C.c_void_p(5) for _ in range(4)]
    assert lib.cart_place_slot(None, 0, *[C.byref(q) for q in ptrs]) != 0 and lib.cart_last_error(None).decode() == "bad arguments"
    assert [q.value for q in ptrs] == [5] * 4
    lib.cart_place_destroy(None)   # a NULL object is ignored


# ---- the frame-loop case of tests/test_gpu_place.py, restated ---------------------------------------------------------------
LOOP_ORDER = [0, 1, 2, 3, 0, 1]            # camera positions of frames 1..6: the last two frames repeat the first two images
LOOP_KEYS = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
LOOP_CONFIG = dict(keyframe_interval=2, min_gap=3, min_score=40, min_inliers=20, capacity=4)
_LOOP = []


def loop_sequence():
    """-> (images per frame, features, stereo matches, temporal matches, expected LOOP_DTYPE records) of the short revisit sequence: the
    source of test_gpu_ego.py's frame loop (2 x 2 block noise, 320 x 96, the camera 3 pixels right and 1 down per position) with the
    positions of LOOP_ORDER, restated through np_orb -> np_match -> np_ego -> np_place.  Computed once per process."""
    if not _LOOP:
        import np_ego as E
        import np_match as M
        import np_orb as N
        from test_gpu_matches import noise_frame, noise_world
        world = noise_world(79)
        cam = E.camera(fx=300.0, fy=300.0, cx=160.0, cy=48.0, baseline=0.5)
        distinct = {k: noise_frame(world, k) for k in set(LOOP_ORDER)}
        orb = {k: (N.orb(l, 5000), N.orb(r, 5000)) for k, (l, r) in distinct.items()}
        images, feats = [distinct[k] for k in LOOP_ORDER], [orb[k] for k in LOOP_ORDER]
        stereo_of = {k: M.match(fl[1], fr[1], M.stereo_params(), fl[0], fr[0])[0] for k, (fl, fr) in orb.items()}
        stereo = [stereo_of[k] for k in LOOP_ORDER]
        temporal = [np.zeros(0, M.MATCH_DTYPE)] + [M.match(feats[f][0][1], feats[f - 1][0][1], M.temporal_params(), feats[f][0][0], feats[f - 1][0][0])[0]
                                                   for f in range(1, len(LOOP_ORDER))]
        lm_of = {k: E.triangulate(cam, fl[0], fr[0], stereo_of[k]) for k, (fl, fr) in orb.items()}
        lms = [lm_of[k] for k in LOOP_ORDER]
        pose, frames, ego = list(E.POSE_IDENTITY), [], []
        for f in range(len(LOOP_ORDER)):
            res = E.estimate(cam, E.params(), lms[f], feats[f][0][0], lms[max(f - 1, 0)], temporal[f], 0, f + 1)[0]
            pose = E.chain(pose, res)
            ego.append((res, list(pose)))
            frames.append((f + 1, feats[f][0][0], feats[f][0][1], lms[f], list(pose)))
        cfg = dict(LOOP_CONFIG)
        place = P.params(min_gap=cfg.pop("min_gap"), min_score=cfg.pop("min_score"))
        records = P.loop_closure(frames, cam, place, E.params(), 5000, **cfg)
        _LOOP.append((images, feats, stereo, temporal, ego, records))
    return _LOOP[0]


def test_the_revisit_sequence_closes_its_loop():
    """The premise of the GPU frame-loop case: the restatement itself recognises frame 2 from frame 6 and nothing before."""
    import np_ego as E
    records = loop_sequence()[5]
    assert records["detected"].tolist() == [0, 0, 0, 0, 0, 1]
    r = records[5]
    assert (r["slot"], r["keyframe_id"]) == (0, 2) and r["score"] >= 10 * LOOP_CONFIG["min_score"]
    rel = r["relative"]
    assert rel["status"] == 1 and rel["n_inliers"] >= 5 * LOOP_CONFIG["min_inliers"]
    # the same image: the relative pose is the identity to a hair, and the loop puts frame 6 where frame 2 was
    assert np.abs(rel["R"] - np.array(E.IDENTITY)).max() < 1e-6 and np.abs(rel["t"]).max() < 1e-6
    assert np.abs(r["pose_loop"] - r["pose_keyframe"]).max() < 1e-6 and r["pose_keyframe"].tolist() == loop_sequence()[4][1][1]
    assert not records[:5].tobytes().strip(b"\0")          # a record without a detection is all zeros

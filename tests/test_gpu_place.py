"""GPU tests of the place recognition stage (spec S27): cart_place_query's scores, candidate records and count equal the
numpy restatement (tests/np_place.py) byte for byte -- the written prefix of the candidate array, with the sentinel behind it untouched --
over the ring, the layouts and the object's lifecycle; and the "loop_closure" module through the C++ frame loop equals the restatement
fed with the restated features, matches and poses of every frame.

The kernels as built: place_score has 128 queries per workgroup and stages 128 stored descriptors in LDS at a time (kPlaceRows,
kMatchTile), one workgroup per (query block, slot); place_select is one workgroup of 1024 threads, one per slot."""
import ctypes as C

import numpy as np
import pytest

import np_match as M
import np_orb as N
import np_place as P
import test_place_spec as S

pytestmark = pytest.mark.gpu

MF = 300                                   # max_features of most objects here: not a multiple of the tile
SENTINEL = 0x5A5A5A5A5A5A5A5A
COUNTS = [0, 1, 127, 128, 129, 257]        # around the tile and the rows of a workgroup


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


def pp(p):
    from cartslam import place_params
    return place_params(**p)


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream_ptr():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def rows_dev(a, rows, step=32, offset=0, fill=None):
    """Device view [rows, 32] of the host rows `a`, `step` bytes apart and starting `offset` bytes into a fresh buffer; the rows from
    len(a) on repeat `fill` (rows that would win every vote if they were read) or are 0xff."""
    torch = _torch()
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
    full = np.full((rows, step), 0xff, np.uint8)
    full[:len(a), :32] = a
    if fill is not None and rows > len(a):
        full[len(a):, :32] = np.resize(fill, (rows - len(a), 32))
    buf = torch.zeros(rows * step + offset + 8, dtype=torch.uint8, device="cuda")
    buf[offset:offset + rows * step] = torch.from_numpy(full.reshape(-1)).cuda()
    view = buf[offset:offset + rows * step].view(rows, step)[:, :32]
    assert view.data_ptr() % 4 == offset % 4 and view.stride(0) == step
    return view


def count_dev(n):
    return _torch().tensor([n], dtype=_torch().int32, device="cuda")


def rand_kps(rng, n):
    k = np.zeros(n, N.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.integers(0, 256, n).astype(np.float32) / 4, rng.integers(0, 64, n).astype(np.float32) / 4
    k["octave"], k["response"] = rng.integers(0, 4, n), rng.random(n).astype(np.float32)
    return k


def kps_dev(k, rows):
    full = np.zeros(rows, N.KEYPOINT_DTYPE)
    full[:len(k)] = k
    return _torch().from_numpy(full.view(np.float32).reshape(-1, 7)).cuda()


def landmarks_dev(lm, rows):
    full = np.zeros((rows, 4), np.float64)
    full[:len(lm)] = lm
    return _torch().from_numpy(full).cuda()


def insert(db, ring, desc, fid, kp=None, lm=None, count=None, step=32, offset=0, fill=None):
    """One frame into the device ring and the restatement; -> the slot (the two must agree)."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    kp = rand_kps(np.random.default_rng(len(desc)), len(desc)) if kp is None else kp
    d, k = rows_dev(desc, db.max_features, step, offset, fill), kps_dev(kp, db.max_features)
    l = landmarks_dev(lm, db.max_features) if lm is not None else None
    c = count_dev(len(desc) if count is None else count)
    slot = C.c_int32(-1)
    db._check(db._lib.cart_place_insert(db._h, vp(d), step, vp(k), vp(l), vp(c), fid, C.byref(slot), stream_ptr()), "cart_place_insert")
    want = ring.insert(desc, fid, kp, lm, count)
    assert slot.value == want
    return want


def query_raw(db, d, step, c, fid, p, want_scores=True):
    """cart_place_query into sentinel-filled outputs on the current stream; -> (scores or None, candidates int64 [max_candidates, 2], n)."""
    torch = _torch()
    scores = torch.full((db.capacity,), -77, dtype=torch.int32, device="cuda") if want_scores else None
    cand = torch.full((p.max_candidates, 2), SENTINEL, dtype=torch.int64, device="cuda")
    n = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    db._check(db._lib.cart_place_query(db._h, C.byref(p), vp(d), step, vp(c), fid, vp(scores), vp(cand), vp(n), stream_ptr()), "cart_place_query")
    return scores, cand, n


def compare(out, expect, what=""):
    """Device outputs of query_raw against the restatement's (scores, candidates): byte for byte."""
    scores, cand, n = out
    escores, ecand = expect
    if scores is not None:
        assert scores.cpu().numpy().tobytes() == escores.tobytes(), f"{what}: scores {scores.cpu().numpy().tolist()} != {escores.tolist()}"
    assert int(n.item()) == len(ecand), f"{what}: count {int(n.item())} != {len(ecand)}"
    got = cand.cpu().numpy()
    assert got[:len(ecand)].tobytes() == ecand.tobytes(), f"{what}: candidates {got[:len(ecand)].view(P.CANDIDATE_DTYPE).tolist()} != {ecand.tolist()}"
    assert (got[len(ecand):] == SENTINEL).all(), f"{what}: written past the count"


def check(db, ring, qd, fid, p, count=None, step=32, offset=0, fill=None, want_scores=True):
    qd = np.ascontiguousarray(qd, np.uint8).reshape(-1, 32)
    out = query_raw(db, rows_dev(qd, db.max_features, step, offset, fill), step, count_dev(len(qd) if count is None else count), fid, pp(p), want_scores)
    expect = ring.query(qd, fid, p, count)
    compare(out, expect, f"nq={len(qd)} fid={fid} {p}")
    return expect


def make_db(max_features, capacity):
    from cartslam import PlaceDB
    return PlaceDB(engine(), max_features, capacity), P.Ring(max_features, capacity)


def related_frame(rng, base, n, noise_every=3):
    """n rows: copies of distinct base rows with 0..80 bits flipped, every noise_every-th one unrelated."""
    rows = S.rand_desc(rng, n)
    for j in range(n):
        if j % noise_every:
            rows[j] = S.flip_bits(rng, base[(7 * j + 3) % len(base)], int(rng.integers(0, 81)))
    return rows


@pytest.fixture(scope="module")
def mixed():
    """One database whose slots hold 0, 1, 127, 128, 129 and 257 features of a common base set."""
    rng = np.random.default_rng(27)
    base = S.rand_desc(rng, 257)
    db, ring = make_db(MF, len(COUNTS))
    for f, n in enumerate(COUNTS):
        insert(db, ring, related_frame(rng, base, n), 10 + f, fill=base)
    yield db, ring, base
    db.close()


@pytest.mark.parametrize("nq", COUNTS)
def test_query_sizes_against_slots_of_different_counts(mixed, nq):
    db, ring, base = mixed
    scores, cand = check(db, ring, base[:nq], 1000, P.params(min_score=1, max_candidates=16), fill=base)
    if nq >= 127:
        assert len(set(scores.tolist())) >= 4 and scores[0] == 0 and len(cand) >= 4
    check(db, ring, base[:nq], 1000, P.params(ratio=0, max_distance=256, min_score=0), fill=base)    # every query votes for every slot that holds a row
    check(db, ring, base[:nq], 1000, P.params(ratio=95, max_distance=70, min_score=nq // 8, max_candidates=2), want_scores=False)
    check(db, ring, base[:nq], 62, P.params(min_score=0, max_candidates=16))                          # slots 0..2 only (10, 11, 12 + 50 <= 62)
    check(db, ring, base[:nq], 59, P.params(min_score=0))                                            # all slots ineligible


@pytest.mark.parametrize("capacity", [1, 3, 5])
def test_ring_and_insert_counts(capacity):
    rng = np.random.default_rng(capacity)
    base = S.rand_desc(rng, 90)
    for inserts in (0, 1, capacity, capacity + 2):
        db, ring = make_db(MF, capacity)
        for f in range(inserts):
            insert(db, ring, related_frame(rng, base, int(rng.integers(20, 90))), 3 * f, lm=rng.random((90, 4)) if f % 2 else None)
        for p in (P.params(min_gap=0, min_score=1), P.params(min_gap=4, ratio=0, min_score=0, max_candidates=1 + capacity // 2)):
            scores, _ = check(db, ring, base, 3 * inserts, p)
            assert (scores >= 0).sum() == sum(1 for s in ring.slots if s is not None and s["frame_id"] + p["min_gap"] <= 3 * inserts)
        db.close()


def test_spec_cases_on_the_device():
    """The hand-worked cases of tests/test_place_spec.py: the vote rule's edges, eligibility and the uint64 wrap, ties, max_candidates."""
    rng = np.random.default_rng(1)
    q = S.rand_desc(rng, 1)[0]
    f = lambda k: S.flip_bits(rng, q, k)   # noqa: E731
    same = f(12)
    edges = [([f(64)], {}, 1), ([f(65)], {}, 0), ([f(65)], dict(max_distance=65), 1), ([f(0)], dict(max_distance=0), 1), ([f(1)], dict(max_distance=0), 0),
             ([f(40), f(50)], {}, 0), ([f(50), f(39)], {}, 1), ([f(40), f(50)], dict(ratio=0), 1), ([f(40), f(50)], dict(ratio=81), 1),
             ([same, same], {}, 0), ([same, same], dict(ratio=0), 1), ([q, q], dict(ratio=100), 0), ([q, f(1)], dict(ratio=1), 1)]
    db, ring = make_db(16, 1)
    for train, fields, want in edges:
        insert(db, ring, np.array(train), 0)
        scores, _ = check(db, ring, q.reshape(1, 32), 100, P.params(min_score=0, **fields))
        assert scores.tolist() == [want]
    db.close()
    # min_gap exactly met and one short, the wrap
    d = S.rand_desc(rng, 3)
    db, ring = make_db(16, 4)
    for fid in (10, 11, (1 << 64) - 10, 0):
        insert(db, ring, d, fid)
    top = (1 << 64) - 1
    for fid, gap, want in ((60, 50, [3, -1, -1, 3]), (61, 50, [3, 3, -1, 3]), (top, 9, [3, 3, 3, 3]), (top, 10, [3, 3, -1, 3]), (5, 20, [-1] * 4),
                           (9, top, [-1] * 4), (top, top, [-1, -1, -1, 3]), (0, 0, [-1, -1, -1, 3])):
        scores, _ = check(db, ring, d, fid, P.params(ratio=0, min_gap=gap, min_score=0))
        assert scores.tolist() == want, (fid, gap)
    db.close()
    # ties by frame id, then slot; max_candidates above and below the number that qualify
    q8, frames = S.tie_case()
    db, ring = make_db(16, 5)
    for s, fid in frames:
        insert(db, ring, s, fid)
    fields = dict(ratio=0, max_distance=0, min_gap=0)
    _, cand = check(db, ring, q8, 100, P.params(min_score=1, max_candidates=16, **fields))
    assert cand.tolist() == [(3, 6, 4), (0, 6, 9), (2, 5, 7), (1, 3, 6), (4, 3, 6)]
    for m in (1, 2, 4, 5, 6):
        check(db, ring, q8, 100, P.params(min_score=1, max_candidates=m, **fields))
    check(db, ring, q8, 100, P.params(min_score=5, max_candidates=16, **fields))
    check(db, ring, q8, 100, P.params(min_score=7, **fields))
    check(db, ring, q8, 6, P.params(min_score=1, max_candidates=16, **fields))
    db.close()
    # an empty slot scores 0 and is a candidate only at min_score = 0; an empty query
    db, ring = make_db(16, 3)
    insert(db, ring, np.zeros((0, 32), np.uint8), 7)
    insert(db, ring, S.rand_desc(rng, 5), 8, count=0)
    for qd in (S.rand_desc(rng, 4), np.zeros((0, 32), np.uint8)):
        assert check(db, ring, qd, 100, P.params())[0].tolist() == [0, 0, -1]
        assert check(db, ring, qd, 100, P.params(min_score=0))[1].tolist() == [(0, 0, 7), (1, 0, 8)]
    db.close()


@pytest.mark.parametrize("step,offset", [(32, 0), (48, 0), (32, 1), (48, 1), (33, 0)])
def test_layouts_of_insert_and_query(step, offset):
    """Pitched rows and a base one byte in (load_desc's byte path), for the stored frames and for the query alike."""
    rng = np.random.default_rng(100 * step + offset)
    base = S.rand_desc(rng, 200)
    db, ring = make_db(MF, 3)
    for f in range(3):
        insert(db, ring, related_frame(rng, base, 140 + 30 * f), f, step=step, offset=offset, fill=base)
    for qs, qo in ((32, 0), (step, offset)):
        scores, _ = check(db, ring, base, 100, P.params(min_score=1), step=qs, offset=qo, fill=base)
        assert scores.min() > 20
    db.close()


def test_counts_are_clamped_on_the_device():
    rng = np.random.default_rng(6)
    base = S.rand_desc(rng, 40)
    db, ring = make_db(40, 3)
    frame = related_frame(rng, base, 40)
    insert(db, ring, frame, 0, count=1000)              # above max_features: the whole buffer, no more
    insert(db, ring, frame, 1, count=-3)                # negative: empty
    insert(db, ring, frame[:25], 2, fill=base)          # the rows behind the count are copies of the queries
    for count, want in ((None, None), (1 << 20, 40), (-1, 0), (0, 0), (17, 17)):
        scores, _ = check(db, ring, base, 100, P.params(min_score=0, ratio=0), count=count, fill=base)
        assert scores[1] == 0
    assert ring.slots[0]["desc"].shape == (40, 32) and ring.slots[1]["desc"].shape == (0, 32)
    db.close()


def test_slot_pointers_feed_the_matcher():
    """cart_place_slot's descriptors, keypoints and count in cart_matcher_match give the matches of the original buffers; the landmarks
    are the inserted ones, or NULL."""
    torch = _torch()
    from cartslam import EngineError, OrbMatcher
    from cartslam.engine import match_params
    rng = np.random.default_rng(7)
    base = S.rand_desc(rng, 150)
    db, ring = make_db(MF, 3)
    frames = [(related_frame(rng, base, 120, 5), rand_kps(rng, 120), rng.random((120, 4))), (related_frame(rng, base, 77, 4), rand_kps(rng, 77), None)]
    for f, (d, k, lm) in enumerate(frames):
        insert(db, ring, d, f, kp=k, lm=lm, step=48, offset=1)
    with pytest.raises(EngineError, match="slot 2"):
        db.slot(2)
    for bad in (-1, 3):
        with pytest.raises(EngineError, match="slot"):
            db.slot(bad)
    matcher = OrbMatcher(engine(), MF)
    qk = rand_kps(rng, 150)
    q = (kps_dev(qk, MF), rows_dev(base, MF), count_dev(150))
    for f, (d, k, lm) in enumerate(frames):
        dp, kp, lp, cp = db.slot(f)
        assert (lp is None) == (lm is None)
        p = M.params(use_gate=1, dx_min=-40.0, dx_max=40.0, dy_min=-12.0, dy_max=12.0, max_octave_diff=2)   # 55 and 41 matches on the restatement
        out = torch.zeros((MF, 4), dtype=torch.int32, device="cuda")
        n = torch.zeros(1, dtype=torch.int32, device="cuda")
        mp = match_params(**p)
        matcher._check(matcher._lib.cart_matcher_match(matcher._h, C.byref(mp), vp(q[1]), 32, vp(q[0]), vp(q[2]), C.c_void_p(dp), 32, C.c_void_p(kp), C.c_void_p(cp),
                                                       vp(out), vp(n), None, stream_ptr()), "cart_matcher_match")
        got = out[:int(n.item())].cpu().numpy().view(M.MATCH_DTYPE).reshape(-1)
        direct = matcher.match((qk, base, None), (k, d, None), mp)
        assert got.tobytes() == direct.tobytes() == M.match(base, d, p, qk, k)[0].tobytes() and len(got) > 10
        if lm is not None:
            back = torch.zeros((len(lm), 4), dtype=torch.float64, device="cuda")
            eng = engine()      # the library's own copy kernel reads the raw address
            eng._check(eng._lib.cart_copy_narrow(eng._h, vp(back), C.c_void_p(lp), back.numel() * 8, 0, stream_ptr()), "cart_copy_narrow")
            assert back.cpu().numpy().tobytes() == np.ascontiguousarray(lm).tobytes()
    matcher.close()
    db.close()


def test_python_object():
    """PlaceDB's own insert / query / clear: host arrays go up, the outputs stay on the device."""
    from cartslam import PLACE_CANDIDATE_DTYPE, EngineError, PlaceDB, place_params
    rng = np.random.default_rng(8)
    base = S.rand_desc(rng, 100)
    db, ring = PlaceDB(engine(), MF, 4), P.Ring(MF, 4)
    for f in range(5):
        d, k = related_frame(rng, base, 60 + 10 * f), rand_kps(rng, 100)
        assert db.insert(d, k, 10 * f, landmarks=rng.random((100, 4)) if f else None) == ring.insert(d, 10 * f)
    p = P.params(min_gap=10, min_score=5)
    scores, cand, n = db.query(base, 45, place_params(**p))
    assert scores.is_cuda and cand.is_cuda and n.is_cuda
    escores, ecand = ring.query(base, 45, p)
    assert scores.cpu().numpy().tobytes() == escores.tobytes() and int(n.item()) == len(ecand) > 1
    assert cand.cpu().numpy().view(PLACE_CANDIDATE_DTYPE).reshape(-1)[:len(ecand)].tobytes() == ecand.tobytes()
    assert db.query(base, 45, place_params(**p), want_scores=False)[0] is None
    db.clear()
    scores, cand, n = db.query(base, 45, place_params(**p))
    assert (scores.cpu().numpy() == -1).all() and int(n.item()) == 0
    with pytest.raises(EngineError, match="slot 0"):
        db.slot(0)
    assert db.insert(base, rand_kps(rng, 100), 1) == 0
    assert db.query(base, 100)[0].cpu().numpy().tolist() == [100, -1, -1, -1]
    db.close()
    db.close()
    with pytest.raises(Exception):
        db.query(base, 100)
    for args in ((0, 4), (65537, 4), (8, 0), (8, 1025)):
        with pytest.raises(EngineError):
            PlaceDB(engine(), *args)


def test_repeats_streams_and_clear():
    torch = _torch()
    rng = np.random.default_rng(9)
    base = S.rand_desc(rng, 260)
    frames = [related_frame(rng, base, 100 + 40 * f) for f in range(4)]
    p = P.params(min_gap=0, min_score=1)
    ring = P.Ring(MF, 3)
    for f, d in enumerate(frames):
        ring.insert(d, f)
    expect = ring.query(base, 10, p)
    qd, qc = rows_dev(base, MF), count_dev(260)
    dev = [(rows_dev(d, MF), kps_dev(rand_kps(rng, len(d)), MF), count_dev(len(d))) for d in frames]
    torch.cuda.synchronize()

    def run(streams):
        """inserts on one stream, the queries on the other, no host synchronisation in between: the object orders them"""
        db, _ = make_db(MF, 3)
        torch.cuda.synchronize()
        outs = []
        with torch.cuda.stream(streams[0]):
            for f, (d, k, c) in enumerate(dev):
                db._check(db._lib.cart_place_insert(db._h, vp(d), 32, vp(k), None, vp(c), f, None, stream_ptr()), "cart_place_insert")
        for s in (streams[1], streams[0], streams[1]):
            with torch.cuda.stream(s):
                outs.append(query_raw(db, qd, 32, qc, 10, pp(p)))
        with torch.cuda.stream(streams[0]):
            db.clear()
        with torch.cuda.stream(streams[1]):
            outs.append(query_raw(db, qd, 32, qc, 10, pp(p)))
        torch.cuda.synchronize()
        db.close()
        return outs

    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for outs in (run((a, a)), run((a, b))):
        for o in outs[:3]:
            compare(o, expect)
        compare(outs[3], (np.full(3, -1, np.int32), expect[1][:0]))


def test_destroyed_after_its_engine():
    from cartslam import Engine, PlaceDB
    rng = np.random.default_rng(10)
    base = S.rand_desc(rng, 50)
    other = Engine(64, 32, num_disparities=0, paths=0)
    db, ring = PlaceDB(other, MF, 2), P.Ring(MF, 2)
    insert(db, ring, base, 0)
    other.close()
    check(db, ring, base, 100, P.params())
    db.close()


def test_bad_arguments_name_the_argument_and_touch_nothing():
    torch = _torch()
    db, ring = make_db(MF, 4)
    rng = np.random.default_rng(11)
    insert(db, ring, S.rand_desc(rng, 30), 0)
    lib = db._lib
    d, k, c = rows_dev(S.rand_desc(rng, 30), MF), kps_dev(rand_kps(rng, 30), MF), count_dev(30)
    lm = landmarks_dev(rng.random((30, 4)), MF)
    err = lambda: lib.cart_last_error(None).decode()   # noqa: E731
    at = lambda t, off: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    slot = C.c_int32(-7)
    for args, word in (((None, 32, vp(k), None, vp(c)), "desc"), ((vp(d), 32, None, None, vp(c)), "kp"), ((vp(d), 32, vp(k), None, None), "count"),
                       ((vp(d), 32, at(k, 2), None, vp(c)), "kp"), ((vp(d), 32, vp(k), at(lm, 4), vp(c)), "landmarks"), ((vp(d), 32, vp(k), None, at(c, 1)), "count"),
                       ((vp(d), 31, vp(k), None, vp(c)), "desc_step"), ((vp(d), 0, vp(k), None, vp(c)), "desc_step")):
        assert lib.cart_place_insert(db._h, *args, 5, C.byref(slot), None) != 0 and word in err(), (word, err())
        assert slot.value == -7
    scores = torch.full((8,), -77, dtype=torch.int32, device="cuda")
    cand = torch.full((6, 2), SENTINEL, dtype=torch.int64, device="cuda")
    n = torch.full((4,), -5, dtype=torch.int32, device="cuda")
    p = pp(P.params(min_gap=0, min_score=0))
    good = (vp(d), 32, vp(c), 100, vp(scores), vp(cand), vp(n))

    def bad(i, v):
        a = list(good)
        a[i] = v
        return a
    cases = [(bad(0, None), "q_desc"), (bad(2, None), "q_count"), (bad(5, None), "candidates"), (bad(6, None), "n_candidates"), (bad(2, at(c, 2)), "q_count"),
             (bad(4, at(scores, 2)), "scores"), (bad(5, at(cand, 4)), "candidates"), (bad(6, at(n, 1)), "n_candidates"), (bad(1, 31), "q_step"),
             (bad(4, at(cand, 8)), "scores and candidates"), (bad(6, at(scores, 12)), "scores and n_candidates"), (bad(6, at(cand, 48)), "candidates and n_candidates"),
             (bad(4, at(d, 64)), "scores and q_desc"), (bad(5, at(d, MF * 32 - 8)), "candidates and q_desc"), (bad(6, vp(c)), "n_candidates and q_count")]
    for args, word in cases:
        assert lib.cart_place_query(db._h, C.byref(p), *args, None) != 0 and word in err(), (word, err())
    torch.cuda.synchronize()
    assert (scores.cpu().numpy() == -77).all() and (cand.cpu().numpy() == SENTINEL).all() and (n.cpu().numpy() == -5).all()
    assert lib.cart_place_query(db._h, C.byref(p), *bad(6, at(cand, 64)), None) == 0       # candidates [4] end where the next buffer starts ...
    assert lib.cart_place_query(db._h, C.byref(p), *good, stream_ptr()) == 0              # ... and the object is still usable
    compare((scores[:4], cand[:4], n[:1]), ring.query(d[:30].cpu().numpy(), 100, P.params(min_gap=0, min_score=0)))
    db.close()


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------
def test_loop_closure_module_frame_loop(tmp_path):
    """[orb_features, orb_matches, ego_motion, loop_closure] over the revisit sequence of tests/test_place_spec.py: every frame's dumped
    record equals the restatement's, whole; test_the_revisit_sequence_closes_its_loop holds the premise (frame 6 finds frame 2)."""
    import json
    import os
    import np_ego as E
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    images, feats, stereo, temporal, ego, records = S.loop_sequence()
    n = len(images)
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for cam in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, cam))
    for f, (l, r) in enumerate(images):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    front = [{"type": "orb_features"}, {"type": "orb_matches"}, dict(S.LOOP_KEYS, type="ego_motion")]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, front + [dict(S.LOOP_KEYS, type="loop_closure", **S.LOOP_CONFIG)], tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    assert records["detected"].tolist() == [0] * (n - 1) + [1]
    for fid in range(1, n + 1):
        got = open(os.path.join(d, f"{fid}_loop_closure.bin"), "rb").read()
        assert len(got) == P.LOOP_DTYPE.itemsize
        assert got == records[fid - 1].tobytes(), f"frame {fid}: {np.frombuffer(got, P.LOOP_DTYPE)} != {records[fid - 1]}"
        # the dumps of the modules before it are what they are without it
        res, pose = ego[fid - 1]
        assert open(os.path.join(d, f"{fid}_ego_motion.bin"), "rb").read() == res.tobytes() + np.array(pose, np.float64).tobytes(), f"frame {fid}: ego_motion"
        assert np.fromfile(os.path.join(d, f"{fid}_feature_matches_temporal.bin"), M.MATCH_DTYPE).tobytes() == temporal[fid - 1].tobytes()
    assert E.RESULT_DTYPE.itemsize == 120
    # creation-time checks: the dependencies, the camera and an out-of-range key with the library's message
    r = run_exe(src, [{"type": "orb_features"}, {"type": "orb_matches"}, dict(S.LOOP_KEYS, type="loop_closure")], tmp)
    assert r.returncode != 0 and 'requires "ego_motion"' in r.stderr
    r = run_exe(src, front + [{"type": "loop_closure"}], tmp)
    assert r.returncode != 0 and "fx" in r.stderr
    for key, bad in (("ratio", 101), ("max_candidates", 17), ("capacity", 1025), ("keyframe_interval", 0), ("hypotheses", 0), ("pose_key", "planes")):
        r = run_exe(src, front + [dict(S.LOOP_KEYS, type="loop_closure", **{key: bad})], tmp)
        assert r.returncode != 0 and key in r.stderr, (key, r.stderr)

"""numpy restatement of spec S22: brute-force matching of 256-bit descriptors.  The checker of
cart_matcher_match; shares no code with it.  Distances come from a 256-entry popcount table over the xor of uint8 rows, the
gate is computed in float32, and the query rows are processed in blocks so that 5000 x 5000 fits in memory.  Sets of more
than LARGE pairs take the distances from a product of the unpacked bit matrices instead (800 M table look-ups take seconds);
tests/test_match_spec.py holds the two forms equal."""
import numpy as np

MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4")])
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)
BIG = 1 << 40   # key of an inadmissible pair
DEFAULTS = dict(use_gate=0, dx_min=0.0, dx_max=0.0, dy_min=0.0, dy_max=0.0, max_octave_diff=-1, max_distance=64, ratio=80,
                cross_check=1)   # cart_match_default_params


def params(**fields):
    assert set(fields) <= set(DEFAULTS)
    return dict(DEFAULTS, **fields)


def stereo_params(max_disparity=256, max_dy=2, **fields):
    """The orb_matches module's stereo preset (build-owned)."""
    return params(use_gate=1, dx_min=0.0, dx_max=float(max_disparity), dy_min=-float(max_dy), dy_max=float(max_dy), max_octave_diff=1, **fields)


def temporal_params(search_radius=128, **fields):
    r = float(search_radius)
    return params(use_gate=1, dx_min=-r, dx_max=r, dy_min=-r, dy_max=r, max_octave_diff=1, **fields)


def distances(q, t):
    """int64 [len(q), len(t)] Hamming distances of uint8 [n, 32] rows."""
    return POPCOUNT[q[:, None, :] ^ t[None, :, :]].sum(2)


LARGE = 1 << 20


def distances_product(q, t):
    """The same distances as popcount(q) + popcount(t) - 2 popcount(q & t), the last term as a float32 matrix product of the
    unpacked bits (sums of at most 256 ones: exact)."""
    bq, bt = np.unpackbits(q, axis=1).astype(np.float32), np.unpackbits(t, axis=1).astype(np.float32)
    both = np.rint(bq @ bt.T).astype(np.int64)
    return POPCOUNT[q].sum(1)[:, None] + POPCOUNT[t].sum(1)[None, :] - 2 * both


def admissible(qk, tk, p):
    """bool [nq, nt]; qk / tk = KEYPOINT_DTYPE records."""
    with np.errstate(invalid="ignore"):
        dx = qk["x"].astype(np.float32)[:, None] - tk["x"].astype(np.float32)[None, :]
        dy = qk["y"].astype(np.float32)[:, None] - tk["y"].astype(np.float32)[None, :]
        assert dx.dtype == np.float32
        ok = (np.float32(p["dx_min"]) <= dx) & (dx <= np.float32(p["dx_max"])) & (np.float32(p["dy_min"]) <= dy) & (dy <= np.float32(p["dy_max"]))
    if p["max_octave_diff"] >= 0:
        ok &= np.abs(qk["octave"].astype(np.int64)[:, None] - tk["octave"].astype(np.int64)[None, :]) <= p["max_octave_diff"]
    return ok


def match(qd, td, p=None, qk=None, tk=None, block=256):
    """-> (matches MATCH_DTYPE [n], forward int32 [nq, 4] = (j1, d1, d2, i1(j1) or -1))."""
    p = params() if p is None else p
    qd = np.ascontiguousarray(qd, np.uint8).reshape(-1, 32)
    td = np.ascontiguousarray(td, np.uint8).reshape(-1, 32)
    nq, nt = len(qd), len(td)
    fwd = np.full((nq, 4), -1, np.int64)
    back = np.full(nt, BIG, np.int64)   # min d * 65536 + i per train column
    for i0 in range(0, nq, block):
        i1 = min(nq, i0 + block)
        if nt == 0:
            break
        d = distances(qd[i0:i1], td) if nq * nt <= LARGE else distances_product(qd[i0:i1], td)
        ok = admissible(qk[i0:i1], tk, p) if p["use_gate"] else np.ones(d.shape, bool)
        key = np.where(ok, d * 65536 + np.arange(nt)[None, :], BIG)
        j1 = key.argmin(1)
        best = key[np.arange(i1 - i0), j1]
        has = best < BIG
        rest = np.where(ok, d, BIG)
        rest[np.arange(i1 - i0), j1] = BIG
        d2 = rest.min(1)
        fwd[i0:i1, 0] = np.where(has, j1, -1)
        fwd[i0:i1, 1] = np.where(has, best >> 16, -1)
        fwd[i0:i1, 2] = np.where(has & (d2 < BIG), d2, -1)
        back = np.minimum(back, np.where(ok, d * 65536 + np.arange(i0, i1)[:, None], BIG).min(0))
    i1_of = np.where(back < BIG, back & 65535, -1)
    has = fwd[:, 0] >= 0
    if p["cross_check"]:
        fwd[has, 3] = i1_of[fwd[has, 0]]
    j1, d1, d2 = fwd[:, 0], fwd[:, 1], fwd[:, 2]
    acc = has & (d1 <= p["max_distance"])
    if p["ratio"]:
        acc &= (d2 < 0) | (100 * d1 < p["ratio"] * d2)
    if p["cross_check"]:
        acc &= fwd[:, 3] == np.arange(nq)
    idx = np.nonzero(acc)[0]
    out = np.zeros(len(idx), MATCH_DTYPE)
    out["query"], out["train"], out["distance"], out["second"] = idx, j1[idx], d1[idx], d2[idx]
    return out, fwd.astype(np.int32)

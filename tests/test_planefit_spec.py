"""CPU tests of the superpixel plane spec: the counter-based generator, the RANSAC restatement on
planar sets, the planecluster merge on a hand-built graph, planefit's literal quirks, the C-ABI symbols and the module
factory.  No GPU: the restatement is tests/np_planefit.py, the merge is the library's host code."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import np_planefit as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cart-slam_amd", "build", "cart_slam_amd")


def _mix_by_hand(z):
    m = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) % (1 << 64)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_generator_is_splitmix64():
    # splitmix64 seeded with 0: its first outputs are the finaliser of k * golden gamma (published reference values)
    assert N.mix(0) == 0xE220A8397B1DCDAF
    assert N.mix(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    for z in (1, 12345, (1 << 64) - 1, 0xDEADBEEF << 20):
        assert N.mix(z) == _mix_by_hand(z)
    s = N.stream(7, 1, 3, 5, 11)
    assert s == N.mix(N.mix(N.mix(N.mix(7 ^ 1) ^ 3) ^ 5) ^ 11)
    assert N.draw(s, 2) == N.mix((s + 2) & ((1 << 64) - 1))
    for n in (1, 16, 1000, 65536):
        u = [N.uniform(N.draw(s, c), n) for c in range(200)]
        assert min(u) >= 0 and max(u) < n
    assert N.uniform(0xFFFFFFFF_FFFFFFFF, 17) == 16 and N.uniform(0, 17) == 0


def _planar(n, rng, outliers=0.0):
    # dyadic grid points on z = 2 + x/2 - y/4: exact in float32, so the plane is recovered to rounding
    x = rng.integers(-64, 64, n) / 16.0
    y = rng.integers(-64, 64, n) / 16.0
    z = 2 + x / 2 - y / 4
    k = int(round(outliers * n))
    z[:k] += rng.uniform(0.5, 3.0, k) * rng.choice([-1, 1], k)
    P = np.stack([x, y, z], 1).astype(np.float32)
    return P[rng.permutation(n)]


def _true_plane():
    n = np.array([0.5, -0.25, -1.0])
    inv = 1.0 / np.linalg.norm(n)
    return n * inv, 2.0 * inv


@pytest.mark.parametrize("outliers", [0.0, 0.3])
def test_ransac_recovers_exact_planes(outliers):
    rng = np.random.default_rng(5)
    nrm, d = _true_plane()
    for label, n in enumerate((16, 40, 64, 65, 200, 700)):
        pl, best = N.ransac_plane(_planar(n, rng, outliers), seed=3, frame_id=9, label=label, return_best=True)
        pl = np.array(pl)
        sign = np.sign(pl[2]) * np.sign(nrm[2])
        assert np.abs(pl[:3] * sign - nrm).max() < 1e-9 and abs(pl[3] * sign - d) < 1e-9, (n, pl)
        assert best[0] == n - int(round(outliers * n))


def test_degenerate_sets_give_zero_planes():
    rng = np.random.default_rng(1)
    t = rng.integers(0, 64, 50) / 8.0
    colinear = np.stack([t, 2 * t, -t], 1).astype(np.float32)
    assert N.ransac_plane(colinear, 0, 0, 0) == (0.0, 0.0, 0.0, 0.0)
    assert N.ransac_plane(_planar(15, rng), 0, 0, 0) == (0.0, 0.0, 0.0, 0.0)
    assert N.ransac_plane(np.zeros((0, 3), np.float32), 0, 0, 0) == (0.0, 0.0, 0.0, 0.0)
    nan = _planar(40, rng)
    nan[:, 2] = np.nan            # the planecluster predicate keeps NaN z: no hypothesis has an inlier
    assert N.ransac_plane(nan, 0, 0, 0) == (0.0, 0.0, 0.0, 0.0)


def test_seed_and_frame_change_the_hypotheses():
    a = N.hypothesis_indices(0, 1, 5, 0, 100)
    assert a == N.hypothesis_indices(0, 1, 5, 0, 100) and len(set(a)) == 4
    assert a != N.hypothesis_indices(1, 1, 5, 0, 100) and a != N.hypothesis_indices(0, 2, 5, 0, 100)


def test_predicates():
    z = np.array([np.nan, np.inf, -np.inf, 0.0, -1.0, 1e-3, 40.0, 40.001, 5.0], np.float32)
    assert N.valid_mask(z, N.PRED_PLANEFIT).tolist() == [False, False, False, False, False, True, True, False, True]
    assert N.valid_mask(z, N.PRED_PLANECLUSTER).tolist() == [True, False, False, False, False, True, True, False, True]


# ---- S18 ---------------------------------------------------------------------------------------------------------
def _chain_graph(n):
    off = np.arange(n + 1) * 2 - 1
    off[0] = 0
    nb = []
    offs = [0]
    for l in range(n):
        nb += [q for q in (l - 1, l + 1) if 0 <= q < n]
        offs.append(len(nb))
    return np.array(offs, np.int32), np.array(nb, np.int32)


def _unit(a, b, c):
    v = np.array([a, b, c], float)
    return v / np.linalg.norm(v)


def test_cluster_groups_and_min_size():
    from cartslam import plane_cluster
    n = 80
    off, nb = _chain_graph(n)
    planes = np.zeros((n, 4))
    planes[:40, :3] = _unit(0, 1, 0.05); planes[:40, 3] = 1.5           # 40 like planes: one group
    planes[40:70, :3] = _unit(1, 0, 0); planes[40:70, 3] = -2.0          # 30 like planes: below 32, no group
    planes[75:, :3] = _unit(0, 1, 0.05); planes[75:, 3] = 1.5            # label 70..74 zero: the chain is cut
    P, A = N.plane_cluster(planes, off, nb)
    assert len(P) == 1 and (A[:40] == 1).all() and (A[40:] == 0).all()
    gP, gA = plane_cluster(planes, off, nb)
    assert (gP == P).all() and (gA == A).all()


def test_cluster_keeps_the_literal_current_assignment_compare():
    """planecluster.cpp:137 compares curr + dDiff with new + dDiff: a label already in a group moves to a later seed's
    group only if the later seed is at least as close in angle (dDiff cancels up to rounding)."""
    from cartslam import plane_cluster
    n = 100
    off, nb = _chain_graph(n)
    planes = np.zeros((n, 4))
    planes[:, :3] = _unit(0, 1, 0.0)
    planes[:, 3] = 1.0
    planes[50:, :3] = _unit(0, 1, 0.12)        # second half tilted: within 0.2 of the first half but not equal
    P, A = N.plane_cluster(planes, off, nb)
    gP, gA = plane_cluster(planes, off, nb)
    assert (gP == P).all() and (gA == A).all()
    assert len(P) == 1 and (A == 1).all()      # the first seed takes everything; no later label seeds a group
    rng = np.random.default_rng(3)
    for trial in range(20):
        planes = np.zeros((n, 4))
        tilt = rng.uniform(-0.15, 0.15, n).cumsum() * 0.2
        for l in range(n):
            if rng.random() < 0.05:
                continue
            planes[l, :3] = _unit(tilt[l], 1, rng.uniform(-0.1, 0.1))
            planes[l, 3] = rng.uniform(0, 5)
        P, A = N.plane_cluster(planes, off, nb)
        gP, gA = plane_cluster(planes, off, nb)
        assert (gP == P).all() and (gA == A).all(), trial


def test_cluster_rejects_null_and_bad_tables():
    from cartslam import EngineError, plane_cluster
    off, nb = _chain_graph(4)
    with pytest.raises(EngineError):
        plane_cluster(np.zeros((4, 4)), off, np.array([0, 9, 1, 2, 1, 3], np.int32))
    with pytest.raises(EngineError):       # a negative first offset would read before the neighbour table
        plane_cluster(np.zeros((4, 4)), np.array([-1, 1, 3, 5, 6], np.int32), nb)


def test_cluster_refusals_by_message_write_nothing():
    """Every refusal of cart_plane_cluster by its words; the outputs keep their sentinel."""
    from cartslam import _lib
    lib = _lib.load()
    off, nb = _chain_graph(4)
    planes = np.zeros((4, 4))
    out, assign, n = np.full((4, 4), -7777.25), np.full(4, 0x5A5B5C5D5E5F6061, np.uint64), C.c_int(-77)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(max_label=3, planes=planes, off=off, nb=nb, out=out, assign=assign, n=n):
        return lib.cart_plane_cluster(ptr(planes) if planes is not None else None, max_label, ptr(off) if off is not None else None,
                                      ptr(nb) if nb is not None else None, ptr(out) if out is not None else None,
                                      ptr(assign) if assign is not None else None, C.byref(n) if n is not None else None)

    def refused(rc, words):
        err = lib.cart_last_error(None).decode()
        assert rc != 0 and words in err, (rc, words, err)
        assert (out == -7777.25).all() and (assign == 0x5A5B5C5D5E5F6061).all() and n.value == -77

    for name in ("planes", "off", "nb", "out", "assign", "n"):
        refused(call(**{name: None}), "NULL pointer")
    for bad in (-1, 16384):
        refused(call(max_label=bad), "max_label must be in [0, 16383]")
    refused(call(off=np.array([1, 1, 3, 5, 6], np.int32)), "offsets[0] must be 0")
    refused(call(off=np.array([-1, 1, 3, 5, 6], np.int32)), "offsets[0] must be 0")
    refused(call(off=np.array([0, 3, 1, 5, 6], np.int32)), "offsets are not ascending")
    refused(call(nb=np.array([1, 0, 2, 1, 4, 2], np.int32)), "neighbour label out of range")
    refused(call(nb=np.array([1, 0, 2, 1, -1, 2], np.int32)), "neighbour label out of range")
    assert call() == 0 and n.value == 0 and (assign == 0).all() and (out == -7777.25).all()      # zero planes: no group, no plane row written


# ---- S19 ---------------------------------------------------------------------------------------------------------
def _scene(w, h, bs, invalid_frac, rng):
    lab = ((np.arange(h)[:, None] // bs) * ((w + bs - 1) // bs) + np.arange(w)[None, :] // bs).astype(np.uint16)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    xyz = np.zeros((h, w, 3), np.float32)
    xyz[..., 0] = (xs - w / 2) / 40.0
    xyz[..., 1] = 1.5 + np.zeros_like(xs)                       # road: y = 1.5
    xyz[..., 2] = 2 + ys / 4.0
    L = int(lab.max())
    bad = rng.random(L + 1) < invalid_frac
    xyz[..., 2][bad[lab]] = np.nan
    return lab, xyz, L


def test_planefit_valid_regions_quirk_and_small_samples():
    rng = np.random.default_rng(2)
    lab, xyz, L = _scene(96, 40, 8, 0.0, rng)           # every region valid: assignmentCount starts at 100 % -> no loop
    P, A, it = N.planefit(lab, xyz, L, 0, 1)
    assert it == 0 and len(P) == 0 and (A == 0).all()
    lab, xyz, L = _scene(96, 40, 8, 0.5, rng)           # half the regions invalid: the loop runs
    P, A, it = N.planefit(lab, xyz, L, 0, 1)
    assert it > 0
    # <= 3 local planes: every sampled label is assigned already / too small -> every iteration is skipped
    lab, xyz, L = _scene(96, 40, 8, 0.5, rng)
    xyz[..., 2][:] = np.where(np.isnan(xyz[..., 2]), np.nan, -1.0)   # all points fail the predicate: no label has 16 points
    counts, _, _ = N.label_points(lab, xyz, L, N.PRED_PLANEFIT)
    P, A, it = N.planefit(lab, xyz, L, 0, 1)
    assert it == 100 and len(P) == 0


def test_sample_grid():
    pos = N.sample_positions(96, 40, 0, 1, 0)
    assert 0 < len(pos) <= 5 * 6
    assert N.sample_positions(5, 40, 0, 1, 0) == []      # a step of 0 yields no samples (the reference would not end)
    assert pos != N.sample_positions(96, 40, 1, 1, 0)      # the seed changes the jitter
    assert pos != N.sample_positions(96, 40, 0, 2, 0)      # and so does the frame id
    assert pos != N.sample_positions(96, 40, 0, 1, 1)      # and the iteration


# ---- C ABI and factory -----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["cart_planefit_create", "cart_planefit_destroy", "cart_planefit_label_planes", "cart_planefit_points",
               "cart_planefit_adjacency", "cart_planefit_fit", "cart_planefit_status", "cart_plane_cluster"]


def test_new_symbols_exported_and_reject_null():
    from cartslam import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        res, args = _lib.PROTOTYPES[name]
        if res is not C.c_int:
            continue
        zeros = [a(0) if a in (C.c_int, C.c_size_t, C.c_float, C.c_double) else None for a in args]
        assert getattr(lib, name)(*zeros) != 0, name
        assert lib.cart_last_error(None), name


@pytest.mark.parametrize("mtype", ["planefit", "planecluster"])
def test_factory_knows_plane_modules(tmp_path, mtype):
    from test_host import make_dataset
    src, _ = make_dataset(str(tmp_path), 1, 64, 32)
    mod = tmp_path / "modules.json"
    json.dump([{"type": mtype + "x"}], open(mod, "w"))
    r = subprocess.run([EXE, src, str(mod), "--frames", "0"], capture_output=True, text=True, timeout=120)
    assert "Unknown module type " + mtype + "x." in r.stderr, r.stderr      # the dataset is read: the factory is reached
    json.dump([{"type": mtype, "seed": 3}], open(mod, "w"))
    r = subprocess.run([EXE, src, str(mod), "--frames", "0"], capture_output=True, text=True, timeout=120)
    assert "Unknown module type" not in r.stderr, r.stderr

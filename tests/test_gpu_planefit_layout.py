"""GPU tests of the planefit device object (csrc/engine_planefit.hip, csrc/planefit_kernels.hip) through the C ABI, on buffers whose layout
the test chooses, in the style of test_gpu_post_layout.py (whose Buf helper is used here).

cartslam.PlaneFit allocates everything tight, so through it no kernel ever sees a step above a row or a base inside an allocation, no
refusal is reached and no label count but the image's own.  Here every input lies in one flat allocation whose slack holds values that
would change the result (label 1, which the image uses; the point (11, 11, 11), a valid z off every plane), every output lies in a
sentinel-filled allocation whose slack must be intact afterwards, and every expected value comes from the numpy restatement
(np_planefit.py) on the tight host arrays, compared exactly.  The inputs and the premises that make them non-trivial are in
planefit_cases.py; test_planefit_cases.py checks the premises without a GPU.

Not reached, because no call can get there: "image too small for the planefit sampling grid" (an engine is at least 16 x 8, whose grid
has at most 8 x 8 slots; for the same reason there is no image with w < 6 or h < 5, see test_refusals), the two allocation failures of
create, and "internal error: adjacency capacity exceeded" (the capacity check in front of the launch rules it out).
"""
import ctypes as C

import numpy as np
import pytest

import np_planefit as N
import planefit_cases as K
from test_gpu_post_layout import Buf, _torch, engine, flat, lib, ok, refused

pytestmark = pytest.mark.gpu

S32, S64, SD, SF = 0x5A5B5C5D, 0x5A5B5C5D5E5F6061, -7777.25, -7777.25      # sentinels: no label, count or offset, and no plane or point of any case
LAYOUTS = ["tight", "steps", "steps2", "offset", "both"]
FIT, CLUSTER = N.PRED_PLANEFIT, N.PRED_PLANECLUSTER


def geometry(layout, w):
    """-> (labels step, labels base, xyz step, xyz base) in bytes.
      steps    labels: the smallest even step above the row; xyz: the row + 4 bytes
      steps2   labels: the next step that is no multiple of 4; xyz: the row + 12 + 8 bytes (one pixel and two floats)
      offset   labels 2 bytes, xyz 4 bytes past the 256-byte aligned start of their allocations
      both     steps2 and offset together"""
    lrow, xrow = 2 * w, 12 * w
    second = lrow + 6 if (lrow + 2) % 4 == 2 else lrow + 4
    assert second % 4 == 2
    return {"tight": (lrow, 0, xrow, 0), "steps": (lrow + 2, 0, xrow + 4, 0), "steps2": (second, 0, xrow + 20, 0),
            "offset": (lrow, 2, xrow, 4), "both": (second, 2, xrow + 20, 4)}[layout]


def place(lab, xyz, layout):
    ls, lbase, xs, xbase = geometry(layout, lab.shape[1])
    return (Buf(lab[None], step=ls, base=lbase, fill=K.SLACK_LABEL), Buf(xyz[None], step=xs, base=xbase, fill=np.float32(K.OFF[0])))


def sentinel(n, dtype, fill):
    return flat(np.full(max(n, 1), fill, dtype), fill)


def ptr(buf):
    return buf.ptr if buf is not None else None


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Obj:
    def __init__(self, eng, capacity):
        self.h = C.c_void_p()
        ok(lib().cart_planefit_create(eng._h, capacity, C.byref(self.h)))

    def close(self):
        lib().cart_planefit_destroy(self.h)


def status(pf):
    bad = C.c_int(-1)
    ok(lib().cart_planefit_status(pf.h, C.byref(bad)))
    return bad.value


def label_planes(pf, lb, xb, mx, pred, seed, frame, thr=0.01, want="pnc"):
    """-> the three optional outputs (planes, npts, counts; None where not asked for), each in a sentinel-filled allocation."""
    L1 = mx + 1
    o = dict(planes=sentinel(L1 * 4, np.float64, SD) if "p" in want else None, npts=sentinel(L1, np.int32, S32) if "n" in want else None,
             counts=sentinel(L1 * 2, np.int32, S32) if "c" in want else None)
    ok(lib().cart_planefit_label_planes(pf.h, lb.ptr, lb.step, mx, xb.ptr, xb.step, pred, thr, seed, frame, ptr(o["planes"]), ptr(o["npts"]),
                                        ptr(o["counts"]), None))
    return o


def check_label_planes(o, e):
    if o["planes"] is not None:
        got = o["planes"].image().reshape(-1, 4)
        bad = np.nonzero((got.view(np.uint64) != bits(e["planes"])).any(1))[0]
        assert len(bad) == 0, f"S17 planes differ at labels {bad[:8]}: {got[bad[:2]]} vs {e['planes'][bad[:2]]}"
    if o["npts"] is not None:
        assert np.array_equal(o["npts"].image().ravel(), e["npts"]), "per-label point counts"
    if o["counts"] is not None:
        assert np.array_equal(o["counts"].image().reshape(-1, 2), e["counts"]), "per-label pixel counts"


def check_points(pf, e):
    """cart_planefit_points with capacity exactly the point count."""
    total, L1 = int(e["off"][-1]), len(e["off"]) - 1
    pts, off = sentinel(total * 4, np.float32, SF), sentinel(L1 + 1, np.int32, S32)
    ok(lib().cart_planefit_points(pf.h, pts.ptr, total, off.ptr, None))
    assert np.array_equal(off.image().ravel(), e["off"])
    got = pts.image().reshape(-1, 4)[:total]
    assert np.array_equal(np.ascontiguousarray(got[:, :3]).view(np.uint32), e["pts"].view(np.uint32)), "point lists (raster order inside a label)"
    assert (got[:, 3].view(np.uint32) == 0).all()


def check_adjacency(pf, lb, mx, e, w, h):
    """cart_planefit_adjacency with capacity exactly the documented minimum; entries behind offsets[L1] keep the sentinel."""
    L1 = mx + 1
    cap = min(8 * w * h, L1 * (L1 - 1))
    off, nb = sentinel(L1 + 1, np.int32, S32), sentinel(cap, np.int32, S32)
    ok(lib().cart_planefit_adjacency(pf.h, lb.ptr, lb.step, mx, off.ptr, nb.ptr, cap, None))
    assert np.array_equal(off.image().ravel(), e["aoff"])
    n, got = int(e["aoff"][-1]), nb.image().ravel()
    assert n <= cap and np.array_equal(got[:n], e["anb"]) and (got[n:] == S32).all()


def run_fit(pf, lb, seed, frame, L1):
    planes, assign, n = sentinel(400, np.float64, SD), sentinel(L1, np.uint64, S64), sentinel(1, np.int32, S32)
    launches = C.c_int(0)
    ok(lib().cart_planefit_fit(pf.h, lb.ptr, lb.step, seed, frame, planes.ptr, assign.ptr, n.ptr, C.byref(launches), None))
    assert launches.value == 202
    return planes.image().reshape(100, 4), assign.image().ravel(), int(n.image().ravel()[0])


def check_fit(got, P, A):
    rows, assign, k = got
    assert k == len(P), (k, len(P))
    assert np.array_equal(rows[:k].view(np.uint64), bits(P).reshape(-1, 4)), (rows[:k], P)
    assert (rows[k:].view(np.uint64) == bits(SD)).all(), "plane rows behind n_planes keep the sentinel"
    assert np.array_equal(assign, A), np.nonzero(assign != A)[0][:8]


# ---- 1. layouts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("w,h", K.SIZES)
def test_layouts(w, h, layout):
    eng = engine(w, h)
    lab, xyz, mx = K.layout_scene(w, h)
    lb, xb = place(lab, xyz, layout)
    pf = Obj(eng, mx)
    try:
        for pred in (CLUSTER, FIT):
            e = K.layout_expected(w, h, pred)
            check_label_planes(label_planes(pf, lb, xb, mx, pred, e["seed"], e["frame"]), e)
            check_points(pf, e)
            check_adjacency(pf, lb, mx, e, w, h)
            assert status(pf) == 0
        check_fit(run_fit(pf, lb, e["seed"], e["frame"], mx + 1), *e["fit"][:2])
        assert lb.untouched() and xb.untouched()
    finally:
        pf.close()
    if layout == "tight":      # the control: what the wrapper returns
        from cartslam import PlaneFit
        torch = _torch()
        tl, tx = torch.from_numpy(lab.view(np.int16)).cuda(), torch.from_numpy(xyz).cuda()
        with PlaneFit(eng, mx) as wp:
            for pred in (CLUSTER, FIT):
                e = K.layout_expected(w, h, pred)
                planes, npts, counts = wp.label_planes(tl, tx, mx, pred, seed=e["seed"], frame_id=e["frame"])
                assert np.array_equal(planes.cpu().numpy().view(np.uint64), bits(e["planes"]))
                assert np.array_equal(npts.cpu().numpy(), e["npts"]) and np.array_equal(counts.cpu().numpy(), e["counts"])
                pts, off = wp.points()
                assert np.array_equal(off.cpu().numpy(), e["off"])
                assert np.array_equal(np.ascontiguousarray(pts.cpu().numpy()[:, :3]).view(np.uint32), e["pts"].view(np.uint32))
                off, nb = wp.adjacency(tl, mx)
                assert np.array_equal(off.cpu().numpy(), e["aoff"]) and np.array_equal(nb.cpu().numpy(), e["anb"])
            P, A, launches = wp.fit(tl, seed=e["seed"], frame_id=e["frame"])
            assert np.array_equal(P.cpu().numpy().view(np.uint64), bits(e["fit"][0]).reshape(-1, 4)) and launches == 202
            assert np.array_equal(A.cpu().numpy().view(np.uint64), e["fit"][1])


def test_optional_outputs():
    """planes, npoints and counts as NULL singly and all together: the ones that are given are unchanged, and so is what the object keeps
    (the point lists, and the fit that follows)."""
    w, h = K.BW, K.BH
    eng = engine(w, h)
    lab, xyz, mx = K.layout_scene(w, h)
    lb, xb = place(lab, xyz, "steps")
    e = K.layout_expected(w, h, FIT)
    pf = Obj(eng, mx)
    try:
        for want in ("nc", "pc", "pn", "", "pnc"):
            check_label_planes(label_planes(pf, lb, xb, mx, FIT, e["seed"], e["frame"], want=want), e)
            check_points(pf, e)
            check_fit(run_fit(pf, lb, e["seed"], e["frame"], mx + 1), *e["fit"][:2])
    finally:
        pf.close()


# ---- 2. label-count boundaries, point counts, RANSAC inputs ------------------------------------------------------------------
@pytest.mark.parametrize("L1", K.L1_VALUES)
def test_label_count_boundaries(L1):
    """max_label + 1 around the steps of pf_scan_kernel (1024 threads), pf_colscan_kernel (256 labels a block) and the adjacency bitmap
    (32 labels a word, 64 words a trip), on an object of exactly that capacity (L1 = 1: capacity 0)."""
    eng = engine(K.BW, K.BH)
    lab, xyz, mx = K.sparse_case(L1)
    e = K.sparse_expected(L1)
    lb, xb = place(lab, xyz, "steps" if L1 % 2 else "both")
    pf = Obj(eng, mx)
    try:
        check_label_planes(label_planes(pf, lb, xb, mx, FIT, e["seed"], e["frame"]), e)
        check_points(pf, e)
        check_adjacency(pf, lb, mx, e, K.BW, K.BH)
        assert status(pf) == 0
    finally:
        pf.close()


@pytest.mark.parametrize("n", K.POINT_COUNTS)
def test_point_counts_of_one_label(n):
    """15 and 16 points (the minimum), 1023, 1024 and 1025 (the LDS stage of pf_ransac_kernel holds 1024)."""
    eng = engine(K.BW, K.BH)
    lab, xyz, mx = K.point_count_case(n)
    e = K.point_count_expected(n)
    lb, xb = place(lab, xyz, "steps2")
    pf = Obj(eng, mx)
    try:
        check_label_planes(label_planes(pf, lb, xb, mx, FIT, e["seed"], e["frame"]), e)
        check_points(pf, e)
    finally:
        pf.close()


@pytest.mark.parametrize("pred,thr", K.RANSAC_RUNS)
def test_ransac_inputs(pred, thr):
    """Identical points, collinear points, a threshold no hypothesis meets, thr = 0.05, NaN / inf in x and y, NaN z under PLANECLUSTER."""
    eng = engine(K.BW, K.BH)
    lab, xyz, mx = K.ransac_case()
    e = K.ransac_expected(pred, thr)
    lb, xb = place(lab, xyz, "offset")
    pf = Obj(eng, mx)
    try:
        check_label_planes(label_planes(pf, lb, xb, mx, pred, e["seed"], e["frame"], thr=thr), e)
        check_points(pf, e)
    finally:
        pf.close()


# ---- 3. labels above max_label -------------------------------------------------------------------------------------------
def test_labels_above_max_label():
    """err bit 0 -> cart_planefit_status -> n_planes = -1, and which call clears what: the status flag belongs to the last label_planes or
    adjacency call, the flag behind n_planes to the label_planes call alone."""
    from cartslam import EngineError, PlaneFit
    w, h = K.BW, K.BH
    eng = engine(w, h)
    lab, xyz, low, mx = K.above_case()
    e, full = K.above_expected(), K.layout_expected(w, h, FIT)
    lb, xb = place(lab, xyz, "steps")
    pf = Obj(eng, mx)

    def refused_fit():
        rows, assign, k = run_fit(pf, lb, e["seed"], e["frame"], low + 1)
        assert k == -1 and (assign == 0).all() and (rows.view(np.uint64) == bits(SD)).all()

    try:
        # label_planes with max_label below the image's largest id: the in-range pixels alone
        check_label_planes(label_planes(pf, lb, xb, low, FIT, e["seed"], e["frame"]), e)
        check_points(pf, e)
        assert status(pf) == 1
        refused_fit()
        # ... then adjacency on a clean image: the status speaks of the last label_planes / adjacency call, as documented, but the statistics
        # that fit rests on still left pixels out, so fit still says -1 (with one shared flag it reported a normal plane count)
        check_adjacency(pf, lb, mx, full, w, h)
        assert status(pf) == 0
        refused_fit()
        # a clean label_planes call clears both flags
        check_label_planes(label_planes(pf, lb, xb, mx, FIT, full["seed"], full["frame"]), full)
        assert status(pf) == 0
        check_fit(run_fit(pf, lb, full["seed"], full["frame"], mx + 1), *full["fit"][:2])
        # adjacency on an image with labels above max_label: no pair through such a pixel, status 1; the clean label_planes call still stands
        check_adjacency(pf, lb, low, e, w, h)
        assert status(pf) == 1
        check_fit(run_fit(pf, lb, full["seed"], full["frame"], mx + 1), *full["fit"][:2])
    finally:
        pf.close()
    torch = _torch()
    tl, tx = torch.from_numpy(lab.view(np.int16)).cuda(), torch.from_numpy(xyz).cuda()
    with PlaneFit(eng, mx) as wp:
        wp.label_planes(tl, tx, low, FIT, seed=e["seed"], frame_id=e["frame"])
        assert wp.status()
        with pytest.raises(EngineError, match="label above max_label"):
            wp.fit(tl, seed=e["seed"], frame_id=e["frame"])


# ---- 4. one object, many calls ----------------------------------------------------------------------------------------------
def test_one_object_many_calls():
    """max_label 16383, 63, 2080, 0 on one object of capacity 16383 (cursor is laid out [tiles][L1] with the call's L1): every result equals
    the restatement, as it does on a fresh object of that capacity, and cart_planefit_points shows the last label_planes call only."""
    w, h = K.BW, K.BH
    eng = engine(w, h)
    shared = Obj(eng, 16383)
    try:
        for k, (mx, pred) in enumerate(K.REUSE_STEPS):
            lab, xyz, mx, pred = K.reuse_case(k)
            e = K.reuse_expected(k)
            lb, xb = place(lab, xyz, LAYOUTS[1 + k])
            fresh = Obj(eng, mx)
            try:
                for pf in (shared, fresh):
                    check_label_planes(label_planes(pf, lb, xb, mx, pred, e["seed"], e["frame"]), e)
                    check_points(pf, e)
                    check_adjacency(pf, lb, mx, e, w, h)
                    if pred == FIT:
                        check_fit(run_fit(pf, lb, e["seed"], e["frame"], mx + 1), *e["fit"][:2])
                    assert status(pf) == 0
            finally:
                fresh.close()
    finally:
        shared.close()


# ---- 5. the S19 loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.FIT_CASES))
def test_fit_loop_branches(name):
    """Outputs only, against N.planefit; which branch each case reaches is stated, from the restatement's trace, in test_planefit_cases.py."""
    w, h = K.FIT_CASES[name][:2]
    eng = engine(w, h)
    lab, xyz, mx = K.fit_case(name)
    e = K.fit_expected(name)
    lb, xb = place(lab, xyz, "both" if name in ("accepted_16", "cap_192") else "tight")
    pf = Obj(eng, mx)
    try:
        o = label_planes(pf, lb, xb, mx, FIT, e["seed"], e["frame"])
        check_label_planes(o, dict(planes=e["planes17"], npts=e["npts"], counts=e["counts"]))
        check_fit(run_fit(pf, lb, e["seed"], e["frame"], mx + 1), e["P"], e["A"])
        assert status(pf) == 0
    finally:
        pf.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every refusal of the eight entry points by its words, before anything is written; the same calls with good arguments work afterwards."""
    from cartslam import Engine, EngineError
    w, h = 67, 37
    eng, L = engine(w, h), lib()
    lab, xyz, mx = K.layout_scene(w, h)
    e = K.layout_expected(w, h, FIT)
    lb, xb = place(lab, xyz, "steps")
    L1, cap = mx + 1, min(8 * w * h, (mx + 1) * mx)
    total = int(e["off"][-1])
    planes, npts, counts = sentinel(L1 * 4, np.float64, SD), sentinel(L1, np.int32, S32), sentinel(L1 * 2, np.int32, S32)
    pts, off = sentinel(total * 4, np.float32, SF), sentinel(L1 + 1, np.int32, S32)
    aoff, anb = sentinel(L1 + 1, np.int32, S32), sentinel(cap, np.int32, S32)
    fplanes, fassign, fn = sentinel(400, np.float64, SD), sentinel(L1, np.uint64, S64), sentinel(1, np.int32, S32)

    # create.  A size whose sampling grid has more than 64 slots (11 x 9), or a grid step of 0 (w < 6, h < 5), is no engine's size
    made = C.c_void_p()
    refused(L.cart_planefit_create(None, 10, C.byref(made)), "bad arguments")
    refused(L.cart_planefit_create(eng._h, 10, None), "bad arguments")
    for bad in (-1, 16384):
        refused(L.cart_planefit_create(eng._h, bad, C.byref(made)), "max_label_capacity must be in [0, 16383]")
    assert not made.value
    for size in ((11, 9), (5, 40), (96, 4)):
        with pytest.raises(EngineError, match="unsupported image size"):
            Engine(*size, num_disparities=0, paths=0)

    pf = Obj(eng, mx)
    good = dict(pf=pf.h, labels=lb.ptr, ls=lb.step, mx=mx, xyz=xb.ptr, xs=xb.step, pred=FIT, thr=0.01)

    def lp(**kw):
        a = dict(good, **kw)
        return L.cart_planefit_label_planes(a["pf"], a["labels"], a["ls"], a["mx"], a["xyz"], a["xs"], a["pred"], a["thr"], e["seed"], e["frame"],
                                            planes.ptr, npts.ptr, counts.ptr, None)

    def points(pf_=pf.h, p=pts.ptr, capacity=total, o=off.ptr):
        return L.cart_planefit_points(pf_, p, capacity, o, None)

    def adjacency(**kw):
        a = dict(good, off=aoff.ptr, nb=anb.ptr, cap=cap)
        a.update(kw)
        return L.cart_planefit_adjacency(a["pf"], a["labels"], a["ls"], a["mx"], a["off"], a["nb"], a["cap"], None)

    def fit(**kw):
        a = dict(good, planes=fplanes.ptr, assign=fassign.ptr, n=fn.ptr)
        a.update(kw)
        return L.cart_planefit_fit(a["pf"], a["labels"], a["ls"], e["seed"], e["frame"], a["planes"], a["assign"], a["n"], None, None)

    def label_steps(call):
        refused(call(ls=2 * w - 2), "labels_step is below the row size")
        refused(call(ls=lb.step + 1), "labels and its step must be 2-byte aligned")
        refused(call(labels=lb.ptr + 1), "labels and its step must be 2-byte aligned")

    try:
        needs = "cart_planefit_fit needs a preceding label_planes call with CART_PLANE_PREDICATE_PLANEFIT"
        # before any label_planes call
        refused(points(), "no label_planes call yet")
        refused(fit(), needs)
        # label_planes
        refused(lp(pf=None), "planefit is NULL")
        refused(lp(labels=None), "NULL image pointer")
        refused(lp(xyz=None), "NULL image pointer")
        for bad in (-1, mx + 1):
            refused(lp(mx=bad), "max_label must be in [0, max_label_capacity]")
        refused(lp(pred=2), "unknown predicate")
        for bad in (0.0, -0.01, float("nan")):
            refused(lp(thr=bad), "thr must be positive")
        label_steps(lp)
        refused(lp(xs=12 * w - 4), "xyz_step is below the row size")
        refused(lp(xs=xb.step + 2), "xyz and its step must be 4-byte aligned")
        refused(lp(xyz=xb.ptr + 2), "xyz and its step must be 4-byte aligned")
        refused(points(), "no label_planes call yet")      # none of the refused calls counts as one
        # adjacency
        refused(adjacency(pf=None), "planefit is NULL")
        for name in ("labels", "off", "nb"):
            refused(adjacency(**{name: None}), "NULL pointer")
        for bad in (-1, mx + 1):
            refused(adjacency(mx=bad), "max_label must be in [0, max_label_capacity]")
        refused(adjacency(cap=cap - 1), "capacity must be >= min(8 * width * height, (max_label + 1) * max_label)")
        label_steps(adjacency)
        _torch().cuda.synchronize()
        for b in (planes, npts, counts, aoff, anb, fplanes, fassign, fn):
            assert b.untouched()
        # after a PLANECLUSTER label_planes call, fit is still refused; points works from here on
        ok(lp(pred=CLUSTER))
        refused(fit(), needs)
        ok(lp())
        # points
        refused(points(pf_=None), "planefit is NULL")
        refused(points(p=None), "NULL pointer")
        refused(points(o=None), "NULL pointer")
        refused(points(capacity=total - 1), "capacity is smaller than the number of points")
        # fit
        refused(fit(pf=None), "planefit is NULL")
        for name in ("labels", "planes", "assign", "n"):
            refused(fit(**{name: None}), "NULL pointer")
        label_steps(fit)
        # status
        bad = C.c_int(-1)
        refused(L.cart_planefit_status(None, C.byref(bad)), "bad arguments")
        refused(L.cart_planefit_status(pf.h, None), "bad arguments")
        assert bad.value == -1
        _torch().cuda.synchronize()
        for b in (pts, off, aoff, anb, fplanes, fassign, fn):
            assert b.untouched()
        # the same calls with good arguments
        check_label_planes(dict(planes=planes, npts=npts, counts=counts), e)
        ok(points())
        assert np.array_equal(off.image().ravel(), e["off"])
        assert np.array_equal(np.ascontiguousarray(pts.image().reshape(-1, 4)[:, :3]).view(np.uint32), e["pts"].view(np.uint32))
        ok(adjacency())
        assert np.array_equal(aoff.image().ravel(), e["aoff"]) and np.array_equal(anb.image().ravel()[:len(e["anb"])], e["anb"])
        ok(fit())
        check_fit((fplanes.image().reshape(100, 4), fassign.image().ravel(), int(fn.image().ravel()[0])), *e["fit"][:2])
        assert status(pf) == 0 and lb.untouched() and xb.untouched()
    finally:
        pf.close()

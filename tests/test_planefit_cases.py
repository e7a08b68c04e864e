"""CPU checks of the premises behind tests/test_gpu_planefit_layout.py: every case of tests/planefit_cases.py is what its name says, according
to the restatement (np_planefit.py) and its per-iteration trace.  The GPU tests compare the device with the same expected values; a case
that turned trivial (no plane, no neighbour, no iteration) would make those comparisons pass for nothing, and fails here first."""
import numpy as np
import pytest

import np_planefit as N
import planefit_cases as K


def nonzero(planes):
    return (np.asarray(planes) != 0).any(axis=-1)


# ---- section 1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", K.SIZES)
def test_layout_scenes(w, h):
    lab, xyz, mx = K.layout_scene(w, h)
    assert w % 64 != 0 and (w * h) % 1024 != 0 and w * h > 1024                     # chunks straddle rows, several tiles, the last partial
    fit, clu = K.layout_expected(w, h, N.PRED_PLANEFIT), K.layout_expected(w, h, N.PRED_PLANECLUSTER)
    assert (fit["npts"] < 16).any() and (fit["npts"] >= 16).sum() > 20 and nonzero(fit["planes"]).sum() > 20
    assert (fit["counts"][:, 1] > 0).any() and fit["off"][-1] < clu["off"][-1] < w * h      # NaN z: points for one predicate only; inf never
    assert (fit["planes"] != clu["planes"]).any()
    # what the slack holds would change the result: label 1 is in the image, has a plane, and the slack point is off it and has a valid z
    assert (lab == K.SLACK_LABEL).any() and nonzero(fit["planes"][K.SLACK_LABEL]) and N.valid_mask(np.float32(K.OFF[2]), N.PRED_PLANEFIT)
    assert N.dist_vec4(fit["planes"][K.SLACK_LABEL], np.array([K.OFF])) > 5
    assert fit["aoff"][-1] > 4 * mx and (np.diff(fit["aoff"]) >= 3).all()
    P, A, it = fit["fit"]
    decided = [s for s in fit["trace"] if s["votes"] is not None]
    assert it > 0 and decided, "the S19 loop runs and decides at least one iteration"
    if w >= 130:
        assert len(P) == 1 and (A == 1).sum() >= 16 and (A == 0).any()
    else:
        assert len(P) == 0 and all(0 < s["votes"] < 16 for s in decided)            # 67 x 37: every winner is rejected


# ---- section 2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L1", K.L1_VALUES)
def test_sparse_label_counts(L1):
    lab, xyz, mx = K.sparse_case(L1)
    e = K.sparse_expected(L1)
    ids = np.unique(lab)
    assert mx == L1 - 1 and ids[0] == 0 and ids[-1] == L1 - 1 and len(ids) == min(L1, len(ids)) and (L1 < 363 or len(ids) > 250)
    assert e["off"][-1] == K.BW * K.BH and nonzero(e["planes"]).any()
    if L1 > 1:
        assert e["aoff"][-1] > 0 and e["aoff"][-1] <= min(8 * K.BW * K.BH, L1 * (L1 - 1))
    else:
        assert e["aoff"][-1] == 0
    if L1 >= 2049:      # the second 64-word trip of the adjacency kernels
        sets = [e["anb"][e["aoff"][l]:e["aoff"][l + 1]] for l in range(L1)]
        assert any(len(q) and (q < 2048).any() and (q >= 2048).any() for q in sets), "a label with neighbours on both sides of id 2048"
        assert any(len(q) and (q >= 2048).all() for q in sets), "a label with all its neighbours at or above id 2048"


@pytest.mark.parametrize("n", K.POINT_COUNTS)
def test_point_counts_of_one_label(n):
    e = K.point_count_expected(n)
    assert e["npts"][7] == n and e["counts"][7].tolist() == [n + 3, 3]
    assert bool(nonzero(e["planes"][7])) == (n >= 16)
    assert (np.delete(e["npts"], 7) < 16).all()


def test_ransac_inputs_the_scene_generator_never_makes():
    lab, xyz, mx = K.ransac_case()
    L = K.RANSAC_LABELS
    fit, clu, wide, tiny = (K.ransac_expected(p, t) for p, t in K.RANSAC_RUNS)
    ordinary = [l for l in range(mx + 1) if l not in L.values()]
    for e in (fit, clu, wide):
        assert nonzero(e["planes"][ordinary]).all()
        for name in ("identical", "collinear"):      # >= 16 points and a zero plane: every hypothesis is degenerate
            l = L[name]
            assert e["npts"][l] >= 16 and not nonzero(e["planes"][l]) and e["best"][l] is None
            seg = e["pts"][e["off"][l]:e["off"][l + 1]].astype(np.float64)
            for h in range(N.ITERS):
                idx = N.hypothesis_indices(e["seed"], e["frame"], l, h, len(seg))
                assert N.plane_sequential([tuple(float(v) for v in seg[i]) for i in idx]) == K.ZERO
    # a threshold no hypothesis meets on noisy points: the count >= 1 rule
    assert tiny["npts"][L["noisy"]] >= 16 and tiny["best"][L["noisy"]] is None and not nonzero(tiny["planes"][L["noisy"]])
    # thr = 0.05 against 0.01: another inlier set, another plane
    l = L["noisy"]
    assert fit["best"][l][0] < wide["best"][l][0] < fit["npts"][l] and (fit["planes"][l] != wide["planes"][l]).any()
    # NaN / +inf / -inf in x or y beside a valid z: points under both predicates
    l = L["nonfinite"]
    for e in (fit, clu):
        seg = e["pts"][e["off"][l]:e["off"][l + 1]]
        assert np.isnan(seg[:, :2]).any() and np.isposinf(seg[:, :2]).any() and np.isneginf(seg[:, :2]).any() and np.isfinite(seg[:, 2]).all()
        assert nonzero(e["planes"][l]) and np.isfinite(e["planes"][l]).all()
    # NaN z: a point under PLANECLUSTER only
    l = L["nanz"]
    assert clu["npts"][l] > fit["npts"][l] >= 16 and np.isnan(clu["pts"][clu["off"][l]:clu["off"][l + 1], 2]).any()
    assert nonzero(clu["planes"][l]) and clu["best"][l][2] != fit["best"][l][2]      # other indices, another winning hypothesis


# ---- section 3 -----------------------------------------------------------------------------------------------------------
def test_labels_above_max_label():
    lab, xyz, low, mx = K.above_case()
    e = K.above_expected()
    full = K.layout_expected(K.BW, K.BH, N.PRED_PLANEFIT)
    assert low < mx and (lab > low).any() and (lab <= low).any()
    assert e["off"][-1] < full["off"][-1] and nonzero(e["planes"]).sum() > 10
    aoff, anb = N.adjacency(lab, mx)
    through = [l for l in range(low + 1) if (anb[aoff[l]:aoff[l + 1]] > low).any()]
    assert through, "in-range labels that touch an out-of-range one"
    assert (e["anb"] <= low).all() and all(e["aoff"][l + 1] - e["aoff"][l] < aoff[l + 1] - aoff[l] for l in through)


# ---- section 4 -----------------------------------------------------------------------------------------------------------
def test_reuse_sequence_changes_everything_between_calls():
    cases = [K.reuse_case(k) for k in range(len(K.REUSE_STEPS))]
    exp = [K.reuse_expected(k) for k in range(len(K.REUSE_STEPS))]
    assert [c[2] for c in cases] == [16383, 63, 2080, 0]
    for a, b in zip(exp, exp[1:]):
        assert a["off"][-1] != b["off"][-1] and a["mx"] != b["mx"]      # another point count and label count: stale lists would show
    assert all(nonzero(e["planes"]).any() for e in exp)
    assert exp[2]["fit"][2] > 0 and len(exp[2]["fit"][0]) > 0


# ---- section 5 -----------------------------------------------------------------------------------------------------------
def summary(name):
    e = K.fit_expected(name)
    tr = e["trace"]
    accepted = [(i, s["votes"]) for i, s in enumerate(tr) if s["accepted"]]
    rejected = [(i, s["votes"]) for i, s in enumerate(tr) if s["votes"] is not None and not s["accepted"]]
    return e, tr, accepted, rejected


def test_fit_no_iteration_at_ninety_percent_valid_regions():
    e, tr, accepted, _ = summary("all_valid")
    valid = (e["counts"][:, 1] < 0.5 * e["counts"][:, 0]).sum()
    assert valid / (e["mx"] + 1) >= 0.9 and e["it"] == 0 and not tr and len(e["P"]) == 0 and (e["A"] == 0).all()


def test_fit_early_ends():
    e, tr, accepted, _ = summary("one_iteration")
    assert e["it"] == 1 and len(e["P"]) == 1 and accepted[0][1] >= 16
    e, tr, accepted, _ = summary("early_end")
    assert e["it"] == 2 and len(e["P"]) == 2 and [i for i, _ in accepted] == [0, 1]


@pytest.mark.parametrize("name", ["cap_96", "cap_96_reseeded", "cap_192", "both", "collinear"])
def test_fit_two_planes_to_the_cap(name):
    e, tr, accepted, _ = summary(name)
    assert e["it"] == 100 and len(tr) == 100 and len(e["P"]) == 2 and all(v >= 16 for _, v in accepted)
    first, second = set(np.nonzero(e["A"] == 1)[0]), set(np.nonzero(e["A"] == 2)[0])
    assert len(first) == accepted[0][1] and len(second) == accepted[1][1] and not first & second
    assert any(s["local"] <= 3 for s in tr) and any(0 < s["local"] <= 3 for s in tr)      # skipped iterations that still sampled
    if name in ("cap_96", "cap_192"):
        # the second plane comes some iterations after the first: iterations in between sampled <= 3 unassigned labels.  A loop that sampled
        # assigned labels again would decide there, and take the second plane from another label
        assert accepted[1][0] - accepted[0][0] >= 6


def test_fit_other_seed_and_frame_change_the_run():
    a, b = K.fit_expected("cap_96"), K.fit_expected("cap_96_reseeded")
    assert (a["P"] != b["P"]).any() and (a["A"] != b["A"]).any()
    assert [s["labels"] for s in a["trace"]] != [s["labels"] for s in b["trace"]]


def test_fit_labels_that_fit_both_planes_stay_with_the_first():
    e, _, _, _ = summary("both")
    lab, xyz, mx = K.fit_case("both")
    for l in K.BOTH:
        assert e["A"][l] == 1 and K.accepts(lab, xyz, mx, e["P"][0], l) and K.accepts(lab, xyz, mx, e["P"][1], l)


def test_fit_winner_bound_of_sixteen_labels():
    e, tr, accepted, rejected = summary("rejected_12")
    assert len(e["P"]) == 2 and rejected and all(8 <= v <= 12 for _, v in rejected)
    e, tr, accepted, rejected = summary("rejected_15")
    assert len(e["P"]) == 2 and rejected and all(v == 15 for _, v in rejected)
    e, tr, accepted, rejected = summary("accepted_16")
    assert len(e["P"]) == 3 and accepted[2][1] == 16 and (e["A"] == 3).sum() == 16
    assert not set(np.nonzero(e["A"] == 3)[0]) & set(np.nonzero((e["A"] == 1) | (e["A"] == 2))[0])


def test_fit_at_most_three_local_planes_in_every_iteration():
    e, tr, accepted, rejected = summary("few_local")
    assert e["it"] == 100 and not accepted and not rejected and {s["local"] for s in tr} <= {0, 1, 2, 3} and any(s["local"] > 0 for s in tr)
    assert (e["npts"] >= 16).sum() == 2


def test_fit_samples_labels_with_a_zero_plane():
    e, tr, _, _ = summary("collinear")
    zero = [l for l in K.COLLINEAR if e["npts"][l] >= 16 and not nonzero(e["planes17"][l])]
    assert len(zero) == len(K.COLLINEAR)
    assert any(s["votes"] is not None and set(s["labels"]) & set(zero) for s in tr), "a zero plane among the local planes of a decided iteration"
    assert (e["A"][list(zero)] == 0).all()

"""CPU tests of spec S31, moving-object tracks from the motion components: the numpy restatement tests/np_objects.py
against its scalar twin and against hand-worked cases, the median, the band, Qp(), the gates, the selection, the tracker's sequences, the
accuracy of the spec on test_motion_spec's synthetic scene, and the library's host-side checks (no GPU: validation comes before any
device call).  tests/test_gpu_objects.py runs the cases built here on the device."""
import ctypes as C
import math

import numpy as np
import pytest

import np_motion as M
import np_objects as OB
import np_ref
import test_motion_spec as S

CAM = S.CAM   # (256, 256, 8, 4, 0.5): fx * baseline = 128


# ---- scene builders (shared with the GPU tests) ---------------------------------------------------------------------------------
def components(h, w, regions, max_components=64, fill=(0, 1, 1 << 20, 0, 0, 0, 0)):
    """regions = [(boolean mask, label)], disjoint -> (ids int32 [h, w] with -1 outside every region, table, count).  A region's id is its
    smallest linear index, as cart_plane_ccl_table numbers a component.  The table rows past the count hold an entry that WOULD be
    selected, so a walk past the count shows."""
    ids = np.full((h, w), -1, np.int32)
    labels = np.full((h, w), 2, np.uint8)
    for mask, label in regions:
        ids[mask] = np.flatnonzero(mask)[0]
        labels[mask] = label
    return (ids,) + OB.component_table(labels, ids, max_components, fill)


def rect(h, w, x0, y0, x1, y1):
    y, x = np.indices((h, w))
    return (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)


def grid_components(seed, w, h, cw=13, ch=7, max_components=4096):
    """The image cut into cw x ch cells, each a component of a random label (a third of them UNKNOWN: id -1)."""
    rng = np.random.default_rng(seed)
    regions = []
    for y0 in range(0, h, ch):
        for x0 in range(0, w, cw):
            label = int(rng.integers(0, 3))
            if label < 2:
                regions.append((rect(h, w, x0, y0, x0 + cw - 1, y0 + ch - 1), label))
    return components(h, w, regions, max_components)


def hand_case():
    """16 x 8, one 4 x 4 MOVING square at x = 6..9, y = 2..5 with d = 32, seen at d = 32 one pixel to the left in the previous frame."""
    h, w = 8, 16
    sq = rect(h, w, 6, 2, 9, 5)
    ids, table, n = components(h, w, [(sq, 1)])
    dc = np.full((h, w), 256, np.int16)
    dp = np.full((h, w), 256, np.int16)
    dc[sq] = 512
    dp[rect(h, w, 5, 2, 8, 5)] = 512
    fl = np.zeros((h, w, 2), np.int16)
    fl[sq, 0] = 32
    return ids, table, n, dc, dp, fl


def test_hand_worked_case():
    """CAM = (256, 256, 8, 4, 0.5): fx b = 128.  Every pixel of the square has s_c = 512: bin 512 >> 4 = 32, n_hist = 16, the cumulative
    count reaches (16 + 1) >> 1 = 8 in bin 32, so B = 32; |512 - (16 * 32 + 8)| = 8 <= band16 = 32: all 16 pixels are points.
    Z = 128 / 32 = 4, X = ((x - 8) * 4) / 256 = (x - 8) / 64, Y = (y - 4) / 64.  Qp(X) = 16 (x - 8) = -32, -16, 0, 16 for x = 6..9, the
    same for y = 2..5, Qp(Z) = 4096: sum = (4 * -32, 4 * -32, 16 * 4096) = (-128, -128, 65536), lo = (-32, -32, 4096), hi = (16, 16, 4096).
    c = ((sum / 1024) / 16) = (-1 / 128, -1 / 128, 4), the centroid under the identity pose; extent = (48 / 1024, 48 / 1024, 0).
    Flow +32 = one pixel: (xp, yp) = (x - 1, y), d_p = 32 there, so q = ((x - 9) / 64, Y, 4) and f = (1 / 64, 0, 0): |f|^2 <= 25.
    Qp(f) = (16, 0, 0), flow_sum = (256, 0, 0), v = ((256 / 1024) / 16, 0, 0) = (1 / 64, 0, 0)."""
    ids, table, n, dc, dp, fl = hand_case()
    p = OB.params(min_area=16)
    for fn in (OB.measure, OB.scalar_measure):
        out, n_selected, seen = fn(CAM, p, OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl, 4)[:3]
        o = out[0]
        assert (n_selected, seen) == (1, 1) and o["component"] == 2 * 16 + 6 and o["area"] == 16
        assert (o["median_bin"], o["n_hist"], o["n_points"], o["n_flow"]) == (32, 16, 16, 16)
        assert o["sum"].tolist() == [-128, -128, 65536] and o["lo"].tolist() == [-32, -32, 4096] and o["hi"].tolist() == [16, 16, 4096]
        assert (o["x0"], o["y0"], o["x1"], o["y1"]) == (6, 2, 9, 5)
        assert o["centroid"].tolist() == [-1 / 128, -1 / 128, 4.0] and o["extent"].tolist() == [48 / 1024, 48 / 1024, 0.0]
        assert o["flow_sum"].tolist() == [256, 0, 0] and o["velocity"].tolist() == [1 / 64, 0.0, 0.0]
        assert o["valid"] == 1 and o["has_velocity"] == 1
        assert out[1:].tobytes() == bytes(3 * 192)
    # a translated, yawed pose moves the centroid and turns the velocity; the velocity takes no translation
    pose = S.yaw_rel(90.0, (10.0, 20.0, 30.0))
    o = OB.measure(CAM, p, OB.IDENTITY, pose, ids, table, n, dc, dp, fl, 4)[0][0]
    c, s = pose[0], pose[2]
    assert o["centroid"].tolist() == [((c * (-1 / 128) + 0.0 * (-1 / 128)) + s * 4.0) + 10.0, -1 / 128 + 20.0, ((-s * (-1 / 128) + 0.0) + c * 4.0) + 30.0]
    assert o["velocity"].tolist() == [(c * (1 / 64) + 0.0) + s * 0.0, 0.0, (-s * (1 / 64) + 0.0) + c * 0.0]


def random_case(seed, w, h, big_flow=False, cells=(13, 7)):
    dc, dp, fl, _ = S.random_frame(seed, w, h, big_flow)
    ids, table, n = grid_components(seed + 1, w, h, *cells)
    return ids, table, n, dc, dp, fl


RANDOM_PARAMS = dict(min_area=8, min_points=4, disparity_band=1.0, max_speed=0.3)   # the band and the speed gate both refuse some pixels of S.random_frame


def premises(info):
    """A comparison says something only if every gate of S31 let pixels through and stopped some."""
    for k in ("pixels", "gate1", "band", "points", "flow", "gate234", "speed"):
        assert info[k] > 0, f"no pixel counted under {k}"


@pytest.mark.parametrize("w,h", [(5, 3), (23, 9), (40, 17), (67, 21)])
def test_vectorised_restatement_equals_the_scalar_loop(w, h):
    selected = 0
    for k, rel in enumerate((OB.IDENTITY, S.yaw_rel(2.0, (-0.05, 0.01, -0.2)), S.rel_t(tz=-9.0))):
        ids, table, n, dc, dp, fl = random_case(100 * w + k, w, h, big_flow=k == 1, cells=(3, 2) if w == 5 else (13, 7))
        p = OB.params(**dict(RANDOM_PARAMS, min_area=2 if w == 5 else 8, min_points=1 if w == 5 else 4))
        pose = S.yaw_rel(30.0 * k, (1.0, -2.0, 3.0 * k))
        a = OB.measure(CAM, p, rel, pose, ids, table, n, dc, dp, fl, 16)
        b = OB.scalar_measure(CAM, p, rel, pose, ids, table, n, dc, dp, fl, 16)
        assert a[1:3] == b[1:3] and a[0].tobytes() == b[0].tobytes(), k
        selected += a[1]
        if k == 0 and w >= 40:
            premises(a[3])
        if k == 2:
            assert a[3]["gate234"] > 0 and a[0]["n_flow"].sum() == 0     # every previous point lands behind the camera
    assert selected >= 1


def test_median_at_ties_and_odd_and_even_counts():
    def hist(**bins):
        hh = np.zeros(OB.BINS, np.int64)
        for k, v in bins.items():
            hh[int(k[1:])] = v
        return hh
    assert OB.median_bin(hist()) == (-1, 0)
    assert OB.median_bin(hist(b7=1)) == (7, 1)                       # target (1 + 1) >> 1 = 1
    assert OB.median_bin(hist(b3=1, b9=1)) == (3, 2)                 # even: target 1, the lower of the two
    assert OB.median_bin(hist(b3=1, b5=1, b9=1)) == (5, 3)           # odd: target 2, the middle
    assert OB.median_bin(hist(b3=2, b9=2)) == (3, 4)                 # a tie between two bins: the cumulative count reaches 2 in bin 3
    assert OB.median_bin(hist(b3=2, b9=3)) == (9, 5)                 # target 3
    assert OB.median_bin(hist(b0=5, b511=5)) == (0, 10) and OB.median_bin(hist(b0=5, b511=6)) == (511, 11)
    # through the measurement: s_c >> 4 and the clamp to bin 511
    h, w = 8, 16
    sq = rect(h, w, 0, 0, 15, 3)
    ids, table, n = components(h, w, [(sq, 1)])
    dc = np.full((h, w), 256, np.int16)
    dc[0, :], dc[1, :], dc[2, :], dc[3, :] = 511, 512, 32767, 8192     # bins 31, 32, clamp(2047) = 511, 512 -> 511
    _, _, fl = S.flat(h, w, 256, 256)
    for fn in (OB.measure, OB.scalar_measure):
        o = fn(CAM, OB.params(min_area=1), OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dc, fl, 2)[0][0]
        assert (o["median_bin"], o["n_hist"]) == (32, 64)             # cumulative 16, 32 >= (64 + 1) >> 1 = 32 in bin 32
        assert o["n_points"] == 16 + 16                               # |511 - 520| = 9 and |512 - 520| = 8 are inside the band, bin 511's pixels are not


def test_band_edges():
    """band16 = floor(2.0 * 16) = 32 around 16 B + 8: s_c = 16 B + 8 +- 32 is a point, one step further is not."""
    h, w = 8, 16
    sq = rect(h, w, 0, 0, 15, 7)
    ids, table, n = components(h, w, [(sq, 1)], fill=(0, 0, 0, 0, 0, 0, 0))
    _, _, fl = S.flat(h, w, 256, 256)
    dc = np.full((h, w), 16 * 20 + 8, np.int16)                       # B = 20 whatever the few others are
    dc[0, :8] = [16 * 20 + 8 + 32, 16 * 20 + 8 + 33, 16 * 20 + 8 - 32, 16 * 20 + 8 - 33, 16 * 20 + 8 + 31, 16 * 20 + 8 - 31, -32768, 15]
    for fn in (OB.measure, OB.scalar_measure):
        o = fn(CAM, OB.params(min_area=1), OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dc, fl, 2)[0][0]
        assert (o["median_bin"], o["n_hist"], o["n_points"]) == (20, 128 - 2, 128 - 4)
    assert OB.band16(OB.params(disparity_band=0.5)) == 8 and OB.band16(OB.params(disparity_band=2.04)) == 32 and OB.band16(OB.params(disparity_band=64.0)) == 1024
    o = OB.measure(CAM, OB.params(min_area=1, disparity_band=2.0625), OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dc, fl, 2)[0][0]
    assert o["n_points"] == 128 - 2                                    # band16 = 33 takes the two at +-33 in


def test_qp_rounding_clamp_and_nan():
    v = np.array([0.0, 1.0, -1.0, 0.5 / 1024, -0.5 / 1024, 1.5 / 1024, -1.5 / 1024, 2097151.999, 2097152.0, 1e300, -2097151.999, -2097152.0, -1e300, np.inf, -np.inf, np.nan])
    exp = [0, 1024, -1024, 1, 0, 2, -1, 2147483647, 2147483647, 2147483647, -2147483647, -2147483647, -2147483647, 2147483647, -2147483647, -2147483647]
    assert OB.qp(v).tolist() == exp and [OB._qp(float(x)) for x in v] == exp    # the .5 rounds up: floor(x + 0.5)
    assert OB.qp(np.array([2097151.5])).tolist() == [2147483136] and OB.qp(v).dtype == np.int64


def speed_case(tx):
    """The hand case's square with a still image (flow 0) under a camera translation t_x: f = (-t_x, 0, 0), |f| = |t_x|."""
    ids, table, n, dc, dp, fl = hand_case()
    dp = dc.copy()
    fl[:] = 0
    return ids, table, n, dc, dp, fl, S.rel_t(tx=tx)


def test_max_speed_at_equality():
    p = OB.params(min_area=16, max_speed=0.5)
    for tx, flows in ((0.5, 16), (0.5 + 2.0 ** -20, 0), (-0.5, 16), (0.25, 16)):
        ids, table, n, dc, dp, fl, rel = speed_case(tx)
        for fn in (OB.measure, OB.scalar_measure):
            o = fn(CAM, p, rel, OB.IDENTITY, ids, table, n, dc, dp, fl, 2)[0][0]
            assert (o["n_points"], o["n_flow"], o["has_velocity"]) == (16, flows, int(flows > 0)), tx
            assert o["velocity"].tolist() == ([-tx, 0.0, 0.0] if flows else [0.0, 0.0, 0.0])     # Qp(-t_x) is exact for these


def test_selection_order_overflow_and_a_truncated_table():
    h, w = 24, 64
    regions = [(rect(h, w, 8 * k, 0, 8 * k + 5, 5 + (k % 3)), k % 2) for k in range(8)]       # labels 0, 1, 0, 1, ...; areas 36, 42, 48, ...
    regions += [(rect(h, w, 8 * k, 12, 8 * k + 1, 13), 1) for k in range(8)]                  # small MOVING ones: area 4
    ids, table, n = components(h, w, regions, 64)
    assert n == 16
    dc, dp, fl = S.flat(h, w, 512, 512)
    p = OB.params(min_area=36, min_points=1)
    out, n_selected, seen, _ = OB.measure(CAM, p, OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl, 8)
    assert (n_selected, seen) == (4, 16) and out["component"][:4].tolist() == [8, 24, 40, 56] and out["area"][:4].tolist() == [42, 36, 48, 42]
    assert out["n_points"][:5].tolist() == [42, 36, 48, 42, 0]
    # max_objects = 2: objects 2 and 3 are dropped, n_selected keeps the count
    out2, n_selected, seen, _ = OB.measure(CAM, p, OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl, 2)
    assert n_selected == 4 and out2.tobytes() == out[:2].tobytes()
    # min_area at equality, and one above
    assert OB.select(table, n, OB.params(min_area=42), 8)[1] == 3 and OB.select(table, n, OB.params(min_area=43), 8)[1] == 1
    assert OB.select(table, n, OB.params(min_area=4), 8)[1] == 12
    # a truncated table: max_components = 3 rows hold ids 0, 8, 16; the true count does not widen the walk, the roots without an entry belong to no object
    out3, n_selected, seen, _ = OB.measure(CAM, p, OB.IDENTITY, OB.IDENTITY, ids, table[:3], n, dc, dp, fl, 8)
    assert (n_selected, seen) == (1, 3) and out3["component"][:2].tolist() == [8, 0] and out3[:1].tobytes() == out[:1].tobytes()
    # a count below the table's rows stops the walk before the filler entry, which would be selected; a negative count walks nothing
    assert OB.select(table, 16, p, 8)[1] == 4 and OB.select(table, 17, p, 8)[1] == 5 and OB.select(table, -3, p, 8)[1:] == (0, 0)
    scalar = OB.scalar_measure(CAM, p, OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl, 8)
    assert scalar[0].tobytes() == out.tobytes()


def test_an_object_without_a_valid_disparity():
    ids, table, n, dc, dp, fl = hand_case()
    dc[ids >= 0] = -32768
    dc[2, 6] = 15                                                     # below min_disparity
    for fn in (OB.measure, OB.scalar_measure):
        o = fn(CAM, OB.params(min_area=16), OB.IDENTITY, OB.IDENTITY, ids, table, n, dc, dp, fl, 2)[0][0]
        assert (o["median_bin"], o["n_hist"], o["n_points"], o["valid"], o["x0"], o["y0"], o["x1"], o["y1"]) == (-1, 0, 0, 0, 0, 0, -1, -1)
        assert o["lo"].tolist() == [0, 0, 0] and o["centroid"].tolist() == [0.0, 0.0, 0.0]


# ---- the tracker ---------------------------------------------------------------------------------------------------------------------
def objects(*rows, n=8):
    """rows = (centroid, velocity or None[, valid]) -> OBJECT_DTYPE [n]"""
    out = np.zeros(n, OB.OBJECT_DTYPE)
    for j, row in enumerate(rows):
        c, v = row[0], row[1]
        out[j]["component"], out[j]["centroid"], out[j]["valid"] = 100 + j, c, row[2] if len(row) > 2 else 1
        out[j]["extent"] = (1.0 + j, 2.0, 3.0)
        if v is not None:
            out[j]["velocity"], out[j]["has_velocity"] = v, 1
    return out, len(rows)


def test_tracker_birth_match_and_the_velocity_blend():
    p = OB.params(gain_percent=25, min_age=3)
    tr = OB.Tracker(8, 4)
    assert tr.associate(*objects(((1.0, 2.0, 3.0), (0.5, 0.0, 0.0)), ((9.0, 9.0, 9.0), None)), p) == (2, 0, 2, 0, 2)
    a, b = tr.tracks[0], tr.tracks[1]
    assert (a["id"], a["state"], a["age"], a["missed"], a["object"], a["component"]) == (1, 1, 1, 0, 0, 100) and (b["id"], b["object"], b["component"]) == (2, 1, 101)
    assert a["position"].tolist() == [1.0, 2.0, 3.0] and a["velocity"].tolist() == [0.5, 0.0, 0.0] and b["velocity"].tolist() == [0.0, 0.0, 0.0]
    assert a["extent"].tolist() == [1.0, 2.0, 3.0] and (tr.tracks["state"][2:] == 0).all() and tr.next_id == 3
    # frame 2: object 0 is track 2's (no velocity: m = centroid - old position), object 1 is track 1's (m = its velocity)
    assert tr.associate(*objects(((9.5, 9.0, 10.0), None), ((1.25, 2.0, 3.0), (1.5, 0.25, 0.0))), p) == (2, 2, 0, 0, 2)
    a, b = tr.tracks[0], tr.tracks[1]
    assert (a["object"], a["age"], a["state"], b["object"], b["age"]) == (1, 2, 1, 0, 2)
    assert a["velocity"].tolist() == [0.5 + 0.25 * (1.5 - 0.5), 0.0 + 0.25 * 0.25, 0.0] and a["position"].tolist() == [1.25, 2.0, 3.0]
    assert b["velocity"].tolist() == [0.25 * 0.5, 0.0, 0.25 * 1.0] and b["extent"].tolist() == [1.0, 2.0, 3.0] and a["extent"].tolist() == [2.0, 2.0, 3.0]
    # frame 3: confirmed at age 3 = min_age; the prediction, not the position, is what the gate is measured from
    pred = [1.25 + 0.75, 2.0 + 0.0625, 3.0]
    assert tr.associate(*objects(((pred[0] + 2.0, pred[1], pred[2]), None)), p) == (1, 1, 0, 0, 2)      # d2 = 4 = gate^2: admissible
    assert (tr.tracks[0]["state"], tr.tracks[0]["age"], tr.tracks[1]["missed"], tr.tracks[1]["object"], tr.tracks[1]["component"]) == (2, 3, 1, -1, -1)
    tr.reset()
    assert tr.tracks.tobytes() == OB.free_tracks(4).tobytes() and tr.next_id == 1
    # gain 0 keeps the velocity, gain 100 replaces it; min_age 1 confirms at birth
    for gain, exp in ((0, 0.5), (100, 2.0)):
        tr = OB.Tracker(8, 4)
        q = OB.params(gain_percent=gain, min_age=1)
        tr.associate(*objects(((0.0, 0.0, 0.0), (0.5, 0.0, 0.0))), q)
        assert tr.tracks[0]["state"] == 2
        tr.associate(*objects(((0.5, 0.0, 0.0), (2.0, 0.0, 0.0))), q)
        assert tr.tracks[0]["velocity"][0] == exp


def test_tracker_gate_coasting_death_and_slot_reuse():
    p = OB.params(max_missed=2, gate=1.0)
    tr = OB.Tracker(8, 2)
    tr.associate(*objects(((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)), ((50.0, 0.0, 0.0), None)), p)
    # just outside the gate of track 1's prediction (1, 0, 0): no match, and no free slot for the object either
    assert tr.associate(*objects(((2.0 + 2.0 ** -40, 0.0, 0.0), None)), p) == (1, 0, 0, 1, 2)
    assert tr.tracks[0]["position"].tolist() == [1.0, 0.0, 0.0] and tr.tracks["missed"].tolist() == [1, 1]
    assert tr.associate(*objects(n=8), p) == (0, 0, 0, 0, 2)
    assert tr.tracks[0]["position"].tolist() == [2.0, 0.0, 0.0] and tr.tracks["missed"].tolist() == [2, 2] and tr.tracks["id"].tolist() == [1, 2]
    # the third miss is max_missed + 1: both die, and the frame's objects take the slots freed in this very frame, with new ids
    assert tr.associate(*objects(((7.0, 7.0, 7.0), None), ((0.0, 0.0, 0.0), None, 0), ((8.0, 8.0, 8.0), None), ((9.0, 9.0, 9.0), None)), p) == (3, 0, 2, 1, 2)
    assert tr.tracks["id"].tolist() == [3, 4] and tr.tracks["object"].tolist() == [0, 2] and tr.tracks["age"].tolist() == [1, 1] and tr.next_id == 5
    # max_missed = 0: one miss kills
    tr = OB.Tracker(8, 2)
    q = OB.params(max_missed=0)
    tr.associate(*objects(((0.0, 0.0, 0.0), None)), q)
    assert tr.associate(*objects(n=8), q) == (0, 0, 0, 0, 0) and tr.tracks.tobytes() == OB.free_tracks(2).tobytes()
    tr.associate(*objects(((0.0, 0.0, 0.0), None)), q)
    assert tr.tracks[0]["id"] == 2                                     # ids never repeat


def test_tracker_greedy_order_and_ties():
    p = OB.params(gate=10.0)
    tr = OB.Tracker(8, 4)
    tr.associate(*objects(((0.0, 0.0, 0.0), None), ((4.0, 0.0, 0.0), None), ((0.0, 100.0, 0.0), None)), p)
    # object 0 at x = 3 is nearest to track 2 (d2 = 1) although track 1 could take it (d2 = 9); track 1 then gets object 1 at x = -1 (d2 = 1)
    tr.associate(*objects(((3.0, 0.0, 0.0), None), ((-1.0, 0.0, 0.0), None)), p)
    assert tr.tracks["object"].tolist() == [1, 0, -1, -1]
    # the smallest d2 goes first even when it starves another pair: objects at x = 1.5 (d2 6.25 / 6.25 from tracks at -1, 4) ...
    tr = OB.Tracker(8, 4)
    tr.associate(*objects(((0.0, 0.0, 0.0), None), ((2.0, 0.0, 0.0), None)), p)
    # ties: object 0 at x = 1 is at d2 = 1 from both tracks -> the smaller slot; then slot 2 takes object 1 (d2 = 4) over nothing
    tr.associate(*objects(((1.0, 0.0, 0.0), None), ((4.0, 0.0, 0.0), None)), p)
    assert tr.tracks["object"].tolist() == [0, 1, -1, -1]
    # one track, two objects at the same d2 -> the smaller object index; the other is born
    tr = OB.Tracker(8, 4)
    tr.associate(*objects(((0.0, 0.0, 0.0), None)), p)
    assert tr.associate(*objects(((0.0, 1.0, 0.0), None), ((1.0, 0.0, 0.0), None)), p) == (2, 1, 1, 0, 2)
    assert tr.tracks["object"].tolist() == [0, 1, -1, -1] and tr.tracks["id"].tolist() == [1, 2, 0, 0]
    # an invalid object is neither matched nor born
    tr = OB.Tracker(8, 4)
    assert tr.associate(*objects(((0.0, 0.0, 0.0), None, 0)), p) == (0, 0, 0, 0, 0)


def test_tracker_full_table_drops_and_counts():
    tr = OB.Tracker(8, 3)
    rows = [((10.0 * k, 0.0, 0.0), None) for k in range(5)]
    assert tr.associate(*objects(*rows), OB.params()) == (5, 0, 3, 2, 3)
    assert tr.tracks["id"].tolist() == [1, 2, 3] and tr.next_id == 4
    assert tr.associate(*objects(*rows), OB.params()) == (5, 3, 0, 2, 3)


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------
_ACCURACY = []


def accuracy_inputs():
    """test_motion_spec.accuracy_scene() through np_motion.segment and np_ref.ccl -> (cam, rel, ids, table, count, disp_cur, disp_prev, flow)"""
    if not _ACCURACY:
        (cam, mp, rel, dc, dp, fl), _, _ = S.accuracy_scene()
        labels = M.segment(cam, mp, rel, dc, dp, fl)["labels"]
        ids, _ = np_ref.ccl(labels)
        table, n = OB.component_table(labels, ids, 64)
        _ACCURACY.append((cam, rel, ids, table, n, dc, dp, fl))
    return _ACCURACY[0]


CENTROID_BOUND, FLOW_BOUND = 2 * 0.005133, 2 * 0.002061   # test_accuracy_on_the_synthetic_scene's docstring derives them


def test_accuracy_on_the_synthetic_scene():
    """The scene's one MOVING component is the rectangle (x 60..99) plus the occlusion rim to its right (x 100..105, background at Z = 8).
    The noise-free rectangle has the camera-frame centroid (1.1172, 0.7109, 4.0) and the mean flow (-0.3203, -0.1016, -0.5714): the
    means over x = 60..99, y = 30..69 of the point at d = 32 minus the point at d = 28 two pixels to the right carried through t_x = 1/8.
    Measured on the restatement at the defaults: 1451 points, box x 60..99; centroid (1.1183, 0.7061, 4.0013), 0.005133 m from the
    ideal; mean flow (-0.3199, -0.1005, -0.5697), 0.002061 m per frame from the ideal.  Each bound sits at twice the measured distance
    (0.010266 m and 0.004122 m per frame), so that the measured value lies half-way between the bound and the ideal."""
    cam, rel, ids, table, n, dc, dp, fl = accuracy_inputs()
    out, n_selected, _, info = OB.measure(cam, OB.params(), rel, OB.IDENTITY, ids, table, n, dc, dp, fl, 8)
    assert n_selected == 1 and out["valid"].tolist() == [1] + [0] * 7
    o = out[0]
    assert (o["x0"], o["x1"]) == (60, 99) and table[table[:, 1] == 1][0, 5] == 105 and info["band"] > 100     # the rim is in the component and not in the object
    y, x = np.mgrid[30:70, 60:100].astype(np.float64)
    Z, Zp = 128.0 / 32.0, 128.0 / 28.0
    ideal_c = np.array([((x - 8.0) * Z / 256.0).mean(), ((y - 4.0) * Z / 256.0).mean(), Z])
    ideal_f = ideal_c - np.array([((x + 2.0 - 8.0) * Zp / 256.0).mean() + 0.125, ((y - 4.0) * Zp / 256.0).mean(), Zp])
    assert np.allclose(ideal_c, (1.1172, 0.7109, 4.0), atol=5e-5) and np.allclose(ideal_f, (-0.3203, -0.1016, -0.5714), atol=5e-5)
    dc_, df_ = float(np.linalg.norm(o["centroid"] - ideal_c)), float(np.linalg.norm(o["velocity"] - ideal_f))
    print(f"centroid {o['centroid']} off by {dc_:.6f} m, flow {o['velocity']} off by {df_:.6f} m per frame, {o['n_points']} points")
    assert dc_ <= CENTROID_BOUND and df_ <= FLOW_BOUND


def test_two_frames_of_the_tracker_on_the_synthetic_scene():
    """The same measurement twice is an object that stood still in the world although its velocity says otherwise: the prediction misses
    by exactly |velocity| = 0.66 m, inside the 2 m gate, and the track is kept; the blended velocity is the same again."""
    cam, rel, ids, table, n, dc, dp, fl = accuracy_inputs()
    tr = OB.Tracker(8, 8)
    first = tr.update(cam, OB.params(), rel, OB.IDENTITY, ids, table, n, dc, dp, fl)
    assert first["counts"].tolist() == [n, 1, 1, 1, 0, 1, 0, 1]
    t = first["tracks"][0]
    pred = t["position"] + t["velocity"]
    second = tr.update(cam, OB.params(), rel, OB.IDENTITY, ids, table, n, dc, dp, fl)
    miss = float(np.linalg.norm(second["objects"][0]["centroid"] - pred))
    print(f"the prediction misses by {miss:.4f} m")
    assert miss <= OB.DEFAULTS["gate"] and abs(miss - float(np.linalg.norm(t["velocity"]))) < 1e-12
    assert second["counts"].tolist() == [n, 1, 1, 1, 1, 0, 0, 1]
    u = second["tracks"][0]
    assert (u["id"], u["age"], u["state"], u["object"]) == (1, 2, 1, 0) and u["velocity"].tolist() == t["velocity"].tolist()


# ---- the library's host side -----------------------------------------------------------------------------------------------------
def test_defaults_struct_sizes_and_exports():
    import cartslam
    from cartslam import _lib
    lib = _lib.load()
    p = _lib.ObjectParams()
    lib.cart_object_default_params(C.byref(p))
    assert {n: getattr(p, n) for n, _ in p._fields_} == OB.DEFAULTS
    assert C.sizeof(_lib.ObjectParams) == 56 and C.sizeof(_lib.Object) == 192 and C.sizeof(_lib.Track) == 96
    assert cartslam.OBJECT_DTYPE == OB.OBJECT_DTYPE and cartslam.TRACK_DTYPE == OB.TRACK_DTYPE
    for f, off in (("lo", 40), ("sum", 64), ("centroid", 112), ("valid", 184)):
        assert getattr(_lib.Object, f).offset == off == OB.OBJECT_DTYPE.fields[f][1]
    assert _lib.Track.position.offset == 24 == OB.TRACK_DTYPE.fields["position"][1]
    assert (_lib.OBJECT_BINS, _lib.OBJECT_MAX_OBJECTS, _lib.OBJECT_MAX_TRACKS) == (OB.BINS, 256, 256)
    for name in ("ObjectParams", "ObjectTracker", "ObjectTracks", "object_params", "OBJECT_DTYPE", "TRACK_DTYPE"):
        assert hasattr(cartslam, name), name
    lib.cart_object_default_params(None)                              # a NULL is ignored


def test_object_params_replaces_named_fields_only():
    from cartslam import object_params
    assert object_params(gate=3.5, min_age=7).gate == 3.5 and object_params(min_age=7).min_age == 7 and object_params(min_age=7).gate == 2.0
    with pytest.raises(ValueError) as err:
        object_params(nope=1)
    assert str(err.value) == "cart_object_params has no field nope"


def lib_error(cam=CAM, rel=OB.IDENTITY, pose=OB.IDENTITY, p=None, w=16, h=8, max_components=64, params_null=False):
    from cartslam import _lib, object_params
    lib = _lib.load()
    c = _lib.EgoCamera(*[cam[k] for k in ("fx", "fy", "cx", "cy", "baseline")]) if cam is not None else None
    op = object_params(**(p or {}))
    arr = lambda m: (C.c_double * 12)(*m) if m is not None else None   # noqa: E731
    rc = lib.cart_object_tracker_update(None, C.byref(c) if c is not None else None, arr(rel), arr(pose), None if params_null else C.byref(op), None, 0, None,
                                        max_components, None, None, 0, None, 0, None, 0, w, h, None, None, None, None)
    assert rc != 0
    return lib.cart_last_error(None).decode()


def test_argument_checks_that_need_no_device():
    """Values and sizes come before the object: a valid configuration gets as far as `bad arguments`, everything else names its argument."""
    from cartslam import _lib
    assert lib_error() == "bad arguments"
    assert lib_error(params_null=True) == "params is NULL"
    nan, inf = float("nan"), float("inf")
    for p, word in ((dict(min_disparity=0.0), "min_disparity must be a positive number"), (dict(min_disparity=nan), "min_disparity"),
                    (dict(disparity_band=0.49), "disparity_band must be in [0.5, 64]"), (dict(disparity_band=64.5), "disparity_band"), (dict(disparity_band=nan), "disparity_band"),
                    (dict(max_speed=0.0), "max_speed must be a positive number"), (dict(max_speed=inf), "max_speed"), (dict(gate=-1.0), "gate must be a positive number"),
                    (dict(min_area=0), "min_area must be in [1, 2^30]"), (dict(min_area=(1 << 30) + 1), "min_area"), (dict(min_points=0), "min_points must be in [1, 2^30]"),
                    (dict(gain_percent=-1), "gain_percent must be in [0, 100]"), (dict(gain_percent=101), "gain_percent"), (dict(max_missed=-1), "max_missed must be in [0, 255]"),
                    (dict(max_missed=256), "max_missed"), (dict(min_age=0), "min_age must be in [1, 255]"), (dict(min_age=256), "min_age")):
        assert word in lib_error(p=p), p
    for p in (dict(disparity_band=0.5), dict(disparity_band=64.0), dict(gain_percent=0), dict(gain_percent=100), dict(max_missed=0), dict(max_missed=255),
              dict(min_age=1), dict(min_age=255), dict(min_area=1 << 30), dict(min_points=1 << 30)):
        assert lib_error(p=p) == "bad arguments", p
    assert lib_error(cam=None) == "camera is NULL" and "fx" in lib_error(cam=M.camera(0.0, 256.0, 8.0, 4.0, 0.5))
    assert lib_error(rel=None) == "rel is NULL" and lib_error(pose=None) == "pose is NULL"
    bad = list(OB.IDENTITY)
    bad[5] = nan
    assert "rel[5]" in lib_error(rel=bad) and "pose[5]" in lib_error(pose=bad)
    bad[5], bad[7] = 1.0, 2e6
    assert "pose[7] must be finite and within 1e6 (translation)" in lib_error(pose=bad)
    assert "width must be in [1, 16384]" in lib_error(w=0) and "height must be in [1, 16384]" in lib_error(h=16385)
    assert "max_components" in lib_error(max_components=0)
    # params come before the camera, the camera before the poses, the poses before the sizes
    assert "min_age" in lib_error(p=dict(min_age=0), cam=None) and lib_error(cam=None, rel=None) == "camera is NULL" and lib_error(rel=None, w=0) == "rel is NULL"
    # create: the sizes before the engine
    lib, out = _lib.load(), C.c_void_p()
    for args, word in (((0, 8, 4, 4), "max_width must be in [1, 16384]"), ((16, 16385, 4, 4), "max_height"), ((16, 8, 0, 4), "max_objects must be in [1, 256]"),
                       ((16, 8, 257, 4), "max_objects"), ((16, 8, 4, 0), "max_tracks must be in [1, 256]"), ((16, 8, 4, 257), "max_tracks"), ((16, 8, 256, 256), "bad arguments")):
        assert lib.cart_object_tracker_create(None, *args, C.byref(out)) != 0 and word in lib.cart_last_error(None).decode(), args
    assert lib.cart_object_tracker_reset(None, None) != 0 and lib.cart_last_error(None).decode() == "bad arguments"
    lib.cart_object_tracker_destroy(None)                             # a NULL is ignored
    assert math.isfinite(OB.DEFAULTS["gate"])

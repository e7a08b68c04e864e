"""CPU tests of the stereo visual odometry spec S23: the numpy restatement tests/np_ego.py against checks that do
not share its code -- numpy's linear algebra, finite differences, hand-built tables -- and its accuracy on a synthetic scene."""
import math

import numpy as np

import np_ego as E


def rotation(axis, deg):
    """Rodrigues' formula (independent of the restatement's quaternion)."""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(deg)
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def rot_err_deg(R, Rt):
    c = (np.trace(np.asarray(R).reshape(3, 3) @ Rt.T) - 1) / 2
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


CAM = E.camera(fx=300.0, fy=300.0, cx=160.0, cy=120.0, baseline=0.5)


def scene(seed, n=40, quant=4.0, shuffled=0.3, deg=2.0, step=0.6):
    """n points at Z in [4, 30] seen by a stereo rig before and after a motion of about `deg` degrees and `step` metres; the
    observations are rounded to 1 / quant pixels (quant = 0: exact, float64 keypoints are not representable so the landmarks are
    made directly), and a fraction `shuffled` of the temporal pairs is permuted among themselves.
    -> (cur landmarks, cur keypoints, prev landmarks, temporal matches, R, t, indices of the unshuffled matches)"""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(4, 30, n)
    P = np.stack([rng.uniform(-0.45, 0.45, n) * Z, rng.uniform(-0.3, 0.3, n) * Z, Z], 1)
    R = rotation(rng.normal(size=3), deg)
    t = rng.normal(size=3)
    t = step * t / np.linalg.norm(t)
    Q = P @ R.T + t

    def observe(X):
        kl, kr = np.zeros(n, E.KEYPOINT_DTYPE), np.zeros(n, E.KEYPOINT_DTYPE)
        u = CAM["fx"] * X[:, 0] / X[:, 2] + CAM["cx"]
        v = CAM["fy"] * X[:, 1] / X[:, 2] + CAM["cy"]
        d = CAM["fx"] * CAM["baseline"] / X[:, 2]
        kl["x"], kl["y"], kr["x"], kr["y"] = (np.round(a * quant) / quant for a in (u, v, u - d, v))
        return kl, kr

    ident = np.zeros(n, E.MATCH_DTYPE)
    ident["query"] = ident["train"] = np.arange(n)
    if quant:
        kpl, kpr = observe(P)
        kcl, kcr = observe(Q)
        prev, cur = E.triangulate(CAM, kpl, kpr, ident), E.triangulate(CAM, kcl, kcr, ident)
    else:
        kcl = np.zeros(n, E.KEYPOINT_DTYPE)
        prev, cur = np.concatenate([P, np.ones((n, 1))], 1), np.concatenate([Q, np.ones((n, 1))], 1)
    temporal = ident.copy()
    bad = rng.choice(n, int(round(shuffled * n)), replace=False)
    if len(bad):
        temporal["train"][bad] = np.roll(temporal["train"][bad], 1)
    good = np.setdiff1d(np.arange(n), bad)
    return cur, kcl, prev, temporal, R, t, good


def test_draws_are_distinct_and_in_range():
    for n in (3, 4, 5, 64, 1000):
        seen = set()
        for h in range(200):
            idx = E.sample(7, 11, h, n)
            assert idx is not None and len(set(idx)) == 3 and all(0 <= v < n for v in idx)
            seen.add(tuple(idx))
        assert len(seen) > (1 if n == 3 else 3)
    assert E.sample(7, 11, 0, 1000) != E.sample(7, 12, 0, 1000) and E.sample(7, 11, 0, 1000) != E.sample(8, 11, 0, 1000)
    assert E.sample(0, 0, 0, 2) is None   # two points never give three distinct indices: the draw budget ends the search


def test_triad_maps_its_sample_points_and_recovers_an_exact_motion():
    worst_R = worst_t = worst_map = 0.0
    for seed in range(20):
        cur, _, prev, _, R, t, _ = scene(seed, quant=0, shuffled=0)
        idx = E.sample(seed, 1, 0, len(cur))
        fit = E.fit_triad(prev[idx, :3], cur[idx, :3])
        assert fit is not None
        Rh, th = np.array(fit[0]).reshape(3, 3), np.array(fit[1])
        worst_map = max(worst_map, np.abs(prev[idx, :3] @ Rh.T + th - cur[idx, :3]).max())
        worst_R = max(worst_R, np.abs(Rh - R).max())
        worst_t = max(worst_t, np.abs(th - t).max())
        assert np.abs(Rh.T @ Rh - np.eye(3)).max() < 1e-14
    # measured over these seeds: map 7.1e-15, R 4.4e-16, t 9.5e-15 (points up to 30 m away); bounds = four times the measured values
    assert worst_map < 2.9e-14 and worst_R < 1.8e-15 and worst_t < 3.9e-14, (worst_map, worst_R, worst_t)


def test_degenerate_samples_are_skipped():
    p = np.array([[1.0, 2.0, 5.0], [2.0, 2.5, 6.0], [0.5, 4.0, 9.0]])
    assert E.fit_triad(p, p) is not None
    assert E.fit_triad(p[[0, 0, 2]], p) is None                                   # coincident
    line = np.array([[0.0, 0.0, 4.0], [1.0, 1.0, 5.0], [3.0, 3.0, 7.0]])
    assert E.fit_triad(line, p) is None and E.fit_triad(p, line) is None          # collinear on either side


def test_quaternion_update_is_a_rotation():
    rng = np.random.default_rng(3)
    for _ in range(50):
        w = rng.normal(size=3) * rng.choice([1e-6, 1e-2, 1.0])
        Rq = np.array(E.quat_rotation(list(w))).reshape(3, 3)
        assert np.abs(Rq.T @ Rq - np.eye(3)).max() < 1e-15 * 4 and abs(np.linalg.det(Rq) - 1) < 1e-15 * 8
        ang = 2 * math.atan(np.linalg.norm(w) / 2)               # the update's angle; axis = w
        assert np.abs(Rq - rotation(w, math.degrees(ang))).max() < 1e-14


def test_jacobian_agrees_with_central_differences():
    cur, kp, prev, temporal, R, t, _ = scene(5, quant=4.0, shuffled=0)
    a, _, uv, _ = E.correspondences(cur, kp, prev, temporal)
    R0, t0 = list(R.ravel()), list(t)
    q, _, _, _, _ = E.residuals(CAM, R0, t0, a, uv, 1e9)
    Ju, Jv = E.jacobian(CAM, q)
    h = 1e-6
    for k in range(6):
        d = [0.0] * 6
        e = []
        for s in (h, -h):
            d[k] = s
            if k < 3:   # an exact rotation about axis k by angle s, not the quaternion step (they agree to O(s^3))
                Rs = rotation(np.eye(3)[k], math.degrees(s)) @ R
                ts = rotation(np.eye(3)[k], math.degrees(s)) @ t
            else:
                Rs, ts = R, t + np.eye(3)[k - 3] * s
            _, eu, ev, _, _ = E.residuals(CAM, list(Rs.ravel()), list(ts), a, uv, 1e9)
            e.append((eu, ev))
        du, dv = (e[0][0] - e[1][0]) / (2 * h), (e[0][1] - e[1][1]) / (2 * h)
        scale = max(np.abs(Ju[k]).max(), np.abs(Jv[k]).max(), 1.0)
        assert np.abs(du - Ju[k]).max() < 1e-6 * scale and np.abs(dv - Jv[k]).max() < 1e-6 * scale, k


def test_solve6_against_numpy():
    rng = np.random.default_rng(4)
    for _ in range(20):
        J = rng.normal(size=(30, 6))
        H, g = J.T @ J, rng.normal(size=6)
        x = E.solve6([list(r) for r in np.triu(H)], list(g))
        assert np.abs(np.array(x) - np.linalg.solve(H, -g)).max() < 1e-10
    assert E.solve6([[0.0] * 6 for _ in range(6)], [1.0] * 6) is None
    bad = np.eye(6)
    bad[3, 3] = -1.0
    assert E.solve6([list(r) for r in bad], [1.0] * 6) is None


def test_lane_sum_is_the_fixed_order():
    rng = np.random.default_rng(6)
    v = rng.normal(size=1000) * 10.0 ** rng.integers(-8, 8, 1000)
    m = rng.random(1000) < 0.6
    lanes = [0.0] * 256
    for c in range(1000):
        if m[c]:
            lanes[c % 256] += float(v[c])
    o = 128
    while o:                                    # lane 0 of the butterfly is the plain halving tree
        lanes = [lanes[l] + lanes[l + o] for l in range(o)]
        o //= 2
    assert E.lane_sum(v, m) == lanes[0]
    assert abs(E.lane_sum(v, m) - math.fsum(v[m])) <= 1e-9 * np.abs(v[m]).sum()


def test_best_hypothesis_order():
    t = np.zeros(8, E.HYP_DTYPE)
    t["count"] = [5, 9, 9, 9, 2, 9, 12, 9]
    t["qerr"] = [1, 70, 50, 50, 0, 10, 0, 10]
    t["skipped"] = [0, 0, 0, 0, 0, 1, 1, 0]
    assert E.best_hypothesis(t) == 7            # 9 inliers; qerr 10 beats 50; h = 5 and 6 are skipped
    t["qerr"][7] = 50
    assert E.best_hypothesis(t) == 2            # ties on (count, qerr) go to the lowest h
    t["count"][:] = 2
    assert E.best_hypothesis(t) == -1           # fewer than 3 inliers everywhere
    t["count"][4] = 3
    assert E.best_hypothesis(t) == 4


def test_pose_chain_inverts_and_accumulates():
    rng = np.random.default_rng(8)
    pose, T = list(E.POSE_IDENTITY), np.eye(4)
    for k in range(5):
        res = np.zeros(1, E.RESULT_DTYPE)
        R, t = rotation(rng.normal(size=3), 3.0), rng.normal(size=3)
        res["R"][0], res["t"][0], res["status"] = R.ravel(), t, k != 2
        Trel = np.eye(4)
        Trel[:3, :3], Trel[:3, 3] = R, t
        if k != 2:
            T = T @ np.linalg.inv(Trel)
        pose = E.chain(pose, res)
        assert np.abs(np.array(pose).reshape(3, 4) - T[:3]).max() < 1e-13


def test_few_correspondences_give_status_0():
    cur, kp, prev, temporal, _, _, _ = scene(1, quant=4.0, shuffled=0)
    for n in (0, 2):
        res, mask, table = E.estimate(CAM, E.params(hypotheses=8), cur, kp, prev, temporal[:n])
        assert int(res["status"][0]) == 0 and tuple(res["R"][0]) == E.IDENTITY and int(res["n_inliers"][0]) == 0
        assert int(res["n_correspondences"][0]) == n and int(res["best_hypothesis"][0]) == -1 and not mask.any() and table["skipped"].all()


def test_refinement_improves_the_best_hypothesis():
    cur, kp, prev, temporal, R, t, _ = scene(2, quant=4.0, shuffled=0.3)
    r0 = E.estimate(CAM, E.params(refine_iterations=0), cur, kp, prev, temporal, seed=1, frame_id=2)[0]
    r4 = E.estimate(CAM, E.params(refine_iterations=4), cur, kp, prev, temporal, seed=1, frame_id=2)[0]
    assert int(r0["best_hypothesis"][0]) == int(r4["best_hypothesis"][0]) >= 0
    assert float(r4["rms"][0]) < float(r0["rms"][0])
    assert np.abs(r4["t"][0] - t).max() < np.abs(r0["t"][0] - t).max()


# worst case of the restatement over the 20 seeds below: rotation 0.0402 deg, translation 0.0098 m; the bounds are twice that
ROT_BOUND_DEG, TRANS_BOUND_M = 0.0804, 0.0196


def test_accuracy_on_the_synthetic_scene():
    """40 points at Z in [4, 30], fx = fy = 300, baseline 0.5, quarter-pixel observations, about 2 degrees and 0.6 m of motion,
    30 % of the temporal pairs shuffled, 20 seeds: the final inliers contain every unshuffled pair, and the pose error stays
    under twice the worst value the restatement shows over these seeds."""
    worst_r = worst_t = 0.0
    for seed in range(20):
        cur, kp, prev, temporal, R, t, good = scene(100 + seed)
        res, mask, _ = E.estimate(CAM, E.params(), cur, kp, prev, temporal, seed=seed, frame_id=seed + 1)
        assert int(res["status"][0]) == 1
        assert mask[good].all(), f"seed {seed}: unshuffled pairs {good[mask[good] == 0]} are not inliers"
        worst_r = max(worst_r, rot_err_deg(res["R"][0], R))
        worst_t = max(worst_t, float(np.linalg.norm(res["t"][0] - t)))
    print(f"accuracy: worst rotation error {worst_r:.4f} deg, worst translation error {worst_t:.4f} m")
    assert worst_r < ROT_BOUND_DEG and worst_t < TRANS_BOUND_M, (worst_r, worst_t)

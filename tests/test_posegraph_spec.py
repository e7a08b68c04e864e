"""CPU tests of spec S29: the numpy restatement of the pose-graph optimisation (tests/np_posegraph.py) against central
differences, a dense solve of the normal equations and a ring trajectory with known truth; and the host side of the built library.  The
scenarios here are shared with tests/test_gpu_posegraph.py."""
import ctypes as C
import math

import numpy as np
import pytest

import np_posegraph as G

W_ROT, W_TRANS = 10000.0, 100.0


# ---- scenarios ---------------------------------------------------------------------------------------------------------------------
def rot(w):
    """Rodrigues: the rotation matrix [3, 3] of the rotation vector w."""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K.dot(K)


def pose12(R, t):
    return [float(v) for v in np.hstack([R, np.asarray(t, np.float64).reshape(3, 1)]).reshape(-1)]


def mat4(p):
    return np.vstack([np.asarray(p, np.float64).reshape(3, 4), [0, 0, 0, 1]])


def ring(n, loops, seed, laps=1, sigma_rot=0.002, sigma_trans=0.02):
    """A ring of n camera poses (KITTI axes: y down, z ahead; one metre between neighbours, `laps` times round) -> (true poses, odometry
    poses chained from the noisy relative poses, loop edges (a, b, R [9], t [3]) from the truth for the node pairs `loops`)."""
    rng = np.random.default_rng(seed)
    radius = n / laps / (2 * math.pi)
    truth = []
    for i in range(n):
        th = 2 * math.pi * laps * i / n
        R = rot([0, th, 0]).dot(rot([0.02 * math.sin(3 * th), 0, 0.03 * math.cos(2 * th)]))
        truth.append(mat4(pose12(R, [radius * math.sin(th), 0.1 * math.sin(2 * th), radius * (1 - math.cos(th))])))
    odom = [truth[0]]
    for i in range(1, n):
        rel = np.linalg.inv(truth[i - 1]).dot(truth[i])
        noise = np.eye(4)
        noise[:3, :3], noise[:3, 3] = rot(rng.normal(0, sigma_rot, 3)), rng.normal(0, sigma_trans, 3)
        odom.append(odom[-1].dot(rel).dot(noise))
    edges = []
    for a, b in loops:
        M = np.linalg.inv(truth[b]).dot(truth[a])      # p_b = M p_a
        edges.append((a, b, [float(v) for v in M[:3, :3].reshape(-1)], [float(v) for v in M[:3, 3]]))
    return [m[:3].reshape(-1).tolist() for m in truth], [m[:3].reshape(-1).tolist() for m in odom], edges


def build(odom, edges, w_rot=W_ROT, w_trans=W_TRANS, graph=None):
    g = graph if graph is not None else G.Graph()
    for p in odom:
        g.add_node(p, w_rot, w_trans)
    for a, b, R, t in edges:
        g.add_loop(a, b, R, t, w_rot, w_trans)
    return g


RING_24 = dict(n=24, loops=[(0, 23)], seed=5)
RING_48 = dict(n=48, loops=[(0, 24), (3, 30), (10, 33), (12, 40)], seed=6, laps=2)   # (3, 30) and (10, 33) cross, (12, 40) holds (24 .. 33) nested


# ---- Jacobians ---------------------------------------------------------------------------------------------------------------------
def test_jacobians_against_central_differences():
    rng = np.random.default_rng(1)
    h, worst = 1e-6, 0.0
    for _ in range(20):
        Ta, Tb = np.eye(4), np.eye(4)
        Ta[:3, :3], Ta[:3, 3] = rot(rng.normal(0, 1, 3)), rng.normal(0, 5, 3)
        Tb[:3, :3], Tb[:3, 3] = rot(rng.normal(0, 1, 3)), rng.normal(0, 5, 3)
        err = np.eye(4)
        err[:3, :3], err[:3, 3] = rot(rng.normal(0, 0.05, 3)), rng.normal(0, 0.1, 3)
        M = err.dot(np.linalg.inv(np.linalg.inv(Ta).dot(Tb)))         # E = M est_a^-1 est_b = err
        edge = (0, 1, [float(v) for v in M[:3, :3].reshape(-1)], [float(v) for v in M[:3, 3]], 1.0, 1.0)
        est = [G.split(Ta[:3].reshape(-1)), G.split(Tb[:3].reshape(-1))]
        Re, r = G.residual(edge, est)
        assert 1e-3 < max(abs(v) for v in r) < 0.5
        Ja, Jb = G.jacobians(edge, Re, r)
        for node, J in ((0, Ja), (1, Jb)):
            for k in range(6):
                d = [0.0] * 6
                d[k] = h
                plus, minus = list(est), list(est)
                plus[node] = G.update_right(est[node], d)
                minus[node] = G.update_right(est[node], [-v for v in d])
                num = (np.array(G.residual(edge, plus)[1]) - np.array(G.residual(edge, minus)[1])) / (2 * h)
                worst = max(worst, float(np.abs(num - np.array(J)[:, k]).max()))
    print("jacobians against central differences:", worst)
    assert worst < 1e-7


# ---- the step against a dense solve --------------------------------------------------------------------------------------------------
# (scenario, bound): ten times what this restatement measured against the dense solve (1.1e-14, 6.2e-14, 1.6e-11), as DESIGN.md 7.11 records
DENSE = [(RING_24, 1.2e-13), (RING_48, 7e-13), (dict(n=256, loops=[(0, 255), (10, 200), (50, 120), (60, 100), (90, 250)], seed=7), 2e-10)]


def step_difference(scenario):
    _, odom, edges = ring(**scenario)
    g = build(odom, edges)
    x = np.array(g.step()[1:])
    ref = G.dense_step(g)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("k", range(len(DENSE)))
def test_step_equals_the_dense_solve(k):
    scenario, bound = DENSE[k]
    diff = step_difference(scenario)
    print("step against np.linalg.solve, relative:", scenario["n"], len(scenario["loops"]), diff)
    assert diff <= bound


# ---- convergence on the ring -------------------------------------------------------------------------------------------------------
# (scenario, bound on cost_after / cost_before): twice what this restatement measured (0.0372, 0.0260), as DESIGN.md 7.11 records
CONVERGENCE = [(RING_24, 0.075), (RING_48, 0.053)]


@pytest.mark.parametrize("k", range(len(CONVERGENCE)))
def test_convergence_on_the_ring(k):
    scenario, bound = CONVERGENCE[k]
    _, odom, edges = ring(**scenario)
    g4, g8 = build(odom, edges), build(odom, edges)
    before = [max(abs(v) for v in G.residual(e, g4.est)[1]) for e in g4.loops]
    r4, r8 = g4.optimize(4)[0], g8.optimize(8)[0]
    after = [max(abs(v) for v in G.residual(e, g4.est)[1]) for e in g4.loops]
    print("ring", scenario["n"], "cost", r4["cost_before"], "->", r4["cost_after"], "ratio", r4["cost_after"] / r4["cost_before"], "after 8:", r8["cost_after"])
    assert r4["status"] == 1 and r4["n_nodes"] == scenario["n"] and r4["n_loops"] == len(scenario["loops"]) and r4["iterations"] == 4
    assert r4["cost_after"] < r4["cost_before"] and r8["cost_before"] == r4["cost_before"]
    assert r4["cost_after"] / r4["cost_before"] <= bound
    assert r4["cost_after"] <= r8["cost_after"] * (1 + 1e-6) and r8["cost_after"] <= r4["cost_after"] * (1 + 1e-6)
    assert all(a < b for a, b in zip(after, before)), (before, after)
    assert g4.poses()[0].tolist() == odom[0]                      # the gauge


def agreeing_loop(odom, a, b):
    o = [mat4(p) for p in odom]
    M = np.linalg.inv(o[b]).dot(o[a])
    return (a, b, [float(v) for v in M[:3, :3].reshape(-1)], [float(v) for v in M[:3, 3]])


def test_a_consistent_chain_stays():
    _, odom, _ = ring(n=24, loops=[], seed=3)
    for edges in ([], [agreeing_loop(odom, 2, 20)], [agreeing_loop(odom, 0, 23), agreeing_loop(odom, 21, 5)]):
        g = build(odom, edges)
        res = g.optimize(4)[0]
        assert res["status"] == 1 and res["cost_before"] < 1e-20
        assert np.abs(g.poses() - np.array(odom)).max() < 1e-12


def test_small_graphs_and_zero_iterations():
    g = G.Graph()
    assert g.optimize(4).tobytes() == np.array([(1, 0, 0, 4, 0.0, 0.0)], G.RESULT_DTYPE).tobytes()
    _, odom, edges = ring(n=5, loops=[(0, 4)], seed=4)
    g.add_node(odom[0], W_ROT, W_TRANS)
    assert g.optimize(4).tobytes() == np.array([(1, 1, 0, 4, 0.0, 0.0)], G.RESULT_DTYPE).tobytes() and g.poses().tolist() == [odom[0]]
    g = build(odom, edges)
    start = g.poses()
    res = g.optimize(0)[0]
    assert res["cost_before"] == res["cost_after"] > 0 and res["iterations"] == 0 and (g.poses() == start).all()


def failing_graph():
    """A finite input whose chain factor meets a pivot that is not > 0: odometry weights of 1e300 beside 1e-300 (the products overflow)."""
    _, odom, edges = ring(n=6, loops=[(0, 5)], seed=2)
    g = G.Graph()
    weights = [1e-300 if i % 2 == 0 else 1e300 for i in range(len(odom))]
    for p, w in zip(odom, weights):
        g.add_node(p, w, w)
    g.add_loop(*edges[0], 1.0, 1.0)
    return g, odom, weights, edges


def test_a_failed_pivot_moves_nothing():
    g = failing_graph()[0]
    start = g.poses()
    with np.errstate(all="ignore"):
        res = g.optimize(2)[0]
    assert res["status"] == 0 and res["cost_after"] == res["cost_before"] and np.isfinite(res["cost_before"])
    assert g.poses().tobytes() == start.tobytes()


def test_the_module_restatement_carries_the_correction():
    """np_posegraph.module on a hand-made sequence: nodes on the keyframes, the loop at the last one, the pose carried between them."""
    import np_place
    truth, odom, _ = ring(n=12, loops=[], seed=8)
    loops = np.zeros(12, np_place.LOOP_DTYPE)
    loops[11]["detected"], loops[11]["keyframe_id"] = 1, 2                     # frame 12 (node 5) recognises frame 2 (node 0)
    M = np.linalg.inv(mat4(truth[11])).dot(mat4(truth[1]))
    loops[11]["relative"]["R"], loops[11]["relative"]["t"], loops[11]["relative"]["status"] = M[:3, :3].reshape(-1), M[:3, 3], 1
    out = G.module(odom, loops, keyframe_interval=2, max_nodes=8, max_loops=1)
    assert [int(r["node"][0]) for r, _, _ in out] == [-1, 0, -1, 1, -1, 2, -1, 3, -1, 4, -1, 5]
    assert out[0][1] == odom[0] and [n is not None for _, _, n in out] == [False] * 11 + [True]
    rec = out[11][0][0]
    assert rec["loop_added"] == 1 and rec["result"]["status"] == 1 and rec["result"]["n_nodes"] == 6 and rec["result"]["cost_after"] < rec["result"]["cost_before"]
    assert np.abs(np.array(out[11][1]) - out[11][2][5]).max() < 1e-12          # a keyframe publishes its node's estimate
    assert np.abs(np.array(out[4][1]) - np.array(odom[4])).max() < 1e-12       # before any loop the chain is the source's


# ---- the library's host side ------------------------------------------------------------------------------------------------------
def lib():
    from cartslam import _lib
    return _lib.load()


def err():
    return lib().cart_last_error(None).decode()


IDENTITY = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def test_exports_defaults_and_layout():
    from cartslam import POSE_GRAPH_RESULT_DTYPE, PoseGraph, PoseGraphParams, PoseGraphResult, _lib, pose_graph_params
    for name in ("default_params", "create", "destroy", "clear", "size", "add_node", "add_loop", "optimize", "poses", "read"):
        assert hasattr(lib(), "cart_pose_graph_" + name) and "cart_pose_graph_" + name in _lib.PROTOTYPES
    assert C.sizeof(PoseGraphParams) == 4 and C.sizeof(PoseGraphResult) == 32 == POSE_GRAPH_RESULT_DTYPE.itemsize and POSE_GRAPH_RESULT_DTYPE == G.RESULT_DTYPE
    assert [(n, POSE_GRAPH_RESULT_DTYPE.fields[n][1]) for n in POSE_GRAPH_RESULT_DTYPE.names] == [(n, getattr(PoseGraphResult, n).offset) for n, _ in PoseGraphResult._fields_]
    assert pose_graph_params().iterations == G.DEFAULT_ITERATIONS == 4 and pose_graph_params(iterations=7).iterations == 7
    with pytest.raises(ValueError):
        pose_graph_params(steps=1)
    lib().cart_pose_graph_default_params(None)   # a NULL pointer is ignored
    assert (_lib.POSE_GRAPH_MAX_NODES, _lib.POSE_GRAPH_MAX_LOOPS, _lib.POSE_GRAPH_MAX_ITERATIONS) == (G.MAX_NODES, G.MAX_LOOPS, G.MAX_ITERATIONS)
    assert G.MODULE_DTYPE.itemsize == 48 and G.MODULE_DTYPE.fields["node"][1] == 32
    assert PoseGraph._name == "pose_graph"


def test_argument_checks_without_an_object():
    from cartslam import pose_graph_params
    L = lib()
    out = C.c_void_p()
    for args, word in (((None, 0, 4), "max_nodes"), ((None, 4097, 4), "max_nodes"), ((None, 8, -1), "max_loops"), ((None, 8, 65), "max_loops"),
                       ((None, 0, 65), "max_nodes"), ((None, 1, 0), "bad arguments"), ((None, 4096, 64), "bad arguments")):
        assert L.cart_pose_graph_create(*args, C.byref(out)) != 0 and word in err(), (args, err())
        assert out.value is None
    # add_node: the pose, then the weights, then the object
    node = C.c_int32(-7)
    bad = lambda k, v: (C.c_double * 12)(*[v if i == k else IDENTITY[i] for i in range(12)])   # noqa: E731
    for pose, wr, wt, word in ((None, 1.0, 1.0, "pose is NULL"), (bad(0, float("nan")), 1.0, 1.0, "pose[0]"), (bad(5, 2.5), 1.0, 1.0, "pose[5]"),
                               (bad(7, 2e6), 1.0, 1.0, "pose[7]"), (IDENTITY, 0.0, 1.0, "w_rot"), (IDENTITY, float("inf"), 1.0, "w_rot"),
                               (IDENTITY, 1.0, -1.0, "w_trans"), (IDENTITY, 1.0, float("nan"), "w_trans"), (bad(3, float("inf")), 0.0, 0.0, "pose[3]"),
                               (IDENTITY, 1.0, 1.0, "graph is NULL")):
        assert L.cart_pose_graph_add_node(None, pose, wr, wt, C.byref(node), None) != 0 and word in err(), (word, err())
        assert node.value == -7
    # add_loop: R, t, the weights, a != b, then the object
    R, t = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 3)(0, 0, 0)
    Rbad, tbad = (C.c_double * 9)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1), (C.c_double * 3)(0, 0, float("inf"))
    for args, word in (((0, 1, None, t, 1.0, 1.0), "R is NULL"), ((0, 1, R, None, 1.0, 1.0), "t is NULL"), ((0, 1, Rbad, t, 1.0, 1.0), "R[4]"),
                       ((0, 1, R, tbad, 1.0, 1.0), "t[2]"), ((0, 1, R, t, 0.0, 1.0), "w_rot"), ((0, 1, R, t, 1.0, float("nan")), "w_trans"),
                       ((3, 3, R, t, 1.0, 1.0), "a and b"), ((0, 1, R, t, 1.0, 1.0), "graph is NULL")):
        assert L.cart_pose_graph_add_loop(None, *args, None) != 0 and word in err(), (word, err())
    # optimize: params, then the object
    assert L.cart_pose_graph_optimize(None, None, None, None) != 0 and "params" in err()
    for it in (-1, 17):
        assert L.cart_pose_graph_optimize(None, C.byref(pose_graph_params(iterations=it)), None, None) != 0 and "iterations" in err()
    for it in (0, 4, 16):
        assert L.cart_pose_graph_optimize(None, C.byref(pose_graph_params(iterations=it)), None, None) != 0 and err() == "graph is NULL"
    # poses / read: the sizes, then the object
    for fn, tail in ((L.cart_pose_graph_poses, (None, None)), (L.cart_pose_graph_read, (None,))):
        assert fn(None, -1, 1, *tail) != 0 and "first" in err()
        assert fn(None, 0, -1, *tail) != 0 and "count" in err()
        assert fn(None, 0, 0, *tail) != 0 and err() == "graph is NULL"
    n = C.c_int(-7)
    assert L.cart_pose_graph_size(None, C.byref(n), C.byref(n)) != 0 and err() == "graph is NULL" and n.value == -7
    assert L.cart_pose_graph_clear(None, None) != 0 and err() == "graph is NULL"
    L.cart_pose_graph_destroy(None)   # a NULL object is ignored

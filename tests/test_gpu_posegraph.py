"""GPU tests of the pose-graph optimisation (spec S29): after every optimise all estimates and the result record equal
the numpy restatement (tests/np_posegraph.py) byte for byte -- over the graph shapes at which each part of the solver can go wrong, the
object's state in call order, the failed pivot and the argument checks; and the "pose_graph" module through the C++ frame loop equals
the restatement fed with the restated poses and loop records of every frame.

The kernel as built: one workgroup of 512 threads; lane 0 factors the chain, lanes 64 .. 448 hold one right-hand-side column each (1 + 6
per loop), the loop system has one row per lane."""
import ctypes as C

import numpy as np
import pytest

import np_posegraph as G
import test_posegraph_spec as S

pytestmark = pytest.mark.gpu


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


def make(max_nodes=80, max_loops=12):
    from cartslam import PoseGraph
    return PoseGraph(engine(), max_nodes, max_loops), G.Graph(max_nodes, max_loops)


def add(pg, g, odom, edges, w_rot=S.W_ROT, w_trans=S.W_TRANS):
    for p in odom:
        assert pg.add_node(p, w_rot, w_trans) == g.add_node(p, w_rot, w_trans)
    for a, b, R, t in edges:
        pg.add_loop(a, b, R, t, w_rot, w_trans)
        g.add_loop(a, b, R, t, w_rot, w_trans)


def same_poses(pg, g):
    got, want = pg.poses(), g.poses()
    assert pg.size() == (len(g.odom), len(g.loops)) and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), f"largest difference {np.abs(got - want).max()}"


def optimize_both(pg, g, iterations=4):
    got = pg.optimize(iterations)
    with np.errstate(all="ignore"):
        want = g.optimize(iterations)
    assert got.tobytes() == want.tobytes(), (got, want)
    same_poses(pg, g)
    return got[0]


def check(n, loops, seed, iterations=4, laps=1, max_nodes=80, max_loops=12):
    _, odom, edges = S.ring(n, loops, seed, laps)
    pg, g = make(max_nodes, max_loops)
    add(pg, g, odom, edges)
    same_poses(pg, g)   # the estimates chained at insertion
    res = optimize_both(pg, g, iterations)
    pg.close()
    return res


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
SHAPES = {
    "one node": (1, []),
    "two nodes": (2, []),
    "three nodes, the loop onto the gauge": (3, [(0, 2)]),
    "a loop between neighbours": (9, [(4, 5)]),
    "a loop between neighbours at the gauge": (5, [(0, 1)]),
    "two loops share a node": (12, [(2, 9), (9, 4)]),
    "crossing and nested loops": (20, [(1, 12), (6, 17), (3, 19), (8, 10)]),
    "a loop given backwards": (10, [(8, 2)]),
    "more nodes than a wave": (70, [(0, 69), (20, 50)]),
    "more right-hand sides than a wave": (40, [(i, 39 - i) for i in range(11)]),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    n, loops = SHAPES[name]
    res = check(n, loops, seed=20 + n)
    assert res["status"] == 1 and (res["cost_after"] < res["cost_before"] if loops else res["cost_before"] < 1e-18)


@pytest.mark.parametrize("iterations", [0, 1, 16])
def test_no_loops_and_the_iteration_range(iterations):
    check(17, [], seed=31, iterations=iterations)
    check(13, [(0, 12)], seed=32, iterations=iterations)


def test_both_tables_filled_exactly():
    from cartslam import EngineError
    _, odom, edges = S.ring(8, [(0, 7), (2, 6)], seed=33)
    pg, g = make(8, 2)
    add(pg, g, odom, edges)
    with pytest.raises(EngineError, match="node table is full"):
        pg.add_node(odom[0], 1.0, 1.0)
    with pytest.raises(EngineError, match="loop table is full"):
        pg.add_loop(1, 5, edges[0][2], edges[0][3], 1.0, 1.0)
    assert pg.size() == (8, 2)
    same_poses(pg, g)
    optimize_both(pg, g)
    pg.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def test_state_in_call_order():
    _, odom, edges = S.ring(30, [(0, 14), (5, 29)], seed=34)
    pg, g = make()
    add(pg, g, odom[:15], edges[:1])
    optimize_both(pg, g)
    add(pg, g, odom[15:], [])                  # a new estimate follows the optimised predecessor, not the odometry
    same_poses(pg, g)
    assert np.abs(pg.poses()[29] - np.array(odom[29])).max() > 1e-6
    add(pg, g, [], edges[1:])
    optimize_both(pg, g)
    optimize_both(pg, g, 2)                    # two optimises in a row
    pg.clear()
    g.clear()
    assert pg.size() == (0, 0) and pg.poses().shape == (0, 12)
    _, odom2, edges2 = S.ring(11, [(1, 9)], seed=35)
    add(pg, g, odom2, edges2)
    optimize_both(pg, g)
    pg.close()


def test_calls_queued_on_two_streams():
    torch = _torch()
    _, odom, edges = S.ring(25, [(0, 24), (3, 20)], seed=36)
    pg, g = make()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for i, p in enumerate(odom):
        with torch.cuda.stream(s1 if i % 2 else s2):
            pg.add_node(p, S.W_ROT, S.W_TRANS)
        g.add_node(p, S.W_ROT, S.W_TRANS)
    with torch.cuda.stream(s1):
        pg.add_loop(*edges[0], S.W_ROT, S.W_TRANS)
    with torch.cuda.stream(s2):
        pg.add_loop(*edges[1], S.W_ROT, S.W_TRANS)
        first = pg.optimize(4, raw=True)
    with torch.cuda.stream(s1):
        second = pg.optimize(1, raw=True)
        poses = pg.poses(raw=True)
    for e in edges:
        g.add_loop(*e, S.W_ROT, S.W_TRANS)
    want = [g.optimize(4), g.optimize(1)]
    torch.cuda.synchronize()
    assert first.cpu().numpy().tobytes() == want[0].tobytes() and second.cpu().numpy().tobytes() == want[1].tobytes()
    assert poses.cpu().numpy().tobytes() == g.poses().tobytes()
    pg.close()


def test_destroyed_after_its_engine():
    from cartslam import Engine, PoseGraph
    other = Engine(64, 32, num_disparities=0, paths=0)
    pg, g = PoseGraph(other, 16, 2), G.Graph(16, 2)
    _, odom, edges = S.ring(10, [(0, 9)], seed=37)
    add(pg, g, odom, edges)
    other.close()
    optimize_both(pg, g)
    pg.close()


# ---- the failed pivot ----------------------------------------------------------------------------------------------------------------
def test_a_failed_pivot_moves_nothing():
    """tests/test_posegraph_spec.py confirms the premise on the restatement: this finite graph meets a pivot that is not > 0."""
    g, odom, weights, edges = S.failing_graph()
    pg, _ = make()
    for p, w in zip(odom, weights):
        pg.add_node(p, w, w)
    pg.add_loop(*edges[0], 1.0, 1.0)
    start = pg.poses()
    res = optimize_both(pg, g, 2)
    assert res["status"] == 0 and pg.poses().tobytes() == start.tobytes()
    pg.close()


# ---- the Python object and the argument checks -----------------------------------------------------------------------------------------
def test_python_object():
    from cartslam import EngineError, PoseGraph, pose_graph_params
    with pytest.raises(EngineError, match="max_nodes"):
        PoseGraph(engine(), 0, 1)
    with pytest.raises(EngineError, match="max_loops"):
        PoseGraph(engine(), 4, 65)
    _, odom, edges = S.ring(6, [(0, 5)], seed=38)
    with PoseGraph(engine(), 6, 0) as pg:              # no loop table at all
        g = G.Graph(6, 0)
        add(pg, g, odom, [])
        with pytest.raises(EngineError, match="loop table is full"):
            pg.add_loop(*edges[0], 1.0, 1.0)
        assert pg.optimize(params=pose_graph_params(iterations=3)).tobytes() == g.optimize(3).tobytes()
        assert pg.poses(2, 3).tobytes() == g.poses()[2:5].tobytes() and pg.poses(6, 0).shape == (0, 12)
        with pytest.raises(EngineError, match="first \\+ count"):
            pg.poses(4, 3)
        with pytest.raises(EngineError, match="iterations"):
            pg.optimize(17)
    assert pg._h is None


def test_bad_arguments_name_the_argument_and_touch_nothing():
    torch = _torch()
    _, odom, edges = S.ring(7, [(0, 6)], seed=39)
    pg, g = make(8, 2)
    add(pg, g, odom, edges)
    lib = pg._lib
    err = lambda: lib.cart_last_error(None).decode()   # noqa: E731
    R, t = (C.c_double * 9)(*edges[0][2]), (C.c_double * 3)(*edges[0][3])
    for a, b, word in ((0, 7, "b must be a node"), (-1, 3, "a must be a node"), (7, 0, "a must be a node"), (2, 2, "a and b")):
        assert lib.cart_pose_graph_add_loop(pg._h, a, b, R, t, 1.0, 1.0, None) != 0 and word in err(), (word, err())
    from cartslam import pose_graph_params
    p = pose_graph_params()
    out = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")
    assert lib.cart_pose_graph_optimize(pg._h, C.byref(p), C.c_void_p(out.data_ptr() + 4), None) != 0 and "result" in err()
    assert lib.cart_pose_graph_poses(pg._h, 0, 1, None, None) != 0 and "out is NULL" in err()
    assert lib.cart_pose_graph_poses(pg._h, 0, 1, C.c_void_p(out.data_ptr() + 2), None) != 0 and "out must be 8-byte aligned" in err()
    assert lib.cart_pose_graph_poses(pg._h, 0, 8, C.c_void_p(out.data_ptr()), None) != 0 and "first + count" in err()
    assert lib.cart_pose_graph_read(pg._h, 0, 1, None) != 0 and "out_host" in err()
    assert lib.cart_pose_graph_read(pg._h, 6, 2, (C.c_double * 24)()) != 0 and "first + count" in err()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and pg.size() == (7, 1)
    same_poses(pg, g)                                   # nothing moved, and the object is still usable
    optimize_both(pg, g)
    host = (C.c_double * 24)()
    assert lib.cart_pose_graph_read(pg._h, 5, 2, host) == 0 and bytes(host) == g.poses()[5:7].tobytes()
    pg.close()


# ---- the C++ frame loop ----------------------------------------------------------------------------------------------------------------
def test_pose_graph_module_frame_loop(tmp_path):
    """[orb_features, orb_matches, ego_motion, loop_closure, pose_graph, plane_map on the corrected pose] over the revisit sequence of
    tests/test_place_spec.py (keyframes 2, 4, 6; frame 6 recognises frame 2: three nodes, the loop (0, 2)): every frame's dumped record
    and pose, and frame 6's node estimates, equal the restatement chain np_orb -> np_match -> np_ego -> np_place -> np_posegraph, whole;
    frame 6's plane map equals np_planemap fed with the corrected poses."""
    import json
    import os
    import np_planemap as M
    import oracle_lib as O
    import test_place_spec as L
    from test_gpu_planemap import check_dump
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    images, _, _, _, ego, records = L.loop_sequence()
    n = len(images)
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for cam in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, cam))
    for f, (l, r) in enumerate(images):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    static = {"type": "static", "horizontal_range_min": 6, "horizontal_range_max": 18, "vertical_range_min": -5, "vertical_range_max": 6}
    grid = dict(cells_x=64, cells_z=64, cell_size=1.0, max_depth=40.0, max_lateral=30.0)
    front = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
             {"type": "disparity_planeseg", "parameter_provider": static},
             {"type": "orb_features"}, {"type": "orb_matches"}, dict(L.LOOP_KEYS, type="ego_motion"), dict(L.LOOP_KEYS, type="loop_closure", **L.LOOP_CONFIG)]
    graph_keys = dict(keyframe_interval=L.LOOP_CONFIG["keyframe_interval"], max_nodes=8, max_loops=2)
    modules = front + [dict(graph_keys, type="pose_graph"), dict(L.LOOP_KEYS, type="plane_map", pose_key="pose_graph", **grid)]
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, modules, tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    want = G.module([pose for _, pose in ego], records, **graph_keys)
    assert [int(rec["node"][0]) for rec, _, _ in want] == [-1, 0, -1, 1, -1, 2] and [int(rec["loop_added"][0]) for rec, _, _ in want] == [0] * 5 + [1]
    for fid in range(1, n + 1):
        rec, pose, nodes = want[fid - 1]
        got = open(os.path.join(d, f"{fid}_pose_graph.bin"), "rb").read()
        assert got == rec.tobytes() + np.array(pose, np.float64).tobytes(), f"frame {fid}: {np.frombuffer(got[:48], G.MODULE_DTYPE)} != {rec}"
        path = os.path.join(d, f"{fid}_pose_graph_nodes.bin")
        assert os.path.exists(path) == (nodes is not None)
        if nodes is not None:
            assert nodes.shape == (3, 12) and open(path, "rb").read() == nodes.tobytes()
    last = want[n - 1][0][0]["result"]
    assert last["status"] == 1 and (last["n_nodes"], last["n_loops"]) == (3, 1) and last["cost_after"] <= last["cost_before"]
    # the plane map took the corrected trajectory
    ref = M.Map(M.camera(**L.LOOP_KEYS), 64, 64, M.params(cell_size=1.0, max_depth=40.0, max_lateral=30.0))
    planes = {}
    for f in range(n):
        k = L.LOOP_ORDER[f]
        if k not in planes:
            ed = O.disparity_module(images[f][0], images[f][1], 64, 8, 4, radius=2, iterations=1)
            planes[k] = (ed, O.classify(O.plane_derivative(ed)[0], (6, 18, -5, 6, 12, 0)))
        ref.update(planes[k][0], planes[k][1], want[f][1])
    check_dump(os.path.join(d, f"{n}_plane_map.bin"), ref, 3, 50)
    # creation-time checks: the dependencies and an out-of-range key with the library's message
    r = run_exe(src, front[2:5] + [dict(graph_keys, type="pose_graph")], tmp)
    assert r.returncode != 0 and 'requires "loop_closure"' in r.stderr
    for key, bad in (("max_nodes", 4097), ("max_loops", 65), ("iterations", 17), ("weight_rotation", 0), ("loop_weight", -1.0), ("keyframe_interval", 3),
                     ("pose_key", "pose_graph")):
        r = run_exe(src, front[2:] + [dict(dict(graph_keys, **{key: bad}), type="pose_graph")], tmp)
        assert r.returncode != 0 and key in r.stderr, (key, r.stderr)
    r = run_exe(src, front[2:5] + [dict(L.LOOP_KEYS, type="loop_closure", pose_key="pose_graph", **L.LOOP_CONFIG)], tmp)
    assert r.returncode != 0 and "pose_key" in r.stderr          # loop_closure keeps refusing it: the dependency would be circular

"""GPU tests of the superpixel plane stages: every output of cart_planefit_* equals the CPU
restatement (tests/np_planefit.py) exactly; planes_eq of the reference's kitti-planefit / kitti-planecluster module lists
through the C++ frame loop equals the restatement fed with the dumped superpixels and depth."""
import json
import math
import os

import numpy as np
import pytest

import np_planefit as N

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def block_labels(w, h, bs):
    nbx = (w + bs - 1) // bs
    return ((np.arange(h)[:, None] // bs) * nbx + np.arange(w)[None, :] // bs).astype(np.uint16), nbx * ((h + bs - 1) // bs) - 1


def scene(w, h, seed, holes=True, noise=0.002):
    """Piecewise planar xyz: road (y = 1.6), a wall (x = 3), a slanted plane; noise and NaN / +-inf / z <= 0 / z > 40 holes."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    xyz = np.zeros((h, w, 3))
    z = 3.0 + 30.0 * (v / h)
    x = (u - w / 2) / (w / 8.0)
    y = np.full_like(z, 1.6)
    wall = u > 0.7 * w
    x[wall] = 3.0; y[wall] = 1.6 - (h - v[wall]) / (h / 3.0); z[wall] = 5 + (u[wall] - 0.7 * w) / 4.0
    slant = (u < 0.25 * w) & (v < 0.5 * h)
    x[slant] = -3 + u[slant] / w; y[slant] = -1 + v[slant] / h; z[slant] = 6 + 0.5 * x[slant] + 0.25 * y[slant]
    xyz[..., 0], xyz[..., 1], xyz[..., 2] = x, y, z
    xyz += rng.normal(0, noise, xyz.shape)
    xyz = xyz.astype(np.float32)
    if holes:
        for val, frac in ((np.nan, 0.03), (np.inf, 0.01), (-np.inf, 0.01), (0.0, 0.01), (-2.0, 0.01), (55.0, 0.02)):
            m = rng.random((h, w)) < frac
            xyz[..., 2][m] = val
        blk = rng.random((h // 8 + 1, w // 8 + 1)) < 0.15   # whole invalid patches: some regions invalid
        xyz[..., 2][np.kron(blk, np.ones((8, 8), bool))[:h, :w]] = np.nan
    return xyz


def engine(w, h):
    from cartslam import Engine
    _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's (see __graft_entry__.build)
    return Engine(w, h, num_disparities=0, paths=0)


def relaxed_labels(eng, w, h, bs, seed):
    from cartslam import Superpixels, synth
    torch = _torch()
    l, _, _ = synth.make_pair(w, h, 64, 4, seed=seed, channels=3)
    sp = Superpixels(eng, block_size=bs, disparity_weight=0.0)
    lab = sp.relax(torch.from_numpy(l).cuda(), None, 6)
    mx = sp.max_label
    sp.close()
    return lab.cpu().numpy().view(np.uint16), mx


def run_label_planes(pf, lab, xyz, mx, pred, seed=0, frame=1):
    torch = _torch()
    tl = torch.from_numpy(lab.view(np.int16)).cuda()
    tx = torch.from_numpy(xyz).cuda()
    planes, npts, counts = pf.label_planes(tl, tx, mx, pred, seed=seed, frame_id=frame)
    return planes.cpu().numpy(), npts.cpu().numpy(), counts.cpu().numpy()


def check_label_planes(pf, lab, xyz, mx, pred, seed=0, frame=1):
    planes, npts, counts = run_label_planes(pf, lab, xyz, mx, pred, seed, frame)
    ec, eoff, epts = N.label_points(lab, xyz, mx, pred)
    assert (counts == ec).all(), "per-label counts"
    assert (npts == np.diff(eoff)).all(), "per-label point counts"
    pts, off = pf.points()
    pts, off = pts.cpu().numpy(), off.cpu().numpy()
    assert (off == eoff).all()
    assert np.array_equal(pts[:, :3].view(np.uint32), epts.view(np.uint32)), "point lists (raster order inside a label)"
    for l in range(mx + 1):
        e = N.ransac_plane(epts[eoff[l]:eoff[l + 1]], seed, frame, l)
        assert np.array_equal(planes[l].view(np.uint64), np.array(e).view(np.uint64)), f"label {l}: {planes[l]} vs {e}"
    return planes, npts


@pytest.mark.parametrize("pred", [N.PRED_PLANEFIT, N.PRED_PLANECLUSTER])
def test_label_planes_block_labels_320x96(pred):
    from cartslam import PlaneFit
    w, h = 320, 96
    eng = engine(w, h)
    pf = PlaneFit(eng, 4000)
    lab, mx = block_labels(w, h, 8)
    xyz = scene(w, h, 1)
    _, npts = check_label_planes(pf, lab, xyz, mx, pred)
    if pred == N.PRED_PLANEFIT:   # the NaN patches leave labels below 16 points (planecluster keeps NaN z)
        assert (npts < 16).any()
    pf.close(); eng.close()


def test_label_planes_edge_cases():
    """Labels with 0, 15, 16 and > 64k points (one > the LDS stage), ids up to 16383, a size that is no tile multiple."""
    from cartslam import PlaneFit
    w, h = 333, 101
    eng = engine(w, h)
    pf = PlaneFit(eng)
    lab, mx = block_labels(w, h, 9)
    rng = np.random.default_rng(4)
    pool = np.setdiff1d(np.arange(16384), [100, 101, 16000, 16383])
    ids = rng.permutation(pool)[:mx + 1].astype(np.uint16)
    ids[0] = 16383
    lab = ids[lab]
    lab[0:48, 0:48] = 16000                      # 2304 pixels
    lab[60:61, 0:15] = 100; lab[61:62, 0:16] = 101   # 15 and 16 pixels (label 100 / 101 are otherwise absent or few)
    xyz = scene(w, h, 2, holes=False)
    for pred in (N.PRED_PLANEFIT, N.PRED_PLANECLUSTER):
        check_label_planes(pf, lab, xyz, 16383, pred, seed=5, frame=3)
    assert not pf.status()
    pf.close(); eng.close()


@pytest.mark.parametrize("pred", [N.PRED_PLANEFIT, N.PRED_PLANECLUSTER])
def test_label_planes_relaxed_1242x375(pred):
    from cartslam import PlaneFit
    w, h = 1242, 375
    eng = engine(w, h)
    lab, mx = relaxed_labels(eng, w, h, 12, 7)
    pf = PlaneFit(eng, mx)
    check_label_planes(pf, lab, scene(w, h, 3), mx, pred, seed=11, frame=42)
    pf.close(); eng.close()


def test_adjacency():
    from cartslam import PlaneFit
    torch = _torch()
    for (w, h, bs) in ((320, 96, 8), (333, 101, 9)):
        eng = engine(w, h)
        lab, mx = relaxed_labels(eng, w, h, bs, 9)
        pf = PlaneFit(eng, mx)
        off, nb = pf.adjacency(torch.from_numpy(lab.view(np.int16)).cuda(), mx)
        eoff, enb = N.adjacency(lab, mx)
        assert (off.cpu().numpy() == eoff).all() and (nb.cpu().numpy() == enb).all()
        pf.close(); eng.close()


def _fit(pf, lab, xyz, mx, seed, frame):
    torch = _torch()
    tl = torch.from_numpy(lab.view(np.int16)).cuda()
    pf.label_planes(tl, torch.from_numpy(xyz).cuda(), mx, N.PRED_PLANEFIT, seed=seed, frame_id=frame)
    P, A, launches = pf.fit(tl, seed=seed, frame_id=frame)
    return P.cpu().numpy(), A.cpu().numpy().view(np.uint64), launches


def _cluster(pf, lab, xyz, mx, seed, frame):
    from cartslam import plane_cluster
    torch = _torch()
    tl = torch.from_numpy(lab.view(np.int16)).cuda()
    planes, _, _ = pf.label_planes(tl, torch.from_numpy(xyz).cuda(), mx, N.PRED_PLANECLUSTER, seed=seed, frame_id=frame)
    off, nb = pf.adjacency(tl, mx)
    return plane_cluster(planes.cpu().numpy(), off.cpu().numpy(), nb.cpu().numpy())


def test_planefit_and_planecluster_match_restatement():
    from cartslam import PlaneFit
    w, h = 320, 96
    eng = engine(w, h)
    lab, mx = block_labels(w, h, 8)
    pf = PlaneFit(eng, mx)
    xyz = scene(w, h, 6)
    P, A, launches = _fit(pf, lab, xyz, mx, 0, 1)
    eP, eA, it = N.planefit(lab, xyz, mx, 0, 1)
    assert it > 0, "the scene must leave > 10 % of the regions invalid so that the loop runs"
    assert len(eP) > 0 and (eA > 0).sum() >= 16, "the scene must make the loop accept a plane"
    assert np.array_equal(P.view(np.uint64), eP.view(np.uint64)) and (A == eA).all()
    assert launches == 202
    cP, cA = _cluster(pf, lab, xyz, mx, 0, 1)
    ep17, _, _, _, _ = N.label_planes(lab, xyz, mx, N.PRED_PLANECLUSTER, 0, 1)
    eoff, enb = N.adjacency(lab, mx)
    ecP, ecA = N.plane_cluster(ep17, eoff, enb)
    assert np.array_equal(cP.view(np.uint64), ecP.view(np.uint64)) and (cA == ecA).all()
    # deterministic: same inputs twice and on another stream; another frame id or seed changes the hypotheses
    torch = _torch()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        P2, A2, _ = _fit(pf, lab, xyz, mx, 0, 1)
    s.synchronize()
    assert np.array_equal(P2.view(np.uint64), P.view(np.uint64)) and (A2 == A).all()
    P3, A3, _ = _fit(pf, lab, xyz, mx, 0, 1)
    assert np.array_equal(P3.view(np.uint64), P.view(np.uint64)) and (A3 == A).all()
    noisy = scene(w, h, 6, noise=0.02)   # noise above the threshold: the inlier set depends on the hypothesis
    p_a, _, _ = run_label_planes(pf, lab, noisy, mx, N.PRED_PLANEFIT, 0, 1)
    p_f, _, _ = run_label_planes(pf, lab, noisy, mx, N.PRED_PLANEFIT, 0, 2)
    p_s, _, _ = run_label_planes(pf, lab, noisy, mx, N.PRED_PLANEFIT, 9, 1)
    assert not np.array_equal(p_a, p_f) and not np.array_equal(p_a, p_s)
    pf.close(); eng.close()


def test_planecluster_recovers_true_planes():
    """Independent of the restatement: a clean road + wall scene -> planes within 1 degree and 1 cm of the truth."""
    from cartslam import PlaneFit
    w, h = 320, 96
    eng = engine(w, h)
    lab, mx = block_labels(w, h, 8)
    pf = PlaneFit(eng, mx)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    xyz = np.zeros((h, w, 3))
    wall = u >= 160
    xyz[..., 0] = np.where(wall, 2.0, (u - 80) / 20.0)
    xyz[..., 1] = np.where(wall, (v - 48) / 20.0, 1.5)
    xyz[..., 2] = np.where(wall, 4 + (u - 160) / 20.0, 3 + v / 10.0)
    P, A = _cluster(pf, lab, xyz.astype(np.float32), mx, 0, 1)
    truth = [np.array([0, 1.0, 0, -1.5]), np.array([1.0, 0, 0, -2.0])]
    assert len(P) == 2
    for t in truth:
        ok = False
        for p in P:
            s = np.sign(np.dot(p[:3], t[:3]))
            ang = math.degrees(math.acos(min(1.0, abs(np.dot(p[:3], t[:3])))))
            ok |= ang < 1.0 and abs(p[3] * s - t[3]) < 0.01
        assert ok, (t, P)
    pf.close(); eng.close()


def test_plane_module_lists_frame_loop(tmp_path):
    """config/modules/kitti-planefit.json and kitti-planecluster.json (sizes / iterations shrunk; planefit_visualization
    skipped, optflow = the native stand-in) through cart_slam_amd --dump: planes_eq of every frame = the restatement fed
    with that frame's dumped superpixels and depth."""
    from test_host import make_dataset, run_exe
    tmp = str(tmp_path)
    w, h, n = 320, 96, 3
    src, _ = make_dataset(tmp, n, w, h, channels=3)
    base = [{"type": "superpixels", "initial_iterations": 5, "iterations": 2, "block_size": 8},
            {"type": "disparity", "num_disparities": 128, "smoothing_radius": 2, "smoothing_iterations": 1},
            {"type": "disparity_derivative"}, {"type": "depth"}, {"type": "optflow", "search_radius": 4}]
    for kind in ("planefit", "planecluster"):
        d = os.path.join(tmp, "dump_" + kind)
        os.makedirs(d)
        mods = base + [{"type": kind, "seed": 7}, {"type": "planefit_visualization"}]
        r = run_exe(src, mods, tmp, ("--dump", d, "--sequential", "1"))
        assert r.returncode == 0, r.stderr
        ran = accepted = 0
        for fid in range(1, n + 1):
            lab = np.fromfile(os.path.join(d, f"{fid}_superpixels.bin"), np.uint16).reshape(h, w)
            xyz = np.fromfile(os.path.join(d, f"{fid}_depth.bin"), np.float32).reshape(h, w, 3)
            mx = int(np.fromfile(os.path.join(d, f"{fid}_superpixels_max_label.bin"), np.uint16)[0])
            P = np.fromfile(os.path.join(d, f"{fid}_planes_eq_planes.bin"), np.float64).reshape(-1, 4)
            A = np.fromfile(os.path.join(d, f"{fid}_planes_eq_assignments.bin"), np.uint64)
            L17 = np.fromfile(os.path.join(d, f"{fid}_planes_eq_label_planes.bin"), np.float64).reshape(-1, 4)
            pred = N.PRED_PLANEFIT if kind == "planefit" else N.PRED_PLANECLUSTER
            p17, _, _, _, _ = N.label_planes(lab, xyz, mx, pred, 7, fid)
            bad = np.nonzero((L17.view(np.uint64) != p17.view(np.uint64)).any(1))[0]
            assert len(bad) == 0, f"{kind} frame {fid}: S17 planes differ at labels {bad[:8]}"
            if kind == "planefit":
                eP, eA, it = N.planefit(lab, xyz, mx, 7, fid, planes17=p17)
                ran += it
                accepted += len(eP)
            else:
                eoff, enb = N.adjacency(lab, mx)
                eP, eA = N.plane_cluster(p17, eoff, enb)
                accepted += len(eP)
            assert np.array_equal(P.view(np.uint64), eP.view(np.uint64)) and (A == eA).all(), f"{kind} frame {fid}"
        assert accepted > 0, f"{kind}: no frame produced a plane"
        if kind == "planefit":
            assert ran > 0, "planefit's loop never ran on this dataset"

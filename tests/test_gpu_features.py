"""GPU tests of the ORB feature stage: cart_orb_detect's keypoints (every field as raw bits) and
descriptors equal the numpy restatement (tests/np_orb.py) exactly, stage by stage through cart_orb_debug_level, and the
reference's "features" module (factory type "orb_features") through the C++ frame loop equals the restatement on every
frame's images."""
import os

import numpy as np
import pytest

import np_orb as N

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def engine(w=64, h=32):
    from cartslam import Engine
    _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's (see __graft_entry__.build)
    return Engine(w, h, num_disparities=0, paths=0)


def block_noise(h, w, b, seed):
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 256, (h // b + 1, w // b + 1)), np.ones((b, b), np.int64))[:h, :w].astype(np.uint8)


def checkerboard(h, w, sq=8, lo=20, hi=230):
    return np.where(((np.arange(h)[:, None] // sq) + (np.arange(w)[None, :] // sq)) % 2 == 0, lo, hi).astype(np.uint8)


def synth_pair(w, h, seed, channels=1):
    from cartslam import synth
    l, r, _ = synth.make_pair(w, h, 64, 4, seed=seed, channels=channels)
    return l, r


def pitched(t, pad=64):
    """The same image as a row-pitched view (each row padded by `pad` bytes)."""
    torch = _torch()
    h, w = t.shape[:2]
    rest = tuple(t.shape[2:])
    row = w * (rest[0] if rest else 1) + pad
    buf = torch.zeros((h, row), dtype=torch.uint8, device="cuda")
    buf[:, :row - pad] = t.reshape(h, -1)
    v = buf[:, :row - pad]
    return v.view(h, w, *rest) if rest else v


def check(kp, de, img, n):
    ekp, ede = N.orb(img, n)
    kp = np.asarray(kp)
    de = de.cpu().numpy()
    assert len(kp) == len(ekp), f"count {len(kp)} != {len(ekp)}"
    got, exp = kp.view(np.uint32).reshape(-1, 7), ekp.view(np.uint32).reshape(-1, 7)
    bad = np.nonzero((got != exp).any(1))[0]
    assert len(bad) == 0, f"keypoints differ at {bad[:8]}: {kp[bad[:3]]} vs {ekp[bad[:3]]}"
    bad = np.nonzero((de != ede).any(1))[0]
    assert len(bad) == 0, f"descriptors differ at {bad[:8]}"
    return len(kp)


def run(orb, imgs, pitch=False):
    torch = _torch()
    ts = [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs]
    if pitch:
        ts = [pitched(t) for t in ts]
    return orb.detect(*ts)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pitch", [False, True])
def test_synthetic_pair_1242x375(channels, pitch):
    from cartslam import OrbFeatures
    eng = engine()
    orb = OrbFeatures(eng, 1242, 375)
    l, r = synth_pair(1242, 375, 11, channels)
    out = run(orb, [l, r], pitch)
    assert check(*out[0], l, 5000) > 20 and check(*out[1], r, 5000) > 20
    orb.close()


def test_ragged_sizes_and_no_level():
    from cartslam import OrbFeatures
    eng = engine()
    orb = OrbFeatures(eng, 400, 200, nfeatures=1000)
    for w, h in ((333, 129), (97, 71), (320, 96), (63, 63)):
        img = block_noise(h, w, 2, w + h)
        out = run(orb, [img])
        check(*out[0], img, 1000)
    img = block_noise(200, 62, 2, 1)   # no level is built: 62 < 63
    (kp, de), = run(orb, [img])
    assert len(kp) == 0 and de.shape == (0, 32)
    orb.close()


def test_flat_and_saturated_images_give_nothing():
    from cartslam import OrbFeatures
    eng = engine()
    orb = OrbFeatures(eng, 320, 96)
    for v in (0, 128, 255):
        img = np.full((96, 320), v, np.uint8)
        (kp, de), = run(orb, [img])
        assert len(kp) == 0
    orb.close()


def test_checkerboard_ties():
    """Mass ties in R: the candidates of a level exceed its quota and the (y, x) tie-break decides."""
    from cartslam import OrbFeatures
    eng = engine()
    orb = OrbFeatures(eng, 1242, 375)
    img = checkerboard(375, 1242, sq=8)
    (kp, de), = run(orb, [img])
    check(kp, de, img, 5000)
    _, counts = N.orb(img, 5000, want_levels=True)[2:]
    q = N.level_quotas(5000)
    assert any(c > n for c, n in zip(counts, q)), "the checkerboard should overfill a level"
    R, ys, xs = N.detect_level(N.pyramid(img)[1])
    assert len(np.unique(R)) < len(R) // 4, "the checkerboard should tie in R"
    orb.close()


@pytest.mark.parametrize("n", [1, 500, 5000, 20000])
def test_noise_every_n(n):
    from cartslam import OrbFeatures
    eng = engine()
    orb = OrbFeatures(eng, 1242, 375, nfeatures=n)
    a, b = block_noise(375, 1242, 2, 5), np.random.default_rng(6).integers(0, 256, (375, 1242)).astype(np.uint8)
    out = run(orb, [a, b])
    got = check(*out[0], a, n)
    check(*out[1], b, n)
    if n <= 5000:
        assert got == n, "2x2 block noise fills every level's quota"
    orb.close()


def test_stage_by_stage():
    from cartslam import OrbFeatures
    eng = engine()
    orb = OrbFeatures(eng, 1242, 375)
    l, r = synth_pair(1242, 375, 3, 3)
    orb.detect(_torch().from_numpy(l).cuda(), _torch().from_numpy(r).cuda())
    for i, img in enumerate((l, r)):
        levels = N.pyramid(img)
        assert len(levels) == 8
        for lv, L in enumerate(levels):
            got, ncand = orb.debug_level(i, lv)
            assert (got.cpu().numpy() == L).all(), f"image {i} level {lv} pyramid"
            assert ncand == len(N.detect_level(L)[0]), f"image {i} level {lv} candidates"
    orb.close()


def test_pair_equals_singles_and_repeats():
    from cartslam import OrbFeatures
    eng = engine()
    orb = OrbFeatures(eng, 1242, 375)
    l, r = synth_pair(1242, 375, 9, 1)
    pair = run(orb, [l, r])
    again = run(orb, [l, r])
    singles = [run(orb, [l])[0], run(orb, [r])[0]]
    for (k1, d1), (k2, d2), (k3, d3) in zip(pair, again, singles):
        assert k1.tobytes() == k2.tobytes() == k3.tobytes()
        assert (d1 == d2).all() and (d1 == d3).all()
    orb.close()


def test_rejects_bad_arguments():
    from cartslam import EngineError, OrbFeatures
    torch = _torch()
    eng = engine()
    with pytest.raises(EngineError):
        OrbFeatures(eng, 320, 96, nfeatures=0)
    orb = OrbFeatures(eng, 320, 96)
    with pytest.raises(EngineError):
        orb.detect(torch.zeros((97, 320), dtype=torch.uint8, device="cuda"))   # larger than the create size
    with pytest.raises(EngineError):
        orb.detect(torch.zeros((96, 320, 2), dtype=torch.uint8, device="cuda"))
    orb.close()


# ---- the C++ frame loop -----------------------------------------------------------------------------------------------
def _dumped(d, fid, side, n_max):
    kp = np.fromfile(os.path.join(d, f"{fid}_features_{side}_keypoints.bin"), N.KEYPOINT_DTYPE)
    de = np.fromfile(os.path.join(d, f"{fid}_features_{side}_descriptors.bin"), np.uint8).reshape(-1, 32)
    assert len(kp) == len(de) <= n_max
    return kp, de


@pytest.mark.parametrize("channels", [1, 3])
def test_features_module_frame_loop(tmp_path, channels):
    from test_host import make_dataset, run_exe
    tmp = str(tmp_path)
    w, h, n = 320, 96, 3
    src, frames = make_dataset(tmp, n, w, h, channels=channels)
    lists = {"alone": ([{"type": "orb_features"}], 5000),
             "with_disparity": ([{"type": "disparity", "num_disparities": 128, "smoothing_radius": 2, "smoothing_iterations": 1},
                                 {"type": "orb_features", "nfeatures": 800}], 800)}
    for name, (mods, nf) in lists.items():
        d = os.path.join(tmp, "dump_" + name)
        os.makedirs(d)
        r = run_exe(src, mods, tmp, ("--dump", d))
        assert r.returncode == 0, r.stderr
        total = 0
        for fid in range(1, n + 1):
            for side, img in zip(("left", "right"), frames[fid - 1]):
                kp, de = _dumped(d, fid, side, nf)
                ekp, ede = N.orb(img, nf)
                assert kp.tobytes() == ekp.tobytes(), f"{name} frame {fid} {side}: keypoints"
                assert (de == ede).all(), f"{name} frame {fid} {side}: descriptors"
                total += len(kp)
        assert total > 0
    r = run_exe(src, [{"type": "orb_features", "feature_type": "sift"}], tmp)
    assert r.returncode != 0 and "Unknown feature type." in r.stderr

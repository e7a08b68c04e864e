"""CPU checks of the premises behind tests/test_gpu_superpixel_edges.py: every case of tests/sp_cases.py is what its name says, and the
oracle alone (spec S13/S14) moves labels where the case says it must.  The GPU tests compare the device with the same oracle; a case that
turned trivial (no border pixel, no move across a seam, no label that vanishes) would let those comparisons pass for nothing, and fails
here first."""
import numpy as np
import pytest

import oracle_lib as O
import sp_cases as K


def ycc(case, image=None):
    image = case.image if image is None else image
    return O.bgr2ycrcb(image if image.ndim == 3 else np.repeat(image[..., None], 3, axis=2))


def run(case, sweeps=None):
    """-> (labels after the case's sweeps, number of changes)."""
    d2 = case.deriv2 if case.params.get("disparity", 1.0) > 0 else None
    return O.sp_relax(O.sp_params(**case.params), case.labels, case.max_label_id, ycc(case), d2, case.sweeps if sweeps is None else sweeps)


def test_hash_mirror():
    # spot values worked out by hand from (L ^ L >> 6 ^ L >> 11) & 63
    assert [int(K.sp_hash(L)) for L in (0, 63, 64, 65, 2048, 4095, 16383)] == [0, 63, 1, 0, 1 ^ 32, 63 ^ 63 ^ 1, 63 ^ 63 ^ 7]
    classes = np.bincount(K.sp_hash(np.arange(K.MAX_LABELS)), minlength=64)
    assert (classes == 256).all()


@pytest.mark.parametrize("name", sorted(K.RELAX_CASES))
def test_every_relax_case_is_well_formed_and_moves(name):
    c = K.RELAX_CASES[name]()
    assert c.labels.shape == (c.h, c.w) and c.labels.dtype == np.uint16 and c.deriv2.shape == (c.h, c.w, 2) and c.deriv2.dtype == np.int16
    assert c.image.dtype == np.uint8 and c.image.shape[:2] == (c.h, c.w) and c.image.ndim in (2, 3)
    assert 1 <= c.max_label_id < K.MAX_LABELS and int(c.labels.max()) < c.max_label_id and len(np.unique(c.labels)) >= 2
    assert c.w <= 96 and c.h <= (48 if name == "thin_1x48" else 40) and 1 <= c.sweeps <= 4
    got, changes = run(c)
    assert changes > 0 and (got != c.labels).any()
    img2, d2b = K.second_scene(c)
    assert (img2 != c.image).any() and (d2b != c.deriv2).any()
    _, more = O.sp_relax(O.sp_params(**c.params), got, c.max_label_id, ycc(c, img2), d2b if c.params.get("disparity", 1.0) > 0 else None, 1)
    assert more > 0 or name == "thin_2x2", "the second frame of the chain moves labels too"


@pytest.mark.parametrize("n", [63, 64, 65])
@pytest.mark.parametrize("colliding", [False, True])
def test_table_exact(n, colliding):
    c = K.table_exact(n, colliding)
    tile, halo = K.tile_label_counts(c.labels)
    assert (c.w, c.h) == (K.TILE_W, K.TILE_H) and tile.tolist() == [[n]] and halo.tolist() == [[n]]
    ids = np.unique(c.labels)
    classes = np.unique(K.sp_hash(ids))
    if colliding:
        assert classes.tolist() == [K.HASH_CLASS] and 0 < K.HASH_CLASS and c.premise["pool"] >= 255   # one chain, from slot 37 past slot 63
        assert int(ids.max()) > 8192                                                                # ids from the whole range
    else:
        assert len(classes) > 32
    got, changes = run(c)
    assert changes >= 10
    # border pixels of every count the cells allow; the labelling is not a refinement of the scene's 5 x 3 period
    assert set(np.unique(K.neighbour_counts(c.labels))) >= {2, 4}


def test_table_mixed():
    c = K.table_mixed()
    tile, halo = K.tile_label_counts(c.labels)
    assert tile.tolist() == c.premise["tile"] and halo.tolist() == c.premise["halo"]
    assert tile[0, 1] > K.SLOTS and halo[0, 1] > K.SLOTS                       # global memory in both kernels
    assert tile[1, 2] <= K.SLOTS < halo[1, 2]                                  # table in sp_stats_kernel, global memory in sp_relax_kernel
    assert max(halo[0, 0], halo[0, 2], halo[1, 1], halo[1, 0]) <= 20           # table in both
    got, changes = run(c)
    moved = got != c.labels
    for i, j in c.premise["about"]:
        assert moved[j * K.TILE_H:(j + 1) * K.TILE_H, i * K.TILE_W:(i + 1) * K.TILE_W].any(), (i, j)
    for name, (ys, xs) in c.premise["seams"].items():
        band = moved[ys, xs]
        first, second = (band[:, 0], band[:, 1]) if band.shape[1] == 2 else (band[0], band[1])
        assert first.any() and second.any(), name                              # pixels move on both sides of the seam


def test_candidates_all():
    c = K.candidates_all()
    nn = K.neighbour_counts(c.labels)
    hist = np.bincount(nn[nn >= 2], minlength=10)
    assert all(hist[k] > 0 for k in c.premise["counts"]) and hist[10:].sum() == 0, hist
    border = nn >= 2
    assert border[0, 0] and border[0, -1] and border[-1, 0] and border[-1, -1]
    assert border[0, 1:-1].any() and border[-1, 1:-1].any() and border[1:-1, 0].any() and border[1:-1, -1].any()
    tile, halo = K.tile_label_counts(c.labels)
    assert tile.shape == (2, 2) and halo.max() <= K.SLOTS                      # the table path: slot ids, not labels, feed the candidate lists
    _, changes = run(c)
    assert changes > 0


def test_candidates_uniform():
    c = K.candidates_uniform()
    nn = K.neighbour_counts(c.labels)
    assert c.image.ndim == 2 and set(np.unique(nn)) == {1, 2} and (nn == 2).sum() == 2 * 7 * c.h
    _, changes = run(c, 1)
    assert changes > 0


def test_vanishing():
    c = K.vanishing()
    before = np.bincount(c.labels.ravel(), minlength=c.max_label_id)
    assert (before == 1).sum() == c.premise["singles"] >= 40 and (before == 0).sum() > 3000 and (before > 100).sum() == 2
    ones = np.flatnonzero(before == 1)
    ys, xs = np.nonzero(np.isin(c.labels, ones))
    assert all(K.neighbour_counts(c.labels)[y, x] <= 3 for y, x in zip(ys, xs))      # isolated: no two of them touch
    got, _ = run(c, 1)
    after = np.bincount(got.ravel(), minlength=c.max_label_id)
    gone = (before == 1) & (after == 0)
    assert gone.sum() >= 5, "one-pixel labels that vanish in the first sweep"
    assert ((before == 1) & (after >= 1)).sum() >= 1, "and one-pixel labels that stay or grow"


def test_ties():
    c = K.ties()
    assert (c.image == c.image[0, 0]).all() and (c.deriv2 == c.deriv2[0, 0]).all() and c.params == {}
    _, changes = run(c)
    assert changes > 0


def test_ties_cliques_decided_by_candidate_order():
    c = K.ties_cliques()
    p = O.sp_params(**c.params)
    assert p.compactness_weight == p.image_weight == p.disparity_weight == 0
    want, tied = K.clique_sweep(c.labels, p.direct_clique_cost, p.diagonal_clique_cost)
    got, changes = run(c, 1)
    assert changes > 0 and (got == want).all(), "the restatement of the clique term is the oracle's"
    assert tied >= 10
    other, _ = K.clique_sweep(c.labels, p.direct_clique_cost, p.diagonal_clique_cost, dy_outer=True)
    assert (other != want).sum() >= 3, "pixels whose label the candidate order alone decides"


@pytest.mark.parametrize("w,h", sorted(K.THIN))
def test_thin(w, h):
    c = K.thin(w, h)
    bw, bh = c.premise["block"]
    lab, mx = O.sp_block_init(w, h, bw, bh)
    assert (lab == c.labels).all() and mx == c.max_label_id >= 2 and bw <= w and bh <= h and mx < K.MAX_LABELS
    assert K.fits_engine(w, h) == ((w, h) in ((33, 17), (32, 16), (31, 15), (20, 40)))
    tile, _ = K.tile_label_counts(c.labels)
    assert tile.shape == {(33, 17): (2, 2), (20, 40): (3, 1), (1, 48): (3, 1), (48, 1): (1, 2)}.get((w, h), (1, 1))      # tiles (y, x)


def test_extremes():
    c = K.extremes()
    assert {32767, -32767, K.INVALID} <= set(np.unique(c.deriv2)) and set(np.unique(c.image)) == {0, 255}
    assert c.max_label_id == 16383 and int(c.labels.max()) == 16382 and int(c.labels.min()) == 0
    _, changes = run(c)
    assert changes > 0


@pytest.mark.parametrize("k", range(len(K.CLASSIFY)))
def test_classify_cases(k):
    w, kind, n_prev = K.CLASSIFY[k]
    c = K.classify_case(w, kind, n_prev)
    assert (c.w, c.h) == (w, 9) and len(c.prev) == len(c.flows) == n_prev and all(int(p.max()) <= 2 for p in c.prev)
    over = c.labels >= c.max_label
    assert over.any() and (~over).any() and (c.labels == 0xFFFF).any()
    if kind == "full":
        assert c.max_label == K.MAX_LABELS and (c.labels == 16383).any() and not (c.labels == 16384).any()
    else:
        assert (c.labels == c.max_label).any() and (c.labels == c.max_label - 1).any()
    if w > 18:
        assert set(c.premise["starts"]) >= {15, 0, 1, 2}, "runs that start at x = 15, 16, 17, 18 (mod 16)"
    elif w == 17:
        assert set(c.premise["starts"]) >= {15, 0}
    for f in c.flows:       # flows that leave the image on every side, and flows that stay
        x = np.arange(w)[None, :] - (f[..., 0] >> 5)
        y = np.arange(c.h)[:, None] - (f[..., 1] >> 5)
        assert (x < 0).any() and (x >= w).any() and (y < 0).any() and (y >= c.h).any() and ((x >= 0) & (x < w) & (y >= 0) & (y < c.h)).any()
    uns, planes = O.sp_classify(c.deriv2, c.labels, c.max_label, c.params, c.prev, c.flows)
    assert len(np.unique(planes)) >= 2 and len(np.unique(uns)) == 3
    assert (planes[over] == 2).all() and (planes[~over] != 2).any()

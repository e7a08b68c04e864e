"""GPU tests of the ORB stage (csrc/orb_kernels.hip, csrc/engine_orb.hip) at the places test_gpu_features.py does not reach, through
the C ABI (cart_orb_detect with ctypes) on buffers the test lays out itself.

Every input comes from orb_patterns.py, which also says what it does to the kernels; test_orb_patterns.py checks those premises
without a GPU, and each test here asserts the ones it rests on again before it compares.  Every comparison is bit-exact against np_orb:
keypoints as raw 32-bit words, descriptors as bytes.  Every output lies in a sentinel-filled allocation (Buf of test_gpu_post_layout.py):
the rows at and past counts[i], the gaps between descriptor rows and the bytes around the buffers must keep the sentinel.

  a  test_deep_radix_passes, test_big_lattice, test_two_class_lattice: orb_select_kernel's radix passes 2..6 (the straddling digit 5
     included) with the threshold inside one class of R of more than 2048 survivors; 1, 2 and 7 rank chunks
  b  test_sel_finish_boundary: exactly 2048 survivors (no pass, the LDS finish buffer exactly full) and 2080 (seven passes)
  c  test_on_ray_and_zero_moments: orb_describe_kernel's `c0 >= 0 && c1 < 0` with the centroid exactly on rays 7 and 22, and hits == 0
  d  test_seam_lattices, test_plateau_on_the_seams: corners on the first / last column and row of the detect tiles and of the
     candidate region, equal scores across the seams
  e  test_pair_with_one_flat_image: keep == 0 in every select block of one image
  f  test_layouts: descriptor steps, output bases inside larger buffers, per-image source steps, odd source addresses
  g  test_refusals_*: one per entry point
  h  test_call_order_on_one_stream

Digit 7 of the selection key is not tested, because no input reaches it: see the module text of orb_patterns.py.
"""
import ctypes as C

import numpy as np
import pytest

import np_orb as N
import orb_patterns as P
from test_gpu_post_layout import Buf, _torch, engine, flat, lib, ok, refused

pytestmark = pytest.mark.gpu

SENT, S32 = 0xA5, 0x5A5B5C5D     # output sentinels: no keypoint word (0xA5A5A5A5 is neither -1 nor a float of any case), no count
SRC_FILL = 255                   # the slack of a source image holds the dots' value: a kernel that read it would see other corners


class Obj:
    def __init__(self, w, h, nfeatures):
        self.h, self.n = C.c_void_p(), nfeatures
        eng = engine(64, 32)      # before lib(): torch's HIP runtime first, then the library's
        ok(lib().cart_orb_create(eng._h, w, h, nfeatures, C.byref(self.h)))

    def close(self):
        lib().cart_orb_destroy(self.h)


def source(img, step=None, base=0):
    return Buf(np.ascontiguousarray(img)[None], step=step, base=base, fill=SRC_FILL)


class Out:
    """The outputs of one cart_orb_detect call of `n` images on an object of `nfeat` features, each in its own sentinel-filled allocation."""

    def __init__(self, n, nfeat, desc_steps=None, kp_bases=(0, 0), de_bases=(0, 0)):
        self.nfeat = nfeat
        self.kp = [Buf(np.full((1, nfeat, 28), SENT, np.uint8), base=kp_bases[i], fill=SENT) for i in range(n)]
        self.de = [Buf(np.full((1, nfeat, 32), SENT, np.uint8), step=desc_steps[i] if desc_steps else None, base=de_bases[i], fill=SENT)
                   for i in range(n)]
        self.counts = flat(np.full(4, S32, np.int32), S32)
        self.args = dict(kps=(C.c_void_p * n)(*[b.ptr for b in self.kp]), des=(C.c_void_p * n)(*[b.ptr for b in self.de]),
                         dsteps=(C.c_size_t * n)(*desc_steps) if desc_steps else None, counts=C.c_void_p(self.counts.ptr))

    def untouched(self):
        return all(b.untouched() for b in self.kp + self.de + [self.counts])

    def count(self, i):
        c = self.counts.image().ravel()
        assert (c[len(self.kp):] == S32).all(), "counts past n_images were written"
        return int(c[i])

    def result(self, i):
        """-> (keypoints [count] KEYPOINT_DTYPE, descriptors [count, 32]) of image i, after the check that nothing else was written."""
        cnt = self.count(i)
        assert 0 <= cnt <= self.nfeat, cnt
        kp, de = self.kp[i].image()[0], self.de[i].image()[0]      # image(): no slack byte changed
        assert (kp[cnt:] == SENT).all() and (de[cnt:] == SENT).all(), "rows at and past counts[i] were written"
        return np.ascontiguousarray(kp[:cnt]).view(N.KEYPOINT_DTYPE).reshape(-1), de[:cnt]


def detect(o, srcs, channels, width, height, out, stream=None, **kw):
    """cart_orb_detect -> its return value; kw replaces single arguments (the refusal tests)."""
    n = len(srcs)
    a = dict(orb=o.h, n=n, images=(C.c_void_p * n)(*[s.ptr for s in srcs]), steps=(C.c_size_t * n)(*[s.step for s in srcs]), ch=channels, w=width,
             h=height, stream=stream, **out.args)
    a.update(kw)
    return lib().cart_orb_detect(a["orb"], a["n"], a["images"], a["steps"], a["ch"], a["w"], a["h"], a["kps"], a["des"], a["dsteps"], a["counts"],
                                 a["stream"])


def same_bits(kp, de, ekp, ede, what):
    assert len(kp) == len(ekp), f"{what}: count {len(kp)} != {len(ekp)}"
    got, exp = kp.view(np.uint32).reshape(-1, 7), ekp.view(np.uint32).reshape(-1, 7)
    bad = np.nonzero((got != exp).any(1))[0]
    assert len(bad) == 0, f"{what}: keypoints differ at {bad[:8]}: {kp[bad[:3]]} vs {ekp[bad[:3]]}"
    bad = np.nonzero((de != ede).any(1))[0]
    assert len(bad) == 0, f"{what}: descriptors differ at {bad[:8]}"


def check(out, i, name, nfeat):
    ekp, ede, _ = P.expected(name, nfeat)
    same_bits(*out.result(i), ekp, ede, f"{name} N={nfeat}")
    return len(ekp)


def check_level_counts(o, image, name, nfeat):
    """cart_orb_debug_level's survivor count of every built level against np_orb."""
    counts = P.expected(name, nfeat)[2]
    h, w = P.image(name).shape[:2]
    assert len(counts) == N.built_levels(w, h)
    for lv, c in enumerate(counts):
        n = C.c_int32(-1)
        ok(lib().cart_orb_debug_level(o.h, image, lv, None, 0, C.byref(n), None))
        assert n.value == c, f"{name}: level {lv} has {n.value} survivors, np_orb {c}"


def run_single(name, nfeat, channels=1, levels=False):
    img = P.image(name)
    h, w = img.shape
    o = Obj(w, h, nfeat)
    try:
        src, out = source(P.gray3(img) if channels == 3 else img), Out(1, nfeat)
        ok(detect(o, [src], channels, w, h, out))
        n = check(out, 0, name, nfeat)
        if levels:
            check_level_counts(o, 0, name, nfeat)
        assert src.untouched()
    finally:
        o.close()
    return n


# ---- a. deep radix passes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeat,quota,passes,chunks", [(500, 109, 7, (1, 1)), (5000, 1086, 7, (1, 2)), (12000, 2606, 7, (2, 3)), (65536, 14233, 0, (2, 3))])
def test_deep_radix_passes(nfeat, quota, passes, chunks):
    """400 x 200 dot lattice: 2856 level-0 survivors in ONE class of R.  A quota below that puts the threshold among the ties: digits 0..5
    hold one bin each, digit 6 one per row, so seven passes run and one row's 84 keys finish in LDS.  quota 2606 > 2048 ranks in two
    chunks with 3 records a thread; quota 14233 > c selects nothing and keeps all."""
    f = P.selection_facts("lattice", nfeat)
    assert (f["c"], f["classes"], f["quota"], f["keep"]) == (2856, 1, quota, min(quota, 2856))
    assert f["trace"]["passes"] == passes and f["trace"]["finish"] == (84 if passes else 0) and P.rank_chunks(f["keep"]) == chunks
    assert run_single("lattice", nfeat, levels=True) > f["keep"]      # further levels add to level 0's share


def test_big_lattice():
    """1242 x 375, N = 65536: 23010 survivors in one class above the quota of 14233; seven rank chunks, 14 records a thread, and y >= 256
    gives digit 5 a second bin."""
    f = P.selection_facts("lattice_big", 65536)
    assert (f["c"], f["classes"], f["quota"]) == (23010, 1, 14233) and P.rank_chunks(f["keep"]) == (7, 14)
    assert f["trace"]["passes"] == 7 and f["trace"]["bins"][5] == 2
    run_single("lattice_big", 65536, levels=True)


@pytest.mark.parametrize("nfeat,passes,finish", [(500, 2, 504), (5000, 7, 84)])
def test_two_class_lattice(nfeat, passes, finish):
    """Four classes of R, the largest (2184) last: N = 5000 subtracts the 672 keys of the classes above in pass 1 and walks on through the
    deep digits; N = 500 stops after the pass that isolates the first class."""
    f = P.selection_facts("two_class", nfeat)
    assert f["classes"] == 4 and f["quota"] < f["c"] == 2856 and (f["trace"]["passes"], f["trace"]["finish"]) == (passes, finish)
    run_single("two_class", nfeat, levels=True)


# ---- b. the kSelFinish boundary ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeat", [500, 5000])
@pytest.mark.parametrize("name,c,passes,finish", [("lattice_full", 2048, 0, 2048), ("lattice_over", 2080, 7, 65)])
def test_sel_finish_boundary(name, c, passes, finish, nfeat):
    """Exactly kSelFinish survivors: `s_matched > kSelFinish` is false at once and the finish buffer holds all 2048 keys; 32 more and
    the passes run.  Quotas 109 and 1086, both below c."""
    f = P.selection_facts(name, nfeat)
    assert (f["c"], f["classes"]) == (c, 1) and f["quota"] < c
    assert (f["trace"]["passes"], f["trace"]["finish"]) == (passes, finish)
    run_single(name, nfeat, levels=True)


# ---- c. on-ray and zero moments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", ["ramp:down", "ramp:up", "ramp:right", "ramp:left", "plain"])
def test_on_ray_and_zero_moments(name, channels):
    R, ys, xs = P.survivors(name)
    m10, m01 = N.moments(P.image(name), ys, xs)
    kind, _, direction = name.partition(":")
    if kind == "plain":
        assert (m10 == 0).all() and (m01 == 0).all()
        bin_ = 0
    else:
        sign = 1 if direction in ("down", "right") else -1
        on, off = (m10, m01) if direction in ("down", "up") else (m01, m10)
        assert (on == 0).all() and (np.sign(off) == sign).all()
        bin_ = P.RAMPS[direction]
    kp = P.expected(name, 2000)[0]
    k0 = kp[kp["octave"] == 0]
    assert len(k0) == len(R) == 384 and (k0["angle"] == np.float32(12 * bin_)).all()
    run_single(name, 2000, channels)


# ---- d. tile and region seams -----------------------------------------------------------------------------------------------------
def test_seam_lattices():
    """160 x 100, all 16 phases of the lattice: dots on the first and last column and row of the tiles (31 | 94, 95 | 128 and
    31 | 46, 47 | 62, 63 | 68), the last tile of each direction partial."""
    h, w = P.SEAM_SIZE
    cols, rows = P.tile_edges(h, w)
    seen_c, seen_r = set(), set()
    o = Obj(w, h, 5000)
    try:
        for ox in range(4):
            for oy in range(4):
                name = f"seam:{ox}{oy}"
                kp = P.expected(name, 5000)[0]
                k0 = kp[kp["octave"] == 0]
                seen_c |= set(k0["x"].astype(int).tolist()) & cols
                seen_r |= set(k0["y"].astype(int).tolist()) & rows
                src, out = source(P.image(name)), Out(1, 5000)
                ok(detect(o, [src], 1, w, h, out))
                check(out, 0, name, 5000)
                check_level_counts(o, 0, name, 5000)
        assert seen_c == cols == {31, 94, 95, 128} and seen_r == rows == {31, 46, 47, 62, 63, 68}
    finally:
        o.close()


def test_plateau_on_the_seams():
    """Equal bright pairs and 2 x 2 blocks inside a tile, across x = 94 | 95, across y = 46 | 47 and 62 | 63, on the corner of four tiles
    and on the ends of the candidate region: strict NMS must drop both sides of an equal pair whichever tile computed the neighbour's score."""
    drops = P.equal_drops(P.image("plateau"))
    assert {(35, 40), (35, 41), (35, 94), (35, 95), (46, 40), (47, 40), (46, 94), (46, 95), (47, 94), (47, 95), (40, 31), (68, 128)} <= drops
    R, ys, xs = P.survivors("plateau")
    assert {(52, 94), (57, 95), (46, 50), (47, 60), (62, 94), (55, 31), (55, 128), (31, 105), (68, 105)} <= set(zip(ys.tolist(), xs.tolist()))
    assert run_single("plateau", 5000, levels=True) >= 15


# ---- e. pairs with unequal content -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flat_first", [True, False])
def test_pair_with_one_flat_image(flat_first):
    h, w = P.image("lattice").shape
    names = ["flat:200x400", "lattice"] if flat_first else ["lattice", "flat:200x400"]
    full = names.index("lattice")
    assert len(P.expected("flat:200x400", 5000)[0]) == 0
    o = Obj(w, h, 5000)
    try:
        out = Out(2, 5000)
        ok(detect(o, [source(P.image(n)) for n in names], 1, w, h, out))
        assert out.count(1 - full) == 0 and out.kp[1 - full].untouched() and out.de[1 - full].untouched()
        assert check(out, full, "lattice", 5000) == out.count(full) > 0
        single = Out(1, 5000)
        ok(detect(o, [source(P.image("lattice"))], 1, w, h, single))
        (k2, d2), (k1, d1) = out.result(full), single.result(0)
        assert k2.tobytes() == k1.tobytes() and (d2 == d1).all()
    finally:
        o.close()


# ---- f. layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dstep", [32, 48, 33])
def test_layouts(dstep, channels):
    """Two images of different source steps at odd addresses, keypoints 4 but not 16 bytes into their allocation, descriptors at an odd
    base with `dstep` bytes a row (the second image one more where dstep > 32): nothing but the first counts[i] rows is written."""
    names, nfeat = ["ramp:down", "ramp:left"], 2000
    h, w = P.image(names[0]).shape
    row = w * channels
    imgs = [P.gray3(P.image(n)) if channels == 3 else P.image(n) for n in names]
    srcs = [source(imgs[0], step=row + 1, base=1), source(imgs[1], step=row + 6, base=259)]
    dsteps = [dstep, dstep + (dstep > 32)]
    out = Out(2, nfeat, desc_steps=dsteps, kp_bases=(4, 20), de_bases=(1, 7))
    assert all(s.ptr % 2 == 1 for s in srcs) and all(b.ptr % 16 == 4 for b in out.kp)
    o = Obj(w, h, nfeat)
    try:
        ok(detect(o, srcs, channels, w, h, out))
        for i, name in enumerate(names):
            assert 0 < check(out, i, name, nfeat) < nfeat      # there are rows past counts[i]
        assert all(s.untouched() for s in srcs)
    finally:
        o.close()


# ---- g. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_create():
    eng = engine(64, 32)      # before lib(), as in Obj
    L = lib()
    made = C.c_void_p()
    refused(L.cart_orb_create(None, 160, 100, 500, C.byref(made)), "bad arguments")
    refused(L.cart_orb_create(eng._h, 160, 100, 500, None), "bad arguments")
    for n in (0, 65537, -1):
        refused(L.cart_orb_create(eng._h, 160, 100, n, C.byref(made)), "nfeatures must be in [1, 65536]")
    for w, h in ((0, 100), (160, 0), (16385, 100), (160, 16385), (-1, 100)):
        refused(L.cart_orb_create(eng._h, w, h, 500, C.byref(made)), "max_width / max_height must be in [1, 16384]")
    assert not made.value
    assert run_single("seam:00", 500) > 0      # the engine still makes objects that work


def test_refusals_levels():
    engine(64, 32)      # host only, but the library must not load ahead of torch's runtime for the tests that follow
    L = lib()
    arr = [(C.c_int * 8)(*[S32] * 8) for _ in range(3)]
    for n in (0, 65537):
        refused(L.cart_orb_levels(160, 100, n, *arr), "nfeatures must be in [1, 65536]")
    for w, h in ((0, 100), (160, 0), (16385, 100), (160, 16385)):
        refused(L.cart_orb_levels(w, h, 500, *arr), "width / height must be in [1, 16384]")
    assert all(list(a) == [S32] * 8 for a in arr)
    assert L.cart_orb_levels(160, 100, 500, *arr) == 3 == N.built_levels(160, 100)
    assert [(arr[0][l], arr[1][l]) for l in range(8)] == [(a, b) for a, b, _ in N.level_sizes(160, 100)] and list(arr[2]) == N.level_quotas(500)
    assert L.cart_orb_levels(16384, 16384, 65536, None, None, None) == 8


def test_refusals_detect():
    names, nfeat = ["seam:13", "plateau"], 500
    h, w = P.SEAM_SIZE
    srcs, out = [source(P.image(n), step=w + 3) for n in names], Out(2, nfeat, desc_steps=[40, 40])
    o = Obj(w, h, nfeat)

    def arr(kind, values):
        return (kind * len(values))(*values)

    def no(word, **kw):
        refused(detect(o, srcs, 1, w, h, out, **kw), word)

    try:
        no("orb is NULL", orb=None)
        for n in (0, 3, -1):
            no("n_images must be 1 or 2", n=n)
        for name in ("images", "steps", "kps", "des", "counts"):
            no("NULL pointer", **{name: None})
        for ch in (2, 0, 4):
            no("channels must be 1 or 3", ch=ch)
        for kw in (dict(w=w + 1), dict(h=h + 1), dict(w=0), dict(h=0)):
            no("image size outside [1, create size]", **kw)
        for i in (0, 1):      # the per-image checks, for either image
            ptrs = lambda bufs, bad: arr(C.c_void_p, [bad if j == i else b.ptr for j, b in enumerate(bufs)])
            no("NULL image / output pointer", images=ptrs(srcs, None))
            no("NULL image / output pointer", kps=ptrs(out.kp, None))
            no("NULL image / output pointer", des=ptrs(out.de, None))
            no("bad step", steps=arr(C.c_size_t, [w - 1 if j == i else w + 3 for j in range(2)]))
            no("bad step", ch=3, steps=arr(C.c_size_t, [3 * w - 1 if j == i else 3 * w for j in range(2)]))
            for off in (1, 2, 3):
                no("keypoints must be 4-byte aligned", kps=ptrs(out.kp, out.kp[i].ptr + off))
            for bad in (31, 0):
                no("descriptor step must be >= 32", dsteps=arr(C.c_size_t, [bad if j == i else 40 for j in range(2)]))
        refused(lib().cart_orb_debug_level(o.h, 0, 0, None, 0, None, None), "image not part of the last detect call")      # none of them was a call
        _torch().cuda.synchronize()
        assert out.untouched()
        ok(detect(o, srcs, 1, w, h, out))
        for i, name in enumerate(names):
            assert check(out, i, name, nfeat) > 0
            check_level_counts(o, i, name, nfeat)
    finally:
        o.close()


def test_refusals_debug_level():
    """After a one-image call of 160 x 100 (three levels) on an object made for 400 x 200 (seven)."""
    name, nfeat = "seam:31", 500
    h, w = P.SEAM_SIZE
    o = Obj(400, 200, nfeat)
    levels = N.pyramid(P.image(name))
    assert len(levels) == 3 and N.built_levels(400, 200) == 7
    dst = Buf(np.full((1, h, w), SENT, np.uint8), step=w + 5, base=3, fill=SENT)
    n = C.c_int32(S32)

    def level(image=0, lv=0, ptr=dst.ptr, step=dst.step, orb=o.h):
        return lib().cart_orb_debug_level(orb, image, lv, ptr, step, C.byref(n), None)

    try:
        refused(level(), "image not part of the last detect call")      # no call yet
        out = Out(1, nfeat)
        ok(detect(o, [source(P.image(name))], 1, w, h, out))
        refused(level(orb=None), "orb is NULL")
        for image in (-1, 1, 2):
            refused(level(image=image), "image not part of the last detect call")
        for lv in (-1, 3, 6, 7, 8):      # 3..6 exist in the object, 3 is the first one that this call did not build
            refused(level(lv=lv), "level not built by the last detect call")
        refused(level(step=w - 1), "bad step")
        refused(level(lv=1, step=levels[1].shape[1] - 1), "bad step")
        _torch().cuda.synchronize()
        assert dst.untouched() and n.value == S32
        check(out, 0, name, nfeat)
        for lv, L in enumerate(levels):
            lh, lw = L.shape
            d = Buf(np.full((1, lh, lw), SENT, np.uint8), step=lw + 5, base=3, fill=SENT)
            ok(level(lv=lv, ptr=d.ptr, step=d.step))
            assert (d.image()[0] == L).all() and n.value == P.expected(name, nfeat)[2][lv]
    finally:
        o.close()


# ---- h. call order on one object ----------------------------------------------------------------------------------------------------
def test_call_order_on_one_stream():
    """400 x 200 with seven levels, 160 x 100 with three, 400 x 200 again (another image) on one non-default stream without a host
    synchronisation in between: each call's own result, and cart_orb_debug_level speaks of the last one."""
    torch = _torch()
    names, nfeat = ["two_class", "seam:22", "lattice"], 5000
    o = Obj(400, 200, nfeat)
    try:
        srcs = [source(P.image(n)) for n in names]
        outs = [Out(1, nfeat) for _ in names]
        lv = 5
        L = N.pyramid(P.image("lattice"))[lv]
        d = Buf(np.full((1,) + L.shape, SENT, np.uint8), step=L.shape[1] + 3, base=1, fill=SENT)
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()      # the uploads are done before the other stream starts
        for name, src, out in zip(names, srcs, outs):
            h, w = P.image(name).shape
            ok(detect(o, [src], 1, w, h, out, stream=C.c_void_p(stream.cuda_stream)))
        n = C.c_int32(-1)
        ok(lib().cart_orb_debug_level(o.h, 0, lv, d.ptr, d.step, C.byref(n), C.c_void_p(stream.cuda_stream)))      # waits for the stream
        stream.synchronize()
        assert n.value == P.expected("lattice", nfeat)[2][lv] != P.expected("two_class", nfeat)[2][lv]
        assert (d.image()[0] == L).all() and not (L == N.pyramid(P.image("two_class"))[lv]).all()
        for name, out in zip(names, outs):
            assert check(out, 0, name, nfeat) > 0
    finally:
        o.close()

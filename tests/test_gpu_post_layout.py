"""GPU tests of the post-stage entry points (csrc/engine_post.hip, csrc/post_kernels.hip) on buffers whose layout the test chooses.

The Python wrappers of cartslam/engine.py allocate every output tight, so through them no kernel ever sees an output row step above a
row, a frame stride above a frame or a base that is not the start of an allocation.  Here the C ABI is called with ctypes on one flat device
allocation per image (Buf): row step, frame stride and base offset are the test's own, the slack of an input holds values that would change
the result if a kernel read them, the slack of an output holds a sentinel that must be intact afterwards -- one exact comparison over the whole
slack (row tails, the rows between frames, the bytes before the base and after the last frame).  Expected values come from the CPU oracle on
the tight host arrays and are compared exactly; beside every comparison stands a premise that the expected output is not trivial.

The layouts (geom()):
  tight           the control; what the existing wrapper returns must equal it
  steps           input rows at the smallest legal step above tight, output rows one alignment unit above that (s16 images: see s16_step)
  steps_swapped   the same with the two kinds of step exchanged
  offset          the base one element past the (256-byte aligned) start of the allocation, where the ABI allows it
  frames          three frames, 2 * step + 6 bytes between frames (+ 8 where the ABI wants the stride on 4 bytes); batched stages only
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

INV = -32768
SIZES = [(16, 8), (67, 9), (130, 33), (257, 37)]      # 257 x 37: one column in the fifth 64-column block, past the 16- and 32-row blocks, past a CCL tile both ways
SINGLE = ["tight", "steps", "steps_swapped", "offset"]
BATCHED = SINGLE + ["frames"]
MAX_TEMPORAL = 8                                      # CART_MAX_TEMPORAL
S8, S16, S32, SF = 0xA5, 0x5A5B, 0x5A5B5C5D, -7777.25  # sentinels: no label, and values no case below produces
PARAMS = [(6, 18, -5, 6, 11, 0), (-3, 2, 2, 40, 0, 20), (0, 0, 0, 0, 0, 0)]
KITTI_Q = O.kitti_q_matrix([718.856, 0, 607.1928, 45.38225, 0, 718.856, 185.2157, -0.113, 0, 0, 1, 0.0037],
                           [718.856, 0, 607.1928, -337.2877, 0, 718.856, 185.2157, 2.369, 0, 0, 1, 0.0049])


def _torch():
    import torch
    return torch


def lib():
    from cartslam import _lib
    return _lib.load()


_ENGINES = {}


def engine(w, h):
    from cartslam import Engine
    if (w, h) not in _ENGINES:
        _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's
        _ENGINES[(w, h)] = Engine(w, h, num_disparities=0, paths=0, max_inflight=4)
    return _ENGINES[(w, h)]


def ok(rc):
    assert rc == 0, lib().cart_last_error(None).decode()


def refused(rc, word):
    err = lib().cart_last_error(None).decode()
    assert rc != 0 and word in err, (rc, word, err)


# ---- the layout helper -----------------------------------------------------------------------------------------------------
class Buf:
    """The host array a = [n, h, w(, c)] in ONE flat device allocation: frame f, row y starts base + f * fs + y * step bytes into it.
    Everything else -- row tails, rows between frames, the bytes before the base and `tail` bytes behind the last frame -- is slack and
    holds `fill` (element-aligned with the rows).  ptr = device address of frame 0."""

    def __init__(self, a, step=None, fs=None, base=0, fill=0, tail=64):
        a = np.ascontiguousarray(a)
        n, h = a.shape[:2]
        rows = a.reshape(n, h, -1).view(np.uint8)
        row = rows.shape[2]
        step = row if step is None else step
        fs = h * step if fs is None else fs
        assert step >= row and fs >= h * step
        total = base + n * fs + tail
        pattern = np.array([fill], a.dtype).view(np.uint8)
        host = pattern[(np.arange(total) - base) % a.itemsize]
        self.index = base + np.arange(n)[:, None, None] * fs + np.arange(h)[None, :, None] * step + np.arange(row)[None, None, :]
        host[self.index] = rows
        self.slack = np.ones(total, bool)
        self.slack[self.index] = False
        self.host, self.shape, self.dtype, self.step, self.fs, self.base = host, a.shape, a.dtype, step, fs, base
        self.dev = _torch().from_numpy(host).cuda()
        assert self.dev.data_ptr() % 256 == 0   # an "aligned allocation start": misalignment comes from `base` alone
        self.ptr = self.dev.data_ptr() + base

    def read(self):
        """-> (image part as an array of the original shape, slack bytes) of the allocation as it is now."""
        now = self.dev.cpu().numpy()
        return now[self.index].view(self.dtype).reshape(self.shape), now[self.slack]

    def image(self):
        """The image part, after the check that NO slack byte changed."""
        image, slack = self.read()
        assert np.array_equal(slack, self.host[self.slack]), f"{int((slack != self.host[self.slack]).sum())} slack bytes were written"
        return image

    def untouched(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


def s16_step(row, kind):
    """Smallest step above a tight s16 row that is = 2 (mod 4) bytes (kind "a") or = 0 (mod 8) bytes (kind "b")."""
    s = row + 2
    while (s % 4 != 2) if kind == "a" else (s % 8 != 0):
        s += 2
    return s


def geom(layout, role, row, h, align, s16=False, k=0):
    """-> (step, frame stride, base offset) in bytes of an image with rows of `row` bytes whose step, stride and base the ABI wants on
    `align` bytes.  role "in" / "out": the two get different steps; k: a further `align` bytes per k (tables of images)."""
    if layout == "tight":
        return row, h * row, 0
    if layout == "offset":
        return row, h * row, align        # one element (or, for outputs written as 4-byte words, one word) past the allocation's start
    kind_a = (role == "in") != (layout == "steps_swapped")
    if layout == "frames_vec":
        kind_a = False
    if s16:
        step = s16_step(row, "a" if kind_a else "b")
    else:
        step = row + (1 if kind_a else 2) * align + k * align
    assert step % align == 0 and step > row
    fs = h * step
    if layout == "frames":
        fs += 2 * step + 6 + (2 if align == 4 else 0)
    elif layout == "frames_vec":
        fs += 2 * step + 8
    assert fs % align == 0
    return step, fs, 0


def place(a, layout, role, fill, align=None, s16=False, k=0):
    a = np.ascontiguousarray(a)
    step, fs, base = geom(layout, role, a[0, 0].nbytes, a.shape[1], a.itemsize if align is None else align, s16, k)
    return Buf(a, step, fs, base, fill)


def flat(a, fill):
    """A contiguous array (histogram, table, counters) 64 bytes into its allocation, sentinel before and behind it."""
    return Buf(np.ascontiguousarray(a).reshape(1, 1, -1), base=64, fill=fill)


def frames_of(layout):
    return 3 if layout.startswith("frames") else 2


def dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def disparities(seed, n, h, w):
    """Random disparities, 15 % invalid, with the s16 wrap values of test_plane_stages (and a vertical pair four rows apart)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(64, 200, (n, h, w)).astype(np.int16)
    d[rng.random(d.shape) < 0.15] = INV
    d[0, 5, 5] = 32767; d[0, 3, 5] = -32767; d[0, 1, 5] = -32767; d[0, 6, 7] = 32767; d[0, 6, 3] = -32767
    return d


def both(a, invalid=INV):
    return bool((a == invalid).any() and (a != invalid).any())


# ---- cart_interpolate ------------------------------------------------------------------------------------------------------
# Which loads interpolate_r2_kernel (radius 2) does on the CALLER's buffer (pass 0; later passes read the tight workspaces), from
# post_kernels.hip:62-63 (vec = base, step and frame stride all on 4 bytes), :73 (vector load where 2 <= xb and xb + 6 <= w, xb = 4 * thread)
# and :97 (vector store of the tight workspace row, not of the caller's buffer):
#   tight          16 x 8 (step 32) and 130 x 33 (step 260, stride 8580): vec -> vector interior, scalar at xb = 0 and in the last group(s)
#                  67 x 9 (step 134) and 257 x 37 (step 514): step = 2 (mod 4) -> scalar everywhere
#   steps          step = 2 (mod 4)                              -> scalar everywhere
#   steps_swapped  step = 0 (mod 8), stride h * step            -> vector interior + scalar edges; with w % 4 != 0 (67, 130, 257) the last group
#                  is partial: the mix of vector interior and bounds-checked scalar edge on a pitched row
#   offset         base = 2 (mod 4)                              -> scalar everywhere
#   frames         step = 2 (mod 4), stride = h * step + 2 * step + 6    -> scalar everywhere, frames 1 and 2 at a non-tight stride
#   frames_vec     step = 0 (mod 8), stride = h * step + 2 * step + 8    -> the vector path on frames 1 and 2 at a non-tight stride
@pytest.mark.parametrize("layout", BATCHED + ["frames_vec"])
@pytest.mark.parametrize("w,h", SIZES)
def test_interpolate_in_place(w, h, layout):
    eng, n = engine(w, h), frames_of(layout)
    rng = np.random.default_rng(w * 31 + h)
    for max_disp in (w, 4096):
        in_range = max_disp > w or w >= 130          # (64, w) holds no or two values at w = 16 and 67: every window stays below its count
        lo, hi = (66, w + 4) if max_disp == w and in_range else (40, 1400)
        d = rng.integers(lo, hi, (n, h, w)).astype(np.int16)
        d[rng.random(d.shape) < 0.3] = INV
        for radius in (1, 2, 3):
            for iterations in (1, 3):
                buf = place(d, layout, "in", fill=65, s16=True)      # 65: a valid disparity in every range used here
                ok(lib().cart_interpolate(eng._h, n, buf.ptr, buf.step, buf.fs, radius, iterations, 64, max_disp, None))
                exp = np.stack([O.interpolate(d[f], radius, iterations, 64, max_disp) for f in range(n)])
                if radius == 1:
                    assert (exp == INV).all()       # a window of one pixel never counts more than r * r + 1 = 2
                elif in_range:
                    assert both(exp)                # filled and invalid pixels both occur (image corners stay invalid at every radius)
                got = buf.image()
                assert np.array_equal(got, exp), (max_disp, radius, iterations, int((got != exp).sum()))
                if layout == "tight":
                    assert np.array_equal(eng.interpolate(dev(d), radius, iterations, 64, max_disp).cpu().numpy(), exp)


# ---- cart_disparity_derivative ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", BATCHED)
@pytest.mark.parametrize("w,h", SIZES)
def test_disparity_derivative(w, h, layout):
    eng, n = engine(w, h), frames_of(layout)
    d = disparities(w + h, n, h, w)
    src = place(d, layout, "in", fill=100, s16=True)
    out = place(np.full((n, h, w, 2), S16, np.int16), layout, "out", fill=S16, align=4)
    hist = flat(np.full(n * 512, S32, np.int32), S32)      # overwritten, not added to
    assert src.step != out.step and (layout != "frames" or src.fs != out.fs)
    ok(lib().cart_disparity_derivative(eng._h, n, src.ptr, src.step, src.fs, out.ptr, out.step, out.fs, hist.ptr, None))
    exp = [O.directional_derivative(d[f]) for f in range(n)]
    exp_d, exp_h = np.stack([e[0] for e in exp]), np.stack([e[1] for e in exp])
    assert both(exp_d[..., 0]) and both(exp_d[..., 1]) and (exp_h.sum(axis=(1, 2)) > 0).all()
    assert exp_d[0, 3, 5, 0] == -2 and exp_d[0, 6, 5, 1] == -2      # 32767 - (-32767) wraps to -2
    assert np.array_equal(out.image(), exp_d)
    assert np.array_equal(hist.image().reshape(n, 256, 2), exp_h)
    assert src.untouched()
    if layout == "tight":
        wd, wh = eng.disparity_derivative(dev(d))
        assert np.array_equal(wd.cpu().numpy(), exp_d) and np.array_equal(wh.cpu().numpy(), exp_h)


# ---- cart_plane_derivative_hist --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", BATCHED)
@pytest.mark.parametrize("w,h", SIZES)
def test_plane_derivative_hist(w, h, layout):
    eng, n = engine(w, h), frames_of(layout)
    d = disparities(2 * w + h, n, h, w)
    src = place(d, layout, "in", fill=100, s16=True)
    exp = [O.plane_derivative(d[f]) for f in range(n)]
    exp_d, exp_h = np.stack([e[0] for e in exp]), np.stack([e[1] for e in exp])
    assert both(exp_d) and (exp_h.sum(axis=1) > 0).all()
    for hist_stride in (0, 256, 300):      # cumulative; one per frame; one per frame with 44 sentinel words between them
        out = place(np.full((n, h, w), S16, np.int16), layout, "out", fill=S16, s16=True)
        assert src.step != out.step or layout in ("tight", "offset")
        assert layout != "frames" or src.fs != out.fs
        hist = Buf(np.zeros((n if hist_stride else 1, 1, 256), np.int32), step=1024, fs=max(hist_stride, 256) * 4, base=64, fill=S32)
        want = exp_h if hist_stride else exp_h.sum(axis=0, keepdims=True)
        for calls in (1, 2):               # the histogram is added to, the image overwritten
            ok(lib().cart_plane_derivative_hist(eng._h, n, src.ptr, src.step, src.fs, out.ptr, out.step, out.fs, hist.ptr, hist_stride, None))
            assert np.array_equal(hist.image()[:, 0], calls * want), (hist_stride, calls)
            assert np.array_equal(out.image(), exp_d), (hist_stride, calls)
    assert src.untouched()
    if layout == "tight":
        wh = _torch().zeros(256, dtype=_torch().int32, device="cuda")
        assert np.array_equal(eng.plane_derivative_hist(dev(d), wh).cpu().numpy(), exp_d) and np.array_equal(wh.cpu().numpy(), exp_h.sum(axis=0))


# ---- cart_plane_classify, cart_plane_classify_dev --------------------------------------------------------------------------
@pytest.mark.parametrize("layout", BATCHED)
@pytest.mark.parametrize("w,h", SIZES)
def test_plane_classify_host_and_device_parameters(w, h, layout):
    from cartslam._lib import PlaneParams
    torch = _torch()
    eng, n = engine(w, h), frames_of(layout)
    rng = np.random.default_rng(3 * w + h)
    deriv = rng.integers(-40, 41, (n, h, w)).astype(np.int16)
    deriv[rng.random(deriv.shape) < 0.15] = INV
    src = place(deriv, layout, "in", fill=10, s16=True)       # 10: HORIZONTAL under PARAMS[0]
    host_params = (PlaneParams * n)(*[PlaneParams(*p) for p in PARAMS[:n]])
    dev_params = torch.tensor(PARAMS[:n], dtype=torch.int32).cuda()
    for entry, per_frame in (("host", 0), ("host", 1), ("dev", 0), ("dev", 1)):
        out = place(np.full((n, h, w), S8, np.uint8), layout, "out", fill=S8)
        assert src.step != out.step and (layout != "frames" or src.fs != out.fs)
        if entry == "host":
            ok(lib().cart_plane_classify(eng._h, n, src.ptr, src.step, src.fs, host_params, per_frame, out.ptr, out.step, out.fs, None))
        else:
            ok(lib().cart_plane_classify_dev(eng._h, n, src.ptr, src.step, src.fs, dev_params.data_ptr(), per_frame, out.ptr, out.step, out.fs, None))
        exp = np.stack([O.classify(deriv[f], PARAMS[f if per_frame else 0]) for f in range(n)])
        assert all((exp[0] == label).any() for label in (0, 1, 2))
        assert per_frame == 0 or (exp[1] != O.classify(deriv[1], PARAMS[0])).any()     # the second parameter set matters
        assert np.array_equal(out.image(), exp), (entry, per_frame)
        if layout == "tight":
            if entry == "host":
                got = eng.plane_classify(dev(deriv), PARAMS[:n] if per_frame else PARAMS[0])
            else:
                got = eng.plane_classify_dev(dev(deriv), dev_params if per_frame else dev_params[0].contiguous())
            assert np.array_equal(got.cpu().numpy(), exp)
    assert src.untouched()


# ---- cart_plane_ccl, cart_plane_ccl_stats, cart_plane_ccl_table ------------------------------------------------------------
def ccl_maps(w, h):
    """The maps of test_ccl_tile_borders: noise, blocks of scale 3 and 9, the U across the first vertical tile border, the frame."""
    rng = np.random.default_rng(4242 + w)
    maps = [rng.integers(0, 3, (h, w)).astype(np.uint8)]
    for scale in (3, 9):
        maps.append(np.kron(rng.integers(0, 3, (h // scale + 1, w // scale + 1)), np.ones((scale, scale), int))[:h, :w].astype(np.uint8))
    u = np.full((h, w), 2, np.uint8)
    if w > 70 and h > 8:
        u[2, 40:70] = 0; u[6, 40:70] = 0; u[2:7, 69] = 0
        u[10:12, :] = 1
    maps.append(u)
    v = np.full((h, w), 2, np.uint8)
    if h > 40 and w > 8:
        v[20:40, 3] = 1; v[20:40, 7] = 1; v[39, 3:8] = 1
    v[0, :] = 0; v[-1, :] = 0; v[:, 0] = 0; v[:, -1] = 0
    maps.append(v)
    return maps


@pytest.mark.parametrize("layout", BATCHED)
@pytest.mark.parametrize("w,h", SIZES)
def test_ccl_ids_counts_and_tables(w, h, layout):
    eng, maps, cap = engine(w, h), ccl_maps(w, h), w * h + 1
    oracle = []
    for m in maps:
        ids, count = O.ccl(m)
        table, count2 = O.ccl_stats(m, ids)
        assert count == count2 == len(table)
        oracle.append((ids, count, table))
    assert oracle[0][1] > 4 and set(oracle[0][2][:, 1]) == {0, 1} and both(oracle[0][0], -1)     # noise: many components of both labels, unknown pixels
    assert oracle[1][1] >= 1 and oracle[4][1] >= 1
    for group in ((0, 1, 2), (2, 3, 4)):
        n = len(group)
        planes = place(np.stack([maps[f] for f in group]), layout, "in", fill=1)       # label 1 in the slack would join components
        exp_ids = np.stack([oracle[f][0] for f in group])
        exp_n = np.array([oracle[f][1] for f in group], np.int32)

        def outputs():
            return (place(np.full((n, h, w), S32, np.int32), layout, "out", fill=S32, align=4), flat(np.full(n * cap * 7, S32, np.int32), S32),
                    flat(np.full(n, S32, np.int32), S32))

        def same_tables(table):
            rows = table.image().reshape(n, cap, 7)
            for k, f in enumerate(group):
                assert np.array_equal(rows[k, :oracle[f][1]], oracle[f][2]), (group, k)

        ids, table, count = outputs()
        assert planes.step != ids.step and (layout != "frames" or planes.fs != ids.fs)
        ok(lib().cart_plane_ccl(eng._h, n, planes.ptr, planes.step, planes.fs, ids.ptr, ids.step, ids.fs, count.ptr, None))
        assert np.array_equal(ids.image(), exp_ids) and np.array_equal(count.image().ravel(), exp_n), group
        count = flat(np.full(n, S32, np.int32), S32)
        ok(lib().cart_plane_ccl_stats(eng._h, n, planes.ptr, planes.step, planes.fs, ids.ptr, ids.step, ids.fs, table.ptr, cap, count.ptr, None))   # reads the pitched ids
        assert eng.debug_ccl_scratch_nonzero() == 0
        same_tables(table)
        assert np.array_equal(count.image().ravel(), exp_n) and np.array_equal(ids.image(), exp_ids)
        ids, table, count = outputs()
        ok(lib().cart_plane_ccl_table(eng._h, n, planes.ptr, planes.step, planes.fs, ids.ptr, ids.step, ids.fs, table.ptr, cap, count.ptr, None))
        assert eng.debug_ccl_scratch_nonzero() == 0
        same_tables(table)
        assert np.array_equal(ids.image(), exp_ids) and np.array_equal(count.image().ravel(), exp_n), group
        assert planes.untouched()
        if layout == "tight":
            t = dev(np.stack([maps[f] for f in group]))
            wi, wn = eng.plane_ccl(t)
            wt, wn2 = eng.plane_ccl_stats(t, wi, max_components=cap)
            wi3, wt3, wn3 = eng.plane_ccl_table(t, max_components=cap)
            assert np.array_equal(wi.cpu().numpy(), exp_ids) and np.array_equal(wi3.cpu().numpy(), exp_ids)
            assert all(np.array_equal(c.cpu().numpy(), exp_n) for c in (wn, wn2, wn3))
            for k, f in enumerate(group):
                assert all(np.array_equal(x[k, :oracle[f][1]].cpu().numpy(), oracle[f][2]) for x in (wt, wt3))


# ---- cart_plane_temporal_vote ----------------------------------------------------------------------------------------------
def vote_inputs(seed, w, h, n_prev, labels=(0, 1, 2, 2, 2)):
    """Label images and S10.5 flows: flows of up to three pixels either way, the image's outermost rows and columns pointing two pixels
    out of it, and a block where every image says UNKNOWN and nothing moves."""
    rng = np.random.default_rng(seed)
    images = [rng.choice(np.array(labels, np.uint8), (h, w)) for _ in range(n_prev + 1)]
    flows = []
    for _ in range(n_prev):
        f = rng.integers(-96, 97, (h, w, 2)).astype(np.int16)
        f[0, :, 1] = 64; f[-1, :, 1] = -64; f[:, 0, 0] = 64; f[:, -1, 0] = -64
        f[2:6, 4:12] = 0
        flows.append(f)
    for a in images:
        a[2:6, 4:12] = 2
    return images[0], images[1:], flows


def vote_call(eng, layout, planes, prev, flows, h, w):
    """cart_plane_temporal_vote with every image in a Buf of its own (every table entry at its own step) -> the smoothed image's Buf."""
    n_prev = len(prev)
    cur = place(planes[None], layout, "in", fill=1)
    pb = [place(p[None], layout, "in", fill=1, k=k + 1) for k, p in enumerate(prev)]
    fb = [place(f[None], layout, "in", fill=32, align=4, k=k) for k, f in enumerate(flows)]      # 32: one whole pixel
    out = place(np.full((1, h, w), S8, np.uint8), layout, "out", fill=S8)
    if layout not in ("tight", "offset"):
        assert len({b.step for b in pb + [cur]}) == n_prev + 1 and len({b.step for b in fb}) == n_prev and out.step != cur.step
    m = max(n_prev, 1)
    P, PS = (C.c_void_p * m)(*[b.ptr for b in pb]), (C.c_size_t * m)(*[b.step for b in pb])
    F, FS = (C.c_void_p * m)(*[b.ptr for b in fb]), (C.c_size_t * m)(*[b.step for b in fb])
    ok(lib().cart_plane_temporal_vote(eng._h, cur.ptr, cur.step, n_prev, P, PS, F, FS, out.ptr, out.step, None))
    assert all(b.untouched() for b in [cur] + pb + fb)
    return out


@pytest.mark.parametrize("layout", SINGLE)
@pytest.mark.parametrize("w,h", SIZES)
def test_temporal_vote(w, h, layout):
    eng = engine(w, h)
    for n_prev in (0, 1, MAX_TEMPORAL):
        planes, prev, flows = vote_inputs(5 * w + n_prev, w, h, n_prev)
        exp = O.temporal_vote(planes, prev, flows)
        assert all((exp == label).any() for label in (0, 1, 2)), n_prev
        if n_prev:
            f = flows[0].astype(np.int64) >> 5
            y, x = np.indices((h, w))
            px, py = x - f[..., 0], y - f[..., 1]
            assert (px < 0).any() and (px >= w).any() and (py < 0).any() and (py >= h).any() and (f < 0).any()     # out on all four sides, negative flows
            assert ((px >= 0) & (px < w) & (py >= 0) & (py < h) & ((px != x) | (py != y))).any()                   # and moved inside the image
        out = vote_call(eng, layout, planes, prev, flows, h, w)
        assert np.array_equal(out.image()[0], exp), n_prev
        if layout == "tight":
            got = eng.plane_temporal_vote(dev(planes), [dev(p) for p in prev], [dev(f) for f in flows])
            assert np.array_equal(got.cpu().numpy(), exp)


def test_temporal_vote_label_bytes_above_two():
    """A label byte above CART_PLANE_UNKNOWN counts as UNKNOWN (it used to index past the three-element vote array, in the kernel and in
    the oracle alike): the result equals the one for the same images with those bytes set to 2."""
    w, h = 130, 33
    planes, prev, flows = vote_inputs(77, w, h, MAX_TEMPORAL, labels=(0, 1, 2, 2, 3, 255))
    assert all((a == 3).any() and (a == 255).any() for a in [planes] + prev)
    exp = O.temporal_vote(planes, prev, flows)
    assert np.array_equal(exp, O.temporal_vote(np.minimum(planes, 2), [np.minimum(p, 2) for p in prev], flows))
    assert all((exp == label).any() for label in (0, 1, 2))
    for layout in ("tight", "steps"):
        assert np.array_equal(vote_call(engine(w, h), layout, planes, prev, flows, h, w).image()[0], exp)


# ---- cart_reproject_depth --------------------------------------------------------------------------------------------------
def q_matrices():
    """KITTI's Q, a dense random one (every entry takes part: no row or operand can be swapped unnoticed) and KITTI's with Q[15] chosen so
    that W = Q[15] + Q[14] * d is exactly zero at d = 10 (the raw disparity 160): Q[15] = -fl(Q[14] * 10), the very product the kernel forms."""
    dense = np.random.default_rng(16).uniform(-2, 2, 16).astype(np.float32).reshape(4, 4)
    wzero = KITTI_Q.copy()
    wzero[3, 3] = -(wzero[3, 2] * np.float32(10))
    return [("kitti", KITTI_Q), ("dense", dense), ("wzero", wzero)]


def ulps(a, b):
    """Largest distance in units in the last place between two float32 arrays, over the entries that are finite in both."""
    def ordered(x):
        i = np.ascontiguousarray(x).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    fin = np.isfinite(a) & np.isfinite(b)
    return int(np.abs(ordered(a) - ordered(b))[fin].max()) if fin.any() else 0


@pytest.mark.parametrize("layout", BATCHED)
@pytest.mark.parametrize("w,h", SIZES)
def test_reproject_depth_exactly(w, h, layout):
    """The kernel and the oracle do the same IEEE single-precision operations in the same order with contraction off (a correctly rounded
    division included): every finite value equal bit for bit, infinities and NaN in the same places."""
    eng, n = engine(w, h), frames_of(layout)
    rng = np.random.default_rng(7 * w + h)
    d = rng.integers(-200, 1200, (n, h, w)).astype(np.int16)
    d[rng.random(d.shape) < 0.1] = INV
    for value in (0, 1, 32767, -1, 160):
        d.reshape(-1)[rng.choice(d.size, 5, replace=False)] = value
    d[:, 1, 2] = 160; d[:, h - 1, w - 1] = 160; d[0, 0, 0] = 0; d[0, 0, 1] = 1; d[0, 0, 2] = 32767; d[0, 0, 3] = INV; d[0, 0, 4] = -16
    src = place(d, layout, "in", fill=100, s16=True)
    for name, Q in q_matrices():
        out = place(np.full((n, h, w, 3), SF, np.float32), layout, "out", fill=SF, align=4)
        assert src.step != out.step and (layout != "frames" or src.fs != out.fs)
        q = (C.c_float * 16)(*[float(v) for v in Q.reshape(16)])
        ok(lib().cart_reproject_depth(eng._h, n, src.ptr, src.step, src.fs, q, out.ptr, out.step, out.fs, None))
        exp = np.stack([O.reproject_depth(d[f], Q) for f in range(n)])
        finite = np.isfinite(exp)
        assert finite.sum() > exp.size // 2 and len(np.unique(exp[finite])) > exp.size // 8
        if name == "wzero":
            zero = d == 160
            assert zero.sum() >= 2 * n and (~finite[zero]).all() and finite[~zero].all()       # W == 0 exactly there, and nowhere else
        got = out.image()
        print(f"reproject {w}x{h} {layout} {name}: max difference {ulps(got, exp)} ulp, {int((~finite).sum())} non-finite values")
        assert np.array_equal(got.view(np.uint32)[finite], exp.view(np.uint32)[finite]), (name, ulps(got, exp))
        assert np.array_equal(got, exp, equal_nan=True), name
        if layout == "tight":
            assert np.array_equal(eng.reproject_depth(dev(d), Q).cpu().numpy(), exp, equal_nan=True)
    assert src.untouched()


# ---- cart_optical_flow -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", SINGLE)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("w,h", [(67, 9), (130, 33)])
def test_optical_flow(w, h, channels, layout):
    """Pitched gray / BGR input and a pitched flow image; at 67 x 9 with R = 16 the search window is taller than the image."""
    eng = engine(w, h)
    rng = np.random.default_rng(w + channels)
    cur = rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 3)).astype(np.uint8)
    prev = np.roll(cur, (1, -2), axis=(0, 1))
    noisy = rng.random(prev.shape) < 0.05
    prev[noisy] = rng.integers(0, 256, int(noisy.sum()))
    gc, gp = (cur, prev) if channels == 1 else (O.bgr2gray(cur), O.bgr2gray(prev))
    cb = place(cur[None], layout, "in", fill=255)
    pb = place(prev[None], layout, "in", fill=255, k=1)
    for radius, block in ((1, 1), (16, 3), (6, 2)):
        out = place(np.full((1, h, w, 2), S16, np.int16), layout, "out", fill=S16, align=4)
        assert layout in ("tight", "offset") or len({cb.step, pb.step, out.step}) == 3
        ok(lib().cart_optical_flow(eng._h, cb.ptr, cb.step, pb.ptr, pb.step, channels, radius, block, out.ptr, out.step, None))
        exp = O.block_flow(gc, gp, radius, block)
        assert (exp != 0).any()
        assert np.array_equal(out.image()[0], exp), (radius, block)
        if layout == "tight":
            assert np.array_equal(eng.optical_flow(dev(cur), dev(prev), radius, block).cpu().numpy(), exp)
    assert cb.untouched() and pb.untouched()


# ---- cart_resize_linear ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", SINGLE)
@pytest.mark.parametrize("sw,sh,dw,dh,channels", [(97, 61, 200, 130, 3), (130, 33, 67, 9, 1)])
def test_resize_linear_into_a_pitched_destination(sw, sh, dw, dh, channels, layout):
    from cartslam.engine import resize_linear
    _torch().zeros(1, device="cuda")
    rng = np.random.default_rng(sw + dw)
    img = rng.integers(0, 256, (sh, sw) if channels == 1 else (sh, sw, 3)).astype(np.uint8)
    src = place(img[None], layout, "in", fill=255)
    out = place(np.full((1, dh, dw) if channels == 1 else (1, dh, dw, 3), S8, np.uint8), layout, "out", fill=S8)
    assert layout in ("tight", "offset") or (src.step > sw * channels and out.step > dw * channels)
    ok(lib().cart_resize_linear(0, src.ptr, src.step, sw, sh, channels, out.ptr, out.step, dw, dh, None))
    exp = O.resize_linear(img, dw, dh)
    assert len(np.unique(exp)) > 50
    assert np.array_equal(out.image()[0], exp)
    assert src.untouched()
    if layout == "tight":
        assert np.array_equal(resize_linear(dev(img), dw, dh).cpu().numpy(), exp)


# ---- refused calls ---------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing():
    """A base that is not on 4 bytes where a kernel writes or reads 4-byte words, and a frame count that is not positive: refused with a
    message that names the argument, before anything is written; the same calls with good arguments work afterwards."""
    w, h, n = 67, 9, 2
    eng, L = engine(w, h), lib()
    rng = np.random.default_rng(9)
    d = disparities(9, n, h, w)
    labels = rng.integers(0, 3, (n, h, w)).astype(np.uint8)
    flow = rng.integers(-96, 97, (1, h, w, 2)).astype(np.int16)
    cap = w * h + 1
    src = place(d, "tight", "in", fill=100, s16=True)
    inplace = place(d, "steps", "in", fill=65, s16=True)
    deriv = place(np.full((n, h, w, 2), S16, np.int16), "steps", "out", fill=S16, align=4)
    hist = flat(np.full(n * 512, S32, np.int32), S32)
    planes = place(labels, "steps", "in", fill=1)
    ids = place(np.full((n, h, w), S32, np.int32), "steps", "out", fill=S32, align=4)
    table, count = flat(np.full(n * cap * 7, S32, np.int32), S32), flat(np.full(n, S32, np.int32), S32)
    xyz = place(np.full((n, h, w, 3), SF, np.float32), "steps", "out", fill=SF, align=4)
    fb = place(flow, "steps", "in", fill=32, align=4)
    smoothed = place(np.full((1, h, w), S8, np.uint8), "steps", "out", fill=S8)
    q = (C.c_float * 16)(*[float(v) for v in KITTI_Q.reshape(16)])

    def vote(flow_ptr):
        P, PS = (C.c_void_p * 1)(planes.ptr + planes.fs), (C.c_size_t * 1)(planes.step)
        F, FS = (C.c_void_p * 1)(flow_ptr), (C.c_size_t * 1)(fb.step)
        return L.cart_plane_temporal_vote(eng._h, planes.ptr, planes.step, 1, P, PS, F, FS, smoothed.ptr, smoothed.step, None)

    def ccl(n_frames, ids_ptr):
        return L.cart_plane_ccl(eng._h, n_frames, planes.ptr, planes.step, planes.fs, ids_ptr, ids.step, ids.fs, count.ptr, None)

    def ccl_stats(n_frames, ids_ptr):
        return L.cart_plane_ccl_stats(eng._h, n_frames, planes.ptr, planes.step, planes.fs, ids_ptr, ids.step, ids.fs, table.ptr, cap, count.ptr, None)

    def ccl_table(n_frames, ids_ptr):
        return L.cart_plane_ccl_table(eng._h, n_frames, planes.ptr, planes.step, planes.fs, ids_ptr, ids.step, ids.fs, table.ptr, cap, count.ptr, None)

    def derivative(out_ptr):
        return L.cart_disparity_derivative(eng._h, n, src.ptr, src.step, src.fs, out_ptr, deriv.step, deriv.fs, hist.ptr, None)

    def reproject(xyz_ptr):
        return L.cart_reproject_depth(eng._h, n, src.ptr, src.step, src.fs, q, xyz_ptr, xyz.step, xyz.fs, None)

    def interpolate(n_frames):
        return L.cart_interpolate(eng._h, n_frames, inplace.ptr, inplace.step, inplace.fs, 2, 1, 64, 4096, None)

    for off in (1, 2, 3):
        refused(derivative(deriv.ptr + off), "out must be 4-byte aligned")
        refused(vote(fb.ptr + off), "flow")
        refused(reproject(xyz.ptr + off), "xyz must be 4-byte aligned")
        for call in (ccl, ccl_stats, ccl_table):
            refused(call(n, ids.ptr + off), "ids must be 4-byte aligned")
    for bad in (0, -1):
        refused(interpolate(bad), "n_frames")
        for call in (ccl, ccl_stats, ccl_table):
            refused(call(bad, ids.ptr), "n_frames")
    _torch().cuda.synchronize()
    for b in (inplace, deriv, hist, ids, table, count, xyz, smoothed):
        assert b.untouched()
    assert eng.debug_ccl_scratch_nonzero() == 0
    # the same calls with good arguments
    ok(derivative(deriv.ptr))
    assert np.array_equal(deriv.image(), np.stack([O.directional_derivative(d[f])[0] for f in range(n)]))
    ok(vote(fb.ptr))
    assert np.array_equal(smoothed.image()[0], O.temporal_vote(labels[0], [labels[1]], [flow[0]]))
    ok(reproject(xyz.ptr))
    assert np.array_equal(xyz.image(), np.stack([O.reproject_depth(d[f], KITTI_Q) for f in range(n)]), equal_nan=True)
    ok(interpolate(n))
    assert np.array_equal(inplace.image(), np.stack([O.interpolate(d[f], 2, 1, 64, 4096) for f in range(n)]))
    exp_ids = np.stack([O.ccl(labels[f])[0] for f in range(n)])
    ok(ccl(n, ids.ptr))
    assert np.array_equal(ids.image(), exp_ids)
    ok(ccl_stats(n, ids.ptr))
    ok(ccl_table(n, ids.ptr))
    rows = table.image().reshape(n, cap, 7)
    for f in range(n):
        et, en = O.ccl_stats(labels[f], exp_ids[f])
        assert en > 1 and np.array_equal(rows[f, :en], et) and count.image().ravel()[f] == en
    assert np.array_equal(ids.image(), exp_ids) and eng.debug_ccl_scratch_nonzero() == 0

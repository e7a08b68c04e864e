"""GPU tests (-m gpu) of the superpixel stage at the edges of its kernels (csrc/superpixel_kernels.hip, csrc/engine_superpixels.hip): the
64-slot label table at 63 / 64 / 65 labels and under one hash class, tiles on either side of that bound next to each other, every candidate
count, labels that vanish, exact ties, images around one tile, buffer layouts, the state behind set_labels / reset, label ranges of the plane
classification, and every refusal.

All calls go through ctypes on the C ABI, on one flat device allocation per image (Buf): row step and base offset are the test's own, the
slack of an input holds values that would change the result if a kernel read them, the slack of an output holds a sentinel that must be
intact afterwards.  Expected values come from the CPU oracle (spec S13/S14) and are compared byte for byte.  tests/sp_cases.py builds the
cases; tests/test_sp_cases.py proves on the CPU that each of them is what it says and moves labels where it must."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import sp_cases as K

pytestmark = pytest.mark.gpu

S8, S16 = 0xA5, 0x5A5B      # output sentinels: no plane class, no label (labels are < 16384)
# (extra bytes per row, byte offset of the base, fill of the slack) of the pitched layouts.  image: an odd offset; derivative and flow: rows
# and base on 4 bytes; labels: on 2 bytes.  The fills: a white image pixel, a derivative far from every label's mean (relax) or one that is
# HORIZONTAL (classify), label 0 (a label of most cases), a previous plane class, a flow that stays inside the image
PITCHED = dict(image=(13, 7, 255), deriv=(12, 4, 12345), cderiv=(12, 4, 12), labels=(6, 2, 0), out=(10, 6, S16), prev=(3, 1, 1), flow=(8, 12, 32),
               uns=(5, 3, S8), planes=(7, 1, S8))
LABEL_MESSAGE = "label image holds a label >= max_label_id"


def _torch():
    import torch
    return torch


def lib():
    from cartslam import _lib
    return _lib.load()


def err():
    return lib().cart_last_error(None).decode()


def plane_params(params):
    from cartslam import _lib
    return C.byref(_lib.PlaneParams(*params))


def ok(rc):
    assert rc == 0, err()


_ENGINES = {}


def engine(w, h):
    from cartslam import Engine
    if (w, h) not in _ENGINES:
        _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's
        _ENGINES[(w, h)] = Engine(w, h, num_disparities=0, paths=0, max_inflight=4)
    return _ENGINES[(w, h)]


def stream_ptr(stream=None):
    return C.c_void_p((stream if stream is not None else _torch().cuda.current_stream()).cuda_stream)


class Buf:
    """The host image a = [h, w(, c)] in ONE flat device allocation: row y starts base + y * step bytes into it.  Row tails, the bytes
    before the base and `tail` bytes behind the last row are slack and hold `fill` (element-aligned with the rows)."""

    def __init__(self, a, extra=0, base=0, fill=0, k=0, tail=64):
        a = np.ascontiguousarray(a)
        h = a.shape[0]
        rows = a.reshape(h, -1).view(np.uint8)
        row = rows.shape[1]
        step, base = row + extra * (k + 1), base * (k + 1)          # k: a further step and offset per image of a table
        total = base + h * step + tail
        pattern = np.array([fill], a.dtype).view(np.uint8)
        host = pattern[(np.arange(total) - base) % a.itemsize].copy()
        self.index = base + np.arange(h)[:, None] * step + np.arange(row)[None, :]
        host[self.index] = rows
        self.slack = np.ones(total, bool)
        self.slack[self.index] = False
        self.host, self.shape, self.dtype, self.step = host, a.shape, a.dtype, step
        self.dev = _torch().from_numpy(host).cuda()
        assert self.dev.data_ptr() % 256 == 0                       # misalignment comes from `base` alone
        self.ptr = self.dev.data_ptr() + base

    def image(self):
        """The image part as it is now, after the check that NO slack byte changed."""
        now = self.dev.cpu().numpy()
        assert np.array_equal(now[self.slack], self.host[self.slack]), f"{int((now != self.host)[self.slack].sum())} slack bytes were written"
        return now[self.index].view(self.dtype).reshape(self.shape)

    def untouched(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host)


def place(a, kind, pitched, k=0):
    extra, base, fill = PITCHED[kind]
    return Buf(a, extra, base, fill, k) if pitched else Buf(a, fill=fill)


def sentinel(shape, dtype, kind, pitched):
    return place(np.full(shape, PITCHED[kind][2], dtype), kind, pitched)


def ycc(image):
    return O.bgr2ycrcb(image if image.ndim == 3 else np.repeat(image[..., None], 3, axis=2))   # gray is replicated into BGR (datasource.cpp:11-13)


class Sp:
    """cart_superpixels through the C ABI as it is: every pointer and step is the caller's."""

    def __init__(self, eng, params, bw, bh):
        from cartslam import _lib
        p = O.sp_params(**params)
        self.params = _lib.SuperpixelParams(*[getattr(p, n) for n, _ in O.SpParams._fields_])
        self.h = C.c_void_p()
        ok(lib().cart_superpixels_create(eng._h, C.byref(self.params), bw, bh, C.byref(self.h)))

    def close(self):
        lib().cart_superpixels_destroy(self.h)
        self.h = None

    @property
    def max_label(self):
        return lib().cart_superpixels_max_label(self.h)

    def set_labels(self, src, max_label_id, stream=None):
        return lib().cart_superpixels_set_labels(self.h, src.ptr, src.step, max_label_id, stream_ptr(stream))

    def reset(self):
        return lib().cart_superpixels_reset(self.h, stream_ptr())

    def relax(self, img, d2, iters, out, stream=None):
        return lib().cart_superpixels_relax(self.h, img.ptr, img.step, 3 if len(img.shape) == 3 else 1, d2.ptr if d2 else None, d2.step if d2 else 0,
                                            iters, out.ptr if out else None, out.step if out else 0, stream_ptr(stream))

    def labels(self, img, d2, iters, pitched=False):
        """relax on buffers of the given layout -> the label image, after the check of the output's slack."""
        out = sentinel(img.shape[:2], np.uint16, "out", pitched)
        ok(self.relax(place(img, "image", pitched), place(d2, "deriv", pitched) if d2 is not None else None, iters, out))
        return out.image()


# ---- 1. every relax case as a chain ------------------------------------------------------------------------------------------
_EXPECTED = {}


def expected(name):
    """The oracle's labels after the chain's steps, computed once per case: sweeps on the case's scene, one sweep on a second scene."""
    if name not in _EXPECTED:
        c = K.RELAX_CASES[name]()
        p = O.sp_params(**c.params)
        use_d2 = p.disparity_weight > 0
        img2, d2b = K.second_scene(c)
        first, n1 = O.sp_relax(p, c.labels, c.max_label_id, ycc(c.image), c.deriv2 if use_d2 else None, c.sweeps)
        second, _ = O.sp_relax(p, first, c.max_label_id, ycc(img2), d2b if use_d2 else None, 1)
        assert n1 > 0
        _EXPECTED[name] = (first, second)
    return _EXPECTED[name]


@pytest.mark.parametrize("pitched", [False, True], ids=["tight", "pitched"])
@pytest.mark.parametrize("name", sorted(K.RELAX_CASES))
def test_relax_chain(name, pitched):
    """set_labels -> relax(sweeps) -> relax(1) on a second scene -> relax(0), each step against the oracle; tight, and with image,
    derivative, set_labels source and labels_out all pitched and offset."""
    from cartslam import Engine, EngineError
    c = K.RELAX_CASES[name]()
    if not K.fits_engine(c.w, c.h):      # below the engine's smallest image the case ends at the oracle (tests/test_sp_cases.py)
        with pytest.raises(EngineError, match="unsupported image size"):
            Engine(c.w, c.h, num_disparities=0, paths=0)
        return
    first, second = expected(name)
    block = c.premise.get("block")
    sp = Sp(engine(c.w, c.h), c.params, *(block or (8, 8)))
    try:
        if block:
            lab, mx = O.sp_block_init(c.w, c.h, *block)
            assert sp.max_label == mx == c.max_label_id and (lab == c.labels).all()
        else:
            src = place(c.labels, "labels", pitched)
            ok(sp.set_labels(src, c.max_label_id))
            assert sp.max_label == c.max_label_id and src.untouched()
        use_d2 = sp.params.disparity_weight > 0 or pitched      # without the disparity feature the derivative may be NULL, or anything
        img2, d2b = K.second_scene(c)
        for step, (img, d2, iters, want) in enumerate(((c.image, c.deriv2, c.sweeps, first), (img2, d2b, 1, second), (img2, d2b, 0, second))):
            got = sp.labels(img, d2 if use_d2 else None, iters, pitched)
            assert got.tobytes() == want.tobytes(), (step, int((got != want).sum()))
    finally:
        sp.close()


# ---- 2. state -----------------------------------------------------------------------------------------------------------------
def test_state_behind_set_labels_reset_and_null_output():
    c = K.table_mixed()
    w, h = c.w, c.h
    p = O.sp_params()
    sp = Sp(engine(w, h), {}, 8, 8)
    state, mx = O.sp_block_init(w, h, 8, 8)
    count = [0]

    def scene():
        count[0] += 1
        return K.scene(900 + count[0], w, h)

    def step(iters):
        nonlocal state
        img, d2 = scene()
        got = sp.labels(img, d2, iters)
        state, n = O.sp_relax(p, state, mx, ycc(img), d2, iters)
        assert n > 0 or iters == 0
        assert got.tobytes() == state.tobytes(), (count[0], iters, int((got != state).sum()))

    bad = c.labels.copy()
    bad[-1, -1] = c.max_label_id                                     # one label that is not < max_label_id, in the last pixel
    assert mx != c.max_label_id

    def refused_set_labels():
        assert sp.set_labels(Buf(bad), c.max_label_id) != 0 and err() == LABEL_MESSAGE
        assert sp.max_label == mx                                    # the spare buffer was overwritten; the state and its label count were not
        step(0)
        step(2)
    try:
        assert sp.max_label == mx
        step(1)
        refused_set_labels()                                         # after an odd number of sweeps
        step(1)
        refused_set_labels()                                         # after an even number
        other = K.wobbling_stripes(np.random.default_rng(5), w, h, [3, 40, 41, 7, 49, 12])
        ok(sp.set_labels(Buf(c.labels), c.max_label_id))             # two accepted in a row: the second one is the state
        ok(sp.set_labels(Buf(other), 50))
        state, mx = other, 50
        assert sp.max_label == 50
        step(0)
        step(2)
        ok(sp.reset())                                               # back to the blocks and their count
        state, mx = O.sp_block_init(w, h, 8, 8)
        assert sp.max_label == mx
        step(0)
        step(1)
        img, d2 = scene()                                            # labels_out = NULL: the sweeps run, the next call shows them
        ok(sp.relax(Buf(img), Buf(d2), 2, None))
        state, n = O.sp_relax(p, state, mx, ycc(img), d2, 2)
        assert n > 0
        step(0)
    finally:
        sp.close()


# ---- 3. classify: layouts and label ranges --------------------------------------------------------------------------------------
class Classify:
    """The buffers of one cart_superpixel_plane_classify call; previous-plane and flow frames each with a step and an offset of their own."""

    def __init__(self, c, pitched):
        self.c = c
        self.deriv, self.labels = place(c.deriv2, "cderiv", pitched), place(c.labels, "labels", pitched)
        self.prev = [place(a, "prev", pitched, k) for k, a in enumerate(c.prev)]
        self.flows = [place(a, "flow", pitched, k) for k, a in enumerate(c.flows)]
        self.uns, self.planes = sentinel((c.h, c.w), np.uint8, "uns", pitched), sentinel((c.h, c.w), np.uint8, "planes", pitched)

    def tables(self):
        n = len(self.prev)
        if n == 0:
            return None, None, None, None
        return ((C.c_void_p * n)(*[b.ptr for b in self.prev]), (C.c_size_t * n)(*[b.step for b in self.prev]),
                (C.c_void_p * n)(*[b.ptr for b in self.flows]), (C.c_size_t * n)(*[b.step for b in self.flows]))

    def call(self, eng, stream=None, **kw):
        a = dict(eng=eng._h, deriv=self.deriv.ptr, deriv_step=self.deriv.step, labels=self.labels.ptr, labels_step=self.labels.step,
                 max_label=self.c.max_label, params=plane_params(self.c.params), n_prev=len(self.prev), uns=self.uns.ptr,
                 uns_step=self.uns.step, planes=self.planes.ptr, planes_step=self.planes.step)
        a["prev"], a["prev_steps"], a["flows"], a["flow_steps"] = self.tables()
        a.update(kw)
        return lib().cart_superpixel_plane_classify(a["eng"], a["deriv"], a["deriv_step"], a["labels"], a["labels_step"], a["max_label"], a["params"],
                                                    a["n_prev"], a["prev"], a["prev_steps"], a["flows"], a["flow_steps"], a["uns"], a["uns_step"],
                                                    a["planes"], a["planes_step"], stream_ptr(stream))

    def check(self):
        c = self.c
        wu, wp = O.sp_classify(c.deriv2, c.labels, c.max_label, c.params, c.prev, c.flows)
        assert len(np.unique(wp)) >= 2 and (c.labels >= c.max_label).any()
        gu, gp = self.uns.image(), self.planes.image()
        assert gu.tobytes() == wu.tobytes() and gp.tobytes() == wp.tobytes(), (int((gu != wu).sum()), int((gp != wp).sum()))
        assert all(b.untouched() for b in [self.deriv, self.labels] + self.prev + self.flows)


@pytest.mark.parametrize("pitched", [False, True], ids=["tight", "pitched"])
@pytest.mark.parametrize("w,kind,n_prev", K.CLASSIFY)
def test_classify_layouts_and_label_ranges(w, kind, n_prev, pitched):
    from cartslam import Engine, EngineError
    c = K.classify_case(w, kind, n_prev)
    if not K.fits_engine(c.w, c.h):
        with pytest.raises(EngineError, match="unsupported image size"):
            Engine(c.w, c.h, num_disparities=0, paths=0)
        return
    call = Classify(c, pitched)
    ok(call.call(engine(c.w, c.h)))
    call.check()


def test_classify_back_to_back_on_two_streams():
    """Three calls on two streams without host synchronisation in between: each takes a vote table of its own (the slot lease)."""
    torch = _torch()
    cases = [K.classify_case(50, "full", 0), K.classify_case(50, "low", 2), K.classify_case(50, "full", 2)]
    eng = engine(50, 9)
    calls = [Classify(c, k == 1) for k, c in enumerate(cases)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for k, call in enumerate(calls):
        ok(call.call(eng, streams[k % 2]))
    torch.cuda.synchronize()
    for call in calls:
        call.check()


# ---- 4. refusals write nothing ---------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    torch = _torch()
    L = lib()
    c = K.classify_case(50, "low", 2)
    w, h = c.w, c.h
    eng = engine(w, h)
    img, d2 = K.scene(77, w, h)
    block, mx = O.sp_block_init(w, h, 5, 3)
    CHUNK = 4096
    items = dict(image=img, deriv=d2, block=block, cderiv=c.deriv2, clabels=c.labels, prev0=c.prev[0], prev1=c.prev[1], flow0=c.flows[0],
                 flow1=c.flows[1], out=np.full((h, w), S16, np.uint16), uns=np.full((h, w), S8, np.uint8), planes=np.full((h, w), S8, np.uint8))
    host = np.full(len(items) * CHUNK, S8, np.uint8)                 # one arena: inputs, outputs and sentinel bytes between them
    at = {}
    for k, (name, a) in enumerate(items.items()):
        raw = np.ascontiguousarray(a).view(np.uint8).ravel()
        assert len(raw) < CHUNK
        host[k * CHUNK:k * CHUNK + len(raw)] = raw
        at[name] = k * CHUNK
    arena = torch.from_numpy(host).cuda()
    ptr = {name: arena.data_ptr() + off for name, off in at.items()}

    def read(name, dtype):
        n = w * h * np.dtype(dtype).itemsize
        return arena[at[name]:at[name] + n].cpu().numpy().view(dtype).reshape(h, w)

    sp = Sp(eng, {}, 5, 3)
    assert sp.max_label == mx
    good_r = dict(sp=sp.h, image=ptr["image"], image_step=3 * w, channels=3, deriv=ptr["deriv"], deriv_step=4 * w, iters=1, out=ptr["out"], out_step=2 * w)

    def relax(**kw):
        a = dict(good_r, **kw)
        return L.cart_superpixels_relax(a["sp"], a["image"], a["image_step"], a["channels"], a["deriv"], a["deriv_step"], a["iters"], a["out"],
                                        a["out_step"], None)
    good_s = dict(sp=sp.h, labels=ptr["block"], step=2 * w, mx=mx)

    def set_labels(**kw):
        a = dict(good_s, **kw)
        return L.cart_superpixels_set_labels(a["sp"], a["labels"], a["step"], a["mx"], None)
    tables = dict(prev=(C.c_void_p * 2)(ptr["prev0"], ptr["prev1"]), prev_steps=(C.c_size_t * 2)(w, w),
                  flows=(C.c_void_p * 2)(ptr["flow0"], ptr["flow1"]), flow_steps=(C.c_size_t * 2)(4 * w, 4 * w))
    good_c = dict(eng=eng._h, deriv=ptr["cderiv"], deriv_step=4 * w, labels=ptr["clabels"], labels_step=2 * w, max_label=c.max_label,
                  params=plane_params(c.params), n_prev=2, uns=ptr["uns"], uns_step=w, planes=ptr["planes"], planes_step=w, **tables)

    def classify(**kw):
        a = dict(good_c, **kw)
        return L.cart_superpixel_plane_classify(a["eng"], a["deriv"], a["deriv_step"], a["labels"], a["labels_step"], a["max_label"], a["params"],
                                                a["n_prev"], a["prev"], a["prev_steps"], a["flows"], a["flow_steps"], a["uns"], a["uns_step"],
                                                a["planes"], a["planes_step"], None)

    def refused(fn, message, **kw):
        rc = fn(**kw)
        assert rc != 0 and err() == message, (fn.__name__, kw, rc, err())

    try:
        # create (the parameter refusals are in test_gpu_superpixels.py)
        made = C.c_void_p()
        for args in ((None, C.byref(sp.params), 5, 3, C.byref(made)), (eng._h, None, 5, 3, C.byref(made)), (eng._h, C.byref(sp.params), 5, 3, None)):
            assert L.cart_superpixels_create(*args) != 0 and err() == "bad arguments"
        assert not made.value
        assert L.cart_superpixels_max_label(None) == -1
        assert L.cart_superpixels_reset(None, None) != 0 and err() == "superpixels is NULL"
        # relax
        refused(relax, "superpixels is NULL", sp=None)
        refused(relax, "NULL pointer", image=None)
        for ch in (0, 2, 4):
            refused(relax, "channels must be 1 or 3", channels=ch)
        refused(relax, "iterations must be >= 0", iters=-1)
        refused(relax, "bad step", image_step=3 * w - 1)
        refused(relax, "bad step", channels=1, image_step=w - 1)
        refused(relax, "the disparity feature needs the 2-channel disparity derivative image", deriv=None)
        refused(relax, "bad step", deriv_step=4 * w - 4)
        refused(relax, "bad step", deriv_step=4 * w + 2)
        refused(relax, "bad step", deriv=ptr["deriv"] + 2)           # a derivative pixel is read as one 32-bit word
        refused(relax, "bad step", out_step=2 * w - 2)
        refused(relax, "bad step", out_step=2 * w + 1)
        # set_labels
        refused(set_labels, "bad arguments", sp=None)
        refused(set_labels, "bad arguments", labels=None)
        for bad in (-1, 0, K.MAX_LABELS):
            refused(set_labels, "max_label_id must be in [1, 16384)", mx=bad)
        refused(set_labels, "bad step", step=2 * w - 2)
        refused(set_labels, "bad step", step=2 * w + 1)
        refused(set_labels, LABEL_MESSAGE, mx=int(block.max()))
        refused(set_labels, LABEL_MESSAGE, labels=ptr["clabels"], mx=K.MAX_LABELS - 1)   # 0xFFFF
        assert sp.max_label == mx
        # classify
        refused(classify, "engine is NULL", eng=None)
        for name in ("deriv", "labels", "params", "uns", "planes"):
            refused(classify, "NULL pointer", **{name: None})
        for bad in (-1, 0, K.MAX_LABELS + 1):
            refused(classify, "max_label must be in [1, 16384]", max_label=bad)
        for bad in (-1, 9):
            refused(classify, "n_prev must be in [0, CART_MAX_TEMPORAL]", n_prev=bad)
        for name in ("prev", "prev_steps", "flows", "flow_steps"):
            refused(classify, "NULL table", **{name: None})
        refused(classify, "NULL entry in the temporal tables", prev=(C.c_void_p * 2)(ptr["prev0"], None))
        refused(classify, "NULL entry in the temporal tables", flows=(C.c_void_p * 2)(None, ptr["flow1"]))
        for name, step in (("deriv_step", 4 * w - 4), ("deriv_step", 4 * w + 2), ("labels_step", 2 * w - 2), ("labels_step", 2 * w + 1),
                           ("uns_step", w - 1), ("planes_step", w - 1)):
            refused(classify, "bad step", **{name: step})
        refused(classify, "bad step in the temporal tables", prev_steps=(C.c_size_t * 2)(w, w - 1))
        refused(classify, "bad step in the temporal tables", flow_steps=(C.c_size_t * 2)(4 * w - 4, 4 * w))
        refused(classify, "bad step in the temporal tables", flow_steps=(C.c_size_t * 2)(4 * w, 4 * w + 2))
        torch.cuda.synchronize()
        assert np.array_equal(arena.cpu().numpy(), host), "a refused call wrote to an input, an output or the bytes between them"
        # the state is the block labelling still, and valid calls work
        ok(relax(iters=0))
        assert read("out", np.uint16).tobytes() == block.tobytes()
        ok(classify())
        wu, wp = O.sp_classify(c.deriv2, c.labels, c.max_label, c.params, c.prev, c.flows)
        assert read("uns", np.uint8).tobytes() == wu.tobytes() and read("planes", np.uint8).tobytes() == wp.tobytes()
        ok(relax(iters=2))
        want, n = O.sp_relax(O.sp_params(), block, mx, ycc(img), d2, 2)
        assert n > 0 and read("out", np.uint16).tobytes() == want.tobytes()
    finally:
        sp.close()

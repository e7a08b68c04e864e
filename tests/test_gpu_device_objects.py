"""The lifecycle the stateful device objects share (cart_superpixels, cart_planefit, cart_orb): two calls on one object that
arrive on different streams, with no host synchronisation in between, equal the same calls on one stream (the object's event
orders them); an object may be closed after its engine; create / use / close cycles do not leak device memory."""
import ctypes as C

import numpy as np
import pytest

from cartslam import OrbFeatures, PlaneFit, Superpixels

pytestmark = pytest.mark.gpu
W, H = 320, 96


def _torch():
    import torch
    return torch


def _engine():
    from cartslam import Engine
    _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's (see __graft_entry__.build)
    return Engine(W, H, num_disparities=0, paths=0)


def _inputs():
    from cartslam import synth
    from test_gpu_planefit import block_labels, scene
    torch = _torch()
    bgr = [torch.from_numpy(np.ascontiguousarray(synth.make_pair(W, H, 64, 4, seed=s, channels=3)[0])).cuda() for s in (3, 4)]
    gray = [torch.from_numpy(np.ascontiguousarray(synth.make_pair(W, H, 64, 4, seed=s)[0])).cuda() for s in (5, 6)]
    lab, mx = block_labels(W, H, 8)
    return dict(bgr=bgr, gray=gray, labels=torch.from_numpy(lab.view(np.int16)).cuda(), max_label=mx,
                xyz=torch.from_numpy(scene(W, H, 6)).cuda())


def _orb_detect(orb, img):
    """cart_orb_detect of one gray image on the current stream, without the host synchronisation OrbFeatures.detect ends with."""
    torch = _torch()
    kp = torch.zeros((orb.nfeatures, 7), dtype=torch.float32, device="cuda")
    de = torch.zeros((orb.nfeatures, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = lambda t: (C.c_void_p * 1)(t.data_ptr())   # noqa: E731
    orb._check(orb._lib.cart_orb_detect(orb._h, 1, one(img), (C.c_size_t * 1)(img.stride(0)), 1, W, H, one(kp), one(de), None,
                                        C.c_void_p(n.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "cart_orb_detect")
    return [n, kp, de]


# kind -> (create on an engine, first call, second call); a call returns device tensors and reads the state the first one left
KINDS = {
    "superpixels": (lambda e: Superpixels(e, block_size=8, disparity_weight=0.0),
                    lambda o, x: [o.relax(x["bgr"][0], None, 3)], lambda o, x: [o.relax(x["bgr"][1], None, 3)]),
    "planefit": (PlaneFit,
                 lambda o, x: list(o.label_planes(x["labels"], x["xyz"], x["max_label"], seed=2, frame_id=1)),
                 lambda o, x: list(o.fit(x["labels"], seed=2, frame_id=1)[:2])),
    "orb": (lambda e: OrbFeatures(e, W, H, nfeatures=500),
            lambda o, x: _orb_detect(o, x["gray"][0]), lambda o, x: _orb_detect(o, x["gray"][1])),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_streams_and_lifecycle(kind):
    torch = _torch()
    make, first, second = KINDS[kind]
    x = _inputs()
    eng = _engine()

    def run(streams):
        obj = make(eng)
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[0]):
            out = first(obj, x)
        with torch.cuda.stream(streams[1]):
            out += second(obj, x)
        torch.cuda.synchronize()
        obj.close()
        return [t.cpu().numpy() for t in out]

    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    same, two = run((a, a)), run((a, b))
    for k, (s, t) in enumerate(zip(same, two)):
        assert s.shape == t.shape and s.tobytes() == t.tobytes(), f"{kind}: output {k} differs across streams"
    # closed after its engine
    other = _engine()
    obj = make(other)
    first(obj, x)
    other.close()
    obj.close()
    # no leak over create / use / close cycles (measured like test_gpu_superpixels' lifecycle test)
    def cycle(n):
        for _ in range(n):
            o = make(eng)
            first(o, x)
            o.close()
        torch.cuda.synchronize()
    cycle(3)
    free0 = torch.cuda.mem_get_info()[0]
    cycle(20)
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 8 << 20, f"{kind} leak: {(free0 - free1) >> 20} MiB over 20 create/use/close cycles"
    eng.close()

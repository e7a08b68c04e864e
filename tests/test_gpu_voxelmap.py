"""GPU tests of the rolling TSDF voxel map (spec S33): cart_voxel_map_integrate / _raycast / _read against the numpy
restatement tests/np_voxelmap.py, byte for byte on pitched buffers that start at a byte offset, and the voxel_map host module in the C++
frame loop.  Beside every byte comparison stands a numeric premise on the restatement (voxels updated with f < 1, ray statuses that must
occur), so that no comparison passes on an empty case."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import np_voxelmap as V
import test_voxelmap_spec as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (63, 3), (65, 3), (130, 70)]   # width x height
VOLUMES = [(16, 16, 16), (24, 16, 40), (64, 16, 16)]
SENTINEL = 77
# the 2 m cubes of the small volumes: the depth range and the look-ahead are cut to them (the look-ahead puts the camera at the window's near face)
SMALL = dict(max_depth=3.0, lookahead=1.0, min_depth=0.25)


def _torch():
    import torch
    return torch


_STATE = {}


def engine():
    from cartslam import Engine
    if "engine" not in _STATE:
        _torch().zeros(1, device="cuda")   # torch's HIP runtime first, then the library's (see __graft_entry__.build)
        _STATE["engine"] = Engine(64, 32, num_disparities=0, paths=0)
    return _STATE["engine"]


def cam_for(w, h):
    """The wider side spans about 50 degrees: a 2 m wide volume is filled at 1.5 m whatever the image's shape; fx baseline = 32 keeps a
    surface at 1.5 m at 21 pixels of disparity whatever the focal length."""
    f = float(max(w, h))
    return V.camera(fx=f, fy=f, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, baseline=32.0 / f)


def cam_tuple(cam):
    return tuple(cam[k] for k in ("fx", "fy", "cx", "cy", "baseline"))


def frame_for(seed, w, h, cam, depth=1.5, masked=True):
    return S.small_frame(seed, w, h, cam, depth=depth, holes=0.1 if w * h >= 64 else 0.0, masked=masked)


def pitched(a, extra, fill, offset):
    """A device tensor of the image `a` whose rows are `extra` pixels longer than the image and whose first pixel lies `offset` pixels
    into its allocation, the slack holding `fill`."""
    torch = _torch()
    h, w = a.shape
    flat = np.full(offset + h * (w + extra), fill, a.dtype)
    rows = flat[offset:].reshape(h, w + extra)
    rows[:, :w] = a
    return torch.from_numpy(flat).cuda()[offset:].view(h, w + extra)[:, :w]


def ptr_step(t):
    if isinstance(t, tuple):
        return t
    return (C.c_void_p(t.data_ptr()), t.stride(0) * t.element_size()) if t is not None else (None, 0)


def _common(cam, pose, stream):
    from cartslam import _lib
    torch = _torch()
    host_pose = (C.c_double * 12)(*[float(v) for v in pose]) if pose is not None else None
    sp = C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)
    return _lib.load(), C.byref(_lib.EgoCamera(*cam_tuple(cam))), host_pose, sp


def counts_ptr(c):
    return C.c_void_p(c.data_ptr()) if isinstance(c, _torch().Tensor) else c


def integrate_call(obj, cam, pose, disp, mask=None, counts=None, size=None, stream=None):
    """cart_voxel_map_integrate on device tensors (or (pointer, step) pairs) as they are -> (rc, message)."""
    lib, c, P, sp = _common(cam, pose, stream)
    w, h = size if size is not None else (int(disp.shape[1]), int(disp.shape[0]))
    rc = lib.cart_voxel_map_integrate(obj._h if obj is not None else None, c, P, *ptr_step(disp), w, h, *ptr_step(mask), counts_ptr(counts), sp)
    return rc, lib.cart_last_error(None).decode()


def raycast_call(obj, cam, pose, size, disp, weight=None, status=None, counts=None, stream=None):
    lib, c, P, sp = _common(cam, pose, stream)
    rc = lib.cart_voxel_map_raycast(obj._h if obj is not None else None, c, P, size[0], size[1], *ptr_step(disp), *ptr_step(weight), *ptr_step(status),
                                    counts_ptr(counts), sp)
    return rc, lib.cart_last_error(None).decode()


def integrate(obj, cam, pose, disp, mask=None, counts=True, stream=None):
    """One integrate on pitched, offset inputs whose slack would pass every gate -> the counts tensor (inside sentinel words) or None."""
    torch = _torch()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d = pitched(disp, 3, 256, 1)
        m = pitched(mask, 5, 0, 3) if mask is not None else None
        n = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")[1:3] if counts else None
    rc, err = integrate_call(obj, cam, pose, d, m, n, stream=stream)
    assert rc == 0, err
    return n


def raycast(obj, cam, pose, w, h, weight=True, status=True, counts=True, stream=None):
    torch = _torch()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        outs = dict(disp=pitched(np.full((h, w), SENTINEL, np.int16), 3, SENTINEL, 1),
                    weight=pitched(np.full((h, w), SENTINEL, np.uint16), 2, SENTINEL, 3).view(torch.int16) if weight else None,
                    status=pitched(np.full((h, w), SENTINEL, np.uint8), 6, SENTINEL, 5) if status else None,
                    counts=torch.full((5,), SENTINEL, dtype=torch.int32, device="cuda")[1:4] if counts else None)
    rc, err = raycast_call(obj, cam, pose, (w, h), stream=stream, **outs)
    assert rc == 0, err
    return outs


def same_ray(outs, ref):
    torch = _torch()
    torch.cuda.synchronize()
    for name in ("disp", "weight", "status", "counts"):
        t = outs[name]
        if t is None:
            continue
        got = t.cpu().numpy()
        if name == "weight":
            got = got.view(np.uint16)
        assert got.dtype == ref[name].dtype and got.shape == ref[name].shape, name
        assert got.tobytes() == ref[name].tobytes(), f"{name}: {int((got != ref[name]).sum())} values differ"
        base = t._base if t._base is not None else t                 # the slack of the pitched output and the words around counts: untouched
        whole = base.cpu().numpy().reshape(-1)
        assert int((whole != SENTINEL).sum()) <= int((got != SENTINEL).sum()), f"{name}: bytes outside the image were written"


def same_counts(n, ref):
    _torch().cuda.synchronize()
    assert n.cpu().numpy().tobytes() == ref.tobytes(), (n.cpu().numpy(), ref)
    assert (n._base.cpu().numpy()[[0, 3]] == SENTINEL).all()


def same_volume(obj, ref):
    vox, origin = obj.read()
    rv, ro = ref.read()
    assert tuple(origin) == tuple(ro), (origin, ro)
    assert vox.dtype == rv.dtype and vox.shape == rv.shape
    assert vox.tobytes() == rv.tobytes(), f"{int((vox != rv).sum())} voxels differ"
    assert obj.window() == (tuple(ro), (ref.nx, ref.ny, ref.nz), ref.origin is not None)


def run_chain(shape, p, cam, frames, ray=None, ray_cam=None, premise=True):
    """frames = [(pose, disp, mask)] or [(pose, disp, mask, camera)] for a frame with a camera of its own.  The device object and the
    restatement integrate every frame; the volume, the counts and a raycast from the frame's pose at the frame's size are compared after
    each.  -> [(integrate counts, ray result)] of the restatement."""
    from cartslam import VoxelMap, voxel_map_params
    ref = V.Map(*shape, V.params(**p))
    out = []
    with VoxelMap(engine(), *shape, voxel_map_params(**p)) as obj:
        for frame in frames:
            pose, disp, mask = frame[:3]
            fcam = frame[3] if len(frame) > 3 else cam
            n = integrate(obj, fcam, pose, disp, mask)
            rn = ref.integrate(fcam, pose, disp, mask)
            same_counts(n, rn)
            same_volume(obj, ref)
            w, h = ray if ray is not None else (disp.shape[1], disp.shape[0])
            rr = ref.raycast(ray_cam or fcam, pose, w, h)
            same_ray(raycast(obj, ray_cam or fcam, pose, w, h), rr)
            if premise:
                assert rn[0] > 0 and 0 < rn[1], rn                   # voxels were updated, some of them inside the truncation band
            out.append((rn, rr))
    return out


@pytest.mark.parametrize("w,h", SHAPES)
def test_image_shapes_on_pitched_offset_buffers(w, h):
    """A frustum one or three pixels thin holds no sample with all eight corners known, so two frames of 130 x 70 come first: the frame of the
    shape under test is integrated into their volume and raycast from it.  The poses lie half a voxel off the lattice on x and y, so that a
    column of voxel centres lies on the optical axis and an image one pixel wide still sees voxels."""
    cam, wide = cam_for(w, h), cam_for(130, 70)
    frames = [(S.pose_t(0.0625, 0.0625, 0.0), *frame_for(900 + k, 130, 70, wide, masked=False), wide) for k in range(2)]
    frames.append((S.pose_t(0.0625, 0.0625, 0.0625), *frame_for(10 * w + h, w, h, cam, masked=w * h >= 64)))
    res = run_chain((16, 16, 16), SMALL, cam, frames)
    rays = res[-1][1]["counts"]
    assert rays.sum() == w * h and rays[V.HIT] > 0, rays


@pytest.mark.parametrize("shape", VOLUMES)
def test_volumes_and_all_three_ray_statuses(shape):
    w, h = 63, 24
    cam = cam_for(w, h)
    frames = [(S.pose_t(), *frame_for(7 + k + shape[0], w, h, cam)) for k in range(2)]
    res = run_chain(shape, dict(SMALL, lookahead=0.125 * shape[2] / 2), cam, frames)
    assert (res[-1][1]["counts"] > 0).all(), res[-1][1]["counts"]     # NONE, HIT and INSIDE


WINDOW_CASES = {
    # name: (poses, look-ahead, wall depth, what the origins must do)
    "forward": ([S.pose_t(tz=0.5 * k) for k in range(4)], 1.0, 1.5, lambda o: [v[2] for v in o] == [0, 0, 8, 8]),
    "lateral_and_vertical": ([S.pose_t(), S.pose_t(tx=1.0), S.pose_t(tx=1.0, ty=-1.0), S.pose_t(tx=-1.0, ty=-1.0)], 1.0, 1.5,
                             lambda o: o[1][0] == o[0][0] + 8 and o[2][1] == o[1][1] - 8 and o[3][0] == o[2][0] - 16),
    "jump": ([S.pose_t(), S.pose_t(tz=0.25), S.pose_t(tz=40.0), S.pose_t(tx=-30.0, ty=9.0, tz=40.25)], 1.0, 1.5,
             lambda o: o[2][2] - o[1][2] >= 16 and o[3][0] - o[2][0] <= -16),
    "camera_outside_its_window": ([S.pose_t(), S.pose_t(tz=0.25)], 6.0, 5.75, lambda o: o[0][2] >= 32),
    "turned_90": ([S.POSE_90, [0.0, 0.0, 1.0, 0.25, 0.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0]], 1.0, 1.5, lambda o: o[0] == (0, -8, -8) and o[1] == (0, -8, -8)),
    "turned_180": ([S.POSE_180, S.yaw_pose(173.0, (0.0, 0.0, -0.125))], 1.0, 1.5, lambda o: o[0] == (-8, -8, -16)),
}


@pytest.mark.parametrize("name", sorted(WINDOW_CASES))
def test_window_cases(name):
    poses, lookahead, depth, origins_ok = WINDOW_CASES[name]
    w, h = 40, 24
    cam = cam_for(w, h)
    p = dict(SMALL, lookahead=lookahead, max_depth=max(3.0, depth + 1.0))
    frames = [(pose, *frame_for(3 * len(name) + k, w, h, cam, depth=depth, masked=k % 2 == 0)) for k, pose in enumerate(poses)]
    ref = V.Map(16, 16, 16, V.params(**p))
    origins = []
    for pose, disp, mask in frames:
        ref.integrate(cam, pose, disp, mask)
        origins.append(ref.origin)
    assert origins_ok(origins), origins
    res = run_chain((16, 16, 16), p, cam, frames)
    assert sum(int(r[1]["counts"][V.HIT]) for r in res) > 0


def test_workgroups_culled_against_the_frustum_change_no_byte():
    """A volume of two workgroups along x and many along y and z, most of them outside the frustum or the depth range (the integrate kernel
    skips a workgroup whose 64 x 4 x 4 box of voxels cannot pass the gates): poses that put the frustum across box borders in every direction."""
    w, h = 63, 24
    cam = cam_for(w, h)
    shape = (128, 16, 64)                                                     # 16 x 2 x 8 m
    p = dict(SMALL, lookahead=4.0, max_depth=4.0)
    poses = [S.pose_t(), S.yaw_pose(35.0, (0.3, 0.0, 0.2)), S.yaw_pose(-62.0, (-0.4, 0.1, 0.5)), [0.0, 0.0, 1.0, -3.0, 0.0, 1.0, 0.0, 0.0, -1.0, 0.0, 0.0, 4.0],
             S.yaw_pose(171.0, (0.2, 0.0, 6.5))]
    frames = [(pose, *frame_for(60 + k, w, h, cam, depth=2.5, masked=False)) for k, pose in enumerate(poses)]
    touched, empty = 0, 0
    for pose, disp, mask in frames:                                           # on an empty volume a frame's updated voxels are those of weight 1
        fresh = V.Map(*shape, V.params(**p))
        assert fresh.integrate(cam, pose, disp, mask)[0] > 500
        boxes = fresh.read()[0]["weight"].astype(np.int64).reshape(16, 4, 4, 4, 2, 64).sum(axis=(1, 3, 5))
        touched, empty = touched + int((boxes > 0).sum()), empty + int((boxes == 0).sum())
    assert touched > 20 and empty > 2 * touched, (touched, empty)            # most workgroups have nothing to do, some do
    run_chain(shape, p, cam, frames)


@pytest.mark.parametrize("max_weight,frames_n,top", [(1, 3, 1), (2, 4, 2)])
def test_weight_cap(max_weight, frames_n, top):
    w, h = 40, 24
    cam = cam_for(w, h)
    frames = [(S.pose_t(), *frame_for(50 + k, w, h, cam, masked=False)) for k in range(frames_n)]
    p = dict(SMALL, max_weight=max_weight)
    ref = V.Map(16, 16, 16, V.params(**p))
    seen = []
    for pose, disp, mask in frames:
        ref.integrate(cam, pose, disp, mask)
        seen.append(ref.read()[0].copy())
    assert seen[-1]["weight"].max() == top and (seen[-1]["tsdf"] != seen[-2]["tsdf"]).sum() > 10     # capped, and still averaging
    run_chain((16, 16, 16), p, cam, frames)


def test_raycast_cases():
    """min_weight = 2 after one frame: nothing is known; a raycast at another image size and camera than the integrated one; a raycast before
    any integrate and after clear: everything NONE."""
    from cartslam import VoxelMap, voxel_map_params
    w, h = 40, 24
    cam = cam_for(w, h)
    disp, _ = frame_for(4, w, h, cam, masked=False)
    p = dict(SMALL, min_weight=2)
    ref = V.Map(16, 16, 16, V.params(**p))
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**p)) as obj:
        same_volume(obj, ref)                                                 # no window: every voxel empty, origin (0, 0, 0)
        rr = ref.raycast(cam, S.pose_t(), 65, 3)
        assert rr["counts"].tolist() == [195, 0, 0]
        same_ray(raycast(obj, cam, S.pose_t(), 65, 3), rr)
        same_counts(integrate(obj, cam, S.pose_t(), disp), ref.integrate(cam, S.pose_t(), disp))
        rr = ref.raycast(cam, S.pose_t(), w, h)
        assert rr["counts"].tolist() == [w * h, 0, 0] and ref.read()[0]["weight"].max() == 1
        same_ray(raycast(obj, cam, S.pose_t(), w, h), rr)
        same_counts(integrate(obj, cam, S.pose_t(), disp), ref.integrate(cam, S.pose_t(), disp))
        other = cam_for(65, 9)
        for size, c, pose in (((w, h), cam, S.pose_t()), ((65, 9), other, S.pose_t()), ((130, 70), cam_for(130, 70), S.yaw_pose(9.0, (0.1, 0.0, 0.05)))):
            rr = ref.raycast(c, pose, *size)
            assert rr["counts"][V.HIT] > 0
            same_ray(raycast(obj, c, pose, *size), rr)
        same_volume(obj, ref)                                                 # a raycast moves and changes nothing
        obj.clear()
        ref.clear()
        same_volume(obj, ref)
        rr = ref.raycast(cam, S.pose_t(), w, h)
        assert rr["counts"].tolist() == [w * h, 0, 0]
        same_ray(raycast(obj, cam, S.pose_t(), w, h), rr)
        same_counts(integrate(obj, cam, S.pose_t(tz=0.5), disp), ref.integrate(cam, S.pose_t(tz=0.5), disp))
        same_volume(obj, ref)
        assert ref.read()[0]["weight"].max() == 1                             # the clear forgot the two earlier frames


def test_optional_outputs_and_the_python_class():
    from cartslam import VOXEL_DTYPE, EngineError, VoxelMap, voxel_map_params
    torch = _torch()
    w, h = 63, 24
    cam = cam_for(w, h)
    disp, mask = frame_for(8, w, h, cam)
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    rn = ref.integrate(cam, S.pose_t(), disp, mask)
    rr = ref.raycast(cam, S.pose_t(), w, h)
    assert rn[1] > 0 and rr["counts"][V.HIT] > 0
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as obj:
        assert integrate(obj, cam, S.pose_t(), disp, mask, counts=False) is None
        same_volume(obj, ref)
        same_ray(raycast(obj, cam, S.pose_t(), w, h, weight=False, status=False, counts=False), rr)
        same_ray(raycast(obj, cam, S.pose_t(), w, h, weight=True, status=False, counts=True), rr)
    with VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL)) as obj:    # host arrays in, host arrays out
        assert obj.window() == ((0, 0, 0), (16, 16, 16), False)
        n = obj.integrate(cam_tuple(cam), S.pose_t(), disp, mask)
        assert n.dtype == np.int32 and n.tobytes() == rn.tobytes()
        dm, wm, st, cnt = obj.raycast(cam_tuple(cam), S.pose_t(), w, h)
        assert dm.tobytes() == rr["disp"].tobytes() and wm.dtype == np.uint16 and wm.tobytes() == rr["weight"].tobytes()
        assert st.tobytes() == rr["status"].tobytes() and cnt.tobytes() == rr["counts"].tobytes()
        dm, wm, st, cnt = obj.raycast(cam_tuple(cam), S.pose_t(), w, h, weight=False, status=False, counts=False)
        assert dm.tobytes() == rr["disp"].tobytes() and wm is None and st is None and cnt is None
        vox, origin = obj.read()
        assert vox.dtype == VOXEL_DTYPE and vox.tobytes() == ref.read()[0].tobytes() and origin == ref.origin
        raw = obj.integrate(cam_tuple(cam), S.pose_t(), torch.from_numpy(disp).cuda(), raw=True)
        assert isinstance(raw, torch.Tensor) and raw.is_cuda and raw.cpu().numpy().tobytes() == ref.integrate(cam, S.pose_t(), disp).tobytes()
        with pytest.raises(EngineError, match="pose"):
            obj.integrate(cam_tuple(cam), [float("nan")] * 12, disp)
        with pytest.raises(EngineError, match="mask"):
            obj.integrate(cam_tuple(cam), S.pose_t(), torch.from_numpy(disp).cuda(), mask=torch.from_numpy(mask).cuda()[:, :8], raw=True)
        with pytest.raises(EngineError, match="width"):
            obj.raycast(cam_tuple(cam), S.pose_t(), 0, 4)
        same_volume(obj, ref)                                                 # the refused calls changed nothing
    with pytest.raises(EngineError, match="cells_y"):
        VoxelMap(engine(), 16, 12, 16)
    with pytest.raises(EngineError, match="march_step"):
        VoxelMap(engine(), 16, 16, 16, voxel_map_params(march_step=1.0))


def test_back_to_back_calls_and_a_second_object_on_another_stream():
    from cartslam import VoxelMap, voxel_map_params
    torch = _torch()
    w, h = 63, 24
    cam = cam_for(w, h)
    frames = [(S.pose_t(tz=0.125 * k), *frame_for(20 + k, w, h, cam, masked=False)) for k in range(4)]
    refs = [V.Map(16, 16, 16, V.params(**SMALL)), V.Map(24, 16, 40, V.params(**dict(SMALL, lookahead=2.5)))]
    side = torch.cuda.Stream()
    a = VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL))
    b = VoxelMap(engine(), 24, 16, 40, voxel_map_params(**dict(SMALL, lookahead=2.5)))
    pending = []
    for k, (pose, disp, _) in enumerate(frames):                              # no synchronisation inside the loop; a alternates between the two streams
        sa = side if k % 2 else None
        na, nb = integrate(a, cam, pose, disp, stream=sa), integrate(b, cam, pose, disp, stream=side)
        ra, rb = raycast(a, cam, pose, w, h, stream=sa), raycast(b, cam, pose, w, h, stream=side)
        pending.append((na, nb, ra, rb))
    torch.cuda.synchronize()
    hits = 0
    for (pose, disp, _), (na, nb, ra, rb) in zip(frames, pending):
        for ref, n, r in ((refs[0], na, ra), (refs[1], nb, rb)):
            rn = ref.integrate(cam, pose, disp)
            assert rn[1] > 0
            same_counts(n, rn)
            rr = ref.raycast(cam, pose, w, h)
            hits += int(rr["counts"][V.HIT])
            same_ray(r, rr)
    assert hits > 0
    same_volume(a, refs[0])
    same_volume(b, refs[1])
    a.close()
    b.close()


def test_bad_arguments_touch_no_output():
    torch = _torch()
    from cartslam import Engine, VoxelMap, voxel_map_params
    w, h = 63, 24
    cam = cam_for(w, h)
    arena = torch.zeros(8 * 4096, dtype=torch.uint8, device="cuda")          # one allocation in a known order

    def carve(k, dtype, shape):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return arena[4096 * k:4096 * k + n].view(dtype).view(shape)
    disp, mask = carve(0, torch.int16, (h, w)), carve(1, torch.uint8, (h, w))
    d0, m0 = frame_for(2, w, h, cam)
    disp.copy_(torch.from_numpy(d0))
    mask.copy_(torch.from_numpy(m0))
    n2 = carve(2, torch.int32, (2,))
    dm, wm, st, n3 = carve(3, torch.int16, (h, w)), carve(4, torch.int16, (h, w)), carve(5, torch.uint8, (h, w)), carve(6, torch.int32, (3,))
    outs = (n2, dm, wm, st, n3)
    for t in outs:
        t.fill_(SENTINEL)
    ref = V.Map(16, 16, 16, V.params(**SMALL))
    obj = VoxelMap(engine(), 16, 16, 16, voxel_map_params(**SMALL))
    rc, err = integrate_call(obj, cam, S.pose_t(), disp, mask, None)
    assert rc == 0, err
    ref.integrate(cam, S.pose_t(), d0, m0)
    moved = S.pose_t(tz=2.0)                                                  # a refused integrate must not move the window either

    def refused_i(word, obj_=obj, pose=moved, size=None, **kw):
        args = dict(dict(disp=disp, mask=mask, counts=n2), **kw)
        rc, err = integrate_call(obj_, cam, pose, size=size or (w, h), **args)
        assert rc != 0 and word in err, (kw, err)

    def refused_r(word, obj_=obj, pose=moved, size=None, **kw):
        args = dict(dict(disp=dm, weight=wm, status=st, counts=n3), **kw)
        rc, err = raycast_call(obj_, cam, pose, size or (w, h), **args)
        assert rc != 0 and word in err, (kw, err)

    for refused in (refused_i, refused_r):
        refused("map is NULL", obj_=None)
        refused("width", size=(0, h))
        refused("height", size=(w, 16385))
        refused("pose is NULL", pose=None)
        refused("pose[7]", pose=S.pose_t(ty=2e6))
        refused("counts must be 4-byte aligned", counts=C.c_void_p(n3.data_ptr() + 2))
    refused_i("disp is NULL", disp=None)
    refused_i("disp and its step must be 2-byte aligned", disp=(C.c_void_p(disp.data_ptr() + 1), 2 * w))
    refused_i("disp and its step must be 2-byte aligned", disp=(C.c_void_p(disp.data_ptr()), 2 * w + 1))
    refused_i("disp_step is below the row size", disp=(C.c_void_p(disp.data_ptr()), 2 * w - 2))
    refused_i("mask_step is below the row size", mask=(C.c_void_p(mask.data_ptr()), w - 1))
    refused_i("disp and counts must not overlap", counts=C.c_void_p(disp.data_ptr() + 2 * w * h - 4))
    refused_i("mask and counts must not overlap", counts=C.c_void_p(mask.data_ptr()))
    refused_r("disp_model is NULL", disp=None)
    for k, name, elem in (("disp", "disp_model", 2), ("weight", "weight_model", 2), ("status", "status", 1)):
        t = dict(disp=dm, weight=wm, status=st)[k]
        if elem > 1:
            refused_r(name + " and its step must be 2-byte aligned", **{k: (C.c_void_p(t.data_ptr() + 1), w * elem)})
            refused_r(name + " and its step must be 2-byte aligned", **{k: (C.c_void_p(t.data_ptr()), w * elem + 1)})
        refused_r(name + "_step is below the row size", **{k: (C.c_void_p(t.data_ptr()), w * elem - elem)})
    refused_r("disp_model and weight_model must not overlap", weight=dm)
    refused_r("disp_model and status must not overlap", status=(C.c_void_p(dm.data_ptr() + 2 * w * h - 1), w))
    refused_r("weight_model and status must not overlap", status=(C.c_void_p(wm.data_ptr()), w))
    refused_r("disp_model and counts must not overlap", counts=C.c_void_p(dm.data_ptr() + 4))
    refused_r("weight_model and counts must not overlap", counts=C.c_void_p(wm.data_ptr()))
    refused_r("status and counts must not overlap", counts=C.c_void_p(st.data_ptr() + 4))
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs)                     # no refused call touched an output
    same_volume(obj, ref)                                                     # nor the volume or its window
    rc, err = integrate_call(obj, cam, S.pose_t(), disp, mask, n2)
    assert rc == 0, err
    rc, err = raycast_call(obj, cam, S.pose_t(), (w, h), dm, wm, st, n3)
    assert rc == 0, err
    torch.cuda.synchronize()
    rn = ref.integrate(cam, S.pose_t(), d0, m0)
    rr = ref.raycast(cam, S.pose_t(), w, h)
    assert rn[1] > 0 and rr["counts"][V.HIT] > 0
    assert n2.cpu().numpy().tobytes() == rn.tobytes() and n3.cpu().numpy().tobytes() == rr["counts"].tobytes()
    assert dm.cpu().numpy().tobytes() == rr["disp"].tobytes() and wm.cpu().numpy().view(np.uint16).tobytes() == rr["weight"].tobytes()
    assert st.cpu().numpy().tobytes() == rr["status"].tobytes()
    eng2 = Engine(64, 32, num_disparities=0, paths=0)
    late = VoxelMap(eng2, 16, 16, 16)
    eng2.close()
    late.close()                                                              # destroy is valid after the engine
    obj.close()


# ---- the C++ frame loop ------------------------------------------------------------------------------------------------------------
def read_dump(path, w, h):
    raw = open(path, "rb").read()
    assert len(raw) == 24 + 12 + 8 + 8 + 12 + 8 + 3 * w * h, path
    out = dict(origin=tuple(np.frombuffer(raw, "<i8", 3).tolist()), cells=tuple(np.frombuffer(raw, "<i4", 3, 24).tolist()),
               voxel_size=float(np.frombuffer(raw, "<f8", 1, 36)[0]), counts=np.frombuffer(raw, "<i4", 2, 44), rays=np.frombuffer(raw, "<i4", 3, 52))
    assert np.frombuffer(raw, "<i4", 2, 64).tolist() == [w, h]
    out["disp"] = np.frombuffer(raw, np.int16, w * h, 72).reshape(h, w)
    out["status"] = np.frombuffer(raw, np.uint8, w * h, 72 + 2 * w * h).reshape(h, w)
    return out


def test_voxel_map_module_in_the_frame_loop(tmp_path):
    """cart_slam_amd over four synthetic frames against the chain of restatements np_ego -> np_voxelmap: voxel_map on the disparity and
    the pose of ego_motion, with the voxels dumped through the snapshot switch; then plane_map voting with the model image."""
    import np_ego as E
    import np_planemap as PM
    import oracle_lib as O
    from test_gpu_ego import restated_frames
    from test_gpu_matches import noise_frame, noise_world
    from test_gpu_planemap import check_dump
    from test_host import run_exe, write_pnm
    tmp = str(tmp_path)
    n, w, h = 4, 320, 96
    world = noise_world(79)
    images = [noise_frame(world, f) for f in range(n)]
    seq = os.path.join(tmp, "dataset", "sequences", "00")
    for side in ("image_2", "image_3"):
        os.makedirs(os.path.join(seq, side))
    for f, (l, r) in enumerate(images):
        write_pnm(os.path.join(seq, "image_2", "%06d.pgm" % f), l)
        write_pnm(os.path.join(seq, "image_3", "%06d.pgm" % f), r)
    src = os.path.join(tmp, "source.json")
    json.dump({"type": "kitti", "path": os.path.join(tmp, "dataset"), "sequence": 0}, open(src, "w"))
    static = {"type": "static", "horizontal_range_min": 6, "horizontal_range_max": 18, "vertical_range_min": -5, "vertical_range_max": 6}
    keys = dict(fx=300, fy=300, cx=160, cy=48, baseline=0.5)
    # the scene is a textured plane at 6 px of disparity, 25 m away: half-metre voxels, a window of 32 x 8 x 32 m that starts at the camera
    vp = dict(voxel_size=0.5, min_disparity=3.5, max_depth=40.0, truncation=1.0, march_step=0.5, lookahead=16.0, max_weight=3)
    shape = dict(cells_x=64, cells_y=16, cells_z=64)
    grid = dict(cells_x=64, cells_z=64, cell_size=1.0, max_depth=40.0, max_lateral=30.0)
    head = [{"type": "disparity", "num_disparities": 64, "paths": 8, "smoothing_radius": 2, "smoothing_iterations": 1},
            {"type": "orb_features"}, {"type": "orb_matches"}, dict(keys, type="ego_motion"), {"type": "disparity_planeseg", "parameter_provider": static}]
    ecam, vcam = E.camera(**keys), V.camera(**keys)
    feats, stereo, temporal = restated_frames(images, 5000)
    lms = [E.triangulate(ecam, feats[f][0][0], feats[f][1][0], stereo[f]) for f in range(n)]
    disps, planes, poses, pose = [], [], [], list(E.POSE_IDENTITY)
    for f in range(n):
        l, rr = images[f]
        disps.append(O.disparity_module(l, rr, 64, 8, 4, radius=2, iterations=1))
        planes.append(O.classify(O.plane_derivative(disps[f])[0], (6, 18, -5, 6, 12, 0)))
        res = E.estimate(ecam, E.params(), lms[f], feats[f][0][0], lms[max(f - 1, 0)], temporal[f], 0, f + 1)[0]
        pose = E.chain(pose, res)
        poses.append(list(pose))
    d = os.path.join(tmp, "dump")
    os.makedirs(d)
    r = run_exe(src, head + [dict(keys, type="voxel_map", **shape, **vp), dict(keys, type="plane_map", disparity_key="disparity_model", **grid)], tmp, ("--dump", d),
                env={"CARTSLAM_VOXEL_MAP_SNAPSHOT": "1"})
    assert r.returncode == 0, r.stderr
    ref = V.Map(64, 16, 64, V.params(**vp))
    ref_map = PM.Map(PM.camera(**keys), 64, 64, PM.params(cell_size=1.0, max_depth=40.0, max_lateral=30.0))
    hits = 0
    for f in range(n):
        rn = ref.integrate(vcam, poses[f], disps[f])
        rr = ref.raycast(vcam, poses[f], w, h)
        got = read_dump(os.path.join(d, f"{f + 1}_voxel_map.bin"), w, h)
        assert got["origin"] == ref.origin and got["cells"] == (64, 16, 64) and got["voxel_size"] == 0.5, f"frame {f + 1}: window"
        assert got["counts"].tobytes() == rn.tobytes() and got["rays"].tobytes() == rr["counts"].tobytes(), f"frame {f + 1}: counts"
        assert got["disp"].tobytes() == rr["disp"].tobytes() and got["status"].tobytes() == rr["status"].tobytes(), f"frame {f + 1}: model"
        assert open(os.path.join(d, f"{f + 1}_voxel_map_voxels.bin"), "rb").read() == ref.read()[0].tobytes(), f"frame {f + 1}: voxels"
        assert np.fromfile(os.path.join(d, f"{f + 1}_disparity.bin"), np.int16).tobytes() == disps[f].tobytes()      # the input is what it is without the module
        assert rn[1] > 1000
        hits += int(rr["counts"][V.HIT])
        ref_map.update(rr["disp"], planes[f], poses[f])
        check_dump(os.path.join(d, f"{f + 1}_plane_map.bin"), ref_map, 3, 50)
    assert hits > w * h and int(ref.read()[0]["weight"].max()) == 3          # the model was seen, and voxels were averaged over every frame up to the cap

    # without the raycast and the snapshot: the window and the integrate counts alone
    d = os.path.join(tmp, "dump_b")
    os.makedirs(d)
    r = run_exe(src, head + [dict(keys, type="voxel_map", raycast=False, **shape, **vp)], tmp, ("--dump", d))
    assert r.returncode == 0, r.stderr
    ref = V.Map(64, 16, 64, V.params(**vp))
    for f in range(n):
        rn = ref.integrate(vcam, poses[f], disps[f])
        got = read_dump(os.path.join(d, f"{f + 1}_voxel_map.bin"), 0, 0)
        assert got["origin"] == ref.origin and got["counts"].tobytes() == rn.tobytes() and got["rays"].tolist() == [0, 0, 0]
        assert not os.path.exists(os.path.join(d, f"{f + 1}_voxel_map_voxels.bin"))

    # configuration errors name their key
    for bad, word in ((dict(type="voxel_map"), "fx"), (dict(keys, type="voxel_map", cells_y=12), "cells_y"), (dict(keys, type="voxel_map", voxel_size=0.001), "voxel_size"),
                      (dict(keys, type="voxel_map", march_step=0.5), "march_step"), (dict(keys, type="voxel_map", max_weight=0), "max_weight"),
                      (dict(keys, type="voxel_map", max_depth=0.25), "max_depth"), (dict(keys, type="voxel_map", pose_key=""), "pose_key")):
        r = run_exe(src, head + [bad], tmp)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    r = run_exe(src, head + [dict(keys, type="voxel_map", use_motion=True)], tmp)
    assert r.returncode != 0 and 'requires "motion"' in r.stderr, r.stderr
    r = run_exe(src, head + [dict(keys, type="voxel_map", pose_key="dense_ego")], tmp)
    assert r.returncode != 0 and 'requires "dense_ego"' in r.stderr, r.stderr

"""Thin Python driver over the C ABI (include/cart_engine.h).

torch is used only for device memory and streams; every op below is one C-ABI call on the
current torch stream.  Tensors are [n, h, w(, c)] or [h, w(, c)] CUDA tensors with a contiguous
innermost row; row and frame pitches are taken from the strides (like cv::cuda::GpuMat::step).
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DenseEgoParams, ModelTrackColorParams, ModelTrackParams, EgoCamera, EgoParams, EngineParams, FusionParams, LocalBAParams, MatchParams, MotionParams, ObjectParams, PlaceParams, PlaneMapParams, PlaneParams, PoseGraphParams, SuperpixelParams, VoxelMapParams

INVALID = -32768  # CARTSLAM_DISPARITY_INVALID, reference include/modules/disparity.hpp:17


class EngineError(RuntimeError):
    pass


def _stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _geom(t, inner):
    """-> (n_frames, data_ptr, step_bytes, frame_stride_bytes); `inner` = trailing dims that form a row."""
    if not t.is_cuda:
        raise EngineError("tensor must live on the GPU")
    batched = t.dim() == inner + 2
    if t.dim() not in (inner + 1, inner + 2):
        raise EngineError(f"expected {inner + 1} or {inner + 2} dims, got {t.dim()}")
    row_dims = t.shape[-inner:]
    exp = 1
    for k in range(inner):
        if t.stride(-1 - k) != exp:
            raise EngineError("innermost row must be contiguous")
        exp *= row_dims[-1 - k]
    es = t.element_size()
    step = t.stride(-inner - 1) * es
    n = t.shape[0] if batched else 1
    fs = t.stride(0) * es if batched else 0
    return n, C.c_void_p(t.data_ptr()), step, fs


def _pitched(t, inner):
    """-> [data_ptr, step_bytes] of one image for a C-ABI call, [None, 0] for an absent optional one."""
    return list(_geom(t, inner)[1:3]) if t is not None else [None, 0]


def _default_params(struct_type, c_name, fields):
    """cart_<c_name>_default_params as a `struct_type` with the given fields replaced: what the public *_params functions do."""
    p = struct_type()
    getattr(_lib.load(), f"cart_{c_name}_default_params")(C.byref(p))
    known = dict(struct_type._fields_)
    for k, v in fields.items():
        if k not in known:
            raise ValueError(f"cart_{c_name}_params has no field {k}")
        setattr(p, k, v)
    return p


def _camera(camera):
    """EgoCamera or (fx, fy, cx, cy, baseline) -> EgoCamera."""
    return camera if isinstance(camera, EgoCamera) else EgoCamera(*[float(v) for v in camera])


def _pose12(m):
    """12 numbers, a 3 x 4 pose in row order -> the host array a C-ABI call takes; None stays None."""
    return (C.c_double * 12)(*[float(v) for v in np.asarray(m, np.float64).reshape(-1)]) if m is not None else None


def _to_device(a, dtype, via_host=False):
    """A host array goes up as a tensor of `dtype`; None stays None.  A tensor is taken as it is, or with via_host copied through the host
    like an array (contiguous, converted to `dtype`)."""
    import torch
    if a is None or (isinstance(a, torch.Tensor) and not via_host):
        return a
    return torch.as_tensor(np.ascontiguousarray(a.cpu() if isinstance(a, torch.Tensor) else a), dtype=dtype).cuda()


def _check_frame_image(t, dtype, what, frame, channels=None):
    """t must be a tensor of `dtype` with the [h, w] of the tensor `frame`, and [h, w, channels] when channels is given."""
    import torch
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != (2 if channels is None else 3) or tuple(t.shape[:2]) != tuple(frame.shape[:2])
            or (channels is not None and t.shape[2] != channels)):
        raise EngineError(f"{what} must be a device tensor of {dtype} and of the frame's size")


def flow_pyramid_levels(w, h, levels):
    """-> [(w_l, h_l)] of the levels spec S21 builds for a w x h frame when `levels` are asked for (cart_flow_pyramid_levels; host only)."""
    lib = _lib.load()
    lw, lh = (C.c_int * _lib.FLOW_MAX_LEVELS)(), (C.c_int * _lib.FLOW_MAX_LEVELS)()
    n = lib.cart_flow_pyramid_levels(int(w), int(h), int(levels), lw, lh)
    if n < 1:
        raise EngineError("cart_flow_pyramid_levels: " + lib.cart_last_error(None).decode())
    return [(lw[k], lh[k]) for k in range(n)]


class Engine:
    """One engine = one (width, height, D, paths, ...) configuration on one GPU.
    num_disparities=0, paths=0 gives a geometry-only engine for the post-SGM entry points."""

    def __init__(self, width, height, num_disparities=256, paths=4, min_disparity=4, p1=10, p2=120,
                 uniqueness_ratio=12, smoothing_radius=-1, smoothing_iterations=5, max_inflight=12, device_id=0):
        self._lib = _lib.load()
        p = EngineParams()
        self._lib.cart_engine_default_params(C.byref(p))
        p.device_id, p.width, p.height = device_id, width, height
        p.min_disparity, p.num_disparities, p.paths, p.p1, p.p2 = min_disparity, num_disparities, paths, p1, p2
        p.uniqueness_ratio, p.smoothing_radius, p.smoothing_iterations = uniqueness_ratio, smoothing_radius, smoothing_iterations
        p.max_inflight = max_inflight
        self.params = p
        self._h = C.c_void_p()
        if self._lib.cart_engine_create(C.byref(p), C.byref(self._h)) != 0:
            raise EngineError("cart_engine_create: " + self._lib.cart_last_error(None).decode())
        self.width, self.height, self.D, self.P = width, height, num_disparities, paths

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.cart_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError(f"{what}: " + self._lib.cart_last_error(self._h).decode())

    # ---- launch plan (every plan gives the same bits; include/cart_engine.h CART_PLAN_*) ----
    def set_plan(self, plan, min_frames=1):
        """plan: "auto" | "slabs" | "fused_up" | "band_up"; a forced plan applies to launches of >= min_frames frames."""
        code = {"auto": _lib.PLAN_AUTO, "slabs": _lib.PLAN_SLABS, "fused_up": _lib.PLAN_FUSED_UP, "band_up": _lib.PLAN_BAND_UP}[plan]
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_PLAN, code), "cart_engine_set_option")
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_PLAN_MIN_FRAMES, int(min_frames)), "cart_engine_set_option")

    def set_spec_variants(self, s8_zero_invalid=False, s7_replicate_border=False, s5_top2=False):
        """The three choices that are open upstream (oracle S8 / S7 / S5 NOTEs); default: the oracle's spec."""
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_SPEC_S5_TOP2, 1 if s5_top2 else 0), "cart_engine_set_option")
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_SPEC_S8_ZERO_INVALID, 1 if s8_zero_invalid else 0), "cart_engine_set_option")
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_SPEC_S7_REPLICATE_BORDER, 1 if s7_replicate_border else 0), "cart_engine_set_option")

    def set_band_rows(self, k, probe=False):
        """K of plan "band_up" (4, 8 or 16 rows per band).  probe: measurement only -- the plan then stores and reads all P slabs and
        recomputes nothing (K = 1 allowed), which times the banded tile's read pattern against the two-kernel WTA's."""
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_BAND_ROWS, int(k)), "cart_engine_set_option")
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_BAND_PROBE, 1 if probe else 0), "cart_engine_set_option")

    def set_band_diag(self, on=True):
        """Plan "band_up": the WTA rebuilds the up-right diagonal path inside its tile instead of reading its slab (default on; same bits
        either way).  Ignored with the probe and by engines that never take the plan."""
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_BAND_DIAG, 1 if on else 0), "cart_engine_set_option")

    def get_option(self, option):
        """The engine's current value of one CART_OPT_* option (cart_engine_get_option)."""
        v = C.c_int(0)
        self._check(self._lib.cart_engine_get_option(self._h, int(option), C.byref(v)), "cart_engine_get_option")
        return int(v.value)

    def set_chunk_frames(self, n):
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_CHUNK_FRAMES, int(n)), "cart_engine_set_option")

    def describe_plan(self, n_frames):
        """-> dict(frames_per_launch, plan, slabs_written) of a batched call of n_frames."""
        lp = _lib.LaunchPlan()
        self._check(self._lib.cart_engine_describe_plan(self._h, int(n_frames), C.byref(lp)), "cart_engine_describe_plan")
        return {"frames_per_launch": lp.frames_per_launch, "plan": {0: "slabs", 1: "fused_up", 2: "band_up"}[lp.plan],
                "slabs_written": lp.slabs_written}

    def copy_narrow(self, dst, src, workgroups=0):
        """dst <- src (same byte size, contiguous; dst may be a PINNED host tensor: its memory is mapped into the device's
        address space) by a copy kernel of a few workgroups on the current stream (cart_copy_narrow)."""
        nbytes = src.numel() * src.element_size()
        if dst.numel() * dst.element_size() != nbytes or not dst.is_contiguous() or not src.is_contiguous():
            raise EngineError("copy_narrow needs two contiguous tensors of the same byte size")
        if not (dst.is_cuda or dst.is_pinned()) or not (src.is_cuda or src.is_pinned()):
            raise EngineError("copy_narrow needs device tensors or pinned host tensors")
        self._check(self._lib.cart_copy_narrow(self._h, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes, int(workgroups),
                                               _stream_ptr()), "cart_copy_narrow")
        return dst

    def tune_placement(self, n_frames, max_tries=8, max_extra_bytes=0, report=False):
        """cart_engine_tune_placement (opt-in set-up step): time the slab-bound launches of an n_frames call on up to max_tries physical
        placements of the slot groups behind it and keep the fastest.  max_extra_bytes bounds what the call may hold beyond the
        workspace while it searches (0: two units' worth; None: no cap but 4 GiB left free).  -> (ms before, ms after), or with
        report=True the whole cart_placement_report as a dict (mode: fast / mixed / uniform / unknown, relative to the sets the search saw; candidates timed, why the search
        stopped).  The engine must be idle."""
        r = _lib.PlacementReport()
        cap = C.c_size_t(-1).value if max_extra_bytes is None else int(max_extra_bytes)
        self._check(self._lib.cart_engine_tune_placement(self._h, int(n_frames), int(max_tries), cap, C.byref(r)), "cart_engine_tune_placement")
        if not report:
            return r.ms_first, r.ms_kept
        return {"ms_first": r.ms_first, "ms_kept": r.ms_kept, "ms_fastest_seen": r.ms_fastest_seen, "ms_slowest_seen": r.ms_slowest_seen,
                "seconds": r.seconds, "units": r.units, "candidates": r.candidates, "mode": _lib.PLACE_MODES.get(r.mode, str(r.mode)),
                "stopped_on": _lib.PLACE_STOPS.get(r.stop_reason, str(r.stop_reason))}

    # ---- disparity module (reference src/modules/disparity/disparity.cu:49-80) ----
    def compute_disparity(self, left, right, out=None):
        import torch
        ch = 3 if (left.dim() >= 3 and left.shape[-1] == 3 and left.shape[-2] == self.width
                   and left.shape[-3] == self.height) else 1
        inner = 2 if ch == 3 else 1
        for t in (left, right):
            if tuple(t.shape[-inner - 1:][:2]) != (self.height, self.width):
                raise EngineError(f"image shape {tuple(t.shape)} does not match the engine's {self.height}x{self.width} (bad step/size)")
        n, lp, ls, lfs = _geom(left, inner)
        n2, rp, rs, rfs = _geom(right, inner)
        if n != n2 or left.dtype != torch.uint8 or right.dtype != torch.uint8:
            raise EngineError("left/right must be uint8 tensors of the same batch size")
        shape = (n, self.height, self.width) if left.dim() == inner + 2 else (self.height, self.width)
        if out is None:
            out = torch.empty(shape, dtype=torch.int16, device=left.device)
        _, op, os_, ofs = _geom(out, 1)
        self._check(self._lib.cart_compute_disparity_batch(self._h, n, lp, ls, lfs, rp, rs, rfs, ch, op, os_, ofs,
                                                           _stream_ptr()), "cart_compute_disparity_batch")
        return out

    def compute_disparity_multi(self, lefts, rights, outs=None):
        """Frames in separate allocations (lists of [H,W] or [H,W,3] uint8 tensors with a common row step) in ONE launch
        sequence: what a module adapter uses to coalesce concurrently entered frames."""
        import torch
        n = len(lefts)
        if n == 0 or len(rights) != n:
            raise EngineError("lefts/rights must be non-empty lists of the same length")
        ch = 3 if lefts[0].dim() == 3 else 1
        if outs is None:
            outs = [torch.empty((self.height, self.width), dtype=torch.int16, device=lefts[0].device) for _ in range(n)]
        geo = [[_geom(t, inner) for t in ts] for ts, inner in ((lefts, 2 if ch == 3 else 1), (rights, 2 if ch == 3 else 1), (outs, 1))]
        for ts, g in zip((lefts, rights, outs), geo):
            if any(tuple(t.shape[:2]) != (self.height, self.width) for t in ts) or len({x[2] for x in g}) != 1:
                raise EngineError("every image of one kind must be HxW with the same row step")
        tables = [(C.c_void_p * n)(*[x[1].value for x in g]) for g in geo]
        self._check(self._lib.cart_compute_disparity_multi(self._h, n, tables[0], geo[0][0][2], tables[1], geo[1][0][2], ch,
                                                           tables[2], geo[2][0][2], _stream_ptr()), "cart_compute_disparity_multi")
        return outs

    def interpolate(self, disp, radius, iterations, min_disp16, max_disp):
        n, p, s, fs = _geom(disp, 1)
        self._check(self._lib.cart_interpolate(self._h, n, p, s, fs, radius, iterations, min_disp16, max_disp,
                                               _stream_ptr()), "cart_interpolate")
        return disp

    # ---- derivative module (reference src/modules/disparity/derivative.cu:151-184) ----
    def disparity_derivative(self, disp):
        import torch
        n, p, s, fs = _geom(disp, 1)
        out = torch.empty(tuple(disp.shape) + (2,), dtype=torch.int16, device=disp.device)
        hist = torch.empty((n, 256, 2), dtype=torch.int32, device=disp.device)
        _, op, os_, ofs = _geom(out, 2)
        self._check(self._lib.cart_disparity_derivative(self._h, n, p, s, fs, op, os_, ofs, C.c_void_p(hist.data_ptr()),
                                                        _stream_ptr()), "cart_disparity_derivative")
        return out, (hist if disp.dim() == 3 else hist[0])

    # ---- plane label module (reference src/modules/planeseg/planeseg.cu:246-377) ----
    def plane_derivative_hist(self, disp, hist, per_frame_hist=False):
        """hist: int32 [256] (persistent, added to) or [n,256] when per_frame_hist."""
        import torch
        n, p, s, fs = _geom(disp, 1)
        out = torch.empty_like(disp)
        _, op, os_, ofs = _geom(out, 1)
        if hist.dtype != torch.int32 or not hist.is_contiguous():
            raise EngineError("hist must be a contiguous int32 tensor")
        self._check(self._lib.cart_plane_derivative_hist(self._h, n, p, s, fs, op, os_, ofs, C.c_void_p(hist.data_ptr()),
                                                         256 if per_frame_hist else 0, _stream_ptr()),
                    "cart_plane_derivative_hist")
        return out

    def plane_classify(self, deriv, params):
        """params: one PlaneParams / 6-tuple, or a list with one per frame."""
        import torch
        n, p, s, fs = _geom(deriv, 1)
        per_frame = isinstance(params, (list,)) and len(params) == n and n > 1
        plist = params if isinstance(params, list) else [params]
        arr = (PlaneParams * len(plist))()
        for i, q in enumerate(plist):
            arr[i] = q if isinstance(q, PlaneParams) else PlaneParams(*q)
        planes = torch.empty(deriv.shape, dtype=torch.uint8, device=deriv.device)
        _, pp, ps, pfs = _geom(planes, 1)
        self._check(self._lib.cart_plane_classify(self._h, n, p, s, fs, arr, 1 if per_frame else 0, pp, ps, pfs,
                                                  _stream_ptr()), "cart_plane_classify")
        return planes

    def plane_label_multi(self, disps, hist, params):
        """Frames in separate allocations (a list of [H,W] int16 disparity tensors with a common row step): plane
        derivative + cumulative histogram (`hist`: int32 [256], added to) and classification with `params` (one
        PlaneParams / 6-tuple for all frames, or a list with one per frame), one launch per stage.
        Returns (list of derivative images, list of plane images)."""
        import torch
        n = len(disps)
        if n == 0:
            raise EngineError("disps must be a non-empty list")
        geo = [_geom(t, 1) for t in disps]
        if any(tuple(t.shape) != (self.height, self.width) or t.dtype != torch.int16 for t in disps) or len({g[2] for g in geo}) != 1:
            raise EngineError("every disparity image must be int16 HxW with the same row step")
        if hist.dtype != torch.int32 or not hist.is_contiguous():
            raise EngineError("hist must be a contiguous int32 tensor")
        derivs = [torch.empty((self.height, self.width), dtype=torch.int16, device=disps[0].device) for _ in range(n)]
        planes = [torch.empty((self.height, self.width), dtype=torch.uint8, device=disps[0].device) for _ in range(n)]
        table = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        self._check(self._lib.cart_plane_derivative_hist_multi(self._h, n, table(disps), geo[0][2], table(derivs), self.width * 2,
                                                               C.c_void_p(hist.data_ptr()), 0, _stream_ptr()), "cart_plane_derivative_hist_multi")
        plist = params if isinstance(params, list) else [params]
        arr = (PlaneParams * len(plist))()
        for i, q in enumerate(plist):
            arr[i] = q if isinstance(q, PlaneParams) else PlaneParams(*q)
        self._check(self._lib.cart_plane_classify_multi(self._h, n, table(derivs), self.width * 2, arr, 1 if len(plist) == n and n > 1 else 0,
                                                        table(planes), self.width, _stream_ptr()), "cart_plane_classify_multi")
        return derivs, planes

    def plane_classify_dev(self, deriv, params_dev):
        """params_dev: int32 CUDA tensor [n,6] (one cart_plane_params per frame) or [6] (shared)."""
        import torch
        n, p, s, fs = _geom(deriv, 1)
        if params_dev.dtype != torch.int32 or not params_dev.is_contiguous() or not params_dev.is_cuda:
            raise EngineError("params_dev must be a contiguous int32 CUDA tensor")
        per_frame = params_dev.dim() == 2
        if per_frame and params_dev.shape[0] != n:
            raise EngineError("one parameter row per frame expected")
        planes = torch.empty(deriv.shape, dtype=torch.uint8, device=deriv.device)
        _, pp, ps, pfs = _geom(planes, 1)
        self._check(self._lib.cart_plane_classify_dev(self._h, n, p, s, fs, C.c_void_p(params_dev.data_ptr()), 1 if per_frame else 0,
                                                      pp, ps, pfs, _stream_ptr()), "cart_plane_classify_dev")
        return planes

    def plane_temporal_vote(self, planes, prev_planes, flows):
        """planes: uint8 [h,w]; prev_planes: list of uint8 [h,w]; flows: list of int16 [h,w,2] (S10.5) -- planeseg.cu:199-240."""
        import torch
        n = len(prev_planes)
        if len(flows) != n:
            raise EngineError("one flow per previous plane image")
        _, p, s, _ = _geom(planes, 1)
        out = torch.empty_like(planes)
        _, op, os_, _ = _geom(out, 1)
        P = (C.c_void_p * max(n, 1))(); PS = (C.c_size_t * max(n, 1))(); F = (C.c_void_p * max(n, 1))(); FS = (C.c_size_t * max(n, 1))()
        for k in range(n):
            _, pp, ps, _ = _geom(prev_planes[k], 1)
            _, fp, fs, _ = _geom(flows[k], 2)
            P[k], PS[k], F[k], FS[k] = pp.value, ps, fp.value, fs
        self._check(self._lib.cart_plane_temporal_vote(self._h, p, s, n, P, PS, F, FS, op, os_, _stream_ptr()), "cart_plane_temporal_vote")
        return out

    # ---- superpixel plane labelling (reference src/modules/planeseg/sp_planeseg.cu:27-178) ----
    def superpixel_plane_classify(self, deriv2, labels, max_label, params, prev_planes=(), flows=()):
        """deriv2: int16 [h,w,2]; labels: uint16 [h,w] (torch has no uint16 arithmetic: pass an int16 view);
        -> (planes_unsmoothed, planes) uint8 [h,w]."""
        import torch
        n = len(prev_planes)
        if len(flows) != n:
            raise EngineError("one flow per previous plane image")
        _, dp, ds, _ = _geom(deriv2, 2)
        _, lp, ls, _ = _geom(labels, 1)
        if labels.element_size() != 2:
            raise EngineError("labels must be a 16-bit tensor")
        pp = params if isinstance(params, PlaneParams) else PlaneParams(*params)
        uns = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
        out = torch.empty_like(uns)
        _, up, us, _ = _geom(uns, 1)
        _, op, os_, _ = _geom(out, 1)
        P = (C.c_void_p * max(n, 1))(); PS = (C.c_size_t * max(n, 1))(); F = (C.c_void_p * max(n, 1))(); FS = (C.c_size_t * max(n, 1))()
        for k in range(n):
            _, q, qs, _ = _geom(prev_planes[k], 1)
            _, fp, fs, _ = _geom(flows[k], 2)
            P[k], PS[k], F[k], FS[k] = q.value, qs, fp.value, fs
        self._check(self._lib.cart_superpixel_plane_classify(self._h, dp, ds, lp, ls, int(max_label), C.byref(pp), n, P, PS, F, FS,
                                                             up, us, op, os_, _stream_ptr()), "cart_superpixel_plane_classify")
        return uns, out

    # ---- optical flow (stand-in for src/modules/optflow.cpp; oracle S15) ----
    def optical_flow(self, cur, prev, radius=8, block=2):
        """cur/prev: uint8 [h,w] or [h,w,3] -> int16 [h,w,2] S10.5 flow (previous position = p - (flow >> 5))."""
        import torch
        ch = 3 if cur.dim() == 3 else 1
        _, cp, cs, _ = _geom(cur, 2 if ch == 3 else 1)
        _, pp, ps, _ = _geom(prev, 2 if ch == 3 else 1)
        if tuple(cur.shape[:2]) != (self.height, self.width) or cur.shape != prev.shape:
            raise EngineError("image shape does not match the engine")
        out = torch.empty((self.height, self.width, 2), dtype=torch.int16, device=cur.device)
        _, op, os_, _ = _geom(out, 2)
        self._check(self._lib.cart_optical_flow(self._h, cp, cs, pp, ps, ch, int(radius), int(block), op, os_, _stream_ptr()),
                    "cart_optical_flow")
        return out

    def optical_flow_pyramid(self, cur, prev, levels=4, radius=4, refine_radius=2, block=2, median=True):
        """Coarse-to-fine form (spec S21): same images and output as optical_flow, reach radius * 2^(L-1) + refine_radius * (2^(L-1) - 1)."""
        import torch
        ch = 3 if cur.dim() == 3 else 1
        _, cp, cs, _ = _geom(cur, 2 if ch == 3 else 1)
        _, pp, ps, _ = _geom(prev, 2 if ch == 3 else 1)
        if tuple(cur.shape[:2]) != (self.height, self.width) or cur.shape != prev.shape:
            raise EngineError("image shape does not match the engine")
        fp = _lib.FlowParams(int(levels), int(radius), int(refine_radius), int(block), 1 if median else 0)
        out = torch.empty((self.height, self.width, 2), dtype=torch.int16, device=cur.device)
        _, op, os_, _ = _geom(out, 2)
        self._check(self._lib.cart_optical_flow_pyramid(self._h, cp, cs, pp, ps, ch, C.byref(fp), op, os_, _stream_ptr()),
                    "cart_optical_flow_pyramid")
        return out

    def flow_debug_level(self, level, what):
        """Level `level` of the calling thread's last optical_flow_pyramid call as a numpy array: what = 0 image of cur, 1 of prev
        (uint8 [h_l, w_l]), 2 flow in whole pixels (int16 [h_l, w_l, 2], after the median when it is on).  Synchronises the device."""
        sizes = flow_pyramid_levels(self.width, self.height, _lib.FLOW_MAX_LEVELS)
        if not 0 <= level < len(sizes):
            raise EngineError("flow_debug_level: that level is not built for this image size")
        w, h = sizes[level]
        out = np.empty((h, w, 2), np.int16) if what == 2 else np.empty((h, w), np.uint8)
        self._check(self._lib.cart_flow_debug_level(self._h, int(level), int(what), out.ctypes.data_as(C.c_void_p), out.nbytes), "cart_flow_debug_level")
        return out

    def set_flow_gather(self, on):
        """Tests and measurements: the refinement kernel of optical_flow_pyramid gathers the previous features from global memory in
        every tile instead of staging them in LDS where they fit (same bits)."""
        self._check(self._lib.cart_engine_set_option(self._h, _lib.OPT_FLOW_GATHER, 1 if on else 0), "cart_engine_set_option")

    # ---- depth module (reference src/modules/depth.cpp:9-25) ----
    def reproject_depth(self, disp, Q):
        import torch
        n, p, s, fs = _geom(disp, 1)
        q = (C.c_float * 16)(*[float(v) for v in np.asarray(Q, np.float32).reshape(16)])
        out = torch.empty(tuple(disp.shape) + (3,), dtype=torch.float32, device=disp.device)
        _, op, os_, ofs = _geom(out, 2)
        self._check(self._lib.cart_reproject_depth(self._h, n, p, s, fs, q, op, os_, ofs, _stream_ptr()), "cart_reproject_depth")
        return out

    def plane_ccl(self, planes):
        import torch
        n, p, s, fs = _geom(planes, 1)
        ids = torch.empty(planes.shape, dtype=torch.int32, device=planes.device)
        ncomp = torch.empty((n,), dtype=torch.int32, device=planes.device)
        _, ip, is_, ifs = _geom(ids, 1)
        self._check(self._lib.cart_plane_ccl(self._h, n, p, s, fs, ip, is_, ifs, C.c_void_p(ncomp.data_ptr()),
                                             _stream_ptr()), "cart_plane_ccl")
        return ids, ncomp

    def plane_ccl_stats(self, planes, ids, max_components=4096):
        """-> (table int32 [n, max_components, 7] rows {id, label, area, x0, y0, x1, y1} in ascending id order,
        n_components int32 [n]) -- frames with more components keep their first max_components rows."""
        import torch
        n, p, s, fs = _geom(planes, 1)
        _, ip, is_, ifs = _geom(ids, 1)
        table = torch.empty((n, max_components, 7), dtype=torch.int32, device=planes.device)  # rows >= n_components stay undefined
        ncomp = torch.empty((n,), dtype=torch.int32, device=planes.device)
        self._check(self._lib.cart_plane_ccl_stats(self._h, n, p, s, fs, ip, is_, ifs, C.c_void_p(table.data_ptr()), int(max_components),
                                                   C.c_void_p(ncomp.data_ptr()), _stream_ptr()), "cart_plane_ccl_stats")
        return table, ncomp

    def plane_ccl_table(self, planes, max_components=4096):
        """plane_ccl + plane_ccl_stats in one call (cart_plane_ccl_table: four launches) -> (ids, table, n_components)."""
        import torch
        n, p, s, fs = _geom(planes, 1)
        ids = torch.empty(planes.shape, dtype=torch.int32, device=planes.device)
        _, ip, is_, ifs = _geom(ids, 1)
        table = torch.empty((n, max_components, 7), dtype=torch.int32, device=planes.device)  # rows >= n_components stay undefined
        ncomp = torch.empty((n,), dtype=torch.int32, device=planes.device)
        self._check(self._lib.cart_plane_ccl_table(self._h, n, p, s, fs, ip, is_, ifs, C.c_void_p(table.data_ptr()), int(max_components),
                                                   C.c_void_p(ncomp.data_ptr()), _stream_ptr()), "cart_plane_ccl_table")
        return ids, table, ncomp

    # ---- diagnostics ----
    def debug_ccl_scratch_nonzero(self):
        """Non-zero words of the component-table scratch (must be 0 between calls)."""
        n = C.c_size_t(0)
        self._check(self._lib.cart_debug_ccl_scratch_nonzero(self._h, C.byref(n)), "cart_debug_ccl_scratch_nonzero")
        return n.value

    def debug_read(self, what, frame_slot=0):
        lib = self._lib
        npx = self.width * self.height
        if what in (0, 1):
            buf = np.empty((self.height, self.width), np.uint8)
        elif what in (2, 3):
            buf = np.empty((self.height, self.width), np.uint32)
        elif 16 <= what < 16 + self.P:
            buf = np.empty((self.height, self.width, self.D), np.uint8)
        elif what in (32, 33):
            buf = np.empty((self.height, self.width), np.uint16)
        else:
            raise EngineError("unknown debug selector")
        assert buf.size >= npx
        self._check(lib.cart_debug_read(self._h, frame_slot, what, buf.ctypes.data_as(C.c_void_p), buf.nbytes),
                    "cart_debug_read")
        return buf

    def slab_layout(self):
        """cart_debug_slab_layout -> dict(group_slots, groups, slot_bytes, group_bytes): how the cost-slab workspace is cut into device allocations."""
        gs, ng, sb, gb = C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.cart_debug_slab_layout(self._h, C.byref(gs), C.byref(ng), C.byref(sb), C.byref(gb)), "cart_debug_slab_layout")
        return {"group_slots": gs.value, "groups": ng.value, "slot_bytes": sb.value, "group_bytes": gb.value}

    def set_timing(self, enabled=True, every=1):
        """Stage events on every `every`-th compute call (every=1: all)."""
        self._check(self._lib.cart_engine_set_timing(self._h, max(1, int(every)) if enabled else 0), "cart_engine_set_timing")

    def collect_timing(self):
        """-> ({stage: mean ms per call}, n_calls) over the calls recorded since set_timing(True)."""
        names = (C.c_char_p * 8)()
        ms = (C.c_float * 8)()
        calls = C.c_int(0)
        n = self._lib.cart_engine_collect_timing(self._h, names, ms, 8, C.byref(calls))
        if n < 0:
            raise EngineError("cart_engine_collect_timing: " + self._lib.cart_last_error(self._h).decode())
        return {names[i].decode(): float(ms[i]) for i in range(n)}, calls.value


class _DeviceObject:
    """A C-ABI object made on an engine: cart_<_name>_create(engine, ..., &out) and cart_<_name>_destroy.  A failing call
    raises EngineError with the library's last error.  A context manager: leaving the block closes the object."""
    _name = None

    def __init__(self, engine, *args):
        self._eng = engine
        self._lib = engine._lib
        self._h = C.c_void_p()
        self._check(getattr(self._lib, f"cart_{self._name}_create")(engine._h, *args, C.byref(self._h)), f"cart_{self._name}_create")

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError(f"{what}: " + self._lib.cart_last_error(self._eng._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, f"cart_{self._name}_destroy")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePlaneSchedule(_DeviceObject):
    """Device-side replay of the reference's plane-parameter bookkeeping (cart_plane_schedule_* in the C ABI)."""
    _name = "plane_schedule"

    def __init__(self, engine, provider="histogram_peak", static_params=None, update_interval=30, reset_interval=10):
        if provider not in ("histogram_peak", "static"):
            raise ValueError("Unknown parameter provider type.")  # cartconfig.cpp:77
        init = PlaneParams(*(static_params or (0,) * 6))
        super().__init__(engine, 1 if provider == "histogram_peak" else 0, C.byref(init), update_interval, reset_interval)

    def advance(self, first_id, hists):
        """hists: int32 CUDA [n,256] in frame-id order -> int32 CUDA [n,6] parameters per frame."""
        import torch
        if hists.dtype != torch.int32 or not hists.is_contiguous() or hists.dim() != 2 or hists.shape[1] != 256:
            raise EngineError("hists must be a contiguous int32 [n,256] CUDA tensor")
        out = torch.empty((hists.shape[0], 6), dtype=torch.int32, device=hists.device)
        self._check(self._lib.cart_plane_schedule_advance(self._h, first_id, hists.shape[0], C.c_void_p(hists.data_ptr()),
                                                          C.c_void_p(out.data_ptr()), _stream_ptr()), "cart_plane_schedule_advance")
        return out

    def read(self):
        p = PlaneParams()
        cum = (C.c_int32 * 256)()
        self._check(self._lib.cart_plane_schedule_read(self._h, C.byref(p), cum), "cart_plane_schedule_read")
        return p, np.array(cum, dtype=np.int32)


class Superpixels(_DeviceObject):
    """The reference's ContourRelaxation object (persistent label image + relax), cart_superpixels_* in the C ABI.
    Label images are uint16; torch tensors carry them as int16 (same bits)."""
    _name = "superpixels"

    def __init__(self, engine, block_size=12, direct_clique_cost=0.5, diagonal_clique_cost=None, compactness_weight=0.1,
                 progressive_compactness_cost=0.0, image_weight=1.5, disparity_weight=1.0, block_h=None):
        p = SuperpixelParams(direct_clique_cost, direct_clique_cost / np.sqrt(2.0) if diagonal_clique_cost is None else diagonal_clique_cost,
                             compactness_weight, progressive_compactness_cost, image_weight, disparity_weight)
        self.params = p
        super().__init__(engine, C.byref(p), int(block_size), int(block_h or block_size))

    @property
    def max_label(self):
        return self._lib.cart_superpixels_max_label(self._h)

    def reset(self):
        self._check(self._lib.cart_superpixels_reset(self._h, _stream_ptr()), "cart_superpixels_reset")

    def set_labels(self, labels, max_label_id):
        _, p, s, _ = _geom(labels, 1)
        if labels.element_size() != 2:
            raise EngineError("labels must be a 16-bit tensor")
        self._check(self._lib.cart_superpixels_set_labels(self._h, p, s, int(max_label_id), _stream_ptr()), "cart_superpixels_set_labels")

    def relax(self, image, deriv2, iterations):
        """image: uint8 [h,w,3] BGR or [h,w] gray; deriv2: int16 [h,w,2] or None -> labels int16-viewed uint16 [h,w]."""
        import torch
        ch = 3 if image.dim() == 3 else 1
        _, ip, is_, _ = _geom(image, 2 if ch == 3 else 1)
        if tuple(image.shape[:2]) != (self._eng.height, self._eng.width):
            raise EngineError("image shape does not match the engine")
        dp, ds = C.c_void_p(None), 0
        if deriv2 is not None:
            _, dp, ds, _ = _geom(deriv2, 2)
        out = torch.empty((self._eng.height, self._eng.width), dtype=torch.int16, device=image.device)
        _, op, os_, _ = _geom(out, 1)
        self._check(self._lib.cart_superpixels_relax(self._h, ip, is_, ch, dp, ds, int(iterations), op, os_, _stream_ptr()),
                    "cart_superpixels_relax")
        return out


class PlaneFit(_DeviceObject):
    """Superpixel plane fitting (cart_planefit_* in the C ABI): per-label RANSAC planes, point lists,
    8-neighbour adjacency and the planefit assignment loop on the device.  Labels are uint16 carried as int16 tensors,
    xyz is float32 [h, w, 3] (the "depth" image)."""
    _name = "planefit"

    def __init__(self, engine, max_label_capacity=16383):
        self.max_label = None
        super().__init__(engine, int(max_label_capacity))

    def _labels(self, labels):
        if labels.element_size() != 2 or tuple(labels.shape) != (self._eng.height, self._eng.width):
            raise EngineError("labels must be a 16-bit [h, w] tensor of the engine's size")
        _, p, s, _ = _geom(labels, 1)
        return p, s

    def label_planes(self, labels, xyz, max_label, predicate=_lib.PRED_PLANEFIT, thr=_lib.PLANEFIT_THRESHOLD, seed=0, frame_id=0):
        """S17 for labels 0..max_label -> (planes f64 [L+1, 4], npoints i32 [L+1], counts i32 [L+1, 2] (all, invalid))."""
        import torch
        lp, ls = self._labels(labels)
        if xyz.dtype != torch.float32 or tuple(xyz.shape) != (self._eng.height, self._eng.width, 3):
            raise EngineError("xyz must be float32 [h, w, 3]")
        _, xp, xs, _ = _geom(xyz, 2)
        L1 = int(max_label) + 1
        dev = labels.device
        planes = torch.empty((L1, 4), dtype=torch.float64, device=dev)
        npts = torch.empty(L1, dtype=torch.int32, device=dev)
        counts = torch.empty((L1, 2), dtype=torch.int32, device=dev)
        self._check(self._lib.cart_planefit_label_planes(self._h, lp, ls, int(max_label), xp, xs, int(predicate), float(thr), int(seed), int(frame_id),
                                                         C.c_void_p(planes.data_ptr()), C.c_void_p(npts.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                         _stream_ptr()), "cart_planefit_label_planes")
        self.max_label = int(max_label)
        return planes, npts, counts

    def points(self, capacity=None):
        """Point lists of the last label_planes call -> (points f32 [n, 4], offsets i32 [L+2])."""
        import torch
        cap = int(capacity) if capacity is not None else self._eng.width * self._eng.height
        pts = torch.empty((cap, 4), dtype=torch.float32, device="cuda")
        off = torch.empty(self.max_label + 2, dtype=torch.int32, device="cuda")
        self._check(self._lib.cart_planefit_points(self._h, C.c_void_p(pts.data_ptr()), cap, C.c_void_p(off.data_ptr()), _stream_ptr()),
                    "cart_planefit_points")
        return pts[:int(off[-1].item())], off

    def adjacency(self, labels, max_label):
        """8-neighbour label sets -> (offsets i32 [L+2], neighbours i32 [offsets[-1]])."""
        import torch
        lp, ls = self._labels(labels)
        L1 = int(max_label) + 1
        cap = max(1, min(8 * self._eng.width * self._eng.height, L1 * (L1 - 1)))
        off = torch.empty(L1 + 1, dtype=torch.int32, device=labels.device)
        nb = torch.empty(cap, dtype=torch.int32, device=labels.device)
        self._check(self._lib.cart_planefit_adjacency(self._h, lp, ls, int(max_label), C.c_void_p(off.data_ptr()), C.c_void_p(nb.data_ptr()), cap,
                                                      _stream_ptr()), "cart_planefit_adjacency")
        return off, nb[:int(off[-1].item())]

    def fit(self, labels, seed=0, frame_id=0):
        """S19 after label_planes(predicate=PRED_PLANEFIT) -> (planes f64 [k, 4], assignments u64 as int64 [L+1], launches)."""
        import torch
        lp, ls = self._labels(labels)
        planes = torch.zeros((_lib.PLANEFIT_MAX_PLANES, 4), dtype=torch.float64, device=labels.device)
        assign = torch.empty(self.max_label + 1, dtype=torch.int64, device=labels.device)
        n = torch.empty(1, dtype=torch.int32, device=labels.device)
        launches = C.c_int(0)
        self._check(self._lib.cart_planefit_fit(self._h, lp, ls, int(seed), int(frame_id), C.c_void_p(planes.data_ptr()), C.c_void_p(assign.data_ptr()),
                                                C.c_void_p(n.data_ptr()), C.byref(launches), _stream_ptr()), "cart_planefit_fit")
        k = int(n.item())
        if k < 0:
            raise EngineError("cart_planefit_fit: the label image holds a label above max_label")
        return planes[:k], assign, launches.value

    def status(self):
        """-> True if a label image since the last label_planes / adjacency call held a label above max_label (synchronises)."""
        bad = C.c_int(0)
        self._check(self._lib.cart_planefit_status(self._h, C.byref(bad)), "cart_planefit_status")
        return bool(bad.value)


KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                           ("class_id", "<i4")])   # cart_keypoint = cv::KeyPoint's layout


def orb_levels(width, height, nfeatures=_lib.ORB_DEFAULT_FEATURES):
    """S20 level layout (cart_orb_levels, host only) -> (built levels, [(w_l, h_l, n_l)] for all 8 levels)."""
    lib = _lib.load()
    arr = [(C.c_int * _lib.ORB_LEVELS)() for _ in range(3)]
    n = lib.cart_orb_levels(int(width), int(height), int(nfeatures), *arr)
    if n < 0:
        raise EngineError("cart_orb_levels: " + lib.cart_last_error(None).decode())
    return n, [(arr[0][l], arr[1][l], arr[2][l]) for l in range(_lib.ORB_LEVELS)]


class OrbFeatures(_DeviceObject):
    """ORB keypoints + steered-BRIEF descriptors (cart_orb_* in the C ABI): the work of the reference's
    ImageFeatureDetectorModule (cv::cuda::ORB::create(5000)->detectAndComputeAsync + convert) for images up to
    max_width x max_height."""
    _name = "orb"

    def __init__(self, engine, max_width, max_height, nfeatures=_lib.ORB_DEFAULT_FEATURES):
        self.nfeatures = int(nfeatures)
        self._size = None
        super().__init__(engine, int(max_width), int(max_height), self.nfeatures)

    def levels(self, width=None, height=None):
        """-> (built levels, [(w_l, h_l, n_l)] x 8) for this object's nfeatures; default size = the last detect call's."""
        w, h = (width, height) if width is not None else self._size
        return orb_levels(w, h, self.nfeatures)

    def detect(self, left, right=None, raw=False):
        """uint8 device images, gray [h, w] or BGR [h, w, 3] (row-pitched views allowed; both of one shape) ->
        one (keypoints, descriptors) per image: keypoints = numpy structured KEYPOINT_DTYPE [n] (host, like the reference's
        orb->convert), descriptors = uint8 device tensor [n, 32].  raw=True gives the keypoints as the device float32
        [n, 7] view of the records instead (octave / class_id as float bits)."""
        import torch
        imgs = [left] if right is None else [left, right]
        if any(t.dtype != torch.uint8 or not t.is_cuda for t in imgs):
            raise EngineError("images must be uint8 CUDA tensors")
        if any(t.dim() != imgs[0].dim() or tuple(t.shape) != tuple(imgs[0].shape) for t in imgs) or imgs[0].dim() not in (2, 3):
            raise EngineError("images must share one shape, [h, w] or [h, w, 3]")
        ch = 1 if imgs[0].dim() == 2 else imgs[0].shape[2]
        if ch not in (1, 3):
            raise EngineError("images must be [h, w] or [h, w, 3]")
        h, w = imgs[0].shape[:2]
        geo = [_geom(t, 1 if ch == 1 else 2) for t in imgs]
        n = len(imgs)
        dev = imgs[0].device
        kp = torch.empty((n, self.nfeatures, 7), dtype=torch.float32, device=dev)
        de = torch.empty((n, self.nfeatures, 32), dtype=torch.uint8, device=dev)
        counts = torch.zeros(n, dtype=torch.int32, device=dev)
        ptrs = (C.c_void_p * n)(*[g[1].value for g in geo])
        steps = (C.c_size_t * n)(*[g[2] for g in geo])
        kps = (C.c_void_p * n)(*[kp[i].data_ptr() for i in range(n)])
        des = (C.c_void_p * n)(*[de[i].data_ptr() for i in range(n)])
        self._check(self._lib.cart_orb_detect(self._h, n, ptrs, steps, int(ch), int(w), int(h), kps, des, None,
                                              C.c_void_p(counts.data_ptr()), _stream_ptr()), "cart_orb_detect")
        self._size = (int(w), int(h))
        cnt = counts.cpu().tolist()
        out = []
        for i in range(n):
            k = kp[i, :cnt[i]]
            if not raw:
                k = k.cpu().numpy().view(KEYPOINT_DTYPE).reshape(-1)
            out.append((k, de[i, :cnt[i]]))
        return out

    def debug_level(self, image, level):
        """Level `level` of image `image` (0 = left) of the last detect call -> (uint8 device tensor [h_l, w_l], number of
        NMS survivors of that level before selection)."""
        import torch
        _, lv = self.levels()
        w, h, _ = lv[level]
        dst = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        n = C.c_int32(0)
        self._check(self._lib.cart_orb_debug_level(self._h, int(image), int(level), C.c_void_p(dst.data_ptr()), w, C.byref(n), _stream_ptr()),
                    "cart_orb_debug_level")
        return dst, n.value


MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<i4"), ("second", "<i4")])   # cart_match


def match_params(**fields):
    """cart_match_default_params (spec S22) with the given fields replaced."""
    return _default_params(MatchParams, "match", fields)


class OrbMatcher(_DeviceObject):
    """Brute-force matching of two sets of ORB descriptors (cart_matcher_* in the C ABI, spec S22 in DESIGN.md 7.4): best and
    second-best Hamming distance per query under an optional position / octave gate, distance, ratio and cross-check tests."""
    _name = "matcher"

    def __init__(self, engine, max_features=_lib.ORB_DEFAULT_FEATURES):
        self.max_features = int(max_features)
        super().__init__(engine, self.max_features)

    def _side(self, side):
        """(keypoints, descriptors, count) -> device (keypoints or None, descriptors, int32 count [1], rows available); host arrays are uploaded."""
        import torch
        kp, de, cnt = side
        if not isinstance(de, torch.Tensor):
            de = torch.from_numpy(np.ascontiguousarray(de, dtype=np.uint8)).cuda()
        if de.dtype != torch.uint8 or not de.is_cuda or de.dim() != 2 or de.shape[1] != _lib.ORB_DESCRIPTOR_BYTES or (de.shape[0] > 1 and de.stride(1) != 1):
            raise EngineError("descriptors must be a uint8 CUDA tensor [n, 32] with unit column stride")
        rows = int(de.shape[0])
        if rows == 0:   # an empty tensor has no address: one unread row
            de = torch.zeros((1, _lib.ORB_DESCRIPTOR_BYTES), dtype=torch.uint8, device=de.device)
            kp = None if kp is None else torch.zeros((1, 7), dtype=torch.float32, device=de.device)
        elif kp is not None:
            if not isinstance(kp, torch.Tensor):
                kp = torch.from_numpy(np.ascontiguousarray(kp).view(np.float32).reshape(-1, 7)).cuda()
            if kp.dtype != torch.float32 or not kp.is_cuda or not kp.is_contiguous() or kp.dim() != 2 or kp.shape[1] != 7 or kp.shape[0] < rows:
                raise EngineError("keypoints must be a contiguous float32 CUDA tensor [>= n, 7] (the cart_keypoint records)")
        if cnt is None:
            cnt = rows
        if not isinstance(cnt, torch.Tensor):
            if int(cnt) > rows:
                raise EngineError("count exceeds the descriptor rows")
            return kp, de, torch.tensor([int(cnt)], dtype=torch.int32, device=de.device)
        if cnt.dtype != torch.int32 or not cnt.is_cuda or cnt.numel() != 1:
            raise EngineError("count must be one int32 on the device")
        if rows < self.max_features or (kp is not None and kp.shape[0] < self.max_features):
            raise EngineError("with a device count the descriptor and keypoint tensors must hold max_features rows")
        return kp, de, cnt

    def match(self, query, train, params=None, want_forward=False):
        """query / train = (keypoints, descriptors, count): keypoints float32 device [n, 7] (OrbFeatures.detect(raw=True)) or a
        KEYPOINT_DTYPE array or None (gate off), descriptors uint8 [n, 32] (rows may be pitched), count = a device int32 (no host
        round trip), an int or None (= n).  -> matches as a MATCH_DTYPE array (host), and with want_forward the int32 [nq, 4]
        forward table (j1, d1, d2, i1(j1))."""
        import torch
        p = params if params is not None else match_params()
        qk, qd, qc = self._side(query)
        tk, td, tc = self._side(train)
        dev = qd.device
        matches = torch.empty((self.max_features, 4), dtype=torch.int32, device=dev)
        n = torch.zeros(1, dtype=torch.int32, device=dev)
        fwd = torch.empty((self.max_features, 4), dtype=torch.int32, device=dev) if want_forward else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        step = lambda d: d.stride(0) if d.shape[0] > 1 else _lib.ORB_DESCRIPTOR_BYTES   # noqa: E731
        self._check(self._lib.cart_matcher_match(self._h, C.byref(p), ptr(qd), step(qd), ptr(qk), ptr(qc), ptr(td), step(td), ptr(tk), ptr(tc),
                                                 ptr(matches), ptr(n), ptr(fwd), _stream_ptr()), "cart_matcher_match")
        both = torch.cat([n, qc.reshape(1)]).cpu().tolist()
        out = matches[:both[0]].cpu().numpy().view(MATCH_DTYPE).reshape(-1)
        if want_forward:
            return out, fwd[:min(max(both[1], 0), self.max_features)].cpu().numpy()
        return out


EGO_RESULT_DTYPE = np.dtype([("R", "<f8", 9), ("t", "<f8", 3), ("rms", "<f8"), ("status", "<i4"), ("n_correspondences", "<i4"),
                             ("n_inliers", "<i4"), ("best_hypothesis", "<i4")])   # cart_ego_result
EGO_HYPOTHESIS_DTYPE = np.dtype([("qerr", "<u8"), ("count", "<i4"), ("skipped", "<i4")])   # cart_ego_hypothesis


def ego_params(**fields):
    """cart_ego_default_params (spec S23) with the given fields replaced."""
    return _default_params(EgoParams, "ego", fields)


class EgoMotion(_DeviceObject):
    """Stereo visual odometry from ORB matches (cart_ego_* in the C ABI, spec S23 in DESIGN.md 7.5): landmarks from the stereo
    matches of a frame, then the relative pose p_cur = R p_prev + t from the temporal matches between two frames' landmarks."""
    _name = "ego"

    def __init__(self, engine, camera, max_features=_lib.ORB_DEFAULT_FEATURES):
        """camera = EgoCamera or (fx, fy, cx, cy, baseline)."""
        self.max_features = int(max_features)
        self.camera = _camera(camera)
        super().__init__(engine, self.max_features)

    def _rows(self, a, dtype, width, what):
        """A host array or device tensor of records -> (device tensor [max_features, width] of torch `dtype`, rows given)."""
        import torch
        if isinstance(a, torch.Tensor):
            if a.dtype != dtype or not a.is_cuda or not a.is_contiguous() or a.dim() != 2 or a.shape[1] != width or a.shape[0] < self.max_features:
                raise EngineError(f"{what} on the device must be a contiguous [>= max_features, {width}] tensor of {dtype}")
            return a, int(a.shape[0])
        np_dtype = {torch.float32: np.float32, torch.int32: np.int32, torch.float64: np.float64}[dtype]
        host = np.ascontiguousarray(a)
        host = host.view(np_dtype).reshape(-1, width) if host.dtype.fields else np.asarray(host, np_dtype).reshape(-1, width)
        if len(host) > self.max_features:
            raise EngineError(f"{what}: more than max_features rows")
        full = np.zeros((self.max_features, width), np_dtype)
        full[:len(host)] = host
        return torch.from_numpy(full).cuda(), len(host)

    def _count(self, cnt, rows, given_on_device):
        import torch
        if isinstance(cnt, torch.Tensor):
            if cnt.dtype != torch.int32 or not cnt.is_cuda or cnt.numel() != 1:
                raise EngineError("a count must be one int32 on the device")
            return cnt
        if cnt is None:
            if given_on_device:
                raise EngineError("a device list needs its count")
            cnt = rows
        return torch.tensor([int(cnt)], dtype=torch.int32, device="cuda")

    def triangulate(self, kp_left, kp_right, stereo_matches, left_count=None, stereo_count=None, params=None, raw=False):
        """Keypoints as KEYPOINT_DTYPE arrays or float32 device [max_features, 7] records, matches as a MATCH_DTYPE array or an
        int32 device [max_features, 4] tensor, counts as ints, device int32 or None (= the rows of a host array).
        -> landmarks float64 [left_count, 4] (host), or with raw=True the device tensor [max_features, 4] with no host round trip."""
        import torch
        p = params if params is not None else ego_params()
        kl, nl = self._rows(kp_left, torch.float32, 7, "keypoints")
        kr, _ = self._rows(kp_right, torch.float32, 7, "keypoints")
        sm, ns = self._rows(stereo_matches, torch.int32, 4, "matches")
        lc = self._count(left_count, nl, isinstance(kp_left, torch.Tensor))
        sc = self._count(stereo_count, ns, isinstance(stereo_matches, torch.Tensor))
        lm = torch.empty((self.max_features, 4), dtype=torch.float64, device=kl.device)
        ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        self._check(self._lib.cart_ego_triangulate(self._h, C.byref(self.camera), C.byref(p), ptr(kl), ptr(kr), ptr(lc), ptr(sm), ptr(sc), ptr(lm),
                                                   _stream_ptr()), "cart_ego_triangulate")
        if raw:
            return lm
        return lm[:min(max(int(lc.item()), 0), self.max_features)].cpu().numpy()

    def estimate(self, cur_landmarks, cur_kp_left, prev_landmarks, temporal_matches, temporal_count=None, seed=0, frame_id=0, params=None,
                 want_mask=False, raw=False):
        """Landmarks as float64 [n, 4] arrays or the device tensors of triangulate(raw=True), the current frame's left keypoints and
        the temporal matches as in triangulate.  -> the result as an EGO_RESULT_DTYPE array of one record (host), with want_mask also
        the int32 inlier mask [max_features]; raw=True returns the device tensors (result as 120 bytes) with no host round trip."""
        import torch
        p = params if params is not None else ego_params()
        cl, _ = self._rows(cur_landmarks, torch.float64, 4, "landmarks")
        pl, _ = self._rows(prev_landmarks, torch.float64, 4, "landmarks")
        kl, _ = self._rows(cur_kp_left, torch.float32, 7, "keypoints")
        tm, nt = self._rows(temporal_matches, torch.int32, 4, "matches")
        tc = self._count(temporal_count, nt, isinstance(temporal_matches, torch.Tensor))
        res = torch.zeros(EGO_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device=cl.device)
        mask = torch.empty(self.max_features, dtype=torch.int32, device=cl.device) if want_mask else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        self._check(self._lib.cart_ego_estimate(self._h, C.byref(self.camera), C.byref(p), ptr(cl), ptr(kl), ptr(pl), ptr(tm), ptr(tc),
                                                C.c_uint64(int(seed)), C.c_uint64(int(frame_id)), ptr(res), ptr(mask), _stream_ptr()), "cart_ego_estimate")
        if raw:
            return (res, mask) if want_mask else res
        out = res.cpu().numpy().view(EGO_RESULT_DTYPE).reshape(-1)
        return (out, mask.cpu().numpy()) if want_mask else out

    def debug_hypotheses(self):
        """The (qerr, count, skipped) table of the last estimate call -> EGO_HYPOTHESIS_DTYPE array [hypotheses] (synchronises)."""
        buf = (_lib.EgoHypothesis * _lib.EGO_MAX_HYPOTHESES)()
        n = C.c_int(0)
        self._check(self._lib.cart_ego_debug_hypotheses(self._h, buf, _lib.EGO_MAX_HYPOTHESES, C.byref(n), _stream_ptr()), "cart_ego_debug_hypotheses")
        return np.frombuffer(buf, EGO_HYPOTHESIS_DTYPE, n.value).copy()


PLANE_MAP_CELL_DTYPE = np.dtype([("horizontal", "<u4"), ("vertical", "<u4"), ("y_min", "<i4"), ("y_max", "<i4")])   # cart_plane_map_cell


def plane_map_params(**fields):
    """cart_plane_map_default_params (spec S24) with the given fields replaced."""
    return _default_params(PlaneMapParams, "plane_map", fields)


class PlaneMap(_DeviceObject):
    """World-frame bird's-eye plane map (cart_plane_map_* in the C ABI, spec S24 in DESIGN.md 7.6): a rolling grid of cells_x x
    cells_z cells that every frame's disparity + plane labels vote into through the frame's camera-to-world pose.  Stateful:
    updates must come in frame order."""
    _name = "plane_map"

    def __init__(self, engine, camera, cells_x, cells_z, params=None):
        """camera = EgoCamera or (fx, fy, cx, cy, baseline); params = PlaneMapParams (default: plane_map_params())."""
        self.camera = _camera(camera)
        self.cells_x, self.cells_z = int(cells_x), int(cells_z)
        self.params = params if params is not None else plane_map_params()
        super().__init__(engine, self.cells_x, self.cells_z, C.byref(self.params))

    def update(self, disp, planes, pose, raw=False):
        """One frame: disp int16 [h, w] (x16), planes uint8 [h, w], pose = 12 numbers (3 x 4 camera-to-world, KITTI row order, host).
        raw=True takes the two device tensors as they are (rows may be pitched) with no conversion or upload.  -> (ox, oz)."""
        import torch
        if not raw:
            disp, planes = _to_device(disp, torch.int16, via_host=True), _to_device(planes, torch.uint8, via_host=True)
        if not isinstance(disp, torch.Tensor) or not isinstance(planes, torch.Tensor) or disp.dtype != torch.int16 or planes.dtype != torch.uint8:
            raise EngineError("disp must be an int16 and planes a uint8 device tensor")
        if disp.dim() != 2 or planes.shape != disp.shape:
            raise EngineError("disp and planes must be [h, w] images of one size")
        images = _pitched(disp, 1) + _pitched(planes, 1)
        self._check(self._lib.cart_plane_map_update(self._h, C.byref(self.camera), _pose12(pose), *images, int(disp.shape[1]), int(disp.shape[0]),
                                                    _stream_ptr()), "cart_plane_map_update")
        return self.window()[:2]

    def window(self):
        """-> (ox, oz, valid): the window origin in absolute cells; valid is False after create / clear (host getter)."""
        ox, oz, valid = C.c_int64(0), C.c_int64(0), C.c_int(0)
        self._check(self._lib.cart_plane_map_window(self._h, C.byref(ox), C.byref(oz), C.byref(valid)), "cart_plane_map_window")
        return ox.value, oz.value, bool(valid.value)

    def read(self):
        """-> (cells PLANE_MAP_CELL_DTYPE [cells_z, cells_x] in window order, (ox, oz)); synchronises."""
        cells = np.empty((self.cells_z, self.cells_x), PLANE_MAP_CELL_DTYPE)
        ox, oz = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.cart_plane_map_read(self._h, C.c_void_p(cells.ctypes.data), C.byref(ox), C.byref(oz), _stream_ptr()), "cart_plane_map_read")
        return cells, (ox.value, oz.value)

    def classify(self, min_votes=3, obstacle_percent=50, raw=False):
        """-> uint8 [cells_z, cells_x] in window order: 0 free, 1 obstacle, 2 unknown (host array; raw=True: the device tensor)."""
        import torch
        out = torch.empty((self.cells_z, self.cells_x), dtype=torch.uint8, device="cuda")
        self._check(self._lib.cart_plane_map_classify(self._h, int(min_votes), int(obstacle_percent), C.c_void_p(out.data_ptr()), self.cells_x,
                                                      _stream_ptr()), "cart_plane_map_classify")
        return out if raw else out.cpu().numpy()

    def clear(self):
        self._check(self._lib.cart_plane_map_clear(self._h), "cart_plane_map_clear")

    def rebuild(self, store, ids, poses, window_pose, raw=False):
        """Spec S30: empties the window of `window_pose` (12 numbers, host) and votes every frame of the PlaneStore
        `store` that `ids` names, entry k through poses[k] (12 numbers each, host).  Ids the store does not hold are skipped.  Ids and
        poses are host data either way; `raw` is accepted for symmetry with update().  -> ((ox, oz), used)."""
        if not isinstance(store, PlaneStore):
            raise EngineError("store must be a PlaneStore")
        ids = [int(i) for i in ids]
        flat = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1))
        if len(flat) != 12 * len(ids):
            raise EngineError("poses must hold 12 numbers for every id")
        used = C.c_int(0)
        self._check(self._lib.cart_plane_map_rebuild(self._h, store._h, C.byref(self.camera), (C.c_uint64 * max(len(ids), 1))(*ids),
                                                     (C.c_double * max(len(flat), 1))(*flat.tolist()), len(ids), _pose12(window_pose), C.byref(used),
                                                     _stream_ptr()), "cart_plane_map_rebuild")
        return self.window()[:2], used.value


class PlaneStore(_DeviceObject):
    """Device-resident ring of keyframe images for PlaneMap.rebuild (cart_plane_store_* in the C ABI, spec S30 in DESIGN.md 7.12):
    up to `capacity` frames of exactly width x height, the disparity (int16 x16) and the labels (uint8) copied verbatim."""
    _name = "plane_store"

    def __init__(self, engine, width, height, capacity):
        self.width, self.height, self.capacity = int(width), int(height), int(capacity)
        super().__init__(engine, self.width, self.height, self.capacity)

    def insert(self, frame_id, disp, planes, raw=False):
        """disp int16 [h, w] (x16) and planes uint8 [h, w] under frame_id; raw=True takes the two device tensors as they are (rows
        may be pitched).  The oldest frame leaves a full store."""
        import torch
        if not raw:
            disp, planes = _to_device(disp, torch.int16, via_host=True), _to_device(planes, torch.uint8, via_host=True)
        if not isinstance(disp, torch.Tensor) or not isinstance(planes, torch.Tensor) or disp.dtype != torch.int16 or planes.dtype != torch.uint8:
            raise EngineError("disp must be an int16 and planes a uint8 device tensor")
        if disp.dim() != 2 or planes.shape != disp.shape:
            raise EngineError("disp and planes must be [h, w] images of one size")
        images = _pitched(disp, 1) + _pitched(planes, 1)
        self._check(self._lib.cart_plane_store_insert(self._h, C.c_uint64(int(frame_id)), *images, int(disp.shape[1]), int(disp.shape[0]), _stream_ptr()),
                    "cart_plane_store_insert")

    def contains(self, frame_id):
        """-> whether frame_id is held (host getter)."""
        slot = C.c_int(-1)
        self._check(self._lib.cart_plane_store_contains(self._h, C.c_uint64(int(frame_id)), C.byref(slot)), "cart_plane_store_contains")
        return slot.value >= 0

    def size(self):
        """-> (frames held, capacity) (host getter)."""
        frames, capacity = C.c_int(0), C.c_int(0)
        self._check(self._lib.cart_plane_store_size(self._h, C.byref(frames), C.byref(capacity)), "cart_plane_store_size")
        return frames.value, capacity.value

    def clear(self):
        self._check(self._lib.cart_plane_store_clear(self._h), "cart_plane_store_clear")


def motion_params(**fields):
    """cart_motion_default_params (spec S25) with the given fields replaced."""
    return _default_params(MotionParams, "motion", fields)


MotionSegmentation = collections.namedtuple("MotionSegmentation", "residual raw labels planes_static")


def motion_segment(engine, camera, rel, disp_cur, disp_prev, flow, params=None, planes=None, residual=True, raw=False):
    """Motion segmentation of one frame (cart_motion_segment, spec S25 in DESIGN.md 7.7): camera = EgoCamera or (fx, fy, cx, cy, baseline),
    rel = 12 numbers, the 3 x 4 (R | t) with p_cur = R p_prev + t (host); disp_cur / disp_prev int16 [h, w] (x16), flow int16 [h, w, 2]
    (S10.5), planes uint8 [h, w] or None.  raw=True takes device tensors as they are (rows may be pitched) and returns device tensors;
    otherwise host arrays go up and numpy arrays come back.  -> MotionSegmentation(residual int16 [h, w, 4] or None when residual is
    false, raw uint8 [h, w], labels uint8 [h, w], planes_static uint8 [h, w] or None when planes is)."""
    import torch
    cam = _camera(camera)
    p = params if params is not None else motion_params()
    dc, dp, fl, pl = disp_cur, disp_prev, flow, planes
    if not raw:   # device tensors go through the host too
        dc, dp, fl, pl = (_to_device(a, dtype, via_host=True) for a, dtype in ((dc, torch.int16), (dp, torch.int16), (fl, torch.int16), (pl, torch.uint8)))
    for t, dtype, what, channels in ((dc, torch.int16, "disp_cur", None), (dp, torch.int16, "disp_prev", None), (fl, torch.int16, "flow", 2), (pl, torch.uint8, "planes", None)):
        if t is not None or what != "planes":
            _check_frame_image(t, dtype, what, dc, channels)
    h, w = int(dc.shape[0]), int(dc.shape[1])
    res = torch.empty((h, w, 4), dtype=torch.int16, device=dc.device) if residual else None
    rawl = torch.empty((h, w), dtype=torch.uint8, device=dc.device)
    labels = torch.empty((h, w), dtype=torch.uint8, device=dc.device)
    static = torch.empty((h, w), dtype=torch.uint8, device=dc.device) if pl is not None else None
    args = _pitched(dc, 1) + _pitched(dp, 1) + _pitched(fl, 2) + [w, h]
    for t, inner in ((res, 2), (rawl, 1), (labels, 1), (pl, 1), (static, 1)):
        args += _pitched(t, inner)
    if _lib.load().cart_motion_segment(engine._h, C.byref(cam), _pose12(rel), C.byref(p), *args, _stream_ptr()) != 0:
        raise EngineError("cart_motion_segment: " + _lib.load().cart_last_error(None).decode())
    out = MotionSegmentation(res, rawl, labels, static)
    return out if raw else MotionSegmentation(*[t.cpu().numpy() if t is not None else None for t in out])


PLACE_CANDIDATE_DTYPE = np.dtype([("slot", "<i4"), ("score", "<i4"), ("frame_id", "<u8")])   # cart_place_candidate


def place_params(**fields):
    """cart_place_default_params (spec S27) with the given fields replaced."""
    return _default_params(PlaceParams, "place", fields)


class PlaceDB(_DeviceObject):
    """Place recognition over a device-resident ring of stored frames (cart_place_* in the C ABI, spec S27 in DESIGN.md 7.9): `capacity`
    slots of up to max_features ORB features each; query() scores a frame's descriptors against every stored frame in two launches."""
    _name = "place"

    def __init__(self, engine, max_features=_lib.ORB_DEFAULT_FEATURES, capacity=256):
        self.max_features, self.capacity = int(max_features), int(capacity)
        super().__init__(engine, self.max_features, self.capacity)

    def _rows(self, desc, count, what, full=False):
        """-> (descriptor tensor, step, device int32 count): host arrays go up; a device count needs max_features rows.  full: a shorter
        set is copied into a buffer of max_features rows, the extent cart_place_query's overlap check takes the query set to have."""
        import torch
        if not isinstance(desc, torch.Tensor):
            desc = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, _lib.ORB_DESCRIPTOR_BYTES)).cuda()
        if desc.dtype != torch.uint8 or not desc.is_cuda or desc.dim() != 2 or desc.shape[1] != _lib.ORB_DESCRIPTOR_BYTES or (desc.shape[0] > 1 and desc.stride(1) != 1):
            raise EngineError(f"{what} must be a uint8 CUDA tensor [n, 32] with unit column stride")
        rows = int(desc.shape[0])
        if count is None:
            count = rows
        if not isinstance(count, torch.Tensor) and int(count) > rows:
            raise EngineError("count exceeds the descriptor rows")
        if rows == 0 or (full and rows < self.max_features):   # an empty tensor has no address: one unread row
            padded = torch.zeros((self.max_features if full else 1, _lib.ORB_DESCRIPTOR_BYTES), dtype=torch.uint8, device=desc.device)
            padded[:rows] = desc
            desc = padded
        if not isinstance(count, torch.Tensor):
            count = torch.tensor([int(count)], dtype=torch.int32, device=desc.device)
        elif count.dtype != torch.int32 or not count.is_cuda or count.numel() != 1:
            raise EngineError("count must be one int32 on the device")
        elif rows < self.max_features:
            raise EngineError("with a device count the tensors must hold max_features rows")
        return desc, (desc.stride(0) if desc.shape[0] > 1 else _lib.ORB_DESCRIPTOR_BYTES), count

    def insert(self, desc, keypoints, frame_id, landmarks=None, count=None):
        """Stores a frame: desc uint8 [n, 32] (rows may be pitched), keypoints float32 device [>= n, 7] or a KEYPOINT_DTYPE array, landmarks
        float64 [>= n, 4] (EgoMotion.triangulate's) or None, count = a device int32, an int or None (= n).  -> the slot taken.  No
        host synchronisation."""
        import torch
        de, step, cnt = self._rows(desc, count, "desc")
        need = self.max_features if isinstance(count, torch.Tensor) else int(de.shape[0])
        kp = keypoints
        if not isinstance(kp, torch.Tensor):
            kp = torch.from_numpy(np.ascontiguousarray(kp).view(np.float32).reshape(-1, 7)).cuda()
        if kp.shape[0] == 0:
            kp = torch.zeros((1, 7), dtype=torch.float32, device=de.device)
        lm = landmarks
        if lm is not None and not isinstance(lm, torch.Tensor):
            lm = torch.from_numpy(np.ascontiguousarray(lm, dtype=np.float64).reshape(-1, 4)).cuda()
        if lm is not None and lm.shape[0] == 0:
            lm = torch.zeros((1, 4), dtype=torch.float64, device=de.device)
        if kp.dtype != torch.float32 or not kp.is_cuda or not kp.is_contiguous() or kp.dim() != 2 or kp.shape[1] != 7 or kp.shape[0] < need:
            raise EngineError("keypoints must be a contiguous float32 CUDA tensor [>= n, 7] (the cart_keypoint records)")
        if lm is not None and (lm.dtype != torch.float64 or not lm.is_cuda or not lm.is_contiguous() or lm.dim() != 2 or lm.shape[1] != 4 or lm.shape[0] < need):
            raise EngineError("landmarks must be a contiguous float64 CUDA tensor [>= n, 4]")
        slot = C.c_int32(-1)
        self._check(self._lib.cart_place_insert(self._h, C.c_void_p(de.data_ptr()), step, C.c_void_p(kp.data_ptr()),
                                                C.c_void_p(lm.data_ptr()) if lm is not None else None, C.c_void_p(cnt.data_ptr()), int(frame_id),
                                                C.byref(slot), _stream_ptr()), "cart_place_insert")
        return slot.value

    def query(self, desc, frame_id, params=None, count=None, want_scores=True):
        """Scores desc (as insert's) of frame frame_id against every slot.  -> (scores int32 [capacity] or None, candidates int64
        [max_candidates, 2] holding the 16-byte cart_place_candidate records (view them as PLACE_CANDIDATE_DTYPE on the host), n int32
        [1]), all device tensors: no host synchronisation.  Records from n on are not written."""
        import torch
        p = params if params is not None else place_params()
        de, step, cnt = self._rows(desc, count, "desc", full=True)
        scores = torch.empty(self.capacity, dtype=torch.int32, device=de.device) if want_scores else None
        cand = torch.zeros((max(int(p.max_candidates), 1), 2), dtype=torch.int64, device=de.device)
        n = torch.zeros(1, dtype=torch.int32, device=de.device)
        self._check(self._lib.cart_place_query(self._h, C.byref(p), C.c_void_p(de.data_ptr()), step, C.c_void_p(cnt.data_ptr()), int(frame_id),
                                               C.c_void_p(scores.data_ptr()) if scores is not None else None, C.c_void_p(cand.data_ptr()),
                                               C.c_void_p(n.data_ptr()), _stream_ptr()), "cart_place_query")
        return scores, cand, n

    def slot(self, k):
        """-> (desc, keypoints, landmarks or None, count) of slot k as device addresses (ints) into the ring, for cart_matcher_match and
        cart_ego_estimate; the descriptor step is 32.  Host only."""
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self._lib.cart_place_slot(self._h, int(k), *[C.byref(q) for q in ptrs]), "cart_place_slot")
        return tuple(q.value for q in ptrs)

    def clear(self):
        self._check(self._lib.cart_place_clear(self._h, _stream_ptr()), "cart_place_clear")


POSE_GRAPH_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_nodes", "<i4"), ("n_loops", "<i4"), ("iterations", "<i4"), ("cost_before", "<f8"),
                                   ("cost_after", "<f8")])   # cart_pose_graph_result


def pose_graph_params(**fields):
    """cart_pose_graph_default_params (spec S29) with the given fields replaced."""
    return _default_params(PoseGraphParams, "pose_graph", fields)


class PoseGraph(_DeviceObject):
    """Pose-graph optimisation over keyframes (cart_pose_graph_* in the C ABI, spec S29 in DESIGN.md 7.11): nodes are camera-to-world poses
    in insertion order with an odometry edge between neighbours, loop edges join any two nodes, optimize() runs Gauss-Newton over all nodes
    but the first on the device.  Stateful in call order."""
    _name = "pose_graph"

    def __init__(self, engine, max_nodes=1024, max_loops=64):
        self.max_nodes, self.max_loops = int(max_nodes), int(max_loops)
        super().__init__(engine, self.max_nodes, self.max_loops)

    def add_node(self, pose, w_rot, w_trans):
        """pose = 12 numbers (3 x 4 camera-to-world, KITTI row order, host); the weights of the odometry edge to the previous node.
        -> the node's index.  No host synchronisation."""
        node = C.c_int32(-1)
        self._check(self._lib.cart_pose_graph_add_node(self._h, _pose12(pose), float(w_rot), float(w_trans), C.byref(node), _stream_ptr()), "cart_pose_graph_add_node")
        return node.value

    def add_loop(self, a, b, R, t, w_rot, w_trans):
        """The loop edge p_b = R p_a + t between nodes a and b: R = 9 numbers in row order, t = 3 (host)."""
        Rh = (C.c_double * 9)(*[float(v) for v in np.asarray(R, np.float64).reshape(-1)])
        th = (C.c_double * 3)(*[float(v) for v in np.asarray(t, np.float64).reshape(-1)])
        self._check(self._lib.cart_pose_graph_add_loop(self._h, int(a), int(b), Rh, th, float(w_rot), float(w_trans), _stream_ptr()), "cart_pose_graph_add_loop")

    def optimize(self, iterations=None, params=None, raw=False):
        """`iterations` Gauss-Newton steps (default: pose_graph_params()'s 4) -> the POSE_GRAPH_RESULT_DTYPE record [1] (synchronises);
        raw=True: the device tensor of 4 doubles that holds it, no host synchronisation."""
        import torch
        p = params if params is not None else (pose_graph_params(iterations=int(iterations)) if iterations is not None else pose_graph_params())
        out = torch.zeros(POSE_GRAPH_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device="cuda")
        self._check(self._lib.cart_pose_graph_optimize(self._h, C.byref(p), C.c_void_p(out.data_ptr()), _stream_ptr()), "cart_pose_graph_optimize")
        return out if raw else out.cpu().numpy().view(POSE_GRAPH_RESULT_DTYPE)

    def poses(self, first=0, count=None, raw=False):
        """-> float64 [count, 12], the estimates of nodes first .. first + count - 1 (default: all); raw=True: the device tensor, no
        host synchronisation."""
        import torch
        n = self.size()[0] - int(first) if count is None else int(count)
        out = torch.zeros((max(n, 0), 12), dtype=torch.float64, device="cuda")
        self._check(self._lib.cart_pose_graph_poses(self._h, int(first), n, C.c_void_p(out.data_ptr()) if n > 0 else C.c_void_p(8), _stream_ptr()), "cart_pose_graph_poses")
        return out if raw else out.cpu().numpy()

    def size(self):
        """-> (nodes, loops); host only."""
        nodes, loops = C.c_int(0), C.c_int(0)
        self._check(self._lib.cart_pose_graph_size(self._h, C.byref(nodes), C.byref(loops)), "cart_pose_graph_size")
        return nodes.value, loops.value

    def clear(self):
        self._check(self._lib.cart_pose_graph_clear(self._h, _stream_ptr()), "cart_pose_graph_clear")


LOCAL_BA_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_frames", "<i4"), ("n_points_active", "<i4"), ("n_observations", "<i4"), ("n_held", "<i4"),
                                  ("iterations", "<i4"), ("cost_before", "<f8"), ("cost_after", "<f8")])   # cart_local_ba_result


def local_ba_params(**fields):
    """cart_local_ba_default_params (spec S32; build-owned, untuned) with the given fields replaced."""
    return _default_params(LocalBAParams, "local_ba", fields)


class LocalBA(_DeviceObject):
    """Windowed bundle adjustment over the last frames (cart_local_ba_* in the C ABI, spec S32 in DESIGN.md 7.14): push() builds feature
    tracks from a frame's keypoints and match lists, optimize() refines the poses of the window and the points they share on the device.
    Stateful in call order.  A context manager; close() destroys the device object."""
    _name = "local_ba"

    def __init__(self, engine, max_features=_lib.ORB_DEFAULT_FEATURES, window=8, max_points=8192):
        self.max_features, self.window, self.max_points = int(max_features), int(window), int(max_points)
        super().__init__(engine, self.max_features, self.window, self.max_points)

    _rows, _count = EgoMotion._rows, EgoMotion._count   # the same lists, padded to max_features, and their device counts

    def push(self, camera, frame_id, pose, kp_left, kp_right, stereo_matches, temporal_matches, left_count=None, stereo_count=None, temporal_count=None,
             params=None, raw=False):
        """One frame: camera = EgoCamera or (fx, fy, cx, cy, baseline); pose = 12 numbers (3 x 4 camera-to-world, host); keypoints as KEYPOINT_DTYPE arrays or float32 device [max_features, 7]
        records, matches as MATCH_DTYPE arrays or int32 device [max_features, 4] tensors, counts as ints, device int32 or None (= the rows
        of a host array).  -> the int32 [8] counts (host, synchronises), or with raw=True the device tensor with no host round trip."""
        import torch
        p = params if params is not None else local_ba_params()
        kl, nl = self._rows(kp_left, torch.float32, 7, "keypoints")
        kr, _ = self._rows(kp_right, torch.float32, 7, "keypoints")
        sm, ns = self._rows(stereo_matches, torch.int32, 4, "matches")
        tm, nt = self._rows(temporal_matches, torch.int32, 4, "matches")
        lc = self._count(left_count, nl, isinstance(kp_left, torch.Tensor))
        sc = self._count(stereo_count, ns, isinstance(stereo_matches, torch.Tensor))
        tc = self._count(temporal_count, nt, isinstance(temporal_matches, torch.Tensor))
        counts = torch.zeros(8, dtype=torch.int32, device="cuda")
        ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        self._check(self._lib.cart_local_ba_push(self._h, C.byref(_camera(camera)), C.byref(p), C.c_uint64(int(frame_id)), _pose12(pose), ptr(kl), ptr(kr), ptr(lc),
                                                 ptr(sm), ptr(sc), ptr(tm), ptr(tc), ptr(counts), _stream_ptr()), "cart_local_ba_push")
        return counts if raw else counts.cpu().numpy()

    def optimize(self, camera, params=None, raw=False, **fields):
        """Gauss-Newton over the window with camera = EgoCamera or (fx, fy, cx, cy, baseline) (local_ba_params(**fields) unless params is given) -> the LOCAL_BA_RESULT_DTYPE record [1]
        (synchronises); raw=True: the device tensor of 5 doubles that holds it, no host synchronisation."""
        import torch
        p = params if params is not None else local_ba_params(**fields)
        out = torch.zeros(LOCAL_BA_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device="cuda")
        self._check(self._lib.cart_local_ba_optimize(self._h, C.byref(_camera(camera)), C.byref(p), C.c_void_p(out.data_ptr()), _stream_ptr()), "cart_local_ba_optimize")
        return out if raw else out.cpu().numpy().view(LOCAL_BA_RESULT_DTYPE)

    def poses(self, raw=False):
        """-> (float64 [window, 12] estimates in age order, oldest first, rows past the frames in the window zero; uint64 [window] frame
        ids); raw=True: the device tensors (the ids as int64), no host synchronisation."""
        import torch
        out = torch.zeros((self.window, 12), dtype=torch.float64, device="cuda")
        ids = torch.zeros(self.window, dtype=torch.int64, device="cuda")
        self._check(self._lib.cart_local_ba_poses(self._h, C.c_void_p(out.data_ptr()), C.c_void_p(ids.data_ptr()), _stream_ptr()), "cart_local_ba_poses")
        return (out, ids) if raw else (out.cpu().numpy(), ids.cpu().numpy().view(np.uint64))

    def points(self, raw=False):
        """-> float64 [max_points, 4] = (X, Y, Z, n_obs) of every point slot, zeros in a free one."""
        import torch
        out = torch.zeros((self.max_points, 4), dtype=torch.float64, device="cuda")
        self._check(self._lib.cart_local_ba_points(self._h, C.c_void_p(out.data_ptr()), _stream_ptr()), "cart_local_ba_points")
        return out if raw else out.cpu().numpy()

    def track_of(self, raw=False):
        """-> int32 [max_features]: the point slot of every left index of the newest frame, -1 without."""
        import torch
        out = torch.zeros(self.max_features, dtype=torch.int32, device="cuda")
        self._check(self._lib.cart_local_ba_track_of(self._h, C.c_void_p(out.data_ptr()), _stream_ptr()), "cart_local_ba_track_of")
        return out if raw else out.cpu().numpy()

    def size(self):
        """-> (frames in the window, max_points); host only."""
        frames, cap = C.c_int(0), C.c_int(0)
        self._check(self._lib.cart_local_ba_size(self._h, C.byref(frames), C.byref(cap)), "cart_local_ba_size")
        return frames.value, cap.value

    def clear(self):
        self._check(self._lib.cart_local_ba_clear(self._h, _stream_ptr()), "cart_local_ba_clear")


DENSE_EGO_RESULT_DTYPE = np.dtype([("R", "<f8", 9), ("t", "<f8", 3), ("rms_initial", "<f8"), ("rms", "<f8"), ("status", "<i4"), ("n_candidates", "<i4"),
                                   ("n_initial", "<i4"), ("n_inliers", "<i4"), ("steps", "<i4"), ("reserved", "<i4")])   # cart_dense_ego_result


def dense_ego_params(**fields):
    """cart_dense_ego_default_params (spec S26) with the given fields replaced."""
    return _default_params(DenseEgoParams, "dense_ego", fields)


class DenseEgo(_DeviceObject):
    """Dense refinement of a relative pose from flow and disparity (cart_dense_ego_* in the C ABI, spec S26 in DESIGN.md 7.8): Gauss-Newton
    over every static pixel of frames of up to max_width x max_height.  A context manager; close() destroys the device object."""
    _name = "dense_ego"

    def __init__(self, engine, max_width, max_height):
        self.max_width, self.max_height = int(max_width), int(max_height)
        super().__init__(engine, self.max_width, self.max_height)

    def refine(self, camera, rel, disp_cur, disp_prev, flow, params=None, mask=None, stream=None, raw=False):
        """camera = EgoCamera or (fx, fy, cx, cy, baseline); rel = 12 numbers, the 3 x 4 (R | t) to refine (host); disp_cur / disp_prev int16
        [h, w] (x16), flow int16 [h, w, 2] (S10.5), mask uint8 [h, w] (motion_segment's labels) or None: device tensors are taken as they
        are (rows may be pitched), host arrays go up.  stream = a torch stream (default: the current one).  -> the result as a
        DENSE_EGO_RESULT_DTYPE array of one record (host); raw=True returns the device tensor (136 bytes as float64) with no host round
        trip."""
        import torch
        cam = _camera(camera)
        p = params if params is not None else dense_ego_params()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # uploads and the result's allocation on the call's stream
            dc, dp, fl, mk = _to_device(disp_cur, torch.int16), _to_device(disp_prev, torch.int16), _to_device(flow, torch.int16), _to_device(mask, torch.uint8)
        for t, dtype, what, channels in ((dc, torch.int16, "disp_cur", None), (dp, torch.int16, "disp_prev", None), (fl, torch.int16, "flow", 2), (mk, torch.uint8, "mask", None)):
            if t is not None or what != "mask":
                _check_frame_image(t, dtype, what, dc, channels)
        h, w = int(dc.shape[0]), int(dc.shape[1])
        args = _pitched(dc, 1) + _pitched(dp, 1) + _pitched(fl, 2) + _pitched(mk, 1)
        res = torch.empty(DENSE_EGO_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device=dc.device)   # every byte is written by the call
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_dense_ego_refine(self._h, C.byref(cam), _pose12(rel), C.byref(p), *args, w, h, C.c_void_p(res.data_ptr()), sp),
                    "cart_dense_ego_refine")
        if raw:
            return res
        if stream is not None:
            stream.synchronize()
        return res.cpu().numpy().view(DENSE_EGO_RESULT_DTYPE).reshape(-1)


def fusion_params(**fields):
    """cart_fusion_default_params (spec S28; the defaults are build-owned and untuned) with the given fields replaced."""
    return _default_params(FusionParams, "fusion", fields)


class DisparityFusion(_DeviceObject):
    """Temporal disparity fusion through ego-motion (cart_fusion_* in the C ABI, spec S28 in DESIGN.md 7.10): the previous call's fused
    disparity, forward-projected through the relative pose into a z-buffer, fused with this frame's disparity, for frames of up to
    max_width x max_height.  A context manager; close() destroys the device object."""
    _name = "fusion"

    def __init__(self, engine, max_width, max_height):
        self.max_width, self.max_height = int(max_width), int(max_height)
        super().__init__(engine, self.max_width, self.max_height)

    def update(self, camera, rel, disp_cur, prev=None, mask_prev=None, mask_cur=None, params=None, source=True, raw=False, stream=None):
        """camera = EgoCamera or (fx, fy, cx, cy, baseline); rel = 12 numbers, the 3 x 4 (R | t) with p_cur = R p_prev + t (host; None is
        allowed without prev); disp_cur int16 [h, w] (x16); prev = (fused, age) of the previous call or None (no previous frame);
        mask_prev / mask_cur uint8 [h, w] (motion_segment's labels of the previous / this frame) or None.  Device tensors are taken as they
        are (rows may be pitched), host arrays go up.  stream = a torch stream (default: the current one).
        -> (fused int16 [h, w], age uint8 [h, w], source uint8 [h, w] or None when source is false, counts int32 [5]) as numpy arrays;
        raw=True returns the device tensors with no host round trip."""
        import torch
        cam = _camera(camera)
        p = params if params is not None else fusion_params()
        pd, pa = prev if prev is not None else (None, None)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # uploads and allocations on the call's stream
            dc, pd, pa = _to_device(disp_cur, torch.int16), _to_device(pd, torch.int16), _to_device(pa, torch.uint8)
            mp, mc = _to_device(mask_prev, torch.uint8), _to_device(mask_cur, torch.uint8)
            if not isinstance(dc, torch.Tensor) or dc.dim() != 2:
                raise EngineError("disp_cur must be an int16 [h, w] image")
            h, w = int(dc.shape[0]), int(dc.shape[1])
            fused = torch.empty((h, w), dtype=torch.int16, device=dc.device)
            age = torch.empty((h, w), dtype=torch.uint8, device=dc.device)
            src = torch.empty((h, w), dtype=torch.uint8, device=dc.device) if source else None
            counts = torch.empty(5, dtype=torch.int32, device=dc.device)
        if (pd is None) != (pa is None):
            raise EngineError("prev must be the pair (fused, age) of the previous call")
        for t, dtype, what in ((dc, torch.int16, "disp_cur"), (pd, torch.int16, "prev[0]"), (pa, torch.uint8, "prev[1]"), (mp, torch.uint8, "mask_prev"), (mc, torch.uint8, "mask_cur")):
            if t is not None:
                _check_frame_image(t, dtype, what, dc)
        args = [v for t in (dc, pd, pa, mp, mc) for v in _pitched(t, 1)] + [w, h] + [v for t in (fused, age, src) for v in _pitched(t, 1)]
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_fusion_update(self._h, C.byref(cam), _pose12(rel), C.byref(p), *args, C.c_void_p(counts.data_ptr()), sp), "cart_fusion_update")
        out = (fused, age, src, counts)
        if raw:
            return out
        if stream is not None:
            stream.synchronize()
        return tuple(t.cpu().numpy() if t is not None else None for t in out)


VOXEL_DTYPE = np.dtype([("tsdf", "<i2"), ("weight", "<u2")])   # cart_voxel
MESH_VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3)])   # cart_mesh_vertex
MESH_QUAD_DTYPE = np.dtype([("v", "<i4", 4)])                                  # cart_mesh_quad


def voxel_map_params(**fields):
    """cart_voxel_map_default_params (spec S33; the defaults are build-owned and untuned) with the given fields replaced."""
    return _default_params(VoxelMapParams, "voxel_map", fields)


class VoxelMap(_DeviceObject):
    """Rolling TSDF voxel map with model raycast (cart_voxel_map_* in the C ABI, spec S33 in DESIGN.md 7.15): a window of cells_x x cells_y x
    cells_z voxels in the world frame that every frame's disparity is averaged into through the frame's camera-to-world pose, and a
    raycast of it from any pose in the format of the disparity image.  Stateful: integrate calls must come in frame order.  A context
    manager; close() destroys the device object."""
    _name = "voxel_map"

    def __init__(self, engine, cells_x, cells_y, cells_z, params=None):
        """params = VoxelMapParams (default: voxel_map_params()); fixed for the object's life."""
        self.cells_x, self.cells_y, self.cells_z = int(cells_x), int(cells_y), int(cells_z)
        self.params = params if params is not None else voxel_map_params()
        super().__init__(engine, self.cells_x, self.cells_y, self.cells_z, C.byref(self.params))

    def integrate(self, camera, pose, disp, mask=None, counts=True, raw=False, stream=None):
        """camera = EgoCamera or (fx, fy, cx, cy, baseline); pose = 12 numbers (3 x 4 camera-to-world, KITTI row order, host); disp int16
        [h, w] (x16); mask uint8 [h, w] (motion_segment's labels) or None.  Device tensors are taken as they are (rows may be pitched), host
        arrays go up.  stream = a torch stream (default: the current one).  -> counts int32 [2] (voxels updated, of them with f < 1) as a
        numpy array, or None when counts is false; raw=True returns the device tensor with no host round trip."""
        import torch
        cam = _camera(camera)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # uploads and allocations on the call's stream
            d, m = _to_device(disp, torch.int16), _to_device(mask, torch.uint8)
            if not isinstance(d, torch.Tensor) or d.dtype != torch.int16 or d.dim() != 2:
                raise EngineError("disp must be an int16 [h, w] image")
            if m is not None:
                _check_frame_image(m, torch.uint8, "mask", d)
            n = torch.empty(2, dtype=torch.int32, device=d.device) if counts else None
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_voxel_map_integrate(self._h, C.byref(cam), _pose12(pose), *_pitched(d, 1), int(d.shape[1]), int(d.shape[0]), *_pitched(m, 1),
                                                       C.c_void_p(n.data_ptr()) if counts else None, sp), "cart_voxel_map_integrate")
        if raw or n is None:
            return n
        if stream is not None:
            stream.synchronize()
        return n.cpu().numpy()

    def raycast(self, camera, pose, width, height, weight=True, status=True, counts=True, raw=False, stream=None):
        """The model seen from `pose` at width x height.  -> (disp_model int16 [h, w], weight uint16 [h, w], status uint8 [h, w], counts
        int32 [3] = rays NONE, HIT, INSIDE) as numpy arrays, None for an output that was not asked for; raw=True returns the device tensors
        (weight as int16: the same bits)."""
        import torch
        cam = _camera(camera)
        w, h = int(width), int(height)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            dm = torch.empty((max(h, 0), max(w, 0)), dtype=torch.int16, device="cuda")
            wm = torch.empty((max(h, 0), max(w, 0)), dtype=torch.int16, device="cuda") if weight else None
            st = torch.empty((max(h, 0), max(w, 0)), dtype=torch.uint8, device="cuda") if status else None
            n = torch.empty(3, dtype=torch.int32, device="cuda") if counts else None
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        images = [C.c_void_p(dm.data_ptr()), 2 * max(w, 0)] + ([C.c_void_p(wm.data_ptr()), 2 * max(w, 0)] if weight else [None, 0]) + \
                 ([C.c_void_p(st.data_ptr()), max(w, 0)] if status else [None, 0])
        self._check(self._lib.cart_voxel_map_raycast(self._h, C.byref(cam), _pose12(pose), w, h, *images, C.c_void_p(n.data_ptr()) if counts else None, sp),
                    "cart_voxel_map_raycast")
        out = (dm, wm, st, n)
        if raw:
            return out
        if stream is not None:
            stream.synchronize()
        dm, wm, st, n = (t.cpu().numpy() if t is not None else None for t in out)
        return dm, (wm.view(np.uint16) if wm is not None else None), st, n

    def window(self):
        """-> ((ox, oy, oz), (cells_x, cells_y, cells_z), valid): the window origin in absolute voxels; valid is False after create / clear
        (host getter)."""
        o, n, valid = (C.c_int64 * 3)(), (C.c_int32 * 3)(), C.c_int(0)
        self._check(self._lib.cart_voxel_map_window(self._h, o, n, C.byref(valid)), "cart_voxel_map_window")
        return tuple(o), tuple(n), bool(valid.value)

    def read(self):
        """-> (voxels VOXEL_DTYPE [cells_z, cells_y, cells_x] in window order, (ox, oy, oz)); synchronises."""
        voxels = np.empty((self.cells_z, self.cells_y, self.cells_x), VOXEL_DTYPE)
        o = (C.c_int64 * 3)()
        self._check(self._lib.cart_voxel_map_read(self._h, C.c_void_p(voxels.ctypes.data), o, _stream_ptr()), "cart_voxel_map_read")
        return voxels, tuple(o)

    def write(self, voxels, origin):
        """The counterpart of read(): voxels VOXEL_DTYPE [cells_z, cells_y, cells_x] in window order (host) become the window at origin =
        (ox, oy, oz), each a multiple of 8 within 2^27; synchronises."""
        v = np.ascontiguousarray(voxels, VOXEL_DTYPE)
        if v.shape != (self.cells_z, self.cells_y, self.cells_x):
            raise EngineError("voxels must be a VOXEL_DTYPE array of [cells_z, cells_y, cells_x]")
        o = (C.c_int64 * 3)(*[int(c) for c in origin])
        self._check(self._lib.cart_voxel_map_write(self._h, C.c_void_p(v.ctypes.data), o, _stream_ptr()), "cart_voxel_map_write")

    def mesh(self, max_vertices, max_quads, min_weight=0, raw=False, stream=None):
        """The surface of the current window by naive surface nets (spec S36).  min_weight = 0 takes the map's own.
        -> (vertices MESH_VERTEX_DTYPE [written], quads MESH_QUAD_DTYPE [written], counts int32 [4] = vertices found, quads found, vertices
        written, quads written, (ox, oy, oz)): positions are metres relative to the window origin; the mesh is whole iff found == written
        for both.  raw=True returns the device tensors instead (vertices float32 [max_vertices, 6], quads int32 [max_quads, 4], counts int32
        [4]) with no host round trip: rows beyond the written counts are uninitialised."""
        import torch
        nv, nq = int(max_vertices), int(max_quads)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # the allocations on the call's stream
            vt = torch.empty((max(nv, 0), 6), dtype=torch.float32, device="cuda")
            qt = torch.empty((max(nq, 0), 4), dtype=torch.int32, device="cuda")
            n = torch.empty(4, dtype=torch.int32, device="cuda")
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        o = (C.c_int64 * 3)()
        self._check(self._lib.cart_voxel_map_mesh(self._h, int(min_weight), C.c_void_p(vt.data_ptr()), nv, C.c_void_p(qt.data_ptr()), nq, C.c_void_p(n.data_ptr()), o, sp),
                    "cart_voxel_map_mesh")
        if raw:
            return vt, qt, n, tuple(o)
        if stream is not None:
            stream.synchronize()
        counts = n.cpu().numpy()
        vertices = vt[:int(counts[2])].cpu().numpy().view(MESH_VERTEX_DTYPE).reshape(-1)
        quads = qt[:int(counts[3])].cpu().numpy().view(MESH_QUAD_DTYPE).reshape(-1)
        return vertices, quads, counts, tuple(o)

    def clear(self):
        self._check(self._lib.cart_voxel_map_clear(self._h), "cart_voxel_map_clear")

    def rebuild(self, store, ids, poses, window_pose, camera, use_mask=False, counts=True, stream=None):
        """Spec S35: starts an empty window at `window_pose` (12 numbers, host) and integrates every frame of the PlaneStore
        `store` that `ids` names into it, entry k through poses[k] (12 numbers each, host), in list order.  Ids the store does not hold are
        skipped.  use_mask reads the stored uint8 plane as integrate's mask.  stream = a torch stream (default: the current one).
        -> ((ox, oy, oz), used, counts int64 [2] (voxel updates over all used entries, of them with f < 1) or None when counts is false)."""
        import torch
        if not isinstance(store, PlaneStore):
            raise EngineError("store must be a PlaneStore")
        cam = _camera(camera)
        ids = [int(i) for i in ids]
        flat = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1))
        if len(flat) != 12 * len(ids):
            raise EngineError("poses must hold 12 numbers for every id")
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # the allocation on the call's stream
            n = torch.empty(2, dtype=torch.int64, device="cuda") if counts else None
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        used = C.c_int(0)
        self._check(self._lib.cart_voxel_map_rebuild(self._h, store._h, C.byref(cam), (C.c_uint64 * max(len(ids), 1))(*ids),
                                                     (C.c_double * max(len(flat), 1))(*flat.tolist()), len(ids), _pose12(window_pose), 1 if use_mask else 0,
                                                     C.byref(used), C.c_void_p(n.data_ptr()) if counts else None, sp), "cart_voxel_map_rebuild")
        if n is not None and stream is not None:
            stream.synchronize()
        return self.window()[0], used.value, (n.cpu().numpy() if n is not None else None)


VOXEL_RGB_DTYPE = np.dtype([("b", "u1"), ("g", "u1"), ("r", "u1"), ("weight", "u1")])   # cart_voxel_rgb


class VoxelColor(_DeviceObject):
    """Colour for a VoxelMap (cart_voxel_color_* in the C ABI, spec S37 in DESIGN.md 7.19): a second volume of (b, g, r, weight) bytes under
    the map's window, which every frame's image is averaged into where the frame's disparity saw the surface, and two read-outs of it: the
    colours of a mesh's vertices and an image of the model behind a disparity image.  Keeps the map's shape and parameters, not the map.
    A context manager; close() destroys the device object."""
    _name = "voxel_color"

    def __init__(self, engine, voxel_map, max_weight=_lib.VOXEL_COLOR_DEFAULT_MAX_WEIGHT):
        if not isinstance(voxel_map, VoxelMap):
            raise EngineError("voxel_map must be a VoxelMap")
        self.cells_x, self.cells_y, self.cells_z, self.max_weight = voxel_map.cells_x, voxel_map.cells_y, voxel_map.cells_z, int(max_weight)
        self._map = voxel_map
        super().__init__(engine, voxel_map._h, self.max_weight)

    def integrate(self, camera, pose, disp, image, mask=None, counts=True, raw=False, stream=None):
        """After the map's integrate of the same frame, with its camera, pose, disp and mask (VoxelMap.integrate), plus image = uint8 [h, w]
        (gray) or [h, w, 3] (B, G, R).  Device tensors are taken as they are (rows may be pitched), host arrays go up.  -> counts int32 [2]
        (voxels coloured, of them without a colour before) as a numpy array, or None when counts is false; raw=True returns the device tensor
        with no host round trip."""
        import torch
        cam = _camera(camera)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # uploads and allocations on the call's stream
            d, im, m = _to_device(disp, torch.int16), _to_device(image, torch.uint8), _to_device(mask, torch.uint8)
            if not isinstance(d, torch.Tensor) or d.dtype != torch.int16 or d.dim() != 2:
                raise EngineError("disp must be an int16 [h, w] image")
            if not isinstance(im, torch.Tensor) or im.dim() not in (2, 3):
                raise EngineError("image must be a uint8 [h, w] or [h, w, 3] image")
            channels = int(im.shape[2]) if im.dim() == 3 else 1
            _check_frame_image(im, torch.uint8, "image", d, channels if im.dim() == 3 else None)
            if m is not None:
                _check_frame_image(m, torch.uint8, "mask", d)
            n = torch.empty(2, dtype=torch.int32, device=d.device) if counts else None
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_voxel_color_integrate(self._h, self._map._h, C.byref(cam), _pose12(pose), *_pitched(d, 1), *_pitched(im, im.dim() - 1), channels,
                                                         int(d.shape[1]), int(d.shape[0]), *_pitched(m, 1), C.c_void_p(n.data_ptr()) if counts else None, sp),
                    "cart_voxel_color_integrate")
        if raw or n is None:
            return n
        if stream is not None:
            stream.synchronize()
        return n.cpu().numpy()

    def colorize(self, vertices, n, origin, raw=False, stream=None):
        """The colours of a mesh's vertices.  vertices, n, origin as VoxelMap.mesh returns them: with raw=True there the float32
        [max_vertices, 6] tensor and the int32 [4] counts tensor (its third word is the count: no host round trip), else the
        MESH_VERTEX_DTYPE array (n is then ignored).  -> VOXEL_RGB_DTYPE [count] whose weight field holds alpha; raw=True returns the
        device tensor uint8 [max_vertices, 4] (b, g, r, alpha), rows beyond the count uninitialised."""
        import torch
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            if isinstance(vertices, torch.Tensor):
                vt, nt = vertices, n[2:3] if n.numel() == 4 else n
                if vt.dtype != torch.float32 or vt.dim() != 2 or vt.shape[1] != 6 or not vt.is_contiguous() or nt.dtype != torch.int32:
                    raise EngineError("vertices must be a contiguous float32 [max_vertices, 6] tensor and n an int32 tensor")
            else:
                v = np.ascontiguousarray(np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1))
                vt = torch.from_numpy(v.view(np.float32).reshape(-1, 6).copy() if len(v) else np.zeros((1, 6), np.float32)).cuda()
                nt = torch.tensor([len(v)], dtype=torch.int32).cuda()
            cap = int(vt.shape[0])
            out = torch.empty((max(cap, 0), 4), dtype=torch.uint8, device="cuda")
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        o = (C.c_int64 * 3)(*[int(c) for c in origin])
        self._check(self._lib.cart_voxel_color_vertices(self._h, C.c_void_p(vt.data_ptr()), C.c_void_p(nt.data_ptr()), cap, o, C.c_void_p(out.data_ptr()), sp),
                    "cart_voxel_color_vertices")
        if raw:
            return out
        if stream is not None:
            stream.synchronize()
        count = max(0, min(int(nt.cpu()[0]), cap))
        return out[:count].cpu().numpy().view(VOXEL_RGB_DTYPE).reshape(-1)

    def render(self, camera, pose, disp, alpha=True, counts=True, raw=False, stream=None):
        """The model's colours behind a disparity image (the purpose: VoxelMap.raycast's model disparity from the same camera and pose).
        disp int16 [h, w].  -> (image uint8 [h, w, 3] B, G, R, alpha uint8 [h, w], counts int32 [1] = pixels with alpha > 0) as numpy arrays,
        None for an output that was not asked for; raw=True returns the device tensors."""
        import torch
        cam = _camera(camera)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            d = _to_device(disp, torch.int16)
            if not isinstance(d, torch.Tensor) or d.dtype != torch.int16 or d.dim() != 2:
                raise EngineError("disp must be an int16 [h, w] image")
            h, w = int(d.shape[0]), int(d.shape[1])
            im = torch.empty((h, w, 3), dtype=torch.uint8, device=d.device)
            al = torch.empty((h, w), dtype=torch.uint8, device=d.device) if alpha else None
            n = torch.empty(1, dtype=torch.int32, device=d.device) if counts else None
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_voxel_color_render(self._h, C.byref(cam), _pose12(pose), *_pitched(d, 1), w, h, C.c_void_p(im.data_ptr()), 3 * w,
                                                      *([C.c_void_p(al.data_ptr()), w] if alpha else [None, 0]), C.c_void_p(n.data_ptr()) if counts else None, sp),
                    "cart_voxel_color_render")
        out = (im, al, n)
        if raw:
            return out
        if stream is not None:
            stream.synchronize()
        return tuple(t.cpu().numpy() if t is not None else None for t in out)

    def window(self):
        """-> ((ox, oy, oz), (cells_x, cells_y, cells_z), valid): the colour volume's own window, the map's as of the last integrate."""
        o, n, valid = (C.c_int64 * 3)(), (C.c_int32 * 3)(), C.c_int(0)
        self._check(self._lib.cart_voxel_color_window(self._h, o, n, C.byref(valid)), "cart_voxel_color_window")
        return tuple(o), tuple(n), bool(valid.value)

    def read(self):
        """-> (voxels VOXEL_RGB_DTYPE [cells_z, cells_y, cells_x] in window order, (ox, oy, oz)); synchronises."""
        voxels = np.empty((self.cells_z, self.cells_y, self.cells_x), VOXEL_RGB_DTYPE)
        o = (C.c_int64 * 3)()
        self._check(self._lib.cart_voxel_color_read(self._h, C.c_void_p(voxels.ctypes.data), o, _stream_ptr()), "cart_voxel_color_read")
        return voxels, tuple(o)

    def write(self, voxels, origin):
        """The counterpart of read(), as VoxelMap.write; synchronises."""
        v = np.ascontiguousarray(voxels, VOXEL_RGB_DTYPE)
        if v.shape != (self.cells_z, self.cells_y, self.cells_x):
            raise EngineError("voxels must be a VOXEL_RGB_DTYPE array of [cells_z, cells_y, cells_x]")
        o = (C.c_int64 * 3)(*[int(c) for c in origin])
        self._check(self._lib.cart_voxel_color_write(self._h, C.c_void_p(v.ctypes.data), o, _stream_ptr()), "cart_voxel_color_write")

    def clear(self):
        self._check(self._lib.cart_voxel_color_clear(self._h), "cart_voxel_color_clear")


def write_ply(path, vertices, quads, origin, voxel_size, colors=None):
    """A mesh of VoxelMap.mesh as a binary little-endian PLY file with quad faces and normals.  origin = the window origin (ox, oy, oz) in
    voxels: the positions are moved to the world frame, o_a voxel_size + p_a in fp64, before the conversion to float.  colors = the
    VOXEL_RGB_DTYPE array of VoxelColor.colorize, one record per vertex: the vertex element then carries uchar red, green, blue, alpha."""
    v = np.asarray(vertices, MESH_VERTEX_DTYPE).reshape(-1)
    q = np.asarray(quads, MESH_QUAD_DTYPE).reshape(-1)
    shift = np.array([int(c) for c in origin], np.float64) * np.float64(voxel_size)
    out = np.empty(len(v), np.dtype([("p", "<f4", 3), ("n", "<f4", 3)] + ([("c", "u1", 4)] if colors is not None else [])))
    out["p"] = (shift + v["position"].astype(np.float64)).astype(np.float32)
    out["n"] = v["normal"]
    if colors is not None:
        c = np.asarray(colors, VOXEL_RGB_DTYPE).reshape(-1)
        if len(c) != len(v):
            raise EngineError("colors must hold one record per vertex")
        out["c"] = np.stack([c["r"], c["g"], c["b"], c["weight"]], axis=1)
    faces = np.empty(len(q), np.dtype([("k", "u1"), ("v", "<i4", 4)]))
    faces["k"], faces["v"] = 4, q["v"]
    header = "ply\nformat binary_little_endian 1.0\ncomment cartslam voxel_map surface nets\nelement vertex %d\n" % len(v) + \
             "".join("property float %s\n" % c for c in ("x", "y", "z", "nx", "ny", "nz")) + \
             ("".join("property uchar %s\n" % c for c in ("red", "green", "blue", "alpha")) if colors is not None else "") + \
             "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(q)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(out.tobytes())
        f.write(faces.tobytes())


MODEL_TRACK_RESULT_DTYPE = np.dtype([("R", "<f8", 9), ("t", "<f8", 3), ("rms_initial", "<f8"), ("rms", "<f8"), ("status", "<i4"), ("n_candidates", "<i4"),
                                     ("n_initial", "<i4"), ("n_inliers", "<i4"), ("steps", "<i4"), ("reserved", "<i4")])   # cart_model_track_result


MODEL_TRACK_COLOR_RESULT_DTYPE = np.dtype(MODEL_TRACK_RESULT_DTYPE.descr + [("rms_photo_initial", "<f8"), ("rms_photo", "<f8"), ("cost_initial", "<f8"), ("cost", "<f8"),
                                                                            ("n_photo_initial", "<i4"), ("n_photo", "<i4")])   # cart_model_track_color_result


def model_track_params(**fields):
    """cart_model_track_default_params (spec S34; the defaults are build-owned and untuned) with the given fields replaced."""
    return _default_params(ModelTrackParams, "model_track", fields)


def model_track_color_params(**fields):
    """cart_model_track_color_default_params (spec S38; the defaults are build-owned and untuned) with the given fields replaced."""
    return _default_params(ModelTrackColorParams, "model_track_color", fields)


class ModelTrack(_DeviceObject):
    """Frame-to-model pose tracking against a VoxelMap (cart_model_track_* in the C ABI, spec S34 in DESIGN.md 7.16): Gauss-Newton on the
    camera-to-world pose over the frame's back-projected pixels, which should lie on the volume's zero level set, for frames of up to
    max_width x max_height.  Reads the volume only.  A context manager; close() destroys the device object."""
    _name = "model_track"

    def __init__(self, engine, max_width, max_height):
        self.max_width, self.max_height = int(max_width), int(max_height)
        super().__init__(engine, self.max_width, self.max_height)

    def refine(self, voxel_map, camera, pose0, disp, params=None, mask=None, stream=None, raw=False):
        """voxel_map = the VoxelMap to track against; camera = EgoCamera or (fx, fy, cx, cy, baseline); pose0 = 12 numbers, the 3 x 4
        camera-to-world pose to refine (host); disp int16 [h, w] (x16), mask uint8 [h, w] (motion_segment's labels) or None: device tensors
        are taken as they are (rows may be pitched), host arrays go up.  stream = a torch stream (default: the current one).  -> the result
        as a MODEL_TRACK_RESULT_DTYPE array of one record (host); raw=True returns the device tensor (136 bytes as float64) with no host
        round trip."""
        import torch
        cam = _camera(camera)
        p = params if params is not None else model_track_params()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # uploads and the result's allocation on the call's stream
            d, mk = _to_device(disp, torch.int16), _to_device(mask, torch.uint8)
            if not isinstance(d, torch.Tensor) or d.dtype != torch.int16 or d.dim() != 2:
                raise EngineError("disp must be an int16 [h, w] image")
            if mk is not None:
                _check_frame_image(mk, torch.uint8, "mask", d)
            res = torch.empty(MODEL_TRACK_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device=d.device)   # every byte is written by the call
        h, w = int(d.shape[0]), int(d.shape[1])
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_model_track_refine(self._h, voxel_map._h, C.byref(cam), _pose12(pose0), C.byref(p), *_pitched(d, 1), *_pitched(mk, 1), w, h,
                                                      C.c_void_p(res.data_ptr()), sp), "cart_model_track_refine")
        if raw:
            return res
        if stream is not None:
            stream.synchronize()
        return res.cpu().numpy().view(MODEL_TRACK_RESULT_DTYPE).reshape(-1)

    def refine_color(self, voxel_map, voxel_color, camera, pose0, disp, image, params=None, color_params=None, mask=None, stream=None, raw=False):
        """refine() with a photometric term (cart_model_track_refine_color, spec S38 in DESIGN.md 7.20): voxel_color = the VoxelColor of
        voxel_map, image = the frame's uint8 [h, w] (gray) or [h, w, 3] (B, G, R) image, color_params = model_track_color_params(...).
        Reads both volumes only.  -> the result as a MODEL_TRACK_COLOR_RESULT_DTYPE array of one record (host); raw=True returns the
        device tensor (176 bytes as float64) with no host round trip."""
        import torch
        cam = _camera(camera)
        p = params if params is not None else model_track_params()
        cp = color_params if color_params is not None else model_track_color_params()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # uploads and the result's allocation on the call's stream
            d, im, mk = _to_device(disp, torch.int16), _to_device(image, torch.uint8), _to_device(mask, torch.uint8)
            if not isinstance(d, torch.Tensor) or d.dtype != torch.int16 or d.dim() != 2:
                raise EngineError("disp must be an int16 [h, w] image")
            if not isinstance(im, torch.Tensor) or im.dim() not in (2, 3):
                raise EngineError("image must be a uint8 [h, w] or [h, w, 3] image")
            channels = int(im.shape[2]) if im.dim() == 3 else 1
            _check_frame_image(im, torch.uint8, "image", d, channels if im.dim() == 3 else None)
            if mk is not None:
                _check_frame_image(mk, torch.uint8, "mask", d)
            res = torch.empty(MODEL_TRACK_COLOR_RESULT_DTYPE.itemsize // 8, dtype=torch.float64, device=d.device)   # every byte is written by the call
        h, w = int(d.shape[0]), int(d.shape[1])
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_model_track_refine_color(self._h, voxel_map._h, voxel_color._h, C.byref(cam), _pose12(pose0), C.byref(p), C.byref(cp), *_pitched(d, 1),
                                                            *_pitched(im, im.dim() - 1), channels, *_pitched(mk, 1), w, h, C.c_void_p(res.data_ptr()), sp),
                    "cart_model_track_refine_color")
        if raw:
            return res
        if stream is not None:
            stream.synchronize()
        return res.cpu().numpy().view(MODEL_TRACK_COLOR_RESULT_DTYPE).reshape(-1)


OBJECT_DTYPE = np.dtype([("component", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("median_bin", "<i4"), ("n_hist", "<i4"),
                         ("n_points", "<i4"), ("n_flow", "<i4"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("sum", "<i8", 3), ("flow_sum", "<i8", 3),
                         ("centroid", "<f8", 3), ("velocity", "<f8", 3), ("extent", "<f8", 3), ("valid", "<i4"), ("has_velocity", "<i4")])   # cart_object
TRACK_DTYPE = np.dtype([("id", "<u4"), ("state", "<i4"), ("age", "<i4"), ("missed", "<i4"), ("object", "<i4"), ("component", "<i4"),
                        ("position", "<f8", 3), ("velocity", "<f8", 3), ("extent", "<f8", 3)])   # cart_track


def object_params(**fields):
    """cart_object_default_params (spec S31; the defaults are build-owned and untuned) with the given fields replaced."""
    return _default_params(ObjectParams, "object", fields)


ObjectTracks = collections.namedtuple("ObjectTracks", "objects tracks counts")


class ObjectTracker(_DeviceObject):
    """Moving objects and their tracks from the motion components (cart_object_tracker_* in the C ABI, spec S31 in DESIGN.md 7.13): every
    MOVING component of plane_ccl_table(motion labels) that is large enough, measured in metres and followed from frame to frame, for
    frames of up to max_width x max_height.  A context manager; close() destroys the device object."""
    _name = "object_tracker"

    def __init__(self, engine, max_width, max_height, max_objects=64, max_tracks=64):
        self.max_width, self.max_height, self.max_objects, self.max_tracks = int(max_width), int(max_height), int(max_objects), int(max_tracks)
        super().__init__(engine, self.max_width, self.max_height, self.max_objects, self.max_tracks)

    def reset(self, stream=None):
        """Frees every track; the next new track gets id 1."""
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_object_tracker_reset(self._h, sp), "cart_object_tracker_reset")

    def update(self, camera, rel, pose, ids, table, n_components, disp_cur, disp_prev, flow, params=None, raw=False, stream=None):
        """camera = EgoCamera or (fx, fy, cx, cy, baseline); rel = 12 numbers, the 3 x 4 (R | t) with p_cur = R p_prev + t, pose = 12 numbers,
        this frame's camera-to-world (both host); ids int32 [h, w], table int32 [max_components, 7] and n_components int32 [1] (or an int)
        as Engine.plane_ccl_table gives them for one frame of motion labels; disp_cur / disp_prev int16 [h, w] (x16), flow int16 [h, w, 2]
        (S10.5).  Device tensors are taken as they are (rows may be pitched), host arrays go up.  stream = a torch stream (default: the
        current one).  -> ObjectTracks(objects OBJECT_DTYPE [max_objects], tracks TRACK_DTYPE [max_tracks], counts int32 [8]) as numpy
        arrays; raw=True returns the device tensors (float64 views of the records) with no host round trip."""
        import torch
        cam = _camera(camera)
        p = params if params is not None else object_params()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):   # uploads and allocations on the call's stream
            if isinstance(n_components, (int, np.integer)):
                n_components = np.array([n_components], np.int32)
            idt, tb, nc = _to_device(ids, torch.int32), _to_device(table, torch.int32), _to_device(n_components, torch.int32)
            dc, dp, fl = _to_device(disp_cur, torch.int16), _to_device(disp_prev, torch.int16), _to_device(flow, torch.int16)
            if not isinstance(dc, torch.Tensor) or dc.dim() != 2:
                raise EngineError("disp_cur must be an int16 [h, w] image")
            objects = torch.empty(self.max_objects * OBJECT_DTYPE.itemsize // 8, dtype=torch.float64, device=dc.device)   # every byte is written by the call
            tracks = torch.empty(self.max_tracks * TRACK_DTYPE.itemsize // 8, dtype=torch.float64, device=dc.device)
            counts = torch.empty(8, dtype=torch.int32, device=dc.device)
        for t, dtype, what, channels in ((dc, torch.int16, "disp_cur", None), (idt, torch.int32, "ids", None), (dp, torch.int16, "disp_prev", None), (fl, torch.int16, "flow", 2)):
            _check_frame_image(t, dtype, what, dc, channels)
        if not isinstance(tb, torch.Tensor) or tb.dtype != torch.int32 or not tb.is_cuda or not tb.is_contiguous() or tb.numel() < 7 or tb.numel() % 7:
            raise EngineError("table must be a contiguous device tensor of int32 rows of 7")
        if not isinstance(nc, torch.Tensor) or nc.dtype != torch.int32 or not nc.is_cuda or nc.numel() < 1:
            raise EngineError("n_components must be an int or a device tensor of int32")
        h, w = int(dc.shape[0]), int(dc.shape[1])
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else _stream_ptr()
        self._check(self._lib.cart_object_tracker_update(self._h, C.byref(cam), _pose12(rel), _pose12(pose), C.byref(p), *_pitched(idt, 1), C.c_void_p(tb.data_ptr()),
                                                         tb.numel() // 7, C.c_void_p(nc.data_ptr()), *_pitched(dc, 1), *_pitched(dp, 1), *_pitched(fl, 2), w, h,
                                                         C.c_void_p(objects.data_ptr()), C.c_void_p(tracks.data_ptr()), C.c_void_p(counts.data_ptr()), sp),
                    "cart_object_tracker_update")
        out = ObjectTracks(objects, tracks, counts)
        if raw:
            return out
        if stream is not None:
            stream.synchronize()
        return ObjectTracks(objects.cpu().numpy().view(OBJECT_DTYPE), tracks.cpu().numpy().view(TRACK_DTYPE), counts.cpu().numpy())


def plane_cluster(planes, offsets, neighbours):
    """S18 on the host (cart_plane_cluster): planes f64 [L+1, 4], adjacency CSR -> (planes [k, 4], assignments uint64 [L+1])."""
    lib = _lib.load()
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    nb = np.ascontiguousarray(neighbours, dtype=np.int32)
    if nb.size == 0:
        nb = np.zeros(1, np.int32)
    L1 = planes.shape[0]
    out = np.zeros((L1, 4), np.float64)
    assign = np.zeros(L1, np.uint64)
    n = C.c_int(0)
    rc = lib.cart_plane_cluster(planes.ctypes.data_as(C.c_void_p), L1 - 1, off.ctypes.data_as(C.c_void_p), nb.ctypes.data_as(C.c_void_p),
                                out.ctypes.data_as(C.c_void_p), assign.ctypes.data_as(C.c_void_p), C.byref(n))
    if rc != 0:
        raise EngineError("cart_plane_cluster: " + lib.cart_last_error(None).decode())
    return out[:n.value], assign


def resize_linear(img, dst_width, dst_height):
    """cv::cuda::resize(..., INTER_LINEAR) of the KITTI source (cart_resize_linear): uint8 CUDA [h,w] or [h,w,3] -> [dh,dw(,3)]."""
    import torch
    lib = _lib.load()
    ch = 3 if img.dim() == 3 else 1
    _, sp, ss, _ = _geom(img, 2 if ch == 3 else 1)
    sh, sw = img.shape[:2]
    out = torch.empty((dst_height, dst_width, 3) if ch == 3 else (dst_height, dst_width), dtype=torch.uint8, device=img.device)
    _, dp, ds, _ = _geom(out, 2 if ch == 3 else 1)
    rc = lib.cart_resize_linear(img.device.index or 0, sp, ss, sw, sh, ch, dp, ds, dst_width, dst_height, _stream_ptr())
    if rc != 0:
        raise EngineError("cart_resize_linear: " + lib.cart_last_error(None).decode())
    return out


def uniq_table(uniqueness_ratio, engine=None):
    """Integer uniqueness thresholds T(best) for best = 0..2047 (cart_debug_uniq_table): from the GPU when an engine is
    given, from the host-compiled copy of the same function otherwise."""
    lib = _lib.load()
    out = np.empty(2048, np.uint16)
    rc = lib.cart_debug_uniq_table(engine._h if engine is not None else None, int(uniqueness_ratio), out.ctypes.data_as(C.POINTER(C.c_uint16)))
    if rc != 0:
        raise EngineError("cart_debug_uniq_table: " + lib.cart_last_error(None).decode())
    return out


def find_plane_params(hist256, params=None):
    """HOST: reference HistogramPeakPlaneParameterProvider::updatePlaneParameters (planeseg.cu:405-458).
    -> (updated: bool, PlaneParams)."""
    lib = _lib.load()
    h = np.ascontiguousarray(np.asarray(hist256, dtype=np.int32).reshape(256))
    p = PlaneParams(*(params.as_tuple() if isinstance(params, PlaneParams) else (params or (0,) * 6)))
    rc = lib.cart_find_plane_params(h.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(p))
    if rc < 0:
        raise EngineError("cart_find_plane_params: " + lib.cart_last_error(None).decode())
    return bool(rc), p


def find_peaks(data):
    """HOST: reference util::findPeaks (src/utils/peaks.cpp:12-72) -> list of (born, died, left, right)."""
    lib = _lib.load()
    d = np.ascontiguousarray(np.asarray(data, dtype=np.int32).ravel())
    n = d.size
    arrs = [(C.c_int * n)() for _ in range(4)]
    k = lib.cart_find_peaks(d.ctypes.data_as(C.POINTER(C.c_int32)), n, *arrs)
    if k < 0:
        raise EngineError("cart_find_peaks: " + lib.cart_last_error(None).decode())
    return [tuple(a[i] for a in arrs) for i in range(k)]

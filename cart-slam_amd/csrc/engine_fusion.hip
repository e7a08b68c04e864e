// engine_fusion.hip -- C ABI of the temporal disparity fusion (include/cart_engine.h): argument checks and the cart_fusion
// device object, which owns the z-buffer and the counters.  Both are zeroed once here and left all zero by every call (the fuse kernel
// writes back the zeros it found), so the call path has no clear launch and no hipMemset.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

struct cart_fusion : SizedObject {
    using SizedObject::SizedObject;
    uint32_t *zbuf = nullptr;      // [max_height * max_width]; a call uses the first width * height keys
    int32_t *counters = nullptr;   // [kFusionCounters]
};

void cart_fusion_default_params(cart_fusion_params *p) {
    if (!p) return;
    *p = cart_fusion_params{1.0, 1.0, 0.75, 4, 2};
}

int cart_fusion_create(cart_engine *e, int max_width, int max_height, cart_fusion **out) {
    if (check_max_size(max_width, max_height)) return -1;
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_fusion *f = new (std::nothrow) cart_fusion(e, max_width, max_height);
    if (!f) return fail("out of host memory");
    const size_t zbytes = (size_t)max_width * max_height * sizeof(uint32_t);
    if (f->alloc(&f->zbuf, zbytes) || f->alloc(&f->counters, kFusionCounters * sizeof(int32_t)) || f->create_event() ||
        hipMemset(f->zbuf, 0, zbytes) != hipSuccess || hipMemset(f->counters, 0, kFusionCounters * sizeof(int32_t)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {   // the zeros are in place before any stream can use the object
        destroy_object(f);
        return fail("allocating the fusion workspaces failed");
    }
    *out = f;
    return 0;
}

void cart_fusion_destroy(cart_fusion *f) { destroy_object(f); }

int cart_fusion_update(cart_fusion *f, const cart_ego_camera *cam, const double *rel, const cart_fusion_params *p, const int16_t *disp_cur,
                       size_t disp_cur_step, const int16_t *prev_disp, size_t prev_disp_step, const uint8_t *prev_age, size_t prev_age_step,
                       const uint8_t *mask_prev, size_t mask_prev_step, const uint8_t *mask_cur, size_t mask_cur_step, int w, int h, int16_t *fused,
                       size_t fused_step, uint8_t *age, size_t age_step, uint8_t *source, size_t source_step, int32_t *counts, void *stream_) {
    if (!p) return fail("params is NULL");
    if (check_positive("min_disparity", p->min_disparity) || check_positive("agree_threshold", p->agree_threshold)) return -1;
    if (!(p->splat_radius >= 0.5 && p->splat_radius < 1.0)) return fail("splat_radius must be in [0.5, 1)");
    if (p->max_weight < 1 || p->max_weight > 255) return fail("max_weight must be in [1, 255]");
    if (p->min_age < 1 || p->min_age > 255) return fail("min_age must be in [1, 255]");
    if (check_camera(cam)) return -1;
    if (!rel && (prev_disp || prev_age)) return fail("rel is NULL although a previous frame is given");
    if (rel && check_pose("rel", rel)) return -1;
    if (check_frame_size(w, h)) return -1;
    if (!f) return fail("bad arguments");
    if (f->check_fits(w, h)) return -1;
    if (!disp_cur) return fail("disp_cur is NULL");
    if ((prev_disp == nullptr) != (prev_age == nullptr)) return fail("prev_disp and prev_age must be given together");
    if (!fused) return fail("fused is NULL");
    if (!age) return fail("age is NULL");
    if (!prev_disp) mask_prev = nullptr;   // nothing is projected: not read
    const auto image = [&](const char *name, const void *ptr, size_t step, size_t elem) { return Extent::image(name, ptr, step, elem, w, h); };
    // the inputs, then the outputs: an output is checked against everything before it
    const Extent all[] = {image("disp_cur", disp_cur, disp_cur_step, 2), image("prev_disp", prev_disp, prev_disp_step, 2), image("prev_age", prev_age, prev_age_step, 1),
                          image("mask_prev", mask_prev, mask_prev_step, 1), image("mask_cur", mask_cur, mask_cur_step, 1), image("fused", fused, fused_step, 2),
                          image("age", age, age_step, 1), image("source", source, source_step, 1), Extent{"counts", counts, 20, 4, 20, 1}};
    constexpr int kInputs = 5, kAll = 9;
    for (int i = 0; i < kAll - 1; ++i)
        if (all[i].ptr && check_pitched(all[i])) return -1;
    if (all[kAll - 1].begin() % 4) return fail("counts must be 4-byte aligned");   // not pitched: its own wording
    // No output may overlap another buffer: the fuse kernel writes its pixels while other workgroups still read theirs, and two outputs
    // in one place would hold whichever store came last.
    if (check_outputs_apart(all, kInputs, kAll)) return -1;

    FusionArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam = *cam; a.p = *p;
    if (rel) std::memcpy(a.rel, rel, sizeof(a.rel));
    a.disp_cur = disp_cur; a.disp_cur_step = disp_cur_step; a.prev_disp = prev_disp; a.prev_disp_step = prev_disp_step;
    a.prev_age = prev_age; a.prev_age_step = prev_age_step; a.mask_prev = mask_prev; a.mask_prev_step = mask_prev_step;
    a.mask_cur = mask_cur; a.mask_cur_step = mask_cur_step; a.fused = fused; a.fused_step = fused_step; a.age = age; a.age_step = age_step;
    a.source = source; a.source_step = source_step; a.counts = counts; a.zbuf = f->zbuf; a.counters = f->counters; a.w = w; a.h = h;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*f, stream);
    if (call.begin()) return -1;
    if (prev_disp) launch_fusion_splat(a, stream);
    launch_fusion_fuse(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// engine_fusion.hip -- C ABI of the temporal disparity fusion (include/cart_engine.h): argument checks and the cart_fusion
// device object, which owns the z-buffer and the counters.  Both are zeroed once here and left all zero by every call (the fuse kernel
// writes back the zeros it found), so the call path has no clear launch and no hipMemset.

#include "engine_host.h"

using namespace cart_amd;

namespace {

struct Extent {   // one device argument, for the checks: `rows` rows of `row_bytes`, `step` apart
    const char *name;
    const void *ptr;
    size_t step, elem, row_bytes;
    int rows;
    uintptr_t begin() const { return reinterpret_cast<uintptr_t>(ptr); }
    uintptr_t end() const { return begin() + (size_t)(rows - 1) * step + row_bytes; }
};

bool overlap(const Extent &a, const Extent &b) { return a.begin() < b.end() && b.begin() < a.end(); }

}  // namespace

extern "C" {

struct cart_fusion : DeviceObject {
    using DeviceObject::DeviceObject;
    int max_width = 0, max_height = 0;
    uint32_t *zbuf = nullptr;      // [max_height * max_width]; a call uses the first width * height keys
    int32_t *counters = nullptr;   // [kFusionCounters]
};

void cart_fusion_default_params(cart_fusion_params *p) {
    if (!p) return;
    *p = cart_fusion_params{1.0, 1.0, 0.75, 4, 2};
}

int cart_fusion_create(cart_engine *e, int max_width, int max_height, cart_fusion **out) {
    if (max_width < 1 || max_width > 16384) return fail("max_width must be in [1, 16384]");
    if (max_height < 1 || max_height > 16384) return fail("max_height must be in [1, 16384]");
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_fusion *f = new (std::nothrow) cart_fusion(e);
    if (!f) return fail("out of host memory");
    f->max_width = max_width;
    f->max_height = max_height;
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
    if (!(p->min_disparity > 0) || !std::isfinite(p->min_disparity)) return fail("min_disparity must be a positive number");
    if (!(p->agree_threshold > 0) || !std::isfinite(p->agree_threshold)) return fail("agree_threshold must be a positive number");
    if (!(p->splat_radius >= 0.5 && p->splat_radius < 1.0)) return fail("splat_radius must be in [0.5, 1)");
    if (p->max_weight < 1 || p->max_weight > 255) return fail("max_weight must be in [1, 255]");
    if (p->min_age < 1 || p->min_age > 255) return fail("min_age must be in [1, 255]");
    if (check_camera(cam)) return -1;
    if (!rel && (prev_disp || prev_age)) return fail("rel is NULL although a previous frame is given");
    for (int k = 0; rel && k < 12; ++k) {
        const double bound = k % 4 == 3 ? 1e6 : 2.0;
        if (!std::isfinite(rel[k]) || std::fabs(rel[k]) > bound)
            return fail("rel[" + std::to_string(k) + "] must be finite and within " + (k % 4 == 3 ? "1e6 (translation)" : "2 (rotation)"));
    }
    if (w < 1 || w > 16384) return fail("width must be in [1, 16384]");
    if (h < 1 || h > 16384) return fail("height must be in [1, 16384]");
    if (f && (w > f->max_width || h > f->max_height))
        return fail("width x height exceeds the object's " + std::to_string(f->max_width) + " x " + std::to_string(f->max_height));
    if (!f) return fail("bad arguments");
    if (!disp_cur) return fail("disp_cur is NULL");
    if ((prev_disp == nullptr) != (prev_age == nullptr)) return fail("prev_disp and prev_age must be given together");
    if (!fused) return fail("fused is NULL");
    if (!age) return fail("age is NULL");
    if (!prev_disp) mask_prev = nullptr;   // nothing is projected: not read
    const auto image = [&](const char *name, const void *ptr, size_t step, size_t elem) { return Extent{name, ptr, step, elem, (size_t)w * elem, h}; };
    // the inputs, then the outputs: an output is checked against everything before it
    const Extent all[] = {image("disp_cur", disp_cur, disp_cur_step, 2), image("prev_disp", prev_disp, prev_disp_step, 2), image("prev_age", prev_age, prev_age_step, 1),
                          image("mask_prev", mask_prev, mask_prev_step, 1), image("mask_cur", mask_cur, mask_cur_step, 1), image("fused", fused, fused_step, 2),
                          image("age", age, age_step, 1), image("source", source, source_step, 1), Extent{"counts", counts, 20, 4, 20, 1}};
    constexpr int kInputs = 5, kAll = 9;
    for (const Extent &x : all) {
        if (!x.ptr) continue;
        const bool is_counts = &x == &all[kAll - 1];
        if (is_counts) {
            if (x.begin() % 4) return fail("counts must be 4-byte aligned");
            continue;
        }
        if ((x.begin() % x.elem) || (x.step % x.elem)) return fail(std::string(x.name) + " and its step must be " + std::to_string(x.elem) + "-byte aligned");
        if (x.step < x.row_bytes) return fail(std::string(x.name) + "_step is below the row size");
    }
    // No output may overlap another buffer: the fuse kernel writes its pixels while other workgroups still read theirs, and two outputs
    // in one place would hold whichever store came last.
    for (int i = kInputs; i < kAll; ++i)
        for (int j = 0; all[i].ptr && j < i; ++j)
            if (all[j].ptr && overlap(all[j], all[i])) return fail(std::string(all[j].name) + " and " + all[i].name + " must not overlap");

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

// engine_motion.hip -- C ABI of the motion segmentation (include/cart_engine.h): argument checks and the two launches.
// Stateless: every buffer is the caller's, so there is no device object and no workspace.

#include "engine_host.h"

using namespace cart_amd;

namespace {

struct Image {   // one pitched argument, for the checks
    const char *name;
    const void *ptr;
    size_t step, elem;   // elem = bytes per pixel = the alignment of the pointer and the step
    uintptr_t begin() const { return reinterpret_cast<uintptr_t>(ptr); }
    uintptr_t end(int w, int h) const { return begin() + (size_t)(h - 1) * step + (size_t)w * elem; }
};

int check_image(const Image &im, int w) {
    if ((im.begin() % im.elem) || (im.step % im.elem)) return fail(std::string(im.name) + " and its step must be " + std::to_string(im.elem) + "-byte aligned");
    if (im.step < (size_t)w * im.elem) return fail(std::string(im.name) + "_step is below the row size");
    return 0;
}

bool overlap(const Image &a, const Image &b, int w, int h) { return a.begin() < b.end(w, h) && b.begin() < a.end(w, h); }

}  // namespace

extern "C" {

void cart_motion_default_params(cart_motion_params *p) {
    if (!p) return;
    *p = cart_motion_params{1.0, 2.0, 1.0, 2, 50};
}

int cart_motion_segment(cart_engine *e, const cart_ego_camera *cam, const double *rel, const cart_motion_params *p, const int16_t *disp_cur,
                        size_t disp_cur_step, const int16_t *disp_prev, size_t disp_prev_step, const int16_t *flow, size_t flow_step, int w, int h,
                        int16_t *residual, size_t residual_step, uint8_t *raw, size_t raw_step, uint8_t *labels, size_t labels_step, const uint8_t *planes,
                        size_t planes_step, uint8_t *planes_static, size_t planes_static_step, void *stream_) {
    if (!p) return fail("params is NULL");
    if (!(p->min_disparity > 0) || !std::isfinite(p->min_disparity)) return fail("min_disparity must be a positive number");
    if (!(p->flow_threshold > 0) || !std::isfinite(p->flow_threshold)) return fail("flow_threshold must be a positive number");
    if (!(p->disparity_threshold > 0) || !std::isfinite(p->disparity_threshold)) return fail("disparity_threshold must be a positive number");
    if (p->radius < 0 || p->radius > kMotionMaxRadius) return fail("radius must be in [0, 4]");
    if (p->support_percent < 1 || p->support_percent > 100) return fail("support_percent must be in [1, 100]");
    if (check_camera(cam)) return -1;
    if (!rel) return fail("rel is NULL");
    for (int k = 0; k < 12; ++k) {
        const double bound = k % 4 == 3 ? 1e6 : 2.0;
        if (!std::isfinite(rel[k]) || std::fabs(rel[k]) > bound)
            return fail("rel[" + std::to_string(k) + "] must be finite and within " + (k % 4 == 3 ? "1e6 (translation)" : "2 (rotation)"));
    }
    if (w < 1 || w > 16384) return fail("width must be in [1, 16384]");
    if (h < 1 || h > 16384) return fail("height must be in [1, 16384]");
    if (!e) return fail("bad arguments");
    const Image in[] = {{"disp_cur", disp_cur, disp_cur_step, 2}, {"disp_prev", disp_prev, disp_prev_step, 2}, {"flow", flow, flow_step, 4},
                        {"raw", raw, raw_step, 1}, {"labels", labels, labels_step, 1}};
    const Image res{"residual", residual, residual_step, 8}, pl{"planes", planes, planes_step, 1}, ps{"planes_static", planes_static, planes_static_step, 1};
    for (const Image &im : in)
        if (!im.ptr) return fail(std::string(im.name) + " is NULL");
    if ((planes == nullptr) != (planes_static == nullptr)) return fail("planes and planes_static must be given together");
    for (const Image &im : in)
        if (check_image(im, w)) return -1;
    if (residual && check_image(res, w)) return -1;
    if (planes && (check_image(pl, w) || check_image(ps, w))) return -1;
    // No output may overlap another buffer: the filter reads `raw` and `planes` beside the pixels other blocks write, the residual kernel gathers
    // from `disp_prev` anywhere, and two outputs in one place would hold whichever store came last.
    const Image *all[] = {&in[0], &in[1], &in[2], planes ? &pl : nullptr, residual ? &res : nullptr, &in[3], &in[4], planes ? &ps : nullptr};
    for (int i = 4; i < 8; ++i)   // the outputs, each against everything before it
        for (int j = 0; all[i] && j < i; ++j)
            if (all[j] && overlap(*all[j], *all[i], w, h)) return fail(std::string(all[j]->name) + " and " + all[i]->name + " must not overlap");

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(e->params.device_id));
    MotionArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam = *cam; a.p = *p;
    std::memcpy(a.rel, rel, sizeof(a.rel));
    a.disp_cur = disp_cur; a.disp_cur_step = disp_cur_step; a.disp_prev = disp_prev; a.disp_prev_step = disp_prev_step;
    a.flow = flow; a.flow_step = flow_step; a.residual = residual; a.residual_step = residual_step;
    a.raw = raw; a.raw_step = raw_step; a.labels = labels; a.labels_step = labels_step;
    a.planes = planes; a.planes_step = planes_step; a.planes_static = planes_static; a.planes_static_step = planes_static_step;
    a.w = w; a.h = h;
    launch_motion_residual(a, stream);
    launch_motion_filter(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// engine_motion.hip -- C ABI of the motion segmentation (include/cart_engine.h): argument checks and the two launches.
// Stateless: every buffer is the caller's, so there is no device object and no workspace.

#include "engine_host.h"

using namespace cart_amd;

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
    if (check_positive("min_disparity", p->min_disparity) || check_positive("flow_threshold", p->flow_threshold) ||
        check_positive("disparity_threshold", p->disparity_threshold))
        return -1;
    if (p->radius < 0 || p->radius > kMotionMaxRadius) return fail("radius must be in [0, 4]");
    if (p->support_percent < 1 || p->support_percent > 100) return fail("support_percent must be in [1, 100]");
    if (check_camera(cam) || check_pose("rel", rel) || check_frame_size(w, h)) return -1;
    if (!e) return fail("bad arguments");
    const auto image = [&](const char *name, const void *ptr, size_t step, size_t elem) { return Extent::image(name, ptr, step, elem, w, h); };
    // the inputs, then the outputs from kOutputs on: an output is checked against everything before it
    enum { kDispCur, kDispPrev, kFlow, kPlanes, kResidual, kRaw, kLabels, kPlanesStatic, kAll, kOutputs = kResidual };
    const Extent all[] = {image("disp_cur", disp_cur, disp_cur_step, 2), image("disp_prev", disp_prev, disp_prev_step, 2), image("flow", flow, flow_step, 4),
                          image("planes", planes, planes_step, 1), image("residual", residual, residual_step, 8), image("raw", raw, raw_step, 1),
                          image("labels", labels, labels_step, 1), image("planes_static", planes_static, planes_static_step, 1)};
    static_assert(sizeof(all) / sizeof(all[0]) == kAll, "one entry per index");
    for (int i : {kDispCur, kDispPrev, kFlow, kRaw, kLabels})   // the required ones
        if (!all[i].ptr) return fail(std::string(all[i].name) + " is NULL");
    if ((planes == nullptr) != (planes_static == nullptr)) return fail("planes and planes_static must be given together");
    for (int i : {kDispCur, kDispPrev, kFlow, kRaw, kLabels, kResidual, kPlanes, kPlanesStatic})   // the required ones first, then the optional ones given
        if (all[i].ptr && check_pitched(all[i])) return -1;
    // No output may overlap another buffer: the filter reads `raw` and `planes` beside the pixels other blocks write, the residual kernel gathers
    // from `disp_prev` anywhere, and two outputs in one place would hold whichever store came last.
    if (check_outputs_apart(all, kOutputs, kAll)) return -1;

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

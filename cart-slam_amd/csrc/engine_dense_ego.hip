// engine_dense_ego.hip -- C ABI of the dense ego-motion refinement (include/cart_engine.h): argument checks and the
// cart_dense_ego device object, which owns the row partials and the pose state of a call.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

struct cart_dense_ego : SizedObject {
    using SizedObject::SizedObject;
    double *partial = nullptr;          // [kDenseWords][max_height]
    DenseEgoState *state = nullptr;
};

void cart_dense_ego_default_params(cart_dense_ego_params *p) {
    if (!p) return;
    *p = cart_dense_ego_params{1.0, 2.0, 1.0, 1.0, 4, 1, 1024};
}

int cart_dense_ego_create(cart_engine *e, int max_width, int max_height, cart_dense_ego **out) {
    if (check_max_size(max_width, max_height)) return -1;
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_dense_ego *g = new (std::nothrow) cart_dense_ego(e, max_width, max_height);
    if (!g) return fail("out of host memory");
    if (g->alloc(&g->partial, (size_t)kDenseWords * max_height * sizeof(double)) || g->alloc(&g->state, sizeof(DenseEgoState)) || g->create_event()) {
        destroy_object(g);
        return fail("allocating the dense ego-motion workspaces failed");
    }
    *out = g;
    return 0;
}

void cart_dense_ego_destroy(cart_dense_ego *g) { destroy_object(g); }

int cart_dense_ego_refine(cart_dense_ego *g, const cart_ego_camera *cam, const double *rel0, const cart_dense_ego_params *p, const int16_t *disp_cur,
                          size_t disp_cur_step, const int16_t *disp_prev, size_t disp_prev_step, const int16_t *flow, size_t flow_step,
                          const uint8_t *mask, size_t mask_step, int w, int h, cart_dense_ego_result *result, void *stream_) {
    if (!p) return fail("params is NULL");
    if (check_positive("min_disparity", p->min_disparity) || check_positive("flow_threshold", p->flow_threshold) ||
        check_positive("disparity_threshold", p->disparity_threshold))
        return -1;
    if (!(p->disparity_weight >= 0) || !std::isfinite(p->disparity_weight)) return fail("disparity_weight must be a number that is not negative");
    if (p->iterations < 0 || p->iterations > CART_DENSE_EGO_MAX_ITERATIONS) return fail("iterations must be in [0, 16]");
    if (p->stride < 1 || p->stride > 16) return fail("stride must be in [1, 16]");
    if (p->min_inliers < 6 || p->min_inliers > (1 << 30)) return fail("min_inliers must be in [6, 2^30]");
    if (check_camera(cam) || check_pose("rel0", rel0) || check_frame_size(w, h)) return -1;
    if (!g) return fail("bad arguments");
    if (g->check_fits(w, h)) return -1;
    const Extent in[] = {Extent::image("disp_cur", disp_cur, disp_cur_step, 2, w, h), Extent::image("disp_prev", disp_prev, disp_prev_step, 2, w, h),
                         Extent::image("flow", flow, flow_step, 4, w, h), Extent::image("mask", mask, mask_step, 1, w, h)};
    for (const Extent &im : in)
        if (!im.ptr && &im != &in[3]) return fail(std::string(im.name) + " is NULL");
    if (!result) return fail("result is NULL");
    const Extent res{"result", result, sizeof(cart_dense_ego_result), 8, sizeof(cart_dense_ego_result), 1};
    for (const Extent &im : in) {
        if (!im.ptr) continue;
        if (check_pitched(im)) return -1;
        if (overlap(res, im)) return fail(std::string("result and ") + im.name + " must not overlap");   // the output is named first here
    }
    if (res.begin() % 8) return fail("result must be 8-byte aligned");

    DenseEgoArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam = *cam; a.p = *p;
    std::memcpy(a.rel0, rel0, sizeof(a.rel0));
    a.disp_cur = disp_cur; a.disp_cur_step = disp_cur_step; a.disp_prev = disp_prev; a.disp_prev_step = disp_prev_step;
    a.flow = flow; a.flow_step = flow_step; a.mask = mask; a.mask_step = mask_step;
    a.w = w; a.h = h;
    a.ni = (w + p->stride - 1) / p->stride; a.nj = (h + p->stride - 1) / p->stride;
    a.rows_cap = g->max_height; a.partial = g->partial; a.state = g->state; a.result = result;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*g, stream);
    if (call.begin()) return -1;
    launch_dense_ego(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

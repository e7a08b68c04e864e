// engine_dense_ego.hip -- C ABI of the dense ego-motion refinement (include/cart_engine.h): argument checks and the
// cart_dense_ego device object, which owns the row partials and the pose state of a call.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

struct cart_dense_ego : DeviceObject {
    using DeviceObject::DeviceObject;
    int max_width = 0, max_height = 0;
    double *partial = nullptr;          // [kDenseWords][max_height]
    DenseEgoState *state = nullptr;
};

void cart_dense_ego_default_params(cart_dense_ego_params *p) {
    if (!p) return;
    *p = cart_dense_ego_params{1.0, 2.0, 1.0, 1.0, 4, 1, 1024};
}

int cart_dense_ego_create(cart_engine *e, int max_width, int max_height, cart_dense_ego **out) {
    if (max_width < 1 || max_width > 16384) return fail("max_width must be in [1, 16384]");
    if (max_height < 1 || max_height > 16384) return fail("max_height must be in [1, 16384]");
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_dense_ego *g = new (std::nothrow) cart_dense_ego(e);
    if (!g) return fail("out of host memory");
    g->max_width = max_width;
    g->max_height = max_height;
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
    if (!(p->min_disparity > 0) || !std::isfinite(p->min_disparity)) return fail("min_disparity must be a positive number");
    if (!(p->flow_threshold > 0) || !std::isfinite(p->flow_threshold)) return fail("flow_threshold must be a positive number");
    if (!(p->disparity_threshold > 0) || !std::isfinite(p->disparity_threshold)) return fail("disparity_threshold must be a positive number");
    if (!(p->disparity_weight >= 0) || !std::isfinite(p->disparity_weight)) return fail("disparity_weight must be a number that is not negative");
    if (p->iterations < 0 || p->iterations > CART_DENSE_EGO_MAX_ITERATIONS) return fail("iterations must be in [0, 16]");
    if (p->stride < 1 || p->stride > 16) return fail("stride must be in [1, 16]");
    if (p->min_inliers < 6 || p->min_inliers > (1 << 30)) return fail("min_inliers must be in [6, 2^30]");
    if (check_camera(cam)) return -1;
    if (!rel0) return fail("rel0 is NULL");
    for (int k = 0; k < 12; ++k) {
        const double bound = k % 4 == 3 ? 1e6 : 2.0;
        if (!std::isfinite(rel0[k]) || std::fabs(rel0[k]) > bound)
            return fail("rel0[" + std::to_string(k) + "] must be finite and within " + (k % 4 == 3 ? "1e6 (translation)" : "2 (rotation)"));
    }
    if (w < 1 || w > 16384) return fail("width must be in [1, 16384]");
    if (h < 1 || h > 16384) return fail("height must be in [1, 16384]");
    if (g && (w > g->max_width || h > g->max_height))
        return fail("width x height exceeds the object's " + std::to_string(g->max_width) + " x " + std::to_string(g->max_height));
    if (!g) return fail("bad arguments");
    struct Image { const char *name; const void *ptr; size_t step, elem; };
    const Image in[] = {{"disp_cur", disp_cur, disp_cur_step, 2}, {"disp_prev", disp_prev, disp_prev_step, 2}, {"flow", flow, flow_step, 4}, {"mask", mask, mask_step, 1}};
    for (const Image &im : in)
        if (!im.ptr && &im != &in[3]) return fail(std::string(im.name) + " is NULL");
    if (!result) return fail("result is NULL");
    const uintptr_t rb = reinterpret_cast<uintptr_t>(result), re = rb + sizeof(cart_dense_ego_result);
    for (const Image &im : in) {
        if (!im.ptr) continue;
        const uintptr_t b = reinterpret_cast<uintptr_t>(im.ptr);
        if ((b % im.elem) || (im.step % im.elem)) return fail(std::string(im.name) + " and its step must be " + std::to_string(im.elem) + "-byte aligned");
        if (im.step < (size_t)w * im.elem) return fail(std::string(im.name) + "_step is below the row size");
        if (rb < b + (size_t)(h - 1) * im.step + (size_t)w * im.elem && b < re) return fail(std::string("result and ") + im.name + " must not overlap");
    }
    if (rb % 8) return fail("result must be 8-byte aligned");

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

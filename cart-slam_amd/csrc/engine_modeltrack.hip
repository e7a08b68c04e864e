// engine_modeltrack.hip -- C ABI of the frame-to-model pose tracking (include/cart_engine.h): argument checks and the
// cart_model_track device object, which owns the row partials and the pose state of a call.  The volume belongs to the cart_voxel_map
// the call is given (engine_voxelmap.h) and is only read.

#include "engine_host.h"
#include "engine_modeltrack.h"
#include "engine_voxelmap.h"

using namespace cart_amd;

extern "C" {

static_assert(sizeof(cart_model_track_params) == 2 * 8 + 3 * 4 + 4, "cart_model_track_params: two doubles and three int32");
static_assert(sizeof(cart_model_track_result) == sizeof(cart_dense_ego_result), "cart_model_track_result has the layout of cart_dense_ego_result");

void cart_model_track_default_params(cart_model_track_params *p) {
    if (!p) return;
    *p = cart_model_track_params{0.9, 0.01, 4, 1, 1024};
}

int cart_model_track_create(cart_engine *e, int max_width, int max_height, cart_model_track **out) {
    if (check_max_size(max_width, max_height)) return -1;
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_model_track *g = new (std::nothrow) cart_model_track(e, max_width, max_height);
    if (!g) return fail("out of host memory");
    if (g->alloc(&g->partial, (size_t)kTrackColorWords * max_height * sizeof(double)) || g->alloc(&g->state, sizeof(DenseEgoState)) ||
        g->alloc(&g->color_state, sizeof(ModelTrackColorState)) || g->create_event()) {
        destroy_object(g);
        return fail("allocating the model tracking workspaces failed");
    }
    *out = g;
    return 0;
}

void cart_model_track_destroy(cart_model_track *g) { destroy_object(g); }

int cart_model_track_refine(cart_model_track *g, cart_voxel_map *m, const cart_ego_camera *cam, const double *pose0, const cart_model_track_params *p,
                            const int16_t *disp, size_t disp_step, const uint8_t *mask, size_t mask_step, int w, int h, cart_model_track_result *result,
                            void *stream_) {
    if (check_model_track_params(p)) return -1;
    if (check_camera(cam) || check_pose("pose0", pose0) || check_frame_size(w, h)) return -1;
    if (!g) return fail("bad arguments");
    if (!m) return fail("map is NULL");
    if (g->device_id != m->device_id) return fail("object and map are on different devices");
    if (g->check_fits(w, h)) return -1;
    const Extent in[] = {Extent::image("disp", disp, disp_step, 2, w, h), Extent::image("mask", mask, mask_step, 1, w, h)};
    if (!disp) return fail("disp is NULL");
    if (!result) return fail("result is NULL");
    const Extent res{"result", result, sizeof(cart_model_track_result), 8, sizeof(cart_model_track_result), 1};
    for (const Extent &im : in) {
        if (!im.ptr) continue;
        if (check_pitched(im)) return -1;
        if (overlap(res, im)) return fail(std::string("result and ") + im.name + " must not overlap");   // the output is named first here
    }
    if (res.begin() % 8) return fail("result must be 8-byte aligned");

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*g, stream);   // the tracker first, then the map: every other call takes the map alone, so the order cannot invert
    if (call.begin()) return -1;
    ObjectCall map_call(*m, stream);
    if (map_call.begin()) return -1;
    ModelTrackArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid_of(m); a.cam = *cam; a.mp = m->p; a.p = *p;
    std::memcpy(a.pose0, pose0, sizeof(a.pose0));
    a.disp = disp; a.disp_step = disp_step; a.mask = mask; a.mask_step = mask_step;
    a.w = w; a.h = h;
    a.ni = (w + p->stride - 1) / p->stride; a.nj = (h + p->stride - 1) / p->stride;
    a.rows_cap = g->max_height; a.empty = m->valid ? 0 : 1;
    a.partial = g->partial; a.state = g->state; a.result = result;
    launch_model_track(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

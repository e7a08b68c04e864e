// engine_modeltrack_color.hip -- C ABI of the colour-aided frame-to-model tracking (include/cart_engine.h): argument checks
// of cart_model_track_refine_color.  The call runs on a cart_model_track (engine_modeltrack.h): its row partials, which hold the 31 words
// of this call's rows, and a pose state of its own.  The TSDF volume belongs to the cart_voxel_map, the colour volume to the
// cart_voxel_color; both are only read, each under its own origin.

#include "engine_host.h"
#include "engine_modeltrack.h"
#include "engine_voxelcolor.h"
#include "engine_voxelmap.h"

using namespace cart_amd;

extern "C" {

static_assert(sizeof(cart_model_track_color_params) == 2 * 8 + 2 * 4, "cart_model_track_color_params: two doubles and two int32");
static_assert(sizeof(cart_model_track_color_result) == 176 && offsetof(cart_model_track_color_result, rms_photo_initial) == sizeof(cart_model_track_result),
              "cart_model_track_color_result: cart_model_track_result, then four doubles and two int32");

void cart_model_track_color_default_params(cart_model_track_color_params *p) {
    if (!p) return;
    *p = cart_model_track_color_params{64.0, 0.25, 1, 0};
}

int cart_model_track_refine_color(cart_model_track *g, cart_voxel_map *m, cart_voxel_color *c, const cart_ego_camera *cam, const double *pose0,
                                  const cart_model_track_params *p, const cart_model_track_color_params *cp, const int16_t *disp, size_t disp_step,
                                  const uint8_t *image, size_t image_step, int channels, const uint8_t *mask, size_t mask_step, int w, int h,
                                  cart_model_track_color_result *result, void *stream_) {
    if (check_model_track_params(p)) return -1;
    if (!cp) return fail("color_params is NULL");
    if (!(cp->photo_weight >= 0) || !std::isfinite(cp->photo_weight)) return fail("photo_weight must be a number that is not negative");
    if (!(cp->photo_gate > 0) || !(cp->photo_gate <= 1)) return fail("photo_gate must be a number in (0, 1]");
    if (cp->color_min_weight < 1 || cp->color_min_weight > 255) return fail("color_min_weight must be in [1, 255]");
    if (cp->reserved != 0) return fail("color_params: reserved must be 0");
    if (channels != 1 && channels != 3) return fail("channels must be 1 or 3");
    if (check_camera(cam) || check_pose("pose0", pose0) || check_frame_size(w, h)) return -1;
    if (!g) return fail("bad arguments");
    if (!m) return fail("map is NULL");
    if (!c) return fail("color is NULL");
    if (g->device_id != m->device_id) return fail("object and map are on different devices");
    if (c->device_id != m->device_id) return fail("color and map are on different devices");
    if (c->n[0] != m->n[0] || c->n[1] != m->n[1] || c->n[2] != m->n[2]) return fail("the map's shape is not the colour object's");
    if (g->check_fits(w, h)) return -1;
    const Extent in[] = {Extent::image("disp", disp, disp_step, 2, w, h), Extent{"image", image, image_step, 1, (size_t)w * channels, h},
                         Extent::image("mask", mask, mask_step, 1, w, h)};
    if (!disp) return fail("disp is NULL");
    if (!image) return fail("image is NULL");
    if (!result) return fail("result is NULL");
    const Extent res{"result", result, sizeof(cart_model_track_color_result), 8, sizeof(cart_model_track_color_result), 1};
    for (const Extent &im : in) {
        if (!im.ptr) continue;
        if (check_pitched(im)) return -1;
        if (overlap(res, im)) return fail(std::string("result and ") + im.name + " must not overlap");   // the output is named first here
    }
    if (res.begin() % 8) return fail("result must be 8-byte aligned");

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*g, stream);   // the tracker first, then the map, then the colour object: S37 takes map before colour, so the order cannot invert
    if (call.begin()) return -1;
    ObjectCall map_call(*m, stream);
    if (map_call.begin()) return -1;
    ObjectCall color_call(*c, stream);
    if (color_call.begin()) return -1;
    ModelTrackColorArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid_of(m); a.cgrid = color_grid(c); a.cam = *cam; a.mp = m->p; a.p = *p; a.cp = *cp;
    std::memcpy(a.pose0, pose0, sizeof(a.pose0));
    a.disp = disp; a.disp_step = disp_step; a.mask = mask; a.mask_step = mask_step; a.image = image; a.image_step = image_step; a.channels = channels;
    a.w = w; a.h = h;
    a.ni = (w + p->stride - 1) / p->stride; a.nj = (h + p->stride - 1) / p->stride;
    a.rows_cap = g->max_height; a.empty = m->valid ? 0 : 1; a.cempty = c->valid ? 0 : 1;
    a.partial = g->partial; a.state = g->color_state; a.result = result;
    launch_model_track_color(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// engine_objects.hip -- C ABI of the moving-object tracks (include/cart_engine.h): argument checks and the
// cart_object_tracker device object, which owns the histograms, the accumulators, the id -> object scratch image and the tracks.  The
// scratch image is set to -1 once here and left all -1 by every call (the last kernel takes back what the first one wrote), so the call
// path has no clear of 4 bytes per pixel.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

static_assert(sizeof(cart_object) == 192 && alignof(cart_object) == 8, "cart_object layout (DESIGN.md S31)");
static_assert(sizeof(cart_track) == 96 && alignof(cart_track) == 8, "cart_track layout (DESIGN.md S31)");
static_assert(sizeof(cart_object_params) == 56, "cart_object_params layout (DESIGN.md S31)");

struct cart_object_tracker : SizedObject {
    using SizedObject::SizedObject;
    int max_objects = 0, max_tracks = 0;
    int32_t *slot_of = nullptr;      // [max_height * max_width]; a call uses the first width * height entries
    int32_t *hist = nullptr;         // [max_objects][CART_OBJECT_BINS]
    int32_t *median = nullptr;       // [max_objects][2]
    ObjectAcc *acc = nullptr;        // [max_objects]
    cart_object *objects = nullptr;  // [max_objects]
    cart_track *tracks = nullptr;    // [max_tracks]
    ObjectState *state = nullptr;
};

void cart_object_default_params(cart_object_params *p) {
    if (!p) return;
    *p = cart_object_params{1.0, 2.0, 5.0, 2.0, 64, 16, 50, 3, 3};
}

int cart_object_tracker_create(cart_engine *e, int max_width, int max_height, int max_objects, int max_tracks, cart_object_tracker **out) {
    if (check_max_size(max_width, max_height)) return -1;
    if (max_objects < 1 || max_objects > kObjectMaxObjects) return fail("max_objects must be in [1, 256]");
    if (max_tracks < 1 || max_tracks > kObjectMaxTracks) return fail("max_tracks must be in [1, 256]");
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_object_tracker *t = new (std::nothrow) cart_object_tracker(e, max_width, max_height);
    if (!t) return fail("out of host memory");
    t->max_objects = max_objects;
    t->max_tracks = max_tracks;
    const size_t sbytes = (size_t)max_width * max_height * sizeof(int32_t);
    if (t->alloc(&t->slot_of, sbytes) || t->alloc(&t->hist, (size_t)max_objects * CART_OBJECT_BINS * sizeof(int32_t)) ||
        t->alloc(&t->median, (size_t)max_objects * 2 * sizeof(int32_t)) || t->alloc(&t->acc, (size_t)max_objects * sizeof(ObjectAcc)) ||
        t->alloc(&t->objects, (size_t)max_objects * sizeof(cart_object)) || t->alloc(&t->tracks, (size_t)max_tracks * sizeof(cart_track)) ||
        t->alloc(&t->state, sizeof(ObjectState)) || t->create_event() || hipMemset(t->slot_of, 0xff, sbytes) != hipSuccess ||
        hipMemset(t->state, 0, sizeof(ObjectState)) != hipSuccess) {
        destroy_object(t);
        return fail("allocating the object tracker's workspaces failed");
    }
    launch_object_reset(t->tracks, max_tracks, t->state, nullptr);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) {   // everything is in place before any stream can use the object
        destroy_object(t);
        return fail("initialising the object tracker failed");
    }
    *out = t;
    return 0;
}

void cart_object_tracker_destroy(cart_object_tracker *t) { destroy_object(t); }

int cart_object_tracker_reset(cart_object_tracker *t, void *stream_) {
    if (!t) return fail("bad arguments");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*t, stream);
    if (call.begin()) return -1;
    launch_object_reset(t->tracks, t->max_tracks, t->state, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_object_tracker_update(cart_object_tracker *t, const cart_ego_camera *cam, const double *rel, const double *pose, const cart_object_params *p,
                               const int32_t *ids, size_t ids_step, const cart_component *table, int max_components, const int32_t *n_components,
                               const int16_t *disp_cur, size_t disp_cur_step, const int16_t *disp_prev, size_t disp_prev_step, const int16_t *flow,
                               size_t flow_step, int w, int h, cart_object *objects_out, cart_track *tracks_out, int32_t *counts_out, void *stream_) {
    if (!p) return fail("params is NULL");
    if (check_positive("min_disparity", p->min_disparity)) return -1;
    if (!(p->disparity_band >= 0.5 && p->disparity_band <= 64.0)) return fail("disparity_band must be in [0.5, 64]");
    if (check_positive("max_speed", p->max_speed) || check_positive("gate", p->gate)) return -1;
    if (p->min_area < 1 || p->min_area > (1 << 30)) return fail("min_area must be in [1, 2^30]");
    if (p->min_points < 1 || p->min_points > (1 << 30)) return fail("min_points must be in [1, 2^30]");
    if (p->gain_percent < 0 || p->gain_percent > 100) return fail("gain_percent must be in [0, 100]");
    if (p->max_missed < 0 || p->max_missed > 255) return fail("max_missed must be in [0, 255]");
    if (p->min_age < 1 || p->min_age > 255) return fail("min_age must be in [1, 255]");
    if (check_camera(cam) || check_pose("rel", rel) || check_pose("pose", pose) || check_frame_size(w, h)) return -1;
    if (max_components < 1 || max_components > (1 << 24)) return fail("max_components must be in [1, 2^24]");
    if (!t) return fail("bad arguments");
    if (t->check_fits(w, h)) return -1;
    const auto image = [&](const char *name, const void *ptr, size_t step, size_t elem) { return Extent::image(name, ptr, step, elem, w, h); };
    const auto block = [](const char *name, const void *ptr, size_t bytes, size_t elem) { return Extent{name, ptr, bytes, elem, bytes, 1}; };
    // the inputs, then the outputs from kOutputs on: an output is checked against everything before it
    enum { kIds, kTable, kCount, kDispCur, kDispPrev, kFlow, kObjects, kTracks, kCounts, kAll, kOutputs = kObjects };
    const Extent all[] = {image("ids", ids, ids_step, 4), block("table", table, (size_t)max_components * sizeof(cart_component), 4),
                          block("n_components", n_components, sizeof(int32_t), 4), image("disp_cur", disp_cur, disp_cur_step, 2),
                          image("disp_prev", disp_prev, disp_prev_step, 2), image("flow", flow, flow_step, 4),
                          block("objects_out", objects_out, (size_t)t->max_objects * sizeof(cart_object), 8),
                          block("tracks_out", tracks_out, (size_t)t->max_tracks * sizeof(cart_track), 8), block("counts_out", counts_out, 8 * sizeof(int32_t), 4)};
    static_assert(sizeof(all) / sizeof(all[0]) == kAll, "one entry per index");
    for (int i = 0; i < kAll; ++i)
        if (!all[i].ptr && i != kObjects) return fail(std::string(all[i].name) + " is NULL");
    for (int i : {kIds, kDispCur, kDispPrev, kFlow})
        if (check_pitched(all[i])) return -1;
    for (int i : {kTable, kCount, kObjects, kTracks, kCounts})   // not pitched: their own wording
        if (all[i].ptr && all[i].begin() % all[i].elem) return fail(std::string(all[i].name) + " must be " + std::to_string(all[i].elem) + "-byte aligned");
    // No output may overlap another buffer: an input under an output would be another frame's by the next call, and two outputs in one
    // place would hold whichever store came last.
    if (check_outputs_apart(all, kOutputs, kAll)) return -1;

    ObjectArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam = *cam; a.p = *p;
    std::memcpy(a.rel, rel, sizeof(a.rel));
    std::memcpy(a.pose, pose, sizeof(a.pose));
    a.ids = ids; a.ids_step = ids_step; a.table = table; a.max_components = max_components; a.n_components = n_components;
    a.disp_cur = disp_cur; a.disp_cur_step = disp_cur_step; a.disp_prev = disp_prev; a.disp_prev_step = disp_prev_step;
    a.flow = flow; a.flow_step = flow_step; a.w = w; a.h = h; a.max_objects = t->max_objects; a.max_tracks = t->max_tracks;
    a.slot_of = t->slot_of; a.hist = t->hist; a.median = t->median; a.acc = t->acc; a.objects = t->objects; a.tracks = t->tracks; a.state = t->state;
    a.objects_out = objects_out; a.tracks_out = tracks_out; a.counts_out = counts_out;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*t, stream);
    if (call.begin()) return -1;
    launch_object_update(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

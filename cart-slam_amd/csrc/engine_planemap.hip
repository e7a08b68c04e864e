// engine_planemap.hip -- C ABI of the world-frame bird's-eye plane map (include/cart_engine.h): argument checks, the
// window arithmetic (host, int64) and the cart_plane_map device object; and of its rebuild from stored keyframes (S30): the
// cart_plane_store ring of keyframe images and cart_plane_map_rebuild.

#include "engine_host.h"
#include "engine_planemap.h"

using namespace cart_amd;

extern "C" {

struct cart_plane_map : DeviceObject {
    using DeviceObject::DeviceObject;
    int nx = 0, nz = 0;
    cart_plane_map_params p{};
    cart_plane_map_cell *cells = nullptr;   // [nz][nx], toroidal (engine_internal.h, PlaneMapGrid)
    bool valid = false;                     // a window exists (guarded by mu)
    int64_t ox = 0, oz = 0;                 // its origin in absolute cells
};

void cart_plane_map_default_params(cart_plane_map_params *p) {
    if (!p) return;
    *p = cart_plane_map_params{0.25, 1.0, 20.0, 10.0, 0.05};
}

static int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }
static int floor_mod(int64_t a, int n) { return (int)(((a % n) + n) % n); }

static PlaneMapGrid grid_of(const cart_plane_map *m) { return PlaneMapGrid{m->cells, m->nx, m->nz, floor_mod(m->ox, m->nx), floor_mod(m->oz, m->nz)}; }

int cart_plane_map_create(cart_engine *e, int cells_x, int cells_z, const cart_plane_map_params *p, cart_plane_map **out) {
    if (cells_x < 32 || cells_x > 4096 || cells_x % 16) return fail("cells_x must be a multiple of 16 in [32, 4096]");
    if (cells_z < 32 || cells_z > 4096 || cells_z % 16) return fail("cells_z must be a multiple of 16 in [32, 4096]");
    if (!p) return fail("params is NULL");
    if (!(p->cell_size >= 0.01) || !std::isfinite(p->cell_size)) return fail("cell_size must be a number >= 0.01");
    if (check_positive("min_disparity", p->min_disparity) || check_positive("max_depth", p->max_depth) || check_positive("max_lateral", p->max_lateral)) return -1;
    if (!(p->height_quantum >= 0.001) || !std::isfinite(p->height_quantum)) return fail("height_quantum must be a number >= 0.001");
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_plane_map *m = new (std::nothrow) cart_plane_map(e);
    if (!m) return fail("out of host memory");
    m->nx = cells_x; m->nz = cells_z; m->p = *p;
    if (m->alloc(&m->cells, (size_t)cells_x * cells_z * sizeof(cart_plane_map_cell)) || m->create_event()) {
        destroy_object(m);
        return fail("allocating the plane map failed");
    }
    *out = m;
    return 0;
}

void cart_plane_map_destroy(cart_plane_map *m) { destroy_object(m); }

int cart_plane_map_clear(cart_plane_map *m) {
    if (!m) return fail("map is NULL");
    std::lock_guard<std::mutex> lk(m->mu);
    m->valid = false;   // the next update empties the grid on its stream
    return 0;
}

int cart_plane_map_update(cart_plane_map *m, const cart_ego_camera *cam, const double *pose, const int16_t *disp, size_t disp_step, const uint8_t *planes,
                          size_t planes_step, int w, int h, void *stream_) {
    if (check_camera(cam) || check_pose("pose", pose) || check_frame_size(w, h)) return -1;
    if (!m) return fail("map is NULL");
    if (!disp || !planes) return fail("NULL pointer");
    if ((reinterpret_cast<uintptr_t>(disp) & 1) || (disp_step & 1)) return fail("disparity and its step must be 2-byte aligned");
    if (disp_step < (size_t)w * sizeof(int16_t)) return fail("disparity_step is below the row size");
    if (check_pitched(Extent::image("planes", planes, planes_step, 1, w, h))) return -1;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    // the window (S24): |t| <= 1e6 and cell_size >= 0.01 keep every value below 2^27
    const int64_t cx = (int64_t)std::floor(pose[3] / m->p.cell_size), cz = (int64_t)std::floor(pose[11] / m->p.cell_size);
    const int64_t ox = 16 * floor_div(cx - m->nx / 2, 16), oz = 16 * floor_div(cz - m->nz / 2, 16);
    const int64_t dx = ox - m->ox, dz = oz - m->oz;
    const bool all = !m->valid || std::llabs(dx) >= m->nx || std::llabs(dz) >= m->nz;
    m->ox = ox; m->oz = oz; m->valid = true;
    const PlaneMapGrid grid = grid_of(m);
    if (all) {
        launch_plane_map_clear(grid, 0, m->nx, 0, m->nz, stream);
    } else {   // the strips that entered: |dx| columns on the side the window moved to, |dz| rows likewise
        if (dx) launch_plane_map_clear(grid, dx > 0 ? m->nx - (int)dx : 0, (int)std::llabs(dx), 0, m->nz, stream);
        if (dz) launch_plane_map_clear(grid, 0, m->nx, dz > 0 ? m->nz - (int)dz : 0, (int)std::llabs(dz), stream);
    }
    PlaneMapVoteArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid; a.cam = *cam; a.p = m->p;
    std::memcpy(a.pose, pose, sizeof(a.pose));
    a.ox = (double)ox; a.oz = (double)oz;
    a.disp = disp; a.disp_step = disp_step; a.planes = planes; a.planes_step = planes_step; a.w = w; a.h = h;
    launch_plane_map_vote(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- S30: the keyframe image store and the rebuild ----
int cart_plane_store_create(cart_engine *e, int width, int height, int capacity, cart_plane_store **out) {
    if (check_frame_size(width, height)) return -1;
    if (capacity < 1 || capacity > 1024) return fail("capacity must be in [1, 1024]");
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_plane_store *s = new (std::nothrow) cart_plane_store(e);
    if (!s) return fail("out of host memory");
    s->w = width; s->h = height; s->capacity = capacity;
    const size_t plane = (size_t)width * height;
    uint8_t *images = nullptr;   // one allocation: the int16 planes, then the u8 planes
    if (s->alloc(&images, 3 * plane * (size_t)capacity) || s->alloc(&s->records, sizeof(PlaneRevoteRecord) * kRevoteMaxEntries) || s->create_event() ||
        hipHostMalloc(reinterpret_cast<void **>(&s->staging), sizeof(PlaneRevoteRecord) * kRevoteMaxEntries, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&s->uploaded, hipEventDisableTiming) != hipSuccess) {
        cart_plane_store_destroy(s);
        return fail("allocating the plane store failed");
    }
    s->disp = reinterpret_cast<int16_t *>(images);
    s->planes = images + 2 * plane * (size_t)capacity;
    s->ids.assign((size_t)capacity, 0);
    *out = s;
    return 0;
}

void cart_plane_store_destroy(cart_plane_store *s) {
    if (!s) return;
    (void)hipSetDevice(s->device_id);
    (void)hipDeviceSynchronize();
    if (s->staging) (void)hipHostFree(s->staging);
    if (s->uploaded) (void)hipEventDestroy(s->uploaded);
    destroy_object(s);
}

int cart_plane_store_clear(cart_plane_store *s) {
    if (!s) return fail("store is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    s->inserted = 0;
    return 0;
}

int cart_plane_store_size(cart_plane_store *s, int *frames, int *capacity) {
    if (!s) return fail("store is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    if (frames) *frames = (int)std::min<uint64_t>(s->inserted, (uint64_t)s->capacity);
    if (capacity) *capacity = s->capacity;
    return 0;
}

int cart_plane_store_contains(cart_plane_store *s, uint64_t frame_id, int *slot) {
    if (!s) return fail("store is NULL");
    if (!slot) return fail("slot is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    *slot = s->find(frame_id);
    return 0;
}

int cart_plane_store_insert(cart_plane_store *s, uint64_t frame_id, const int16_t *disp, size_t disp_step, const uint8_t *planes, size_t planes_step, int w, int h,
                            void *stream_) {
    if (check_frame_size(w, h)) return -1;
    if (!s) return fail("store is NULL");
    if (!disp || !planes) return fail("NULL pointer");
    if ((reinterpret_cast<uintptr_t>(disp) & 1) || (disp_step & 1)) return fail("disparity and its step must be 2-byte aligned");
    if (disp_step < (size_t)w * sizeof(int16_t)) return fail("disparity_step is below the row size");
    if (check_pitched(Extent::image("planes", planes, planes_step, 1, w, h))) return -1;
    if (w != s->w || h != s->h) return fail("width x height must equal the store's W x H");

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*s, stream);
    if (call.begin()) return -1;
    const int slot = (int)(s->inserted % (uint64_t)s->capacity);
    const size_t at = (size_t)slot * w * h;
    launch_plane_store_insert(disp, disp_step, planes, planes_step, s->disp + at, s->planes + at, w, h, stream);
    HIP_TRY(hipGetLastError());
    s->ids[slot] = frame_id;
    s->inserted += 1;
    return 0;
}

int cart_plane_map_rebuild(cart_plane_map *m, cart_plane_store *s, const cart_ego_camera *cam, const uint64_t *ids, const double *poses, int count,
                           const double *window_pose, int *used_out, void *stream_) {
    if (count < 0 || count > kRevoteMaxEntries) return fail("count must be in [0, 4096]");
    if (check_camera(cam) || check_pose("window_pose", window_pose)) return -1;
    if (count > 0 && !ids) return fail("ids is NULL");
    if (count > 0 && !poses) return fail("poses is NULL");
    for (int k = 0; k < count; ++k)
        if (check_pose(("poses[" + std::to_string(k) + "]").c_str(), poses + 12 * (size_t)k)) return -1;
    if (!m) return fail("map is NULL");
    if (!s) return fail("store is NULL");
    if (m->device_id != s->device_id) return fail("map and store are on different devices");

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall map_call(*m, stream);   // the map first, then the store: insert takes the store alone, so the order cannot invert
    if (map_call.begin()) return -1;
    ObjectCall store_call(*s, stream);
    if (store_call.begin()) return -1;
    int used = 0;
    if (stage_rebuild_entries(s, ids, poses, count, stream, &used)) return -1;
    // the window (S24) of window_pose, emptied whole
    const int64_t cx = (int64_t)std::floor(window_pose[3] / m->p.cell_size), cz = (int64_t)std::floor(window_pose[11] / m->p.cell_size);
    m->ox = 16 * floor_div(cx - m->nx / 2, 16); m->oz = 16 * floor_div(cz - m->nz / 2, 16); m->valid = true;
    const PlaneMapGrid grid = grid_of(m);
    launch_plane_map_clear(grid, 0, m->nx, 0, m->nz, stream);
    PlaneMapVoteArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid; a.cam = *cam; a.p = m->p;
    a.ox = (double)m->ox; a.oz = (double)m->oz;
    a.disp = s->disp; a.disp_step = (size_t)s->w * sizeof(int16_t); a.planes = s->planes; a.planes_step = (size_t)s->w; a.w = s->w; a.h = s->h;
    launch_plane_map_revote(a, s->records, used, stream);
    HIP_TRY(hipGetLastError());
    if (used_out) *used_out = used;
    return 0;
}

int cart_plane_map_window(cart_plane_map *m, int64_t *origin_x, int64_t *origin_z, int *valid) {
    if (!m) return fail("map is NULL");
    if (!origin_x || !origin_z || !valid) return fail("NULL pointer");
    std::lock_guard<std::mutex> lk(m->mu);
    *origin_x = m->valid ? m->ox : 0;
    *origin_z = m->valid ? m->oz : 0;
    *valid = m->valid ? 1 : 0;
    return 0;
}

int cart_plane_map_read(cart_plane_map *m, cart_plane_map_cell *host_cells, int64_t *origin_x, int64_t *origin_z, void *stream_) {
    if (!m) return fail("map is NULL");
    if (!host_cells || !origin_x || !origin_z) return fail("NULL pointer");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    const size_t n = (size_t)m->nx * m->nz;
    if (!m->valid) {
        std::fill(host_cells, host_cells + n, cart_plane_map_cell{0, 0, INT32_MAX, INT32_MIN});
        *origin_x = *origin_z = 0;
        return 0;
    }
    std::vector<cart_plane_map_cell> stored(n);
    HIP_TRY(hipMemcpyAsync(stored.data(), m->cells, n * sizeof(cart_plane_map_cell), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const PlaneMapGrid g = grid_of(m);   // toroidal storage -> window order: two pieces per row
    for (int rz = 0; rz < g.nz; ++rz) {
        const cart_plane_map_cell *row = stored.data() + (size_t)((rz + g.mz) % g.nz) * g.nx;
        cart_plane_map_cell *dst = host_cells + (size_t)rz * g.nx;
        std::copy(row + g.mx, row + g.nx, dst);
        std::copy(row, row + g.mx, dst + (g.nx - g.mx));
    }
    *origin_x = m->ox; *origin_z = m->oz;
    return 0;
}

int cart_plane_map_classify(cart_plane_map *m, int min_votes, int obstacle_percent, uint8_t *classes, size_t classes_step, void *stream_) {
    if (!m) return fail("map is NULL");
    if (min_votes < 1) return fail("min_votes must be at least 1");
    if (obstacle_percent < 1 || obstacle_percent > 100) return fail("obstacle_percent must be in [1, 100]");
    if (!classes) return fail("classes is NULL");
    if (classes_step < (size_t)m->nx) return fail("classes_step is below the row size");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    launch_plane_map_classify(grid_of(m), m->valid ? 0 : 1, (unsigned)min_votes, (unsigned)obstacle_percent, classes, classes_step, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

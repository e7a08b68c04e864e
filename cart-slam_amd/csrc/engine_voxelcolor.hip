// engine_voxelcolor.hip -- C ABI of the colour companion of the TSDF voxel map (include/cart_engine.h): argument checks
// and the cart_voxel_color device object, which owns the colour volume, its window origin and its counter block.  The object keeps the
// shape and the parameters of the map it was made for, not the map.  It has no window arithmetic: cart_voxel_color_integrate follows the
// map's current origin (read under the map's lock; lock order map, then colour) and empties what S33's move rule empties, with S33's
// launch_voxel_clear.  The volume is never cleared by hipMemset: the first integrate after create / clear empties it by a kernel on the
// call's stream.  The counter block is zeroed once at create and left all zero by every call.

#include "engine_host.h"
#include "engine_voxelcolor.h"
#include "engine_voxelmap.h"

using namespace cart_amd;

extern "C" {

static_assert(sizeof(cart_voxel_rgb) == 4, "cart_voxel_rgb is one 32-bit word");

int cart_voxel_color_create(cart_engine *e, cart_voxel_map *map, int max_weight, cart_voxel_color **out) {
    if (max_weight < 1 || max_weight > 255) return fail("max_weight must be in [1, 255]");
    if (!e || !out) return fail("bad arguments");
    if (!map) return fail("map is NULL");
    if (map->device_id != e->params.device_id) return fail("map and engine are on different devices");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_voxel_color *c = new (std::nothrow) cart_voxel_color(e);
    if (!c) return fail("out of host memory");
    for (int a = 0; a < 3; ++a) c->n[a] = map->n[a];   // fixed for the map's life: no lock
    c->p = map->p; c->max_weight = max_weight;
    if (c->alloc(&c->voxels, (size_t)c->n[0] * c->n[1] * c->n[2] * sizeof(uint32_t)) || c->alloc(&c->counters, kColorCounters * sizeof(int32_t)) ||
        c->create_event() || hipMemset(c->counters, 0, kColorCounters * sizeof(int32_t)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {   // the zeros are in place before any stream can use the object
        destroy_object(c);
        return fail("allocating the colour volume failed");
    }
    *out = c;
    return 0;
}

void cart_voxel_color_destroy(cart_voxel_color *c) { destroy_object(c); }

int cart_voxel_color_clear(cart_voxel_color *c) {
    if (!c) return fail("color is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    c->valid = false;   // the next integrate empties the volume on its stream
    return 0;
}

int cart_voxel_color_window(cart_voxel_color *c, int64_t *origin3, int32_t *shape3, int *valid) {
    if (!c) return fail("color is NULL");
    if (!origin3) return fail("origin3 is NULL");
    if (!shape3) return fail("shape3 is NULL");
    if (!valid) return fail("valid is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    for (int a = 0; a < 3; ++a) {
        origin3[a] = c->valid ? c->o[a] : 0;
        shape3[a] = c->n[a];
    }
    *valid = c->valid ? 1 : 0;
    return 0;
}

int cart_voxel_color_integrate(cart_voxel_color *c, cart_voxel_map *m, const cart_ego_camera *cam, const double *pose, const int16_t *disp, size_t disp_step,
                               const uint8_t *image, size_t image_step, int channels, int w, int h, const uint8_t *mask, size_t mask_step, int32_t *counts,
                               void *stream_) {
    if (channels != 1 && channels != 3) return fail("channels must be 1 or 3");
    if (check_camera(cam) || check_pose("pose", pose) || check_frame_size(w, h)) return -1;
    if (!c) return fail("color is NULL");
    if (!m) return fail("map is NULL");
    if (c->device_id != m->device_id) return fail("color and map are on different devices");
    if (c->n[0] != m->n[0] || c->n[1] != m->n[1] || c->n[2] != m->n[2]) return fail("the map's shape is not the colour object's");
    if (!disp) return fail("disp is NULL");
    if (!image) return fail("image is NULL");
    const Extent all[] = {Extent::image("disp", disp, disp_step, 2, w, h), Extent{"image", image, image_step, 1, (size_t)w * channels, h},
                          Extent::image("mask", mask, mask_step, 1, w, h), Extent{"counts", counts, 8, 4, 8, 1}};
    for (int i = 0; i < 3; ++i)
        if (all[i].ptr && check_pitched(all[i])) return -1;
    if (all[3].begin() % 4) return fail("counts must be 4-byte aligned");   // not pitched: its own wording
    if (check_outputs_apart(all, 3, 4)) return -1;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    std::unique_lock<std::mutex> map_lock(m->mu);   // the map first, then the colour object: no call takes them the other way round
    if (!m->valid) return fail("the map has no window");
    const int64_t o[3] = {m->o[0], m->o[1], m->o[2]};
    ObjectCall call(*c, stream);
    if (call.begin()) return -1;
    bool all_new = !c->valid;
    for (int a = 0; a < 3; ++a)
        if (c->valid && std::llabs(o[a] - c->o[a]) >= c->n[a]) all_new = true;
    int64_t d[3] = {0, 0, 0};
    for (int a = 0; a < 3; ++a) {
        d[a] = all_new ? 0 : o[a] - c->o[a];
        c->o[a] = o[a];
    }
    c->valid = true;
    const VoxelGrid grid = color_grid(c);
    if (all_new) {
        launch_voxel_clear(grid, 0, grid.nx, 0, grid.ny, 0, grid.nz, stream);
    } else {   // the slabs that entered (S33): |d| layers on the side the window moved to, one launch per axis that moved
        if (d[0]) launch_voxel_clear(grid, d[0] > 0 ? grid.nx - (int)d[0] : 0, (int)std::llabs(d[0]), 0, grid.ny, 0, grid.nz, stream);
        if (d[1]) launch_voxel_clear(grid, 0, grid.nx, d[1] > 0 ? grid.ny - (int)d[1] : 0, (int)std::llabs(d[1]), 0, grid.nz, stream);
        if (d[2]) launch_voxel_clear(grid, 0, grid.nx, 0, grid.ny, d[2] > 0 ? grid.nz - (int)d[2] : 0, (int)std::llabs(d[2]), stream);
    }
    ColorIntegrateArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid; a.cam = *cam; a.p = c->p;
    std::memcpy(a.pose, pose, sizeof(a.pose));
    a.disp = disp; a.disp_step = disp_step; a.mask = mask; a.mask_step = mask_step; a.image = image; a.image_step = image_step;
    a.channels = channels; a.max_weight = c->max_weight; a.counts = counts; a.counters = c->counters; a.w = w; a.h = h;
    launch_color_integrate(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_voxel_color_vertices(cart_voxel_color *c, const cart_mesh_vertex *vertices, const int32_t *n_vertices, int max_vertices, const int64_t *origin3,
                              cart_voxel_rgb *colors, void *stream_) {
    if (max_vertices < 1 || max_vertices > 1 << 26) return fail("max_vertices must be in [1, 2^26]");
    if (!origin3) return fail("origin3 is NULL");
    for (int a = 0; a < 3; ++a)
        if (std::llabs(origin3[a]) > ((int64_t)1 << 27)) return fail("origin3[" + std::to_string(a) + "] must be within 2^27");
    if (!c) return fail("color is NULL");
    if (!vertices) return fail("vertices is NULL");
    if (!n_vertices) return fail("n_vertices is NULL");
    if (!colors) return fail("colors is NULL");
    const size_t vbytes = (size_t)max_vertices * sizeof(cart_mesh_vertex), cbytes = (size_t)max_vertices * sizeof(cart_voxel_rgb);
    const Extent all[] = {Extent{"vertices", vertices, vbytes, 4, vbytes, 1}, Extent{"n_vertices", n_vertices, 4, 4, 4, 1}, Extent{"colors", colors, cbytes, 4, cbytes, 1}};
    for (const Extent &x : all)
        if (x.begin() % 4) return fail(std::string(x.name) + " must be 4-byte aligned");   // not pitched: its own wording
    if (check_outputs_apart(all, 2, 3)) return -1;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*c, stream);
    if (call.begin()) return -1;
    ColorVerticesArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = color_grid(c); a.voxel_size = c->p.voxel_size;
    a.mx = (double)origin3[0]; a.my = (double)origin3[1]; a.mz = (double)origin3[2];
    a.vertices = vertices; a.n_vertices = n_vertices; a.max_vertices = max_vertices; a.colors = reinterpret_cast<uint32_t *>(colors);
    a.empty = c->valid ? 0 : 1;
    launch_color_vertices(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_voxel_color_render(cart_voxel_color *c, const cart_ego_camera *cam, const double *pose, const int16_t *disp, size_t disp_step, int w, int h,
                            uint8_t *image_bgr, size_t image_step, uint8_t *alpha, size_t alpha_step, int32_t *counts, void *stream_) {
    if (check_camera(cam) || check_pose("pose", pose) || check_frame_size(w, h)) return -1;
    if (!c) return fail("color is NULL");
    if (!disp) return fail("disp is NULL");
    if (!image_bgr) return fail("image_bgr is NULL");
    const Extent all[] = {Extent::image("disp", disp, disp_step, 2, w, h), Extent{"image_bgr", image_bgr, image_step, 1, (size_t)w * 3, h},
                          Extent::image("alpha", alpha, alpha_step, 1, w, h), Extent{"counts", counts, 4, 4, 4, 1}};
    for (int i = 0; i < 3; ++i)
        if (all[i].ptr && check_pitched(all[i])) return -1;
    if (all[3].begin() % 4) return fail("counts must be 4-byte aligned");   // not pitched: its own wording
    if (check_outputs_apart(all, 1, 4)) return -1;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*c, stream);
    if (call.begin()) return -1;
    ColorRenderArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = color_grid(c); a.cam = *cam; a.voxel_size = c->p.voxel_size;
    std::memcpy(a.pose, pose, sizeof(a.pose));
    a.disp = disp; a.disp_step = disp_step; a.image = image_bgr; a.image_step = image_step; a.alpha = alpha; a.alpha_step = alpha_step;
    a.counts = counts; a.counters = c->counters; a.w = w; a.h = h; a.empty = c->valid ? 0 : 1;
    launch_color_render(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_voxel_color_read(cart_voxel_color *c, cart_voxel_rgb *host_voxels, int64_t *origin3, void *stream_) {
    if (!c) return fail("color is NULL");
    if (!host_voxels) return fail("host_voxels is NULL");
    if (!origin3) return fail("origin3 is NULL");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*c, stream);
    if (call.begin()) return -1;
    const size_t count = (size_t)c->n[0] * c->n[1] * c->n[2];
    if (!c->valid) {
        std::memset(host_voxels, 0, count * sizeof(cart_voxel_rgb));
        origin3[0] = origin3[1] = origin3[2] = 0;
        return 0;
    }
    std::vector<cart_voxel_rgb> stored(count);
    HIP_TRY(hipMemcpyAsync(stored.data(), c->voxels, count * sizeof(cart_voxel_rgb), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const VoxelGrid g = color_grid(c);   // toroidal storage -> window order: two pieces per row
    for (int rz = 0; rz < g.nz; ++rz)
        for (int ry = 0; ry < g.ny; ++ry) {
            const cart_voxel_rgb *row = stored.data() + ((size_t)((rz + g.mz) % g.nz) * g.ny + (size_t)((ry + g.my) % g.ny)) * g.nx;
            cart_voxel_rgb *dst = host_voxels + ((size_t)rz * g.ny + ry) * g.nx;
            std::copy(row + g.mx, row + g.nx, dst);
            std::copy(row, row + g.mx, dst + (g.nx - g.mx));
        }
    for (int a = 0; a < 3; ++a) origin3[a] = c->o[a];
    return 0;
}

int cart_voxel_color_write(cart_voxel_color *c, const cart_voxel_rgb *host_voxels, const int64_t *origin3, void *stream_) {
    if (!origin3) return fail("origin3 is NULL");
    for (int a = 0; a < 3; ++a)
        if (origin3[a] % 8 || std::llabs(origin3[a]) > ((int64_t)1 << 27)) return fail("origin3[" + std::to_string(a) + "] must be a multiple of 8 within 2^27");
    if (!c) return fail("color is NULL");
    if (!host_voxels) return fail("host_voxels is NULL");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*c, stream);
    if (call.begin()) return -1;
    VoxelGrid g = color_grid(c);
    g.mx = floor_mod(origin3[0], g.nx); g.my = floor_mod(origin3[1], g.ny); g.mz = floor_mod(origin3[2], g.nz);
    const size_t count = (size_t)g.nx * g.ny * g.nz;
    std::vector<cart_voxel_rgb> stored(count);   // window order -> toroidal storage: two pieces per row, the inverse of _read
    for (int rz = 0; rz < g.nz; ++rz)
        for (int ry = 0; ry < g.ny; ++ry) {
            cart_voxel_rgb *row = stored.data() + ((size_t)((rz + g.mz) % g.nz) * g.ny + (size_t)((ry + g.my) % g.ny)) * g.nx;
            const cart_voxel_rgb *src = host_voxels + ((size_t)rz * g.ny + ry) * g.nx;
            std::copy(src, src + (g.nx - g.mx), row + g.mx);
            std::copy(src + (g.nx - g.mx), src + g.nx, row);
        }
    HIP_TRY(hipMemcpyAsync(c->voxels, stored.data(), count * sizeof(cart_voxel_rgb), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int a = 0; a < 3; ++a) c->o[a] = origin3[a];
    c->valid = true;
    return 0;
}

}  // extern "C"

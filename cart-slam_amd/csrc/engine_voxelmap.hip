// engine_voxelmap.hip -- C ABI of the rolling TSDF voxel map (include/cart_engine.h): argument checks, the window
// arithmetic (host, int64) and the cart_voxel_map device object, which owns the volume and the counter block.  The volume is never
// cleared by hipMemset: the first integrate after create / clear empties the whole window by a kernel on the call's stream.  The counter
// block is zeroed once at create and left all zero by every call.  cart_voxel_map_rebuild (S35) integrates the frames of a cart_plane_store
// (engine_planemap.h) into a fixed window in one launch.  cart_voxel_map_mesh (S36) extracts the window's surface (voxelmesh_kernels.hip) and
// cart_voxel_map_write puts host voxels under the kernels.

#include "engine_host.h"
#include "engine_planemap.h"
#include "engine_voxelmap.h"

using namespace cart_amd;

extern "C" {

static_assert(sizeof(cart_voxel) == 4, "cart_voxel is one 32-bit word");
static_assert(sizeof(cart_voxel_map_params) == 8 * 8 + 2 * 4, "cart_voxel_map_params: eight doubles and two int32");

void cart_voxel_map_default_params(cart_voxel_map_params *p) {
    if (!p) return;
    *p = cart_voxel_map_params{0.125, 1.0, 0.5, 16.0, 0.25, 0.5, 8.0, 0.125, 64, 1};
}

static int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

static int check_cells(const char *name, int n) {
    if (n < 16 || n > 1024 || n % 8) return fail(std::string(name) + " must be a multiple of 8 in [16, 1024]");
    return 0;
}

static int check_params(const cart_voxel_map_params *p) {
    if (!p) return fail("params is NULL");
    if (!(p->voxel_size >= 0.01) || !std::isfinite(p->voxel_size)) return fail("voxel_size must be a number >= 0.01");
    if (check_positive("min_disparity", p->min_disparity) || check_positive("min_depth", p->min_depth)) return -1;
    if (!(p->max_depth > p->min_depth) || !std::isfinite(p->max_depth)) return fail("max_depth must be a number above min_depth");
    if (check_positive("truncation", p->truncation)) return -1;
    if (!(p->disparity_sigma >= 0) || !std::isfinite(p->disparity_sigma)) return fail("disparity_sigma must be a number >= 0");
    if (!std::isfinite(p->lookahead) || std::fabs(p->lookahead) > 1000.0) return fail("lookahead must be finite and within 1000");
    if (!(p->march_step > 0) || !std::isfinite(p->march_step) || !(p->march_step <= p->truncation)) return fail("march_step must be a positive number <= truncation");
    if (!(std::floor((p->max_depth - p->min_depth) / p->march_step) <= 8192.0)) return fail("march_step gives more than 8192 steps between min_depth and max_depth");
    if (p->max_weight < 1 || p->max_weight > 65535) return fail("max_weight must be in [1, 65535]");
    if (p->min_weight < 1 || p->min_weight > 65535) return fail("min_weight must be in [1, 65535]");
    return 0;
}

int cart_voxel_map_create(cart_engine *e, int cells_x, int cells_y, int cells_z, const cart_voxel_map_params *p, cart_voxel_map **out) {
    if (check_cells("cells_x", cells_x) || check_cells("cells_y", cells_y) || check_cells("cells_z", cells_z)) return -1;
    if ((int64_t)cells_x * cells_y * cells_z > (int64_t)1 << 26) return fail("cells_x * cells_y * cells_z must be at most 2^26");
    if (check_params(p)) return -1;
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_voxel_map *m = new (std::nothrow) cart_voxel_map(e);
    if (!m) return fail("out of host memory");
    m->n[0] = cells_x; m->n[1] = cells_y; m->n[2] = cells_z; m->p = *p;
    if (m->alloc(&m->voxels, (size_t)cells_x * cells_y * cells_z * sizeof(uint32_t)) || m->alloc(&m->counters, kVoxelCounters * sizeof(int32_t)) ||
        m->create_event() || hipMemset(m->counters, 0, kVoxelCounters * sizeof(int32_t)) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {   // the zeros are in place before any stream can use the object
        destroy_object(m);
        return fail("allocating the voxel map failed");
    }
    *out = m;
    return 0;
}

void cart_voxel_map_destroy(cart_voxel_map *m) { destroy_object(m); }

int cart_voxel_map_clear(cart_voxel_map *m) {
    if (!m) return fail("map is NULL");
    std::lock_guard<std::mutex> lk(m->mu);
    m->valid = false;   // the next integrate empties the volume on its stream
    return 0;
}

int cart_voxel_map_window(cart_voxel_map *m, int64_t *origin3, int32_t *shape3, int *valid) {
    if (!m) return fail("map is NULL");
    if (!origin3) return fail("origin3 is NULL");
    if (!shape3) return fail("shape3 is NULL");
    if (!valid) return fail("valid is NULL");
    std::lock_guard<std::mutex> lk(m->mu);
    for (int a = 0; a < 3; ++a) {
        origin3[a] = m->valid ? m->o[a] : 0;
        shape3[a] = m->n[a];
    }
    *valid = m->valid ? 1 : 0;
    return 0;
}

int cart_voxel_map_integrate(cart_voxel_map *m, const cart_ego_camera *cam, const double *pose, const int16_t *disp, size_t disp_step, int w, int h,
                             const uint8_t *mask, size_t mask_step, int32_t *counts, void *stream_) {
    if (check_camera(cam) || check_pose("pose", pose) || check_frame_size(w, h)) return -1;
    if (!m) return fail("map is NULL");
    if (!disp) return fail("disp is NULL");
    const Extent all[] = {Extent::image("disp", disp, disp_step, 2, w, h), Extent::image("mask", mask, mask_step, 1, w, h), Extent{"counts", counts, 8, 4, 8, 1}};
    for (int i = 0; i < 2; ++i)
        if (all[i].ptr && check_pitched(all[i])) return -1;
    if (all[2].begin() % 4) return fail("counts must be 4-byte aligned");   // not pitched: its own wording
    if (check_outputs_apart(all, 2, 3)) return -1;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    // the window (S33): |t| <= 1e6, |lookahead R| <= 2000 and voxel_size >= 0.01 keep every value below 2^27
    int64_t o[3];
    bool all_new = !m->valid;
    for (int a = 0; a < 3; ++a) {
        const int64_t c = (int64_t)std::floor((pose[4 * a + 3] + m->p.lookahead * pose[4 * a + 2]) / m->p.voxel_size);
        o[a] = 8 * floor_div(c - m->n[a] / 2, 8);
        if (m->valid && std::llabs(o[a] - m->o[a]) >= m->n[a]) all_new = true;
    }
    int64_t d[3] = {0, 0, 0};
    for (int a = 0; a < 3; ++a) {
        d[a] = all_new ? 0 : o[a] - m->o[a];
        m->o[a] = o[a];
    }
    m->valid = true;
    const VoxelGrid grid = grid_of(m);
    if (all_new) {
        launch_voxel_clear(grid, 0, grid.nx, 0, grid.ny, 0, grid.nz, stream);
    } else {   // the slabs that entered: |d| layers on the side the window moved to, one launch per axis that moved
        if (d[0]) launch_voxel_clear(grid, d[0] > 0 ? grid.nx - (int)d[0] : 0, (int)std::llabs(d[0]), 0, grid.ny, 0, grid.nz, stream);
        if (d[1]) launch_voxel_clear(grid, 0, grid.nx, d[1] > 0 ? grid.ny - (int)d[1] : 0, (int)std::llabs(d[1]), 0, grid.nz, stream);
        if (d[2]) launch_voxel_clear(grid, 0, grid.nx, 0, grid.ny, d[2] > 0 ? grid.nz - (int)d[2] : 0, (int)std::llabs(d[2]), stream);
    }
    VoxelIntegrateArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid; a.cam = *cam; a.p = m->p;
    std::memcpy(a.pose, pose, sizeof(a.pose));
    a.disp = disp; a.disp_step = disp_step; a.mask = mask; a.mask_step = mask_step; a.counts = counts; a.counters = m->counters; a.w = w; a.h = h;
    launch_voxel_integrate(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_voxel_map_rebuild(cart_voxel_map *m, cart_plane_store *s, const cart_ego_camera *cam, const uint64_t *ids, const double *poses, int count,
                           const double *window_pose, int use_mask, int *used_out, int64_t *counts, void *stream_) {
    if (count < 0 || count > kRevoteMaxEntries) return fail("count must be in [0, 4096]");
    if (use_mask != 0 && use_mask != 1) return fail("use_mask must be 0 or 1");
    if (check_camera(cam) || check_pose("window_pose", window_pose)) return -1;
    if (count > 0 && !ids) return fail("ids is NULL");
    if (count > 0 && !poses) return fail("poses is NULL");
    for (int k = 0; k < count; ++k)
        if (check_pose(("poses[" + std::to_string(k) + "]").c_str(), poses + 12 * (size_t)k)) return -1;
    if (!m) return fail("map is NULL");
    if (!s) return fail("store is NULL");
    if (m->device_id != s->device_id) return fail("map and store are on different devices");
    if (reinterpret_cast<uintptr_t>(counts) % 8) return fail("counts must be 8-byte aligned");

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall map_call(*m, stream);   // the map first, then the store, as cart_plane_map_rebuild: insert takes the store alone, so the order cannot invert
    if (map_call.begin()) return -1;
    ObjectCall store_call(*s, stream);
    if (store_call.begin()) return -1;
    int used = 0;
    if (stage_rebuild_entries(s, ids, poses, count, stream, &used)) return -1;
    // the window (S33) of window_pose; the kernel writes every voxel of it, so nothing is emptied first
    for (int a = 0; a < 3; ++a) {
        const int64_t c = (int64_t)std::floor((window_pose[4 * a + 3] + m->p.lookahead * window_pose[4 * a + 2]) / m->p.voxel_size);
        m->o[a] = 8 * floor_div(c - m->n[a] / 2, 8);
    }
    m->valid = true;
    VoxelRebuildArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid_of(m); a.cam = *cam; a.p = m->p;
    a.disp = s->disp; a.planes = use_mask ? s->planes : nullptr; a.records = s->records; a.entries = used; a.w = s->w; a.h = s->h;
    a.counts = reinterpret_cast<long long *>(counts); a.counters = m->counters;
    launch_voxel_rebuild(a, stream);
    HIP_TRY(hipGetLastError());
    if (used_out) *used_out = used;
    return 0;
}

int cart_voxel_map_raycast(cart_voxel_map *m, const cart_ego_camera *cam, const double *pose, int w, int h, int16_t *disp_model, size_t disp_model_step,
                           uint16_t *weight_model, size_t weight_model_step, uint8_t *status, size_t status_step, int32_t *counts, void *stream_) {
    if (check_camera(cam) || check_pose("pose", pose) || check_frame_size(w, h)) return -1;
    if (!m) return fail("map is NULL");
    if (!disp_model) return fail("disp_model is NULL");
    const Extent all[] = {Extent::image("disp_model", disp_model, disp_model_step, 2, w, h), Extent::image("weight_model", weight_model, weight_model_step, 2, w, h),
                          Extent::image("status", status, status_step, 1, w, h), Extent{"counts", counts, 12, 4, 12, 1}};
    for (int i = 0; i < 3; ++i)
        if (all[i].ptr && check_pitched(all[i])) return -1;
    if (all[3].begin() % 4) return fail("counts must be 4-byte aligned");   // not pitched: its own wording
    // every argument is an output: two in one place would hold whichever store came last
    if (check_outputs_apart(all, 0, 4)) return -1;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    VoxelRaycastArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid_of(m); a.cam = *cam; a.p = m->p;
    std::memcpy(a.pose, pose, sizeof(a.pose));
    a.disp = disp_model; a.disp_step = disp_model_step; a.weight = weight_model; a.weight_step = weight_model_step; a.status = status; a.status_step = status_step;
    a.counts = counts; a.counters = m->counters; a.w = w; a.h = h;
    a.steps = (int)std::floor((m->p.max_depth - m->p.min_depth) / m->p.march_step);
    a.empty = m->valid ? 0 : 1;
    launch_voxel_raycast(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_voxel_map_read(cart_voxel_map *m, cart_voxel *host_voxels, int64_t *origin3, void *stream_) {
    if (!m) return fail("map is NULL");
    if (!host_voxels) return fail("host_voxels is NULL");
    if (!origin3) return fail("origin3 is NULL");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    const size_t count = (size_t)m->n[0] * m->n[1] * m->n[2];
    if (!m->valid) {
        std::memset(host_voxels, 0, count * sizeof(cart_voxel));
        origin3[0] = origin3[1] = origin3[2] = 0;
        return 0;
    }
    std::vector<cart_voxel> stored(count);
    HIP_TRY(hipMemcpyAsync(stored.data(), m->voxels, count * sizeof(cart_voxel), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const VoxelGrid g = grid_of(m);   // toroidal storage -> window order: two pieces per row
    for (int rz = 0; rz < g.nz; ++rz)
        for (int ry = 0; ry < g.ny; ++ry) {
            const cart_voxel *row = stored.data() + ((size_t)((rz + g.mz) % g.nz) * g.ny + (size_t)((ry + g.my) % g.ny)) * g.nx;
            cart_voxel *dst = host_voxels + ((size_t)rz * g.ny + ry) * g.nx;
            std::copy(row + g.mx, row + g.nx, dst);
            std::copy(row, row + g.mx, dst + (g.nx - g.mx));
        }
    for (int a = 0; a < 3; ++a) origin3[a] = m->o[a];
    return 0;
}

int cart_voxel_map_mesh(cart_voxel_map *m, int min_weight, cart_mesh_vertex *vertices, int max_vertices, cart_mesh_quad *quads, int max_quads,
                        int32_t *counts, int64_t *origin3, void *stream_) {
    if (min_weight < 0 || min_weight > 65535) return fail("min_weight must be 0 (the map's own) or in [1, 65535]");
    if (max_vertices < 1 || max_vertices > 1 << 26) return fail("max_vertices must be in [1, 2^26]");
    if (max_quads < 1 || max_quads > 1 << 26) return fail("max_quads must be in [1, 2^26]");
    if (!m) return fail("map is NULL");
    if (!vertices) return fail("vertices is NULL");
    if (!quads) return fail("quads is NULL");
    if (!counts) return fail("counts is NULL");
    const size_t vbytes = (size_t)max_vertices * sizeof(cart_mesh_vertex), qbytes = (size_t)max_quads * sizeof(cart_mesh_quad);
    const Extent all[] = {Extent{"vertices", vertices, vbytes, 4, vbytes, 1}, Extent{"quads", quads, qbytes, 4, qbytes, 1}, Extent{"counts", counts, 16, 4, 16, 1}};
    for (const Extent &x : all)
        if (x.begin() % 4) return fail(std::string(x.name) + " must be 4-byte aligned");   // not pitched: its own wording
    if (check_outputs_apart(all, 0, 3)) return -1;

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    const size_t voxels = (size_t)m->n[0] * m->n[1] * m->n[2], blocks = (voxels + kMeshBlock - 1) / kMeshBlock;
    // the first call: the workspace, kept for the object's life (a call whose second allocation failed leaves the first for the next one)
    if (!m->mesh_cells && m->alloc(&m->mesh_cells, voxels * sizeof(uint32_t))) return -1;
    if (!m->mesh_blocks && m->alloc(&m->mesh_blocks, 2 * blocks * sizeof(uint32_t))) return -1;
    VoxelMeshArgs a;
    std::memset(&a, 0, sizeof(a));
    a.grid = grid_of(m); a.voxel_size = m->p.voxel_size; a.min_weight = min_weight ? min_weight : m->p.min_weight;
    a.max_vertices = max_vertices; a.max_quads = max_quads; a.blocks = m->valid ? (int)blocks : 0;
    a.cells = m->mesh_cells; a.block_vertices = m->mesh_blocks; a.block_quads = m->mesh_blocks + blocks;
    a.vertices = vertices; a.quads = quads; a.counts = counts;
    launch_voxel_mesh(a, stream);
    HIP_TRY(hipGetLastError());
    if (origin3)
        for (int k = 0; k < 3; ++k) origin3[k] = m->valid ? m->o[k] : 0;
    return 0;
}

int cart_voxel_map_write(cart_voxel_map *m, const cart_voxel *host_voxels, const int64_t *origin3, void *stream_) {
    if (!origin3) return fail("origin3 is NULL");
    for (int a = 0; a < 3; ++a)
        if (origin3[a] % 8 || std::llabs(origin3[a]) > ((int64_t)1 << 27)) return fail("origin3[" + std::to_string(a) + "] must be a multiple of 8 within 2^27");
    if (!m) return fail("map is NULL");
    if (!host_voxels) return fail("host_voxels is NULL");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    VoxelGrid g = grid_of(m);
    g.mx = floor_mod(origin3[0], g.nx); g.my = floor_mod(origin3[1], g.ny); g.mz = floor_mod(origin3[2], g.nz);
    const size_t count = (size_t)g.nx * g.ny * g.nz;
    std::vector<cart_voxel> stored(count);   // window order -> toroidal storage: two pieces per row, the inverse of _read
    for (int rz = 0; rz < g.nz; ++rz)
        for (int ry = 0; ry < g.ny; ++ry) {
            cart_voxel *row = stored.data() + ((size_t)((rz + g.mz) % g.nz) * g.ny + (size_t)((ry + g.my) % g.ny)) * g.nx;
            const cart_voxel *src = host_voxels + ((size_t)rz * g.ny + ry) * g.nx;
            std::copy(src, src + (g.nx - g.mx), row + g.mx);
            std::copy(src + (g.nx - g.mx), src + g.nx, row);
        }
    HIP_TRY(hipMemcpyAsync(m->voxels, stored.data(), count * sizeof(cart_voxel), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int a = 0; a < 3; ++a) m->o[a] = origin3[a];
    m->valid = true;
    return 0;
}

}  // extern "C"

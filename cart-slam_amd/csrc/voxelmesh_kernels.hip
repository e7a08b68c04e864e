// voxelmesh_kernels.hip -- the surface of the TSDF volume as an indexed quad mesh by naive surface nets (spec S36; C ABI
// in engine_voxelmap.hip).  A thread owns the window voxel of its linear index v = (z ny + y) nx + x: lanes run along x, the contiguous
// storage axis, and v is at once the order of the cells (cell c has its origin corner at voxel c) and of the voxels that own edges, so one
// stable compaction over v gives both output orders.  Five launches:
//   mesh_classify   the eight corners of every cell -> one word per cell (known, active, the crossings of the three edges its origin voxel
//                   owns, the origin corner's side), and the number of active cells of every workgroup (wave ballots, summed in LDS)
//   mesh_count      the quads every voxel's edges emit, from the neighbouring cells' words -> their number per workgroup
//   mesh_scan       one workgroup: both per-workgroup arrays become exclusive offsets; the four counts go to the caller
//   mesh_vertices   every active cell's vertex at offset + rank inside the workgroup; the rank is also written into the cell word
//   mesh_quads      every quad at offset + rank, from the four cells' vertex indices
// Prefix sums only: no atomic decides where a record lands, so the output is the same on every run.  fp64 with + - * / sqrt only, every
// expression in the written order; the normal is voxel_value's gradient (voxel_sample.h), not restated here.

#include "engine_internal.h"
#include "voxel_sample.h"

#pragma clang fp contract(off)

namespace cart_amd {

namespace {

struct MeshVoxel { int x, y, z; bool cell; };   // `cell`: the voxel is the origin corner of an existing cell

__device__ __forceinline__ MeshVoxel mesh_voxel(const VoxelGrid &g, unsigned v) {
    MeshVoxel r;
    const unsigned yz = v / (unsigned)g.nx;
    r.x = (int)(v - yz * (unsigned)g.nx); r.y = (int)(yz % (unsigned)g.ny); r.z = (int)(yz / (unsigned)g.ny);
    r.cell = r.z < g.nz && r.x < g.nx - 1 && r.y < g.ny - 1 && r.z < g.nz - 1;
    return r;
}

// the eight corners of cell (x, y, z) from the toroidal storage, c.v[dy][dz][dx] as voxel_gather leaves them
__device__ __forceinline__ void mesh_corners(const VoxelGrid &g, const MeshVoxel &m, VoxelCorners &c) {
    const int x0 = voxel_wrap(m.x + g.mx, g.nx), y0 = voxel_wrap(m.y + g.my, g.ny), z0 = voxel_wrap(m.z + g.mz, g.nz);
    const int x1 = voxel_wrap(x0 + 1, g.nx), y1 = voxel_wrap(y0 + 1, g.ny), z1 = voxel_wrap(z0 + 1, g.nz);
    const uint32_t *r00 = g.voxels + ((size_t)z0 * g.ny + y0) * g.nx, *r10 = g.voxels + ((size_t)z0 * g.ny + y1) * g.nx;
    const uint32_t *r01 = g.voxels + ((size_t)z1 * g.ny + y0) * g.nx, *r11 = g.voxels + ((size_t)z1 * g.ny + y1) * g.nx;
    c.v[0][0][0] = r00[x0]; c.v[0][0][1] = r00[x1]; c.v[0][1][0] = r01[x0]; c.v[0][1][1] = r01[x1];
    c.v[1][0][0] = r10[x0]; c.v[1][0][1] = r10[x1]; c.v[1][1][0] = r11[x0]; c.v[1][1][1] = r11[x1];
    c.inside = true;
}

__device__ __forceinline__ int mesh_tsdf(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }

// The sum of `n` over the workgroup's threads before this one, and over the whole workgroup in `total`; every thread calls it.
__device__ __forceinline__ unsigned block_rank(unsigned n_before_in_wave, unsigned n_wave, unsigned *wave_sums, unsigned &total) {
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_sums[wave] = n_wave;
    __syncthreads();
    unsigned before = n_before_in_wave;
    total = 0;
#pragma unroll
    for (int k = 0; k < kMeshBlock / 64; ++k) {
        before += k < wave ? wave_sums[k] : 0u;
        total += wave_sums[k];
    }
    return before;
}

__global__ __launch_bounds__(kMeshBlock) void mesh_classify_kernel(VoxelMeshArgs a) {
    __shared__ unsigned wave_sums[kMeshBlock / 64];
    const unsigned v = blockIdx.x * kMeshBlock + threadIdx.x;   // below 2^26
    const MeshVoxel m = mesh_voxel(a.grid, v);
    uint32_t word = 0u;
    if (m.cell) {
        VoxelCorners c;
        mesh_corners(a.grid, m, c);
        unsigned wmin = 65535u, inside = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t w = c.v[k >> 2][(k >> 1) & 1][k & 1];
            wmin = min(wmin, w >> 16);
            inside += mesh_tsdf(w) <= 0 ? 1u : 0u;
        }
        const bool in0 = mesh_tsdf(c.v[0][0][0]) <= 0;
        const bool known = wmin >= (unsigned)a.min_weight;
        word = (known ? kMeshKnown : 0u) | (known && inside != 0u && inside != 8u ? kMeshActive : 0u) | (in0 ? kMeshInside : 0u) |
               (in0 != (mesh_tsdf(c.v[0][0][1]) <= 0) ? kMeshCrossX : 0u) | (in0 != (mesh_tsdf(c.v[1][0][0]) <= 0) ? kMeshCrossX << 1 : 0u) |
               (in0 != (mesh_tsdf(c.v[0][1][0]) <= 0) ? kMeshCrossX << 2 : 0u);
    }
    if (m.z < a.grid.nz) a.cells[v] = word;
    const unsigned long long active = __ballot((word & kMeshActive) != 0u);
    unsigned total;
    (void)block_rank(0u, (unsigned)__popcll(active), wave_sums, total);
    if (threadIdx.x == 0) a.block_vertices[blockIdx.x] = total;
}

// Bit `axis` is set iff the edge that leaves voxel m along that axis emits a quad: the cell of the voxel exists (so the upper voxel is in
// the window), the edge crosses, and the three other cells around it exist and are known as this one is.
__device__ __forceinline__ unsigned mesh_quad_mask(const VoxelMeshArgs &a, const MeshVoxel &m, unsigned v, uint32_t word) {
    if (!m.cell || !(word & kMeshKnown) || !(word & (7u * kMeshCrossX))) return 0u;
    const size_t sy = (size_t)a.grid.nx, sz = (size_t)a.grid.nx * a.grid.ny;
    const bool bx = m.x >= 1, by = m.y >= 1, bz = m.z >= 1;
    // the known bits of the six neighbouring cells that share an owned edge: -y, -z, -y-z, -x, -x-z, -x-y
    const uint32_t ky = by ? a.cells[v - sy] : 0u, kz = bz ? a.cells[v - sz] : 0u, kyz = by && bz ? a.cells[v - sy - sz] : 0u;
    const uint32_t kx = bx ? a.cells[v - 1] : 0u, kxz = bx && bz ? a.cells[v - 1 - sz] : 0u, kxy = bx && by ? a.cells[v - 1 - sy] : 0u;
    unsigned mask = 0u;
    if ((word & kMeshCrossX) && (ky & kz & kyz & kMeshKnown)) mask |= 1u;
    if ((word & (kMeshCrossX << 1)) && (kx & kz & kxz & kMeshKnown)) mask |= 2u;
    if ((word & (kMeshCrossX << 2)) && (kx & ky & kxy & kMeshKnown)) mask |= 4u;
    return mask;
}

__global__ __launch_bounds__(kMeshBlock) void mesh_count_kernel(VoxelMeshArgs a) {
    __shared__ unsigned wave_sums[kMeshBlock / 64];
    const unsigned v = blockIdx.x * kMeshBlock + threadIdx.x;   // below 2^26
    const MeshVoxel m = mesh_voxel(a.grid, v);
    const unsigned mask = mesh_quad_mask(a, m, v, m.cell ? a.cells[v] : 0u);
    const unsigned n = (unsigned)(__popcll(__ballot(mask & 1u)) + __popcll(__ballot(mask & 2u)) + __popcll(__ballot(mask & 4u)));
    unsigned total;
    (void)block_rank(0u, n, wave_sums, total);
    if (threadIdx.x == 0) a.block_quads[blockIdx.x] = total;
}

// One workgroup.  A thread sums its run of consecutive workgroups' counts, vertices in the low and quads in the high half of one 64-bit
// word (both below 2^32: at most 2^26 cells and three quads a voxel); the runs' sums are scanned in LDS; the run is rewritten as offsets.
__global__ __launch_bounds__(kMeshScanThreads) void mesh_scan_kernel(VoxelMeshArgs a) {
    __shared__ unsigned long long sums[kMeshScanThreads];
    const int t = threadIdx.x;
    const int run = (a.blocks + kMeshScanThreads - 1) / kMeshScanThreads;
    const int b0 = min(t * run, a.blocks), b1 = min(b0 + run, a.blocks);
    unsigned long long mine = 0ull;
    for (int b = b0; b < b1; ++b) mine += (unsigned long long)a.block_vertices[b] | ((unsigned long long)a.block_quads[b] << 32);
    sums[t] = mine;
    __syncthreads();
    for (int d = 1; d < kMeshScanThreads; d <<= 1) {   // inclusive scan over the threads
        const unsigned long long add = t >= d ? sums[t - d] : 0ull;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    unsigned long long at = sums[t] - mine;
    for (int b = b0; b < b1; ++b) {
        const unsigned nv = a.block_vertices[b], nq = a.block_quads[b];
        a.block_vertices[b] = (unsigned)at;
        a.block_quads[b] = (unsigned)(at >> 32);
        at += (unsigned long long)nv | ((unsigned long long)nq << 32);
    }
    if (t == kMeshScanThreads - 1) {
        const long long nv = (long long)(unsigned)sums[t], nq = (long long)(sums[t] >> 32);
        a.counts[0] = (int32_t)nv;
        a.counts[1] = (int32_t)nq;
        a.counts[2] = (int32_t)min(nv, (long long)a.max_vertices);
        a.counts[3] = (int32_t)min(nq, (long long)a.max_quads);
    }
}

__global__ __launch_bounds__(kMeshBlock) void mesh_vertices_kernel(VoxelMeshArgs a) {
    __shared__ unsigned wave_sums[kMeshBlock / 64];
    const unsigned v = blockIdx.x * kMeshBlock + threadIdx.x;   // below 2^26
    const int lane = threadIdx.x & 63;
    const MeshVoxel m = mesh_voxel(a.grid, v);
    const uint32_t word = m.cell ? a.cells[v] : 0u;
    const bool active = (word & kMeshActive) != 0u;
    const unsigned long long ballot = __ballot(active);
    unsigned total;
    const unsigned rank = block_rank((unsigned)__popcll(ballot & ((1ull << lane) - 1ull)), (unsigned)__popcll(ballot), wave_sums, total);
    if (!active) return;
    const unsigned index = a.block_vertices[blockIdx.x] + rank;
    a.cells[v] = word | (index << kMeshIndexShift);
    if (index >= (unsigned)a.max_vertices) return;
    VoxelCorners c;
    mesh_corners(a.grid, m, c);
    int t[2][2][2];                           // [dy][dz][dx]
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k >> 2][(k >> 1) & 1][k & 1] = mesh_tsdf(c.v[k >> 2][(k >> 1) & 1][k & 1]);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int n = 0;
    // the twelve edges in the spec's order: x-edges (dy, dz), y-edges (dx, dz), z-edges (dx, dy), each over (0,0), (1,0), (0,1), (1,1)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = e & 1, q = e >> 1;
        const int ta = t[p][q][0], tb = t[p][q][1];
        if ((ta <= 0) != (tb <= 0)) {
            const double f = (double)ta / (double)(ta - tb);
            sx += f; sy += (double)p; sz += (double)q;
            ++n;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = e & 1, q = e >> 1;
        const int ta = t[0][q][p], tb = t[1][q][p];
        if ((ta <= 0) != (tb <= 0)) {
            const double f = (double)ta / (double)(ta - tb);
            sx += (double)p; sy += f; sz += (double)q;
            ++n;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = e & 1, q = e >> 1;
        const int ta = t[q][0][p], tb = t[q][1][p];
        if ((ta <= 0) != (tb <= 0)) {
            const double f = (double)ta / (double)(ta - tb);
            sx += (double)p; sy += (double)q; sz += f;
            ++n;
        }
    }
    c.frx = sx / (double)n; c.fry = sy / (double)n; c.frz = sz / (double)n;   // an active cell has a crossing edge: n >= 3
    VoxelSample s;
    (void)voxel_value(c, 0, s);               // the weights were checked by mesh_classify
    const double n2 = (s.gx * s.gx + s.gy * s.gy) + s.gz * s.gz;
    const double len = sqrt(n2);
    cart_mesh_vertex out;
    out.position[0] = (float)((((double)m.x + 0.5) + c.frx) * a.voxel_size);
    out.position[1] = (float)((((double)m.y + 0.5) + c.fry) * a.voxel_size);
    out.position[2] = (float)((((double)m.z + 0.5) + c.frz) * a.voxel_size);
    out.normal[0] = n2 > 0.0 ? (float)(s.gx / len) : 0.0f;
    out.normal[1] = n2 > 0.0 ? (float)(s.gy / len) : 0.0f;
    out.normal[2] = n2 > 0.0 ? (float)(s.gz / len) : 0.0f;
    a.vertices[index] = out;                  // 4-byte aligned: six dword stores
}

__global__ __launch_bounds__(kMeshBlock) void mesh_quads_kernel(VoxelMeshArgs a) {
    __shared__ unsigned wave_sums[kMeshBlock / 64];
    const unsigned v = blockIdx.x * kMeshBlock + threadIdx.x;   // below 2^26
    const int lane = threadIdx.x & 63;
    const MeshVoxel m = mesh_voxel(a.grid, v);
    const uint32_t word = m.cell ? a.cells[v] : 0u;
    const unsigned mask = mesh_quad_mask(a, m, v, word);
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long b0 = __ballot(mask & 1u), b1 = __ballot(mask & 2u), b2 = __ballot(mask & 4u);
    unsigned total;
    const unsigned rank = block_rank((unsigned)(__popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below)),
                                     (unsigned)(__popcll(b0) + __popcll(b1) + __popcll(b2)), wave_sums, total);
    if (!mask) return;
    unsigned index = a.block_quads[blockIdx.x] + rank;
    const size_t sx = 1, sy = (size_t)a.grid.nx, sz = (size_t)a.grid.nx * a.grid.ny;
    const bool forward = (word & kMeshInside) != 0u;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        if (!(mask & (1u << axis))) continue;
        if (index >= (unsigned)a.max_quads) return;
        // the two axes after this one, cyclically: x -> (y, z), y -> (z, x), z -> (x, y); the cells are (-p-q), (-q), (0), (-p)
        const size_t p = axis == 0 ? sy : axis == 1 ? sz : sx, q = axis == 0 ? sz : axis == 1 ? sx : sy;
        const int c0 = (int)(a.cells[v - p - q] >> kMeshIndexShift), c1 = (int)(a.cells[v - q] >> kMeshIndexShift);
        const int c2 = (int)(word >> kMeshIndexShift), c3 = (int)(a.cells[v - p] >> kMeshIndexShift);
        cart_mesh_quad out;
        out.v[0] = forward ? c0 : c3; out.v[1] = forward ? c1 : c2; out.v[2] = forward ? c2 : c1; out.v[3] = forward ? c3 : c0;
        a.quads[index] = out;                 // 4-byte aligned: four dword stores
        ++index;
    }
}

}  // namespace

void launch_voxel_mesh(const VoxelMeshArgs &a, hipStream_t s) {
    if (a.blocks) {
        hipLaunchKernelGGL(mesh_classify_kernel, dim3((unsigned)a.blocks), dim3(kMeshBlock), 0, s, a);
        hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)a.blocks), dim3(kMeshBlock), 0, s, a);
    }
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kMeshScanThreads), 0, s, a);   // without a window: the four zeros
    if (a.blocks) {
        hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)a.blocks), dim3(kMeshBlock), 0, s, a);
        hipLaunchKernelGGL(mesh_quads_kernel, dim3((unsigned)a.blocks), dim3(kMeshBlock), 0, s, a);
    }
}

}  // namespace cart_amd

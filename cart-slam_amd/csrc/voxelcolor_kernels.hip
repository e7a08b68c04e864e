// voxelcolor_kernels.hip -- the colour companion of the TSDF voxel map (spec S37; C ABI in engine_voxelcolor.hip):
//   voxel_color_integrate  one frame's image into the colour volume.  The form of voxel_integrate_kernel (voxelmap_kernels.hip): lanes run
//                          along x, a workgroup of 4 waves owns 64 x 4 x kColorDepth voxels, a lane walks its z column kVoxelSlices at a time.
//                          Gates 1 and 2 of a group first, then its disparity, mask and image loads together, then gates 3 to 5 and f < 1
//                          (the gate expressions are S33's, copied); one 4-byte load and one 4-byte store per voxel that passed.  A voxel that
//                          fails a gate is neither read nor written.  Nothing of the TSDF volume is read.
//   voxel_color_render     the colours of the points behind a disparity image.  A wave owns an 8 x 8 pixel tile, as the raycast does, so the
//                          eight-corner gathers of neighbouring pixels share storage rows; the eight loads are issued before the first use.
//   voxel_color_vertices   the colours of a mesh's vertices, one lane per vertex; the count is read from device memory.
// The two read-outs share the sample rule (color_sample): a weight-weighted integer mean of the eight voxels around the point.
// The counters: wave ballots, a sum over the workgroup's waves in LDS, one 64-bit integer atomic per workgroup plus its ticket (the render:
// one atomic that carries both); the workgroup with the last ticket hands the sums to the caller's `counts` and zeroes the block again
// (as voxel_integrate_kernel).
// fp64 with + - * / floor only, in the association order of warp_device.h; integers after the projection.  No atomic on the volume.

#include "engine_internal.h"
#include "warp_device.h"

namespace cart_amd {

namespace {

__device__ __forceinline__ int wrap(int v, int n) { return v >= n ? v - n : v; }

// storage index of window voxel (rx, ry, rz)
__device__ __forceinline__ size_t voxel_slot(const VoxelGrid &g, int rx, int ry, int rz) {
    return ((size_t)wrap(rz + g.mz, g.nz) * g.ny + wrap(ry + g.my, g.ny)) * g.nx + wrap(rx + g.mx, g.nx);
}

// The last step of the integrate: `mine` = this workgroup's two sums packed as lo | hi << 32, added to the uint64 word c[0]; c[1] carries
// the ticket in its upper half.  Returns true in the one thread of the grid that came last, with the grid's total in
// `total` and the words zeroed again.  Called by thread 0 only.
__device__ __forceinline__ bool hand_over(unsigned long long *c, unsigned long long mine, unsigned workgroups, unsigned long long &total) {
    if (mine) atomicAdd(c + 0, mine);
    __threadfence();                          // this workgroup's addition before its ticket
    const unsigned long long before = atomicAdd(c + 1, 1ull << 32);
    if ((unsigned)(before >> 32) != workgroups - 1u) return false;
    __threadfence();                          // the last workgroup: every other one's additions are visible
    total = atomicExch(c + 0, 0ull);
    atomicExch(c + 1, 0ull);
    return true;
}

__global__ __launch_bounds__(256) void voxel_color_integrate_kernel(ColorIntegrateArgs a) {
    __shared__ unsigned wave_counts[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rx = blockIdx.x * 64 + lane, ry = blockIdx.y * 4 + wave;
    const bool in = rx < a.grid.nx;           // ny is a multiple of 8: no guard on y
    const double fxb = a.cam.fx * a.cam.baseline;
    const double *P = a.pose;
    const unsigned cap = (unsigned)a.max_weight;
    unsigned n_coloured = 0, n_fresh = 0;
    // kColorDepth slices of z per workgroup, kVoxelSlices at a time; nz is a multiple of kVoxelSlices, so a group of slices is inside or outside whole
#pragma unroll 1
    for (int rz0 = blockIdx.z * kColorDepth; rz0 < min((int)(blockIdx.z + 1) * kColorDepth, a.grid.nz); rz0 += kVoxelSlices) {
    bool ok[kVoxelSlices];
    int sx[kVoxelSlices], sy[kVoxelSlices];
    double qz[kVoxelSlices];
    // gates 1 and 2 of every slice: the pixel
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        ok[k] = false; sx[k] = 0; sy[k] = 0; qz[k] = 0.0;
        if (!in) continue;
        const double gx = a.grid.ox + (double)rx, gy = a.grid.oy + (double)ry, gz = a.grid.oz + (double)(rz0 + k);
        const double d0 = (gx + 0.5) * a.p.voxel_size - P[3], d1 = (gy + 0.5) * a.p.voxel_size - P[7], d2 = (gz + 0.5) * a.p.voxel_size - P[11];
        WarpPoint q;
        q.x = (P[0] * d0 + P[4] * d1) + P[8] * d2;
        q.y = (P[1] * d0 + P[5] * d1) + P[9] * d2;
        q.z = (P[2] * d0 + P[6] * d1) + P[10] * d2;
        if (!(q.z >= a.p.min_depth)) continue;
        const double xd = floor(project_u(a.cam, q) + 0.5), yd = floor(project_v(a.cam, q) + 0.5);
        if (!(xd >= 0.0 && xd <= (double)(a.w - 1) && yd >= 0.0 && yd <= (double)(a.h - 1))) continue;   // a NaN fails
        sx[k] = (int)xd; sy[k] = (int)yd; qz[k] = q.z;
        ok[k] = true;
    }
    // the image loads of the slices that got this far, together: disparity, mask and the pixel's one or three bytes
    int s[kVoxelSlices];
    unsigned m[kVoxelSlices], ob[kVoxelSlices], og[kVoxelSlices], orr[kVoxelSlices];
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        s[k] = ok[k] ? row_ptr(a.disp, a.disp_step, sy[k])[sx[k]] : -32768;
        m[k] = ok[k] && a.mask ? row_ptr(a.mask, a.mask_step, sy[k])[sx[k]] : 0u;
        ob[k] = 0u; og[k] = 0u; orr[k] = 0u;
        if (ok[k]) {
            const uint8_t *row = row_ptr(a.image, a.image_step, sy[k]);
            if (a.channels == 3) {            // uniform over the grid
                ob[k] = row[3 * sx[k]]; og[k] = row[3 * sx[k] + 1]; orr[k] = row[3 * sx[k] + 2];
            } else {
                ob[k] = og[k] = orr[k] = row[sx[k]];
            }
        }
    }
    // gates 3 to 5, then f < 1 on the unclamped f
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        if (!ok[k]) continue;
        ok[k] = false;
        if (s[k] == -32768) continue;
        const double d = (double)s[k] / 16.0;
        if (!(d >= a.p.min_disparity)) continue;
        const double Z = fxb / d;
        if (!(Z <= a.p.max_depth) || m[k] == 1u) continue;
        const double tr = a.p.truncation + a.p.disparity_sigma * ((Z * Z) / fxb);
        const double sdf = Z - qz[k];
        if (!(sdf >= -tr)) continue;
        const double f = sdf / tr;
        ok[k] = f < 1.0;
    }
    // the words of the voxels that passed, loaded together, then averaged and stored
    size_t slot[kVoxelSlices];
    uint32_t word[kVoxelSlices];
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        slot[k] = ok[k] ? voxel_slot(a.grid, rx, ry, rz0 + k) : 0;
        word[k] = ok[k] ? a.grid.voxels[slot[k]] : 0u;
    }
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        const unsigned w = word[k] >> 24;
        if (ok[k]) {
            // every term is non-negative and below 2^18: plain unsigned division rounds half up
            const unsigned den = 2u * (w + 1u);
            const unsigned bn = (2u * (w * (word[k] & 0xffu) + ob[k]) + (w + 1u)) / den;
            const unsigned gn = (2u * (w * ((word[k] >> 8) & 0xffu) + og[k]) + (w + 1u)) / den;
            const unsigned rn = (2u * (w * ((word[k] >> 16) & 0xffu) + orr[k]) + (w + 1u)) / den;
            const unsigned wn = w + 1u < cap ? w + 1u : cap;
            a.grid.voxels[slot[k]] = bn | (gn << 8) | (rn << 16) | (wn << 24);
        }
        if (a.counts) {
            n_coloured += (unsigned)__popcll(__ballot(ok[k]));
            n_fresh += (unsigned)__popcll(__ballot(ok[k] && w == 0u));
        }
    }
    }                                         // the groups of slices
    if (!a.counts) return;                    // uniform over the grid
    if (lane == 0) { wave_counts[wave][0] = n_coloured; wave_counts[wave][1] = n_fresh; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long u = (unsigned long long)wave_counts[0][0] + wave_counts[1][0] + wave_counts[2][0] + wave_counts[3][0];
        const unsigned long long n = (unsigned long long)wave_counts[0][1] + wave_counts[1][1] + wave_counts[2][1] + wave_counts[3][1];
        unsigned long long t = 0;
        if (hand_over(reinterpret_cast<unsigned long long *>(a.counters), u | (n << 32), gridDim.x * gridDim.y * gridDim.z, t)) {
            a.counts[0] = (int32_t)(unsigned)t;
            a.counts[1] = (int32_t)(t >> 32);
        }
    }
}

// The sample rule: (ix, iy, iz) = the absolute index of the lowest of the eight corners, as doubles.  -> b | g << 8 | r << 16 | alpha << 24,
// or 0 when a corner lies outside the window (a NaN fails the comparison) or no corner has a weight.
__device__ __forceinline__ uint32_t color_sample(const VoxelGrid &g, double ix, double iy, double iz) {
    const double hx = g.ox + (double)(g.nx - 2), hy = g.oy + (double)(g.ny - 2), hz = g.oz + (double)(g.nz - 2);   // the last i0 with both corners inside
    if (!(ix >= g.ox && ix <= hx && iy >= g.oy && iy <= hy && iz >= g.oz && iz <= hz)) return 0u;
    const int x0 = wrap((int)(ix - g.ox) + g.mx, g.nx), y0 = wrap((int)(iy - g.oy) + g.my, g.ny), z0 = wrap((int)(iz - g.oz) + g.mz, g.nz);
    const int x1 = wrap(x0 + 1, g.nx), y1 = wrap(y0 + 1, g.ny), z1 = wrap(z0 + 1, g.nz);
    const uint32_t *r00 = g.voxels + ((size_t)z0 * g.ny + y0) * g.nx, *r10 = g.voxels + ((size_t)z0 * g.ny + y1) * g.nx;
    const uint32_t *r01 = g.voxels + ((size_t)z1 * g.ny + y0) * g.nx, *r11 = g.voxels + ((size_t)z1 * g.ny + y1) * g.nx;
    // the eight corners before the first use
    const uint32_t v[8] = {r00[x0], r00[x1], r01[x0], r01[x1], r10[x0], r10[x1], r11[x0], r11[x1]};
    unsigned W = 0u, Sb = 0u, Sg = 0u, Sr = 0u;   // W <= 2040, the sums <= 520200
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned w = v[k] >> 24;
        W += w;
        Sb += w * (v[k] & 0xffu);
        Sg += w * ((v[k] >> 8) & 0xffu);
        Sr += w * ((v[k] >> 16) & 0xffu);
    }
    if (W == 0u) return 0u;
    const unsigned den = 2u * W;
    return ((2u * Sb + W) / den) | (((2u * Sg + W) / den) << 8) | (((2u * Sr + W) / den) << 16) | ((W < 255u ? W : 255u) << 24);
}

__global__ __launch_bounds__(256) void voxel_color_render_kernel(ColorRenderArgs a) {
    __shared__ unsigned wave_counts[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 32 + wave * 8 + (lane & 7), y = blockIdx.y * 8 + (lane >> 3);   // a wave = an 8 x 8 tile
    const bool in = x < a.w && y < a.h;
    uint32_t c = 0u;
    if (in && !a.empty) {
        const int s = row_ptr(a.disp, a.disp_step, y)[x];
        if (s != -32768 && s >= 1) {
            const double d = (double)s / 16.0;
            const double Z = (a.cam.fx * a.cam.baseline) / d;
            const WarpPoint pw = pose_carry(a.pose, WarpPoint{back_project_x(a.cam, x, Z), back_project_y(a.cam, y, Z), Z});
            const double ax = pw.x / a.voxel_size - 0.5, ay = pw.y / a.voxel_size - 0.5, az = pw.z / a.voxel_size - 0.5;
            c = color_sample(a.grid, floor(ax), floor(ay), floor(az));
        }
    }
    if (in) {
        uint8_t *px = row_ptr(a.image, a.image_step, y) + 3 * (size_t)x;   // one thread writes a pixel's three bytes
        px[0] = (uint8_t)(c & 0xffu); px[1] = (uint8_t)((c >> 8) & 0xffu); px[2] = (uint8_t)((c >> 16) & 0xffu);
        if (a.alpha) row_ptr(a.alpha, a.alpha_step, y)[x] = (uint8_t)(c >> 24);
    }
    if (!a.counts) return;                    // uniform over the grid
    const unsigned n = (unsigned)__popcll(__ballot((c >> 24) != 0u));
    if (lane == 0) wave_counts[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        // one word and one atomic per workgroup: the count (at most 2^28 pixels) in the low half, the ticket in the high half.  The render
        // has one workgroup per 256 pixels and little else to do: with hand_over's two atomics the tickets were most of its time.
        unsigned long long *c = reinterpret_cast<unsigned long long *>(a.counters) + 2;
        const unsigned long long mine = (unsigned long long)wave_counts[0] + wave_counts[1] + wave_counts[2] + wave_counts[3];
        const unsigned long long before = atomicAdd(c, mine | (1ull << 32));
        if ((unsigned)(before >> 32) == gridDim.x * gridDim.y - 1u) {   // the last workgroup: `before` holds every other one's count
            a.counts[0] = (int32_t)(unsigned)(before + mine);
            atomicExch(c, 0ull);
        }
    }
}

__global__ __launch_bounds__(256) void voxel_color_vertices_kernel(ColorVerticesArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int n = min(*a.n_vertices, a.max_vertices);
    if (k >= n) return;
    uint32_t c = 0u;
    if (!a.empty) {
        const float *p = a.vertices[k].position;
        const double ax = (double)p[0] / a.voxel_size - 0.5, ay = (double)p[1] / a.voxel_size - 0.5, az = (double)p[2] / a.voxel_size - 0.5;
        c = color_sample(a.grid, a.mx + floor(ax), a.my + floor(ay), a.mz + floor(az));
    }
    a.colors[k] = c;
}

}  // namespace

void launch_color_integrate(const ColorIntegrateArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(voxel_color_integrate_kernel, dim3((unsigned)((a.grid.nx + 63) / 64), (unsigned)(a.grid.ny / 4), (unsigned)((a.grid.nz + kColorDepth - 1) / kColorDepth)), dim3(256), 0, s, a);
}

void launch_color_render(const ColorRenderArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(voxel_color_render_kernel, dim3((unsigned)((a.w + 31) / 32), (unsigned)((a.h + 7) / 8)), dim3(256), 0, s, a);
}

void launch_color_vertices(const ColorVerticesArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(voxel_color_vertices_kernel, dim3((unsigned)((a.max_vertices + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace cart_amd

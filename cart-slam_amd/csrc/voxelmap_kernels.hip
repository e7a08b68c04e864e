// voxelmap_kernels.hip -- the rolling TSDF voxel map and its model raycast (spec S33; C ABI in engine_voxelmap.hip):
//   voxel_clear      empties a box of the window (the slabs a window move brings in, or the whole grid); a lane writes four voxels
//   voxel_integrate  one frame into the volume.  Lanes run along x, the contiguous storage axis; a lane owns a column of kVoxelDepth voxels
//                    along z for the whole call, walks it kVoxelSlices voxels at a time and computes each from scratch (incremental forms
//                    along an axis would change bits).  The gate chain runs first for a group's voxels, so their image loads are in flight
//                    together; then the 4-byte words of the voxels that passed are loaded together, averaged and stored.  A voxel that fails
//                    a gate is neither read nor written.  With CART_VOXEL_CULL a group of slices whose box cannot pass the gates is skipped.
//   voxel_raycast    the model seen from a pose.  A wave owns an 8 x 8 pixel tile and its 64 rays march the same z_k in lock-step, so the
//                    eight-corner gathers of a step fall into a few neighbouring storage rows; the eight loads of a sample are issued
//                    before the first use.  A wave leaves the loop when all of its rays have ended.
// The counters: wave ballots, a sum over the workgroup's waves in LDS, one 64-bit integer atomic per workgroup plus its ticket; the
// workgroup with the last ticket hands the sums to the caller's `counts` and zeroes the block again (as fusion_fuse_kernel).
// fp64 with + - * / floor only, in the association order of warp_device.h, which holds the warp chain.  No atomic on the volume.

#include "engine_internal.h"
#include "warp_device.h"

namespace cart_amd {

namespace {

__device__ __forceinline__ int wrap(int v, int n) { return v >= n ? v - n : v; }

// storage index of window voxel (rx, ry, rz)
__device__ __forceinline__ size_t voxel_slot(const VoxelGrid &g, int rx, int ry, int rz) {
    return ((size_t)wrap(rz + g.mz, g.nz) * g.ny + wrap(ry + g.my, g.ny)) * g.nx + wrap(rx + g.mx, g.nx);
}

__global__ __launch_bounds__(256) void voxel_clear_kernel(VoxelGrid g, int rx0, int rw4, int ry0, int rh, int rz0, int rd) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rw4 * rh * rd) return;
    const int qx = (int)(i % rw4), ry = (int)((i / rw4) % rh), rz = (int)(i / ((size_t)rw4 * rh));
    // rx0 + 4 qx and g.mx are multiples of 4 and nx of 8: the four voxels do not straddle the wrap and are 16-byte aligned
    *reinterpret_cast<uint4 *>(g.voxels + voxel_slot(g, rx0 + 4 * qx, ry0 + ry, rz0 + rz)) = make_uint4(0u, 0u, 0u, 0u);
}

// The last step of both counting kernels: `mine` = this workgroup's two sums packed as lo | hi << 32 for word 0 and the sum for word 1
// (below 2^32), added to the two uint64 words at c; word 1 carries the ticket in its upper half.  Returns true in the one thread of the
// workgroup that came last, with the grid's totals in total0 / total1 and the words zeroed again.  Called by thread 0 only.
__device__ __forceinline__ bool hand_over(unsigned long long *c, unsigned long long mine0, unsigned long long mine1, unsigned workgroups,
                                          unsigned long long &total0, unsigned long long &total1) {
    if (mine0) atomicAdd(c + 0, mine0);
    __threadfence();                          // this workgroup's addition before its ticket
    const unsigned long long before = atomicAdd(c + 1, mine1 | (1ull << 32));
    if ((unsigned)(before >> 32) != workgroups - 1u) return false;
    __threadfence();                          // the last workgroup: every other one's additions are visible
    total0 = atomicExch(c + 0, 0ull);
    total1 = atomicExch(c + 1, 0ull);
    return true;
}

#if CART_VOXEL_CULL
// Conservative culling of a whole workgroup (CART_VOXEL_CULL): true only if no voxel of the box of 64 x 4 x kVoxelSlices voxels can pass gates
// 1, 2 and 4.  q is affine in the voxel index, so a linear functional of q over the box lies between its value at the box's base corner
// plus the negative and plus the positive contributions of the three edges; `slack` is a million times the rounding error of these sums and
// of the gates' own expressions.  The functionals: q_z against min_depth and against the farthest z a voxel may have (gate 4 with Z <=
// max_depth), and the four image borders, u >= -0.5 <=> fx q_x + (cx + 0.5) q_z >= 0 for q_z > 0 and likewise for the other three.
__device__ __forceinline__ double dabs(double v) { return v < 0.0 ? -v : v; }
__device__ __forceinline__ bool voxel_box_culled(const VoxelIntegrateArgs &a, int rx0, int rx1, int ry0, int rz0) {
    const double *P = a.pose;
    const double vs = a.p.voxel_size;
    const double b[3] = {((a.grid.ox + (double)rx0) + 0.5) * vs - P[3], ((a.grid.oy + (double)ry0) + 0.5) * vs - P[7], ((a.grid.oz + (double)rz0) + 0.5) * vs - P[11]};
    const double e[3] = {(double)(rx1 - rx0) * vs, 3.0 * vs, (double)(kVoxelSlices - 1) * vs};
    const double slack = 1e-8 * (1.0 + dabs(b[0]) + dabs(b[1]) + dabs(b[2]) + e[0] + e[1] + e[2] + dabs(P[3]) + dabs(P[7]) + dabs(P[11]));
    const double fxb = a.cam.fx * a.cam.baseline;
    const double zfar = (a.p.max_depth + (a.p.truncation + a.p.disparity_sigma * ((a.p.max_depth * a.p.max_depth) / fxb))) * (1.0 + 1e-9);
    // coefficient of q_x (kx), q_y (ky) and q_z (kz) of each functional; > 0 inside for the first three, < 0 inside for the last three
    const double kx[6] = {0.0, a.cam.fx, 0.0, 0.0, a.cam.fx, 0.0};
    const double ky[6] = {0.0, 0.0, a.cam.fy, 0.0, 0.0, a.cam.fy};
    const double kz[6] = {1.0, a.cam.cx + 0.5, a.cam.cy + 0.5, 1.0, a.cam.cx - ((double)a.w - 0.5), a.cam.cy - ((double)a.h - 0.5)};
    const double bound[6] = {a.p.min_depth, 0.0, 0.0, zfar, 0.0, 0.0};
    const double scale[6] = {1.0, a.cam.fx + dabs(a.cam.cx) + 1.0, a.cam.fy + dabs(a.cam.cy) + 1.0, 1.0, a.cam.fx + dabs(a.cam.cx) + (double)a.w,
                             a.cam.fy + dabs(a.cam.cy) + (double)a.h};
    bool culled = false;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        double lo = 0.0, hi = 0.0;            // the functional over the box lies in [lo, hi] + rounding
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double c = (kx[f] * P[4 * r] + ky[f] * P[4 * r + 1]) + kz[f] * P[4 * r + 2];
            const double at = c * b[r], edge = c * e[r];
            lo += at + (edge < 0.0 ? edge : 0.0);
            hi += at + (edge > 0.0 ? edge : 0.0);
        }
        const double s = 8.0 * slack * scale[f];
        culled = culled || (f < 3 ? hi + s < bound[f] : lo - s > bound[f]);
    }
    return culled;
}
#endif

__global__ __launch_bounds__(256) void voxel_integrate_kernel(VoxelIntegrateArgs a) {
    __shared__ unsigned wave_counts[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rx = blockIdx.x * 64 + lane, ry = blockIdx.y * 4 + wave;
    const bool in = rx < a.grid.nx;           // ny is a multiple of 8: no guard on y
    const double fxb = a.cam.fx * a.cam.baseline;
    const double *P = a.pose;
    unsigned n_updated = 0, n_near = 0;
    // kVoxelDepth slices of z per workgroup, kVoxelSlices at a time; nz is a multiple of kVoxelSlices, so a group of slices is inside or outside whole
#pragma unroll 1
    for (int rz0 = blockIdx.z * kVoxelDepth; rz0 < min((int)(blockIdx.z + 1) * kVoxelDepth, a.grid.nz); rz0 += kVoxelSlices) {
#if CART_VOXEL_CULL
    // uniform over the workgroup
    if (voxel_box_culled(a, (int)blockIdx.x * 64, min((int)blockIdx.x * 64 + 63, a.grid.nx - 1), (int)blockIdx.y * 4, rz0)) continue;
#endif
    int obs[kVoxelSlices];
    bool ok[kVoxelSlices], near[kVoxelSlices];
    int sx[kVoxelSlices], sy[kVoxelSlices];
    double qz[kVoxelSlices];
    // gates 1 and 2 of every slice: the pixel
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        ok[k] = false; near[k] = false; obs[k] = 0; sx[k] = 0; sy[k] = 0; qz[k] = 0.0;
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
    // the image loads of the slices that got this far, together
    int s[kVoxelSlices];
    unsigned m[kVoxelSlices];
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        s[k] = ok[k] ? row_ptr(a.disp, a.disp_step, sy[k])[sx[k]] : -32768;
        m[k] = ok[k] && a.mask ? row_ptr(a.mask, a.mask_step, sy[k])[sx[k]] : 0u;
    }
    // gates 3 to 5
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
        double f = sdf / tr;
        near[k] = f < 1.0;
        if (f > 1.0) f = 1.0;
        obs[k] = (int)floor(f * 32767.0 + 0.5);
        ok[k] = true;
    }
    // gate 6: the words of the voxels that passed, loaded together, then averaged and stored
    size_t slot[kVoxelSlices];
    uint32_t word[kVoxelSlices];
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        slot[k] = ok[k] ? voxel_slot(a.grid, rx, ry, rz0 + k) : 0;
        word[k] = ok[k] ? a.grid.voxels[slot[k]] : 0u;
    }
#pragma unroll
    for (int k = 0; k < kVoxelSlices; ++k) {
        if (ok[k]) {
            const long long t = (long long)(int16_t)(word[k] & 0xffffu), w = (long long)(word[k] >> 16);
            const long long num = 2 * (w * t + (long long)obs[k]) + (w + 1), den = 2 * (w + 1);
            const long long tn = num / den - ((num % den != 0) && (num < 0));   // floor division, den > 0
            const long long wn = w + 1 < (long long)a.p.max_weight ? w + 1 : (long long)a.p.max_weight;
            a.grid.voxels[slot[k]] = ((uint32_t)(uint16_t)(int16_t)tn) | ((uint32_t)wn << 16);
        }
        if (a.counts) {
            n_updated += (unsigned)__popcll(__ballot(ok[k]));
            n_near += (unsigned)__popcll(__ballot(ok[k] && near[k]));
        }
    }
    }                                         // the groups of slices
    if (!a.counts) return;                    // uniform over the grid
    if (lane == 0) { wave_counts[wave][0] = n_updated; wave_counts[wave][1] = n_near; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long u = (unsigned long long)wave_counts[0][0] + wave_counts[1][0] + wave_counts[2][0] + wave_counts[3][0];
        const unsigned long long n = (unsigned long long)wave_counts[0][1] + wave_counts[1][1] + wave_counts[2][1] + wave_counts[3][1];
        unsigned long long t0 = 0, t1 = 0;
        if (hand_over(reinterpret_cast<unsigned long long *>(a.counters), u | (n << 32), 0ull, gridDim.x * gridDim.y * gridDim.z, t0, t1)) {
            a.counts[0] = (int32_t)(unsigned)t0;
            a.counts[1] = (int32_t)(t0 >> 32);
        }
    }
}

__global__ __launch_bounds__(256) void voxel_raycast_kernel(VoxelRaycastArgs a) {
    __shared__ unsigned wave_counts[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 32 + wave * 8 + (lane & 7), y = blockIdx.y * 8 + (lane >> 3);   // a wave = an 8 x 8 tile
    const bool in = x < a.w && y < a.h;
    const double fxb = a.cam.fx * a.cam.baseline;
    const VoxelGrid &g = a.grid;
    const double hx = g.ox + (double)(g.nx - 2), hy = g.oy + (double)(g.ny - 2), hz = g.oz + (double)(g.nz - 2);   // the last i0 with both corners inside
    unsigned status = 0u, wout = 0u;
    int sout = -32768;
    bool live = in && !a.empty, have_prev = false;
    double Fp = 0.0, zp = 0.0;
#pragma unroll 1
    for (int k = 0; k <= a.steps; ++k) {
        if (!__any(live)) break;
        if (!live) continue;
        const double z = a.p.min_depth + (double)k * a.p.march_step;
        const WarpPoint pw = pose_carry(a.pose, WarpPoint{back_project_x(a.cam, x, z), back_project_y(a.cam, y, z), z});
        const double ax = pw.x / a.p.voxel_size - 0.5, ay = pw.y / a.p.voxel_size - 0.5, az = pw.z / a.p.voxel_size - 0.5;
        const double ix = floor(ax), iy = floor(ay), iz = floor(az);
        if (!(ix >= g.ox && ix <= hx && iy >= g.oy && iy <= hy && iz >= g.oz && iz <= hz)) {   // a NaN fails
            have_prev = false;
            continue;
        }
        const double frx = ax - ix, fry = ay - iy, frz = az - iz;
        const int x0 = wrap((int)(ix - g.ox) + g.mx, g.nx), y0 = wrap((int)(iy - g.oy) + g.my, g.ny), z0 = wrap((int)(iz - g.oz) + g.mz, g.nz);
        const int x1 = wrap(x0 + 1, g.nx), y1 = wrap(y0 + 1, g.ny), z1 = wrap(z0 + 1, g.nz);
        const uint32_t *r00 = g.voxels + ((size_t)z0 * g.ny + y0) * g.nx, *r10 = g.voxels + ((size_t)z0 * g.ny + y1) * g.nx;
        const uint32_t *r01 = g.voxels + ((size_t)z1 * g.ny + y0) * g.nx, *r11 = g.voxels + ((size_t)z1 * g.ny + y1) * g.nx;
        // the eight corners before the first use: v[dy][dz][dx]
        const uint32_t v000 = r00[x0], v001 = r00[x1], v010 = r01[x0], v011 = r01[x1];
        const uint32_t v100 = r10[x0], v101 = r10[x1], v110 = r11[x0], v111 = r11[x1];
        unsigned wmin = min(min(min(v000 >> 16, v001 >> 16), min(v010 >> 16, v011 >> 16)), min(min(v100 >> 16, v101 >> 16), min(v110 >> 16, v111 >> 16)));
        if (wmin < (unsigned)a.p.min_weight) {
            have_prev = false;
            continue;
        }
#define CART_VOX_T(v) ((int)(int16_t)((v) & 0xffffu))
        const double c00 = (double)CART_VOX_T(v000) + frx * (double)(CART_VOX_T(v001) - CART_VOX_T(v000));
        const double c01 = (double)CART_VOX_T(v010) + frx * (double)(CART_VOX_T(v011) - CART_VOX_T(v010));
        const double c10 = (double)CART_VOX_T(v100) + frx * (double)(CART_VOX_T(v101) - CART_VOX_T(v100));
        const double c11 = (double)CART_VOX_T(v110) + frx * (double)(CART_VOX_T(v111) - CART_VOX_T(v110));
#undef CART_VOX_T
        const double e0 = c00 + fry * (c10 - c00), e1 = c01 + fry * (c11 - c01);
        const double F = e0 + frz * (e1 - e0);
        if (F > 0.0) {
            have_prev = true; Fp = F; zp = z;
            continue;
        }
        live = false;                         // a known F <= 0 ends the ray
        if (!have_prev) { status = 2u; continue; }
        const double zs = zp + (a.p.march_step * Fp) / (Fp - F);
        const double swd = floor((fxb / zs) * 16.0 + 0.5);
        if (swd >= 1.0 && swd <= 32767.0) { sout = (int)swd; wout = wmin; status = 1u; }
    }
    if (in) {
        row_ptr(a.disp, a.disp_step, y)[x] = (int16_t)sout;
        if (a.weight) row_ptr(a.weight, a.weight_step, y)[x] = (uint16_t)wout;
        if (a.status) row_ptr(a.status, a.status_step, y)[x] = (uint8_t)status;
    }
    if (!a.counts) return;                    // uniform over the grid
    const unsigned cls = in ? status : 3u;
    unsigned n[3];
#pragma unroll
    for (unsigned k = 0; k < 3u; ++k) n[k] = (unsigned)__popcll(__ballot(cls == k));
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) wave_counts[wave][k] = n[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = (unsigned long long)wave_counts[0][k] + wave_counts[1][k] + wave_counts[2][k] + wave_counts[3][k];
        unsigned long long t0 = 0, t1 = 0;
        if (hand_over(reinterpret_cast<unsigned long long *>(a.counters) + 2, t[0] | (t[1] << 32), t[2], gridDim.x * gridDim.y, t0, t1)) {
            a.counts[0] = (int32_t)(unsigned)t0;
            a.counts[1] = (int32_t)(t0 >> 32);
            a.counts[2] = (int32_t)(unsigned)t1;
        }
    }
}

}  // namespace

void launch_voxel_clear(const VoxelGrid &grid, int rx0, int rw, int ry0, int rh, int rz0, int rd, hipStream_t s) {
    if (rw <= 0 || rh <= 0 || rd <= 0) return;
    const size_t n = (size_t)(rw / 4) * rh * rd;   // at most 2^24
    hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, grid, rx0, rw / 4, ry0, rh, rz0, rd);
}

void launch_voxel_integrate(const VoxelIntegrateArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(voxel_integrate_kernel, dim3((unsigned)((a.grid.nx + 63) / 64), (unsigned)(a.grid.ny / 4), (unsigned)((a.grid.nz + kVoxelDepth - 1) / kVoxelDepth)), dim3(256), 0, s, a);
}

void launch_voxel_raycast(const VoxelRaycastArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(voxel_raycast_kernel, dim3((unsigned)((a.w + 31) / 32), (unsigned)((a.h + 7) / 8)), dim3(256), 0, s, a);
}

}  // namespace cart_amd

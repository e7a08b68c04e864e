// voxel_sample.h -- one trilinear sample of the TSDF volume with its gradient (spec S34; the sampling rule is S33's
// raycast's): the eight corners i0 + {0,1}^3 around a world point, gathered from the toroidal storage, then the value F and the gradient
// g = dF / d(voxel index) in tsdf units.  Two steps, so that a caller can issue the gathers of several samples before the first use.
// fp64 with + - * / floor only, every expression in the written order.  Device only; included by modeltrack_kernels.hip.
#pragma once

#include "engine_internal.h"
#include "warp_device.h"

#pragma clang fp contract(off)

namespace cart_amd {

struct VoxelCorners {
    uint32_t v[2][2][2];       // [dy][dz][dx]: tsdf in the low half, weight in the high half
    double frx, fry, frz;
    bool inside;               // all eight corners lie in the window
};

struct VoxelSample { double F, gx, gy, gz; };

__device__ __forceinline__ int voxel_wrap(int v, int n) { return v >= n ? v - n : v; }

// a = p / voxel_size - 0.5, i0 = floor(a), fr = a - i0 per axis; the corners are loaded iff all eight lie in the window (compared as
// doubles: a NaN fails).  `want` false skips the sample (no load, inside = false).
__device__ __forceinline__ void voxel_gather(const VoxelGrid &g, double voxel_size, WarpPoint p, bool want, VoxelCorners &c) {
    const double hx = g.ox + (double)(g.nx - 2), hy = g.oy + (double)(g.ny - 2), hz = g.oz + (double)(g.nz - 2);   // the last i0 with both corners inside
    const double ax = p.x / voxel_size - 0.5, ay = p.y / voxel_size - 0.5, az = p.z / voxel_size - 0.5;
    const double ix = floor(ax), iy = floor(ay), iz = floor(az);
    c.inside = want && ix >= g.ox && ix <= hx && iy >= g.oy && iy <= hy && iz >= g.oz && iz <= hz;
    c.frx = ax - ix; c.fry = ay - iy; c.frz = az - iz;
    // outside: slot 0 of the storage, a valid address whose value is not used
    const int x0 = c.inside ? voxel_wrap((int)(ix - g.ox) + g.mx, g.nx) : 0, y0 = c.inside ? voxel_wrap((int)(iy - g.oy) + g.my, g.ny) : 0;
    const int z0 = c.inside ? voxel_wrap((int)(iz - g.oz) + g.mz, g.nz) : 0;
    const int x1 = c.inside ? voxel_wrap(x0 + 1, g.nx) : 0, y1 = c.inside ? voxel_wrap(y0 + 1, g.ny) : 0, z1 = c.inside ? voxel_wrap(z0 + 1, g.nz) : 0;
    const uint32_t *r00 = g.voxels + ((size_t)z0 * g.ny + y0) * g.nx, *r10 = g.voxels + ((size_t)z0 * g.ny + y1) * g.nx;
    const uint32_t *r01 = g.voxels + ((size_t)z1 * g.ny + y0) * g.nx, *r11 = g.voxels + ((size_t)z1 * g.ny + y1) * g.nx;
    // the eight corners before the first use
    c.v[0][0][0] = r00[x0]; c.v[0][0][1] = r00[x1]; c.v[0][1][0] = r01[x0]; c.v[0][1][1] = r01[x1];
    c.v[1][0][0] = r10[x0]; c.v[1][0][1] = r10[x1]; c.v[1][1][0] = r11[x0]; c.v[1][1][1] = r11[x1];
}

// The sample is known iff the corners were inside and each has weight >= min_weight; then s holds F (S33's trilinear form, unchanged) and
// the gradient: gz = e1 - e0, gy = h0 + fr_z (h1 - h0) over the y differences of c, gx = a0 + fr_z (a1 - a0) over the integer x differences.
__device__ __forceinline__ bool voxel_value(const VoxelCorners &c, int min_weight, VoxelSample &s) {
    unsigned wmin = 65535u;
    int t[2][2][2];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t v = c.v[k >> 2][(k >> 1) & 1][k & 1];
        wmin = min(wmin, v >> 16);
        t[k >> 2][(k >> 1) & 1][k & 1] = (int)(int16_t)(v & 0xffffu);
    }
    if (!c.inside || wmin < (unsigned)min_weight) return false;
    const double d00 = (double)(t[0][0][1] - t[0][0][0]), d01 = (double)(t[0][1][1] - t[0][1][0]);   // D[dy][dz]
    const double d10 = (double)(t[1][0][1] - t[1][0][0]), d11 = (double)(t[1][1][1] - t[1][1][0]);
    const double c00 = (double)t[0][0][0] + c.frx * d00, c01 = (double)t[0][1][0] + c.frx * d01;
    const double c10 = (double)t[1][0][0] + c.frx * d10, c11 = (double)t[1][1][0] + c.frx * d11;
    const double h0 = c10 - c00, h1 = c11 - c01;
    const double e0 = c00 + c.fry * h0, e1 = c01 + c.fry * h1;
    s.gz = e1 - e0;
    s.F = e0 + c.frz * s.gz;
    s.gy = h0 + c.frz * (h1 - h0);
    const double a0 = d00 + c.fry * (d10 - d00), a1 = d01 + c.fry * (d11 - d01);
    s.gx = a0 + c.frz * (a1 - a0);
    return true;
}

}  // namespace cart_amd

// color_sample.h -- one trilinear sample of the colour volume's luminance with its gradient (spec S38): the eight corners
// i0 + {0,1}^3 around a world point, gathered from the colour object's own toroidal storage, then the value C of t = b + 2 g + r
// (0 .. 1020) and the gradient gc = dC / d(voxel index).  The arithmetic is voxel_sample.h's voxel_value word for word on other integers;
// the gather differs in one point: a sample that is not wanted or lies outside loads nothing at all (with photo_weight == 0 the colour
// volume is not read).  Two steps, so that a caller can issue the gathers before the first use.
// fp64 with + - * / floor only, every expression in the written order.  Device only; included by modeltrack_color_kernels.hip.
#pragma once

#include "engine_internal.h"
#include "voxel_sample.h"

#pragma clang fp contract(off)

namespace cart_amd {

// voxel_gather's index rule against the colour grid `g`; c.v holds the colour words b | g << 8 | r << 16 | weight << 24, or zeros.
__device__ __forceinline__ void color_gather(const VoxelGrid &g, double voxel_size, WarpPoint p, bool want, VoxelCorners &c) {
    const double hx = g.ox + (double)(g.nx - 2), hy = g.oy + (double)(g.ny - 2), hz = g.oz + (double)(g.nz - 2);   // the last i0 with both corners inside
    const double ax = p.x / voxel_size - 0.5, ay = p.y / voxel_size - 0.5, az = p.z / voxel_size - 0.5;
    const double ix = floor(ax), iy = floor(ay), iz = floor(az);
    c.inside = want && ix >= g.ox && ix <= hx && iy >= g.oy && iy <= hy && iz >= g.oz && iz <= hz;
    c.frx = ax - ix; c.fry = ay - iy; c.frz = az - iz;
#pragma unroll
    for (int k = 0; k < 8; ++k) c.v[k >> 2][(k >> 1) & 1][k & 1] = 0u;
    if (!c.inside) return;
    const int x0 = voxel_wrap((int)(ix - g.ox) + g.mx, g.nx), y0 = voxel_wrap((int)(iy - g.oy) + g.my, g.ny), z0 = voxel_wrap((int)(iz - g.oz) + g.mz, g.nz);
    const int x1 = voxel_wrap(x0 + 1, g.nx), y1 = voxel_wrap(y0 + 1, g.ny), z1 = voxel_wrap(z0 + 1, g.nz);
    const uint32_t *r00 = g.voxels + ((size_t)z0 * g.ny + y0) * g.nx, *r10 = g.voxels + ((size_t)z0 * g.ny + y1) * g.nx;
    const uint32_t *r01 = g.voxels + ((size_t)z1 * g.ny + y0) * g.nx, *r11 = g.voxels + ((size_t)z1 * g.ny + y1) * g.nx;
    // [dy][dz][dx], the eight corners before the first use
    c.v[0][0][0] = r00[x0]; c.v[0][0][1] = r00[x1]; c.v[0][1][0] = r01[x0]; c.v[0][1][1] = r01[x1];
    c.v[1][0][0] = r10[x0]; c.v[1][0][1] = r10[x1]; c.v[1][1][0] = r11[x0]; c.v[1][1][1] = r11[x1];
}

// The sample is known iff the corners were inside and each has weight >= min_weight; then s.F holds C and (s.gx, s.gy, s.gz) holds gc.
__device__ __forceinline__ bool color_value(const VoxelCorners &c, int min_weight, VoxelSample &s) {
    unsigned wmin = 255u;
    int t[2][2][2];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t v = c.v[k >> 2][(k >> 1) & 1][k & 1];
        wmin = min(wmin, v >> 24);
        t[k >> 2][(k >> 1) & 1][k & 1] = (int)(v & 0xffu) + 2 * (int)((v >> 8) & 0xffu) + (int)((v >> 16) & 0xffu);
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

// warp_device.h -- the pose-warp chain of the plane map, motion segmentation, dense ego-motion and temporal fusion kernels (spec S24 - S28):
// packed flow -> previous pixel, pixel + disparity -> camera-frame point, point -> through a 3 x 4 row-major pose, point -> pixel.
//
// The association order below IS the spec: these kernels are compared bit for bit against the oracle, so every helper keeps its expression
// parenthesis for parenthesis.  fp64 with + - * / only; the library is built with -ffp-contract=off, so every product and sum is rounded
// on its own:
//   back-project  Z = fxb / d,  X = ((u - cx) * Z) / fx,  Y = ((v - cy) * Z) / fy          (fxb = fx * baseline, d = disparity in pixels)
//   carry         q_r = ((P[4r] * X + P[4r + 1] * Y) + P[4r + 2] * Z) + P[4r + 3]          (r = 0, 1, 2)
//   project       u = (fx * q_x) / q_z + cx,  v = (fy * q_y) / q_z + cy
// Device only; included by planemap_kernels.hip, motion_kernels.hip, dense_ego_kernels.hip, fusion_kernels.hip, localba_kernels.hip and voxel_sample.h / modeltrack_kernels.hip.
#pragma once

#include "engine_internal.h"

namespace cart_amd {

struct WarpPoint { double x, y, z; };

template <typename T>
__device__ __forceinline__ T *row_ptr(T *base, size_t step, int y) {   // pitched rows are addressed in bytes
    return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(base) + (size_t)y * step);
}

// Packed S10.5 flow word (x in the low half, y in the high half): previous position = p - (flow >> 5), arithmetic shift per component.
__device__ __forceinline__ int2 flow_previous(int fl, int x, int y) { return make_int2(x - ((int)(int16_t)(fl & 0xffff) >> 5), y - (fl >> 21)); }

// Back-projection, one coordinate at a time for the caller that gates between them (plane_map's vote_key).
__device__ __forceinline__ double back_project_x(const cart_ego_camera &cam, int u, double Z) { return (((double)u - cam.cx) * Z) / cam.fx; }
__device__ __forceinline__ double back_project_y(const cart_ego_camera &cam, int v, double Z) { return (((double)v - cam.cy) * Z) / cam.fy; }

__device__ __forceinline__ WarpPoint back_project(const cart_ego_camera &cam, double fxb, int u, int v, double d) {
    const double Z = fxb / d;
    return WarpPoint{back_project_x(cam, u, Z), back_project_y(cam, v, Z), Z};
}

// The same for a position between pixels (a keypoint of spec S32): the operations and their order are the ones above.
__device__ __forceinline__ WarpPoint back_project(const cart_ego_camera &cam, double fxb, double u, double v, double d) {
    const double Z = fxb / d;
    return WarpPoint{((u - cam.cx) * Z) / cam.fx, ((v - cam.cy) * Z) / cam.fy, Z};
}

// Row r of the 3 x 4 row-major pose P applied to p, and all three.
__device__ __forceinline__ double pose_row(const double *P, int r, WarpPoint p) {
    return ((P[4 * r] * p.x + P[4 * r + 1] * p.y) + P[4 * r + 2] * p.z) + P[4 * r + 3];
}

__device__ __forceinline__ WarpPoint pose_carry(const double *P, WarpPoint p) { return WarpPoint{pose_row(P, 0, p), pose_row(P, 1, p), pose_row(P, 2, p)}; }

// Pinhole projection of q, one image coordinate at a time.
__device__ __forceinline__ double project_u(const cart_ego_camera &cam, WarpPoint q) { return (cam.fx * q.x) / q.z + cam.cx; }
__device__ __forceinline__ double project_v(const cart_ego_camera &cam, WarpPoint q) { return (cam.fy * q.y) / q.z + cam.cy; }

}  // namespace cart_amd

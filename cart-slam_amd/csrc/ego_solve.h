// ego_solve.h -- the Gauss-Newton step of the pose refinements (spec S23, shared by S26): the unpivoted Cholesky solve of the 6 x 6
// normal equations and the quaternion pose update.  Included by ego_kernels.hip, dense_ego_kernels.hip and modeltrack_kernels.hip; IEEE double in the spec's
// operation order, no FMA contraction.
#pragma once

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace cart_amd {

// unpivoted Cholesky of the symmetric 6 x 6 system H x = -g (upper entries of H); false at a pivot that is not > 0
__device__ inline bool ego_solve6(const double H[6][6], const double g[6], double x[6]) {
    double L[6][6];
    for (int j = 0; j < 6; ++j) {
        double s = H[j][j];
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0)) return false;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
            s = H[j][i];
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

// R <- Rq R, t <- Rq t + upsilon, Rq = the rotation of the unit quaternion (1, omega / 2) / |(1, omega / 2)|
__device__ inline void ego_update(const double d[6], double R[9], double t[3]) {
    const double hx = 0.5 * d[0], hy = 0.5 * d[1], hz = 0.5 * d[2];
    const double s = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double w = 1.0 / s, x = hx / s, y = hy / s, z = hz / s;
    const double Rq[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                          2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                          2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    double Rn[9], tn[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (Rq[3 * r] * R[c] + Rq[3 * r + 1] * R[3 + c]) + Rq[3 * r + 2] * R[6 + c];
        tn[r] = ((Rq[3 * r] * t[0] + Rq[3 * r + 1] * t[1]) + Rq[3 * r + 2] * t[2]) + d[3 + r];
    }
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
}

// the right-multiplying form (spec S29): R <- R Rq, t <- t + R upsilon with the R from before the update
__device__ inline void ego_update_right(const double d[6], double R[9], double t[3]) {
    const double hx = 0.5 * d[0], hy = 0.5 * d[1], hz = 0.5 * d[2];
    const double s = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double w = 1.0 / s, x = hx / s, y = hy / s, z = hz / s;
    const double Rq[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                          2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                          2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    double Rn[9], tn[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (R[3 * r] * Rq[c] + R[3 * r + 1] * Rq[3 + c]) + R[3 * r + 2] * Rq[6 + c];
        tn[r] = t[r] + ((R[3 * r] * d[3] + R[3 * r + 1] * d[4]) + R[3 * r + 2] * d[5]);
    }
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
}

}  // namespace cart_amd

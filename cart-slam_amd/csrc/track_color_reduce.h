// track_color_reduce.h -- the workgroup level of the S26 summation order for the 29 fp64 sums and three counts of spec S38
// (modeltrack_color_kernels.hip): the ascending butterfly v[l] += v[l ^ o], o = 1, 2, .. 128, over the workgroup's 256 lanes, as
// dense_reduce.h does it for 28 sums and two counts.  Device only.
#pragma once

#include "engine_internal.h"

#pragma clang fp contract(off)

namespace cart_amd {

// Lane 0 of the ascending butterfly over the workgroup's 256 lanes, for every sum and the three counts: on return lanes 0 .. 28 hold the
// total of sum `lane` in tot, and every lane holds the counts.
__device__ __forceinline__ void track_color_reduce(double (&acc)[kTrackColorSums], int &cnt, int &ncand, int &nphoto, double &tot) {
    __shared__ double s_w[kTrackColorSums][4];
    __shared__ int s_c[3][4];
    const int lane = threadIdx.x, wave = lane >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int k = 0; k < kTrackColorSums; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], o);
        cnt += __shfl_xor(cnt, o);
        ncand += __shfl_xor(ncand, o);
        nphoto += __shfl_xor(nphoto, o);
    }
    if ((lane & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kTrackColorSums; ++k) s_w[k][wave] = acc[k];
        s_c[0][wave] = cnt;
        s_c[1][wave] = ncand;
        s_c[2][wave] = nphoto;
    }
    __syncthreads();
    tot = 0.0;
    if (lane < kTrackColorSums) tot = (s_w[lane][0] + s_w[lane][1]) + (s_w[lane][2] + s_w[lane][3]);   // o = 64, then o = 128
    cnt = (s_c[0][0] + s_c[0][1]) + (s_c[0][2] + s_c[0][3]);
    ncand = (s_c[1][0] + s_c[1][1]) + (s_c[1][2] + s_c[1][3]);
    nphoto = (s_c[2][0] + s_c[2][1]) + (s_c[2][2] + s_c[2][3]);
}

}  // namespace cart_amd

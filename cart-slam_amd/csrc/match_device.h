// match_device.h -- what the kernels that compare 256-bit ORB descriptors share (match_kernels.hip: S22, place_kernels.hip: S27): the
// packed key (distance << 16 | column), the descriptor load, the Hamming distance and the best / second update.  The tile and row
// constants (kMatchRows, kMatchTile) are engine_internal.h's.
#pragma once

#include "engine_internal.h"

namespace cart_amd {

constexpr int kNoKey = 0x7fffffff;   // no admissible column yet: distance field 0x7fff
constexpr int kNoDist = 0x7fff;

__device__ __forceinline__ int clamp_count(const int32_t *p, int cap) { return min(max(*p, 0), cap); }

// 32 descriptor bytes as 8 little-endian dwords (dword loads when pointer and step allow them)
__device__ __forceinline__ void load_desc(const uint8_t *row, bool aligned, unsigned v[8]) {
    if (aligned) {
        const unsigned *p = reinterpret_cast<const unsigned *>(row);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[k];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = (unsigned)row[4 * k] | ((unsigned)row[4 * k + 1] << 8) | ((unsigned)row[4 * k + 2] << 16) | ((unsigned)row[4 * k + 3] << 24);
    }
}

__device__ __forceinline__ bool desc_aligned(const uint8_t *base, size_t step) { return ((reinterpret_cast<uintptr_t>(base) | step) & 3) == 0; }

// popcount(q xor t), t as the two halves of a staged row
__device__ __forceinline__ int hamming256(const unsigned q[8], const uint4 &lo, const uint4 &hi) {
    return __popc(q[0] ^ lo.x) + __popc(q[1] ^ lo.y) + __popc(q[2] ^ lo.z) + __popc(q[3] ^ lo.w) +
           __popc(q[4] ^ hi.x) + __popc(q[5] ^ hi.y) + __popc(q[6] ^ hi.z) + __popc(q[7] ^ hi.w);
}

// the loser of (best, key) is a candidate for the second distance
__device__ __forceinline__ void match_update(int &best, int &second, int key) {
    second = min(second, max(best, key) >> 16);
    best = min(best, key);
}

}  // namespace cart_amd

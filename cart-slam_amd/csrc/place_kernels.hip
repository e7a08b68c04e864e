// place_kernels.hip -- place recognition over the keyframe ring.  One query is two launches:
//   place_score   match_pairs' body with the slot as a grid axis: one lane per query (kPlaceLaneQueries of them), the slot's descriptors
//                 streamed through LDS in tiles of kMatchTile, no train chunks; at the end of the slot every lane applies the vote rule
//                 and the workgroup stores its vote count to partial[query block][slot].  A workgroup on an ineligible or empty slot,
//                 or beyond the query count, leaves at once and stores nothing.
//   place_select  one workgroup, one thread per slot: sums the partials that place_score wrote, writes the scores, and picks the
//                 candidates by repeated arg-max under (score desc, frame id asc, slot asc).
// place_insert copies a frame into its slot and writes the slot's header, so eligibility is decided from device memory.
#include "match_device.h"

namespace cart_amd {

namespace {
__device__ __forceinline__ bool place_eligible(const PlaceSlotHeader &h, uint64_t frame_id, uint64_t min_gap) {
    const uint64_t sum = h.frame_id + min_gap;
    return (h.flags & kPlaceOccupied) && sum >= h.frame_id && sum <= frame_id;   // sum < frame_id_k: the addition wrapped
}

__global__ __launch_bounds__(kMatchRows) void place_score_kernel(PlaceQueryArgs a) {
    __shared__ uint4 s_desc[kMatchTile][2];
    __shared__ int s_votes[kMatchRows / 64];
    const int slot = blockIdx.y;
    const int nq = clamp_count(a.q_count, a.db.max_features);
    const int row0 = blockIdx.x * kPlaceRows;
    if (row0 >= nq) return;   // uniform, as the two below
    const PlaceSlotHeader h = a.db.hdr[slot];
    if (!place_eligible(h, a.frame_id, a.p.min_gap)) return;
    const int nt = h.count;   // clamped by place_insert
    if (nt == 0) return;
    unsigned q[kPlaceLaneQueries][8] = {};
    bool live[kPlaceLaneQueries];
    const bool q_aligned = desc_aligned(a.q_desc, a.q_step);
#pragma unroll
    for (int u = 0; u < kPlaceLaneQueries; ++u) {
        const int row = row0 + u * kMatchRows + threadIdx.x;
        live[u] = row < nq;
        if (live[u]) load_desc(a.q_desc + (size_t)row * a.q_step, q_aligned, q[u]);
    }
    const uint4 *train = reinterpret_cast<const uint4 *>(a.db.desc + (size_t)slot * a.db.max_features * CART_ORB_DESCRIPTOR_BYTES);
    int best[kPlaceLaneQueries], second[kPlaceLaneQueries];
#pragma unroll
    for (int u = 0; u < kPlaceLaneQueries; ++u) { best[u] = kNoKey; second[u] = kNoDist; }
    for (int c0 = 0; c0 < nt; c0 += kMatchTile) {
        const int n = min(kMatchTile, nt - c0);   // uniform
        __syncthreads();
        for (int v = threadIdx.x; v < 2 * n; v += kMatchRows) (&s_desc[0][0])[v] = train[2 * (size_t)c0 + v];   // the ring's rows are tight
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            const uint4 lo = s_desc[t][0], hi = s_desc[t][1];
#pragma unroll
            for (int u = 0; u < kPlaceLaneQueries; ++u) match_update(best[u], second[u], (hamming256(q[u], lo, hi) << 16) | (c0 + t));
        }
    }
    int votes = 0;
#pragma unroll
    for (int u = 0; u < kPlaceLaneQueries; ++u) {
        const int d1 = best[u] >> 16, d2 = second[u] > 256 ? -1 : second[u];   // nt > 0 and no gate: every live query has a j1
        const bool vote = live[u] && d1 <= a.p.max_distance && (a.p.ratio == 0 || d2 < 0 || 100 * d1 < a.p.ratio * d2);
        votes += __popcll(__ballot(vote));
    }
    if ((threadIdx.x & 63) == 0) s_votes[threadIdx.x >> 6] = votes;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kMatchRows / 64; ++w) total += s_votes[w];
        a.partial[(size_t)blockIdx.x * a.db.capacity + slot] = total;
    }
}

struct PlaceKey {   // the order of the candidate list
    int score, slot;
    uint64_t frame_id;
};
__device__ __forceinline__ bool place_before(const PlaceKey &x, const PlaceKey &y) {
    return x.score != y.score ? x.score > y.score : x.frame_id != y.frame_id ? x.frame_id < y.frame_id : x.slot < y.slot;
}

__global__ __launch_bounds__(kPlaceMaxSlots) void place_select_kernel(PlaceQueryArgs a) {
    __shared__ PlaceKey s_best[kPlaceMaxSlots / 64];
    const int k = threadIdx.x;
    const int nq = clamp_count(a.q_count, a.db.max_features);
    const int blocks = (nq + kPlaceRows - 1) / kPlaceRows;
    PlaceKey mine{-1, k, 0};
    if (k < a.db.capacity) {
        const PlaceSlotHeader h = a.db.hdr[k];
        if (place_eligible(h, a.frame_id, a.p.min_gap)) {
            mine.score = 0;
            mine.frame_id = h.frame_id;
            if (h.count > 0)   // exactly the partials that place_score stored
                for (int b = 0; b < blocks; ++b) mine.score += a.partial[(size_t)b * a.db.capacity + k];
        }
        if (a.scores) a.scores[k] = mine.score;
    }
    if (mine.score < a.p.min_score) mine.score = -1;   // min_score >= 0: -1 marks what is no candidate (any more)
    int found = 0;
    for (int r = 0; r < a.p.max_candidates; ++r) {   // uniform
        PlaceKey b = mine;
        for (int o = 32; o; o >>= 1) {
            const PlaceKey x{__shfl_xor(b.score, o), __shfl_xor(b.slot, o), __shfl_xor(b.frame_id, o)};
            if (place_before(x, b)) b = x;
        }
        if ((k & 63) == 0) s_best[k >> 6] = b;
        __syncthreads();
        b = s_best[0];
        for (int w = 1; w < kPlaceMaxSlots / 64; ++w)
            if (place_before(s_best[w], b)) b = s_best[w];
        __syncthreads();
        if (b.score < 0) break;   // uniform: every thread read the same table
        if (k == b.slot) {
            a.candidates[r] = cart_place_candidate{b.slot, b.score, b.frame_id};
            mine.score = -1;
        }
        ++found;
    }
    if (k == 0) *a.n_candidates = found;
}

__global__ __launch_bounds__(256) void place_insert_kernel(PlaceInsertArgs a) {
    const int n = clamp_count(a.count, a.db.max_features);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) a.db.hdr[a.slot] = PlaceSlotHeader{n, kPlaceOccupied | (a.landmarks ? kPlaceHasLandmarks : 0), a.frame_id};
    if (i >= n) return;
    const size_t row = (size_t)a.slot * a.db.max_features + i;
    unsigned v[8];
    load_desc(a.desc + (size_t)i * a.desc_step, desc_aligned(a.desc, a.desc_step), v);
    uint4 *d = reinterpret_cast<uint4 *>(a.db.desc + row * CART_ORB_DESCRIPTOR_BYTES);
    d[0] = make_uint4(v[0], v[1], v[2], v[3]);
    d[1] = make_uint4(v[4], v[5], v[6], v[7]);
    a.db.kp[row] = a.kp[i];
    if (a.landmarks) {
#pragma unroll
        for (int c = 0; c < 4; ++c) a.db.landmarks[4 * row + c] = a.landmarks[4 * (size_t)i + c];
    }
}
}  // namespace

void launch_place_insert(const PlaceInsertArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(place_insert_kernel, dim3((a.db.max_features + 255) / 256), dim3(256), 0, s, a);
}

void launch_place_query(const PlaceQueryArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(place_score_kernel, dim3((a.db.max_features + kPlaceRows - 1) / kPlaceRows, a.db.capacity), dim3(kMatchRows), 0, s, a);
    hipLaunchKernelGGL(place_select_kernel, dim3(1), dim3(kPlaceMaxSlots), 0, s, a);
}

}  // namespace cart_amd

// match_kernels.hip -- brute-force matching of 256-bit ORB descriptors.  Three launches per call:
//   match_pairs  one lane per ROW descriptor, the COLUMN set streamed through LDS in tiles of kMatchTile (every lane reads the same
//                LDS address: a broadcast); grid = row blocks x column chunks x directions.  Direction 0 has the queries as rows
//                (forward table: best key and second distance), direction 1 the train set as rows (backward table: best key).
//                Each workgroup writes its rows' partials of its chunk.
//   match_merge  folds the partials of a row in chunk order into the forward records / the backward best query.
//   match_select acceptance rule and the ordered compaction, one workgroup of 1024 threads.
// The set sizes are read on the device; the grids are sized by the matcher's capacity and surplus workgroups leave at once.
#include "match_device.h"

namespace cart_amd {

namespace {
struct MatchSide {
    const uint8_t *desc; size_t step;
    const cart_keypoint *kp;
};

// kSwap = false: rows are the queries (dx = row - column); true: rows are the train set (dx = column - row)
template <bool kSwap>
__device__ __forceinline__ void match_rows(const MatchArgs &a, const MatchSide &R, int nrows, const MatchSide &Cs, int ncols, int chunk) {
    __shared__ uint4 s_desc[kMatchTile][2];
    __shared__ float4 s_gate[kMatchTile];   // x, y, octave bits, unused
    const int row = blockIdx.x * kMatchRows + threadIdx.x;
    const bool live = row < nrows;
    const bool gate = a.p.use_gate != 0;
    unsigned q[8] = {};
    float qx = 0.f, qy = 0.f;
    int qo = 0;
    if (live) {
        load_desc(R.desc + (size_t)row * R.step, desc_aligned(R.desc, R.step), q);
        if (gate) { qx = R.kp[row].x; qy = R.kp[row].y; qo = R.kp[row].octave; }
    }
    const bool c_aligned = desc_aligned(Cs.desc, Cs.step);
    const int col_end = min(ncols, (chunk + 1) * a.chunk_len);
    int best = kNoKey, second = kNoDist;
    for (int c0 = chunk * a.chunk_len; c0 < col_end; c0 += kMatchTile) {
        const int nt = min(kMatchTile, col_end - c0);   // uniform
        __syncthreads();
        for (int t = threadIdx.x; t < nt; t += kMatchRows) {
            unsigned v[8];
            load_desc(Cs.desc + (size_t)(c0 + t) * Cs.step, c_aligned, v);
            s_desc[t][0] = make_uint4(v[0], v[1], v[2], v[3]);
            s_desc[t][1] = make_uint4(v[4], v[5], v[6], v[7]);
            if (gate) s_gate[t] = make_float4(Cs.kp[c0 + t].x, Cs.kp[c0 + t].y, __int_as_float(Cs.kp[c0 + t].octave), 0.f);
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const uint4 lo = s_desc[t][0], hi = s_desc[t][1];
            int d = hamming256(q, lo, hi);
            if (gate) {   // uniform
                const float4 g = s_gate[t];
                const float dx = kSwap ? g.x - qx : qx - g.x, dy = kSwap ? g.y - qy : qy - g.y;   // one float32 subtraction each (S22)
                const int od = abs(qo - __float_as_int(g.z));
                const bool ok = a.p.dx_min <= dx && dx <= a.p.dx_max && a.p.dy_min <= dy && dy <= a.p.dy_max &&   // false for NaN
                                (a.p.max_octave_diff < 0 || od <= a.p.max_octave_diff);
                d = ok ? d : kNoDist;
            }
            match_update(best, second, (d << 16) | (c0 + t));
        }
    }
    if (!live) return;
    if (kSwap) a.bwd_part[(size_t)chunk * a.cap + row] = best;
    else a.fwd_part[(size_t)chunk * a.cap + row] = make_int2(best, second);
}

__global__ __launch_bounds__(kMatchRows) void match_pairs_kernel(MatchArgs a) {
    const int nq = clamp_count(a.q_count, a.cap), nt = clamp_count(a.t_count, a.cap);
    const bool swap = blockIdx.z != 0;
    const int nrows = swap ? nt : nq, ncols = swap ? nq : nt;
    const int chunk = blockIdx.y;
    if ((int)blockIdx.x * kMatchRows >= nrows || chunk * a.chunk_len >= ncols) return;   // uniform
    const MatchSide Q{a.q_desc, a.q_step, a.q_kp}, T{a.t_desc, a.t_step, a.t_kp};
    if (swap) match_rows<true>(a, T, nrows, Q, ncols, chunk);
    else match_rows<false>(a, Q, nrows, T, ncols, chunk);
}

// fwd[i] = (j1, d1, d2, -1), bwd[j] = i1(j) or -1
__global__ __launch_bounds__(256) void match_merge_kernel(MatchArgs a) {
    const int nq = clamp_count(a.q_count, a.cap), nt = clamp_count(a.t_count, a.cap);
    const bool swap = blockIdx.y != 0;
    const int nrows = swap ? nt : nq, ncols = swap ? nq : nt;
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= nrows) return;
    const int chunks = (ncols + a.chunk_len - 1) / a.chunk_len;
    int best = kNoKey, second = kNoDist;
    for (int c = 0; c < chunks; ++c) {
        int key, sec = kNoDist;
        if (swap) key = a.bwd_part[(size_t)c * a.cap + row];
        else { const int2 p = a.fwd_part[(size_t)c * a.cap + row]; key = p.x; sec = p.y; }
        second = min(min(second, sec), max(best, key) >> 16);
        best = min(best, key);
    }
    const bool none = (best >> 16) > 256;
    if (swap) a.bwd[row] = none ? -1 : (best & 0xffff);
    else a.fwd[row] = none ? make_int4(-1, -1, -1, -1) : make_int4(best & 0xffff, best >> 16, second > 256 ? -1 : second, -1);
}

constexpr int kSelectThreads = 1024;
__global__ __launch_bounds__(kSelectThreads) void match_select_kernel(MatchArgs a) {
    __shared__ int s_wave[kSelectThreads / 64];
    __shared__ int s_base;
    const int nq = clamp_count(a.q_count, a.cap);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < nq; i0 += kSelectThreads) {   // uniform
        const int i = i0 + threadIdx.x;
        int4 f = make_int4(-1, -1, -1, -1);
        bool ok = false;
        if (i < nq) {
            f = a.fwd[i];
            if (a.p.cross_check && f.x >= 0) f.w = a.bwd[f.x];
            ok = f.x >= 0 && f.y <= a.p.max_distance && (a.p.ratio == 0 || f.z < 0 || 100 * f.y < a.p.ratio * f.z) &&
                 (!a.p.cross_check || f.w == i);
            if (a.forward) {   // the caller's table is only 4-byte aligned
                int32_t *o = a.forward + 4 * (size_t)i;
                o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = f.w;
            }
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = s_base, total = 0;
        for (int w = 0; w < kSelectThreads / 64; ++w) {
            const int n = s_wave[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (ok) a.matches[before + __popcll(m & ((1ull << lane) - 1))] = cart_match{i, f.x, f.y, f.z};
        __syncthreads();
        if (threadIdx.x == 0) s_base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *a.match_count = s_base;
}
}  // namespace

void launch_match(const MatchArgs &a, hipStream_t s) {
    const int chunks = (a.cap + a.chunk_len - 1) / a.chunk_len;
    const int dirs = a.p.cross_check ? 2 : 1;
    hipLaunchKernelGGL(match_pairs_kernel, dim3((a.cap + kMatchRows - 1) / kMatchRows, chunks, dirs), dim3(kMatchRows), 0, s, a);
    hipLaunchKernelGGL(match_merge_kernel, dim3((a.cap + 255) / 256, dirs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(match_select_kernel, dim3(1), dim3(kSelectThreads), 0, s, a);
}

}  // namespace cart_amd

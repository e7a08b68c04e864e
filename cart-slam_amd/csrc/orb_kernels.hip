// orb_kernels.hip -- ORB keypoints and steered-BRIEF descriptors, replacing cv::cuda::ORB's
// detectAndComputeAsync in ImageFeatureDetectorModule (src/modules/features.cpp:48-66).  Both images of a stereo pair go
// through every launch: pyramid (one launch per level), detect (FAST-9 + NMS + Harris over every image / level / tile),
// select (exact top-n_l per image and level) and describe (one wave per keypoint).
#include <climits>

#include "engine_internal.h"

namespace cart_amd {

namespace {
constexpr int kFastT = 20;
constexpr int kHalo = 4;   // FAST reads +-3 around the tile plus its 1-pixel score ring; Harris reads +-4
constexpr int kLdsW = kOrbTileW + 2 * kHalo, kLdsH = kOrbTileH + 2 * kHalo;
constexpr int kSelThreads = 1024;
constexpr int kSelFinish = 2048;   // radix passes stop once this few keys share the selected prefix
constexpr int kSelChunk = 2048;

__constant__ int8_t c_circle[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3},
                                       {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};
__constant__ int8_t c_umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
// boundary rays B_j = round(2^20 (cos, sin)((12j + 6) deg)), half away from zero (tests/test_orb_spec.py pins it)
__constant__ int c_bound[30][2] = {
    {1042832, 109606}, {997255, 324028}, {908093, 524288}, {779244, 701634}, {616338, 848316}, {426494, 957922},
    {218011, 1025662}, {0, 1048576}, {-218011, 1025662}, {-426494, 957922}, {-616338, 848316}, {-779244, 701634},
    {-908093, 524288}, {-997255, 324028}, {-1042832, 109606}, {-1042832, -109606}, {-997255, -324028}, {-908093, -524288},
    {-779244, -701634}, {-616338, -848316}, {-426494, -957922}, {-218011, -1025662}, {0, -1048576}, {218011, -1025662},
    {426494, -957922}, {616338, -848316}, {779244, -701634}, {908093, -524288}, {997255, -324028}, {1042832, -109606}};

// S20 order as one 96-bit key, larger = earlier: (R + 2^54) in the high 64 bits (|R| < 2^56), ~(y << 16 | x) below.
struct Key { unsigned long long hi; unsigned lo; };
__device__ __forceinline__ Key cand_key(const OrbCand &c) {
    return Key{(unsigned long long)(c.R + (1LL << 54)), ~(((unsigned)c.y << 16) | (unsigned)c.x)};
}
__device__ __forceinline__ bool key_gt(Key a, Key b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
__device__ __forceinline__ bool key_ge(Key a, Key b) { return a.hi > b.hi || (a.hi == b.hi && a.lo >= b.lo); }
// 12-bit digit d (0 = most significant) of the 96-bit key, and the key's top 12 * d bits
__device__ __forceinline__ unsigned key_digit(Key k, int d) {
    const int lo_bit = 84 - 12 * d;   // digit covers bits [lo_bit, lo_bit + 12)
    if (lo_bit >= 32) return (unsigned)(k.hi >> (lo_bit - 32)) & 4095u;
    if (lo_bit + 12 <= 32) return (k.lo >> lo_bit) & 4095u;
    return ((unsigned)(k.hi << (32 - lo_bit)) | (k.lo >> lo_bit)) & 4095u;   // lo_bit = 24: 4 bits of hi, 8 of lo
}
__device__ __forceinline__ bool key_prefix_is(Key k, int digits, const unsigned *prefix) {
    for (int d = 0; d < digits; ++d)
        if (key_digit(k, d) != prefix[d]) return false;
    return true;
}

// S16 (oracle/cart_oracle.h) at destination pixel (x, y) of a 1-channel image: the arithmetic of resize_linear_kernel
// (post_kernels.hip) in the same order; fx / fy = (float)((double)sw / dw), (float)((double)sh / dh).  -ffp-contract=off.
__device__ __forceinline__ uint8_t s16_resize_px(const uint8_t *src, size_t sstep, int sw, int sh, int x, int y, float fx, float fy) {
    const float src_x = (float)x * fx, src_y = (float)y * fy;
    const int x1 = (int)floorf(src_x), y1 = (int)floorf(src_y), x2 = x1 + 1, y2 = y1 + 1;
    const int x2r = min(x2, sw - 1), y2r = min(y2, sh - 1);
    const float wx1 = (float)x2 - src_x, wx2 = src_x - (float)x1, wy1 = (float)y2 - src_y, wy2 = src_y - (float)y1;
    const uint8_t *r1 = src + (size_t)y1 * sstep, *r2 = src + (size_t)y2r * sstep;
    float out = 0.f;   // four multiplies and four adds in this order, like the oracle
    out = out + (float)r1[x1] * (wx1 * wy1);
    out = out + (float)r1[x2r] * (wx2 * wy1);
    out = out + (float)r2[x1] * (wx1 * wy2);
    out = out + (float)r2[x2r] * (wx2 * wy2);
    const float r = rintf(out);
    return (uint8_t)fminf(fmaxf(r, 0.f), 255.f);
}

__device__ __forceinline__ int level_of_tile(const OrbPlan &p, int t) {
    int l = 0;
    while (l + 1 < p.n_levels && t >= p.lev[l + 1].tile0) ++l;
    return l;
}

// FAST-9 score (S20) at LDS position (cx, cy); 0 = not a corner.  Any score >= 20 needs 9 differences of one sign
// beyond +-20, so pixels with fewer are rejected before the 32 arc minima.
__device__ __forceinline__ int fast_score(const uint8_t (*t)[kLdsW], int cx, int cy) {
    const int c = t[cy][cx];
    int d[16], nb = 0, nd = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        d[j] = (int)t[cy + c_circle[j][1]][cx + c_circle[j][0]] - c;
        nb += d[j] > kFastT;
        nd += d[j] < -kFastT;
    }
    if (nb < 9 && nd < 9) return 0;
    int best = INT_MIN;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        int mn = d[k], mx = d[k];
#pragma unroll
        for (int j = 1; j < 9; ++j) {
            mn = min(mn, d[(k + j) & 15]);
            mx = max(mx, d[(k + j) & 15]);
        }
        best = max(best, max(mn, -mx));
    }
    const int s = best - 1;
    return s >= kFastT ? s : 0;
}

// R = 25 (ab - c^2) - (a + b)^2 over the 7x7 window at LDS position (cx, cy) (OpenCV ORB's HarrisResponses sums)
__device__ __forceinline__ long long harris_r(const uint8_t (*t)[kLdsW], int cx, int cy) {
    int a = 0, b = 0, c = 0;
    for (int v = -3; v <= 3; ++v) {
        const uint8_t *rm = t[cy + v - 1], *r0 = t[cy + v], *rp = t[cy + v + 1];
#pragma unroll
        for (int u = -3; u <= 3; ++u) {
            const int x = cx + u;
            const int ix = 2 * ((int)r0[x + 1] - (int)r0[x - 1]) + ((int)rm[x + 1] - (int)rm[x - 1]) + ((int)rp[x + 1] - (int)rp[x - 1]);
            const int iy = 2 * ((int)rp[x] - (int)rm[x]) + ((int)rp[x - 1] - (int)rm[x - 1]) + ((int)rp[x + 1] - (int)rm[x + 1]);
            a += ix * ix;
            b += iy * iy;
            c += ix * iy;
        }
    }
    const long long A = a, B = b, Cc = c;
    return 25 * (A * B - Cc * Cc) - (A + B) * (A + B);
}
}  // namespace

// ------------------------------------------------------------------ pyramid
// Level 0 = the input (S1 gray for 3 channels); level l = S16 resize of level l-1.  grid.z = image.
__global__ __launch_bounds__(256) void orb_pyramid_kernel(OrbPlan p, int level, OrbOut o, uint8_t *pyr) {
    const OrbLevel &L = p.lev[level];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, img = blockIdx.z;
    if (x >= L.w || y >= L.h) return;
    uint8_t *base = pyr + (size_t)img * p.pyr_stride;
    uint8_t v;
    if (level == 0) {
        const uint8_t *s = o.src[img] + (size_t)y * o.src_step[img];
        if (o.channels == 3) {
            const int b = s[3 * x], g = s[3 * x + 1], r = s[3 * x + 2];
            v = (uint8_t)((1868 * b + 9617 * g + 4899 * r + 8192) >> 14);
        } else {
            v = s[x];
        }
    } else {
        const OrbLevel &U = p.lev[level - 1];
        v = s16_resize_px(base + U.pyr_off, (size_t)U.w, U.w, U.h, x, y, L.fx, L.fy);
    }
    base[L.pyr_off + (size_t)y * L.w + x] = v;
}

// ------------------------------------------------------------------ detect
// One block per (tile, image): a 64 x 16 tile of the level's candidate region with a 4-pixel halo in LDS, FAST scores on
// the tile plus a 1-pixel ring, strict 3x3 NMS, Harris for the survivors, wave-aggregated append to the level's list.
__global__ __launch_bounds__(256) void orb_detect_kernel(OrbPlan p, const uint8_t *pyr, OrbCand *cand, int32_t *cand_cnt) {
    __shared__ uint8_t tile[kLdsH][kLdsW];
    __shared__ int score[kOrbTileH + 2][kOrbTileW + 2];
    const int img = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int l = level_of_tile(p, t);
    const OrbLevel &L = p.lev[l];
    const int tt = t - L.tile0, x0 = kOrbEdge + (tt % L.tiles_x) * kOrbTileW, y0 = kOrbEdge + (tt / L.tiles_x) * kOrbTileH;
    const uint8_t *I = pyr + (size_t)img * p.pyr_stride + L.pyr_off;
    for (int i = tid; i < kLdsH * kLdsW; i += 256) {   // x0 - 4, y0 - 4 >= 27: only the far side can leave the image
        const int ly = i / kLdsW, lx = i % kLdsW;
        const int gy = min(y0 - kHalo + ly, L.h - 1), gx = min(x0 - kHalo + lx, L.w - 1);
        tile[ly][lx] = I[(size_t)gy * L.w + gx];
    }
    __syncthreads();
    const int xe = L.w - kOrbEdge, ye = L.h - kOrbEdge;   // candidates: [31, xe) x [31, ye)
    for (int i = tid; i < (kOrbTileH + 2) * (kOrbTileW + 2); i += 256) {
        const int sy = i / (kOrbTileW + 2), sx = i % (kOrbTileW + 2);
        const int gx = x0 - 1 + sx, gy = y0 - 1 + sy;
        const bool cand_px = gx >= kOrbEdge && gx < xe && gy >= kOrbEdge && gy < ye;
        score[sy][sx] = cand_px ? fast_score(tile, sx - 1 + kHalo, sy - 1 + kHalo) : 0;
    }
    __syncthreads();
    OrbCand *list = cand + (size_t)img * p.cand_stride + L.cand_off;
    int32_t *counter = cand_cnt + img * kOrbLevels + l;
    const int lane = tid & 63;
    for (int i = tid; i < kOrbTileH * kOrbTileW; i += 256) {
        const int sy = i / kOrbTileW, sx = i % kOrbTileW;
        const int s = score[sy + 1][sx + 1];
        bool keep = s > 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
                if (dy != 1 || dx != 1) keep = keep && s > score[sy + dy][sx + dx];
        long long R = 0;
        if (keep) R = harris_r(tile, sx + kHalo, sy + kHalo);
        const unsigned long long mask = __ballot(keep);
        if (!mask) continue;
        const int leader = __ffsll((long long)mask) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(counter, __popcll(mask));
        base = __shfl(base, leader);
        if (keep) {
            const int idx = base + __popcll(mask & ((1ull << lane) - 1));
            if (idx < L.cap) list[idx] = OrbCand{R, y0 + sy, x0 + sx};
        }
    }
}

// ------------------------------------------------------------------ select
// One block per (level, image).  The threshold key T (the quota-th largest) comes from a radix select over 12-bit digits
// of the 96-bit key, finished in LDS once at most kSelFinish keys share the prefix; keys are unique, so exactly
// min(count, quota) records have key >= T.  They are gathered into `sel` and each is placed by its rank among them.
__global__ __launch_bounds__(kSelThreads) void orb_select_kernel(OrbPlan p, const OrbCand *cand, const int32_t *cand_cnt, OrbCand *sel, int4 *kpi,
                                                                 int32_t *counts) {
    __shared__ unsigned hist[4096];
    __shared__ unsigned part[kSelThreads];
    __shared__ unsigned long long khi[kSelChunk];
    __shared__ unsigned klo[kSelChunk];
    __shared__ unsigned prefix[8];
    __shared__ int s_need, s_matched, s_bin, s_n;
    __shared__ Key s_T;
    const int l = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const OrbLevel &L = p.lev[l];
    const int32_t *cnt = cand_cnt + img * kOrbLevels;
    int offset = 0, total = 0;
    for (int j = 0; j < p.n_levels; ++j) {
        const int k = min(min(cnt[j], p.lev[j].cap), p.lev[j].quota);
        offset += j < l ? k : 0;
        total += k;
    }
    if (l == 0 && tid == 0) counts[img] = total;
    const int c = min(cnt[l], L.cap), keep = min(c, L.quota);
    if (keep == 0) return;
    const OrbCand *list = cand + (size_t)img * p.cand_stride + L.cand_off;
    if (tid == 0) { s_need = keep; s_matched = c; s_T = Key{0ull, 0u}; }
    __syncthreads();
    int digits = 0;
    if (keep < c) {
        // radix passes: the prefix narrows to the digits of T while more than kSelFinish keys match it
        while (digits < 8 && s_matched > kSelFinish) {
            for (int i = tid; i < 4096; i += kSelThreads) hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < c; i += kSelThreads) {
                const Key k = cand_key(list[i]);
                if (key_prefix_is(k, digits, prefix)) atomicAdd(&hist[key_digit(k, digits)], 1u);
            }
            __syncthreads();
            unsigned mine = hist[4 * tid] + hist[4 * tid + 1] + hist[4 * tid + 2] + hist[4 * tid + 3];
            part[tid] = mine;
            __syncthreads();
            for (int o = 1; o < kSelThreads; o <<= 1) {   // inclusive suffix sums over the threads' 4-bin groups
                const unsigned v = tid + o < kSelThreads ? part[tid + o] : 0u;
                __syncthreads();
                part[tid] += v;
                __syncthreads();
            }
            unsigned above = part[tid] - mine;   // keys in bins above this thread's group
            const unsigned need = (unsigned)s_need;
            for (int b = 4 * tid + 3; b >= 4 * tid; --b) {
                if (above < need && need <= above + hist[b]) {
                    s_bin = b;
                    s_n = (int)above;
                }
                above += hist[b];
            }
            __syncthreads();
            if (tid == 0) {
                prefix[digits] = (unsigned)s_bin;
                s_need -= s_n;
                s_matched = (int)hist[s_bin];
            }
            __syncthreads();
            ++digits;
        }
        // finish: the keys with the prefix go to LDS; T is the one with exactly need - 1 larger keys among them
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (int i = tid; i < c; i += kSelThreads) {
            const Key k = cand_key(list[i]);
            if (key_prefix_is(k, digits, prefix)) {
                const int j = atomicAdd(&s_n, 1);
                if (j < kSelChunk) { khi[j] = k.hi; klo[j] = k.lo; }
            }
        }
        __syncthreads();
        const int m = min(s_n, kSelChunk);
        for (int i = tid; i < m; i += kSelThreads) {
            const Key k{khi[i], klo[i]};
            int r = 0;
            for (int j = 0; j < m; ++j) r += key_gt(Key{khi[j], klo[j]}, k);
            if (r == s_need - 1) s_T = k;
        }
        __syncthreads();
    }
    // gather the kept records, then place each by its rank (keys are unique)
    const Key T = s_T;
    OrbCand *kept = sel + (size_t)img * p.nfeatures + offset;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i = tid; i < c; i += kSelThreads) {
        const OrbCand r = list[i];
        if (key_ge(cand_key(r), T)) {
            const int j = atomicAdd(&s_n, 1);
            if (j < keep) kept[j] = r;
        }
    }
    __threadfence_block();
    __syncthreads();
    constexpr int kPer = 16;   // kept records per thread (keep <= 16384 > any level quota of N <= 65536)
    const int nq = (keep + kSelThreads - 1) / kSelThreads;
    Key mine[kPer];
    int rank[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int i = tid + q * kSelThreads;
        mine[q] = i < keep ? cand_key(kept[i]) : Key{0ull, 0u};
        rank[q] = 0;
    }
    for (int c0 = 0; c0 < keep; c0 += kSelChunk) {
        const int n = min(kSelChunk, keep - c0);
        __syncthreads();
        for (int j = tid; j < n; j += kSelThreads) {
            const Key k = cand_key(kept[c0 + j]);
            khi[j] = k.hi;
            klo[j] = k.lo;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const Key k{khi[j], klo[j]};
#pragma unroll
            for (int q = 0; q < kPer; ++q)
                if (q < nq) rank[q] += key_gt(k, mine[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int i = tid + q * kSelThreads;
        if (i < keep) {
            const OrbCand r = kept[i];
            const float resp = (float)((double)r.R / 64972990404000000.0);   // 25 * 7140^4, OpenCV's Harris scale
            kpi[(size_t)img * p.nfeatures + offset + rank[q]] = make_int4(r.x, r.y, l, __float_as_int(resp));
        }
    }
}

// ------------------------------------------------------------------ describe
// One wave per keypoint: intensity-centroid moments over the 749-pixel patch, the 12-degree bin by integer cross products,
// 4 ballots of 64 steered comparisons = the 256-bit descriptor.
__global__ __launch_bounds__(256) void orb_describe_kernel(OrbPlan p, const uint8_t *pyr, const int4 *kpi, const char4 *pattern, OrbOut o) {
    const int img = blockIdx.y, lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= o.counts[img]) return;
    const int4 k = kpi[(size_t)img * p.nfeatures + idx];
    const int x = k.x, y = k.y, l = k.z;
    const OrbLevel &L = p.lev[l];
    const uint8_t *I = pyr + (size_t)img * p.pyr_stride + L.pyr_off;
    const size_t w = (size_t)L.w;
    int m10 = 0, m01 = 0;
    for (int i = lane; i < 31 * 31; i += 64) {
        const int v = i / 31 - 15, u = i % 31 - 15;
        const int um = c_umax[v < 0 ? -v : v];
        if (u >= -um && u <= um) {
            const int val = I[(size_t)(y + v) * w + (x + u)];
            m10 += u * val;
            m01 += v * val;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m10 += __shfl_xor(m10, off);
        m01 += __shfl_xor(m01, off);
    }
    bool hit = false;
    if (lane < 30) {
        const int pj = lane == 0 ? 29 : lane - 1;
        const long long c0 = (long long)c_bound[pj][0] * m01 - (long long)c_bound[pj][1] * m10;
        const long long c1 = (long long)c_bound[lane][0] * m01 - (long long)c_bound[lane][1] * m10;
        hit = c0 >= 0 && c1 < 0;
    }
    const unsigned long long hits = __ballot(hit);
    const int bin = hits ? __ffsll((long long)hits) - 1 : 0;   // m = 0 crosses nothing: bin 0
    const char4 *pat = pattern + bin * 256;
    unsigned long long bits[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const char4 q = pat[c * 64 + lane];
        const int a = I[(size_t)(y + q.y) * w + (x + q.x)], b = I[(size_t)(y + q.w) * w + (x + q.z)];
        bits[c] = __ballot(a < b);
    }
    if (lane < 32) {
        const unsigned long long word = lane < 8 ? bits[0] : lane < 16 ? bits[1] : lane < 24 ? bits[2] : bits[3];
        o.desc[img][(size_t)idx * o.desc_step[img] + lane] = (uint8_t)(word >> (8 * (lane & 7)));
    }
    if (lane == 0) {
        cart_keypoint r;
        r.x = (float)x * L.scale;
        r.y = (float)y * L.scale;
        r.size = 31.0f * L.scale;
        r.angle = 12.0f * (float)bin;
        r.response = __int_as_float(k.w);
        r.octave = l;
        r.class_id = -1;
        o.kp[img][idx] = r;
    }
}

void launch_orb_pyramid_level(const OrbPlan &p, int level, const OrbOut &o, uint8_t *pyr, hipStream_t s) {
    const OrbLevel &L = p.lev[level];
    hipLaunchKernelGGL(orb_pyramid_kernel, dim3((L.w + 63) / 64, (L.h + 3) / 4, p.n_images), dim3(64, 4), 0, s, p, level, o, pyr);
}
void launch_orb_detect(const OrbPlan &p, const uint8_t *pyr, OrbCand *cand, int32_t *cand_cnt, hipStream_t s) {
    hipLaunchKernelGGL(orb_detect_kernel, dim3(p.total_tiles, p.n_images), dim3(256), 0, s, p, pyr, cand, cand_cnt);
}
void launch_orb_select(const OrbPlan &p, const OrbCand *cand, const int32_t *cand_cnt, OrbCand *sel, int4 *kpi, int32_t *counts, hipStream_t s) {
    hipLaunchKernelGGL(orb_select_kernel, dim3(p.n_levels, p.n_images), dim3(kSelThreads), 0, s, p, cand, cand_cnt, sel, kpi, counts);
}
void launch_orb_describe(const OrbPlan &p, const uint8_t *pyr, const int4 *kpi, const char4 *pattern, const OrbOut &o, hipStream_t s) {
    hipLaunchKernelGGL(orb_describe_kernel, dim3((p.nfeatures + 3) / 4, p.n_images), dim3(256), 0, s, p, pyr, kpi, pattern, o);
}

}  // namespace cart_amd

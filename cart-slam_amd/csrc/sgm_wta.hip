// sgm_wta.hip -- winner takes all of the SGM core: two-kernel, banded and fused with the "up" direction (stage overview: sgm_census.hip).
#include <cstdlib>
#include <type_traits>

#include "sgm_device.h"

namespace cart_amd {

// ------------------------------------------------------------------ winner takes all
// Block = 64 pixels of one row; a pixel is owned by LPP = D/16 lanes, 16 disparities per lane as 8
// packed u16 pairs.  Per path one 16-byte non-temporal load per lane, the
// bytes are widened by v_perm_b32 and summed with v_pk_add_u16 (1 VALU op per cell and path).
//   * the slab bytes of a lane's 16 disparities arrive in the aggregation kernel's split-halves order, whose even /
//     odd bytes are natural adjacent disparity pairs: one v_and or v_perm plus a plain add per two cells;
//   * argmin (ties -> lowest d, oracle S5): packed keys S*16 + local index, packed min tree, then one
//     32-bit key (S<<16 | d) per lane reduced over the pixel's lanes by DPP;
//   * uniqueness: (float)S*u >= (float)best is monotone in S, so it equals S >= T for the integer
//     threshold T = min{s : (float)s*u >= (float)best}; the pixel is unique iff every S[d] < T lies within
//     |d - best| <= 1, i.e. iff sum_d max(T-S[d],0) equals the same sum over the three neighbours;
//   * the summed costs of the tile live in LDS as u16 [64][D]: sub-pixel neighbours and the right-view
//     diagonal minima S(p+d, d) (oracle S6) come from there; per-tile right minima are merged across tiles
//     with one packed atomicMin per right pixel and tile.
// The fused sweep's right-view rows (one u32 key per right pixel of a block row) can be indexed through rv_slot: one pad per
// 16 entries.  The lanes that own one pixel hold disparity chunks 16 apart, so their candidates for one `da` land 16 entries
// apart -- on TWO of the 32 LDS banks without the pad (8-way conflicts on every ds_min_u32 at D = 256), on 16 different
// banks with it.  Used where it measured faster: D = 256 / 4 paths (sweep 1.58 -> 1.43 ms per 16 pairs).  The 8-path sweeps
// sit at the 168-VGPR limit of three waves per SIMD and the 16 slot addresses spill (D = 256 / 8 paths: 2.5 -> 4.0 ms), and
// the two-kernel WTA did not move (2.03 ms at D = 256 with or without).
__host__ __device__ constexpr int rv_slot(int i) { return i + (i >> 4); }
__host__ __device__ constexpr int rv_size(int n) { return ((n + (n >> 4) + 1) + 3) & ~3; }   // slots for n entries (+ a spare), multiple of 4
// Slots of one right-view row of a fused-sweep block (cols + D - 1 entries + a spare, padded or not), a multiple of 8: in
// the partial buffer a slot is ONE u16 -- (S << log2(cols)) | (d mod cols), 0xffff = empty -- and a burst packs 8 of them
// per lane.  For entry e of a block the candidates are the block's columns xl = 0..cols-1 with d = D-1-e + xl, so d mod cols
// identifies the column and rv_key32 gives the (S << 16 | d) key back; S <= 8 * 255 leaves 5 bits for cols = 32.
__host__ __device__ constexpr int rv_row_slots(int cols, int D, bool padded) { return ((padded ? rv_size(cols + D - 1) : cols + D) + 7) & ~7; }
__host__ __device__ constexpr uint32_t rv_key16(uint32_t key32, int cols) {   // cols = 16 or 32; 0xffffffff -> 0xffff
    return ((((key32 >> 16) << (cols == 32 ? 5 : 4)) | (key32 & (uint32_t)(cols - 1))) & 0xffffu);
}
__host__ __device__ constexpr uint32_t rv_key32(uint32_t key16, int e, int cols, int D) {   // key16 != 0xffff
    const int sh = cols == 32 ? 5 : 4, base = D - 1 - e;
    return ((key16 >> sh) << 16) | (uint32_t)(base + (((int)(key16 & (uint32_t)(cols - 1)) - base) & (cols - 1)));
}

__device__ __forceinline__ uint32_t pk_sub_sat(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// smallest s with (float)s*u >= (float)bc, clamped to 4095 (> any reachable cost sum, <= 8*255)
__host__ __device__ __forceinline__ uint32_t uniq_threshold(uint32_t bc, float u) {
    if (bc == 0) return 0;
    if (!(u > 0.f)) return 4095u;
    const float bcf = (float)bc;
    const float q = bcf / u;
    if (q > 4000.f) return 4095u;
    const int g = (int)q;
    int T = g + 3;
#pragma unroll
    for (int c = 2; c >= -2; --c) {
        const int v = g + c;
        if (v >= 0 && (float)v * u >= bcf) T = v;
    }
    return (uint32_t)(T < 4095 ? T : 4095);
}

// test access (cart_debug_uniq_table): the threshold of every best cost 0..2047 for one uniqueness ratio, computed by
// the device code the WTA kernels use, or by the same function compiled for the host
__global__ void uniq_table_kernel(float u, uint16_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2048) out[i] = (uint16_t)uniq_threshold((uint32_t)i, u);
}
void launch_uniq_table(float u, uint16_t *out_dev, hipStream_t s) { hipLaunchKernelGGL(uniq_table_kernel, dim3(8), dim3(256), 0, s, u, out_dev); }
void uniq_table_host(float u, uint16_t *out) {
    for (int i = 0; i < 2048; ++i) out[i] = (uint16_t)uniq_threshold((uint32_t)i, u);
}

struct WtaArgs {
    SlabTable slabs;
    uint16_t *wta_l;
    uint32_t *right_pk;
    Geometry g;
    const uint16_t *thr;             // integer uniqueness threshold by best cost, 2048 entries (uniq_threshold of every cost, built at engine create)
    int nslabs;
    int slab_idx[kMaxPaths];
};

__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}


// ---- one row of the WTA: the pieces wta_kernel, wta_band_kernel and wta_fused_kernel share.  Bit-exactness against the oracle lives here (ties go to
// the lowest d, the integer uniqueness threshold, the sub-pixel rounding): each piece exists once.
// A lane holds the cost sums S of its 16 disparities as natural adjacent pairs: sm[q] = (S[d0+2q], S[d0+2q+1]), sm[4+q] = (S[d0+8+2q], S[d0+9+2q]).

// + one path's 16 slab bytes v[0..3].  Slab chunk order {0,8,1,9,...}: the even bytes of dword q are disparities (2q, 2q+1), the odd bytes (2q+8, 2q+9).
// Even bytes need one v_and, odd bytes one v_perm; the accumulation is a plain 32-bit add (sums stay < 2^16 per half).
template <typename V>
__device__ __forceinline__ void sum_add_slab(uint32_t (&sm)[8], const V &v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sm[q] += v[q] & 0x00ff00ffu;
        sm[4 + q] += perm(0u, v[q], 0x0c030c01u);
    }
}
// path costs in agg_step's split-halves registers, st[i] = (L[d0+i], L[d0+i+8]), as the same pairs
__device__ __forceinline__ void sum_from_state(uint32_t (&sm)[8], const uint32_t (&st)[8]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sm[q] = perm(st[2 * q + 1], st[2 * q], 0x05040100u);
        sm[4 + q] = perm(st[2 * q + 1], st[2 * q], 0x07060302u);
    }
}

// right view (oracle S6): the lane min-reduces its 16 keys (S << 16 | d) into the row's array indexed by p = x - d (ds_min_u32); rm = the slot of d = d0
__device__ __forceinline__ void rv_scatter(uint32_t *rm, const uint32_t (&sm)[8], int d0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int da = q < 4 ? 2 * q : 8 + 2 * (q - 4);   // local disparity of the low half of sm[q]
        atomicMin(rm - da, (sm[q] << 16) | (uint32_t)(d0 + da));
        atomicMin(rm - da - 1, (sm[q] & 0xffff0000u) | (uint32_t)(d0 + da + 1));
    }
}

// left view, argmin (ties -> lowest d): packed keys S*16 + local disparity index ...
__device__ __forceinline__ void wta_keys(const uint32_t (&sm)[8], uint32_t (&key)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // (a shift and an or per register; one v_pk_mad_u16 with the index pair in an SGPR measured level to slower, profiles/r04_fused.txt)
        const u16x2 kk = __builtin_bit_cast(u16x2, sm[k]) * (u16x2){16, 16} + (u16x2){(uint16_t)(2 * k), (uint16_t)(2 * k + 1)};
        key[k] = __builtin_bit_cast(uint32_t, kk);
    }
}
// ... the lane's best as (S << 16 | d); group_allmin over the pixel's lanes gives the pixel's
__device__ __forceinline__ uint32_t wta_lane_best(const uint32_t (&key)[8], int d0) {
    uint32_t m = pk_min(pk_min(pk_min(key[0], key[1]), pk_min(key[2], key[3])), pk_min(pk_min(key[4], key[5]), pk_min(key[6], key[7])));
    m = pk_min(m, __builtin_amdgcn_alignbit(m, m, 16)) & 0xffffu;
    return ((m >> 4) << 16) | (uint32_t)(d0 + (int)(m & 15u));
}
// uniqueness: sum over the pixel's D disparities of max(T - S[d], 0), T = the integer threshold of the pixel's best cost
template <int LPP>
__device__ __forceinline__ uint32_t wta_uniq_sum(const uint32_t (&sm)[8], uint32_t T) {
    const uint32_t tt = T * 0x10001u;
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = pk_add(acc, pk_sub_sat(tt, sm[k]));
    return group_allsum<LPP>((acc & 0xffffu) + (acc >> 16));
}
// the plain sequence: pk = the pixel's best (S << 16 | d), T = thr[best cost] (= uniq_threshold: one load from the engine's 4 KB table or its LDS copy
// instead of the float search -- a division and five multiply-compares, ~45 VALU instructions per lane and row), tot = its uniqueness sum
template <int LPP>
__device__ __forceinline__ void wta_best_and_sum(const uint32_t (&sm)[8], int d0, const uint16_t *thr, uint32_t &pk, uint32_t &T, uint32_t &tot) {
    uint32_t key[8];
    wta_keys(sm, key);
    pk = group_allmin<LPP>(wta_lane_best(key, d0));
    T = thr[pk >> 16];
    tot = wta_uniq_sum<LPP>(sm, T);
}

struct WtaPick { int bd, bc, l, r; bool unique; };   // best disparity, its cost sum, the sums at d-1 / d+1 (0x7fff outside [0, D)), unique?
// The pixel's first lane decides.  srow = the pixel's D sums in LDS; tot = its uniqueness sum: every S[d] < T lies within |d - best| <= 1 iff the sum
// equals the same sum over the three neighbours.  TOP2: tot is the pixel's second-smallest (S << 16 | d) key instead.
template <int D, bool TOP2 = false>
__device__ __forceinline__ WtaPick wta_decide(uint32_t pk, uint32_t thr, uint32_t tot, const uint16_t *srow) {
    const int bd = (int)(pk & 0xffffu), bc = (int)(pk >> 16), T = (int)thr;
    const int l = bd > 0 ? srow[bd - 1] : 0x7fff, r = bd < D - 1 ? srow[bd + 1] : 0x7fff;
    const int tot_nbr = max(T - bc, 0) + max(T - l, 0) + max(T - r, 0);
    // TOP2: unique iff the runner-up's cost reaches the threshold or it sits next to the winner
    const bool unique = TOP2 ? ((int)(tot >> 16) >= T || abs((int)(tot & 0xffffu) - bd) <= 1) : (int)tot == tot_nbr;
    return WtaPick{bd, bc, l, r, unique};
}
// oracle S5 sub-pixel: the pixel's u16 in the left WTA map
template <int D>
__device__ __forceinline__ uint32_t wta_subpixel(const WtaPick &w) {
    uint32_t out = kWtaInvalid;
    if (w.unique) {
        int subp = w.bd * 16;
        if (w.bd > 0 && w.bd < D - 1) {
            const int num = w.l - w.r, den = w.l - 2 * w.bc + w.r;
            if (den != 0) subp += (num * 16 + den) / (2 * den);
        }
        out = (uint32_t)subp & 0xffffu;
    }
    return out;
}

// ---- set-up of the kernels that recompute the "up" path while they walk a block of columns bottom-up (wta_band_kernel, wta_fused_kernel) ----
// Block = waves of P = 64/LPP adjacent columns from x0 on, one pixel per lane group like a wave of aggregate_kernel, so the right-census window goes
// through the same wave-private LDS staging (Win / WinLane) and the step is the same agg_step.  Every load is "row-0 base (wave-uniform, SGPRs) + row
// offset + constant per-lane byte offset".  Columns past the image compute on census padding and the clamped last slab column and never write.
template <int LPP>
struct UpSweep {
    using WN = Win<LPP>;
    int lane, wid, gl, pg, d0;             // lane, wave (uniform), lane inside the pixel's lane group, pixel inside the wave, the lane's first disparity
    int xl, x, xw0;                        // column inside the block / the image; the wave's first column (uniform)
    bool valid;                            // x < w
    uint32_t sel_lo, sel_hi, p1p1, p2p2;   // agg_step's stitching selectors (see aggregate_kernel) and packed penalties
    WinLane<LPP> wl;
    const uint32_t *pw0, *pl0;             // row 0: the wave's right-census window, its first left feature
    const uint8_t *ps0;                    // row 0 of slab 0 at the wave's first (clamped) column
    unsigned lo_l, lo_s;
    int cpitch;
    ptrdiff_t row_bytes, slab_bytes;

    __device__ __forceinline__ void init(const Geometry &g, const uint32_t *cen_l, const uint32_t *cen_r, const uint8_t *slabs, int frame, int x0) {
        constexpr int D = WN::D, P = WN::P;
        lane = threadIdx.x & 63; wid = uniform((int)(threadIdx.x >> 6));
        gl = lane % LPP; pg = lane / LPP; d0 = gl * 16;
        xl = wid * P + pg; x = x0 + xl;
        xw0 = x0 + wid * P;
        valid = x < g.w;
        p1p1 = (uint32_t)g.p1 * 0x10001u; p2p2 = (uint32_t)g.p2 * 0x10001u;
        sel_lo = gl == 0 ? 0x05040d0du : 0x05040302u;
        sel_hi = gl == LPP - 1 ? 0x0d0d0302u : 0x05040302u;
        wl.init(lane);
        const ptrdiff_t cen0 = (ptrdiff_t)frame * (ptrdiff_t)g.census_elems + g.cpadl + xw0;
        pw0 = cen_r + uniform(cen0 - g.min_disp - (D - 1));
        pl0 = cen_l + uniform(cen0);
        lo_l = (unsigned)pg * 4u;
        const int xbase = min(xw0, g.w - 1), xc = min(x, g.w - 1);   // xbase <= xc
        ps0 = slabs + uniform((ptrdiff_t)xbase * D);
        lo_s = (unsigned)((xc - xbase) * D + d0);
        cpitch = g.cpitch; row_bytes = (ptrdiff_t)g.w * D; slab_bytes = (ptrdiff_t)g.slab_bytes;
    }
    // the wave's cooperative window loads and the lane's left feature of row y
    __device__ __forceinline__ void load_census_row(int y, uint32_t (&win)[WN::NLD], uint32_t &fl) {
        const uint32_t *pw = pw0 + (ptrdiff_t)y * cpitch;
#pragma unroll
        for (int i = 0; i < WN::NLD; ++i) win[i] = ld_u32(pw, wl.goff[i]);
        fl = ld_u32(pl0 + (ptrdiff_t)y * cpitch, lo_l);
    }
    __device__ __forceinline__ v4u load_slab(int y, int path) {
        const uint8_t *ps = ps0 + (ptrdiff_t)y * row_bytes + (ptrdiff_t)path * slab_bytes;
        return __builtin_nontemporal_load((const CART_GLOBAL v4u *)((const CART_GLOBAL char *)sgpr(ps) + pin_v(lo_s)));
    }
    // row y of the stored slabs into sv[k]: every path, or the paths other than kUpPath (SKIP_UP) and kUpRightPath (SKIP_UR)
    template <bool SKIP_UP, bool SKIP_UR = false, int NS>
    __device__ __forceinline__ void load_slab_row(int y, uint32_t (&sv)[NS][4]) {
#pragma unroll
        for (int p = 0; p < NS + (SKIP_UP ? 1 : 0) + (SKIP_UR ? 1 : 0); ++p) {
            if (SKIP_UP && p == kUpPath) continue;
            if (SKIP_UR && p == kUpRightPath) continue;
            const int k = p - (SKIP_UP && p > kUpPath ? 1 : 0) - (SKIP_UR && p > kUpRightPath ? 1 : 0);   // compile-time after unrolling
            const v4u v = load_slab(y, p);
            sv[k][0] = v.x; sv[k][1] = v.y; sv[k][2] = v.z; sv[k][3] = v.w;
        }
    }
};

// TOP2 = the S5 variant (CART_OPT_SPEC_S5_TOP2): uniqueness looks at the SECOND-best (cost, d) only -- the second-smallest
// (cost << 16 | d) key of the pixel -- instead of at every disparity.
template <int LPP, bool TOP2 = false>
__global__ __launch_bounds__(256) void wta_kernel(WtaArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t s_lds[];  // [kWtaTileX][DP]
    constexpr int D = LPP * 16;
    constexpr int DP = D + 8;                 // LDS row pitch in u16: 16 B of padding spread the pixels' rows over the banks
    constexpr int PPP = 256 / LPP;            // pixels per pass
    constexpr int NPASS = kWtaTileX / PPP;    // 1 (D=64), 2 (D=128), 4 (D=256)
    uint16_t *wta_l = a.wta_l;
    uint32_t *right_pk = a.right_pk;
    const Geometry &g = a.g;
    const int x0 = blockIdx.x * kWtaTileX, y = blockIdx.y, frame = blockIdx.z;
    const uint8_t *slabs = a.slabs.frame[frame];   // this frame's path slabs
    const int grp = threadIdx.x / LPP, gl = threadIdx.x % LPP, d0 = gl * 16;
    // Right view: every lane min-reduces its 16 (S << 16 | d) keys into the tile's array indexed by p = x - d (ds_min_u32),
    // slot p - (x0 - (D-1)).  (Walking the tile's diagonals per right pixel instead -- 64 dependent LDS reads on 127 of
    // the 256 threads at D = 64 -- was over half of this kernel's VALU instructions and made the D = 64 variant VALU-bound.)
    __shared__ uint32_t s_rv[kWtaTileX + D];
    for (int i = threadIdx.x; i < kWtaTileX + D; i += 256) s_rv[i] = 0xffffffffu;
    __syncthreads();

    uint32_t pk_res[NPASS], tot_res[NPASS], thr_res[NPASS];   // TOP2: tot_res holds the pixel's second-smallest key
    constexpr bool PREFETCH = NPASS >= 4;
    v4u pf[PREFETCH ? 2 : 1][PREFETCH ? kMaxPaths : 1];
    auto issue_pass = [&](int pass, v4u (&dst)[PREFETCH ? kMaxPaths : 1]) {
        if constexpr (PREFETCH) {
            const int xcp = min(x0 + pass * PPP + grp, g.w - 1);
            const uint8_t *p = slabs + ((size_t)y * g.w + xcp) * D + d0;
#pragma unroll
            for (int r = 0; r < kMaxPaths; ++r)
                if (r < a.nslabs) dst[r] = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(p + (size_t)a.slab_idx[r] * g.slab_bytes));
        }
    };
    if constexpr (PREFETCH) issue_pass(0, pf[0]);
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        const int xl = pass * PPP + grp;
        const int xc = min(x0 + xl, g.w - 1);
        uint32_t sm[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) sm[k] = 0;
        if constexpr (PREFETCH) {
            // D = 256: four passes per block and four blocks per CU (LDS) -- with every pass waiting for its own loads the
            // launch ran at memory latency (7.6 GB in 2.0 ms); the next pass's slab bytes are requested before this pass computes
            if (pass + 1 < NPASS) issue_pass(pass + 1, pf[(pass + 1) & 1]);
#pragma unroll
            for (int r = 0; r < kMaxPaths; ++r)
                if (r < a.nslabs) sum_add_slab(sm, pf[pass & 1][r]);
        } else {
            const uint8_t *p = slabs + ((size_t)y * g.w + xc) * D + d0;
            for (int r = 0; r < a.nslabs; ++r)
                sum_add_slab(sm, __builtin_nontemporal_load(reinterpret_cast<const v4u *>(p + (size_t)a.slab_idx[r] * g.slab_bytes)));
        }
        v4u *dst = reinterpret_cast<v4u *>(s_lds + xl * DP + d0);  // LDS tile in natural disparity order
        dst[0] = v4u{sm[0], sm[1], sm[2], sm[3]};
        dst[1] = v4u{sm[4], sm[5], sm[6], sm[7]};
        if (x0 + xl < g.w) {   // columns past the image (clamped duplicates of the last one) have no right view
            // rv_scatter's text, kept here: through the shared function wta_kernel<8> takes 38 instead of 31 VGPRs (profiles/wta_refactor.txt).  The
            // choice is made per kernel template, not per instantiation: the D = 64 and D = 256 variants would not have lost registers.
            uint32_t *rm = &s_rv[xl + D - 1 - d0];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int da = q < 4 ? 2 * q : 8 + 2 * (q - 4);   // local disparity of the low half of sm[q]
                atomicMin(rm - da, (sm[q] << 16) | (uint32_t)(d0 + da));
                atomicMin(rm - da - 1, (sm[q] & 0xffff0000u) | (uint32_t)(d0 + da + 1));
            }
        }
        uint32_t key[8];
        wta_keys(sm, key);
        uint32_t pk = wta_lane_best(key, d0);
        uint32_t cand = 0;
        if constexpr (TOP2) {
            // the lane's two smallest 16-bit keys: a tournament on (min, second) pairs, both halves of the packed registers at once
            uint32_t lo[4], hi[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { lo[k] = pk_min(key[2 * k], key[2 * k + 1]); hi[k] = pk_max(key[2 * k], key[2 * k + 1]); }
            const uint32_t m01 = pk_min(lo[0], lo[1]), s01 = pk_min(pk_max(lo[0], lo[1]), pk_min(hi[0], hi[1]));
            const uint32_t m23 = pk_min(lo[2], lo[3]), s23 = pk_min(pk_max(lo[2], lo[3]), pk_min(hi[2], hi[3]));
            const uint32_t mm4 = pk_min(m01, m23), ss4 = pk_min(pk_max(m01, m23), pk_min(s01, s23));
            const uint32_t mL = mm4 & 0xffffu, mH = mm4 >> 16, sL = ss4 & 0xffffu, sH = ss4 >> 16;
            const uint32_t second = min(max(mL, mH), min(sL, sH));   // (the smaller of mL, mH is the lane's best key)
            const uint32_t second_full = ((second >> 4) << 16) | (uint32_t)(d0 + (int)(second & 15u));
            const uint32_t best_all = group_allmin<LPP>(pk);
            cand = pk == best_all ? second_full : pk;   // the lane that holds the pixel's best key offers its runner-up
            pk = best_all;
            cand = group_allmin<LPP>(cand);
        } else {
            pk = group_allmin<LPP>(pk);
        }
        const uint32_t T = a.thr[pk >> 16];
        tot_res[pass] = TOP2 ? cand : wta_uniq_sum<LPP>(sm, T);
        pk_res[pass] = pk;
        thr_res[pass] = T;
    }
    __syncthreads();

    if (gl == 0) {
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            const int xl = pass * PPP + grp, x = x0 + xl;
            if (x >= g.w) continue;
            const WtaPick w = wta_decide<D, TOP2>(pk_res[pass], thr_res[pass], tot_res[pass], s_lds + xl * DP);
            wta_l[(size_t)frame * g.npx + (size_t)y * g.w + x] = (uint16_t)wta_subpixel<D>(w);
        }
    }

    // right view (oracle S6): the tile's minima per right pixel are complete in s_rv, merged across tiles by atomicMin
    for (int pi = threadIdx.x; pi < kWtaTileX + D - 1; pi += 256) {
        const int p = x0 - (D - 1) + pi;
        const uint32_t best = s_rv[pi];
        if (p >= 0 && p < g.w && best != 0xffffffffu) atomicMin(&right_pk[(size_t)frame * g.npx + (size_t)y * g.w + p], best);
    }
}

void launch_wta(const SlabTable &slabs, uint16_t *wta_l, uint32_t *right_pk, const Geometry &g, const uint16_t *thr,
                int n_frames, hipStream_t s, bool top2) {
    dim3 grid((g.w + kWtaTileX - 1) / kWtaTileX, g.h, n_frames), block(256);
    const size_t lds = (size_t)kWtaTileX * (g.D + 8) * sizeof(uint16_t);
    WtaArgs a{slabs, wta_l, right_pk, g, thr, g.P, {0, 1, 2, 3, 4, 5, 6, 7}};
    with_lpp(g.D, [&](auto lpp) {
        constexpr int LPP = decltype(lpp)::value;
        if (top2) hipLaunchKernelGGL((wta_kernel<LPP, true>), grid, block, lds, s, a);   // S5 variant (CART_OPT_SPEC_S5_TOP2)
        else hipLaunchKernelGGL((wta_kernel<LPP>), grid, block, lds, s, a);
    });
}

// ------------------------------------------------------------------ winner takes all over row bands, "up" path recomputed (plan BAND_UP)
// The "up" path of a pixel depends only on the pixel below it, so a tile of 64 columns x K consecutive rows can recompute it in registers from the
// path's state on the row under the band: the aggregation launch stores that slab only on the rows y % K == 0 (AggArgs::ckpt_rows), and this kernel
// reads the other P-1 slabs -- 2 (P-1 + 1/K) D slab bytes per pixel and launch pair instead of 2 P D -- with wta_kernel's access structure: short-lived
// blocks in address order, each reading 8 KB runs of every slab.  Block = 64 columns x the rows [bK, min(h, bK+K)) of one frame, walked bottom to top,
// 64 LPP threads: one pixel per lane group, wave w on columns P w .. P w + P-1 like a wave of aggregate_kernel, so the right-census window goes through
// the same wave-private LDS staging (Win / WinLane) and the step is the same agg_step.  Per row
//   * census window of the row (prefetched a row ahead) -> LDS -> one agg_step<LPP, false>: the row's "up" costs, in registers,
//   * + the P-1 stored slabs; their loads for row y-1 are issued as soon as row y has been summed, before anything else of row y,
//   * the row's WTA exactly as wta_kernel (packed keys, uniqueness table, sub-pixel from the LDS sum tile, right view through s_rv).
// One LDS-only barrier per row (lds_barrier: the prefetched loads stay in flight across it): s_rv alternates between two buffers, the sum tile is only
// read by the wave that wrote it, and the uniqueness table is copied to LDS so that no load the row has to wait for queues behind the prefetch (vmcnt
// retires in order).  Columns past the image compute on census padding and the clamped last slab column and write nothing.
struct BandArgs {
    const uint32_t *cen_l, *cen_r;
    SlabTable slabs;
    uint16_t *wta_l;
    uint32_t *right_pk;
    Geometry g;
    const uint16_t *thr;   // as WtaArgs::thr
};

// RECOMP = false is the read-rate probe of the design: the same walk over all P stored slabs with no recompute, i.e. wta_kernel's work
// in K-row tiles (CART_OPT_BAND_PROBE; K = 1 is wta_kernel's tiling).
//
// DIAG (CART_OPT_BAND_DIAG) rebuilds the up-right diagonal {dx = +1, dy = -1} (slab kUpRightPath) inside the tile as well and reads one slab less.  Like
// "up" that path advances one row per step of the bottom-to-top walk; its predecessor of pixel (x, y) is (x - 1, y + 1), the pixel the lane group to the
// left finished one row earlier.  The 16 slab-format bytes every lane produces for row y go to s_dg[y & 1][its lane] before the row's barrier, and the
// lane group of column xl reads those of xl - 1 from s_dg[(y + 1) & 1] on the next row.  From HBM the path then needs only
//   * row y1 under the band (all columns; nothing when y1 = h: the path starts fresh on the image's last row, oracle S4), which seeds s_dg[y1 & 1], and
//   * per row the one pixel left of the tile, (x0 - 1, y + 1): a 16-byte load per lane from a wave-uniform base, every pixel of the block reading the
//     same line, issued a row ahead with the slab prefetch and unconditional for every lane (exact counted vmcnt waits); lane group xl = 0 selects it
//     over the LDS value.  At x0 = 0 the load is clamped to column 0 and the value replaced by the fresh state (bytes 0, minimum 0): x = 0 starts a line.
// Both recurrences of a row sit on the same pixel, so the eight packed matching costs are computed once and both run through agg_step_c; the diagonal's
// returned bytes are the slab's own (same kSlabChunkOrder) and enter the sum through sum_add_slab.  The diagonal keeps no registers across rows: its
// state is unpacked from the predecessor's bytes with the checkpoint's two v_perm selectors and its minimum recomputed by path_min.
// s_dg needs TWO buffers and no barrier of its own.  In row y a wave reads buffer (y + 1) & 1 and writes buffer y & 1, both before the barrier of row y.
// A wave that writes buffer (y + 1) & 1 again does so in row y - 1, i.e. after it has passed the barrier of row y, which every wave reaches only after its
// row-y read has returned (lds_barrier waits for lgkmcnt(0)); and the values a wave reads in row y were written before the barrier of row y + 1 (or the
// set-up barrier for the seed).  With one buffer a fast wave's write of row y would race the slower neighbour's read of row y + 1's bytes.
// Columns past the image compute on census padding and clamped slab columns as before and never write.  The path flows rightwards, so such a column can
// never be the predecessor of a valid one -- which is why this diagonal is rebuilt and not its mirror image {-1, -1}.
template <int LPP, int K, bool RECOMP = true, bool DIAG = false>
__global__ __launch_bounds__(64 * LPP, 4) void wta_band_kernel(BandArgs a) {
    using WN = Win<LPP>;
    static_assert(RECOMP || !DIAG, "the diagonal shares the matching costs of the \"up\" recompute");
    constexpr int D = WN::D, P = WN::P, NT = 64 * LPP, NP = kMaxPaths, NS = RECOMP ? (DIAG ? NP - 2 : NP - 1) : NP;
    constexpr int DP = D + 8;                    // LDS pitch of a pixel's sum row (as wta_kernel)
    constexpr int NRV = kWtaTileX + D;
    static_assert(P * LPP == 64 && NT / LPP == kWtaTileX, "one pixel of the tile per lane group");
    __shared__ __attribute__((aligned(16))) uint16_t s_sum[kWtaTileX * DP];
    __shared__ uint32_t s_rv[2][NRV];
    __shared__ uint32_t s_win[RECOMP ? LPP : 1][WN::BUF];     // one window buffer per wave
    __shared__ uint16_t s_thr[2048];
    __shared__ v4u s_dg[DIAG ? 2 : 1][DIAG ? NT : 1];          // DIAG: the diagonal's slab bytes of the previous and of this row, one entry per lane
    const Geometry &g = a.g;
    keep_f16_denormals();
    const int x0 = blockIdx.x * kWtaTileX, frame = blockIdx.z;
    const int y0 = (int)blockIdx.y * K, y1 = min(g.h, y0 + K);   // the band's rows [y0, y1)

    for (int i = threadIdx.x; i < 2 * NRV; i += NT) (&s_rv[0][0])[i] = 0xffffffffu;
    for (int i = threadIdx.x; i < 2048; i += NT) s_thr[i] = a.thr[i];

    UpSweep<LPP> sw;
    sw.init(g, a.cen_l, a.cen_r, a.slabs.frame[frame], frame, x0);
    const int gl = sw.gl, d0 = sw.d0, xl = sw.xl, x = sw.x;
    const bool valid = sw.valid;
    uint32_t *wbuf = &s_win[RECOMP ? sw.wid : 0][0];
    uint32_t cw[WN::NLD], cfl, sv[NS][4];
    // DIAG: slab kUpRightPath at the column left of the tile (clamped to column 0 at x0 = 0, where the value is not used) -- wave-uniform row-0 base,
    // the lane's 16 bytes at d0; dg_rd = where the lane group left of this one put its bytes (xl = 0 reads its own entry and discards it)
    const uint8_t *pc0 = nullptr;
    unsigned lo_c = (unsigned)d0;
    v4u cv = {0u, 0u, 0u, 0u};
    bool colz = true;   // block-uniform: the pixel left of the tile starts the path (x0 = 0, or the row under it is past the image)
    const int dg_wr = (int)threadIdx.x, dg_rd = xl == 0 ? dg_wr : dg_wr - LPP;
    if constexpr (DIAG) pc0 = a.slabs.frame[frame] + uniform((ptrdiff_t)kUpRightPath * (ptrdiff_t)g.slab_bytes + (ptrdiff_t)max(x0 - 1, 0) * D);
    auto load_col = [&](int yy) {
        const uint8_t *pc = pc0 + (ptrdiff_t)yy * sw.row_bytes;
        return __builtin_nontemporal_load((const CART_GLOBAL v4u *)((const CART_GLOBAL char *)sgpr(pc) + pin_v(lo_c)));
    };

    // the path's state under the band: nothing below the image's last row (the scan starts there, oracle S4), else the checkpoint row y1
    uint32_t st[8], mm = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = 0;
    if constexpr (RECOMP) sw.load_census_row(y1 - 1, cw, cfl);
    if (RECOMP && y1 < g.h) {
        const v4u v = sw.load_slab(y1, kUpPath);
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // slab dword q = the low bytes of (st[2q], st[2q+1]) (agg_step's store)
            st[2 * q] = perm(0u, v[q], 0x0c010c00u);
            st[2 * q + 1] = perm(0u, v[q], 0x0c030c02u);
        }
        mm = path_min<LPP>(st);
    }
    if constexpr (DIAG) {
        // the diagonal under the band: row y1 of its slab at the lane's own (clamped) column -- the lane group to the right reads it as its
        // predecessor (x - 1, y1) -- and (x0 - 1, y1) for xl = 0; fresh state when y1 is past the image.  Row y1 is read only when it exists.
        v4u seed = {0u, 0u, 0u, 0u};
        if (y1 < g.h) seed = sw.load_slab(y1, kUpRightPath);
        cv = load_col(min(y1, g.h - 1));
        colz = x0 == 0 || y1 >= g.h;
        sw.template load_slab_row<RECOMP, DIAG>(y1 - 1, sv);
        s_dg[y1 & 1][dg_wr] = seed;   // (after the band's first slab loads have been issued: the store waits for the seed)
    } else {
        sw.template load_slab_row<RECOMP>(y1 - 1, sv);
    }
    lds_barrier();   // s_rv and s_thr (and the seed of s_dg) are set up; the first row's loads stay in flight

    auto row = [&](int y, auto last_c) {
        constexpr bool LAST = decltype(last_c)::value;   // the band's top row: nothing left to prefetch (every VMEM instruction of the body unconditional)
        uint32_t *rvb = &s_rv[y & 1][0];
        uint32_t sm[8];
        if constexpr (RECOMP) {
#pragma unroll
            for (int i = 0; i < WN::NLD; ++i) wbuf[sw.wl.lslot[i]] = cw[i];
            CensusRegs c;
            c.fl = cfl;
            win_read<LPP>(wbuf, sw.wl.rbase, c.r);
            uint32_t xr[16];
            agg_xor(c, xr);
            if constexpr (!LAST) sw.load_census_row(y - 1, cw, cfl);
            if constexpr (DIAG) {
                uint32_t mc[8];   // the pixel's matching costs, once for both recurrences: the pairs agg_step builds from its popcounts
#pragma unroll
                for (int i = 0; i < 8; ++i) mc[i] = ((uint32_t)__builtin_popcount(xr[7 - i]) << 16) + (uint32_t)__builtin_popcount(xr[15 - i]);
                (void)agg_step_c<LPP>(st, mm, mc, sw.sel_lo, sw.sel_hi, sw.p1p1, sw.p2p2);
                sum_from_state(sm, st);
                // the diagonal: predecessor bytes from the lane group to the left (LDS) or, for xl = 0, from the column left of the tile
                const v4u nb = s_dg[(y + 1) & 1][dg_rd];
                const bool edge = xl == 0;
                uint32_t pv[4], ds[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    pv[q] = edge ? (colz ? 0u : cv[q]) : nb[q];
                    ds[2 * q] = perm(0u, pv[q], 0x0c010c00u);       // slab dword q = the low bytes of (ds[2q], ds[2q+1]), as the checkpoint above
                    ds[2 * q + 1] = perm(0u, pv[q], 0x0c030c02u);
                }
                uint32_t dm = path_min<LPP>(ds);
                const v4u dq = agg_step_c<LPP>(ds, dm, mc, sw.sel_lo, sw.sel_hi, sw.p1p1, sw.p2p2);
                s_dg[y & 1][dg_wr] = dq;
                sum_add_slab(sm, dq);
            } else {
                agg_step<LPP, false>(st, mm, xr, sw.sel_lo, sw.sel_hi, sw.p1p1, sw.p2p2, nullptr);
                sum_from_state(sm, st);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) sm[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) sum_add_slab(sm, sv[k]);
        if constexpr (!LAST) {
            if constexpr (DIAG) cv = load_col(y);   // (x0 - 1, y): the predecessor of the tile's first column on row y - 1
            sw.template load_slab_row<RECOMP, DIAG>(y - 1, sv);
        }
        v4u *dst = reinterpret_cast<v4u *>(s_sum + xl * DP + d0);  // LDS tile in natural disparity order
        dst[0] = v4u{sm[0], sm[1], sm[2], sm[3]};
        dst[1] = v4u{sm[4], sm[5], sm[6], sm[7]};
        if (valid) rv_scatter(rvb + (xl + D - 1 - d0), sm, d0);   // columns past the image have no right view
        uint32_t pk, T, tot;
        wta_best_and_sum<LPP>(sm, d0, s_thr, pk, T, tot);
        if (gl == 0 && valid) {   // the sum row read here was written by lanes of this wave (LDS operations of one wave execute in order)
            const WtaPick w = wta_decide<D>(pk, T, tot, s_sum + xl * DP);
            a.wta_l[(size_t)frame * g.npx + (size_t)y * g.w + x] = (uint16_t)wta_subpixel<D>(w);
        }
        lds_barrier();
        // right view (oracle S6): the tile's minima of this row are complete in s_rv[y & 1]; the entry is reset for row y - 2 by the thread that read it
        // (every thread passes the barrier of row y - 1 in between)
        for (int pi = threadIdx.x; pi < kWtaTileX + D - 1; pi += NT) {
            const int p = x0 - (D - 1) + pi;
            const uint32_t best = rvb[pi];
            rvb[pi] = 0xffffffffu;
            if (p >= 0 && p < g.w && best != 0xffffffffu) atomicMin(&a.right_pk[(size_t)frame * g.npx + (size_t)y * g.w + p], best);
        }
    };
    for (int y = y1 - 1; y > y0; --y) {
        row(y, std::false_type{});
        if constexpr (DIAG) colz = x0 == 0;   // rows above the band's first have a row under them
    }
    row(y0, std::true_type{});
}

bool wta_band_supported(const Geometry &g, int K, bool probe) { return g.D == 128 && g.P == kMaxPaths && (K == 4 || K == 8 || K == 16 || (probe && K == 1)); }

void launch_wta_band(const uint32_t *cen_l, const uint32_t *cen_r, const SlabTable &slabs, uint16_t *wta_l, uint32_t *right_pk,
                     const Geometry &g, const uint16_t *thr, int n_frames, int K, bool probe, bool diag, hipStream_t s) {
    dim3 grid((g.w + kWtaTileX - 1) / kWtaTileX, (g.h + K - 1) / K, n_frames), block(64 * (g.D / 16));
    BandArgs a{cen_l, cen_r, slabs, wta_l, right_pk, g, thr};
    if (probe) {
        switch (K) {
            case 1: hipLaunchKernelGGL((wta_band_kernel<8, 1, false>), grid, block, 0, s, a); break;
            case 4: hipLaunchKernelGGL((wta_band_kernel<8, 4, false>), grid, block, 0, s, a); break;
            case 8: hipLaunchKernelGGL((wta_band_kernel<8, 8, false>), grid, block, 0, s, a); break;
            default: hipLaunchKernelGGL((wta_band_kernel<8, 16, false>), grid, block, 0, s, a); break;
        }
        return;
    }
    if (diag) {
        switch (K) {
            case 4: hipLaunchKernelGGL((wta_band_kernel<8, 4, true, true>), grid, block, 0, s, a); break;
            case 8: hipLaunchKernelGGL((wta_band_kernel<8, 8, true, true>), grid, block, 0, s, a); break;
            default: hipLaunchKernelGGL((wta_band_kernel<8, 16, true, true>), grid, block, 0, s, a); break;
        }
        return;
    }
    switch (K) {
        case 4: hipLaunchKernelGGL((wta_band_kernel<8, 4>), grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL((wta_band_kernel<8, 8>), grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL((wta_band_kernel<8, 16>), grid, block, 0, s, a); break;
    }
}

// ------------------------------------------------------------------ winner takes all, fused with the "up" direction
// For batches the slab of ONE direction never has to exist: this kernel sweeps every column bottom-up, computes the
// "up" path costs on the fly (the same agg_step, registers only), adds the other P-1 slabs and runs the WTA of the row
// it is on.  That removes 1/P of the slab writes and reads (the launch sequence is HBM bound: aggregate writes at
// ~4.6 TB/s, WTA reads at ~6 TB/s).  Block = 4 waves = 4*P adjacent columns, one image row per step; per step
//   * cost recurrence of the block's columns (wave-private right-census window through LDS like aggregate_kernel),
//   * S = L_up + sum of the stored slabs (16-byte non-temporal loads, prefetched one step ahead),
//   * left disparity exactly as wta_kernel (packed keys, integer uniqueness threshold, sub-pixel from the LDS tile),
//   * right view: every lane min-reduces its 16 (S<<16|d) keys into a block-local LDS array indexed by p = x - d
//     (ds_min_u32); the block's NR = 4P + D - 1 minima of the row go to a per-block partial buffer with plain stores
//     and rv_merge_kernel takes the min over the <= ceil((D-1)/4P)+1 blocks that cover a right pixel (global atomics
//     straight from this kernel cost 0.16 ms per 16-frame launch, the partial buffer is 2 % of the slab traffic).
// The row loop has no block barrier (the LDS sum tile is only read by the wave that wrote it); left disparities and
// right-view minima are buffered in LDS for 16 rows and written out in one burst between two barriers, so the row
// loop itself holds loads only and the prefetches stay in flight while a row is processed.
// Waves per block of the fused sweep.  The sweep has frames*W/(64/LPP) waves in total (2484 at 16 x 1242, D=128: 2.4 per
// SIMD), so small blocks spread them evenly over the CUs: with 4-wave blocks a quarter of the CUs carried 3 blocks, the
// rest 2, and the launch took the time of 3.  D=256 keeps 4 waves: its blocks would otherwise be 8 columns wide and the
// right-view partial rows (columns + D - 1 entries per block and row) would grow to 17 % of the slab traffic.
constexpr int fused_waves(int lpp) { return lpp >= 16 ? 4 : 2; }
constexpr int kFusedRB = 16;   // rows buffered in LDS between two bursts of the fused sweep (8 and 32 measured level / slower)
// ... except on wide images at D = 256, where blocks of 8 waves (32 columns) give ~one block per CU and halve the partial
// right-view rows again: 1920x1080, 4 frames: 2.65 instead of 3.08 ms per launch (at 1242 wide 8 waves lose 10 %)
inline int fused_waves_for(const Geometry &g) { return g.D >= 256 && g.w >= 1600 ? 2 * fused_waves(16) : fused_waves(g.D / 16); }


struct FusedArgs {
    const uint32_t *cen_l, *cen_r;
    SlabTable slabs;
    uint16_t *wta_l;
    uint32_t *partial;   // [frame][block][sweep step][rv_row_slots] u16 right-view minima of every block (rv_key16; last slot of a row: unused sink)
    Geometry g;
    const uint16_t *thr; // as WtaArgs::thr
    int xcd_frames;      // xcd_placement(): blocks are decoded per XCD
};

template <int LPP, int NP>
struct FusedRegs {
    uint32_t win[Win<LPP>::NLD];
    uint32_t fl;
    uint32_t sv[2][NP - 1][4];   // two rows of slab bytes in flight (see the Little's-law note at the kernel; one row at <= 128 VGPRs measured slower, profiles/r04_fused.txt)
};

// NP = number of paths (compile time: every VMEM instruction of the row loop is unconditional, so that the compiler
// can use exact counted vmcnt waits and the loads of row y-1 stay in flight while row y is processed)
template <int LPP, int NP, int WPB_ = fused_waves(LPP)>
__global__ __launch_bounds__(64 * WPB_, 3) void wta_fused_kernel(FusedArgs a) {  // >= 3 waves per SIMD (HIP: min waves per EU); 4 for the 4-path variants (120 VGPRs, 39 KB of LDS) measured the same
    using WN = Win<LPP>;
    constexpr int WPB = WPB_, NT = 64 * WPB;
    constexpr bool RVPAD = LPP == 16 && NP == 4;   // see rv_slot
    constexpr int P = WN::P, D = WN::D, COLS = WPB * P, NR = COLS + D - 1, NRP = rv_row_slots(COLS, D, RVPAD);   // slots per row, the last one a spare
    static_assert(COLS == 16 || COLS == 32, "rv_key16 packs the column into 4 or 5 bits");
    static_assert((RVPAD ? rv_slot(NR - 1) : NR - 1) < NRP - 1, "the row's last slot is a spare");
    __shared__ uint32_t s_win[WPB][WN::BUF];
    constexpr int DP = D + 8;                    // LDS pitch of a pixel's sum row (16 B of padding against bank conflicts)
    __shared__ __attribute__((aligned(16))) uint16_t s_tile[1][COLS * DP];
    constexpr int RB = kFusedRB;                 // rows buffered in LDS between two bursts (32 rows cost an LDS-limited block per CU)
    __shared__ __attribute__((aligned(16))) uint32_t s_rmin[RB][NRP];
    __shared__ uint2 s_rec[RB][COLS];            // per pixel: best disparity, unique flag, best cost | its two neighbour costs
    constexpr int NTHR = NP <= 4 ? 1024 : 2048;  // sums are <= NP * 255
    __shared__ uint16_t s_thr[NTHR];             // uniqueness threshold by best cost
    const Geometry &g = a.g;
    keep_f16_denormals();
    const int nblk = (g.w + COLS - 1) / COLS;
    // same XCD placement as aggregate_kernel (frames x, x + 8, ... on XCD x): the sweep re-reads the census planes the
    // aggregation launch has just pulled into that XCD's L2
    int bid = (int)blockIdx.x, frame0 = 0, fstep = 1;
    if (a.xcd_frames) { frame0 = bid & 7; bid >>= 3; fstep = 8; }
    const int frame = frame0 + fstep * (bid / nblk), blk = bid - (bid / nblk) * nblk, x0 = blk * COLS;
    const int hpad = (g.h + RB - 1) / RB * RB + RB;   // rows of one block in the partial buffer (see flush)

    for (int i = threadIdx.x; i < RB * NRP; i += NT) (&s_rmin[0][0])[i] = 0xffffffffu;
    for (int i = threadIdx.x; i < NTHR; i += NT) s_thr[i] = a.thr[i];

    UpSweep<LPP> sw;
    sw.init(g, a.cen_l, a.cen_r, a.slabs.frame[frame], frame, x0);
    const int wid = sw.wid, gl = sw.gl, d0 = sw.d0, xl = sw.xl;
    const bool valid = sw.valid;
    uint32_t *wbuf = &s_win[wid][0];

    // Census registers: one set, re-loaded for row y-1 as soon as row y has consumed it.  Slab registers: two sets, each
    // re-loaded for row y-2 when row y has consumed it -- the sweep has only frames*W/P waves (2484 at 16 x 1242, D=128)
    // with 7 KB of slab bytes per wave and row, and one row in flight (17 MB) capped the reads at 4.7 TB/s.
    FusedRegs<LPP, NP> r;
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = 0;
    uint32_t mm = 0;

    // The two halves of a row are split so that they can be software-pipelined: agg(y) advances the "up" path state to
    // row y (the only cross-row dependency), wta(...) runs the WTA of the PREVIOUS row on a copy of its state.  The two
    // instruction streams are independent, so the scheduler interleaves them and the long latency chains of one (LDS
    // round trips, DPP reductions) are filled with the other's work.
    auto agg = [&](int y) {   // census registers hold row y; they are re-loaded for row y-1 once consumed
#pragma unroll
        for (int i = 0; i < WN::NLD; ++i) wbuf[sw.wl.lslot[i]] = r.win[i];
        CensusRegs c;
        c.fl = r.fl;
        win_read<LPP>(wbuf, sw.wl.rbase, c.r);
        uint32_t xr[16];
        agg_xor(c, xr);
        sw.load_census_row(max(y - 1, 0), r.win, r.fl);
        agg_step<LPP, false>(st, mm, xr, sw.sel_lo, sw.sel_hi, sw.p1p1, sw.p2p2, nullptr);
    };

    auto wta = [&](const uint32_t (&sp)[8], int lr, int y, auto set_c) {   // sp: path costs of row y; lr: LDS output row
        constexpr int SET = decltype(set_c)::value;
        uint32_t sm[8];
        sum_from_state(sm, sp);
#pragma unroll
        for (int k = 0; k < NP - 1; ++k) sum_add_slab(sm, r.sv[SET][k]);
        sw.template load_slab_row<true>(max(y - 2, 0), r.sv[SET]);   // this slab set is free again: prefetch row y-2 into it
        uint16_t *tile = &s_tile[0][0];   // single buffer: every wave only touches the rows of its own pixels
        v4u *dst = reinterpret_cast<v4u *>(tile + xl * DP + d0);
        dst[0] = v4u{sm[0], sm[1], sm[2], sm[3]};
        dst[1] = v4u{sm[4], sm[5], sm[6], sm[7]};
        uint32_t pk, T, tot;
        wta_best_and_sum<LPP>(sm, d0, s_thr, pk, T, tot);   // the float search of uniq_threshold runs once per engine, not per row
        // ---- right view (oracle S6): key (S<<16 | d) into slot p - (x0 - (D-1)) = xl + D-1 - d.  (Issued before the pixel record below:
        // after it, the record's LDS reads no longer queue behind the atomics, and the sweep was 4 % SLOWER, profiles/r04_fused.txt.)
        if (valid) {
            uint32_t *rrow = &s_rmin[lr][0];
            if constexpr (RVPAD) {
                // Padded rows (rv_slot): slot of entry base - j = s0 - j - [j > b4] with b4 = (xl - 1) & 15 and xl = 4 wid + pg (P = 4 pixels
                // per wave, 16 lanes each): the pad's carry depends on the lane only through pg = lane >> 4, and on the wave only through
                // wid & 3.  One code version per wave class, in which every carry is a COMPILE-TIME lane mask: no lane (slot s0 - j), every
                // lane (s0 - 1 - j), or one of six partial masks (one v_cndmask, shared by the j's with the same mask).  <= 3 selects per
                // row instead of 45 compare / select / shift instructions (246 instead of 288 VALU per wave-step): the D=256 / 4-path
                // sweep 1.36 -> 1.29 ms per 16 frames, means of five alternating runs (profiles/r04_fused.txt).
                static_assert(P == 4 && LPP == 16, "lane masks below assume four 16-lane pixels per wave");
                const int s0 = rv_slot(xl + D - 1 - d0);
                auto emit = [&](auto wc) {
                    constexpr int W4 = decltype(wc)::value;
                    const int ia = s0, ib = s0 - 1;
                    int base = ia;                     // s0 or s0 - 1 per lane: an INDEX into the row (the select works on 32-bit values, never on pointers)
                    unsigned long long prev = 0;       // the carry mask `base` was made for: masks only grow with j, so equal masks are adjacent
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        unsigned long long mask = 0;   // lanes whose slot carries the pad: j > b4(pg)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (j > ((4 * W4 + q - 1) & 15)) mask |= 0xffffull << (16 * q);
                        if (mask != prev) {
                            if (mask == ~0ull) base = ib;
                            // The lane mask goes into VCC as two 32-bit halves.  Handed over as ONE 64-bit "s" operand, the compiler
                            // rematerialises it with s_mov_b64 and a 32-bit literal, and 0x00000000ffff0000 and 0xffffffffffff0000 then
                            // share one encoding (literal 0xffff0000): the last two rows of every sweep came out wrong that way.
                            else asm volatile("s_mov_b32 vcc_lo, %3\n\ts_mov_b32 vcc_hi, %4\n\tv_cndmask_b32 %0, %1, %2, vcc"
                                              : "=v"(base) : "v"(ia), "v"(ib), "i"((int)(uint32_t)mask), "i"((int)(uint32_t)(mask >> 32)) : "vcc");
                            prev = mask;
                        }
                        const int q = j < 8 ? j / 2 : 4 + (j - 8) / 2;   // sm[q] holds local disparities (2q', 2q'+1), low / high half
                        const uint32_t keyv = (j & 1) ? ((sm[q] & 0xffff0000u) | (uint32_t)(d0 + j)) : ((sm[q] << 16) | (uint32_t)(d0 + j));
                        atomicMin(rrow + (base - j), keyv);   // - j rides on the instruction's immediate offset
                    }
                };
                switch (wid & 3) {   // wave-uniform
                    case 0: emit(std::integral_constant<int, 0>{}); break;
                    case 1: emit(std::integral_constant<int, 1>{}); break;
                    case 2: emit(std::integral_constant<int, 2>{}); break;
                    default: emit(std::integral_constant<int, 3>{}); break;
                }
            } else {
                rv_scatter(rrow + (xl + D - 1 - d0), sm, d0);
            }
        }
        // No block barrier: the tile rows a lane reads below are its own pixel's, written by lanes of the same wave (LDS
        // operations of one wave execute in order); the block-wide arrays (s_rmin, s_rec) are only read in the burst.
        // The pixel's first lane records (best d, unique?, best cost | neighbour costs); the sub-pixel division is
        // deferred to the burst, where all lanes work on it.
        if (gl == 0) {
            // wta_decide's text (and wta_subpixel's in flush), kept here: through the shared functions the D = 256 / 4-path sweeps take 142 and 139
            // instead of 140 and 126 VGPRs (profiles/wta_refactor.txt); per kernel template, as for wta_kernel's scatter
            const int bd = (int)(pk & 0xffffu), bc = (int)(pk >> 16);
            const uint16_t *srow = tile + xl * DP;
            const int l = bd > 0 ? srow[bd - 1] : 0x7fff, rr = bd < D - 1 ? srow[bd + 1] : 0x7fff;
            const int Ti = (int)T;
            const int tot_nbr = max(Ti - bc, 0) + max(Ti - l, 0) + max(Ti - rr, 0);
            const uint32_t unique = (int)tot == tot_nbr ? 1u : 0u;
            s_rec[lr][xl] = make_uint2((uint32_t)bd | (unique << 8) | ((uint32_t)bc << 9), (uint32_t)l | ((uint32_t)rr << 16));
        }
    };

    // one pipelined iteration: WTA of sweep step r (image row h-1-r) + path costs of step r+1
    auto iter = [&](int r_, int lr, auto set_c) {
        uint32_t sp[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) sp[i] = st[i];
        agg(g.h - 2 - r_);
        wta(sp, lr, g.h - 1 - r_, set_c);
    };

    // Burst of the buffered rows (LDS row r holds image row ytop + nrows-1-r).  Stores inside the row loop would sit
    // between the prefetch loads in vmcnt's in-order retirement; the row loop itself is branch-free and holds loads only.
    // Burst of the buffered rows.  It is branch-free with a fixed number of stores per lane: the partial buffer is laid out
    // [frame][block][sweep step][NRP u16 keys] (rows padded to a multiple of RB), so a burst is one linear copy of RB*NRP slots
    // (rows past the last one land in the padding), and the few left-disparity stores of dead lanes go to a sink entry.
    // With a data-dependent store count (or addresses that spill) the compiler cannot count the VMEM operations between
    // the prefetches issued before the burst and their use after it and waits for everything, including the
    // acknowledgement of the burst's own stores: ~13 us per burst, 0.3 ms per 16-frame launch.
    auto flush = [&](int t0, int nrows) {   // LDS row r = sweep step t0 + r = image row h-1-t0-r
        lds_barrier();
        // partial rows hold u16 keys (rv_key16): NRP / 2 dwords per row
        uint32_t *pbase = a.partial + (((size_t)frame * nblk + blk) * (size_t)hpad + t0) * (NRP / 2);
#pragma unroll
        for (int i0 = 0; i0 < RB * COLS; i0 += NT) {
            const int i = min(i0 + (int)threadIdx.x, RB * COLS - 1);
            const int r = i / COLS, c = i - r * COLS;
            const uint2 rec = s_rec[r][c];
            const int bd = (int)(rec.x & 0xffu), bc = (int)(rec.x >> 9), l = (int)(rec.y & 0xffffu), rr = (int)(rec.y >> 16);
            uint32_t out = kWtaInvalid;
            if (rec.x & 0x100u) {  // oracle S5 sub-pixel (wta_subpixel's text, see the row loop)
                int subp = bd * 16;
                if (bd > 0 && bd < D - 1) {
                    const int num = l - rr, den = l - 2 * bc + rr;
                    if (den != 0) subp += (num * 16 + den) / (2 * den);
                }
                out = (uint32_t)subp & 0xffffu;
            }
            const bool live = r < nrows && x0 + c < g.w && i0 + (int)threadIdx.x < RB * COLS;
            uint16_t *dst = live ? a.wta_l + (size_t)frame * g.npx + (size_t)(g.h - 1 - t0 - r) * g.w + x0 + c
                                 : reinterpret_cast<uint16_t *>(pbase) + NRP - 1;   // the spare slot of the chunk's first row
            *dst = (uint16_t)out;
        }
        static_assert(RB * NRP % 8 == 0, "a lane packs eight right-view slots into one 16-byte store");
#pragma unroll
        for (int i0 = 0; i0 < RB * NRP / 8; i0 += NT) {
            const int i = i0 + (int)threadIdx.x;
            const bool live = i < RB * NRP / 8;   // excess lanes store ones into the last (never used) row of the block's area
            const v4u ones = v4u{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
            v4u v = ones;
            if (live) {
                v4u *src = reinterpret_cast<v4u *>(&s_rmin[0][0]) + 2 * i;
                const v4u t0v = src[0], t1v = src[1];
                src[0] = ones; src[1] = ones;
                v = v4u{rv_key16(t0v.x, COLS) | (rv_key16(t0v.y, COLS) << 16), rv_key16(t0v.z, COLS) | (rv_key16(t0v.w, COLS) << 16),
                        rv_key16(t1v.x, COLS) | (rv_key16(t1v.y, COLS) << 16), rv_key16(t1v.z, COLS) | (rv_key16(t1v.w, COLS) << 16)};
            }
            v4u *dst = live ? reinterpret_cast<v4u *>(pbase) + i
                            : reinterpret_cast<v4u *>(a.partial + (((size_t)frame * nblk + blk + 1) * (size_t)hpad) * (NRP / 2)) - 1;
            *dst = v;
        }
        lds_barrier();
    };

    __syncthreads();
    sw.load_census_row(g.h - 1, r.win, r.fl);
    sw.template load_slab_row<true>(g.h - 1, r.sv[0]);
    sw.template load_slab_row<true>(max(g.h - 2, 0), r.sv[1]);
    agg(g.h - 1);
    flush(0, 0);   // writes nothing that survives (chunk 0 is rewritten by its own burst); it only gives the first entry into
                   // the chunk loop the same VMEM history as every later one, so that the counted waits after a burst stand
    // Sweep steps r = 0..h-1 (image row h-1-r, slab set r & 1).  The pipelined iterations cover r = 0..h-2 in chunks of RB,
    // two per loop trip, straight-line; what is left (one pipelined iteration if h-1 is odd, then the WTA of the last row)
    // runs after the loop: inside it the compiler would have to assume "odd tail, then another chunk" and would shrink the
    // counted waits of slab set 0 to one row in flight.
    const int r_even = (g.h - 1) & ~1;
    for (int r0 = 0; r0 < r_even; r0 += RB) {
        const int nrows = min(RB, r_even - r0);
        // the first pair is peeled so that the waits right after a burst are computed for that history alone (20 stores
        // behind the prefetches) instead of being merged with the loop's back edge
        iter(r0, 0, std::integral_constant<int, 0>{});
        iter(r0 + 1, 1, std::integral_constant<int, 1>{});
        for (int k = 2; k < nrows; k += 2) {
            iter(r0 + k, k, std::integral_constant<int, 0>{});
            iter(r0 + k + 1, k + 1, std::integral_constant<int, 1>{});
        }
        flush(r0, nrows);
    }
    if ((g.h - 1) & 1) {
        iter(r_even, 0, std::integral_constant<int, 0>{});
        wta(st, 1, 0, std::integral_constant<int, 1>{});
        flush(r_even, 2);
    } else {
        wta(st, 0, 0, std::integral_constant<int, 0>{});
        flush(r_even, 1);
    }
}

// right_pk[p] = min over the blocks whose p-range [blk*COLS - (D-1), blk*COLS + COLS - 1] holds p.
// partial = [frame][block][sweep step t = h-1-y][rv_row_slots u16 keys] (rows padded, see wta_fused_kernel's flush)
// At most NB = ceil((D-1)/COLS) + 1 blocks cover a right pixel (17 at D = 256 with 16-column blocks): all NB keys are requested at once,
// out-of-range blocks clamped onto the first one and masked, so that the loads do not wait for each other (as a loop over b0..b1 the
// merge took 0.14 ms per 16-frame launch at D = 256 / 4 paths: a tenth of the sweep it follows).
template <int D, int COLS, bool PADDED>
__global__ __launch_bounds__(256) void rv_merge_kernel(const uint32_t *partial, uint32_t *right_pk, int w, int h, int nblk) {
    constexpr int NB = (D - 1 + COLS - 1) / COLS + 1, NRP = rv_row_slots(COLS, D, PADDED);
    const int p = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), frame = blockIdx.z;
    if (p >= w || y >= h) return;
    const int hpad = (h + kFusedRB - 1) / kFusedRB * kFusedRB + kFusedRB;
    const uint16_t *keys = reinterpret_cast<const uint16_t *>(partial) + ((size_t)frame * nblk * hpad + (size_t)(h - 1 - y)) * NRP;
    const int b0 = p / COLS, b1 = min((p + D - 1) / COLS, nblk - 1);
    uint32_t k[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int b = min(b0 + i, b1);
        const int e = p - (b * COLS - (D - 1));
        k[i] = keys[(size_t)b * hpad * NRP + (PADDED ? rv_slot(e) : e)];
    }
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int b = min(b0 + i, b1);   // (a clamped duplicate of the last block changes nothing)
        if (k[i] != 0xffffu) best = min(best, rv_key32(k[i], p - (b * COLS - (D - 1)), COLS, D));
    }
    right_pk[((size_t)frame * h + y) * w + p] = best;
}

inline bool fused_rv_padded(const Geometry &g) { return g.D >= 256 && g.P == 4; }   // = RVPAD of the kernel that will run

size_t wta_fused_partial_elems(const Geometry &g) {
    const int cols = fused_waves_for(g) * (64 / (g.D / 16));
    const int hpad = (g.h + kFusedRB - 1) / kFusedRB * kFusedRB + kFusedRB;
    return (size_t)hpad * ((g.w + cols - 1) / cols) * (rv_row_slots(cols, g.D, fused_rv_padded(g)) / 2);   // u32 elements of u16 keys
}

void launch_wta_fused(const uint32_t *cen_l, const uint32_t *cen_r, const SlabTable &slabs, uint16_t *wta_l, uint32_t *right_pk,
                      uint32_t *partial, const Geometry &g, const uint16_t *thr, int n_frames, hipStream_t s) {
    FusedArgs a{cen_l, cen_r, slabs, wta_l, partial, g, thr, xcd_placement(g, n_frames) ? 1 : 0};
    const int wpb = fused_waves_for(g), cols = wpb * (64 / (g.D / 16));
    const int nblk = (g.w + cols - 1) / cols;
    dim3 grid(nblk * n_frames), block(64 * wpb);
    const bool wide = wpb != fused_waves(g.D / 16);   // D = 256 on wide images: twice the waves per block
    with_lpp(g.D, [&](auto lpp) {
        constexpr int LPP = decltype(lpp)::value;
        auto go = [&](auto np) {
            constexpr int NP = decltype(np)::value;
            if constexpr (LPP == 16) {
                if (wide) { hipLaunchKernelGGL((wta_fused_kernel<16, NP, 2 * fused_waves(16)>), grid, block, 0, s, a); return; }
            }
            hipLaunchKernelGGL((wta_fused_kernel<LPP, NP>), grid, block, 0, s, a);
        };
        if (g.P == 4) go(std::integral_constant<int, 4>{});
        else go(std::integral_constant<int, 8>{});
    });
    const dim3 mgrid((g.w + 63) / 64, (g.h + 3) / 4, n_frames), mblock(256);
    const bool padded = fused_rv_padded(g);
#define CART_MERGE(DD, CC, PP) hipLaunchKernelGGL((rv_merge_kernel<DD, CC, PP>), mgrid, mblock, 0, s, (const uint32_t *)partial, right_pk, g.w, g.h, nblk)
    if (g.D == 64) CART_MERGE(64, 32, false);
    else if (g.D == 128) CART_MERGE(128, 16, false);
    else if (cols == 32) { if (padded) CART_MERGE(256, 32, true); else CART_MERGE(256, 32, false); }
    else { if (padded) CART_MERGE(256, 16, true); else CART_MERGE(256, 16, false); }
#undef CART_MERGE
}

}  // namespace cart_amd

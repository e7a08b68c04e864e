// sgm_device.h -- device helpers shared by the SGM kernel files (sgm_census.hip, sgm_aggregate.hip, sgm_wta.hip, sgm_post.hip):
// packed-u16 arithmetic, DPP reductions inside a pixel's lane group, scalar-base addressing, the cost recurrence step and the
// LDS staging of the right-census window.  Private to those files; the launchers are declared in engine_internal.h.
#pragma once

#include <type_traits>

#include "engine_internal.h"

namespace cart_amd {

// ------------------------------------------------------------------ packed u16 pairs (layout: see the path aggregation notes in sgm_aggregate.hip)
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));   // one 16-byte load / store

__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// min of three packed u16 pairs in ONE instruction: gfx950's v_pk_minimum3_f16 applied to the bit patterns.  Valid where every operand
// half is a cost below 0x7C00 (no inf / NaN pattern; non-negative, so IEEE order = unsigned order) -- the recurrence's operands are
// <= 255 + P2 < 1024, i.e. f16 denormals, which the wave's mode register must preserve (keep_f16_denormals below).  Issue cost as
// v_pk_min_u16 (profiles/tools/valu_rate.hip), so each use saves one of ~100 instructions of the VALU-bound step.
// (A/B against two v_pk_min_u16: profiles/r03_min3.txt.)  The instruction exists on gfx950 only -- the one target the SGM files are written
// for; the host pass of the compiler and any other --offload-arch get the two-instruction form.
__device__ __forceinline__ uint32_t pk_min3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__gfx950__)
    uint32_t r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return pk_min(pk_min(a, b), c);
#endif
}
// MODE.FP_DENORM[3:2] (f16 / f64) = 3: denormals in and out.  That is the code object's default mode, and the default is what pk_min3
// relies on (the asm above carries no dependency on this s_setreg, so the compiler may order the two freely; every kernel that uses
// pk_min3 still states the mode once at its entry, so that a changed default cannot go unnoticed).  hwreg(HW_REG_MODE = 1, offset 6, width 2)
__device__ __forceinline__ void keep_f16_denormals() { __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 3); }
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t perm(uint32_t hi_src, uint32_t lo_src, uint32_t sel) {
    return __builtin_amdgcn_perm(hi_src, lo_src, sel);  // selector bytes: 0-3 = lo_src, 4-7 = hi_src, 0x0c = 0x00, 0x0d = 0xFF
}

// ------------------------------------------------------------------ DPP helpers
constexpr int DPP_ROW_SHL1 = 0x101;
constexpr int DPP_ROW_SHR1 = 0x111;
constexpr int DPP_QUAD_XOR1 = 0xB1;   // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;   // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;
constexpr int DPP_ROW_MIRROR = 0x140;

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

// all-reduce (min) over the LPP lanes that own one pixel; v is an unsigned key
template <int LPP>
__device__ __forceinline__ uint32_t group_allmin(uint32_t v) {
    v = min(v, dpp_mov<DPP_QUAD_XOR1>(v));
    v = min(v, dpp_mov<DPP_QUAD_XOR2>(v));
    if constexpr (LPP >= 8) v = min(v, dpp_mov<DPP_ROW_HALF_MIRROR>(v));
    if constexpr (LPP >= 16) v = min(v, dpp_mov<DPP_ROW_MIRROR>(v));
    return v;
}

template <int LPP>
__device__ __forceinline__ uint32_t group_allsum(uint32_t v) {
    v += dpp_mov<DPP_QUAD_XOR1>(v);
    v += dpp_mov<DPP_QUAD_XOR2>(v);
    if constexpr (LPP >= 8) v += dpp_mov<DPP_ROW_HALF_MIRROR>(v);
    if constexpr (LPP >= 16) v += dpp_mov<DPP_ROW_MIRROR>(v);
    return v;
}

// wave-uniform values kept in SGPRs: per-lane addresses become "scalar base + 32-bit lane offset" (saddr form), and
// the per-step pointer increments run on the scalar unit instead of 64-bit VALU adds
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ ptrdiff_t uniform(ptrdiff_t v) {  // element offsets from kernel-argument bases (pointer provenance kept)
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (ptrdiff_t)(((uint64_t)hi << 32) | lo);
}

// Pins a wave-uniform pointer into an SGPR pair so that "pointer + zero-extended 32-bit lane byte offset" selects the
// scalar-base addressing form (global_load ... v_off, s[base:base+1]) instead of a 64-bit VALU add per access.  The
// result is typed as a GLOBAL-address-space pointer: the asm hides the kernel-argument provenance the compiler would
// otherwise use to pick global_* over flat_* instructions.
#define CART_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ CART_GLOBAL T *sgpr(T *p) {
    asm volatile("" : "+s"(p));
    return (CART_GLOBAL T *)p;
}
// keeps the zero-extension of a lane offset next to its use: hoisted out of the loop as a 64-bit value it would no longer
// match the scalar-base addressing pattern
__device__ __forceinline__ unsigned pin_v(unsigned &off) {  // in place: no register copy
    asm volatile("" : "+v"(off));
    return off;
}
__device__ __forceinline__ uint32_t ld_u32(const uint32_t *ubase, unsigned &byte_off) {
    return *(const CART_GLOBAL uint32_t *)((const CART_GLOBAL char *)sgpr(ubase) + pin_v(byte_off));
}

struct CensusRegs {
    uint32_t fl;
    uint32_t r[16];
};

// x[k] = left feature ^ right feature k: consumes the loaded registers right away so that the next
// prefetch can land in them while the rest of the step runs
__device__ __forceinline__ void agg_xor(const CensusRegs &c, uint32_t (&xr)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) xr[k] = c.fl ^ c.r[k];
}

// min over the pixel's D path costs (split-halves registers), replicated into both halves: the (m,m) operand of the next step
template <int LPP>
__device__ __forceinline__ uint32_t path_min(const uint32_t (&n)[8]) {
    uint32_t x = pk_min(pk_min3(n[0], n[1], n[2]), pk_min3(n[3], n[4], pk_min3(n[5], n[6], n[7])));
    x = pk_min(x, __builtin_amdgcn_alignbit(x, x, 16));
    return group_allmin<LPP>(x);
}

// store_row (wave-uniform): false skips the slab store of this step -- the checkpointed "up" scan of plan BAND_UP
template <int LPP, bool STORE = true>
__device__ __forceinline__ void agg_step(uint32_t (&a)[8], uint32_t &mm, const uint32_t (&xr)[16], uint32_t sel_lo,
                                         uint32_t sel_hi, uint32_t p1p1, uint32_t p2p2, CART_GLOBAL uint8_t *po, bool store_row = true) {
    // Issue cost on gfx950 (profiles/tools/valu_rate.hip): v_add/v_sub/v_xor ~2.7 clk, packed ops / v_perm / v_bcnt /
    // shifts ~4.5 clk.  Wherever a packed op cannot carry or borrow between the halves, the plain 32-bit one is used.
    const uint32_t mp2 = mm + p2p2;  // halves stay < 2^15
    // neighbour vectors at the two ends: (prev lane's L[d0-1], own L[d0+7]) and (own L[d0+8], next lane's L[d0+16])
    const uint32_t lo0 = perm(a[7], dpp_mov<DPP_ROW_SHR1>(a[7]), sel_lo);
    const uint32_t hi7 = perm(dpp_mov<DPP_ROW_SHL1>(a[0]), a[0], sel_hi);
    uint32_t n[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t lo = i == 0 ? lo0 : a[i - 1];
        const uint32_t hi = i == 7 ? hi7 : a[i + 1];
        uint32_t t = pk_min(lo, hi) + p1p1;  // no carry between halves (min(lo,hi) is a real cost < 2^15)
        t = pk_min3(t, a[i], mp2);
        // oracle S4: L = C + (min(...) - m).  Every candidate of the min is >= m in both halves, so "- m" is a plain
        // 32-bit subtract; the low-half cost rides on v_bcnt's accumulate operand, the high-half one is shifted in.
        uint32_t u = t - mm;
        asm volatile("" : "+v"(u));  // keep the three adds apart: v_sub (fast), v_bcnt with accumulate, v_lshl_add
        uint32_t lo_sum = (uint32_t)__builtin_popcount(xr[15 - i]) + u;
        asm volatile("" : "+v"(lo_sum));
        n[i] = ((uint32_t)__builtin_popcount(xr[7 - i]) << 16) + lo_sum;
    }
    // u8 slab bytes of the lane's 16 disparities in the kernel's native order (one v_perm per register pair): dword q
    // holds d0 + {2q, 2q+8, 2q+1, 2q+9}; the WTA widens byte pairs straight back into the same split-halves registers
    // (slab byte layout: see kSlabChunkOrder in engine_internal.h)
    if constexpr (STORE) {
        uint4 o;
        o.x = perm(n[1], n[0], 0x06040200u); o.y = perm(n[3], n[2], 0x06040200u);
        o.z = perm(n[5], n[4], 0x06040200u); o.w = perm(n[7], n[6], 0x06040200u);
        // write-once streaming data: non-temporal so the slabs do not evict the census planes from L2
        const v4u q = {o.x, o.y, o.z, o.w};
        if (store_row) __builtin_nontemporal_store(q, (CART_GLOBAL v4u *)po);
    } else {
        (void)po; (void)store_row;  // the fused and banded WTA consume the new costs from the registers
    }
    mm = path_min<LPP>(n);
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = n[i];
}

template <int LPP>
__device__ __forceinline__ v4u agg_step_c(uint32_t (&a)[8], uint32_t &mm, const uint32_t (&c)[8], uint32_t sel_lo, uint32_t sel_hi,
                                          uint32_t p1p1, uint32_t p2p2) {
    // agg_step with the matching costs handed in: c[i] = (C[d0+8+i] << 16) + C[d0+i], the pair agg_step builds from its popcounts;
    // returns the lane's 16 slab bytes (the caller stores them).  Used where one cost vector serves more than one consumer: the split
    // horizontal scans of aggregate_kernel (producer / consumer waves) and the two recurrences of wta_band_kernel<.., DIAG = true>.
    const uint32_t mp2 = mm + p2p2;
    const uint32_t lo0 = perm(a[7], dpp_mov<DPP_ROW_SHR1>(a[7]), sel_lo);
    const uint32_t hi7 = perm(dpp_mov<DPP_ROW_SHL1>(a[0]), a[0], sel_hi);
    uint32_t n[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t lo = i == 0 ? lo0 : a[i - 1];
        const uint32_t hi = i == 7 ? hi7 : a[i + 1];
        uint32_t t = pk_min(lo, hi) + p1p1;
        t = pk_min3(t, a[i], mp2);
        n[i] = (t - mm) + c[i];   // both halves of t are >= m (see agg_step)
    }
    const v4u q = {perm(n[1], n[0], 0x06040200u), perm(n[3], n[2], 0x06040200u), perm(n[5], n[4], 0x06040200u), perm(n[7], n[6], 0x06040200u)};
    uint32_t x = pk_min(pk_min3(n[0], n[1], n[2]), pk_min3(n[3], n[4], pk_min3(n[5], n[6], n[7])));
    x = pk_min(x, __builtin_amdgcn_alignbit(x, x, 16));
    mm = group_allmin<LPP>(x);
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = n[i];
    return q;
}

// ---- LDS staging of the right-census window (vertical + diagonal directions) ----
// The P = 64/LPP pixels a wave works on at one step are adjacent columns of one image row, so the
// P windows of D right features overlap in all but P-1 entries.  Per-lane window loads cost 4 B per
// DP cell through the L1->VGPR path (rocprofv3: TA_BUSY 76 %, TD_BUSY 78 %, 3x line-access inflation
// from the 4-byte-aligned dwordx4 loads) and bound the first two versions of aggregate_kernel; instead the
// wave loads the window once, coalesced, writes it to a wave-private LDS buffer and every lane reads
// its 16 features from there.
// Layout: one REGION per disparity chunk g (= lane gl of a pixel): the RL = 16 + P-1 window dwords the P pixels'
// chunk-g lanes read, contiguous, so that a lane's 16 features sit at region base + pg + k -- one address register
// and immediate offsets (the first layout padded every 16 dwords and needed P-1 extra address registers per lane,
// 15 of them at D = 64, which cost that variant an occupancy step and 47 % of its LDS cycles in bank conflicts).
// Regions start RS dwords apart with RS = P/2 (mod 32): the 32 lanes one ds_read_b32 cycle serves are P/2 pixels x
// LPP chunks = LPP runs of P/2 consecutive dwords, which then tile the 32 banks exactly, for every k.
template <int LPP>
struct Win {
    static constexpr int P = 64 / LPP;              // pixels (scan lines) per wave
    static constexpr int D = 16 * LPP;
    static constexpr int RL = 16 + P - 1;           // dwords per region
    static constexpr int RS = LPP == 4 ? 40 : LPP == 8 ? 36 : 34;   // region stride: >= RL, = P/2 mod 32
    static constexpr int NE = LPP * RL;             // staged dwords per step (window dwords shared by two regions are staged twice)
    static constexpr int NLD = (NE + 63) / 64;      // cooperative dword loads per lane and step
    static constexpr int BUF = LPP * RS;            // dwords per LDS buffer
    static_assert(RS >= RL && RS % 32 == (P / 2) % 32, "region stride");
};

// per-lane constants of the staging: where the lane's i-th cooperative load comes from / goes to, and where it reads
template <int LPP>
struct WinLane {
    unsigned goff[Win<LPP>::NLD];   // byte offset from the window's first dword (window dword 0 = disparity D-1 of the wave's first pixel)
    int lslot[Win<LPP>::NLD];       // LDS dword index inside the buffer
    int rbase;                      // LDS dword index of this lane's feature 0
    __device__ __forceinline__ void init(int lane) {
        using WN = Win<LPP>;
#pragma unroll
        for (int i = 0; i < WN::NLD; ++i) {
            const int e = min(64 * i + lane, WN::NE - 1);   // the last round's excess lanes repeat the last element
            const int g = e / WN::RL, o = e - g * WN::RL;
            goff[i] = (unsigned)(WN::D - 16 - 16 * g + o) * 4u;
            lslot[i] = g * WN::RS + o;
        }
        rbase = (lane % LPP) * WN::RS + lane / LPP;
    }
};

template <int LPP>
__device__ __forceinline__ void win_read(const uint32_t *lds_buf, int rbase, uint32_t (&r)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) r[k] = lds_buf[rbase + k];
}

// Block barrier that orders LDS traffic only.  __syncthreads() carries a workgroup fence, i.e. s_waitcnt vmcnt(0): at the
// end of a burst every wave would sit out the acknowledgement of its global stores (~10 us under this read load), 23
// times per sweep (0.3 ms per 16-frame launch).  The bursts only exchange data through LDS.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// f(std::integral_constant<int, LPP>) with LPP = D/16 lanes per pixel as a compile-time constant: the launchers' dispatch on the engine's D (64, 128 or 256)
template <typename F>
inline void with_lpp(int D, F &&f) {
    switch (D) {
        case 64: f(std::integral_constant<int, 4>{}); break;
        case 128: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}

// XCD-aware grid decode of the aggregation launch and the fused sweep: on when the launch's frames divide over the 8 XCDs and
// one frame's two census planes are of the order of an XCD's 4 MB L2.  Measured A/B on one box (profiles/r03_xcd.txt):
// 1242x375 D=128 P=8 aggregate 1.607-1.613 vs 1.619-1.631 ms (+0.7 % pairs/s), D=256 P=4 aggregate 1.21-1.23 vs 1.25-1.26,
// D=64 P=4 level; at 1920x1080 (17 MB of census per frame) it costs the aggregate 7 % (7.83 vs 7.32 ms per 8 frames): off there.
inline bool xcd_placement(const Geometry &g, int n_frames) {
    return n_frames > 0 && (n_frames & 7) == 0 && g.census_elems * 8 <= (size_t)(8u << 20);
}

}  // namespace cart_amd

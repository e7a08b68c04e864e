// sgm_aggregate.hip -- path aggregation of the SGM core (stage overview: sgm_census.hip).
#include <algorithm>

#include "sgm_device.h"

namespace cart_amd {

// ------------------------------------------------------------------ path aggregation
// All directions of all frames in ONE launch (blockIdx.x -> direction + a group of scan lines,
// blockIdx.y -> frame).  Every direction is a set of independent 1-D lines: vertical and
// diagonal lines are indexed by their (skewed) entry column so no state ever crosses pixels.
//
// The kernel is VALU-issue bound (rocprofv3: SQ_ACTIVE_INST_VALU ~ 93 % of SIMD time in the first,
// 32-bit version), so the recurrence runs on PACKED u16 pairs (v_pk_min_u16 / v_pk_add_u16: two
// disparities per instruction).  A pixel is owned by LPP = D/16 adjacent lanes, 16 disparities per
// lane held in 8 registers with a split-halves layout  reg i = (L[d0+i], L[d0+i+8]) :
//   * the d-1 / d+1 neighbour vectors of reg i are simply reg i-1 / reg i+1 (register renaming);
//     only reg 0 / reg 7 need one v_perm_b32 that stitches in the neighbouring lane's value
//     (DPP row_shr/row_shl), and that same v_perm writes 0xFFFF (= never chosen) at the ends of the
//     disparity range through a per-lane selector,
//   * the matching cost is popcount(xor) with the "- min" of the recurrence folded into
//     v_bcnt_u32_b32's accumulate operand, packed by one v_perm_b32 per pair,
//   * the u8 slab bytes are produced by v_perm_b32 byte gathers (8 per 16 cells),
//   * min over D = packed min tree + DPP (quad_perm / row_half_mirror / row_mirror) on the
//     replicated pair, which doubles as the packed (m,m) operand of the next step.

typedef uint32_t u32x4_g4 __attribute__((ext_vector_type(4), aligned(4)));
// 16 consecutive features at a 4-byte aligned address (4 x dwordx4)
__device__ __forceinline__ void ld_u32x16(const uint32_t *ubase, unsigned &byte_off, uint32_t (&r)[16]) {
    const CART_GLOBAL char *b = (const CART_GLOBAL char *)sgpr(ubase) + pin_v(byte_off);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u32x4_g4 v = *(const CART_GLOBAL u32x4_g4 *)(b + 16 * i);
        r[4 * i + 0] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    }
}

// left feature + the lane's 16 right features; pl / pr are wave-uniform, the offsets per lane (bytes)
__device__ __forceinline__ void load_census(const uint32_t *pl, unsigned &off_l, const uint32_t *pr, unsigned &off_r, CensusRegs &c) {
    c.fl = ld_u32(pl, off_l);
    ld_u32x16(pr, off_r, c.r);
}

// 6 waves per SIMD (<= 80 VGPRs) fit without spills for D >= 128; the D = 64 variant carries 15 lane offsets more
// ---- horizontal scans with a sliding right-feature window --------------------------------------------------------
// Along a row the lane's 16 right features move by ONE element per step, so the window lives in 16 registers that are
// renamed instead of reloaded (a 16-step group is unrolled; logical slot k of sub-step j is register (k + j*DX) & 15)
// and a step loads two dwords -- the left feature and the entering right feature -- instead of 17.  Those two come from
// a FIFO filled HS_PF steps ahead: a horizontal wave is alone on its SIMD for most of its 1242 steps, nothing else hides
// the load latency, and with the two-step prefetch of the reloading loop every step waited for memory (0.75 us per step
// against 0.2 us of issue time).  The first group is peeled so that the loop header merges two identical VMEM
// histories (counted s_waitcnt, see the NOTE in aggregate_kernel).
constexpr int HS_PF = 8;
template <int LPP, int DX>
__device__ __forceinline__ void hscan_sliding(uint32_t (&st)[8], uint32_t &mm, const uint32_t *&pl, unsigned &lo_l, const uint32_t *&pr,
                                              unsigned &lo_r, uint8_t *&po, unsigned &lo_o, ptrdiff_t ostride, int groups, uint32_t sel_lo,
                                              uint32_t sel_hi, uint32_t p1p1, uint32_t p2p2) {
    uint32_t win[16], ffl[HS_PF], fnw[HS_PF], xr[16];
    ld_u32x16(pr, lo_r, win);                          // window of step 0
    unsigned lo_n = lo_r + (DX > 0 ? 15u * 4u : 0u);   // the element that enters the window: slot 15 going right, slot 0 going left
#pragma unroll
    for (int q = 0; q < HS_PF; ++q) {                  // FIFO entry q: left feature of step q, entering element of step q + 1
        ffl[q] = ld_u32(pl + q * DX, lo_l);
        fnw[q] = ld_u32(pr + (q + 1) * DX, lo_n);
    }
    auto group = [&]() {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            constexpr int M = 15;
            const int slot = j % HS_PF;
#pragma unroll
            for (int k = 0; k < 16; ++k) xr[k] = ffl[slot] ^ win[(DX > 0 ? k + j : k - j + 16) & M];
            win[(DX > 0 ? j : 15 - j) & M] = fnw[slot];
            __builtin_amdgcn_sched_barrier(0);
            ffl[slot] = ld_u32(pl + (j + HS_PF) * DX, lo_l);          // step j + HS_PF (reads row padding past the end)
            fnw[slot] = ld_u32(pr + (j + HS_PF + 1) * DX, lo_n);
            __builtin_amdgcn_sched_barrier(0);
            agg_step<LPP>(st, mm, xr, sel_lo, sel_hi, p1p1, p2p2, sgpr(po + j * ostride) + pin_v(lo_o));
            __builtin_amdgcn_sched_barrier(0);
        }
        pl += 16 * DX; pr += 16 * DX; po += 16 * ostride;
    };
    group();
    for (int gi = 1; gi < groups; ++gi) group();
}

// ---- horizontal scans split over a wave PAIR (AggArgs::hsplit) ----------------------------------------------------------
// A horizontal scan is a chain of `width` steps on which one wave issues ~102 instructions per step and nothing can be done
// in parallel along the row: alone on its SIMD it already uses every issue slot (1242 steps x ~445 clocks = 0.27 ms whatever
// the launch holds), and launches with few frames -- or D = 64, where the other directions are short -- wait for these chains.
// 40 of the 102 instructions do not depend on the recurrence at all: the matching cost (xor, popcount, pack).  In split mode a
// PRODUCER wave keeps the sliding census window and writes the packed costs of step t+1 into LDS while the CONSUMER wave of
// the pair runs the recurrence of step t on the costs it reads back: ~60 instructions per step on the chain instead of 102.
// The two sit on different SIMDs of the CU (waves of a workgroup are dealt over its four SIMDs); one s_barrier per step keeps
// them one step apart (double-buffered costs).  A 4-wave workgroup holds two pairs, i.e. 2 P rows instead of 4 P.
constexpr int kHsCostDwords = 2 * 2 * 64 * 4;   // per pair: [buffer][half][lane][4 dwords]

// producer of a pair: costs of every step t = 0 .. w-1 into buffer t & 1, one barrier after each, one more at the end (the consumer's last step)
template <int LPP, int DX>
__device__ __forceinline__ void hsplit_producer(const uint32_t *pl, unsigned lo_l, const uint32_t *pr, unsigned lo_r, int w, uint32_t *cost, int lane) {
    auto emit = [&](int parity, const uint32_t (&c)[8]) {
        v4u *dst = reinterpret_cast<v4u *>(cost) + parity * 128 + lane;
        dst[0] = v4u{c[0], c[1], c[2], c[3]};
        dst[64] = v4u{c[4], c[5], c[6], c[7]};
        lds_barrier();
    };
    const int groups = w / 16;
    if (groups > 0) {
        uint32_t win[16], ffl[HS_PF], fnw[HS_PF];
        ld_u32x16(pr, lo_r, win);                          // window of step 0
        unsigned lo_n = lo_r + (DX > 0 ? 15u * 4u : 0u);   // the element that enters the window (see hscan_sliding)
#pragma unroll
        for (int q = 0; q < HS_PF; ++q) {
            ffl[q] = ld_u32(pl + q * DX, lo_l);
            fnw[q] = ld_u32(pr + (q + 1) * DX, lo_n);
        }
        auto group = [&]() {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int slot = j % HS_PF;
                const uint32_t f = ffl[slot];
                uint32_t c[8];   // c[i] = (C[d0+8+i] << 16) + C[d0+i]: logical window slot k of this sub-step is register (k +- j) & 15
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    c[i] = ((uint32_t)__builtin_popcount(f ^ win[(DX > 0 ? 7 - i + j : 7 - i - j + 16) & 15]) << 16) +
                           (uint32_t)__builtin_popcount(f ^ win[(DX > 0 ? 15 - i + j : 15 - i - j + 16) & 15]);
                win[(DX > 0 ? j : 15 - j) & 15] = fnw[slot];
                ffl[slot] = ld_u32(pl + (j + HS_PF) * DX, lo_l);          // step j + HS_PF (reads row padding past the end)
                fnw[slot] = ld_u32(pr + (j + HS_PF + 1) * DX, lo_n);
                emit(j & 1, c);
            }
            pl += 16 * DX; pr += 16 * DX;
        };
        group();
        for (int gi = 1; gi < groups; ++gi) group();
    }
    for (int t = groups * 16; t < w; ++t) {   // the last w % 16 steps: plain loads
        CensusRegs cr;
        load_census(pl, lo_l, pr, lo_r, cr);
        uint32_t c[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            c[i] = ((uint32_t)__builtin_popcount(cr.fl ^ cr.r[7 - i]) << 16) + (uint32_t)__builtin_popcount(cr.fl ^ cr.r[15 - i]);
        emit(t & 1, c);
        pl += DX; pr += DX;
    }
    lds_barrier();
}

// lanes 32..63 of `a` <-> lanes 0..31 of `b` (gfx950's v_permlane32_swap): a = {a.lo, b.lo}, b = {a.hi, b.hi}
// (gfx950 only, like pk_min3: any other --offload-arch stops here instead of failing in the assembler)
__device__ __forceinline__ void swap_halves(uint32_t &a, uint32_t &b) {
#if defined(__gfx950__)
    asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
#elif defined(__HIP_DEVICE_COMPILE__)
#error "sgm_aggregate.hip is written for gfx950 (v_permlane32_swap_b32)"
#endif
}

// consumer of a pair.  D = 64 (LPP = 4): a pixel is 64 bytes, half a 128-byte line, and a step's store would write 16 rows x 64 B; the stores of TWO
// steps are regrouped instead (four lane-half swaps) so that each instruction writes whole lines: rows 0-7 of both steps, then rows 8-15 (lo_a / lo_b:
// this lane's byte offsets in the two stores, from the LOWER-x pixel of the step pair).  Measured with a timing build that wrote whole KB per store:
// aggregate 0.545 -> 0.499 ms at 1242x375 D=64 P=4, and this form reaches it (0.503); D >= 128 pixels are whole lines already and gain nothing
// (profiles/r04_hsplit.txt).
template <int LPP, int DX>
__device__ __forceinline__ void hsplit_consumer(uint32_t (&st)[8], uint32_t &mm, uint8_t *po, unsigned lo_o, unsigned lo_a, unsigned lo_b, int D, int w,
                                                const uint32_t *cost, int lane, uint32_t sel_lo, uint32_t sel_hi, uint32_t p1p1, uint32_t p2p2) {
    const ptrdiff_t ostride = (ptrdiff_t)DX * D;
    auto step = [&](int parity) {
        const v4u *src = reinterpret_cast<const v4u *>(cost) + parity * 128 + lane;
        const v4u c0 = src[0], c1 = src[64];
        const uint32_t c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const v4u q = agg_step_c<LPP>(st, mm, c, sel_lo, sel_hi, p1p1, p2p2);
        lds_barrier();
        return q;
    };
    lds_barrier();   // the costs of step 0 are in buffer 0
    int t = 0;
    for (; t + 1 < w; t += 2) {
        if constexpr (LPP == 4) {
            const v4u s0 = step(0), s1 = step(1);
            uint32_t u0[4] = {s0.x, s0.y, s0.z, s0.w}, u1[4] = {s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) swap_halves(u0[i], u1[i]);
            const v4u q0 = {u0[0], u0[1], u0[2], u0[3]}, q1 = {u1[0], u1[1], u1[2], u1[3]};
            uint8_t *pp = DX > 0 ? po : po + ostride;   // the pair's lower-x pixel
            __builtin_nontemporal_store(q0, (CART_GLOBAL v4u *)(sgpr(pp) + pin_v(lo_a)));
            __builtin_nontemporal_store(q1, (CART_GLOBAL v4u *)(sgpr(pp) + pin_v(lo_b)));
        } else {
            const v4u q0 = step(0);
            __builtin_nontemporal_store(q0, (CART_GLOBAL v4u *)(sgpr(po) + pin_v(lo_o)));
            const v4u q1 = step(1);
            __builtin_nontemporal_store(q1, (CART_GLOBAL v4u *)(sgpr(po + ostride) + pin_v(lo_o)));
        }
        po += 2 * ostride;
    }
    if (t < w) {
        const v4u q = step(0);
        __builtin_nontemporal_store(q, (CART_GLOBAL v4u *)(sgpr(po) + pin_v(lo_o)));
    }
}

// prefetch depth of the vertical / diagonal scans in steps (see the note at the loop): 4 at D = 64 (-10 %), 2 elsewhere (flat)
template <int LPP> constexpr int v_depth() { return LPP == 4 ? 4 : 2; }

constexpr int kAggWaves = 4;   // waves per workgroup: nothing in the kernel is shared between waves (1-2: 1.85 instead of 1.58 ms at the headline; 8: slower but at D=64)
// HS: the launch runs its horizontal scans as producer / consumer wave pairs (hsplit_*); a separate instantiation, so that the plain launch keeps its
// 70 VGPRs (7 waves per SIMD) and the split one gets the registers its producer needs without spilling
// CKPT: the launch of plan BAND_UP (AggArgs::ckpt_rows = K): the "up" scan runs on every row but stores only the rows y % K == 0, y > 0, in place in
// its slab -- the state wta_band_kernel restarts from.  A separate instantiation: the scan loop exists twice in it (the store of the "up" waves
// sits behind a wave-uniform branch, every other direction keeps its unconditional stores and exact counted vmcnt waits), the other plans' kernels
// are what they were.
template <int LPP, bool HS = false, bool CKPT = false>
__global__ __launch_bounds__(64 * kAggWaves, (LPP >= 8 && !HS) ? 6 : 4) void aggregate_kernel(AggArgs a) {
    using WN = Win<LPP>;
    constexpr int P = WN::P;
    constexpr int LINES_PER_BLOCK = kAggWaves * P;
    __shared__ uint32_t s_win[kAggWaves][2][WN::BUF];
    __shared__ __attribute__((aligned(16))) uint32_t s_cost[HS ? kAggWaves / 2 : 1][HS ? kHsCostDwords : 4];   // split horizontal scans: the pairs' cost buffers
    const Geometry &g = a.g;
    // 1-D grid, direction-major: [dir][frame][line group].  The horizontal directions come first so that
    // their W-step serial scans of EVERY frame start at once; the H-step scans fill in behind them.
    // XCD placement (speed only, never correctness): workgroups are dealt round-robin over the 8 XCDs, each with an L2 of its
    // own, and every direction re-reads its frame's census planes (4.2 MB per frame).  With n_frames a multiple of 8 the
    // grid is decoded per XCD (xcd_placement() in sgm_device.h): XCD x works on frames x, x + 8, ... in the same direction-major order,
    // so that a frame's planes are fetched into ONE L2 instead of all eight.
    keep_f16_denormals();
    int bid = (int)blockIdx.x, nfr = a.n_frames, frame0 = 0, fstep = 1;
    if (a.xcd_frames) { frame0 = bid & 7; bid >>= 3; nfr = a.n_frames >> 3; fstep = 8; }
    int di = 0;
    for (int i = 1; i < a.ndirs; ++i)
        if (bid >= a.dirs[i].blk0 * nfr) di = i;
    const int dx = a.dirs[di].dx, dy = a.dirs[di].dy;
    const bool hsplit = HS && dy == 0;   // this workgroup runs two producer / consumer pairs on 2 P rows (launch_aggregate counted its blocks that way)
    const int lpb = hsplit ? 2 * P : LINES_PER_BLOCK;
    const int nblk = (a.dirs[di].nlines + lpb - 1) / lpb;
    const int rb = bid - a.dirs[di].blk0 * nfr;
    const int frame = frame0 + fstep * (rb / nblk);
    const int bl = rb - (rb / nblk) * nblk;   // block inside the frame's share of this direction
    const int lane = threadIdx.x & 63, wid = uniform((int)(threadIdx.x >> 6));
    const int gl = lane % LPP, pg = lane / LPP;  // lane inside the pixel's lane group, pixel group inside the wave
    const int line0 = bl * lpb + (hsplit ? wid >> 1 : wid) * P;  // wave-uniform
    const int line = line0 + pg;
    const int nlines = a.dirs[di].nlines;
    if (line0 >= nlines && !hsplit) return;  // whole wave idle (a split-scan workgroup keeps all four waves: they meet at a barrier every step)
    const int d0 = gl * 16;
    const uint32_t p1p1 = (uint32_t)g.p1 * 0x10001u, p2p2 = (uint32_t)g.p2 * 0x10001u;
    // selectors of the two stitching v_perm: 0x0d bytes inject 0xFFFF where d-1 / d+1 leave [0, D)
    const uint32_t sel_lo = gl == 0 ? 0x05040d0du : 0x05040302u;
    const uint32_t sel_hi = gl == LPP - 1 ? 0x0d0d0302u : 0x05040302u;

    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = 0;
    uint32_t mm = 0;
    CensusRegs ca, cb;

    // NOTE on the loop shapes below.  vmcnt retires in issue order and counts stores too, so a load issued
    // AFTER a slab store cannot be consumed before that store has been written back (>1 us under write
    // pressure).  Each step therefore issues the loads of step t+2 BEFORE its own store, consumes the loads
    // of step t+1 after it, and keeps every VMEM instruction of the main loops unconditional (prefetches past
    // the last step read valid padding / slack) so that the compiler can use exact counted vmcnt waits.
    if (dy == 0) {
        // ---- horizontal scans: the wave's pixels sit on P different rows, nothing to share; per-lane loads.
        // These waves carry the longest dependency chain of the launch: let them win VALU arbitration.
        __builtin_amdgcn_s_setprio(3);
        if constexpr (HS) {
            // rows past the image (the last wave pair of a direction) clone the pair's last valid row: same reads, same bytes to the same cells,
            // and every wave that entered reaches every barrier.  Two waves then store to the same slab cells without ordering: benign only because
            // both compute the same state from the same census rows -- held by tests/test_gpu_parity.py::test_split_horizontal_scans_equal_plain_ones,
            // whose heights leave the last workgroup a partial pair and an idle pair (every slab row, the cloned ones included, against the oracle)
            const int l0 = min(line0, nlines - 1), pgv = min(pg, nlines - l0 - 1);   // (a pair wholly past the image clones the last row)
            const int y0s = a.dirs[di].jmin + l0, xs = dx > 0 ? 0 : g.w - 1;
            const uint32_t *pls = a.cen_l + uniform((ptrdiff_t)frame * (ptrdiff_t)g.census_elems + (ptrdiff_t)y0s * g.cpitch + g.cpadl + xs);
            const uint32_t *prs = a.cen_r + uniform((ptrdiff_t)frame * (ptrdiff_t)g.census_elems + (ptrdiff_t)y0s * g.cpitch + g.cpadl + xs - g.min_disp - (WN::D - 1));
            uint8_t *pos = a.slabs.frame[frame] + uniform((ptrdiff_t)a.dirs[di].path * (ptrdiff_t)g.slab_bytes + ((ptrdiff_t)y0s * g.w + xs) * g.D);
            const unsigned so_l = (unsigned)pgv * g.cpitch * 4u, so_r = so_l + (unsigned)(WN::D - 16 - d0) * 4u;
            const unsigned so_o = (unsigned)pgv * g.w * g.D + d0;
            // paired-step stores of the D = 64 consumer (hsplit_consumer): lanes 0-31 store the pair's first step, lanes 32-63 its second, of rows
            // pg & 7 (first store) and 8 + (pg & 7) (second); offsets count from the pair's lower-x pixel
            const int rlim = nlines - l0 - 1, r8 = (lane & 31) / LPP;
            const unsigned xo = ((dx > 0) == (lane >= 32)) ? (unsigned)g.D : 0u;
            const unsigned so_a = (unsigned)min(r8, rlim) * g.w * g.D + d0 + xo, so_b = (unsigned)min(r8 + 8, rlim) * g.w * g.D + d0 + xo;
            uint32_t *cost = &s_cost[wid >> 1][0];
            // D = 64: the producer has ~30 % slack per step; below the consumers' priority it stops taking issue slots from the consumer of ANOTHER pair
            // on its SIMD (aggregate 0.505 -> 0.498 ms at 16 frames, 0.305 -> 0.296 at 8).  At D = 256 the same costs 7 % (0.491 -> 0.524, 6 frames): left at 3.
            if constexpr (LPP == 4) { if ((wid & 1) == 0) __builtin_amdgcn_s_setprio(1); }
            if ((wid & 1) == 0) {
                if (dx > 0) hsplit_producer<LPP, 1>(pls, so_l, prs, so_r, g.w, cost, lane);
                else hsplit_producer<LPP, -1>(pls, so_l, prs, so_r, g.w, cost, lane);
            } else {
                if (dx > 0) hsplit_consumer<LPP, 1>(st, mm, pos, so_o, so_a, so_b, g.D, g.w, cost, lane, sel_lo, sel_hi, p1p1, p2p2);
                else hsplit_consumer<LPP, -1>(st, mm, pos, so_o, so_a, so_b, g.D, g.w, cost, lane, sel_lo, sel_hi, p1p1, p2p2);
            }
            return;
        }
        if (line >= nlines) return;
        const int y0r = a.dirs[di].jmin + line0;          // row of the wave's first line (uniform)
        const int x = dx > 0 ? 0 : g.w - 1, t1 = g.w;
        // uniform bases + non-negative per-lane element offsets
        const uint32_t *pl_u = a.cen_l + uniform((ptrdiff_t)frame * (ptrdiff_t)g.census_elems + (ptrdiff_t)y0r * g.cpitch + g.cpadl + x);
        const uint32_t *pr_u = a.cen_r + uniform((ptrdiff_t)frame * (ptrdiff_t)g.census_elems + (ptrdiff_t)y0r * g.cpitch + g.cpadl + x - g.min_disp - (WN::D - 1));
        uint8_t *po_u = a.slabs.frame[frame] + uniform((ptrdiff_t)a.dirs[di].path * (ptrdiff_t)g.slab_bytes + ((ptrdiff_t)y0r * g.w + x) * g.D);
        unsigned lo_l = (unsigned)pg * g.cpitch * 4u, lo_r = lo_l + (unsigned)(WN::D - 16 - d0) * 4u;  // bytes
        unsigned lo_o = (unsigned)pg * g.w * g.D + d0;
        const ptrdiff_t cstride = dx, ostride = (ptrdiff_t)dx * g.D;
        const uint32_t *pl = pl_u, *pr = pr_u;
        uint8_t *po = po_u;
        // full 16-step groups with the sliding window; the last w % 16 steps (and images narrower than a group) through
        // the reloading loop below, which can start anywhere
        const int groups = t1 / 16;
        if (groups > 0) {
            if (dx > 0) hscan_sliding<LPP, 1>(st, mm, pl, lo_l, pr, lo_r, po, lo_o, ostride, groups, sel_lo, sel_hi, p1p1, p2p2);
            else hscan_sliding<LPP, -1>(st, mm, pl, lo_l, pr, lo_r, po, lo_o, ostride, groups, sel_lo, sel_hi, p1p1, p2p2);
        }
        uint32_t xr[16];
        load_census(pl, lo_l, pr, lo_r, ca);
        load_census(pl + cstride, lo_l, pr + cstride, lo_r, cb);
        int t = groups * 16;
        for (; t + 1 < t1; t += 2) {
            agg_xor(ca, xr);
            __builtin_amdgcn_sched_barrier(0);
            load_census(pl + 2 * cstride, lo_l, pr + 2 * cstride, lo_r, ca);  // step t+2 (reads row padding past the end)
            __builtin_amdgcn_sched_barrier(0);
            agg_step<LPP>(st, mm, xr, sel_lo, sel_hi, p1p1, p2p2, sgpr(po) + pin_v(lo_o));
            __builtin_amdgcn_sched_barrier(0);
            agg_xor(cb, xr);
            __builtin_amdgcn_sched_barrier(0);
            load_census(pl + 3 * cstride, lo_l, pr + 3 * cstride, lo_r, cb);  // step t+3
            __builtin_amdgcn_sched_barrier(0);
            agg_step<LPP>(st, mm, xr, sel_lo, sel_hi, p1p1, p2p2, sgpr(po + ostride) + pin_v(lo_o));
            __builtin_amdgcn_sched_barrier(0);
            pl += 2 * cstride; pr += 2 * cstride; po += 2 * ostride;
        }
        if (t < t1) {
            agg_xor(ca, xr);
            agg_step<LPP>(st, mm, xr, sel_lo, sel_hi, p1p1, p2p2, sgpr(po) + pin_v(lo_o));
        }
        return;
    }

    // ---- vertical / diagonal scans: lines are indexed by their (skewed) entry column j
    // A wave that holds fewer than P lines (the last one of a direction: 1242 columns = 77 x 16 + 10 at D = 64,
    // 155 x 8 + 2 at D = 128) lets its surplus lane groups CLONE its last valid line: same reads, same arithmetic, the
    // same bytes stored to the same cells.  (Sending such waves through the synchronous ragged path instead made one wave
    // per frame and direction walk all its steps at memory latency -- 0.26 ms on an idle GPU, ~0.6 ms under load, which
    // was the whole launch time at D = 64 / 4 paths.)
    const int nv = min(P, nlines - line0);  // valid lines in this wave (wave-uniform)
    const int pgv = min(pg, nv - 1);        // the line of the wave this lane group works on
    const int j = a.dirs[di].jmin + line0 + pgv;
    const int ys = dy > 0 ? 0 : g.h - 1;
    int t0, t1;  // this lane group's active steps
    if (dx > 0) { t0 = max(0, -j); t1 = min(g.h, g.w - j); }
    else if (dx < 0) { t0 = max(0, j - g.w + 1); t1 = min(g.h, j + 1); }
    else { t0 = 0; t1 = g.h; }
    // wave-uniform ranges: [tb, te) = union of the wave's (adjacent) lines, [tm0, tm1) = steps on which
    // every lane group of the wave is active
    const int jf = a.dirs[di].jmin + line0, jl = jf + nv - 1;
    int tb, te, tm0, tm1;
    if (dx > 0) { tb = max(0, -jl); te = min(g.h, g.w - jf); tm0 = max(0, -jf); tm1 = min(g.h, g.w - jl); }
    else if (dx < 0) { tb = max(0, jf - g.w + 1); te = min(g.h, jl + 1); tm0 = max(0, jl - g.w + 1); tm1 = min(g.h, jf + 1); }
    else { tb = 0; te = g.h; tm0 = 0; tm1 = g.h; }
    if (tb >= te) return;
    if (tm0 >= tm1) { tm0 = te; tm1 = te; }  // no step with every line active: everything through the ragged path

    // cooperative window load + this lane's 16 features (window dwords pg + D-16 - 16*gl + k), see Win / WinLane
    WinLane<LPP> wlane;
    wlane.init(lane);
    unsigned (&goff)[WN::NLD] = wlane.goff;
    const int (&lslot)[WN::NLD] = wlane.lslot;
    const int rbase = gl * WN::RS + pgv;
    uint32_t *buf0 = &s_win[wid][0][0], *buf1 = &s_win[wid][1][0];

    // pointers as a function of the step t
    const ptrdiff_t cstride = (ptrdiff_t)dy * g.cpitch + dx;
    const ptrdiff_t ostride = ((ptrdiff_t)dy * g.w + dx) * g.D;
    // uniform bases (line jf = first line of the wave) + per-lane offsets (pg = this lane's line inside the wave)
    const ptrdiff_t cen_off = (ptrdiff_t)frame * (ptrdiff_t)g.census_elems + (ptrdiff_t)ys * g.cpitch + g.cpadl + jf;
    const uint32_t *pw_base = a.cen_r + uniform(cen_off - g.min_disp - (WN::D - 1));  // window start at t = 0
    const uint32_t *pl_u = a.cen_l + uniform(cen_off);
    uint8_t *po_u = a.slabs.frame[frame] + uniform((ptrdiff_t)a.dirs[di].path * (ptrdiff_t)g.slab_bytes + ((ptrdiff_t)ys * g.w + jf) * g.D);
    unsigned lo_l = (unsigned)pgv * 4u, lo_o = (unsigned)(pgv * WN::D + d0);  // bytes

    // ragged start / end of diagonal lines (and waves with invalid lines): simple, fully synchronous steps
    auto ragged = [&](int ta, int tz) {
        for (int t = ta; t < tz; ++t) {
            const uint32_t *pw = pw_base + t * cstride;
#pragma unroll
            for (int i = 0; i < WN::NLD; ++i) buf0[lslot[i]] = ld_u32(pw, goff[i]);
            if (t >= t0 && t < t1) {
                uint32_t xr[16];
                ca.fl = ld_u32(pl_u + t * cstride, lo_l);
                win_read<LPP>(buf0, rbase, ca.r);
                agg_xor(ca, xr);
                agg_step<LPP>(st, mm, xr, sel_lo, sel_hi, p1p1, p2p2, sgpr(po_u + t * ostride) + pin_v(lo_o));
            }
        }
    };
    ragged(tb, tm0);
    // ck: this wave's scan stores checkpoint rows only (vertical scans have no ragged steps: every store of the "up" scan is in here)
    auto scan = [&](auto ck) {
        constexpr bool CK = decltype(ck)::value;
        const uint32_t *pw = pw_base + tm0 * cstride, *pl = pl_u + tm0 * cstride;
        uint8_t *po = po_u + tm0 * ostride;
        // K register sets of prefetched windows: the loads of step t+K are issued at the start of step t.  vmcnt retires in
        // issue order and counts stores, so the loads consumed at step t wait for the slab stores issued up to step t-K:
        // with K = 2 every step of a wave sat out the acknowledgement of a two-step-old store (~2 us under write pressure,
        // i.e. ~1 us per step however few waves shared the SIMD) -- invisible at D = 128 / 8 paths, where enough waves per
        // SIMD cover it, but 0.4 ms per launch at D = 64 / 4 paths, whose vertical waves finish last on their own.
        constexpr int K = v_depth<LPP>();
        static_assert(K % 2 == 0 && K >= 2, "the LDS window buffers alternate");
        uint32_t gs[K][WN::NLD], fs[K];
#pragma unroll
        for (int i = 0; i < WN::NLD; ++i) buf0[lslot[i]] = ld_u32(pw, goff[i]);   // step tm0 straight into its LDS buffer
        fs[0] = ld_u32(pl, lo_l);
#pragma unroll
        for (int j = 1; j < K; ++j) {
#pragma unroll
            for (int i = 0; i < WN::NLD; ++i) gs[j][i] = ld_u32(pw + j * cstride, goff[i]);
            fs[j] = ld_u32(pl + j * cstride, lo_l);
        }
        uint32_t xr[16];
        int t = tm0;
        // sub-step J of a K-step trip: buffer J&1 holds the window of step t+J, fs[J] its left feature, set J is free
        auto sub = [&](auto jc, auto reload) {
            constexpr int J = decltype(jc)::value;
            uint32_t *cur = (J & 1) ? buf1 : buf0, *nxt = (J & 1) ? buf0 : buf1;
            ca.fl = fs[J];
            if constexpr (decltype(reload)::value) {
#pragma unroll
                for (int i = 0; i < WN::NLD; ++i) gs[J][i] = ld_u32(pw + (J + K) * cstride, goff[i]);  // step t+J+K, issued before this step's store
                fs[J] = ld_u32(pl + (J + K) * cstride, lo_l);
            }
            __builtin_amdgcn_sched_barrier(0);
            win_read<LPP>(cur, rbase, ca.r);
            agg_xor(ca, xr);
            bool store_row = true;
            if constexpr (CK) { const int yy = ys + (t + J) * dy; store_row = yy > 0 && (yy & (a.ckpt_rows - 1)) == 0; }   // wave-uniform
            agg_step<LPP>(st, mm, xr, sel_lo, sel_hi, p1p1, p2p2, sgpr(po + J * ostride) + pin_v(lo_o), store_row);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < WN::NLD; ++i) nxt[lslot[i]] = gs[(J + 1) % K][i];   // window of step t+J+1
        };
        for (; t + K <= tm1; t += K) {
            sub(std::integral_constant<int, 0>{}, std::true_type{});
            sub(std::integral_constant<int, 1>{}, std::true_type{});
            if constexpr (K > 2) {
                sub(std::integral_constant<int, 2>{}, std::true_type{});
                sub(std::integral_constant<int, 3>{}, std::true_type{});
            }
            if constexpr (K > 4) {
                sub(std::integral_constant<int, 4>{}, std::true_type{});
                sub(std::integral_constant<int, 5>{}, std::true_type{});
            }
            pw += K * cstride; pl += K * cstride; po += K * ostride;
        }
        // the last tm1 - t < K steps: their windows are already in flight
        if (t < tm1) sub(std::integral_constant<int, 0>{}, std::false_type{});
        if (t + 1 < tm1) sub(std::integral_constant<int, 1>{}, std::false_type{});
        if constexpr (K > 2) {
            if (t + 2 < tm1) sub(std::integral_constant<int, 2>{}, std::false_type{});
        }
        if constexpr (K > 4) {
            if (t + 3 < tm1) sub(std::integral_constant<int, 3>{}, std::false_type{});
            if (t + 4 < tm1) sub(std::integral_constant<int, 4>{}, std::false_type{});
        }
    };
    if (tm0 < tm1) {
        if constexpr (CKPT) {
            if (a.dirs[di].path == kUpPath) scan(std::true_type{});
            else scan(std::false_type{});
        } else {
            scan(std::false_type{});
        }
    }
    ragged(tm1, te);
}

int agg_lines_per_block(int D) { return 64 * kAggWaves / (D / 16); }

// 4-wave workgroups of the aggregation launch allowed per CU at a time (0 = no cap: 7 fit).  One row per measured case
// (ms per launch, residency 7 / 5 / 4 / 3 / 2; round 2, one box per row -- DESIGN.md 4.1):
//   ndirs <= 4 (half the work is W-step horizontal scans)
//     D = 64   0.52-0.63 / 0.52-0.57 / - / 0.49-0.51 / 0.52; with the second stream on: 2 per CU 1.04-1.10 ms per step, 3 per CU 1.13-1.18  -> 2
//     D = 128  1.00-1.07 / - / 0.86 / 0.82 / -; with the second stream: 3 per CU 1.68-1.75, 2 per CU 1.72-1.77                                  -> 3
//     D = 256  1.215 / - / 1.19 / - / 1.23 (3 directions + fused sweep)                                                                          -> 4
//   ndirs 7-8
//     D = 256  3.51 / - / 3.29 / - / 3.56 (1080p, 4 frames)                                                                                      -> 4
//     D <= 128, fewer than 16 frames (the frame loop's coalesced groups): 4.73-4.88 k pairs/s against 4.54-4.61 k                              -> 4
//     D <= 128, 16 frames (the headline): 1.574 / 1.547 / 1.540 / 1.60 / 1.69 alone, but beside the second stream's plane kernels the cap
//       costs 1 % (1.61-1.68 against 1.59-1.63)                                                                                                  -> none
//   split horizontal scans (round 4, pairs/s at 2 / 3 / 4 per CU): D = 256 P = 4, 6 frames 5 128 / 5 382 / 5 072, 8 frames 5 134 / 5 360 / 5 332, 12 frames
//     5 428 / 5 542 / 5 565 -> 3;  D = 64 P = 4, 16 frames 15 407 / 14 984 / 14 227, 8 frames 12 853 / 12 337 / 11 789 -> 2 (as without the split)
int agg_residency_cap(int ndirs, int D, int n_frames, bool hsplit) {
    if (ndirs <= 4) return D <= 64 ? 2 : D <= 128 ? 3 : hsplit ? 3 : 4;
    return (D >= 256 || n_frames < 16) ? 4 : 0;
}

// When the horizontal scans run as producer / consumer wave pairs (hsplit_*).  They pay where the launch waits for its W-step chains --
// few directions beside them, or few frames -- and cost 1-2 % where the launch has enough other work (profiles/r04_hsplit.txt; aggregate ms per
// launch, plain / split, means of three alternating runs, 1242x375 unless noted):
//   D = 64  P = 4:  16 frames 0.598 / 0.548   8 frames 0.482 / 0.339   4 frames 0.292 / 0.248   (with the consumer's whole-line stores: 0.503 / 0.305 / 0.244)
//   D = 256 P = 4:  16 frames 1.210 / 1.230   12 frames 0.984 / 0.962   8 frames 0.796 / 0.651   6 frames 0.701 / 0.553   1920x1080, 4 frames 1.493 / 1.448
//   D = 64  P = 8:  16 frames 0.957 / 0.861   8 frames 0.686 / 0.504   (pairs/s 9 253 -> 9 870, 7 353 -> 8 856)
//   D = 128 P = 8:  16 frames 1.453 / 1.456   12 frames 1.147 / 1.166   8 frames 0.782 / 0.785   4 frames 0.473 / 0.451      D = 128 P = 4, 16 frames 0.844 / 0.862
bool agg_hsplit(const Geometry &g, int ndirs, int n_frames) {
    if (g.D == 64) return true;   // whatever else the launch holds: a D = 64 pixel is half a line, and only the split consumer stores whole lines
    return ndirs <= 4 ? n_frames <= 12 : n_frames < 8;
}

void launch_aggregate(const AggArgs &a_in, int n_frames, hipStream_t s) {
    AggArgs a = a_in;
    a.n_frames = n_frames;
    a.xcd_frames = xcd_placement(a.g, n_frames) ? 1 : 0;
    a.hsplit = agg_hsplit(a.g, a.ndirs, n_frames) ? 1 : 0;
    {   // blocks per direction: 4 P lines each, 2 P for the horizontal directions in split mode
        const int lpb_full = agg_lines_per_block(a.g.D);
        int blk = 0;
        for (int i = 0; i < a.ndirs; ++i) {
            const int l = a.hsplit && a.dirs[i].dy == 0 ? lpb_full / 2 : lpb_full;
            a.dirs[i].blk0 = blk;
            blk += (a.dirs[i].nlines + l - 1) / l;
        }
        a.blocks_per_frame = blk;
    }
    dim3 grid(a.blocks_per_frame * n_frames), block(64 * kAggWaves);
    // A cap on the workgroups resident per CU (agg_residency_cap above), enforced with unused dynamic LDS: the others are
    // dispatched as slots free up.  With everything resident at once (7 waves per SIMD fit) the CUs that hold the W-step
    // horizontal scans end up with as many of the short vertical / diagonal scans as the others and finish last; with 2-4
    // workgroups per CU the dispatcher hands the short scans to whichever CU is free, the long scans keep most of their SIMD,
    // and the census planes the directions re-read stay in L2.  Smaller workgroups are slower (two waves or one: the headline's
    // launch 1.85 instead of 1.58 ms), eight-wave ones too except at D=64.
    constexpr int kLdsPerCu = 160 * 1024, kLdsGranule = 1280;
    const int resident = agg_residency_cap(a.ndirs, a.g.D, n_frames, a.hsplit != 0) * 4 / kAggWaves;   // the rule counts 4-wave workgroups
    const int lpp = a.g.D / 16;
    const size_t static_lds = sizeof(uint32_t) * (kAggWaves * 2 * (lpp == 4 ? Win<4>::BUF : lpp == 8 ? Win<8>::BUF : Win<16>::BUF) + (a.hsplit ? (kAggWaves / 2) * kHsCostDwords : 4));
    // (never more than 64 KB per workgroup in all, the limit that needs no opt-in: two of those per CU are still two)
    const size_t pad = resident ? std::min<size_t>(kLdsPerCu / resident - kLdsGranule, 64 * 1024) - static_lds : 0;
    if (a.ckpt_rows) {   // plan BAND_UP (D = 128 only: cart_engine.hip, band_plan_ok)
        if (a.hsplit) hipLaunchKernelGGL((aggregate_kernel<8, true, true>), grid, block, pad, s, a);
        else hipLaunchKernelGGL((aggregate_kernel<8, false, true>), grid, block, pad, s, a);
        return;
    }
    with_lpp(a.g.D, [&](auto lpp_c) {
        constexpr int LPP = decltype(lpp_c)::value;
        if (a.hsplit) hipLaunchKernelGGL((aggregate_kernel<LPP, true>), grid, block, pad, s, a);
        else hipLaunchKernelGGL((aggregate_kernel<LPP>), grid, block, pad, s, a);
    });
}

}  // namespace cart_amd

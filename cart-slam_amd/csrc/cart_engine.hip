// cart_engine.hip -- C-ABI implementation (include/cart_engine.h): the engine itself -- creation, options, the slot and slab
// pools, the placement tuner, stage timing, the disparity entry points and the debug reads.  The later stages and the device
// objects live in engine_*.hip.  No exceptions cross the ABI and nothing exits.
#include <chrono>
#include <cstdio>

#include "engine_host.h"

using namespace cart_amd;

namespace cart_amd {

thread_local std::string g_last_error;
thread_local int g_last_slot = 0;

int fail(const std::string &msg) {
    g_last_error = msg;
    return -1;
}

int SlotLease::begin(cart_engine *e, int n, hipStream_t stream) {
    if (n <= 0 || n > (int)e->slots.size()) return fail("n_frames must be in [1, max_inflight]");
    std::unique_lock<std::mutex> lk(e->mu);
    int s0 = -1;
    for (;;) {
        // Preference: a free range last used on THIS stream (or never): no event wait at all; otherwise the free range that
        // was released longest ago -- a first fit would hand a pipelined caller the slots of its previous batch, whose tail
        // may still be queued on another stream, and serialise the two streams.
        const int total = (int)e->slots.size();
        int oldest = -1;
        unsigned long long oldest_seq = ~0ull;
        for (int i = 0; i + n <= total && s0 < 0; ++i) {
            bool ok = true, same = true;
            unsigned long long seq = 0;
            for (int k = 0; k < n; ++k) {
                const Slot &sl = e->slots[i + k];
                if (sl.busy) { ok = false; i += k; break; }
                same &= !sl.used || sl.last_stream == stream;
                seq = std::max(seq, sl.released_seq);
            }
            if (!ok) continue;
            if (same) s0 = i;
            else if (seq < oldest_seq) { oldest_seq = seq; oldest = i; }
        }
        if (s0 < 0) s0 = oldest;
        if (s0 >= 0) break;
        e->cv.wait(lk);
    }
    for (int k = 0; k < n; ++k) e->slots[s0 + k].busy = true;
    lk.unlock();
    // Cross-stream reuse of a slot waits for the event of the lease that used it last.  That event may have been
    // re-recorded by a later lease of its owner slot: waiting for more than necessary is harmless (an event wait only
    // ever refers to work enqueued before the wait).
    int waited = -1;
    for (int k = 0; k < n; ++k) {
        Slot &s = e->slots[s0 + k];
        if (s.used && s.last_stream != stream && s.owner != waited) {
            hipError_t err = hipStreamWaitEvent(stream, e->slots[s.owner].done, 0);
            if (err != hipSuccess) {   // hand the slots back: later callers must not wait for a lease that never existed
                {
                    std::lock_guard<std::mutex> relk(e->mu);
                    for (int j = 0; j < n; ++j) e->slots[s0 + j].busy = false;
                }
                e->cv.notify_all();
                return fail(std::string("hipStreamWaitEvent: ") + hipGetErrorString(err));
            }
            waited = s.owner;
        }
    }
    this->e = e; this->s0 = s0; this->n = n; this->stream = stream;
    return 0;
}

SlotLease::~SlotLease() {
    if (!e) return;
    (void)hipEventRecord(e->slots[s0].done, stream);  // ONE in-queue marker per lease (16 of them cost ~80 us of GPU idle)
    for (int k = 0; k < n; ++k) {
        Slot &s = e->slots[s0 + k];
        s.owner = s0;
        s.last_stream = stream;
        s.used = true;
    }
    {
        std::lock_guard<std::mutex> lk(e->mu);
        const unsigned long long seq = ++e->release_counter;
        for (int k = 0; k < n; ++k) { e->slots[s0 + k].busy = false; e->slots[s0 + k].released_seq = seq; }
    }
    e->cv.notify_all();
}

int ensure_ws_locked(cart_engine *e, void **ws, size_t bytes_per_slot, bool zero) {
    if (*ws) return 0;
    const size_t bytes = e->slots.size() * bytes_per_slot;
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    if (zero && (hipMemset(p, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) { (void)hipFree(p); return fail("hipMemset of a zeroed workspace failed"); }
    e->bufs.push_back(p);
    *ws = p;
    return 0;
}

}  // namespace cart_amd

static_assert(kMaxLaunchFrames == 64, "cart_engine_set_option(CART_OPT_CHUNK_FRAMES) documents 1..64");

namespace {

void build_agg_args(cart_engine *e, AggArgs &a, unsigned keep) {
    const Geometry &g = e->g;
    a.g = g;
    // launch order: the long serial scans (horizontal, W steps) get the lowest block ids so they
    // start first; slab index `path` keeps the oracle's order {down, up, right, left, diagonals}.
    struct D { int dx, dy, path; };
    static const D order8[8] = {{1, 0, 2}, {-1, 0, 3}, {0, 1, 0}, {0, -1, 1}, {1, 1, 4}, {-1, 1, 5}, {-1, -1, 6}, {1, -1, 7}};
    const unsigned mask = keep;
    int blk = 0, nd = 0;
    const int lpb = agg_lines_per_block(g.D);
    for (int i = 0; i < g.P; ++i) {
        if (!((mask >> i) & 1u)) continue;
        DirDesc &d = a.dirs[nd++];
        d.dx = order8[i].dx; d.dy = order8[i].dy; d.path = order8[i].path;
        if (d.dy == 0) { d.nlines = g.h; d.jmin = 0; }
        else if (d.dx == 0) { d.nlines = g.w; d.jmin = 0; }
        else { d.nlines = g.w + g.h - 1; d.jmin = d.dx > 0 ? -(g.h - 1) : 0; }
        d.blk0 = blk;
        blk += (d.nlines + lpb - 1) / lpb;
    }
    a.ndirs = nd;
    a.blocks_per_frame = blk;
    a.cen_l = e->cen_l; a.cen_r = e->cen_r; a.slabs = SlabTable{};   // filled per launch
}

// The options a call works with: read once under the engine's mutex, so that a concurrent cart_engine_set_option
// cannot change the plan between the workspace allocation and the launches of one call.
struct Options {
    int plan, plan_min_frames, chunk_frames;
    bool timing;
    int spec;
    int band_rows;
    bool band_probe;
    bool band_diag;
};
Options snapshot_options(const cart_engine *e) {   // caller holds e->mu
    return Options{e->opt_plan, e->opt_plan_min_frames, e->chunk_frames, e->timing, e->opt_spec, e->opt_band_rows, e->opt_band_probe != 0, e->opt_band_diag != 0};
}

// The launch plan of `n` frames handed to one launch sequence (include/cart_engine.h, CART_PLAN_*).
int plan_for(const cart_engine *e, const Options &o, int n) {
    if (o.spec & 4) return CART_PLAN_SLABS;   // the S5 variant exists in the two-kernel WTA only
    const bool band_ok = wta_band_supported(e->g, o.band_rows, o.band_probe);
    if (o.plan == CART_PLAN_AUTO) {
        if (band_ok && !o.band_probe && n >= e->auto_band_min_frames) return CART_PLAN_BAND_UP;
        return n >= e->auto_fused_min_frames ? CART_PLAN_FUSED_UP : CART_PLAN_SLABS;
    }
    if (n < o.plan_min_frames) return CART_PLAN_SLABS;
    if (o.plan == CART_PLAN_BAND_UP && !band_ok) return CART_PLAN_SLABS;   // the banded WTA exists for D = 128 with 8 paths
    return o.plan;
}

int validate(const cart_engine_params *p) {
    if (!p) return fail("params is NULL");
    if (p->width < 16 || p->height < 8 || p->width > 16384 || p->height > 16384) return fail("unsupported image size");
    const bool post_only = p->num_disparities == 0 && p->paths == 0;
    if (!post_only && !(p->num_disparities == 64 || p->num_disparities == 128 || p->num_disparities == 256))
        return fail("num_disparities must be 64, 128 or 256");
    if (!post_only && !(p->paths == 4 || p->paths == 8)) return fail("paths must be 4 or 8");
    if (p->min_disparity < 0 || p->min_disparity > 64) return fail("min_disparity must be in [0, 64]");
    if (p->p1 < 0 || p->p2 < p->p1 || p->p2 + 31 > 255) return fail("need 0 <= p1 <= p2 and 31 + p2 <= 255");
    if (p->uniqueness_ratio < 0 || p->uniqueness_ratio > 100) return fail("uniqueness_ratio must be in [0, 100]");
    if (p->smoothing_radius > 8) return fail("smoothing_radius must be <= 8");
    if (p->max_inflight < 1 || p->max_inflight > 4096) return fail("max_inflight must be in [1, 4096]");
    return 0;
}

template <typename T>
int dev_alloc(T **p, size_t count) {
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), count * sizeof(T)));
    return 0;
}

template <typename T>
int engine_alloc(cart_engine *e, T **p, size_t count) {   // a workspace of the engine's lifetime: recorded in e->bufs
    if (dev_alloc(p, count)) return -1;
    e->bufs.push_back(*p);
    return 0;
}

int ensure_rv_partial(cart_engine *e) {   // the fused WTA's right-view partials; the caller holds e->mu
    return ensure_ws_locked(e, reinterpret_cast<void **>(&e->rv_partial), wta_fused_partial_elems(e->g) * sizeof(uint32_t), false);
}

// The slab workspace.  Measured on MI355X (profiles/r03_alloc.txt): the aggregation launch writes its slabs 8-9 % faster into a device
// allocation of at most 8 GiB than into a larger one (1.41-1.43 against 1.53-1.55 ms per 16 pairs at 1242x375 D=128 P=8; the L2's write
// requests to the fabric stall 20-30x as often in the larger one; TLB counters and clock are the same) -- whatever the physical layout
// rule behind it, it goes by the size of the PHYSICAL allocation.  So the workspace is cut into groups of slots, each group one plain
// hipMalloc of at most kSlabChunkBytes (a single slot larger than that gets an allocation of its own).  Round 3 kept one address range
// and backed it with several hipMemCreate / hipMemMap allocations instead; that path met two behaviours of ROCm 7.2's virtual-memory
// management that end in GPU memory access faults (profiles/r04_vmm_faults.txt: a hipMemSetAccess per mapping returns success and leaves
// the range inaccessible; a range re-reserved while other ranges are live did the same) and is gone: nothing in the engine calls
// hipMemAddressReserve / hipMemMap any more.
constexpr size_t kSlabChunkBytes = ((size_t)8 << 30) - ((size_t)64 << 20);
// cart_engine_tune_placement.  Each of the two launches has a fast and a slow level per placement: probed on a warmed-up GPU with real census planes the
// launch pair times at ~2.52-2.57 ms (both fast), ~2.63-2.65 (one slow) or ~2.75-2.78 (both slow) at the headline, and a set re-timed twelve times
// scatters by 0.4 % (profiles/r05_placement.txt sections 2, 5, 6; on an idle GPU straight after engine creation the extremes lie 12-13 % apart,
// which is where round 4's 0.87 came from).  A candidate replaces the kept set when it is 1.5 % faster (both timed back to back); the search stops at
// the first kept set 7 % under the slowest seen (both launches fast against both slow); the kept set is called fast when it is 5.5 % under the
// slowest seen; after kUniformAfter timed placements that are all within 1.5 % of each other the pool offers one kind only.
constexpr float kStopRatio = 0.930f, kFastRatio = 0.945f, kUniformRatio = 0.985f, kSwitchRatio = 0.985f;
constexpr int kUniformAfter = 6;

void slab_pool_free(SlabPool &sp) {
    for (uint8_t *b : sp.base)
        if (b) (void)hipFree(b);
    sp = SlabPool{};
}

// slots per group: as many as fit kSlabChunkBytes; from 16 up a multiple of kLaunchFrames, so that the default launch sequences of a
// call whose lease starts on a multiple of 16 stay inside one group
int slab_group_slots(size_t slot_bytes, int slots) {
    size_t g = std::max<size_t>(1, kSlabChunkBytes / std::max<size_t>(1, slot_bytes));
    if (g >= (size_t)kLaunchFrames) g = g / kLaunchFrames * kLaunchFrames;
    return (int)std::min<size_t>(g, (size_t)slots);
}

int slab_pool_alloc(SlabPool &sp, size_t slot_bytes, int slots) {
    sp = SlabPool{};
    sp.slot_bytes = slot_bytes;
    sp.slots = slots;
    sp.group_slots = slab_group_slots(slot_bytes, slots);
    const int ng = (slots + sp.group_slots - 1) / sp.group_slots;
    for (int gi = 0; gi < ng; ++gi) {
        uint8_t *b = nullptr;
        if (dev_alloc(&b, sp.bytes_of(gi))) { slab_pool_free(sp); return -1; }
        sp.base.push_back(b);
    }
    return 0;
}

// slab pointers of the n frames of one launch at slots [s0, s0 + n); `subst` (may be null) replaces the base of some groups (placement probes)
// A range that does not lie inside the pool (a caller passing a wrong s0 / n) yields an EMPTY table (frame[0] == nullptr) and the callers fail
// on the host: a launch must never see a pointer computed from a slot the pool does not hold (profiles/r04_vmm_faults.txt, fault 3).
SlabTable slab_table(const SlabPool &sp, int s0, int n, const std::vector<uint8_t *> *subst = nullptr) {
    SlabTable t{};
    if (s0 < 0 || n < 1 || n > kMaxLaunchFrames || s0 + n > sp.slots || sp.group_slots < 1) return t;
    for (int f = 0; f < n; ++f) {
        const int s = s0 + f, gi = s / sp.group_slots;
        uint8_t *b = subst && (*subst)[gi] ? (*subst)[gi] : sp.base[gi];
        t.frame[f] = b + (size_t)(s % sp.group_slots) * sp.slot_bytes;
    }
    return t;
}

// The aggregation + WTA launches of `n` frames at slots [s0, s0 + n) with their slabs at `slabs`, on stream `st`: what a compute
// call runs between its census and post stages, and what the placement probe times.  `between` runs between the two launches.
template <typename F>
void launch_agg_wta(cart_engine *e, const Options &opt, const SlabTable &slabs, size_t s0, int n, hipStream_t st, F between) {
    const Geometry &g = e->g;
    uint32_t *cl = e->cen_l + s0 * g.census_elems, *cr = e->cen_r + s0 * g.census_elems;
    uint16_t *wl = e->wta_l + s0 * g.npx;
    uint32_t *rpk = e->right_pk + s0 * g.npx;
    const int plan = plan_for(e, opt, n);
    const bool fused = plan == CART_PLAN_FUSED_UP && e->rv_partial, band = plan == CART_PLAN_BAND_UP;
    AggArgs a = fused ? e->agg_fused : e->agg;
    a.cen_l = cl; a.cen_r = cr; a.slabs = slabs;
    a.ckpt_rows = band && !opt.band_probe ? opt.band_rows : 0;   // the "up" scan stores its checkpoint rows only
    launch_aggregate(a, n, st);
    between();
    if (band) launch_wta_band(cl, cr, slabs, wl, rpk, g, e->uniq_thr, n, opt.band_rows, opt.band_probe, opt.band_diag, st);
    else if (fused) launch_wta_fused(cl, cr, slabs, wl, rpk, e->rv_partial + s0 * wta_fused_partial_elems(g), g, e->uniq_thr, n, st);
    else launch_wta(slabs, wl, rpk, g, e->uniq_thr, n, st, (opt.spec & 4) != 0);
}

}  // namespace

extern "C" {

void cart_engine_default_params(cart_engine_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->device_id = 0;
    p->min_disparity = 4;       // cartconfig.cpp:147
    p->num_disparities = 256;   // cartconfig.cpp:148
    p->paths = 4;               // cv::cuda::createStereoSGM default mode MODE_HH4
    p->p1 = 10; p->p2 = 120;    // cv::cuda::createStereoSGM defaults
    p->uniqueness_ratio = 12;   // disparity.hpp:32
    p->smoothing_radius = -1;   // cartconfig.cpp:150
    p->smoothing_iterations = 5;  // cartconfig.cpp:151
    p->max_inflight = 12;       // CARTSLAM_CONCURRENT_RUN_LIMIT, cartslam.hpp:4
}

int cart_engine_create(const cart_engine_params *params, cart_engine **out) {
    if (!out) return fail("out is NULL");
    *out = nullptr;
    if (validate(params)) return -1;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (params->device_id < 0 || params->device_id >= ndev) return fail("device_id out of range (no such GPU)");
    HIP_TRY(hipSetDevice(params->device_id));
    cart_engine *e = new (std::nothrow) cart_engine();
    if (!e) return fail("out of host memory");
    e->params = *params;
    Geometry &g = e->g;
    g.w = params->width; g.h = params->height; g.D = params->num_disparities; g.P = params->paths;
    g.min_disp = params->min_disparity; g.p1 = params->p1; g.p2 = params->p2;
    g.cpadl = ((g.min_disp + g.D + 15) / 16) * 16;
    g.cpitch = ((g.cpadl + g.w + 16 + 15) / 16) * 16;
    g.npx = (size_t)g.w * g.h;
    g.census_elems = (size_t)g.h * g.cpitch;
    g.slab_bytes = g.npx * g.D;
    e->uniq = (float)(100 - params->uniqueness_ratio) / 100.0f;  // oracle S5
    const size_t n = (size_t)params->max_inflight;
    int rc = 0;
    e->post_only = g.D == 0;   // geometry-only engine: interpolate ping-pong and CCL links are all the post stages need
    if (!e->post_only) {
        rc |= engine_alloc(e, &e->gray_l, n * g.npx);
        rc |= engine_alloc(e, &e->gray_r, n * g.npx);
        // the cooperative window loads of waves whose leading scan lines are still outside the image touch
        // addresses up to (h + D + min_disp + 64) features before / after a frame's census plane
        // and the software-pipelined prefetches run up to 3 rows past the first / last step
        e->cen_slack = (size_t)4 * g.cpitch + g.h + 1024;
        rc |= engine_alloc(e, &e->cen_l_alloc, n * g.census_elems + 2 * e->cen_slack);
        rc |= engine_alloc(e, &e->cen_r_alloc, n * g.census_elems + 2 * e->cen_slack);
        rc |= slab_pool_alloc(e->slab_pool, (size_t)g.P * g.slab_bytes, (int)n);
        rc |= engine_alloc(e, &e->wta_l, n * g.npx);
        rc |= engine_alloc(e, &e->right_pk, n * g.npx);
    }
    rc |= engine_alloc(e, &e->tmp_a, n * g.npx);
    rc |= engine_alloc(e, &e->tmp_b, n * g.npx);
    rc |= engine_alloc(e, &e->ccl_work, n * g.npx);
    if (rc) { cart_engine_destroy(e); return -1; }
    e->cen_l = e->cen_l_alloc + e->cen_slack;
    e->cen_r = e->cen_r_alloc + e->cen_slack;
    // the census padding columns are never written again: out-of-image right features read as 0 (oracle S3)
    if (!e->post_only && (hipMemset(e->cen_l_alloc, 0, (n * g.census_elems + 2 * e->cen_slack) * 4) != hipSuccess ||
                          hipMemset(e->cen_r_alloc, 0, (n * g.census_elems + 2 * e->cen_slack) * 4) != hipSuccess)) {
        cart_engine_destroy(e);
        return fail("hipMemset of census workspace failed");
    }
    e->slots.resize(n);
    for (auto &s : e->slots)
        if (hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) {
            cart_engine_destroy(e);
            return fail("hipEventCreate failed");
        }
    if (e->post_only) { *out = e; return 0; }
    // the WTA kernels' uniqueness test as a table: uniq_threshold() evaluated once per cost by the device function itself
    if (engine_alloc(e, &e->uniq_thr, 2048)) { cart_engine_destroy(e); return -1; }
    launch_uniq_table(e->uniq, e->uniq_thr, nullptr);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) { cart_engine_destroy(e); return fail("building the uniqueness table failed"); }
    build_agg_args(e, e->agg, 0xffu);
    build_agg_args(e, e->agg_fused, 0xffu & ~(1u << 3));  // launch-order slot 3 = {0,-1} = "up" (slab kUpPath)
    // Fused WTA (the "up" direction computed inside the WTA sweep, 1/P less slab traffic): measured on MI355X at
    // 1242x375, batch 16 (profiles/tools/disparity_only.py): D=256 -9 % (4 paths) / -15 % (8 paths) per batch, D=128
    // even, D=64 +4..6 %; D=256 batches of 4 frames: +5 % at 1242x375, -11 % at 1920x1080 -- so it is the default for
    // D=256 batches that give the sweep enough workgroups.  Every plan gives the same bits; cart_engine_set_option
    // overrides the choice (tests and measurements), nothing is read from the environment.
    {   // from ~450 workgroups (16 columns each at D=256) the sweep fills the chip: 6 frames at 1242 px, 4 at 1920 px
        const int nblk = (g.w + 15) / 16;
        e->auto_fused_min_frames = g.D >= 256 ? std::max(2, (448 + nblk - 1) / nblk) : 1 << 30;
    }
    // Banded WTA with the "up" path recomputed from checkpoint rows: D = 128 with 8 paths, launches of at least kBandAutoMinFrames frames
    // (engine_host.h: the measured basis is in DESIGN.md 4.1)
    e->auto_band_min_frames = wta_band_supported(g, kBandRowsDefault, false) ? kBandAutoMinFrames : 1 << 30;
    *out = e;
    return 0;
}

void cart_engine_destroy(cart_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->params.device_id);   // the caller's current device may be another one
    (void)hipDeviceSynchronize();
    slab_pool_free(e->slab_pool);
    for (void *b : e->bufs) (void)hipFree(b);
    for (auto &s : e->slots) {
        if (s.done) (void)hipEventDestroy(s.done);
    }
    for (auto &r : e->ring)
        for (auto &ev : r.ev)
            if (ev) (void)hipEventDestroy(ev);
    delete e;
}

const char *cart_last_error(const cart_engine *) { return g_last_error.c_str(); }

const char *cart_engine_version(void) {
    static char buf[64];
    std::snprintf(buf, sizeof(buf), "cart_engine gfx950 %d kernels", kernel_count());
    return buf;
}

int cart_engine_set_option(cart_engine *e, int option, int value) {
    if (!e) return fail("engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    switch (option) {
        case CART_OPT_PLAN:
            if (value < CART_PLAN_AUTO || value > CART_PLAN_BAND_UP) return fail("unknown plan");
            e->opt_plan = value;
            return 0;
        case CART_OPT_PLAN_MIN_FRAMES:
            if (value < 1) return fail("min frames must be >= 1");
            e->opt_plan_min_frames = value;
            return 0;
        case CART_OPT_CHUNK_FRAMES:
            if (value < 1 || value > kMaxLaunchFrames) return fail("chunk frames must be in [1, 64]");   // 64 = entries of the per-launch slab table (SlabTable); pointer-table (multi) calls stay at kLaunchFrames
            e->chunk_frames = value;
            return 0;
        case CART_OPT_BAND_ROWS:
            if (value != 1 && value != 4 && value != 8 && value != 16) return fail("band rows must be 4, 8 or 16 (1 with the probe)");
            e->opt_band_rows = value;
            return 0;
        case CART_OPT_BAND_PROBE:
            if (value != 0 && value != 1) return fail("the band probe is 0 or 1");
            e->opt_band_probe = value;
            return 0;
        case CART_OPT_BAND_DIAG:
            if (value != 0 && value != 1) return fail("the band diagonal option is 0 or 1");
            e->opt_band_diag = value;   // engines that never take BAND_UP keep the value and never read it
            return 0;
        case CART_OPT_FLOW_GATHER:
            if (value != 0 && value != 1) return fail("the flow gather option is 0 or 1");
            e->opt_flow_gather = value;
            return 0;
        case CART_OPT_SPEC_S8_ZERO_INVALID:
        case CART_OPT_SPEC_S7_REPLICATE_BORDER:
        case CART_OPT_SPEC_S5_TOP2: {
            if (value != 0 && value != 1) return fail("spec variants are 0 or 1");
            const int bit = option == CART_OPT_SPEC_S8_ZERO_INVALID ? 1 : option == CART_OPT_SPEC_S7_REPLICATE_BORDER ? 2 : 4;
            e->opt_spec = value ? (e->opt_spec | bit) : (e->opt_spec & ~bit);
            return 0;
        }
        default: return fail("unknown option");
    }
}

int cart_engine_get_option(cart_engine *e, int option, int *value) {
    if (!e || !value) return fail("bad arguments");
    std::lock_guard<std::mutex> lk(e->mu);
    switch (option) {
        case CART_OPT_PLAN: *value = e->opt_plan; return 0;
        case CART_OPT_PLAN_MIN_FRAMES: *value = e->opt_plan_min_frames; return 0;
        case CART_OPT_CHUNK_FRAMES: *value = e->chunk_frames; return 0;
        case CART_OPT_BAND_ROWS: *value = e->opt_band_rows; return 0;
        case CART_OPT_BAND_PROBE: *value = e->opt_band_probe; return 0;
        case CART_OPT_BAND_DIAG: *value = e->opt_band_diag; return 0;
        case CART_OPT_FLOW_GATHER: *value = e->opt_flow_gather; return 0;
        case CART_OPT_SPEC_S8_ZERO_INVALID: *value = (e->opt_spec & 1) ? 1 : 0; return 0;
        case CART_OPT_SPEC_S7_REPLICATE_BORDER: *value = (e->opt_spec & 2) ? 1 : 0; return 0;
        case CART_OPT_SPEC_S5_TOP2: *value = (e->opt_spec & 4) ? 1 : 0; return 0;
        default: return fail("unknown option");
    }
}

int cart_engine_describe_plan(cart_engine *e, int n_frames, cart_launch_plan *out) {
    if (!e || !out) return fail("bad arguments");
    if (e->post_only) return fail("this engine was created without SGM workspaces (num_disparities = 0)");
    if (n_frames < 1) return fail("n_frames must be positive");
    std::lock_guard<std::mutex> lk(e->mu);
    const Options o = snapshot_options(e);
    out->frames_per_launch = std::min(n_frames, o.chunk_frames);
    out->plan = plan_for(e, o, out->frames_per_launch);
    // (BAND_UP: P - 1 whole slabs + the checkpoint rows, 1/K of one more; the probe stores all P)
    out->slabs_written = out->plan == CART_PLAN_FUSED_UP || (out->plan == CART_PLAN_BAND_UP && !o.band_probe) ? e->g.P - 1 : e->g.P;
    return 0;
}

namespace {
// Time of the aggregation + WTA launches of `n` frames at slots [s0, s0 + n) with their slabs at `slabs` (ms, best of three after one
// warm-up; the census planes hold whatever they hold: the cost of these launches does not depend on the data).  < 0 on error.
float probe_placement(cart_engine *e, const Options &opt, const SlabTable &slabs, size_t s0, int n, hipEvent_t ev0, hipEvent_t ev1) {
    const Geometry &g = e->g;
    if (!slabs.frame[0]) return -1.f;   // slot range outside the pool (slab_table)
    uint32_t *rpk = e->right_pk + s0 * g.npx;
    float best = -1.f;
    for (int rep = 0; rep < 4; ++rep) {   // one warm-up (first touch of a fresh allocation), three timed: the fastest counts
        if (hipMemsetAsync(rpk, 0xff, (size_t)n * g.npx * sizeof(uint32_t), nullptr) != hipSuccess) return -1.f;   // what launch_census leaves there
        if (hipEventRecord(ev0, nullptr) != hipSuccess) return -1.f;
        launch_agg_wta(e, opt, slabs, s0, n, nullptr, [] {});
        if (hipEventRecord(ev1, nullptr) != hipSuccess || hipEventSynchronize(ev1) != hipSuccess || hipGetLastError() != hipSuccess) return -1.f;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) return -1.f;
        if (rep && (best < 0.f || ms < best)) best = ms;
    }
    return best;
}
}  // namespace

int cart_engine_tune_placement(cart_engine *e, int n_frames, int max_tries, size_t max_extra_bytes, cart_placement_report *report) {
    if (report) std::memset(report, 0, sizeof(*report));
    if (!e) return fail("engine is NULL");
    if (e->post_only) return fail("this engine was created without SGM workspaces (num_disparities = 0)");
    if (n_frames < 1 || n_frames > (int)e->slots.size()) return fail("n_frames must be in [1, max_inflight]");
    HIP_TRY(hipSetDevice(e->params.device_id));
    std::unique_lock<std::mutex> lk(e->mu);
    for (const auto &sl : e->slots)
        if (sl.busy) return fail("cart_engine_tune_placement needs an idle engine");
    const Options opt = snapshot_options(e);
    HIP_TRY(hipDeviceSynchronize());
    const int n = std::min(n_frames, opt.chunk_frames);
    if (plan_for(e, opt, n) == CART_PLAN_FUSED_UP && ensure_rv_partial(e)) return -1;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    HIP_TRY(hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) { (void)hipEventDestroy(ev0); return fail("hipEventCreate failed"); }
    SlabPool &sp = e->slab_pool;
    // The search runs per UNIT = the groups behind the slots [k n, (k + 1) n) of one n-frame call, for the first (at most four) such
    // ranges: a lease takes the lowest free range its stream used last (SlotLease::begin), so a caller with one call in flight lives in unit 0
    // and one with several walks up the units.  A group already settled by an earlier unit is not touched again.  A group that holds
    // more slots than the launch has frames (32-slot groups, 16-frame launches) is scored on the slots of its first launch only.
    const int units = std::max(1, std::min(4, (int)e->slots.size() / n));
    std::vector<char> settled((size_t)sp.groups(), 0);
    // Candidates that lost stay allocated while the search goes on (freed at once, their pages would come straight back from the
    // allocator), oldest first out when the byte cap is reached; everything is plain hipMalloc / hipFree.
    struct Held { uint8_t *p; size_t bytes; };
    std::vector<Held> held;
    size_t extra = 0;
    const auto t_begin = std::chrono::steady_clock::now();
    auto seconds_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    // Allocating tens of GB takes 0.1-0.6 s per candidate: no more than 0.25 s per allowed try + 1 s per 20 GB of workspace in all (the caller
    // buys search time with max_tries), and every unit gets its own share of that, so that unit 0 cannot spend what units 1-3 were promised.
    const double unit_budget = (0.25 * max_tries + (double)sp.slots * (double)sp.slot_bytes / 20e9) / units;
    double sum_first = 0.0, sum_kept = 0.0;
    int rc = 0, probed = 0, total_candidates = 0;
    for (int u = 0; u < units && rc == 0; ++u) {
        const auto t_unit = std::chrono::steady_clock::now();
        const int s0 = u * n, g0 = s0 / sp.group_slots, g1 = (s0 + n - 1) / sp.group_slots;
        std::vector<int> mine;
        size_t unit_bytes = 0;
        for (int gi = g0; gi <= g1; ++gi)
            if (!settled[(size_t)gi]) { mine.push_back(gi); unit_bytes += sp.bytes_of(gi); settled[(size_t)gi] = 1; }
        float kept = probe_placement(e, opt, slab_table(sp, s0, n), (size_t)s0, n, ev0, ev1);
        if (kept < 0.f) { rc = fail("placement probe failed"); break; }
        sum_first += kept;
        ++probed;
        // Every candidate is judged against the kept set RE-TIMED right after it (same clock, same temperature: the GPU's clock drifts by a few per
        // cent over a search, which is as much as the modes differ), and replaces it only when it is kSwitchRatio faster -- a search that follows
        // the probe's noise ends on a worse set than it started from as often as not (profiles/r05_placement.txt section 5).  `worst_rel` = the
        // slowest set seen, as a multiple of the kept one.
        float worst_rel = 1.f;
        int seen = 1, stop = mine.empty() ? CART_PLACE_STOP_NOTHING_TO_DO : CART_PLACE_STOP_TRIES;
        // at most this many bytes beyond the workspace at any time (0 = two units' worth); SIZE_MAX = whatever leaves 4 GiB free
        const size_t cap = max_extra_bytes ? max_extra_bytes : 2 * unit_bytes;
        for (int t = 1; t < max_tries && !mine.empty(); ++t) {
            // a kept placement 7 % under the slowest pair seen has both launches in their fast modes -- stop looking
            if (worst_rel * kStopRatio > 1.f) { stop = CART_PLACE_STOP_FAST_FOUND; break; }
            // A process in which no placement is fast (round 4's driver box: 64 candidates between 2.57 and 2.60 ms, 7.7 s of search for 1.4 %): once
            // kUniformAfter placements have been timed and the slowest is within 1.5 % of the kept one, there is nothing to find here -- stop.
            if (seen >= kUniformAfter && worst_rel * kUniformRatio < 1.f) { stop = CART_PLACE_STOP_UNIFORM; break; }
            if (seconds_since(t_unit) > unit_budget) { stop = CART_PLACE_STOP_TIME; break; }
            while (extra + unit_bytes > cap && !held.empty()) {   // make room under the cap: the oldest loser goes
                (void)hipFree(held.front().p);
                extra -= held.front().bytes;
                held.erase(held.begin());
            }
            if (extra + unit_bytes > cap) { stop = CART_PLACE_STOP_MEMORY; break; }
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < unit_bytes + ((size_t)4 << 30)) { stop = CART_PLACE_STOP_MEMORY; break; }   // no room for another candidate
            std::vector<uint8_t *> cand((size_t)sp.groups(), nullptr);
            bool ok = true;
            for (int gi : mine)
                if (dev_alloc(&cand[(size_t)gi], sp.bytes_of(gi))) { ok = false; break; }
            if (!ok) {
                (void)hipGetLastError();
                for (int gi : mine) if (cand[(size_t)gi]) (void)hipFree(cand[(size_t)gi]);
                stop = CART_PLACE_STOP_MEMORY;
                break;
            }
            extra += unit_bytes;
            const float sc = probe_placement(e, opt, slab_table(sp, s0, n, &cand), (size_t)s0, n, ev0, ev1);
            const float again = sc < 0.f ? -1.f : probe_placement(e, opt, slab_table(sp, s0, n), (size_t)s0, n, ev0, ev1);
            if (sc < 0.f || again < 0.f) {
                for (int gi : mine) (void)hipFree(cand[(size_t)gi]);
                extra -= unit_bytes;
                rc = fail("placement probe failed");
                break;
            }
            ++seen;
            const float rel = sc / again;   // the candidate as a multiple of the kept set, both timed now
            const bool better = rel < kSwitchRatio;
            for (int gi : mine) {   // the loser of every group joins the held list
                uint8_t *lose = better ? sp.base[(size_t)gi] : cand[(size_t)gi];
                if (better) sp.base[(size_t)gi] = cand[(size_t)gi];
                held.push_back(Held{lose, sp.bytes_of(gi)});
            }
            if (better) { worst_rel = std::max(worst_rel / rel, 1.f / rel); kept = sc; }   // everything seen so far, the old kept set included, relative to the new one
            else { worst_rel = std::max(worst_rel, rel); kept = again; }
        }
        if (stop == CART_PLACE_STOP_TRIES && worst_rel * kStopRatio > 1.f) stop = CART_PLACE_STOP_FAST_FOUND;   // the last allowed try was the fast one
        const float worst = kept * worst_rel;
        sum_kept += kept;
        total_candidates += seen;
        if (u == 0 && report && rc == 0) {   // the unit a caller with one call in flight lives in
            report->stop_reason = stop;
            report->mode = worst_rel * kFastRatio > 1.f ? CART_PLACE_MODE_FAST
                         : (seen >= kUniformAfter && worst_rel * kUniformRatio < 1.f) ? CART_PLACE_MODE_UNIFORM
                         : seen == 1 ? CART_PLACE_MODE_UNKNOWN : CART_PLACE_MODE_MIXED;
            report->ms_fastest_seen = kept;
            report->ms_slowest_seen = worst;
        }
    }
    (void)hipDeviceSynchronize();
    for (auto &h : held) (void)hipFree(h.p);
    (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
    if (probed && rc == 0 && report) {   // mean over the probed units, before and after
        report->ms_first = (float)(sum_first / probed);
        report->ms_kept = (float)(sum_kept / probed);
        report->units = probed;
        report->candidates = total_candidates;
        report->seconds = (float)seconds_since(t_begin);
    }
    return rc;
}

int cart_engine_set_timing(cart_engine *e, int enabled) {
    if (!e) return fail("engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    if (enabled && e->ring.empty()) {
        e->ring.resize(kTimingRing);
        for (auto &r : e->ring)
            for (auto &ev : r.ev)
                if (hipEventCreate(&ev) != hipSuccess) return fail("hipEventCreate failed");
    }
    for (auto &r : e->ring) r.n = 0;
    e->ring_calls = 0;
    e->timing = enabled != 0;
    e->timing_every = enabled > 1 ? enabled : 1;
    e->timing_calls = 0;
    return 0;
}

int cart_engine_collect_timing(cart_engine *e, const char **names, float *mean_ms, int cap, int *n_calls) {
    if (!e || !names || !mean_ms) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(e->mu);
    int nstages = 0, calls = 0;
    double sum[kMaxTimings] = {};
    for (auto &r : e->ring) {
        if (r.n == 0) continue;
        if (nstages == 0) { nstages = r.n; for (int i = 0; i < r.n; ++i) names[i < cap ? i : 0] = r.names[i]; }
        if (r.n != nstages) continue;
        for (int i = 0; i < r.n; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.ev[i], r.ev[i + 1]) != hipSuccess) return fail("hipEventElapsedTime failed");
            sum[i] += ms;
        }
        ++calls;
    }
    const int n = std::min(cap, nstages);
    for (int i = 0; i < n; ++i) mean_ms[i] = calls ? (float)(sum[i] / calls) : 0.f;
    if (n_calls) *n_calls = calls;
    return n;
}

namespace {
// Where the frames of one call live: a base + stride per image (the batch entry point) or one pointer per frame (multi).
struct FrameSet {
    const uint8_t *left, *right; size_t left_fs, right_fs;
    int16_t *out; size_t out_fs;
    const uint8_t *const *lefts, *const *rights; int16_t *const *outs;   // non-NULL: scattered frames
    size_t left_step, right_step, out_step;
    ImageBatch images(bool right_side, int f0, int n) const {
        const size_t step = right_side ? right_step : left_step;
        if (!lefts) return strided_images((right_side ? right : left) + (size_t)f0 * (right_side ? right_fs : left_fs), step, right_side ? right_fs : left_fs);
        ImageBatch b{}; b.step = step; b.scattered = 1;
        for (int f = 0; f < n; ++f) b.frames[f] = (right_side ? rights : lefts)[f0 + f];
        return b;
    }
    OutBatch output(int f0, int n) const {
        if (!outs) return strided_out(reinterpret_cast<int16_t *>(reinterpret_cast<uint8_t *>(out) + (size_t)f0 * out_fs), out_step, out_fs);
        OutBatch b{}; b.step = out_step; b.scattered = 1;
        for (int f = 0; f < n; ++f) b.frames[f] = outs[f0 + f];
        return b;
    }
};

int compute_disparity_impl(cart_engine *e, int n_frames, const FrameSet &fr, int channels, void *stream_) {
    if (!e) return fail("engine is NULL");
    if (e->post_only) return fail("this engine was created without SGM workspaces (num_disparities = 0)");
    if (channels != 1 && channels != 3) return fail("channels must be 1 (gray) or 3 (BGR)");
    const Geometry &g = e->g;
    if (fr.left_step < (size_t)g.w * channels || fr.right_step < (size_t)g.w * channels) return fail("input step smaller than a row");
    if (fr.out_step < (size_t)g.w * 2 || (fr.out_step & 1)) return fail("out_step must be even and >= 2*width");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(e->params.device_id));
    Options opt;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        opt = snapshot_options(e);
        // later (shorter) launches of the call never need more
        if (plan_for(e, opt, std::min(n_frames, opt.chunk_frames)) == CART_PLAN_FUSED_UP && ensure_rv_partial(e)) return -1;
    }
    SlotLease l;
    if (l.begin(e, n_frames, stream)) return -1;
    g_last_slot = l.s0;
    TimingRec *rec = nullptr;
    if (opt.timing) {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!e->ring.empty() && e->timing_calls++ % (unsigned long long)e->timing_every == 0) { rec = &e->ring[e->ring_calls++ % kTimingRing]; rec->n = 0; }
    }
    int nt = 0;
    auto stage = [&](const char *name, hipStream_t st) {   // a stage of this call begins on `st`
        if (!rec || nt >= kMaxTimings) return;
        (void)hipEventRecord(rec->ev[nt], st);
        rec->names[nt++] = name;
    };
    const int radius = e->params.smoothing_radius, iters = e->params.smoothing_iterations;
    const bool smooth = radius > 0 && iters > 0;  // disparity.cu:73
    const size_t tight_step = (size_t)g.w * 2, tight_fs = g.npx * 2;
    // Enqueues every stage for frames [f0, f0+n) of this call on stream `st`.
    bool bad_slots = false;
    auto enqueue = [&](int f0, int n, hipStream_t st, bool timed) {
        const size_t s0 = (size_t)l.s0 + f0;
        const SlabTable slabs = slab_table(e->slab_pool, (int)s0, n);
        if (!slabs.frame[0]) { bad_slots = true; return; }   // nothing is launched on a slot range the pool does not hold
        uint8_t *gl = e->gray_l + s0 * g.npx, *gr = e->gray_r + s0 * g.npx;
        uint32_t *cl = e->cen_l + s0 * g.census_elems, *cr = e->cen_r + s0 * g.census_elems;
        uint16_t *wl = e->wta_l + s0 * g.npx;
        uint32_t *rpk = e->right_pk + s0 * g.npx;
        int16_t *ta = e->tmp_a + s0 * g.npx, *tb = e->tmp_b + s0 * g.npx;
        const OutBatch o = fr.output(f0, n);
        TimingRec *rec_save = rec;
        if (!timed) rec = nullptr;
        stage("census", st);
        launch_census(fr.images(false, f0, n), fr.images(true, f0, n), channels, n, gl, gr, cl, cr, rpk, g, st);
        stage("aggregate", st);
        launch_agg_wta(e, opt, slabs, s0, n, st, [&] { stage("wta", st); });
        stage("post", st);
        // disparity.hpp:27-28: minDisparity = cfg*16, maxDisparity = image width (not x16)
        const int min16 = e->params.min_disparity * 16, maxd = g.w;
        if (!smooth) {
            launch_post(wl, rpk, gl, o, g, n, st, opt.spec);
        } else {
            int16_t *src = ta, *dst = tb;
            int it = 0;
            if (post_interp_fusable(radius, min16, maxd)) {   // the first pass rides on the post stage: one launch, no intermediate image
                launch_post_interp(wl, rpk, gl, iters == 1 ? o : strided_out(ta, tight_step, tight_fs), g, n, st, opt.spec, min16, maxd);
                it = 1;
            } else {
                launch_post(wl, rpk, gl, strided_out(ta, tight_step, tight_fs), g, n, st, opt.spec);
            }
            if (it < iters) stage("interpolate", st);
            for (; it < iters; ++it) {
                const bool last = it == iters - 1;
                launch_interpolate(src, tight_step, tight_fs, last ? o : strided_out(dst, tight_step, tight_fs), g.w, g.h, radius, min16, maxd, n, st);
                std::swap(src, dst);
            }
        }
        if (rec) {
            (void)hipEventRecord(rec->ev[nt], st);
            std::lock_guard<std::mutex> lk(e->mu);
            rec->n = nt;
        }
        rec = rec_save;
    };
    // Large batches run as cache-sized sub-batches on the caller's stream: the census planes every direction
    // re-reads (4.2 MB per frame) then stay in L2 + Infinity Cache (measured: 64 frames in one launch are 13 %
    // slower per frame than 4 x 16).  Two-stream overlap of sub-batches was measured and buys nothing.
    const int chunk = fr.lefts ? std::min(opt.chunk_frames, kLaunchFrames) : opt.chunk_frames;  // pointer tables hold kLaunchFrames entries
    for (int f0 = 0; f0 < n_frames; f0 += chunk) enqueue(f0, std::min(chunk, n_frames - f0), stream, f0 == 0);
    const hipError_t err = hipGetLastError();
    if (bad_slots) return fail("internal error: a launch's slot range lies outside the slab pool");
    if (err != hipSuccess) return fail(std::string("kernel launch failed: ") + hipGetErrorString(err));
    return 0;
}
}  // namespace

int cart_compute_disparity_batch(cart_engine *e, int n_frames, const uint8_t *left, size_t left_step,
                                 size_t left_frame_stride, const uint8_t *right, size_t right_step,
                                 size_t right_frame_stride, int channels, int16_t *out, size_t out_step,
                                 size_t out_frame_stride, void *stream) {
    if (!left || !right || !out) return fail("NULL image pointer");
    if (out_frame_stride & 1) return fail("out_frame_stride must be even");
    FrameSet fr{};
    fr.left = left; fr.right = right; fr.left_fs = left_frame_stride; fr.right_fs = right_frame_stride; fr.out = out; fr.out_fs = out_frame_stride;
    fr.left_step = left_step; fr.right_step = right_step; fr.out_step = out_step;
    return compute_disparity_impl(e, n_frames, fr, channels, stream);
}

int cart_compute_disparity_multi(cart_engine *e, int n_frames, const uint8_t *const *left, size_t left_step,
                                 const uint8_t *const *right, size_t right_step, int channels, int16_t *const *out,
                                 size_t out_step, void *stream) {
    if (!left || !right || !out) return fail("NULL pointer table");
    for (int f = 0; f < n_frames; ++f) {
        if (!left[f] || !right[f] || !out[f]) return fail("NULL image pointer in a pointer table");
        if (reinterpret_cast<uintptr_t>(out[f]) & 1) return fail("output images must be 2-byte aligned");
    }
    FrameSet fr{};
    fr.lefts = left; fr.rights = right; fr.outs = out;
    fr.left_step = left_step; fr.right_step = right_step; fr.out_step = out_step;
    return compute_disparity_impl(e, n_frames, fr, channels, stream);
}

int cart_compute_disparity(cart_engine *e, const uint8_t *left, size_t left_step, const uint8_t *right,
                           size_t right_step, int channels, int16_t *out, size_t out_step, void *stream) {
    return cart_compute_disparity_batch(e, 1, left, left_step, 0, right, right_step, 0, channels, out, out_step, 0, stream);
}

int cart_debug_slab_layout(cart_engine *e, int *group_slots, int *n_groups, size_t *slot_bytes, size_t *group_bytes) {
    if (!e) return fail("engine is NULL");
    if (e->post_only) return fail("this engine was created without SGM workspaces (num_disparities = 0)");
    const SlabPool &sp = e->slab_pool;
    if (group_slots) *group_slots = sp.group_slots;
    if (n_groups) *n_groups = sp.groups();
    if (slot_bytes) *slot_bytes = sp.slot_bytes;
    if (group_bytes) *group_bytes = sp.bytes_of(0);
    return 0;
}

int cart_debug_ccl_scratch_nonzero(cart_engine *e, size_t *nonzero) {
    if (!e || !nonzero) return fail("bad arguments");
    *nonzero = 0;
    if (!e->ccl_stats_ws) return 0;
    HIP_TRY(hipSetDevice(e->params.device_id));
    HIP_TRY(hipDeviceSynchronize());
    try {
        const size_t per_slot = e->g.npx * kCclStatInts;   // the statistics scratch of one slot (the segment counts behind it are overwritten, not accumulated)
        std::vector<int32_t> host(per_slot);
        for (size_t sl = 0; sl < e->slots.size(); ++sl) {
            HIP_TRY(hipMemcpy(host.data(), e->ccl_stats_ws + sl * per_slot, per_slot * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int32_t v : host) *nonzero += v != 0;
        }
    } catch (const std::bad_alloc &) { return fail("out of host memory"); }
    return 0;
}

int cart_debug_uniq_table(cart_engine *e, int uniqueness_ratio, uint16_t *out2048) {
    if (!out2048) return fail("bad arguments");
    if (uniqueness_ratio < 0 || uniqueness_ratio > 100) return fail("uniqueness_ratio must be in [0, 100]");
    const float u = (float)(100 - uniqueness_ratio) / 100.0f;   // as cart_engine_create (oracle S5)
    if (!e) { uniq_table_host(u, out2048); return 0; }
    HIP_TRY(hipSetDevice(e->params.device_id));
    uint16_t *dev = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dev), 2048 * sizeof(uint16_t)));
    launch_uniq_table(u, dev, nullptr);
    hipError_t err = hipMemcpy(out2048, dev, 2048 * sizeof(uint16_t), hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    if (err != hipSuccess) return fail(std::string("uniq table: ") + hipGetErrorString(err));
    return 0;
}

int cart_debug_read(cart_engine *e, int frame_slot, int what, void *host_dst, size_t bytes) {
    if (!e || !host_dst) return fail("bad arguments");
    if (e->post_only) return fail("this engine has no SGM workspaces");
    const Geometry &g = e->g;
    const int slot = g_last_slot + frame_slot;
    if (frame_slot < 0 || slot >= (int)e->slots.size()) return fail("frame_slot out of range");
    HIP_TRY(hipSetDevice(e->params.device_id));
    HIP_TRY(hipDeviceSynchronize());
    const void *src = nullptr;
    size_t need = 0;
    try {
    if (what == CART_DBG_GRAY_L || what == CART_DBG_GRAY_R) {
        src = (what == CART_DBG_GRAY_L ? e->gray_l : e->gray_r) + (size_t)slot * g.npx; need = g.npx;
        if (bytes < need) return fail("buffer too small");
        HIP_TRY(hipMemcpy(host_dst, src, need, hipMemcpyDeviceToHost));
    } else if (what == CART_DBG_CENSUS_L || what == CART_DBG_CENSUS_R) {
        const uint32_t *c = (what == CART_DBG_CENSUS_L ? e->cen_l : e->cen_r) + (size_t)slot * g.census_elems + g.cpadl;
        need = g.npx * 4;
        if (bytes < need) return fail("buffer too small");
        HIP_TRY(hipMemcpy2D(host_dst, (size_t)g.w * 4, c, (size_t)g.cpitch * 4, (size_t)g.w * 4, g.h, hipMemcpyDeviceToHost));
    } else if (what >= CART_DBG_PATH0 && what < CART_DBG_PATH0 + g.P) {
        src = e->slab_pool.slot_ptr(slot) + (size_t)(what - CART_DBG_PATH0) * g.slab_bytes; need = g.npx * g.D;
        if (bytes < need) return fail("buffer too small");
        std::vector<uint8_t> raw(need);
        HIP_TRY(hipMemcpy(raw.data(), src, need, hipMemcpyDeviceToHost));
        uint8_t *d = static_cast<uint8_t *>(host_dst);  // undo the in-slab chunk order -> plain [h][w][D]
        for (size_t c = 0; c < need; c += 16)
            for (int k = 0; k < 16; ++k) d[c + kSlabChunkOrder[k]] = raw[c + k];
    } else if (what == CART_DBG_WTA_L) {
        src = e->wta_l + (size_t)slot * g.npx; need = g.npx * 2;
        if (bytes < need) return fail("buffer too small");
        HIP_TRY(hipMemcpy(host_dst, src, need, hipMemcpyDeviceToHost));
    } else if (what == CART_DBG_WTA_R) {  // packed (cost<<16 | disparity) -> u16 disparity
        std::vector<uint32_t> tmp(g.npx);
        need = g.npx * 2;
        if (bytes < need) return fail("buffer too small");
        HIP_TRY(hipMemcpy(tmp.data(), e->right_pk + (size_t)slot * g.npx, g.npx * 4, hipMemcpyDeviceToHost));
        uint16_t *d = static_cast<uint16_t *>(host_dst);
        for (size_t i = 0; i < g.npx; ++i) d[i] = (uint16_t)(tmp[i] & 0xffffu);
    } else {
        return fail("unknown debug selector");
    }
    } catch (const std::bad_alloc &) { return fail("out of host memory"); }   // the staging vectors (a slab is up to 530 MB)
    return 0;
}

}  // extern "C"

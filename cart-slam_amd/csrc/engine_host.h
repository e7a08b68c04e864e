// engine_host.h -- what the host translation units of the C ABI share (cart_engine.hip, engine_*.hip): error reporting, the
// engine with its slot and slab pools, the scoped slot lease, the per-slot workspaces, the lifecycle of the device objects and the
// argument checks the entry points share.
// Private to csrc/; the host <-> kernel contract is engine_internal.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "engine_internal.h"

#pragma GCC visibility push(hidden)   // nothing declared here is part of the library's interface

namespace cart_amd {

extern thread_local std::string g_last_error;   // cart_last_error
extern thread_local int g_last_slot;            // first slot of this thread's most recent compute lease (cart_debug_read)

int fail(const std::string &msg);   // sets g_last_error, returns -1

// ---- argument checks shared by the entry points (engine_checks.hip): each returns 0, or fail() with the message quoted ----
int check_positive(const char *name, double v);   // "<name> must be a positive number" unless v > 0 and finite
int check_camera(const cart_ego_camera *cam);     // "camera is NULL"; fx, fy, baseline positive numbers, "cx / cy must be finite"
int check_pose(const char *name, const double *m);   // "<name> is NULL"; "<name>[k] must be finite and within 2 (rotation) / 1e6 (translation)", 3 x 4 row-major
int check_frame_size(int w, int h);               // "width / height must be in [1, 16384]"
int check_max_size(int max_width, int max_height);   // the same for "max_width / max_height"

struct Extent {   // one device argument, for the checks: `rows` rows of `row_bytes`, `step` apart; elem = the alignment of the pointer and the step
    const char *name;
    const void *ptr;
    size_t step, elem, row_bytes;
    int rows;
    static Extent image(const char *name, const void *ptr, size_t step, size_t elem, int w, int h) {   // a w x h image of elem-byte pixels
        return Extent{name, ptr, step, elem, (size_t)w * elem, h};
    }
    uintptr_t begin() const { return reinterpret_cast<uintptr_t>(ptr); }
    uintptr_t end() const { return begin() + (size_t)(rows - 1) * step + row_bytes; }
};
int check_pitched(const Extent &x);               // "<name> and its step must be <elem>-byte aligned", then "<name>_step is below the row size"
bool overlap(const Extent &a, const Extent &b);
// all[first_output .. n) are the outputs: each against every entry before it, "<earlier> and <later> must not overlap"; NULL entries are skipped
int check_outputs_apart(const Extent *all, int first_output, int n);

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess)                                                                       \
            return fail(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + __FILE__ + ":" + \
                        std::to_string(__LINE__) + ")");                                           \
    } while (0)

struct Slot {
    bool busy = false;
    hipEvent_t done = nullptr;          // recorded only on the FIRST slot of a lease ...
    int owner = -1;                     // ... every slot of the lease points at that slot
    hipStream_t last_stream = nullptr;
    bool used = false;
    unsigned long long released_seq = 0;  // order of the last release (guarded by mu)
};

// Plan BAND_UP (sgm_wta.hip, wta_band_kernel): rows per band, and the launch size from which CART_PLAN_AUTO takes the plan at D = 128 with
// 8 paths.  Both from the A/B at 1242x375 in DESIGN.md 4.1 (profiles/band_up.txt).
constexpr int kBandRowsDefault = 8;
constexpr int kBandDiagDefault = 1;     // the banded WTA rebuilds the up-right diagonal in LDS (CART_OPT_BAND_DIAG; profiles/band_diag.txt)
constexpr int kBandAutoMinFrames = 4;   // 2-frame launches stay on SLABS; 4, 6, 8, 12 and 16 frames measured
constexpr int kMaxTimings = 8;
constexpr int kTimingRing = 256;

struct TimingRec {
    hipEvent_t ev[kMaxTimings + 1] = {};
    const char *names[kMaxTimings] = {};
    int n = 0;
};

// The slab workspace: one plain hipMalloc per GROUP of workspace slots, no group larger than kSlabChunkBytes (see slab_pool_alloc).
// Slot s lives at base[s / group_slots] + (s % group_slots) * slot_bytes; the kernels of a launch get the slab pointers of their
// frames as a table (SlabTable), so a launch may span groups.
struct SlabPool {
    std::vector<uint8_t *> base;   // one device allocation per group
    int group_slots = 0;           // slots per group (the last group may hold fewer)
    int slots = 0;
    size_t slot_bytes = 0;         // P path slabs of one frame
    int groups() const { return (int)base.size(); }
    int slots_of(int gi) const { return std::min(group_slots, slots - gi * group_slots); }
    size_t bytes_of(int gi) const { return (size_t)slots_of(gi) * slot_bytes; }
    uint8_t *slot_ptr(int s) const { return base[s / group_slots] + (size_t)(s % group_slots) * slot_bytes; }
};

}  // namespace cart_amd

struct cart_engine {
    cart_engine_params params;
    cart_amd::Geometry g;
    float uniq;
    uint16_t *uniq_thr = nullptr;   // device: integer uniqueness threshold of every best cost 0..2047 for this engine's ratio (WTA kernels)
    // workspaces, each [max_inflight][...]
    uint8_t *gray_l = nullptr, *gray_r = nullptr;
    uint32_t *cen_l = nullptr, *cen_r = nullptr;      // point `cen_slack` elements into their allocations
    uint32_t *cen_l_alloc = nullptr, *cen_r_alloc = nullptr;
    size_t cen_slack = 0;
    uint16_t *wta_l = nullptr;
    uint32_t *right_pk = nullptr;
    int16_t *tmp_a = nullptr, *tmp_b = nullptr;  // tight s16 planes (interpolate ping-pong)
    int32_t *ccl_work = nullptr;
    // allocated by the first call that needs them (ensure_ws)
    uint32_t *rv_partial = nullptr; // [max_inflight][wta_fused_partial_elems]: fused batches
    uint8_t *flow_ws = nullptr;     // [max_inflight][flow_ws_bytes]: gray x2, census x2, scratch (cart_optical_flow)
    uint8_t *flow_pyr_ws = nullptr; // [max_inflight][FlowPyrLayout::bytes]: level images, census planes and level flows (cart_optical_flow_pyramid)
    int32_t *ccl_stats_ws = nullptr; // component-table workspace: [max_inflight][npx][kCclStatInts] scratch + [max_inflight][h][tile columns]
    unsigned *sp_votes = nullptr;   // [max_inflight][kSpMaxLabels*3] (cart_superpixel_plane_classify)
    std::vector<void *> bufs;       // every device allocation above, freed by cart_engine_destroy
    cart_amd::AggArgs agg;
    cart_amd::AggArgs agg_fused;    // the same launch without the "up" direction (computed inside wta_fused_kernel)
    cart_amd::SlabPool slab_pool;   // the cost slabs of every slot (slab_pool_alloc / slab_pool_free / cart_engine_tune_placement)
    int auto_fused_min_frames = 1 << 30; // CART_OPT_PLAN = auto: launches of at least this many frames take the fused WTA
    int opt_plan = CART_PLAN_AUTO;       // cart_engine_set_option
    int auto_band_min_frames = 1 << 30;  // CART_OPT_PLAN = auto: launches of at least this many frames take BAND_UP (D = 128, 8 paths)
    int opt_band_rows = cart_amd::kBandRowsDefault, opt_band_probe = 0;   // CART_OPT_BAND_ROWS / CART_OPT_BAND_PROBE
    int opt_band_diag = cart_amd::kBandDiagDefault;                       // CART_OPT_BAND_DIAG
    int opt_plan_min_frames = 1;         // with a forced plan: launches of fewer frames still take CART_PLAN_SLABS
    int opt_flow_gather = 0;             // CART_OPT_FLOW_GATHER
    int opt_spec = 0;                    // CART_OPT_SPEC_* bits: upstream variants of S8 / S7 (default: the oracle's spec)
    std::mutex mu;
    std::condition_variable cv;
    std::vector<cart_amd::Slot> slots;
    unsigned long long release_counter = 0;    // guarded by mu
    int chunk_frames = cart_amd::kLaunchFrames;   // frames per launch sequence inside one batched call
    bool post_only = false;         // no SGM workspaces (num_disparities == 0)
    bool timing = false;
    int timing_every = 1;           // stage events on every timing_every-th compute call (cart_engine_set_timing)
    unsigned long long timing_calls = 0;   // compute calls seen while timing is on (guarded by mu)
    std::vector<cart_amd::TimingRec> ring;  // stage events of the last kTimingRing compute calls (guarded by mu)
    size_t ring_calls = 0;
};

namespace cart_amd {

// One entry point's hold on `n` contiguous workspace slots [s0, s0 + n).  begin() waits for a free range and makes `stream`
// wait for earlier work on it from other streams.  Once begin() has succeeded, the end of the guard's scope -- every way out of
// the call, after its last launch on `stream` -- records the lease's event there and hands the slots back.
class SlotLease {
   public:
    SlotLease() = default;
    SlotLease(const SlotLease &) = delete;
    SlotLease &operator=(const SlotLease &) = delete;
    int begin(cart_engine *e, int n, hipStream_t stream);
    ~SlotLease();
    int s0 = -1;

   private:
    cart_engine *e = nullptr;   // set by a successful begin()
    int n = 0;
    hipStream_t stream = nullptr;
};

// The workspaces a first call allocates: *ws = [max_inflight][bytes_per_slot], recorded in e->bufs; returns at once when *ws is
// set.  `zero` clears the new buffer and waits for that (the component-table scratch, the flow pyramid's census padding).  The caller of the _locked form holds e->mu.
int ensure_ws_locked(cart_engine *e, void **ws, size_t bytes_per_slot, bool zero);
template <typename T>
int ensure_ws(cart_engine *e, T **ws, size_t bytes_per_slot, bool zero = false) {
    std::lock_guard<std::mutex> lk(e->mu);
    return ensure_ws_locked(e, reinterpret_cast<void **>(ws), bytes_per_slot, zero);
}

// The lifecycle of the stateful device objects (cart_superpixels, cart_planefit, cart_orb).  An object keeps the device and
// geometry of the engine it was made on, not the engine, so that it may be destroyed after its engine.  Calls on one object are
// serialised by `mu` (superpixels.cu:97-99); a call that arrives on another stream than the previous one first waits for
// `done`, which every call records on its stream (ObjectCall).
struct DeviceObject {
    int device_id;
    Geometry g;
    std::mutex mu;
    hipEvent_t done = nullptr;
    hipStream_t last_stream = nullptr;
    bool used = false;
    std::vector<void *> bufs;   // every device allocation, freed by destroy_object

    explicit DeviceObject(const cart_engine *e) : device_id(e->params.device_id), g(e->g) {}
    // hipMalloc recorded in bufs; a zero-byte request gets a small real buffer (hipMalloc would hand back no pointer)
    template <typename T>
    int alloc(T **p, size_t bytes) {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), bytes ? bytes : 256));
        bufs.push_back(*p);
        return 0;
    }
    int create_event() {
        HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        return 0;
    }
};

// One entry point's hold on an object: begin() makes the object's device current, takes its lock and orders the call after
// the previous one if that came on another stream; once begin() has succeeded, every way out of the call, early error
// returns included, records `done` on the call's stream.
class ObjectCall {
   public:
    ObjectCall(DeviceObject &o, hipStream_t stream) : o(o), stream(stream) {}
    int begin() {
        HIP_TRY(hipSetDevice(o.device_id));
        lk = std::unique_lock<std::mutex>(o.mu);
        if (o.used && o.last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, o.done, 0));
        entered = true;
        return 0;
    }
    ~ObjectCall() {
        if (!entered) return;
        (void)hipEventRecord(o.done, stream);
        o.last_stream = stream;
        o.used = true;
    }

   private:
    DeviceObject &o;
    hipStream_t stream;
    std::unique_lock<std::mutex> lk;   // released after the record above
    bool entered = false;
};

// A device object made for frames of up to max_width x max_height (cart_dense_ego, cart_fusion).
struct SizedObject : DeviceObject {
    int max_width, max_height;
    SizedObject(const cart_engine *e, int max_width, int max_height) : DeviceObject(e), max_width(max_width), max_height(max_height) {}
    int check_fits(int w, int h) const;   // "width x height exceeds the object's W x H" (engine_checks.hip)
};

template <typename T>
void destroy_object(T *o) {
    if (!o) return;
    (void)hipSetDevice(o->device_id);   // the caller's current device may be another one
    (void)hipDeviceSynchronize();
    for (void *b : o->bufs) (void)hipFree(b);
    if (o->done) (void)hipEventDestroy(o->done);
    delete o;
}

}  // namespace cart_amd

#pragma GCC visibility pop

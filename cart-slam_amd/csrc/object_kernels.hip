// object_kernels.hip -- moving-object measurements and tracks from the motion components (spec S31; C ABI in
// engine_objects.hip).  One call is five launches:
//   object_select   workgroup 0 walks the component table in order (ballot + prefix per 256 entries) and numbers the selected entries;
//                   it writes each object's index into the scratch image at the component's id, which is how a pixel finds its object.
//                   Every workgroup clears a share of the histograms and accumulators.
//   object_hist     pass 1.  A lane walks kObjectHistStrip rows of one column and keeps one pending run of equal (object, bin) keys; when
//                   a lane's key changes, the wave merges the pending runs of neighbouring lanes with the same key (planemap_kernels.hip's
//                   wave_emit) and only the run heads issue an atomic: one per (wave, run), never one per pixel.
//   object_median   one wave per object: the cumulative histogram -> B_j and n_hist.
//   object_points   pass 2.  The same walk with the object as the key, so a lane's run stays open down its strip; the 24 dwords of a run
//                   (counts, minima, maxima, pixel box, six int64 sums) are merged across the wave the same way before the run heads
//                   issue one set of integer atomics.
//   object_tracks   one workgroup: the fp64 fields of every record, then the association (one thread per track slot, a parallel minimum
//                   per greedy round), the updates, the births in order, the outputs, and the scratch image back to -1.
// fp64 with + - * / floor only, in the association order of warp_device.h, which holds the warp chain.  The only atomics are integer
// additions, minima and maxima: exact in any order.

#include "engine_internal.h"
#include "warp_device.h"

namespace cart_amd {

namespace {

constexpr int kSelectBlocks = 64;

__device__ __forceinline__ long long quantise_point(double v) {   // Qp(v) = clamp(floor(1024 v + 0.5), -2147483647, 2147483647)
    const double q = floor(v * 1024.0 + 0.5);
    return (long long)(!(q > -2147483647.0) ? -2147483647.0 : (q > 2147483647.0 ? 2147483647.0 : q));
}

__device__ __forceinline__ cart_track free_track() {
    cart_track t;
    t.id = 0; t.state = 0; t.age = 0; t.missed = 0; t.object = -1; t.component = -1;
#pragma unroll
    for (int i = 0; i < 3; ++i) { t.position[i] = 0.0; t.velocity[i] = 0.0; t.extent[i] = 0.0; }
    return t;
}

__global__ __launch_bounds__(256) void object_reset_kernel(cart_track *tracks, int max_tracks, ObjectState *state) {
    if ((int)threadIdx.x < max_tracks) tracks[threadIdx.x] = free_track();
    if (threadIdx.x == 0) state->next_id = 1u;
}

__global__ __launch_bounds__(256) void object_select_kernel(ObjectArgs a) {
    const int gid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    for (int i = gid; i < a.max_objects * CART_OBJECT_BINS; i += gsz) a.hist[i] = 0;
    for (int j = gid; j < a.max_objects; j += gsz) {
        ObjectAcc z;
        z.n_points = 0; z.n_flow = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) { z.lo[i] = INT32_MAX; z.hi[i] = INT32_MIN; z.sum[i] = 0; z.flow_sum[i] = 0; }
        z.x0 = INT32_MAX; z.y0 = INT32_MAX; z.x1 = INT32_MIN; z.y1 = INT32_MIN;
        a.acc[j] = z;
    }
    if (blockIdx.x != 0) return;
    __shared__ int wave_total[4];
    const int n = min(max(*a.n_components, 0), a.max_components);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, npx = a.w * a.h;
    int base = 0;   // selected entries before this chunk: every thread keeps its own copy
    for (int k0 = 0; k0 < n; k0 += 256) {
        const int k = k0 + threadIdx.x;
        int id = -1, area = 0;
        bool sel = false;
        if (k < n) {
            id = a.table[k].id;
            area = a.table[k].area;
            sel = a.table[k].label == 1 && area >= a.p.min_area;
        }
        const unsigned long long votes = __ballot(sel);
        if (lane == 0) wave_total[wave] = __popcll(votes);
        __syncthreads();
        int j = base + __popcll(votes & ((1ull << lane) - 1ull));
        for (int v = 0; v < wave; ++v) j += wave_total[v];
        if (sel && j < a.max_objects) {
            a.objects[j].component = id;
            a.objects[j].area = area;
            if (id >= 0 && id < npx) a.slot_of[id] = j;
        }
        base += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.state->n_seen = n;
        a.state->n_selected = base;
        a.state->n_objects = min(base, a.max_objects);
    }
}

// the object of a component id, -1 for a pixel of none (UNKNOWN pixels, components that were not selected or have no table entry)
__device__ __forceinline__ int object_of(const ObjectArgs &a, int id) { return (id >= 0 && id < a.w * a.h) ? a.slot_of[id] : -1; }

// Wave-collective: the last lane of the run of equal keys this lane belongs to, and whether this lane is the run's head.
__device__ __forceinline__ int run_end(int key, bool &head) {
    const int lane = threadIdx.x & 63;
    const int below = __shfl_up(key, 1);
    head = lane == 0 || key != below;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    return above ? lane + __ffsll((long long)above) - 1 : 63;
}

__device__ __forceinline__ void wave_count(int32_t *hist, int key, unsigned cnt) {
    const int lane = threadIdx.x & 63;
    bool head;
    const int end = run_end(key, head);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned c = __shfl_down(cnt, d);
        if (lane + d <= end) cnt += c;
    }
    if (head && key >= 0) atomicAdd(hist + key, (int)cnt);
}

__global__ __launch_bounds__(256) void object_hist_kernel(ObjectArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y0 = blockIdx.y * kObjectHistStrip;
    int id[kObjectHistStrip], sc[kObjectHistStrip], obj[kObjectHistStrip];
#pragma unroll
    for (int r = 0; r < kObjectHistStrip; ++r) {   // every load of the strip before the first use
        const bool in = x < a.w && y0 + r < a.h;
        id[r] = in ? row_ptr(a.ids, a.ids_step, y0 + r)[x] : -1;
        sc[r] = in ? row_ptr(a.disp_cur, a.disp_cur_step, y0 + r)[x] : -32768;
    }
#pragma unroll
    for (int r = 0; r < kObjectHistStrip; ++r) obj[r] = object_of(a, id[r]);   // the gathers together
    int run = -1;
    unsigned cnt = 0;
#pragma unroll
    for (int r = 0; r < kObjectHistStrip; ++r) {
        const bool ok = obj[r] >= 0 && sc[r] != -32768 && (double)sc[r] / 16.0 >= a.p.min_disparity;
        const int key = ok ? obj[r] * CART_OBJECT_BINS + min(sc[r] >> 4, CART_OBJECT_BINS - 1) : -1;
        const bool flush = key >= 0 && run >= 0 && key != run;   // a pixel that does not count leaves the pending run open
        if (__any(flush)) wave_count(a.hist, flush ? run : -1, cnt);
        if (flush) cnt = 0;
        if (key >= 0) { run = key; ++cnt; }
    }
    if (__any(run >= 0)) wave_count(a.hist, run, cnt);
}

__global__ __launch_bounds__(64) void object_median_kernel(ObjectArgs a) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= a.state->n_objects) return;
    const int4 *bins = reinterpret_cast<const int4 *>(a.hist + (size_t)j * CART_OBJECT_BINS) + 2 * lane;   // 8 bins per lane
    const int4 b0 = bins[0], b1 = bins[1];
    const int v[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    int own = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) own += v[k];
    int incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, 63);
    const int target = (total + 1) >> 1;
    if (total == 0) {
        if (lane == 0) { a.median[2 * j] = -1; a.median[2 * j + 1] = 0; }
        return;
    }
    int cum = incl - own;
    if (cum < target && incl >= target) {   // exactly one lane: the cumulative count is monotone
        int B = 8 * lane;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cum += v[k];
            if (cum >= target) break;
            ++B;
        }
        a.median[2 * j] = B;
        a.median[2 * j + 1] = total;
    }
}

struct PointRun {   // what a lane holds for its open run: ObjectAcc in registers
    unsigned np, nf;
    int lo[3], hi[3], x0, y0, x1, y1;
    unsigned long long sum[3], fsum[3];
    __device__ __forceinline__ void clear() {
        np = 0; nf = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) { lo[i] = INT32_MAX; hi[i] = INT32_MIN; sum[i] = 0; fsum[i] = 0; }
        x0 = INT32_MAX; y0 = INT32_MAX; x1 = INT32_MIN; y1 = INT32_MIN;
    }
};

// Wave-collective: every lane brings a run (key = the object, or -1).  Neighbouring lanes with the same key form one run, the run's head
// lane gets its totals and issues the one set of atomics.
__device__ __forceinline__ void wave_points(ObjectAcc *acc, int key, PointRun p) {
    const int lane = threadIdx.x & 63;
    bool head;
    const int end = run_end(key, head);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const bool in = lane + d <= end;
        const unsigned np = __shfl_down(p.np, d), nf = __shfl_down(p.nf, d);
        const int x0 = __shfl_down(p.x0, d), y0 = __shfl_down(p.y0, d), x1 = __shfl_down(p.x1, d), y1 = __shfl_down(p.y1, d);
        if (in) { p.np += np; p.nf += nf; p.x0 = min(p.x0, x0); p.y0 = min(p.y0, y0); p.x1 = max(p.x1, x1); p.y1 = max(p.y1, y1); }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int lo = __shfl_down(p.lo[i], d), hi = __shfl_down(p.hi[i], d);
            const unsigned long long s = __shfl_down(p.sum[i], d), f = __shfl_down(p.fsum[i], d);
            if (in) { p.lo[i] = min(p.lo[i], lo); p.hi[i] = max(p.hi[i], hi); p.sum[i] += s; p.fsum[i] += f; }
        }
    }
    if (head && key >= 0 && p.np) {
        ObjectAcc *o = acc + key;
        atomicAdd(&o->n_points, p.np);
        atomicMin(&o->x0, p.x0); atomicMin(&o->y0, p.y0); atomicMax(&o->x1, p.x1); atomicMax(&o->y1, p.y1);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            atomicMin(&o->lo[i], p.lo[i]);
            atomicMax(&o->hi[i], p.hi[i]);
            atomicAdd(&o->sum[i], p.sum[i]);
        }
        if (p.nf) {
            atomicAdd(&o->n_flow, p.nf);
#pragma unroll
            for (int i = 0; i < 3; ++i) atomicAdd(&o->flow_sum[i], p.fsum[i]);
        }
    }
}

__global__ __launch_bounds__(256) void object_points_kernel(ObjectArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y0 = blockIdx.y * kObjectPointStrip;
    int id[kObjectPointStrip], sc[kObjectPointStrip], fl[kObjectPointStrip], obj[kObjectPointStrip], B[kObjectPointStrip];
#pragma unroll
    for (int r = 0; r < kObjectPointStrip; ++r) {   // every load of the strip before the first use
        const bool in = x < a.w && y0 + r < a.h;
        id[r] = in ? row_ptr(a.ids, a.ids_step, y0 + r)[x] : -1;
        sc[r] = in ? row_ptr(a.disp_cur, a.disp_cur_step, y0 + r)[x] : -32768;
        fl[r] = in ? reinterpret_cast<const int *>(row_ptr(a.flow, a.flow_step, y0 + r))[x] : 0;
    }
#pragma unroll
    for (int r = 0; r < kObjectPointStrip; ++r) obj[r] = object_of(a, id[r]);
#pragma unroll
    for (int r = 0; r < kObjectPointStrip; ++r) B[r] = obj[r] >= 0 ? a.median[2 * obj[r]] : -1;
    const int band16 = (int)floor(a.p.disparity_band * 16.0);
    bool point[kObjectPointStrip];
    int xp[kObjectPointStrip], yp[kObjectPointStrip], sp[kObjectPointStrip];
#pragma unroll
    for (int r = 0; r < kObjectPointStrip; ++r) {   // the gates of a point, then every gather of the strip before the first use
        const int off = sc[r] - (16 * B[r] + 8);
        point[r] = B[r] >= 0 && sc[r] != -32768 && (double)sc[r] / 16.0 >= a.p.min_disparity && (off < 0 ? -off : off) <= band16;
        const int2 prev = flow_previous(fl[r], x, y0 + r);
        xp[r] = prev.x;
        yp[r] = prev.y;
        const bool ok = point[r] && xp[r] >= 0 && xp[r] < a.w && yp[r] >= 0 && yp[r] < a.h;
        sp[r] = ok ? row_ptr(a.disp_prev, a.disp_prev_step, yp[r])[xp[r]] : -32768;
    }
    const double fxb = a.cam.fx * a.cam.baseline;
    const double speed2 = a.p.max_speed * a.p.max_speed;
    int run = -1;
    PointRun acc;
    acc.clear();
#pragma unroll
    for (int r = 0; r < kObjectPointStrip; ++r) {
        const int key = point[r] ? obj[r] : -1;
        const bool flush = key >= 0 && run >= 0 && key != run;   // a pixel that is no point leaves the pending run open
        if (__any(flush)) {
            PointRun none;
            none.clear();
            wave_points(a.acc, flush ? run : -1, flush ? acc : none);
        }
        if (flush) acc.clear();
        if (key < 0) continue;
        run = key;
        const int y = y0 + r;
        const WarpPoint P = back_project(a.cam, fxb, x, y, (double)sc[r] / 16.0);
        const double Pc[3] = {P.x, P.y, P.z};
        ++acc.np;
        acc.x0 = min(acc.x0, x); acc.y0 = min(acc.y0, y); acc.x1 = max(acc.x1, x); acc.y1 = max(acc.y1, y);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const long long q = quantise_point(Pc[i]);
            acc.sum[i] += (unsigned long long)q;
            acc.lo[i] = min(acc.lo[i], (int)q);
            acc.hi[i] = max(acc.hi[i], (int)q);
        }
        const double dp = (double)sp[r] / 16.0;
        if (sp[r] != -32768 && dp >= a.p.min_disparity) {   // gate 3 (a failed gate 2 left sp invalid)
            const WarpPoint q = pose_carry(a.rel, back_project(a.cam, fxb, xp[r], yp[r], dp));
            if (q.z > 0) {                                   // gate 4
                const double f[3] = {P.x - q.x, P.y - q.y, P.z - q.z};
                if ((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] <= speed2) {
                    ++acc.nf;
#pragma unroll
                    for (int i = 0; i < 3; ++i) acc.fsum[i] += (unsigned long long)quantise_point(f[i]);
                }
            }
        }
    }
    if (__any(run >= 0)) wave_points(a.acc, run, acc);
}

__global__ __launch_bounds__(256) void object_tracks_kernel(ObjectArgs a) {
    __shared__ double centroid[kObjectMaxObjects][3];
    __shared__ int obj_valid[kObjectMaxObjects], obj_track[kObjectMaxObjects];   // obj_track: the slot an object was matched to, -1 while free
    __shared__ double red_d2[256];
    __shared__ int red_t[256], red_o[256];
    __shared__ int slot_state[kObjectMaxTracks];
    const int tid = threadIdx.x;
    const int n_obj = a.state->n_objects;
    const int npx = a.w * a.h;
    // ---- the records
    {
        cart_object o = {};
        if (tid < n_obj) {
            const ObjectAcc acc = a.acc[tid];
            o.component = a.objects[tid].component;
            o.area = a.objects[tid].area;
            o.median_bin = a.median[2 * tid];
            o.n_hist = a.median[2 * tid + 1];
            o.n_points = (int)acc.n_points;
            o.n_flow = (int)acc.n_flow;
            o.x1 = -1; o.y1 = -1;
            if (acc.n_points) {
                o.x0 = acc.x0; o.y0 = acc.y0; o.x1 = acc.x1; o.y1 = acc.y1;
#pragma unroll
                for (int i = 0; i < 3; ++i) { o.lo[i] = acc.lo[i]; o.hi[i] = acc.hi[i]; }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) { o.sum[i] = (long long)acc.sum[i]; o.flow_sum[i] = (long long)acc.flow_sum[i]; }
            o.valid = o.n_points >= a.p.min_points;
            o.has_velocity = o.valid && o.n_flow >= a.p.min_points;
            if (o.valid) {
                WarpPoint c;
                c.x = ((double)o.sum[0] / 1024.0) / (double)o.n_points;
                c.y = ((double)o.sum[1] / 1024.0) / (double)o.n_points;
                c.z = ((double)o.sum[2] / 1024.0) / (double)o.n_points;
                const WarpPoint world = pose_carry(a.pose, c);
                o.centroid[0] = world.x; o.centroid[1] = world.y; o.centroid[2] = world.z;
#pragma unroll
                for (int i = 0; i < 3; ++i) o.extent[i] = (double)((long long)o.hi[i] - (long long)o.lo[i]) / 1024.0;
            }
            if (o.has_velocity) {
                double v[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) v[i] = ((double)o.flow_sum[i] / 1024.0) / (double)o.n_flow;
#pragma unroll
                for (int r = 0; r < 3; ++r) o.velocity[r] = (a.pose[4 * r] * v[0] + a.pose[4 * r + 1] * v[1]) + a.pose[4 * r + 2] * v[2];
            }
            if (o.component >= 0 && o.component < npx) a.slot_of[o.component] = -1;   // the scratch image goes back as it was found
        }
        if (tid < a.max_objects) {
            a.objects[tid] = o;
            if (a.objects_out) a.objects_out[tid] = o;
        }
        obj_valid[tid] = o.valid;
        obj_track[tid] = -1;
#pragma unroll
        for (int i = 0; i < 3; ++i) centroid[tid][i] = o.centroid[i];
    }
    // ---- the association: a thread per track slot
    cart_track t = tid < a.max_tracks ? a.tracks[tid] : free_track();
    const bool live = t.state != 0;
    double pred[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pred[i] = t.position[i] + t.velocity[i];
    const double gate2 = a.p.gate * a.p.gate;
    int match = -1, cand = -1;
    double cand_d2 = 0.0;
    bool rescan = live;
    __syncthreads();
    for (;;) {
        if (match < 0 && cand >= 0 && obj_track[cand] >= 0) rescan = true;   // the candidate went to another track
        if (rescan) {   // the nearest free object; objects only leave, so a candidate that is still free is still the nearest
            cand = -1;
            for (int o = 0; o < n_obj; ++o) {
                if (!obj_valid[o] || obj_track[o] >= 0) continue;
                const double dx = centroid[o][0] - pred[0], dy = centroid[o][1] - pred[1], dz = centroid[o][2] - pred[2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= gate2 && (cand < 0 || d2 < cand_d2)) { cand = o; cand_d2 = d2; }
            }
            rescan = false;
        }
        const bool bids = match < 0 && cand >= 0;
        red_d2[tid] = bids ? cand_d2 : 0.0;
        red_t[tid] = bids ? tid : INT32_MAX;
        red_o[tid] = cand;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {   // the smallest d2, ties to the smaller slot (a slot bids for one object: its smallest)
            if (tid < s) {
                const int ot = red_t[tid + s];
                const bool take = ot != INT32_MAX && (red_t[tid] == INT32_MAX || red_d2[tid + s] < red_d2[tid] || (red_d2[tid + s] == red_d2[tid] && ot < red_t[tid]));
                if (take) { red_d2[tid] = red_d2[tid + s]; red_t[tid] = ot; red_o[tid] = red_o[tid + s]; }
            }
            __syncthreads();
        }
        const int win_t = red_t[0], win_o = red_o[0];
        __syncthreads();   // everyone has read the winner before the next round's bids overwrite it
        if (win_t == INT32_MAX) break;
        if (tid == win_t) { match = win_o; obj_track[win_o] = tid; }
        __syncthreads();
    }
    // ---- the updates
    if (live) {
        if (match >= 0) {
            const cart_object &o = a.objects[match];   // written by this workgroup before the barrier above
            const double g = (double)a.p.gain_percent / 100.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double m = o.has_velocity ? o.velocity[i] : o.centroid[i] - t.position[i];
                t.velocity[i] = t.velocity[i] + g * (m - t.velocity[i]);
                t.position[i] = o.centroid[i];
                t.extent[i] = o.extent[i];
            }
            t.age += 1;
            t.missed = 0;
            t.object = match;
            t.component = o.component;
            t.state = t.age >= a.p.min_age ? 2 : 1;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) t.position[i] = pred[i];
            t.missed += 1;
            t.object = -1;
            t.component = -1;
            if (t.missed > a.p.max_missed) t = free_track();
        }
        a.tracks[tid] = t;
    }
    slot_state[tid] = tid < a.max_tracks ? t.state : -1;   // a slot past max_tracks is never free
    __syncthreads();
    // ---- the births in object order, and the counts
    if (tid == 0) {
        int n_valid = 0, n_matched = 0, n_born = 0, n_dropped = 0, n_live = 0, slot = 0;
        unsigned next_id = a.state->next_id;
        for (int o = 0; o < n_obj; ++o) {
            if (!obj_valid[o]) continue;
            ++n_valid;
            if (obj_track[o] >= 0) { ++n_matched; continue; }
            while (slot < a.max_tracks && slot_state[slot] != 0) ++slot;
            if (slot >= a.max_tracks) { ++n_dropped; continue; }
            const cart_object &ob = a.objects[o];
            cart_track b = free_track();
            b.id = next_id++;
            b.state = a.p.min_age <= 1 ? 2 : 1;
            b.age = 1;
            b.object = o;
            b.component = ob.component;
#pragma unroll
            for (int i = 0; i < 3; ++i) { b.position[i] = ob.centroid[i]; b.velocity[i] = ob.velocity[i]; b.extent[i] = ob.extent[i]; }
            a.tracks[slot] = b;
            slot_state[slot] = b.state;
            ++n_born;
        }
        for (int s = 0; s < a.max_tracks; ++s) n_live += slot_state[s] != 0;
        a.state->next_id = next_id;
        a.counts_out[0] = a.state->n_seen;
        a.counts_out[1] = a.state->n_selected;
        a.counts_out[2] = n_obj;
        a.counts_out[3] = n_valid;
        a.counts_out[4] = n_matched;
        a.counts_out[5] = n_born;
        a.counts_out[6] = n_dropped;
        a.counts_out[7] = n_live;
    }
    __syncthreads();
    if (tid < a.max_tracks) a.tracks_out[tid] = a.tracks[tid];
}

}  // namespace

void launch_object_reset(cart_track *tracks, int max_tracks, ObjectState *state, hipStream_t s) {
    hipLaunchKernelGGL(object_reset_kernel, dim3(1), dim3(256), 0, s, tracks, max_tracks, state);
}

void launch_object_update(const ObjectArgs &a, hipStream_t s) {
    const unsigned bx = (unsigned)((a.w + 255) / 256);
    hipLaunchKernelGGL(object_select_kernel, dim3(kSelectBlocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(object_hist_kernel, dim3(bx, (unsigned)((a.h + kObjectHistStrip - 1) / kObjectHistStrip)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(object_median_kernel, dim3((unsigned)a.max_objects), dim3(64), 0, s, a);
    hipLaunchKernelGGL(object_points_kernel, dim3(bx, (unsigned)((a.h + kObjectPointStrip - 1) / kObjectPointStrip)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(object_tracks_kernel, dim3(1), dim3(256), 0, s, a);
}

}  // namespace cart_amd

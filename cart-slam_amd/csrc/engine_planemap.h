// engine_planemap.h -- the cart_plane_store device object (spec S30), for the host translation units that read its ring: engine_planemap.hip,
// which owns it, and engine_voxelmap.hip (S35), whose rebuild integrates the stored frames.  Private to csrc/.
#pragma once

#include <algorithm>
#include <vector>

#include "engine_host.h"

extern "C" {

// S30: a ring of `capacity` frames of exactly w x h.  The id table and the insertion count are host state (guarded by mu).
struct cart_plane_store : cart_amd::DeviceObject {
    using cart_amd::DeviceObject::DeviceObject;
    int w = 0, h = 0, capacity = 0;
    int16_t *disp = nullptr;             // [capacity][h][w], packed
    uint8_t *planes = nullptr;           // [capacity][h][w], packed
    cart_amd::PlaneRevoteRecord *records = nullptr;   // device [kRevoteMaxEntries]: the entries of the rebuild in flight
    cart_amd::PlaneRevoteRecord *staging = nullptr;   // pinned host [kRevoteMaxEntries]: what the upload reads
    hipEvent_t uploaded = nullptr;       // recorded after every upload: the next rebuild waits for it before it rewrites `staging`
    bool staged = false;
    std::vector<uint64_t> ids;           // [capacity]: the frame_id of every slot
    uint64_t inserted = 0;               // since create / clear: insertion n went to slot n mod capacity
    int find(uint64_t id) const {        // newest first, so a repeated id names its latest insertion; -1 = not stored
        const uint64_t live = std::min<uint64_t>(inserted, (uint64_t)capacity);
        for (uint64_t k = 1; k <= live; ++k) {
            const int slot = (int)((inserted - k) % (uint64_t)capacity);
            if (ids[slot] == id) return slot;
        }
        return -1;
    }
};

}  // extern "C"

namespace cart_amd {

// The entries of a rebuild (S30, S35) into the store's device records on `stream`; the caller holds the store's ObjectCall.  Entries whose
// id the store does not hold (evicted or never inserted) are skipped; *used = the number that went up, in list order.  The previous
// rebuild's upload may still be reading the pinned records: the wait is for that copy alone, not for the stream.
inline int stage_rebuild_entries(cart_plane_store *s, const uint64_t *ids, const double *poses, int count, hipStream_t stream, int *used_out) {
    if (s->staged) HIP_TRY(hipEventSynchronize(s->uploaded));
    int used = 0;
    for (int k = 0; k < count; ++k) {
        const int slot = s->find(ids[k]);
        if (slot < 0) continue;
        PlaneRevoteRecord &r = s->staging[used++];
        r.slot = slot; r.pad = 0;
        std::memcpy(r.pose, poses + 12 * (size_t)k, sizeof(r.pose));
    }
    if (used) {
        HIP_TRY(hipMemcpyAsync(s->records, s->staging, sizeof(PlaneRevoteRecord) * (size_t)used, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(s->uploaded, stream));
        s->staged = true;
    }
    *used_out = used;
    return 0;
}

}  // namespace cart_amd

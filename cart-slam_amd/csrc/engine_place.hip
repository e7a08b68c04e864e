// engine_place.hip -- C ABI of the place recognition stage (include/cart_engine.h): argument checks and the
// cart_place_db device object, which owns the keyframe ring, the slot headers and the query's partial table.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

struct cart_place_db : DeviceObject {
    using DeviceObject::DeviceObject;
    PlaceStore store{};
    int32_t *partial = nullptr;          // [ceil(max_features / kPlaceRows)][capacity]
    uint64_t inserts = 0;                // since create / clear
    std::vector<uint8_t> taken;          // per slot: PlaceSlotHeader::flags as the host knows them (cart_place_slot)
};

void cart_place_default_params(cart_place_params *p) {
    if (!p) return;
    *p = cart_place_params{64, 80, 30, 4, 50};
}

int cart_place_create(cart_engine *e, int max_features, int capacity, cart_place_db **out) {
    if (max_features < 1 || max_features > CART_ORB_MAX_FEATURES) return fail("max_features must be in [1, 65536]");
    if (capacity < 1 || capacity > CART_PLACE_MAX_CAPACITY) return fail("capacity must be in [1, 1024]");
    if (!e || !out) return fail("bad arguments");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_place_db *db = new (std::nothrow) cart_place_db(e);
    if (!db) return fail("out of host memory");
    PlaceStore &s = db->store;
    s.max_features = max_features;
    s.capacity = capacity;
    db->taken.assign(capacity, 0);
    const size_t rows = (size_t)max_features * capacity;
    const size_t blocks = (max_features + kPlaceRows - 1) / kPlaceRows;
    if (db->alloc(&s.desc, rows * CART_ORB_DESCRIPTOR_BYTES) || db->alloc(&s.kp, rows * sizeof(cart_keypoint)) ||
        db->alloc(&s.landmarks, rows * 4 * sizeof(double)) || db->alloc(&s.hdr, (size_t)capacity * sizeof(PlaceSlotHeader)) ||
        db->alloc(&db->partial, blocks * capacity * sizeof(int32_t)) || db->create_event() ||
        hipMemset(s.hdr, 0, (size_t)capacity * sizeof(PlaceSlotHeader)) != hipSuccess) {
        destroy_object(db);
        return fail("allocating the place database failed");
    }
    *out = db;
    return 0;
}

void cart_place_destroy(cart_place_db *db) { destroy_object(db); }

int cart_place_clear(cart_place_db *db, void *stream_) {
    if (!db) return fail("bad arguments");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*db, stream);
    if (call.begin()) return -1;
    HIP_TRY(hipMemsetAsync(db->store.hdr, 0, (size_t)db->store.capacity * sizeof(PlaceSlotHeader), stream));
    db->inserts = 0;
    std::fill(db->taken.begin(), db->taken.end(), 0);
    return 0;
}

int cart_place_insert(cart_place_db *db, const uint8_t *desc, size_t desc_step, const cart_keypoint *kp, const double *landmarks,
                      const int32_t *count, uint64_t frame_id, int32_t *slot_out, void *stream_) {
    if (!db) return fail("bad arguments");
    if (!desc) return fail("desc is NULL");
    if (!kp) return fail("kp is NULL");
    if (!count) return fail("count is NULL");
    if (reinterpret_cast<uintptr_t>(kp) & 3) return fail("kp must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(landmarks) & 7) return fail("landmarks must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(count) & 3) return fail("count must be 4-byte aligned");
    if (desc_step < CART_ORB_DESCRIPTOR_BYTES) return fail("desc_step must be >= 32");
    PlaceInsertArgs a;
    std::memset(&a, 0, sizeof(a));
    a.db = db->store;
    a.desc = desc; a.desc_step = desc_step; a.kp = kp; a.landmarks = landmarks; a.count = count; a.frame_id = frame_id;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*db, stream);
    if (call.begin()) return -1;
    a.slot = (int)(db->inserts % (uint64_t)db->store.capacity);
    launch_place_insert(a, stream);
    HIP_TRY(hipGetLastError());
    db->inserts += 1;
    db->taken[a.slot] = (uint8_t)(kPlaceOccupied | (landmarks ? kPlaceHasLandmarks : 0));
    if (slot_out) *slot_out = a.slot;
    return 0;
}

int cart_place_query(cart_place_db *db, const cart_place_params *params, const uint8_t *q_desc, size_t q_step, const int32_t *q_count,
                     uint64_t frame_id, int32_t *scores, cart_place_candidate *candidates, int32_t *n_candidates, void *stream_) {
    if (!params) return fail("params is NULL");
    const cart_place_params &p = *params;
    if (p.max_distance < 0 || p.max_distance > 256) return fail("max_distance must be in [0, 256]");
    if (p.ratio < 0 || p.ratio > 100) return fail("ratio must be in [0, 100]");
    if (p.min_score < 0 || p.min_score > 65536) return fail("min_score must be in [0, 65536]");
    if (p.max_candidates < 1 || p.max_candidates > CART_PLACE_MAX_CANDIDATES) return fail("max_candidates must be in [1, 16]");
    if (!db) return fail("bad arguments");
    if (!q_desc) return fail("q_desc is NULL");
    if (!q_count) return fail("q_count is NULL");
    if (!candidates) return fail("candidates is NULL");
    if (!n_candidates) return fail("n_candidates is NULL");
    if (reinterpret_cast<uintptr_t>(q_count) & 3) return fail("q_count must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(scores) & 3) return fail("scores must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(candidates) & 7) return fail("candidates must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(n_candidates) & 3) return fail("n_candidates must be 4-byte aligned");
    if (q_step < CART_ORB_DESCRIPTOR_BYTES) return fail("q_step must be >= 32");
    const PlaceStore &s = db->store;
    struct Range { const char *name; uintptr_t b, e; };
    const uintptr_t qb = reinterpret_cast<uintptr_t>(q_desc);
    const Range in[] = {{"q_desc", qb, qb + (size_t)(s.max_features - 1) * q_step + CART_ORB_DESCRIPTOR_BYTES},
                        {"q_count", reinterpret_cast<uintptr_t>(q_count), reinterpret_cast<uintptr_t>(q_count) + sizeof(int32_t)}};
    const Range outs[] = {{"scores", reinterpret_cast<uintptr_t>(scores), reinterpret_cast<uintptr_t>(scores) + (size_t)s.capacity * sizeof(int32_t)},
                          {"candidates", reinterpret_cast<uintptr_t>(candidates), reinterpret_cast<uintptr_t>(candidates) + (size_t)p.max_candidates * sizeof(cart_place_candidate)},
                          {"n_candidates", reinterpret_cast<uintptr_t>(n_candidates), reinterpret_cast<uintptr_t>(n_candidates) + sizeof(int32_t)}};
    for (const Range &o : outs) {
        if (!o.b) continue;   // scores may be NULL
        for (const Range &i : in)
            if (o.b < i.e && i.b < o.e) return fail(std::string(o.name) + " and " + i.name + " must not overlap");
        for (const Range &o2 : outs)
            if (&o2 < &o && o2.b && o.b < o2.e && o2.b < o.e) return fail(std::string(o2.name) + " and " + o.name + " must not overlap");
    }
    PlaceQueryArgs a;
    std::memset(&a, 0, sizeof(a));
    a.db = s;
    a.p = p;
    a.q_desc = q_desc; a.q_step = q_step; a.q_count = q_count; a.frame_id = frame_id;
    a.partial = db->partial; a.scores = scores; a.candidates = candidates; a.n_candidates = n_candidates;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*db, stream);
    if (call.begin()) return -1;
    launch_place_query(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_place_slot(cart_place_db *db, int slot, const uint8_t **desc, const cart_keypoint **kp, const double **landmarks, const int32_t **count) {
    if (!db) return fail("bad arguments");
    const PlaceStore &s = db->store;
    if (slot < 0 || slot >= s.capacity) return fail("slot must be in [0, " + std::to_string(s.capacity - 1) + "]");
    std::lock_guard<std::mutex> lk(db->mu);
    if (!db->taken[slot]) return fail("slot " + std::to_string(slot) + " holds no frame");
    const size_t row = (size_t)slot * s.max_features;
    if (desc) *desc = s.desc + row * CART_ORB_DESCRIPTOR_BYTES;
    if (kp) *kp = s.kp + row;
    if (landmarks) *landmarks = (db->taken[slot] & kPlaceHasLandmarks) ? s.landmarks + 4 * row : nullptr;
    if (count) *count = &s.hdr[slot].count;
    return 0;
}

}  // extern "C"

// engine_match.hip -- C ABI of the ORB descriptor matcher (include/cart_engine.h): argument checks and the
// cart_matcher device object.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

struct cart_matcher : DeviceObject {
    using DeviceObject::DeviceObject;
    int max_features = 0, chunk_len = 0, chunks = 0;
    int2 *fwd_part = nullptr;      // [chunks][max_features]
    int32_t *bwd_part = nullptr;   // [chunks][max_features]
    int4 *fwd = nullptr;           // [max_features]
    int32_t *bwd = nullptr;        // [max_features]
};

void cart_match_default_params(cart_match_params *p) {
    if (!p) return;
    *p = cart_match_params{0, 0.f, 0.f, 0.f, 0.f, -1, 64, 80, 1};
}

int cart_matcher_create(cart_engine *e, int max_features, cart_matcher **out) {
    if (!e || !out) return fail("bad arguments");
    if (max_features < 1 || max_features > CART_ORB_MAX_FEATURES) return fail("max_features must be in [1, 65536]");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_matcher *m = new (std::nothrow) cart_matcher(e);
    if (!m) return fail("out of host memory");
    m->max_features = max_features;
    const int tiles = (max_features + kMatchTile - 1) / kMatchTile;
    m->chunk_len = kMatchTile * ((tiles + kMatchMaxChunks - 1) / kMatchMaxChunks);   // one tile per chunk up to 8192 features
    m->chunks = (max_features + m->chunk_len - 1) / m->chunk_len;
    const size_t part = (size_t)m->chunks * max_features;
    if (m->alloc(&m->fwd_part, part * sizeof(int2)) || m->alloc(&m->bwd_part, part * sizeof(int32_t)) ||
        m->alloc(&m->fwd, (size_t)max_features * sizeof(int4)) || m->alloc(&m->bwd, (size_t)max_features * sizeof(int32_t)) || m->create_event()) {
        destroy_object(m);
        return fail("allocating the matcher workspaces failed");
    }
    *out = m;
    return 0;
}

void cart_matcher_destroy(cart_matcher *m) { destroy_object(m); }

int cart_matcher_match(cart_matcher *m, const cart_match_params *params, const uint8_t *q_desc, size_t q_step, const cart_keypoint *q_kp,
                       const int32_t *q_count, const uint8_t *t_desc, size_t t_step, const cart_keypoint *t_kp, const int32_t *t_count,
                       cart_match *matches, int32_t *match_count, int32_t *forward, void *stream_) {
    if (!m) return fail("matcher is NULL");
    if (!params) return fail("params is NULL");
    if (!q_desc || !t_desc || !q_count || !t_count || !matches || !match_count) return fail("NULL pointer");
    if (q_step < CART_ORB_DESCRIPTOR_BYTES || t_step < CART_ORB_DESCRIPTOR_BYTES) return fail("descriptor step must be >= 32");
    const cart_match_params &p = *params;
    if (p.use_gate != 0 && p.use_gate != 1) return fail("use_gate must be 0 or 1");
    if (p.cross_check != 0 && p.cross_check != 1) return fail("cross_check must be 0 or 1");
    if (p.max_distance < 0 || p.max_distance > 256) return fail("max_distance must be in [0, 256]");
    if (p.ratio < 0 || p.ratio > 100) return fail("ratio must be in [0, 100]");
    if (p.use_gate && (!q_kp || !t_kp)) return fail("the gate needs the keypoints of both sets");
    if ((reinterpret_cast<uintptr_t>(q_kp) | reinterpret_cast<uintptr_t>(t_kp) | reinterpret_cast<uintptr_t>(q_count) | reinterpret_cast<uintptr_t>(t_count) |
         reinterpret_cast<uintptr_t>(matches) | reinterpret_cast<uintptr_t>(match_count) | reinterpret_cast<uintptr_t>(forward)) & 3)
        return fail("keypoints, counts and outputs must be 4-byte aligned");
    MatchArgs a;
    std::memset(&a, 0, sizeof(a));
    a.p = p;
    a.q_desc = q_desc; a.q_step = q_step; a.q_kp = q_kp; a.q_count = q_count;
    a.t_desc = t_desc; a.t_step = t_step; a.t_kp = t_kp; a.t_count = t_count;
    a.cap = m->max_features; a.chunk_len = m->chunk_len;
    a.fwd_part = m->fwd_part; a.bwd_part = m->bwd_part; a.fwd = m->fwd; a.bwd = m->bwd;
    a.matches = matches; a.match_count = match_count; a.forward = forward;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*m, stream);
    if (call.begin()) return -1;
    launch_match(a, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

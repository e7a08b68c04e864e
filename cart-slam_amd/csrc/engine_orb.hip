// engine_orb.hip -- C ABI of the ORB features (include/cart_engine.h): level layout and steered pattern on the
// host, the cart_orb device object.

#include "engine_host.h"

using namespace cart_amd;

extern "C" {

// ---- ORB features ----
namespace {
struct OrbLayout {
    int n_levels = 0;
    int w[kOrbLevels], h[kOrbLevels], n[kOrbLevels];
    double s[kOrbLevels];
};
// Level sizes, scales and quotas (S20): doubles and rint only, no libm transcendentals.
void orb_layout(int width, int height, int nfeatures, OrbLayout &L) {
    L = OrbLayout();
    double s = 1.0;
    bool built = true;
    for (int l = 0; l < kOrbLevels; ++l) {
        L.s[l] = s;
        L.w[l] = (int)std::nearbyint((double)width / s);
        L.h[l] = (int)std::nearbyint((double)height / s);
        built = built && L.w[l] >= 2 * kOrbEdge + 1 && L.h[l] >= 2 * kOrbEdge + 1;
        if (built) L.n_levels = l + 1;
        s *= 1.2;
    }
    const double f = 1.0 / 1.2;
    double f8 = 1.0;
    for (int l = 0; l < kOrbLevels; ++l) f8 *= f;
    double nd = (double)nfeatures * (1.0 - f) / (1.0 - f8);
    int sum = 0;
    for (int l = 0; l < kOrbLevels - 1; ++l) {
        L.n[l] = std::min((int)std::nearbyint(nd), nfeatures - sum);
        sum += L.n[l];
        nd *= f;
    }
    L.n[kOrbLevels - 1] = nfeatures - sum;
}
uint64_t orb_mix(uint64_t z) {   // S17's splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
int orb_rnd20(long long v) { return (int)(v < 0 ? -((-v + (1LL << 19)) >> 20) : ((v + (1LL << 19)) >> 20)); }
// The 256 pairs (S20: stream(0, 3, i, attempt, 0), 16 draws, index rule of S17) steered to the 30 bins: [30][256] char4.
void orb_steered_pattern(std::vector<char4> &out) {
    static const int kSteer[15][2] = {{1048576, 0}, {1025662, 218011}, {957922, 426494}, {848316, 616338}, {701634, 779244},
                                      {524288, 908093}, {324028, 997255}, {109606, 1042832}, {-109606, 1042832}, {-324028, 997255},
                                      {-524288, 908093}, {-701634, 779244}, {-848316, 616338}, {-957922, 426494}, {-1025662, 218011}};
    int pat[256][4];
    for (uint64_t i = 0; i < 256; ++i)
        for (uint64_t a = 0;; ++a) {
            const uint64_t st = orb_mix(orb_mix(orb_mix(orb_mix(0 ^ 3) ^ i) ^ a) ^ 0);
            int v[4];
            for (int t = 0; t < 4; ++t) {
                int sum = 0;
                for (int d = 0; d < 4; ++d) sum += (int)(((orb_mix(st + (uint64_t)(4 * t + d)) >> 32) * 27ull) >> 32);
                v[t] = (sum + 2) / 4 - 13;
            }
            if (v[0] != v[2] || v[1] != v[3]) {
                for (int t = 0; t < 4; ++t) pat[i][t] = v[t];
                break;
            }
        }
    out.assign(30 * 256, char4());
    for (int k = 0; k < 30; ++k) {
        const long long C = k < 15 ? kSteer[k][0] : -kSteer[k - 15][0], S = k < 15 ? kSteer[k][1] : -kSteer[k - 15][1];
        for (int i = 0; i < 256; ++i) {
            int r[4];
            for (int t = 0; t < 4; t += 2) {
                const long long x = pat[i][t], y = pat[i][t + 1];
                r[t] = orb_rnd20(x * C - y * S);
                r[t + 1] = orb_rnd20(x * S + y * C);
            }
            out[k * 256 + i] = make_char4((signed char)r[0], (signed char)r[1], (signed char)r[2], (signed char)r[3]);
        }
    }
}
int orb_cap(int w, int h) {   // strict NMS: at most one survivor per 2x2 block of the candidate region
    const int iw = w - 2 * kOrbEdge, ih = h - 2 * kOrbEdge;
    return (iw > 0 && ih > 0) ? ((iw + 1) / 2) * ((ih + 1) / 2) : 0;
}
}  // namespace

struct cart_orb : DeviceObject {
    using DeviceObject::DeviceObject;
    int max_w = 0, max_h = 0, nfeatures = 0;
    size_t pyr_off[kOrbLevels] = {}, cand_off[kOrbLevels] = {};
    int cap[kOrbLevels] = {};
    size_t pyr_stride = 0, cand_stride = 0;
    uint8_t *pyr = nullptr;        // [2][pyr_stride]
    OrbCand *cand = nullptr;       // [2][cand_stride]
    int32_t *cand_cnt = nullptr;   // [2][8]
    OrbCand *sel = nullptr;        // [2][nfeatures]
    int4 *kpi = nullptr;           // [2][nfeatures] (x_l, y_l, level, response bits)
    char4 *pattern = nullptr;      // [30][256]
    OrbLayout last;                // of the last detect call
    int last_images = 0;
};

int cart_orb_levels(int width, int height, int nfeatures, int *level_w, int *level_h, int *level_n) {
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return fail("width / height must be in [1, 16384]");
    if (nfeatures < 1 || nfeatures > CART_ORB_MAX_FEATURES) return fail("nfeatures must be in [1, 65536]");
    OrbLayout L;
    orb_layout(width, height, nfeatures, L);
    for (int l = 0; l < kOrbLevels; ++l) {
        if (level_w) level_w[l] = L.w[l];
        if (level_h) level_h[l] = L.h[l];
        if (level_n) level_n[l] = L.n[l];
    }
    return L.n_levels;
}

int cart_orb_create(cart_engine *e, int max_width, int max_height, int nfeatures, cart_orb **out) {
    if (!e || !out) return fail("bad arguments");
    if (max_width < 1 || max_height < 1 || max_width > 16384 || max_height > 16384) return fail("max_width / max_height must be in [1, 16384]");
    if (nfeatures < 1 || nfeatures > CART_ORB_MAX_FEATURES) return fail("nfeatures must be in [1, 65536]");
    HIP_TRY(hipSetDevice(e->params.device_id));
    cart_orb *o = new (std::nothrow) cart_orb(e);
    if (!o) return fail("out of host memory");
    o->max_w = max_width; o->max_h = max_height; o->nfeatures = nfeatures;
    OrbLayout L;
    orb_layout(max_width, max_height, nfeatures, L);
    for (int l = 0; l < L.n_levels; ++l) {   // sizes only shrink with the image, so the create-size layout holds every call
        o->pyr_off[l] = o->pyr_stride;
        o->pyr_stride += ((size_t)L.w[l] * L.h[l] + 255) & ~(size_t)255;
        o->cap[l] = orb_cap(L.w[l], L.h[l]);
        o->cand_off[l] = o->cand_stride;
        o->cand_stride += (size_t)o->cap[l];
    }
    std::vector<char4> pat;
    orb_steered_pattern(pat);
    if (o->alloc(&o->pyr, 2 * o->pyr_stride) || o->alloc(&o->cand, 2 * o->cand_stride * sizeof(OrbCand)) ||   // both 0 when no level is built
        o->alloc(&o->cand_cnt, 2 * kOrbLevels * 4) || o->alloc(&o->sel, 2 * (size_t)nfeatures * sizeof(OrbCand)) ||
        o->alloc(&o->kpi, 2 * (size_t)nfeatures * sizeof(int4)) || o->alloc(&o->pattern, pat.size() * sizeof(char4)) ||
        hipMemcpy(o->pattern, pat.data(), pat.size() * sizeof(char4), hipMemcpyHostToDevice) != hipSuccess || o->create_event()) {
        destroy_object(o);
        return fail("allocating the ORB workspaces failed");
    }
    *out = o;
    return 0;
}

void cart_orb_destroy(cart_orb *o) { destroy_object(o); }

int cart_orb_detect(cart_orb *o, int n_images, const uint8_t *const *images, const size_t *steps, int channels, int width, int height,
                    cart_keypoint *const *keypoints, uint8_t *const *descriptors, const size_t *descriptor_steps, int32_t *counts, void *stream_) {
    if (!o) return fail("orb is NULL");
    if (n_images != 1 && n_images != 2) return fail("n_images must be 1 or 2");
    if (!images || !steps || !keypoints || !descriptors || !counts) return fail("NULL pointer");
    if (channels != 1 && channels != 3) return fail("channels must be 1 or 3");
    if (width < 1 || height < 1 || width > o->max_w || height > o->max_h) return fail("image size outside [1, create size]");
    OrbOut out;
    std::memset(&out, 0, sizeof(out));
    out.channels = channels;
    out.counts = counts;
    for (int i = 0; i < n_images; ++i) {
        if (!images[i] || !keypoints[i] || !descriptors[i]) return fail("NULL image / output pointer");
        if (steps[i] < (size_t)width * channels) return fail("bad step");
        if (reinterpret_cast<uintptr_t>(keypoints[i]) & 3) return fail("keypoints must be 4-byte aligned");
        out.src[i] = images[i]; out.src_step[i] = steps[i];
        out.kp[i] = keypoints[i]; out.desc[i] = descriptors[i];
        out.desc_step[i] = descriptor_steps ? descriptor_steps[i] : CART_ORB_DESCRIPTOR_BYTES;
        if (out.desc_step[i] < CART_ORB_DESCRIPTOR_BYTES) return fail("descriptor step must be >= 32");
    }
    OrbLayout L;
    orb_layout(width, height, o->nfeatures, L);
    OrbPlan p;
    std::memset(&p, 0, sizeof(p));
    p.n_images = n_images; p.n_levels = L.n_levels; p.nfeatures = o->nfeatures;
    p.pyr_stride = o->pyr_stride; p.cand_stride = o->cand_stride;
    for (int l = 0; l < L.n_levels; ++l) {
        OrbLevel &v = p.lev[l];
        v.w = L.w[l]; v.h = L.h[l];
        v.tiles_x = (L.w[l] - 2 * kOrbEdge + kOrbTileW - 1) / kOrbTileW;
        v.tile0 = p.total_tiles;
        p.total_tiles += v.tiles_x * ((L.h[l] - 2 * kOrbEdge + kOrbTileH - 1) / kOrbTileH);
        v.quota = L.n[l];
        v.cap = o->cap[l];
        v.pyr_off = o->pyr_off[l]; v.cand_off = o->cand_off[l];
        if (l > 0) {
            v.fx = (float)((double)L.w[l - 1] / (double)L.w[l]);
            v.fy = (float)((double)L.h[l - 1] / (double)L.h[l]);
        }
        v.scale = (float)L.s[l];
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*o, stream);
    if (call.begin()) return -1;
    o->last = L;
    o->last_images = n_images;
    if (L.n_levels == 0) {   // no level is large enough: no keypoints
        HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_images * 4, stream));
        return 0;
    }
    for (int l = 0; l < L.n_levels; ++l) launch_orb_pyramid_level(p, l, out, o->pyr, stream);
    HIP_TRY(hipMemsetAsync(o->cand_cnt, 0, 2 * kOrbLevels * 4, stream));
    launch_orb_detect(p, o->pyr, o->cand, o->cand_cnt, stream);
    launch_orb_select(p, o->cand, o->cand_cnt, o->sel, o->kpi, counts, stream);
    launch_orb_describe(p, o->pyr, o->kpi, o->pattern, out, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cart_orb_debug_level(cart_orb *o, int image, int level, uint8_t *dst, size_t dst_step, int32_t *n_candidates, void *stream_) {
    if (!o) return fail("orb is NULL");
    if (image < 0 || image >= o->last_images) return fail("image not part of the last detect call");
    if (level < 0 || level >= o->last.n_levels) return fail("level not built by the last detect call");
    const int w = o->last.w[level], h = o->last.h[level];
    if (dst && dst_step < (size_t)w) return fail("bad step");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ObjectCall call(*o, stream);
    if (call.begin()) return -1;
    if (dst) HIP_TRY(hipMemcpy2DAsync(dst, dst_step, o->pyr + (size_t)image * o->pyr_stride + o->pyr_off[level], (size_t)w, (size_t)w, (size_t)h,
                                      hipMemcpyDeviceToDevice, stream));
    if (n_candidates) {
        HIP_TRY(hipMemcpyAsync(n_candidates, o->cand_cnt + image * kOrbLevels + level, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return 0;
}

}  // extern "C"

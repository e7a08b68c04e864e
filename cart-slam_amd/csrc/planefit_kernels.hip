// planefit_kernels.hip -- superpixel plane fitting for gfx950.
//
// What the reference does (read as text, nothing copied):
//   SuperPixelPlaneFitModule::runInternal    src/modules/planefit.cu:357-445   labels + depth downloaded every frame,
//   SuperPixelPlaneClusterModule             src/modules/planecluster.cpp:19-177  per-label point lists on the host,
//   segmentPlane / getPlaneFromPoints        src/utils/plane.cpp:56-180         Open3D-style RANSAC under OpenMP with a
//                                                                              std::random_device sampler;
//   attemptAssignment                        src/modules/planefit.cu:223-327    two blocking host syncs per iteration.
//
// MI355X design: everything per pixel and per point runs here, nothing is downloaded until planefit's outputs.
//   pf_hist_kernel      one wave per 1024-pixel raster tile (all its loads issued first): per-label counts of all / invalid pixels (integer atomics,
//                       one per label run of a 64-pixel chunk) and the tile's count of valid points per label
//   pf_colscan_kernel   per label: exclusive prefix of the tile counts (tile order) and the label's point count
//   pf_scan_kernel      one workgroup: exclusive prefix over labels -> start of every label's point list
//   pf_scatter_kernel   the same tile walk again; a label run's points go to start + tile prefix + rank in the run:
//                       a stable counting sort, i.e. raster order inside every label (no atomics-ordered scatter)
//   pf_ransac_kernel    one wave per label (S17): points staged in LDS, lane j owns hypotheses j and j + 64 (sampling,
//                       4-point fit, inlier count + integer qerr over all points), wave arg-max, then the refit with
//                       lane j summing inliers j, j + 64, ... and a butterfly (the order the spec fixes)
//   pf_adj_*            8-neighbour label sets: a bitmap [label][label] (atomic OR: order independent), popcounts,
//                       prefix, CSR fill in ascending label order
//   pf_fit_*            the S19 loop on the device: state in device memory, one inlier launch and one decide+sample
//                       launch per iteration; iterations after termination are no-ops.
// All plane arithmetic is IEEE double in the spec's operation order, no FMA contraction.
#include "engine_internal.h"

#pragma clang fp contract(off)

namespace cart_amd {

namespace {

__device__ inline uint64_t pf_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline uint64_t pf_stream(uint64_t seed, uint64_t tag, uint64_t a, uint64_t b, uint64_t c) {
    return pf_mix(pf_mix(pf_mix(pf_mix(seed ^ tag) ^ a) ^ b) ^ c);
}
__device__ inline uint32_t pf_uniform(uint64_t s, uint64_t c, uint32_t n) {
    return (uint32_t)(((pf_mix(s + c) >> 32) * (uint64_t)n) >> 32);
}

__device__ inline bool pf_valid(float z, int pred) {
    if (pred == CART_PLANE_PREDICATE_PLANEFIT) return isfinite(z) && z <= 40.0f && z > 0.0f;   // IS_VALID_DEPTH (planefit.cu:20)
    return !(z <= 0.0f || z > 40.0f);                                                            // planecluster.cpp:35 (NaN kept)
}

__device__ inline uint64_t lanemask_lt() { return (1ull << (threadIdx.x & 63u)) - 1ull; }

// getPlaneFromPoints after the sums (plane.cpp:76-95): determinant branch order, Vec /= norm as a multiply by 1/norm.
__device__ inline void plane_from_moments(double cx, double cy, double cz, double xx, double xy, double xz, double yy, double yz,
                                          double zz, double out[4]) {
    const double detX = yy * zz - yz * yz, detY = xx * zz - xz * xz, detZ = xx * yy - xy * xy;
    if (detX <= 0 && detY <= 0 && detZ <= 0) { out[0] = out[1] = out[2] = out[3] = 0.0; return; }
    double a, b, c;
    if (detX > detY && detX > detZ) { a = detX; b = xz * yz - xy * zz; c = xy * yz - xz * yy; }
    else if (detY > detZ) { a = xz * yz - xy * zz; b = detY; c = xy * xz - yz * xx; }
    else { a = xy * yz - xz * yy; b = xy * xz - yz * xx; c = detZ; }
    const double inv = 1.0 / sqrt((a * a + b * b) + c * c);
    a *= inv; b *= inv; c *= inv;
    out[0] = a; out[1] = b; out[2] = c; out[3] = -((a * cx + b * cy) + c * cz);
}

constexpr int kPfTile = 1024;        // pixels per raster tile (16 chunks of 64): ~455 waves at 1242x375
constexpr int kPfStage = 1024;       // points of one label staged in LDS (larger labels read global memory)
constexpr int kPfHyps = 100;         // plane.hpp:7-12
constexpr int kPfMinPoints = 16;
constexpr double kPfFitThr = 0.02;   // planefit.cu:433

struct TileArgs {
    const uint16_t *labels; size_t lstep;
    const float *xyz; size_t xstep;
    int w, h, L1, pred, ntiles;
    int32_t *cursor;     // [ntiles][L1]
    int32_t *cnt;        // [L1][2] all, invalid
    const int32_t *start;
    float4 *pts;
    int32_t *err, *lp_err;   // label out of range: the status word and the word cart_planefit_fit reads
};

// One wave walks tile t chunk by chunk and handles the chunk label run by label run (ballot of the lanes that share the
// first pending lane's label): counts (kScatter = false) or the stable scatter of the run's valid points (kScatter = true).
template <bool kScatter>
__global__ __launch_bounds__(256) void pf_tile_kernel(TileArgs a) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.ntiles) return;
    const long npx = (long)a.w * a.h;
    constexpr int kChunks = kPfTile / 64;
    // all loads of the tile first (one round trip instead of one per chunk), then the chunks in raster order
    int lab[kChunks];
    float x[kChunks], y[kChunks], z[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const long p = (long)t * kPfTile + c * 64 + lane;
        lab[c] = -1; x[c] = y[c] = z[c] = 0.f;
        if (p < npx) {
            const int py = (int)(p / a.w), px = (int)(p - (long)py * a.w);
            lab[c] = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(a.labels) + py * a.lstep + px * 2);
            const float *q = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(a.xyz) + py * a.xstep) + px * 3;
            x[c] = q[0]; y[c] = q[1]; z[c] = q[2];
        }
    }
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        bool act = lab[c] >= 0;
        if (act && lab[c] >= a.L1) { act = false; if (!kScatter) { atomicOr(a.err, 1); atomicOr(a.lp_err, 1); } }
        const bool val = act && pf_valid(z[c], a.pred);
        uint64_t pending = __ballot(act);
        const uint64_t vmask = __ballot(val);
        while (pending) {
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const int l = __shfl(lab[c], leader);
            const uint64_t run = __ballot(act && lab[c] == l);
            const uint64_t vrun = run & vmask;
            if (!kScatter) {
                if (lane == leader) {
                    atomicAdd(&a.cnt[2 * l], __popcll(run));
                    atomicAdd(&a.cnt[2 * l + 1], __popcll(run) - __popcll(vrun));
                    if (vrun) atomicAdd(&a.cursor[(size_t)t * a.L1 + l], __popcll(vrun));
                }
            } else if (vrun) {
                int old = 0;
                if (lane == leader) old = atomicAdd(&a.cursor[(size_t)t * a.L1 + l], __popcll(vrun));   // only this wave owns row t
                old = __shfl(old, leader);
                if ((vrun >> lane) & 1ull) {
                    const int dst = a.start[l] + old + __popcll(vrun & lanemask_lt());
                    a.pts[dst] = make_float4(x[c], y[c], z[c], 0.f);
                }
            }
            pending &= ~run;
        }
    }
}

__global__ __launch_bounds__(256) void pf_colscan_kernel(int32_t *cursor, int ntiles, int L1, int32_t *npts) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= L1) return;
    int run = 0;
    int t = 0;
    for (; t + 8 <= ntiles; t += 8) {   // eight independent loads in flight
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = cursor[(size_t)(t + k) * L1 + l];
#pragma unroll
        for (int k = 0; k < 8; ++k) { cursor[(size_t)(t + k) * L1 + l] = run; run += v[k]; }
    }
    for (; t < ntiles; ++t) {
        const int v = cursor[(size_t)t * L1 + l];
        cursor[(size_t)t * L1 + l] = run;
        run += v;
    }
    npts[l] = run;
}

// exclusive prefix of n <= 16384 counts -> out[0..n], one workgroup of 1024
__global__ __launch_bounds__(1024) void pf_scan_kernel(const int32_t *in, int n, int32_t *out) {
    __shared__ int part[1024];
    const int per = (n + 1023) / 1024, b = threadIdx.x * per;
    int s = 0;
    for (int i = 0; i < per; ++i) if (b + i < n) s += in[b + i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = 0; i < per; ++i) if (b + i < n) { out[b + i] = run; run += in[b + i]; }
    if (threadIdx.x == 1023) out[n] = part[1023];
}

struct RansacArgs {
    const float4 *pts; const int32_t *start; const int32_t *npts;
    int L1; double thr;
    uint64_t seed, frame;
    double *planes;    // [L1][4]
};

__device__ inline double4 ld_pt(const float4 *P, int i) { const float4 q = P[i]; return make_double4(q.x, q.y, q.z, 0.0); }

__global__ __launch_bounds__(64) void pf_ransac_kernel(RansacArgs a) {
    __shared__ float4 stage[kPfStage];
    __shared__ double slot[64][3];
    const int l = blockIdx.x, lane = threadIdx.x;
    const int n = a.npts[l];
    double *out = a.planes + (size_t)l * 4;
    if (n < kPfMinPoints) { if (lane < 4) out[lane] = 0.0; return; }
    const float4 *src = a.pts + a.start[l];
    const float4 *P = src;
    if (n <= kPfStage) {
        for (int i = lane; i < n; i += 64) stage[i] = src[i];
        __syncthreads();
        P = stage;
    }
    const double thr = a.thr, thr2 = thr * thr;
    // ---- hypotheses: lane owns h = lane and h = lane + 64 ----
    int bcnt = 0, bh = kPfHyps;
    unsigned long long bq = 0;
    double bpl[4] = {0, 0, 0, 0};
    for (int h = lane; h < kPfHyps; h += 64) {
        const uint64_t s = pf_stream(a.seed, 1, a.frame, (uint64_t)l, (uint64_t)h);
        int idx[4], k = 0;
        for (uint64_t c = 0; k < 4; ++c) {
            const int i = (int)pf_uniform(s, c, (uint32_t)n);
            bool dup = false;
            for (int j = 0; j < k; ++j) dup |= idx[j] == i;
            if (!dup) idx[k++] = i;
        }
        double sx = 0, sy = 0, sz = 0;
        for (int j = 0; j < 4; ++j) { const double4 p = ld_pt(P, idx[j]); sx += p.x; sy += p.y; sz += p.z; }
        const double cx = sx / 4.0, cy = sy / 4.0, cz = sz / 4.0;
        double xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
        for (int j = 0; j < 4; ++j) {
            const double4 p = ld_pt(P, idx[j]);
            const double rx = p.x - cx, ry = p.y - cy, rz = p.z - cz;
            xx += rx * rx; xy += rx * ry; xz += rx * rz; yy += ry * ry; yz += ry * rz; zz += rz * rz;
        }
        double pl[4];
        plane_from_moments(cx, cy, cz, xx, xy, xz, yy, yz, zz, pl);
        if (pl[0] == 0.0 && pl[1] == 0.0 && pl[2] == 0.0 && pl[3] == 0.0) continue;
        int cnt = 0;
        unsigned long long q = 0;
        for (int i = 0; i < n; ++i) {
            const double4 p = ld_pt(P, i);
            const double d = fabs(((pl[0] * p.x + pl[1] * p.y) + pl[2] * p.z) + pl[3]);
            if (d < thr) { ++cnt; q += (unsigned long long)floor((d * d) / thr2 * 16777216.0); }
        }
        if (cnt >= 1 && (cnt > bcnt || (cnt == bcnt && q < bq))) {   // h ascends within a lane: ties keep the first
            bcnt = cnt; bq = q; bh = h;
            for (int j = 0; j < 4; ++j) bpl[j] = pl[j];
        }
    }
    // ---- wave arg-max of (count, -qerr, -h) ----
    int rc = bcnt, rh = bh;
    unsigned long long rq = bq;
    for (int o = 32; o >= 1; o >>= 1) {
        const int oc = __shfl_xor(rc, o), oh = __shfl_xor(rh, o);
        const unsigned long long oq = __shfl_xor(rq, o);
        if (oc > rc || (oc == rc && (oq < rq || (oq == rq && oh < rh)))) { rc = oc; rq = oq; rh = oh; }
    }
    if (rc < 1) { if (lane < 4) out[lane] = 0.0; return; }
    double pl[4];
    for (int j = 0; j < 4; ++j) pl[j] = __shfl(bpl[j], rh & 63);
    // ---- refit on the inliers: lane j sums inliers j, j + 64, ...; butterfly; lane 0 ----
    double acc[6] = {0, 0, 0, 0, 0, 0};
    double c3[3] = {0, 0, 0};
    int ninl = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int base = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            double4 p = make_double4(0, 0, 0, 0);
            bool inl = false;
            if (i < n) {
                p = ld_pt(P, i);
                inl = fabs(((pl[0] * p.x + pl[1] * p.y) + pl[2] * p.z) + pl[3]) < thr;
            }
            const uint64_t m = __ballot(inl);
            if (inl) {
                const int r = (base + __popcll(m & lanemask_lt())) & 63;
                slot[r][0] = p.x; slot[r][1] = p.y; slot[r][2] = p.z;
            }
            __syncthreads();
            const int cm = __popcll(m);
            if (((lane - base) & 63) < cm) {
                const double x = slot[lane][0], y = slot[lane][1], z = slot[lane][2];
                if (pass == 0) { acc[0] += x; acc[1] += y; acc[2] += z; }
                else {
                    const double rx = x - c3[0], ry = y - c3[1], rz = z - c3[2];
                    acc[0] += rx * rx; acc[1] += rx * ry; acc[2] += rx * rz; acc[3] += ry * ry; acc[4] += ry * rz; acc[5] += rz * rz;
                }
            }
            base += cm;
            __syncthreads();
        }
        ninl = base;
        const int nacc = pass == 0 ? 3 : 6;
        for (int k = 0; k < nacc; ++k) {
            double v = acc[k];
            for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
            acc[k] = __shfl(v, 0);
        }
        if (pass == 0) {
            for (int k = 0; k < 3; ++k) { c3[k] = acc[k] / (double)ninl; acc[k] = 0.0; }
        }
    }
    double res[4];
    plane_from_moments(c3[0], c3[1], c3[2], acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], res);
    if (lane == 0) { out[0] = res[0]; out[1] = res[1]; out[2] = res[2]; out[3] = res[3]; }
}

// ---- adjacency ----
__global__ __launch_bounds__(256) void pf_adj_mark_kernel(const uint16_t *labels, size_t lstep, int w, int h, int L1, int words,
                                                           uint32_t *bits, int32_t *err) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)w * h) return;
    const int y = (int)(p / w), x = (int)(p - (long)y * w);
    auto lab = [&](int xx, int yy) { return (int)*reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(labels) + yy * lstep + xx * 2); };
    const int a = lab(x, y);
    if (a >= L1) { atomicOr(err, 1); return; }
    const int dx[4] = {1, -1, 0, 1}, dy[4] = {0, 1, 1, 1};
    for (int k = 0; k < 4; ++k) {
        const int nx = x + dx[k], ny = y + dy[k];
        if (nx < 0 || nx >= w || ny >= h) continue;
        const int b = lab(nx, ny);
        if (b == a || b >= L1) continue;
        atomicOr(&bits[(size_t)a * words + (b >> 5)], 1u << (b & 31));
        atomicOr(&bits[(size_t)b * words + (a >> 5)], 1u << (a & 31));
    }
}

__global__ __launch_bounds__(256) void pf_adj_count_kernel(const uint32_t *bits, int L1, int words, int32_t *cnt) {
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (l >= L1) return;
    int s = 0;
    for (int k = lane; k < words; k += 64) s += __popc(bits[(size_t)l * words + k]);
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) cnt[l] = s;
}

__global__ __launch_bounds__(256) void pf_adj_fill_kernel(const uint32_t *bits, int L1, int words, const int32_t *off, int32_t *neigh,
                                                           size_t capacity, int32_t *err) {
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (l >= L1) return;
    int pos = off[l];
    for (int k0 = 0; k0 < words; k0 += 64) {
        const int k = k0 + lane;
        uint32_t v = k < words ? bits[(size_t)l * words + k] : 0u;
        const int c = __popc(v);
        int incl = c;
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
        int dst = pos + incl - c;
        while (v) {
            const int b = __ffs(v) - 1;
            v &= v - 1;
            if ((size_t)dst < capacity) neigh[dst] = k * 32 + b; else atomicOr(err, 2);
            ++dst;
        }
        pos += __shfl(incl, 63);
    }
}

// ---- S19 loop ----
__device__ inline bool pf_region_valid(const int32_t *cnt, int l) { return (double)cnt[2 * l + 1] < 0.5 * (double)cnt[2 * l]; }

__global__ __launch_bounds__(1024) void pf_fit_init_kernel(PfFitArgs a) {
    __shared__ int nvalid;
    if (threadIdx.x == 0) nvalid = 0;
    __syncthreads();
    int s = 0;
    for (int l = threadIdx.x; l < a.L1; l += 1024) {
        a.assign[l] = 0;
        s += pf_region_valid(a.cnt, l) ? 1 : 0;
    }
    atomicAdd(&nvalid, s);
    __syncthreads();
    if (threadIdx.x == 0) {
        PfFitState st{};
        st.assigned = nvalid;    // planefit.cu:390-396: the count starts at the number of VALID regions
        st.err = *a.err;
        st.done = st.err ? 1 : 0;
        *a.state = st;
        *a.nplanes_out = st.err ? -1 : 0;
    }
}

// decide iteration i (if it had > 3 local planes), then sample iteration i + 1
__global__ __launch_bounds__(1024) void pf_fit_step_kernel(PfFitArgs a) {
    __shared__ int votes[kPfMaxLocal];
    __shared__ int winner;
    __shared__ PfFitState st;
    if (threadIdx.x == 0) st = *a.state;
    if (threadIdx.x < kPfMaxLocal) votes[threadIdx.x] = 0;
    __syncthreads();
    if (st.done) return;
    if (st.pending) {
        for (int l = threadIdx.x; l < a.L1; l += 1024) {
            uint64_t m = a.accept[l];
            while (m) { atomicAdd(&votes[__ffsll((unsigned long long)m) - 1], 1); m &= m - 1; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int best = 0, bc = 0;
            for (int k = 0; k < st.nlocal; ++k) if (votes[k] > bc) { best = k; bc = votes[k]; }   // planefit.cu:304-312
            winner = -1;
            if (bc >= 16) {   // acceptable labels of the winner (planefit.cu:428-430)
                for (int j = 0; j < 4; ++j) a.planes_out[(size_t)st.nplanes * 4 + j] = a.local[best * 4 + j];
                st.nplanes += 1;
                st.assigned += bc;
                winner = best;
            }
            st.pending = 0;
        }
        __syncthreads();
        if (winner >= 0)
            for (int l = threadIdx.x; l < a.L1; l += 1024)
                if ((a.accept[l] >> winner) & 1ull) a.assign[l] = (uint64_t)st.nplanes;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (!((double)st.assigned / (double)a.L1 < 0.9) || st.iter >= 100) {
            st.done = 1;
        } else {
            const int it = st.iter++;
            const int ystep = a.h / 5, xstep = a.w / 6;   // selectRandomSuperpixels(4, 3): planefit.cu:333-334
            int nl = 0, s = 0;
            if (ystep > 0 && xstep > 0) {
                for (int y = ystep; y < a.h; y += ystep)
                    for (int x = xstep; x < a.w; x += xstep, ++s) {
                        const uint64_t r = pf_stream(a.seed, 2, a.frame, (uint64_t)it, (uint64_t)s);
                        const int hx = xstep / 2, hy = ystep / 2;
                        const int xo = x - hx + (int)pf_uniform(r, 0, (uint32_t)(2 * hx + 1));
                        const int yo = y - hy + (int)pf_uniform(r, 1, (uint32_t)(2 * hy + 1));
                        if (xo < 0 || xo >= a.w || yo < 0 || yo >= a.h) continue;
                        const int l = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(a.labels) + yo * a.lstep + xo * 2);
                        if (l >= a.L1 || a.assign[l] != 0 || !pf_region_valid(a.cnt, l) || a.npts[l] < kPfMinPoints) continue;
                        if (nl < kPfMaxLocal) for (int j = 0; j < 4; ++j) a.local[nl * 4 + j] = a.planes17[(size_t)l * 4 + j];
                        ++nl;
                    }
            }
            st.nlocal = nl < kPfMaxLocal ? nl : kPfMaxLocal;   // the C ABI checks that the grid has at most kPfMaxLocal slots
            st.pending = nl > 3 ? 1 : 0;   // planefit.cu:420-422
        }
        *a.state = st;
        *a.nplanes_out = st.nplanes;
    }
}

// per label x local plane: inliers at 0.02 (planefit.cu:34-36, 103-137), accepted when > half the label's pixels
__global__ __launch_bounds__(256) void pf_fit_inliers_kernel(PfFitArgs a) {
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const PfFitState st = *a.state;
    if (st.done || !st.pending || l >= a.L1) return;
    uint64_t acc = 0;
    if (pf_region_valid(a.cnt, l) && a.assign[l] == 0) {
        const float4 *P = a.pts + a.start[l];
        const int n = a.npts[l];
        const double half = 0.5 * (double)a.cnt[2 * l];
        for (int k = 0; k < st.nlocal; ++k) {
            const double pa = a.local[k * 4], pb = a.local[k * 4 + 1], pc = a.local[k * 4 + 2], pd = a.local[k * 4 + 3];
            const double nrm = sqrt(pa * pa + pb * pb + pc * pc);
            int inl = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                bool in = false;
                if (i0 + lane < n) {
                    const double4 p = ld_pt(P, i0 + lane);
                    in = fabs(pa * p.x + pb * p.y + pc * p.z + pd) / nrm < kPfFitThr;
                }
                inl += __popcll(__ballot(in));
            }
            if ((double)inl > half) acc |= 1ull << k;
        }
    }
    if (lane == 0) a.accept[l] = acc;
}

}  // namespace

static_assert(kPfMaxLocal <= 64, "accept masks are 64-bit");

void launch_pf_points(const uint16_t *labels, size_t lstep, const float *xyz, size_t xstep, int w, int h, int L1, int pred,
                      int32_t *cursor, int ntiles, int32_t *cnt, int32_t *npts, int32_t *start, float4 *pts, int32_t *err, int32_t *lp_err,
                      hipStream_t s) {
    TileArgs a{labels, lstep, xyz, xstep, w, h, L1, pred, ntiles, cursor, cnt, start, pts, err, lp_err};
    const dim3 tg((ntiles + 3) / 4);
    hipLaunchKernelGGL(pf_tile_kernel<false>, tg, dim3(256), 0, s, a);
    hipLaunchKernelGGL(pf_colscan_kernel, dim3((L1 + 255) / 256), dim3(256), 0, s, cursor, ntiles, L1, npts);
    hipLaunchKernelGGL(pf_scan_kernel, dim3(1), dim3(1024), 0, s, (const int32_t *)npts, L1, start);
    hipLaunchKernelGGL(pf_tile_kernel<true>, tg, dim3(256), 0, s, a);
}

int pf_tiles(int w, int h) { return (int)(((long)w * h + kPfTile - 1) / kPfTile); }

void launch_pf_ransac(const float4 *pts, const int32_t *start, const int32_t *npts, int L1, double thr, uint64_t seed, uint64_t frame,
                      double *planes, hipStream_t s) {
    RansacArgs a{pts, start, npts, L1, thr, seed, frame, planes};
    hipLaunchKernelGGL(pf_ransac_kernel, dim3(L1), dim3(64), 0, s, a);
}

void launch_pf_adjacency(const uint16_t *labels, size_t lstep, int w, int h, int L1, uint32_t *bits, int32_t *cnt, int32_t *off,
                         int32_t *neigh, size_t capacity, int32_t *err, hipStream_t s) {
    const int words = (L1 + 31) / 32;
    hipLaunchKernelGGL(pf_adj_mark_kernel, dim3((unsigned)(((long)w * h + 255) / 256)), dim3(256), 0, s, labels, lstep, w, h, L1, words, bits, err);
    hipLaunchKernelGGL(pf_adj_count_kernel, dim3((L1 + 3) / 4), dim3(256), 0, s, (const uint32_t *)bits, L1, words, cnt);
    hipLaunchKernelGGL(pf_scan_kernel, dim3(1), dim3(1024), 0, s, (const int32_t *)cnt, L1, off);
    hipLaunchKernelGGL(pf_adj_fill_kernel, dim3((L1 + 3) / 4), dim3(256), 0, s, (const uint32_t *)bits, L1, words, (const int32_t *)off, neigh,
                       capacity, err);
}

int launch_pf_fit(const PfFitArgs &a, hipStream_t s) {
    int launches = 0;
    hipLaunchKernelGGL(pf_fit_init_kernel, dim3(1), dim3(1024), 0, s, a); ++launches;
    hipLaunchKernelGGL(pf_fit_step_kernel, dim3(1), dim3(1024), 0, s, a); ++launches;
    for (int it = 0; it < 100; ++it) {
        hipLaunchKernelGGL(pf_fit_inliers_kernel, dim3((a.L1 + 3) / 4), dim3(256), 0, s, a); ++launches;
        hipLaunchKernelGGL(pf_fit_step_kernel, dim3(1), dim3(1024), 0, s, a); ++launches;
    }
    return launches;
}

}  // namespace cart_amd

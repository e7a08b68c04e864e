// engine_internal.h -- shared declarations between the C-ABI host code and the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cart_engine.h"

namespace cart_amd {

constexpr int kMaxPaths = 8;
constexpr int kWtaTileX = 64;        // pixels of one row handled by one WTA block
constexpr int kMaxBatchArgs = 128;   // frames per classify launch (params travel as kernel args)
constexpr uint32_t kWtaInvalid = 0xFFFFu;
// Byte order of the 16 disparities of one lane chunk inside a cost slab: byte k of the chunk holds disparity
// chunk_base + kSlabChunkOrder[k] (the aggregation kernel's split-halves register order; the WTA consumes it as is).
constexpr int kSlabChunkOrder[16] = {0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15};

// Geometry of one engine instance; all buffers below are per workspace slot (= frame).
struct Geometry {
    int w, h, D, P;
    int min_disp, p1, p2;
    int cpitch;          // census row pitch in u32 elements (zero padded left/right)
    int cpadl;           // index of image column 0 inside a census row
    size_t npx;          // w*h
    size_t census_elems; // h*cpitch
    size_t slab_bytes;   // npx*D (one path)
};

// One scan direction inside the fused path-aggregation launch.
struct DirDesc {
    int dx, dy;
    int nlines;   // number of scan lines
    int jmin;     // line index of line 0 (skewed start column, or row for horizontal paths)
    int blk0;     // first block of this direction
    int path;     // slab index (oracle order: down, up, right, left, diagonals)
};

// Where the cost slabs of the frames of ONE launch live: frame f's P path slabs are frame[f] + path * slab_bytes, each [h][w][D].
// The slab workspace is a set of separate device allocations of at most 8 GiB (engine_host.h, SlabPool), so the frames of a
// launch need not be one address range; every SGM kernel takes this table by value (wave-uniform index: one scalar load).
constexpr int kMaxLaunchFrames = 64;   // upper bound of CART_OPT_CHUNK_FRAMES
struct SlabTable { uint8_t *frame[kMaxLaunchFrames]; };

struct AggArgs {
    const uint32_t *cen_l, *cen_r;   // slot 0 of the lease
    SlabTable slabs;                 // per frame of the launch: [path][h][w][D]
    Geometry g;
    int ndirs;
    int blocks_per_frame;
    int n_frames;        // filled by launch_aggregate
    int xcd_frames;      // filled by launch_aggregate: decode the grid per XCD (frames x, x + 8, ... on XCD x)
    int hsplit;          // filled by launch_aggregate: horizontal scans run as producer / consumer wave pairs (2 P rows per workgroup)
    int ckpt_rows;       // plan BAND_UP: K, the "up" scan stores only the rows y % K == 0, y > 0 (a power of two); 0 = every row of every scan
    DirDesc dirs[kMaxPaths];
};

constexpr int kLaunchFrames = 16;   // frames per launch sequence (cart_engine::chunk_frames) = size of the per-launch frame tables

// Pitched caller image(s) of one launch: frame f starts at ptr + f * frame_stride, or -- for frames that live in separate
// allocations (cart_compute_disparity_multi) -- at frames[f].
struct ImageBatch {
    const uint8_t *ptr;
    size_t step, frame_stride;
    const uint8_t *frames[kLaunchFrames];
    int scattered;
};
inline ImageBatch strided_images(const uint8_t *ptr, size_t step, size_t frame_stride) {
    ImageBatch b{}; b.ptr = ptr; b.step = step; b.frame_stride = frame_stride; return b;
}

struct OutBatch {   // the same for the s16 disparity images a launch writes
    int16_t *ptr;
    size_t step, frame_stride;
    int16_t *frames[kLaunchFrames];
    int scattered;
};
inline OutBatch strided_out(int16_t *ptr, size_t step, size_t frame_stride) {
    OutBatch b{}; b.ptr = ptr; b.step = step; b.frame_stride = frame_stride; return b;
}

// ---- launchers (sgm_census.hip, sgm_aggregate.hip, sgm_wta.hip, sgm_post.hip) ----
void launch_census(const ImageBatch &left, const ImageBatch &right, int channels, int n_frames,
                   uint8_t *gray_l, uint8_t *gray_r, uint32_t *cen_l, uint32_t *cen_r, uint32_t *right_pk,
                   const Geometry &g, hipStream_t s);
int agg_lines_per_block(int D);  // scan lines per 256-thread block (a pixel is owned by D/16 lanes)
int agg_residency_cap(int ndirs, int D, int n_frames, bool hsplit = false);  // 4-wave aggregation workgroups allowed per CU at a time, 0 = uncapped (measured table at its definition)
bool agg_hsplit(const Geometry &g, int ndirs, int n_frames);  // the launch runs its horizontal scans as producer / consumer wave pairs
void launch_aggregate(const AggArgs &a, int n_frames, hipStream_t s);
// thr = device table of the integer uniqueness threshold for every best cost 0..2047 (launch_uniq_table, built once per engine)
void launch_wta(const SlabTable &slabs, uint16_t *wta_l, uint32_t *right_pk, const Geometry &g, const uint16_t *thr,
                int n_frames, hipStream_t s, bool top2 = false);   // top2: the S5 variant (second-best only), two-kernel WTA only
// Slab index of the "up" direction (oracle order: down, up, right, left, diagonals).  The fused WTA computes that path itself and never reads its slab
// (the aggregate launch may skip the direction); plan BAND_UP keeps only its checkpoint rows there.
constexpr int kUpPath = 1;
// Slab index of the up-right diagonal {dx = +1, dy = -1}: the banded WTA can rebuild it inside its tile (CART_OPT_BAND_DIAG) and then reads
// only the row under each band and the column left of each tile from this slab.  The aggregation launch always writes it in full.
constexpr int kUpRightPath = 7;
size_t wta_fused_partial_elems(const Geometry &g);  // u32 elements of the per-frame right-view partial buffer
void launch_wta_fused(const uint32_t *cen_l, const uint32_t *cen_r, const SlabTable &slabs, uint16_t *wta_l, uint32_t *right_pk,
                      uint32_t *partial, const Geometry &g, const uint16_t *thr, int n_frames, hipStream_t s);
// WTA over bands of K rows that recomputes the "up" path from the checkpoint rows a launch_aggregate with ckpt_rows = K left in slab
// kUpPath (plan BAND_UP: D = 128, 8 paths, K = 4, 8 or 16)
// probe: the read-rate probe -- all P slabs are read (the aggregation launch stored every row), nothing is recomputed; K = 1 allowed
// diag: the kernel also rebuilds path kUpRightPath in LDS instead of reading its slab (CART_OPT_BAND_DIAG; ignored with the probe)
bool wta_band_supported(const Geometry &g, int K, bool probe);
void launch_wta_band(const uint32_t *cen_l, const uint32_t *cen_r, const SlabTable &slabs, uint16_t *wta_l, uint32_t *right_pk,
                     const Geometry &g, const uint16_t *thr, int n_frames, int K, bool probe, bool diag, hipStream_t s);
void launch_uniq_table(float u, uint16_t *out_dev, hipStream_t s);   // test access to the integer uniqueness threshold
void uniq_table_host(float u, uint16_t *out);
void launch_post(const uint16_t *wta_l, const uint32_t *right_pk, const uint8_t *gray_l, const OutBatch &out, const Geometry &g, int n_frames, hipStream_t s,
                 int spec = 0);
// post stage + first Jacobi pass of the radius-2 interpolation in one launch (sgm_post.hip, post_interp_kernel)
bool post_interp_fusable(int radius, int min_disp16, int max_disp);
void launch_post_interp(const uint16_t *wta_l, const uint32_t *right_pk, const uint8_t *gray_l, const OutBatch &out, const Geometry &g, int n_frames,
                        hipStream_t s, int spec, int min_disp16, int max_disp);   // spec: CART_OPT_SPEC_* bits (1 = S8 zero-disparity-invalid, 2 = S7 replicated border)

// ---- launchers (post_kernels.hip) ----
void launch_interpolate(const int16_t *src, size_t src_step, size_t src_fs, const OutBatch &dst, int w, int h, int radius,
                        int min_disp16, int max_disp, int n_frames, hipStream_t s);
void launch_dir_derivative(const int16_t *disp, size_t step, size_t fs, int16_t *out, size_t ostep, size_t ofs,
                           int32_t *hist512, int w, int h, int n_frames, hipStream_t s);
// Optional per-launch frame table of the plane kernels: with `scattered` the image of frame f is p[f] instead of
// base + f * frame_stride (the *_multi entry points: frames in separate allocations).
struct FrameTable { const void *p[kLaunchFrames]; int scattered; };
void launch_plane_derivative(const int16_t *disp, size_t step, size_t fs, int16_t *out, size_t ostep, size_t ofs,
                             int32_t *hist256, size_t hist_fs, int w, int h, int n_frames, hipStream_t s,
                             const FrameTable *disp_table = nullptr, const FrameTable *out_table = nullptr);
struct ClassifyParams { cart_plane_params p[kMaxBatchArgs]; };
void launch_classify(const int16_t *deriv, size_t step, size_t fs, const ClassifyParams &params, int per_frame,
                     uint8_t *planes, size_t pstep, size_t pfs, int w, int h, int n_frames, hipStream_t s,
                     const FrameTable *deriv_table = nullptr, const FrameTable *planes_table = nullptr);
// stat / seg / table non-null: ids + count + component table in four launches (stat = [n_frames][npx][5] scratch, all zero between calls;
// seg = [n_frames][h][tile columns] roots per row segment); null: ids + count in three
void launch_ccl(const uint8_t *planes, size_t pstep, size_t pfs, int32_t *work, int32_t *ids, size_t istep, size_t ifs,
                int32_t *ncomp, int w, int h, int n_frames, hipStream_t s, int32_t *stat = nullptr, int32_t *seg = nullptr,
                cart_component *table = nullptr, int max_components = 0);
// component table (S12) of a given id map
void launch_ccl_stats(const uint8_t *planes, size_t pstep, size_t pfs, const int32_t *ids, size_t istep, size_t ifs, int32_t *stat, int32_t *seg,
                      cart_component *table, int max_components, int32_t *ncomp, int w, int h, int n_frames, hipStream_t s);
constexpr int kCclStatInts = 5;   // int32 fields of one component's entry in the statistics scratch
size_t ccl_stats_ws_ints(int w, int h);   // int32 elements of the table workspace per slot: scratch + segment counts

void launch_classify_dev(const int16_t *deriv, size_t step, size_t fs, const cart_plane_params *params_dev, int params_stride,
                         uint8_t *planes, size_t pstep, size_t pfs, int w, int h, int n_frames, hipStream_t s);
struct ScheduleState {   // device resident
    int32_t cum[256];
    cart_plane_params params;
};
void launch_plane_schedule(ScheduleState *state, int provider, int first_id, int n_frames, int update_interval, int reset_interval,
                           const int32_t *hists, cart_plane_params *params_out, hipStream_t s);

struct TemporalArgs {
    int n_prev;
    const uint8_t *prev[CART_MAX_TEMPORAL];
    size_t prev_step[CART_MAX_TEMPORAL];
    const int16_t *flow[CART_MAX_TEMPORAL];
    size_t flow_step[CART_MAX_TEMPORAL];
};
void launch_temporal_vote(const uint8_t *planes, size_t pstep, const TemporalArgs &t, uint8_t *smoothed, size_t sstep, int w, int h, hipStream_t s);
struct QMatrix { float q[16]; };
void launch_reproject(const int16_t *disp, size_t step, size_t fs, const QMatrix &Q, float *xyz, size_t ostep, size_t ofs, int w, int h,
                      int n_frames, hipStream_t s);

// ---- superpixels (superpixel_kernels.hip) ----
constexpr int kSpChannels = 7;    // 0 x, 1 y | 2,3 disparity-derivative ch0,ch1 | 4,5,6 Y,Cr,Cb
constexpr int kSpStatRows = 15;   // 0 pixel count | 1..7 channel sums | 8..14 channel sums of squares
constexpr int kSpMaxLabels = 16384;  // the reference reserves 1 << 14 as its out-of-image marker (contourrelaxation.cu:21)
struct SpRelaxArgs {
    const uint16_t *cur;     // tight [h][w]
    uint16_t *next;
    const uint32_t *ycc;     // tight [h][w], Y | Cr << 8 | Cb << 16
    const int16_t *deriv;    // caller's 2-channel derivative image (NULL when the disparity feature is off)
    size_t deriv_step;       // bytes
    long long *stats;        // [kSpStatRows][ld]
    const double *costs;     // [kSpChannels][ld]
    long long *delta;        // [kSpStatRows][ld]
    int ld;                  // max_label_id + 1
    int w, h;
    unsigned ch_mask;        // bit ch = channel takes part
    double direct, diagonal, w_comp, prog, w_img, w_disp;
};
void launch_sp_block_init(uint16_t *labels, int w, int h, int bw, int bh, hipStream_t s);
void launch_sp_ycrcb(const uint8_t *img, size_t step, int channels, uint32_t *ycc, int w, int h, hipStream_t s);
void launch_sp_stats(const SpRelaxArgs &a, hipStream_t s);
void launch_sp_fold(long long *stats, long long *delta, double *costs, int ld, unsigned ch_mask, hipStream_t s);
void launch_sp_relax(const SpRelaxArgs &a, hipStream_t s);
void launch_sp_copy(const uint16_t *src, size_t src_step, uint16_t *dst, size_t dst_step, int w, int h, int *max_seen, hipStream_t s);
struct SpClassifyArgs {
    const int16_t *deriv; size_t deriv_step;      // 2-channel, bytes
    const uint16_t *labels; size_t labels_step;   // bytes
    int w, h, max_label;
    cart_plane_params p;
    TemporalArgs t;
    uint8_t *unsmoothed; size_t unsmoothed_step;
    uint8_t *planes; size_t planes_step;
    unsigned *votes;                              // [max_label][3], zeroed by the caller
};
void launch_sp_classify(const SpClassifyArgs &a, hipStream_t s);

// ---- superpixel plane fitting (planefit_kernels.hip) ----
constexpr int kPfMaxLocal = 64;     // grid slots of selectRandomSuperpixels(4, 3): at most 8 x 8 for any image the engine accepts
constexpr int kPfMaxPlanes = 100;   // planefit.cu:400 (iterations)
struct PfFitState { int assigned, done, iter, nplanes, nlocal, pending, err, pad; };
struct PfFitArgs {
    const uint16_t *labels; size_t lstep;
    int w, h, L1;
    uint64_t seed, frame;
    const int32_t *cnt, *npts, *start;
    const int32_t *err;       // the label_planes call's own flag (cart_planefit.lp_err): non-zero -> n_planes = -1
    const float4 *pts;
    const double *planes17;   // [L1][4]
    PfFitState *state;
    double *local;            // [kPfMaxLocal][4]
    uint64_t *accept;         // [L1]
    double *planes_out;       // [kPfMaxPlanes][4]
    uint64_t *assign;         // [L1]
    int32_t *nplanes_out;
};
int pf_tiles(int w, int h);   // 1024-pixel raster tiles of the point sort
void launch_pf_points(const uint16_t *labels, size_t lstep, const float *xyz, size_t xstep, int w, int h, int L1, int pred,
                      int32_t *cursor, int ntiles, int32_t *cnt, int32_t *npts, int32_t *start, float4 *pts, int32_t *err, int32_t *lp_err,
                      hipStream_t s);   // a label >= L1 sets bit 0 of *err and of *lp_err
void launch_pf_ransac(const float4 *pts, const int32_t *start, const int32_t *npts, int L1, double thr, uint64_t seed, uint64_t frame,
                      double *planes, hipStream_t s);
void launch_pf_adjacency(const uint16_t *labels, size_t lstep, int w, int h, int L1, uint32_t *bits, int32_t *cnt, int32_t *off,
                         int32_t *neigh, size_t capacity, int32_t *err, hipStream_t s);
int launch_pf_fit(const PfFitArgs &a, hipStream_t s);   // returns the number of launches it queued

// ---- optical flow (flow_kernels.hip) ----
void launch_block_flow(const uint32_t *cen_cur, const uint32_t *cen_prev, const Geometry &g, int radius, int block, int16_t *flow,
                       size_t flow_step, hipStream_t s, int scale = 32);   // flow = scale * (u, v): 32 = S10.5, 1 = whole pixels
// ---- coarse-to-fine flow (flow_pyramid_kernels.hip); level flows are tight s16 [h][w][2] in whole pixels ----
void launch_flow_downsample(const uint8_t *src_c, const uint8_t *src_p, int sw, int sh, uint8_t *dst_c, uint8_t *dst_p, hipStream_t s);
// g = the level's geometry; coarse = flow of the next coarser level (coarse_w wide); out32 non-null: also the S10.5 image of the caller
void launch_flow_refine(const uint32_t *cen_cur, const uint32_t *cen_prev, const Geometry &g, const int16_t *coarse, int coarse_w, int refine_radius,
                        int block, bool force_gather, int16_t *flow, int16_t *out32, size_t out32_step, hipStream_t s);
void launch_flow_median(const int16_t *in, int w, int h, bool filter, int16_t *out, int16_t *out32, size_t out32_step, hipStream_t s);

void launch_resize_linear(const uint8_t *src, size_t sstep, int sw, int sh, int channels, uint8_t *dst, size_t dstep, int dw, int dh, hipStream_t s);
// ---- ORB features (orb_kernels.hip) ----
constexpr int kOrbLevels = 8;
constexpr int kOrbEdge = 31;          // edge threshold = patch size
constexpr int kOrbTileW = 64, kOrbTileH = 16;
struct OrbCand { long long R; int y, x; };   // one NMS survivor of a level (16 B)
struct OrbLevel {
    int w, h;            // level size of this call
    int tiles_x, tile0;  // detect tiles of this level: [tile0, tile0 + tiles_x * tiles_y)
    int quota;           // n_l
    int cap;             // capacity of the level's candidate list
    size_t pyr_off;      // level image offset inside one image's pyramid (tight rows of w bytes)
    size_t cand_off;     // first record of the level inside one image's candidate lists
    float fx, fy;        // S16 ratios from the level above (level >= 1)
    float scale;         // (float)s_l
};
struct OrbPlan {
    int n_images, n_levels, total_tiles, nfeatures;
    size_t pyr_stride, cand_stride;   // per image
    OrbLevel lev[kOrbLevels];
};
struct OrbOut {
    const uint8_t *src[2]; size_t src_step[2]; int channels;
    cart_keypoint *kp[2]; uint8_t *desc[2]; size_t desc_step[2];
    int32_t *counts;
};
void launch_orb_pyramid_level(const OrbPlan &p, int level, const OrbOut &o, uint8_t *pyr, hipStream_t s);
void launch_orb_detect(const OrbPlan &p, const uint8_t *pyr, OrbCand *cand, int32_t *cand_cnt, hipStream_t s);
void launch_orb_select(const OrbPlan &p, const OrbCand *cand, const int32_t *cand_cnt, OrbCand *sel, int4 *kpi, int32_t *counts, hipStream_t s);
void launch_orb_describe(const OrbPlan &p, const uint8_t *pyr, const int4 *kpi, const char4 *pattern, const OrbOut &o, hipStream_t s);
// ---- ORB descriptor matching (match_kernels.hip) ----
constexpr int kMatchRows = 128;     // rows (one lane each) of a match_pairs workgroup
constexpr int kMatchTile = 128;     // columns staged in LDS at a time; a chunk is a whole number of tiles
constexpr int kMatchMaxChunks = 64; // column chunks of the largest matcher: bounds the partial tables
struct MatchArgs {
    cart_match_params p;
    const uint8_t *q_desc; size_t q_step; const cart_keypoint *q_kp; const int32_t *q_count;
    const uint8_t *t_desc; size_t t_step; const cart_keypoint *t_kp; const int32_t *t_count;
    int cap, chunk_len;   // max_features; columns per chunk
    int2 *fwd_part;       // [chunks][cap] (best key, second distance) of every query and train chunk
    int32_t *bwd_part;    // [chunks][cap] best key of every train row and query chunk
    int4 *fwd;            // [cap] (j1, d1, d2, -1)
    int32_t *bwd;         // [cap] i1(j)
    cart_match *matches; int32_t *match_count; int32_t *forward;
};
void launch_match(const MatchArgs &a, hipStream_t s);
// ---- stereo visual odometry (ego_kernels.hip) ----
constexpr int kEgoHypLanes = 64;    // hypotheses (one lane each) of an ego_score workgroup
constexpr int kEgoTile = 256;       // correspondences of one ego_score workgroup, staged in LDS
constexpr int kEgoLanes = 256;      // threads of the refinement workgroup = virtual lanes of the S23 sums
constexpr int kEgoCorrRows = 8;     // SoA rows of the correspondence list: a.xyz, b.xyz, u, v
struct EgoHyp { double R[9], t[3]; };   // pose of one hypothesis
struct EgoArgs {
    cart_ego_camera cam;
    cart_ego_params p;
    int cap;                           // max_features
    // triangulation
    const cart_keypoint *kpL, *kpR; const int32_t *left_count;
    const cart_match *stereo; const int32_t *stereo_count;
    double *landmarks;                 // [cap][4]
    // estimation
    const double *cur, *prev; const cart_keypoint *cur_kp;
    const cart_match *temporal; const int32_t *temporal_count;
    uint64_t seed, frame;
    double *corr;                      // [kEgoCorrRows][cap]
    int32_t *corr_k;                   // [cap] temporal match index of every correspondence
    int32_t *n;                        // number of correspondences
    EgoHyp *hyp;                       // [CART_EGO_MAX_HYPOTHESES]
    cart_ego_hypothesis *table;        // [CART_EGO_MAX_HYPOTHESES]
    cart_ego_result *result; int32_t *mask;
};
void launch_ego_triangulate(const EgoArgs &a, hipStream_t s);
void launch_ego_estimate(const EgoArgs &a, hipStream_t s);
// ---- world-frame plane map (planemap_kernels.hip) ----
// The grid is stored toroidally: window cell (rx, rz) = absolute cell (ox + rx, oz + rz) lives at column (rx + mx) mod nx, row
// (rz + mz) mod nz with mx = ox mod nx, mz = oz mod nz, so a window move copies nothing.
constexpr int kMapStrip = 8;        // image rows one lane of the vote kernel walks
struct PlaneMapGrid {
    cart_plane_map_cell *cells;        // [nz][nx], toroidal
    int nx, nz, mx, mz;
};
struct PlaneMapVoteArgs {
    PlaneMapGrid grid;
    cart_ego_camera cam;
    cart_plane_map_params p;
    double pose[12];
    double ox, oz;                     // window origin in absolute cells (integers, exact in a double)
    const int16_t *disp; size_t disp_step;
    const uint8_t *planes; size_t planes_step;
    int w, h;
};
// empties the window rectangle [rx0, rx0 + rw) x [rz0, rz0 + rh)
void launch_plane_map_clear(const PlaneMapGrid &grid, int rx0, int rw, int rz0, int rh, hipStream_t s);
void launch_plane_map_vote(const PlaneMapVoteArgs &a, hipStream_t s);
// ---- rebuilding the map from stored keyframes (planemap_kernels.hip) ----
constexpr int kRevoteStrip = 32;    // image rows one lane of the re-vote kernel walks with one open run: a multiple of kMapStrip
constexpr int kRevoteMaxEntries = 4096;
static_assert(kRevoteStrip % kMapStrip == 0, "the re-vote kernel loads kMapStrip rows at a time");
struct PlaneRevoteRecord {             // one entry of a rebuild, written by the call into the store's device array
    int32_t slot, pad;
    double pose[12];
};
static_assert(sizeof(PlaneRevoteRecord) == 104, "PlaneRevoteRecord layout (DESIGN.md S30)");
// pitched disparity + labels -> the packed planes of one store slot
void launch_plane_store_insert(const int16_t *disp, size_t disp_step, const uint8_t *planes, size_t planes_step, int16_t *dst_disp, uint8_t *dst_planes, int w, int h,
                               hipStream_t s);
// a.disp / a.planes = the store's packed planes [slot][h][w] (the steps are not read), a.pose is not read: records[k] names entry k's slot and pose
void launch_plane_map_revote(const PlaneMapVoteArgs &a, const PlaneRevoteRecord *records, int entries, hipStream_t s);
// empty != 0: the map has no window, every class is UNKNOWN
void launch_plane_map_classify(const PlaneMapGrid &grid, int empty, unsigned min_votes, unsigned percent, uint8_t *out, size_t out_step, hipStream_t s);
// ---- motion segmentation (motion_kernels.hip) ----
constexpr int kMotionStrip = 2;     // image rows one lane of the residual kernel handles
constexpr int kMotionTileW = 64, kMotionTileH = 16, kMotionMaxRadius = 4;   // the filter's tile and the largest halo
struct MotionArgs {
    cart_ego_camera cam;
    cart_motion_params p;
    double rel[12];
    const int16_t *disp_cur; size_t disp_cur_step;
    const int16_t *disp_prev; size_t disp_prev_step;
    const int16_t *flow; size_t flow_step;
    int16_t *residual; size_t residual_step;     // may be NULL
    uint8_t *raw; size_t raw_step;
    uint8_t *labels; size_t labels_step;
    const uint8_t *planes; size_t planes_step;   // may be NULL, then planes_static is
    uint8_t *planes_static; size_t planes_static_step;
    int w, h;
};
void launch_motion_residual(const MotionArgs &a, hipStream_t s);
void launch_motion_filter(const MotionArgs &a, hipStream_t s);
// ---- dense ego-motion refinement (dense_ego_kernels.hip) ----
constexpr int kDenseLanes = 256;    // threads of a workgroup = virtual lanes of the S26 sums
constexpr int kDenseSums = 28;      // 21 upper entries of H (row-major, i <= j), the 6 of g, e2
constexpr int kDenseWords = 29;     // 8-byte words of a row partial: the sums, then (count, candidates) as two int32
constexpr int kDenseCols = 4;       // sampled columns of a lane whose loads are issued together
struct DenseEgoState {              // what stays on the device between the launches of one call
    double R[9], t[3];
    double rms_initial;
    int32_t n_initial, n_candidates, steps, stop;
};
struct DenseEgoArgs {
    cart_ego_camera cam;
    cart_dense_ego_params p;
    double rel0[12];
    const int16_t *disp_cur; size_t disp_cur_step;
    const int16_t *disp_prev; size_t disp_prev_step;
    const int16_t *flow; size_t flow_step;
    const uint8_t *mask; size_t mask_step;       // may be NULL
    int w, h, ni, nj;                            // the image and its sample grid
    int rows_cap;                                // rows of the partial table: word k of sampled row j is partial[k * rows_cap + j]
    double *partial;
    DenseEgoState *state;
    cart_dense_ego_result *result;
};
void launch_dense_ego(const DenseEgoArgs &a, hipStream_t s);   // the 2 (iterations + 1) launches of one call
// ---- place recognition over an ORB keyframe database (place_kernels.hip) ----
#ifndef CART_PLACE_QUERIES_PER_LANE
#define CART_PLACE_QUERIES_PER_LANE 1   // the A/B of DESIGN.md 7.9 builds the library a second time with 2
#endif
constexpr int kPlaceLaneQueries = CART_PLACE_QUERIES_PER_LANE;
constexpr int kPlaceRows = kMatchRows * kPlaceLaneQueries;   // queries of a place_score workgroup = rows of the partial table's blocks
constexpr int kPlaceMaxSlots = 1024;       // capacity limit = threads of place_select
constexpr int kPlaceMaxCandidates = 16;
constexpr int kPlaceOccupied = 1, kPlaceHasLandmarks = 2;   // PlaceSlotHeader::flags
struct PlaceSlotHeader {                   // 16 bytes per slot, device memory: what a query needs to know about a slot
    int32_t count, flags;
    uint64_t frame_id;
};
struct PlaceStore {                        // the ring: slot k's rows start at row k * max_features of each array
    uint8_t *desc;                         // [capacity][max_features][32]
    cart_keypoint *kp;                     // [capacity][max_features]
    double *landmarks;                     // [capacity][max_features][4]
    PlaceSlotHeader *hdr;                  // [capacity]
    int max_features, capacity;
};
struct PlaceInsertArgs {
    PlaceStore db;
    const uint8_t *desc; size_t desc_step;
    const cart_keypoint *kp;
    const double *landmarks;               // may be NULL
    const int32_t *count;
    uint64_t frame_id;
    int slot;
};
struct PlaceQueryArgs {
    PlaceStore db;
    cart_place_params p;
    const uint8_t *q_desc; size_t q_step;
    const int32_t *q_count;
    uint64_t frame_id;
    int32_t *partial;                      // [query blocks][capacity] votes of one workgroup
    int32_t *scores;                       // may be NULL
    cart_place_candidate *candidates;
    int32_t *n_candidates;
};
void launch_place_insert(const PlaceInsertArgs &a, hipStream_t s);
void launch_place_query(const PlaceQueryArgs &a, hipStream_t s);   // the two launches of one query
// ---- temporal disparity fusion through ego-motion (fusion_kernels.hip) ----
#ifndef CART_FUSION_MERGE
#define CART_FUSION_MERGE 0           // the A/B of DESIGN.md 7.10 builds the library a second time with 1 (neighbouring lanes merge equal targets): no faster
#endif
constexpr int kFusionStrip = 2;       // image rows one lane of the splat kernel handles
constexpr int kFusionRows = 8;        // image rows one lane of the fuse kernel handles
constexpr int kFusionCounters = 6;    // int32 words of the object's counter block: the five source classes, then the workgroup ticket (read as three uint64)
struct FusionArgs {
    cart_ego_camera cam;
    cart_fusion_params p;
    double rel[12];
    const int16_t *disp_cur; size_t disp_cur_step;
    const int16_t *prev_disp; size_t prev_disp_step;   // NULL with prev_age: no previous frame, no splat launch
    const uint8_t *prev_age; size_t prev_age_step;
    const uint8_t *mask_prev; size_t mask_prev_step;   // may be NULL
    const uint8_t *mask_cur; size_t mask_cur_step;     // may be NULL
    int16_t *fused; size_t fused_step;
    uint8_t *age; size_t age_step;
    uint8_t *source; size_t source_step;               // may be NULL
    int32_t *counts;                                   // may be NULL
    uint32_t *zbuf;                                    // the object's z-buffer, rows of w keys; all zero between calls
    int32_t *counters;                                 // the object's [kFusionCounters]; all zero between calls
    int w, h;
};
void launch_fusion_splat(const FusionArgs &a, hipStream_t s);
void launch_fusion_fuse(const FusionArgs &a, hipStream_t s);
// ---- pose-graph optimisation over keyframes (posegraph_kernels.hip) ----
constexpr int kPgMaxNodes = 4096, kPgMaxLoops = 64, kPgMaxIterations = 16;
constexpr int kPgLinDoubles = 120;     // per odometry edge: Haa [36], Hbb [36], Hba [36], ga [6], gb [6]
constexpr int kPgLoopDoubles = 84;     // per loop edge: the U block at a [36], at b [36], ga [6], gb [6]
constexpr int kPgFacDoubles = 80;      // per node: L [36] (lower entries), 1 / diagonal [6], the sub-diagonal block [36], 2 unused
struct PgEdge {                        // 128 bytes; p_b = R p_a + t
    double R[9], t[3], w_rot, w_trans;
    int32_t a, b, pad[2];
};
struct PoseGraphStore {
    double *odom, *est, *snap;         // [max_nodes][12] each
    PgEdge *edges;                     // [max_nodes + max_loops]: the odometry edge (n - 1, n) at n, loop e at max_nodes + e
    double *lin, *lin_loop, *fac;      // [max_nodes][kPgLinDoubles], [max_loops][kPgLoopDoubles], [max_nodes][kPgFacDoubles]
    double *cols;                      // [max_nodes * 6][1 + 6 max_loops]: column 0 the right-hand side b, 1 + 6 e + c column c of loop e
    double *lc, *lr;                   // the loop system: columns of 6 max_loops + 1 rows (the last row is the right-hand side); its rows
    double *cd, *ld;                   // the diagonal of C and of its factor, [6 max_loops] each
    int max_nodes, max_loops;
};
struct PoseGraphNodeArgs {
    PoseGraphStore g;
    double pose[12], w_rot, w_trans;
    int n;                             // the new node's index
};
struct PoseGraphLoopArgs {
    PoseGraphStore g;
    PgEdge edge;
    int e;                             // the new loop's index
};
struct PoseGraphArgs {
    PoseGraphStore g;
    int n_nodes, n_loops, iterations;
    cart_pose_graph_result *result;    // may be NULL
};
void launch_pose_graph_add_node(const PoseGraphNodeArgs &a, hipStream_t s);
void launch_pose_graph_add_loop(const PoseGraphLoopArgs &a, hipStream_t s);
void launch_pose_graph_optimize(const PoseGraphArgs &a, hipStream_t s);   // one launch whatever the counts
// ---- moving-object tracks from the motion components (object_kernels.hip) ----
constexpr int kObjectHistStrip = 8;     // image rows one lane of the histogram kernel walks with one open run
constexpr int kObjectPointStrip = 4;    // image rows one lane of the point kernel walks with one open run
constexpr int kObjectMaxObjects = CART_OBJECT_MAX_OBJECTS, kObjectMaxTracks = CART_OBJECT_MAX_TRACKS;   // both = threads of object_tracks
struct ObjectAcc {                      // 96 bytes per object, all integers: what pass 2 accumulates
    uint32_t n_points, n_flow;
    int32_t lo[3], hi[3];
    int32_t x0, y0, x1, y1;
    unsigned long long sum[3], flow_sum[3];   // int64 sums, added as unsigned (two's complement)
};
static_assert(sizeof(ObjectAcc) == 96, "ObjectAcc layout (DESIGN.md S31)");
struct ObjectState {                    // the tracker's device words beside the tracks
    uint32_t next_id;
    int32_t n_seen, n_selected, n_objects;   // of the call in flight, written by object_select
};
struct ObjectArgs {
    cart_ego_camera cam;
    cart_object_params p;
    double rel[12], pose[12];
    const int32_t *ids; size_t ids_step;
    const cart_component *table; int max_components;
    const int32_t *n_components;
    const int16_t *disp_cur; size_t disp_cur_step;
    const int16_t *disp_prev; size_t disp_prev_step;
    const int16_t *flow; size_t flow_step;
    int w, h, max_objects, max_tracks;
    // the tracker's own memory
    int32_t *slot_of;                   // [max_width * max_height] by component id: the object index, -1 everywhere between calls
    int32_t *hist;                      // [max_objects][CART_OBJECT_BINS]
    int32_t *median;                    // [max_objects][2]: B_j, n_hist
    ObjectAcc *acc;                     // [max_objects]
    cart_object *objects;               // [max_objects]: the selection's fields, then the whole record
    cart_track *tracks;                 // [max_tracks]
    ObjectState *state;
    // the caller's outputs
    cart_object *objects_out;           // may be NULL
    cart_track *tracks_out;
    int32_t *counts_out;
};
void launch_object_reset(cart_track *tracks, int max_tracks, ObjectState *state, hipStream_t s);
void launch_object_update(const ObjectArgs &a, hipStream_t s);   // the five launches of one call
// ---- windowed bundle adjustment over the last frames (localba_kernels.hip) ----
constexpr int kLbaMaxWindow = CART_LOCAL_BA_MAX_WINDOW, kLbaMaxIterations = CART_LOCAL_BA_MAX_ITERATIONS;
constexpr int kLbaLanes = 256;          // threads of the reducing workgroups = virtual lanes of the S23 sums
constexpr int kLbaPointRows = 12;       // SoA rows of the per-point blocks of a step: V^-1 [9] in row order, g_p [3]
constexpr int kLbaInBit = 31;           // bit of LbaStore::used: the point takes part in the step; bit a < 16: its observation in age a does
struct LbaObs { float u, v, ur; int32_t valid; };   // one observation
static_assert(sizeof(LbaObs) == 16, "LbaObs layout (DESIGN.md S32)");
struct LbaControl {                     // the optimiser's device words
    int32_t fail, skip, n_active, n_observations, n_held;
    int32_t count[2][kLbaMaxWindow];    // usable observations per age, of the even and of the odd steps
    int32_t pad;
    double cost_before;
};
struct LbaStore {
    // the frame ring, [window] by ring slot
    double *odom, *est, *lin_est, *snap_est;   // [window][12]: as handed in, the estimate, the estimate a step linearises at, the call's snapshot
    uint64_t *frame_id;
    // the point table and the dense observation table
    double *X, *snap_X;                 // [max_points][3]
    int32_t *n_obs, *state;             // [max_points]; state 0 = free
    LbaObs *obs;                        // [max_points][window]
    // push
    LbaObs *sobs;                       // [max_features]: the stereo observation of every left index
    int32_t *tmatch;                    // [max_features]: the train index of the left index's temporal match, -1 without
    int32_t *claim;                     // [max_points]: the smallest left index that continues the point
    int32_t *free_list;                 // [max_points]: the free slots in ascending order
    int32_t *track[2];                  // [max_features] each: track_of of the newest frame and of the one before, swapped per push
    int32_t *counts;                    // [8] of the last push, then [1]: points freed by the push in flight
    // optimise
    double *blocks;                     // [kLbaPointRows][max_points]
    int32_t *used;                      // [max_points]
    LbaControl *ctl;
    double *S;                          // [6 (window - 1) + 1][6 (window - 1)]: the reduced system's lower entries, the last row its right-hand side
    double *delta;                      // [6 (window - 1)]
    int max_features, window, max_points;
};
struct LbaPushArgs {
    LbaStore g;
    cart_ego_camera cam;
    double min_disparity;
    double pose[12];
    uint64_t frame_id;
    int slot, prev_slot;                // the new frame's ring slot; the previous frame's, -1 for the first push after a clear
    int evict;                          // the ring is full: the frame in `slot` leaves
    int cur;                            // which of g.track the new frame writes
    int frames;                         // frames in the window after the push
    const cart_keypoint *kpL, *kpR; const int32_t *left_count;
    const cart_match *stereo; const int32_t *stereo_count;
    const cart_match *temporal; const int32_t *temporal_count;
    int32_t *counts_out;                // may be NULL
};
struct LbaOptArgs {
    LbaStore g;
    cart_ego_camera cam;
    cart_local_ba_params p;
    int frames, first_slot;             // age a lives in ring slot (first_slot + a) mod window
    cart_local_ba_result *result;       // may be NULL
};
void launch_local_ba_push(const LbaPushArgs &a, hipStream_t s);        // 4 launches
void launch_local_ba_optimize(const LbaOptArgs &a, hipStream_t s);     // 2 + 5 iterations launches
void launch_local_ba_poses(const LbaStore &g, int frames, int first_slot, double *out, uint64_t *ids_out, hipStream_t s);
void launch_local_ba_points(const LbaStore &g, double *out, hipStream_t s);
// ---- rolling TSDF voxel map with model raycast (voxelmap_kernels.hip) ----
// Global voxel g lives at (gx mod nx, gy mod ny, gz mod nz), x fastest; window voxel r = g - o therefore lives at (r + m) mod n per axis
// with m = o mod n.  o and n are multiples of 8, so eight window voxels along x are 32 contiguous, 32-byte aligned bytes.
#ifndef CART_VOXEL_CULL
#define CART_VOXEL_CULL 0               // the A/B of DESIGN.md 7.15 builds the library a second time with 1 (groups of slices outside the frustum are skipped): no faster
#endif
constexpr int kVoxelSlices = 4;         // z slices one lane of the integrate kernel handles at a time (nz is a multiple of 8)
#ifndef CART_VOXEL_DEPTH
#define CART_VOXEL_DEPTH 16             // the A/B of DESIGN.md 7.15 also builds 4: one group of slices per workgroup, four times the workgroups and tickets
#endif
constexpr int kVoxelDepth = CART_VOXEL_DEPTH;   // z slices per workgroup of the integrate kernel: a multiple of kVoxelSlices
constexpr int kVoxelCounters = 14;      // int32 words of the object's counter block, read as seven uint64: integrate {updated | near << 32, ticket},
                                        // raycast {NONE | HIT << 32, INSIDE | ticket << 32}, rebuild {updated, near, ticket}; all zero between calls
struct VoxelGrid {
    uint32_t *voxels;                   // [nz][ny][nx] words: tsdf in the low half, weight in the high half
    int nx, ny, nz, mx, my, mz;
    double ox, oy, oz;                  // the window origin (|o| < 2^28: exact)
};
struct VoxelIntegrateArgs {
    VoxelGrid grid;
    cart_ego_camera cam;
    cart_voxel_map_params p;
    double pose[12];
    const int16_t *disp; size_t disp_step;
    const uint8_t *mask; size_t mask_step;              // may be NULL
    int32_t *counts;                                    // may be NULL
    int32_t *counters;
    int w, h;
};
struct VoxelRaycastArgs {
    VoxelGrid grid;
    cart_ego_camera cam;
    cart_voxel_map_params p;
    double pose[12];
    int16_t *disp; size_t disp_step;
    uint16_t *weight; size_t weight_step;               // may be NULL
    uint8_t *status; size_t status_step;                // may be NULL
    int32_t *counts;                                    // may be NULL
    int32_t *counters;
    int w, h, steps;                                    // steps = K of the spec
    int empty;                                          // the map has no window: every sample is unknown
};
// empties the window box [rx0, rx0 + rw) x [ry0, ry0 + rh) x [rz0, rz0 + rd); rx0 and rw are multiples of 8
void launch_voxel_clear(const VoxelGrid &grid, int rx0, int rw, int ry0, int rh, int rz0, int rd, hipStream_t s);
void launch_voxel_integrate(const VoxelIntegrateArgs &a, hipStream_t s);
void launch_voxel_raycast(const VoxelRaycastArgs &a, hipStream_t s);
// ---- rebuilding the volume from stored keyframes (voxel_rebuild_kernels.hip) ----
struct VoxelRebuildArgs {
    VoxelGrid grid;                                     // the rebuild's fixed window
    cart_ego_camera cam;
    cart_voxel_map_params p;
    const int16_t *disp;                                // the store's planes: [capacity][h][w], packed
    const uint8_t *planes;                              // NULL = use_mask 0: the u8 plane is not read
    const PlaneRevoteRecord *records;                   // [entries], in list order
    int entries;
    int w, h;
    long long *counts;                                  // may be NULL
    int32_t *counters;                                  // the map's block; the rebuild's words start at uint64 word 4
};
void launch_voxel_rebuild(const VoxelRebuildArgs &a, hipStream_t s);   // one launch: every voxel of the window is written
// ---- surface mesh of the volume by naive surface nets (voxelmesh_kernels.hip) ----
// A thread owns the window voxel of its linear index v = (z ny + y) nx + x, which is also the order of the cells and of the voxels that own
// edges; a workgroup of kMeshBlock consecutive voxels is the unit of the two prefix sums.
#ifndef CART_MESH_BLOCK
#define CART_MESH_BLOCK 1024            // the A/B of DESIGN.md 7.18 also builds 256 and 512: fewer, larger units shorten the one-workgroup scan
#endif
constexpr int kMeshBlock = CART_MESH_BLOCK;   // a multiple of 64; the last workgroup may be partly outside the volume
constexpr int kMeshScanThreads = 1024;  // the one workgroup of the scan
constexpr uint32_t kMeshKnown = 1u, kMeshActive = 2u, kMeshCrossX = 4u, kMeshInside = 32u;   // the cell word; cross y, z = 8, 16
constexpr int kMeshIndexShift = 6;      // the cell's vertex index (< 2^26) above the flags
struct VoxelMeshArgs {
    VoxelGrid grid;
    double voxel_size;
    int min_weight;                                     // resolved: never 0
    int max_vertices, max_quads;
    int blocks;                                         // workgroups of the per-voxel passes; 0 = the map has no window
    uint32_t *cells;                                    // [nz ny nx] cell words, window order
    uint32_t *block_vertices, *block_quads;             // [blocks] counts, then exclusive offsets
    cart_mesh_vertex *vertices;
    cart_mesh_quad *quads;
    int32_t *counts;
};
void launch_voxel_mesh(const VoxelMeshArgs &a, hipStream_t s);   // 5 launches, or 1 without a window
// ---- frame-to-model pose tracking against the TSDF volume (modeltrack_kernels.hip) ----
constexpr int kTrackCols = 2;           // sampled columns of a lane whose image loads and corner gathers are issued together
struct ModelTrackArgs {                 // the sums, the row partials and the pose state are S26's (kDense*, DenseEgoState)
    VoxelGrid grid;
    cart_ego_camera cam;
    cart_voxel_map_params mp;           // the map's own: the pixel gates, voxel_size and min_weight
    cart_model_track_params p;
    double pose0[12];
    const int16_t *disp; size_t disp_step;
    const uint8_t *mask; size_t mask_step;              // NULL = no mask
    int w, h, ni, nj;                                   // the image and its sample grid
    int rows_cap;                                       // rows of the partial table: word k of sampled row j is partial[k * rows_cap + j]
    int empty;                                          // the map has no window: no pixel is a candidate
    double *partial;
    DenseEgoState *state;
    cart_model_track_result *result;
};
void launch_model_track(const ModelTrackArgs &a, hipStream_t s);   // the 2 (iterations + 1) launches of one call
// ---- the colour companion of the TSDF volume (voxelcolor_kernels.hip) ----
// The colour volume is a VoxelGrid of its own: words b | g << 8 | r << 16 | weight << 24, the empty word 0, S33's toroidal storage.
constexpr int kColorDepth = 16;         // z slices per workgroup of the colour integrate kernel: a multiple of kVoxelSlices (nz is a multiple of 8)
constexpr int kColorCounters = 8;       // int32 words of the object's counter block, read as four uint64: integrate {coloured | fresh << 32, ticket},
                                        // render {pixels with alpha > 0 | ticket << 32, unused}; all zero between calls
struct ColorIntegrateArgs {
    VoxelGrid grid;                                     // the colour volume under the map's current origin
    cart_ego_camera cam;
    cart_voxel_map_params p;                            // the map's own: the gates are S33's
    double pose[12];
    const int16_t *disp; size_t disp_step;
    const uint8_t *mask; size_t mask_step;              // NULL = no mask
    const uint8_t *image; size_t image_step;
    int channels;                                       // 1 (gray) or 3 (B, G, R)
    int max_weight;
    int32_t *counts;                                    // [2] or NULL
    int32_t *counters;
    int w, h;
};
struct ColorRenderArgs {
    VoxelGrid grid;
    cart_ego_camera cam;
    double voxel_size;
    double pose[12];
    const int16_t *disp; size_t disp_step;
    uint8_t *image; size_t image_step;                  // 8UC3
    uint8_t *alpha; size_t alpha_step;                  // NULL = not asked for
    int32_t *counts;                                    // [1] or NULL
    int32_t *counters;
    int w, h;
    int empty;                                          // the colour object has no window: every sample is (0, 0, 0, 0)
};
struct ColorVerticesArgs {
    VoxelGrid grid;
    double voxel_size;
    double mx, my, mz;                                  // the mesh origin (|o| <= 2^27: exact)
    const cart_mesh_vertex *vertices;
    const int32_t *n_vertices;                          // DEVICE
    int max_vertices;
    uint32_t *colors;                                   // [max_vertices] cart_voxel_rgb words
    int empty;
};
void launch_color_integrate(const ColorIntegrateArgs &a, hipStream_t s);
void launch_color_render(const ColorRenderArgs &a, hipStream_t s);
void launch_color_vertices(const ColorVerticesArgs &a, hipStream_t s);
// ---- colour-aided frame-to-model tracking (modeltrack_color_kernels.hip) ----
constexpr int kTrackColorSums = 29;     // S34's 28 sums, then the sum of rc rc
constexpr int kTrackColorWords = 31;    // 8-byte words of a row partial: the sums, (count, candidates) as two int32, (photometric count, 0)
constexpr int kTrackColorCols = 1;      // sampled columns of a lane whose loads and sixteen corner gathers are issued together
struct ModelTrackColorState {           // what stays on the device between the launches of one call
    double R[9], t[3];
    double rms_initial, rms_photo_initial, cost_initial;
    int32_t n_initial, n_photo_initial, n_candidates, steps, stop, reserved;
};
struct ModelTrackColorArgs {
    VoxelGrid grid;                     // the TSDF volume under the map's origin
    VoxelGrid cgrid;                    // the colour volume under the colour object's own origin
    cart_ego_camera cam;
    cart_voxel_map_params mp;           // the map's own: the pixel gates, voxel_size and min_weight
    cart_model_track_params p;
    cart_model_track_color_params cp;
    double pose0[12];
    const int16_t *disp; size_t disp_step;
    const uint8_t *mask; size_t mask_step;              // NULL = no mask
    const uint8_t *image; size_t image_step;
    int channels;                                       // 1 (gray) or 3 (B, G, R)
    int w, h, ni, nj;                                   // the image and its sample grid
    int rows_cap;                                       // rows of the partial table: word k of sampled row j is partial[k * rows_cap + j]
    int empty;                                          // the map has no window: no pixel is a candidate
    int cempty;                                         // the colour object has no window: no pixel is a photometric inlier
    double *partial;
    ModelTrackColorState *state;
    cart_model_track_color_result *result;
};
void launch_model_track_color(const ModelTrackColorArgs &a, hipStream_t s);   // the 2 (iterations + 1) launches of one call
void launch_narrow_copy(const void *src, void *dst, size_t bytes, int blocks, hipStream_t s);
int kernel_count();

}  // namespace cart_amd

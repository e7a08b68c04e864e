/*
 * cart_engine.h -- C ABI of the MI355X (gfx950) dense-stereo engine.
 *
 * This is the drop-in boundary for CART-SLAM's per-frame stereo hot path.  Every
 * entry point names the reference interface it replaces (paths relative to the
 * LorgeN/CART-SLAM tree).  Conventions:
 *   - plain C types and one opaque handle; no C++/torch/OpenCV types;
 *   - image pointers are DEVICE pointers, row-pitched (`*_step` in BYTES, like
 *     cv::cuda::GpuMat::step); the caller owns every image buffer, the engine owns
 *     only its workspaces (census maps, cost slabs, WTA maps) sized at create time;
 *   - every call returns 0 on success, non-zero on failure, never throws and never
 *     exits (the reference's CUDA_SAFE_CALL -> exit(), include/utils/cuda.cuh:193-201,
 *     is deliberately NOT replicated); cart_last_error() gives the message;
 *   - calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream).  The module adapter synchronises to mimic
 *     cv::cuda::Stream::waitForCompletion() (src/modules/disparity/disparity.cu:77);
 *   - thread-safe: one engine may be entered concurrently from many host threads
 *     (the reference enters one module object for up to 12 frames at once,
 *     include/cartslam.hpp:4-5); each call leases `n_frames` workspace slots.
 */
#ifndef CART_ENGINE_H
#define CART_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CART_DISPARITY_INVALID (-32768) /* include/modules/disparity.hpp:17 */

/* include/modules/planeseg.hpp:37-41 */
enum { CART_PLANE_HORIZONTAL = 0, CART_PLANE_VERTICAL = 1, CART_PLANE_UNKNOWN = 2 };

typedef struct cart_engine cart_engine;

/* Constructor arguments of cart::ImageDisparityModule (include/modules/disparity.hpp:26-34,
 * JSON keys src/cartconfig.cpp:144-152) plus the cv::cuda::createStereoSGM parameters the
 * reference leaves at OpenCV's defaults (P1, P2, mode -> paths). */
typedef struct {
    int device_id;
    int width, height;        /* DataSource::getImageSize(), include/datasource.hpp:75 */
    int min_disparity;        /* "min_disparity", default 4; 0..64 supported */
    int num_disparities;      /* "num_disparities": 64 | 128 | 256; 0 (with paths 0) = geometry-only engine for the
                                 post-SGM entry points: no SGM workspaces, cart_compute_disparity* fail */
    int paths;                /* 4 (MODE_HH4) | 8 (MODE_HH) */
    int p1, p2;               /* 10, 120 ; 31 + p2 must fit u8 */
    int uniqueness_ratio;     /* disparity.hpp:32 -> 12 */
    int smoothing_radius;     /* "smoothing_radius", default -1 (off); <= 8 */
    int smoothing_iterations; /* "smoothing_iterations", default 5 */
    int max_inflight;         /* workspace slots = frames that may be in flight / batched */
} cart_engine_params;

/* include/modules/planeseg.hpp:25-34 (PlaneParameters) */
typedef struct {
    int horizontal_min, horizontal_max; /* horizontalRange.first / .second */
    int vertical_min, vertical_max;     /* verticalRange.first / .second */
    int horizontal_center, vertical_center;
} cart_plane_params;

/* Fills *p with the reference's defaults (cartconfig.cpp:144-152, disparity.hpp:26-34). */
void cart_engine_default_params(cart_engine_params *p);

/* replaces: ImageDisparityModule ctor + cv::cuda::createStereoSGM (disparity.hpp:26-34) */
int cart_engine_create(const cart_engine_params *params, cart_engine **out);
void cart_engine_destroy(cart_engine *engine);

/* Launch plans of the SGM core.  Every plan produces the same bits; they differ in which path slabs exist in HBM.
 *   SLABS     all P path slabs are written by the aggregation launch and read by the WTA launch (2*P*D bytes / pixel);
 *   FUSED_UP  the "up" path is computed inside the WTA sweep and never stored (2*(P-1)*D bytes / pixel);
 *   BAND_UP   the "up" path is stored on every K-th row only (checkpoints, in place in its slab) and recomputed in registers by a
 *             WTA that works on tiles of 64 columns x K rows.  The aggregation launch WRITES (P-1 + 1/K)*D bytes / pixel.  The WTA
 *             READS less than that: it also rebuilds the up-right diagonal {+1, -1} inside its tile (CART_OPT_BAND_DIAG, default 1) and
 *             takes from that path's slab only the row under each band and the column left of each tile:
 *             (P-2 + 2/K + 1/64)*D bytes / pixel, 6.27 instead of 7.125 slabs at K = 8.  The slab is still written in full, and
 *             cart_engine_describe_plan still reports P-1 slabs.  D = 128 with 8 paths only: any other engine answers SLABS.
 * AUTO picks per launch from the measured table in DESIGN.md section 4.  Options are plain integers so that the
 * boundary stays C; nothing in the engine reads the environment.
 */
enum { CART_PLAN_AUTO = -1, CART_PLAN_SLABS = 0, CART_PLAN_FUSED_UP = 1, CART_PLAN_BAND_UP = 2 };
enum {
    CART_OPT_PLAN = 0,            /* CART_PLAN_*; default AUTO */
    CART_OPT_PLAN_MIN_FRAMES = 1, /* with a forced plan: launches of fewer frames take SLABS (default 1) */
    CART_OPT_CHUNK_FRAMES = 2,    /* frames per launch sequence inside one batched call (default 16, 1..64) */
    /* The three choices that are open upstream (cv::cuda::StereoSGM is un-vendored and un-versioned in the reference:
     * oracle/cart_oracle.h, NOTEs at S7 and S8).  Default 0 = the oracle's spec.  Whoever runs tools/ref_pin against the
     * reference's OpenCV flips the one that its outputs ask for; both forms are held bit-exact against the oracle's
     * variants by tests/test_gpu_parity.py::test_spec_variants.  These change results, by design; nothing else does. */
    CART_OPT_SPEC_S8_ZERO_INVALID = 3,      /* 1: the LR check also invalidates pixels whose integer disparity is 0 (older libSGM's `d <= 0`) */
    CART_OPT_SPEC_S7_REPLICATE_BORDER = 4,  /* 1: the 3x3 medians filter the one-pixel image border over a replicated border instead of passing it through */
    CART_OPT_SPEC_S5_TOP2 = 5,              /* 1: uniqueness tests the second-best (cost, d) only -- the top-2 wording of SURVEY.md 8a-4(4) -- instead of every
                                               disparity (the libSGM form, oracle S5); such an engine always takes plan SLABS */
    CART_OPT_BAND_ROWS = 6,                 /* K of plan BAND_UP: 4, 8 or 16 rows per band (default: the measured winner); 1 with the probe */
    CART_OPT_BAND_PROBE = 7,                /* measurement only, 1: plan BAND_UP stores and reads all P slabs and recomputes nothing -- the two-kernel WTA's
                                               work in K-row tiles (the read-rate probe of DESIGN.md 8); describe_plan then reports P slabs */
    CART_OPT_FLOW_GATHER = 8,               /* tests and measurements, 1: the refinement kernel of cart_optical_flow_pyramid never stages the previous
                                               features in LDS and gathers them from global memory in every tile (same bits; default 0: per tile) */
    CART_OPT_BAND_DIAG = 9                  /* 0 | 1 (default 1): the WTA of plan BAND_UP rebuilds the up-right diagonal path in LDS instead of reading its
                                               slab (same bits; what the aggregation launch writes does not change).  Ignored with CART_OPT_BAND_PROBE;
                                               engines that never take BAND_UP accept and ignore it */
};
int cart_engine_set_option(cart_engine *engine, int option, int value);
int cart_engine_get_option(cart_engine *engine, int option, int *value);
/* What a batched call of n_frames will do: frames per launch sequence, the plan of a full launch, and the number of
 * path slabs that plan materialises (bench.py prices its roofline line from this instead of re-deriving it). */
typedef struct {
    int frames_per_launch;
    int plan;             /* CART_PLAN_SLABS | FUSED_UP | BAND_UP */
    int slabs_written;    /* u8 slabs of D bytes per pixel written per frame (and, except under BAND_UP, read once).  BAND_UP reports P - 1: its
                             checkpoint rows are 1/K of one more slab, which this integer cannot say, and with CART_OPT_BAND_DIAG its WTA reads
                             only P - 2 + 2/K + 1/64 slabs (bench.py's moved_bytes, priced as written = read, is 3.4 % high at K = 8) */
} cart_launch_plan;
int cart_engine_describe_plan(cart_engine *engine, int n_frames, cart_launch_plan *out);

/* Placement tuning of the cost-slab workspace (no reference counterpart; OPTIONAL and opt-in: nothing calls it unless the caller asks).
 * On MI355X the time of the two slab-bound launches depends on WHICH physical memory backs the slabs: the same kernels run in one of two
 * modes per allocation (aggregation 1.41-1.43 or 1.53-1.55 ms, WTA 1.15 or 1.27 ms per 16 pairs at 1242x375 D=128 P=8;
 * profiles/r03_alloc.txt: the L2's write requests to the fabric stall 20-30x as often in the slow mode, TLB misses and clock are the same;
 * allocations above 8 GiB are always slow, which is why the engine cuts its slab workspace into groups of slots, each one plain hipMalloc
 * of at most 8 GiB - 64 MiB).
 * The call works per UNIT = the slot groups behind slots [k n, (k+1) n) of an `n_frames` call (n = min(n_frames, frames per launch)),
 * for the first (at most four) such ranges: it times the aggregation + WTA launches of n frames on the unit's current allocations, then on
 * up to `max_tries - 1` freshly allocated sets, keeps the fastest and frees the others (a candidate is compared with the kept set RE-TIMED right after it and replaces it when it is
 * 1.5 % faster: the clock drifts by more than the modes differ over a search).  A unit's search stops (cart_placement_report::stop_reason)
 *   FAST_FOUND  once the kept set is 7 % faster than the slowest one seen (both launches fast against both slow);
 *   UNIFORM     once six sets have been timed and the slowest is within 1.5 % of the kept one: the pool offers one kind of placement only
 *               (about one fresh box in ten; 64 tries bought 1.4 % on such a box) -- the best seen is kept, set-up stays under 2 s;
 *   TRIES / TIME / MEMORY  out of tries, out of the unit's time share ((0.25 s per allowed try + 1 s per 20 GB of workspace) / units),
 *               or no room for another candidate.
 * `mode` says what unit 0 -- where a caller with one call in flight lives -- ended on, RELATIVE to what the search saw (the engine knows no absolute
 * level): FAST = the kept set is at least 5.5 % under the slowest seen, i.e. a set with a launch in its slow mode was met and avoided; MIXED = the sets
 * seen differ by 1.5-5.5 % and the fastest is kept (no both-slow set was met to compare with: the kept one may well have both launches fast); UNIFORM =
 * six sets within 1.5 % of each other (all fast or all slow: the stage times tell which -- at 1242x375 D=128 P=8 the aggregation launch takes ~1.45 ms in
 * its fast mode and ~1.55 in its slow one); UNKNOWN = one try, nothing to compare with.  The ratios hold for a probe on a warmed-up GPU (call it after
 * a few real calls, as bench.py does; straight after engine creation the levels lie 12-13 % apart).
 * TRANSIENT FOOTPRINT: candidates that lost stay allocated while the search goes on (freed at once, the allocator would hand the same
 * pages back); at no time does the call hold more than `max_extra_bytes` beyond the engine's own workspace -- 0 selects two units' worth
 * (one unit = the groups of one n-frame call: 7.6 GB at 1242x375 D=128 P=8 with n = 16), SIZE_MAX lifts the cap (the search then stops
 * when the next candidate would not leave 4 GiB of device memory free; that check is not atomic across processes: pass a finite cap when
 * several processes share a GPU).  With a cap below one unit the call measures and returns without trying anything.  Peak device memory
 * of the process during the call = workspace + min(max_extra_bytes, (max_tries - 1) x unit); after it, the workspace alone.
 * The engine must be idle; results do not change (every placement gives the same bits).  `report` may be NULL. */
enum { CART_PLACE_MODE_UNKNOWN = 0, CART_PLACE_MODE_FAST = 1, CART_PLACE_MODE_MIXED = 2, CART_PLACE_MODE_UNIFORM = 3 };
enum { CART_PLACE_STOP_NOTHING_TO_DO = 0, CART_PLACE_STOP_FAST_FOUND = 1, CART_PLACE_STOP_UNIFORM = 2, CART_PLACE_STOP_TRIES = 3,
       CART_PLACE_STOP_TIME = 4, CART_PLACE_STOP_MEMORY = 5 };
typedef struct {
    float ms_first, ms_kept;                 /* launch-pair time (aggregation + WTA of n frames), mean over the probed units, before / after */
    float ms_fastest_seen, ms_slowest_seen;  /* unit 0: the kept placement and the slowest one timed */
    float seconds;                           /* wall time of the call */
    int units, candidates;                   /* units probed; placements timed in all (the initial ones included) */
    int mode, stop_reason;                   /* CART_PLACE_MODE_* / CART_PLACE_STOP_* of unit 0 */
} cart_placement_report;
int cart_engine_tune_placement(cart_engine *engine, int n_frames, int max_tries, size_t max_extra_bytes, cart_placement_report *report);

/* Message of the last failed call made by THIS thread on `engine` (or of a failed
 * create when engine == NULL).  Never NULL. */
const char *cart_last_error(const cart_engine *engine);

/* replaces: ImageDisparityModule::runInternal (src/modules/disparity/disparity.cu:49-80):
 * cvtColor x2 (:66-67) -> StereoSGM::compute (:71) -> disparity::interpolate (:73-75,
 * src/modules/disparity/interpolation.cu:85-99).  channels = 1 (gray) or 3 (BGR8).
 * out: CV_16SC1-shaped, disparity x16, invalid pixels as the reference produces them. */
int cart_compute_disparity(cart_engine *engine, const uint8_t *left, size_t left_step,
                           const uint8_t *right, size_t right_step, int channels,
                           int16_t *out, size_t out_step, void *stream);

/* Batched-frame mode (north-star config 5): frame f of each array starts at
 * base + f * <frame_stride> BYTES.  n_frames <= max_inflight. */
int cart_compute_disparity_batch(cart_engine *engine, int n_frames,
                                 const uint8_t *left, size_t left_step, size_t left_frame_stride,
                                 const uint8_t *right, size_t right_step, size_t right_frame_stride,
                                 int channels, int16_t *out, size_t out_step, size_t out_frame_stride,
                                 void *stream);

/* The same for frames that live in separate allocations: left[f] / right[f] / out[f] are the device images of frame f
 * (host arrays of n_frames device pointers, read before the call returns; one step per image kind).  This is what a
 * module adapter uses to coalesce the frames that the reference's runtime enters concurrently -- up to 12 worker threads
 * inside ImageDisparityModule::runInternal at once (cartslam.hpp:4-5, cartslam.cpp:196) -- into one launch sequence:
 * one frame per launch leaves the path-aggregation kernel latency-bound (0.67 ms per frame against 0.10 ms batched). */
int cart_compute_disparity_multi(cart_engine *engine, int n_frames,
                                 const uint8_t *const *left, size_t left_step,
                                 const uint8_t *const *right, size_t right_step, int channels,
                                 int16_t *const *out, size_t out_step, void *stream);

/* replaces: cart::disparity::interpolate (interpolation.cu:85-99) on its own; in place like the
 * reference's (the engine double-buffers internally).  min_disp16 / max_disp as disparity.hpp:27-28.
 * n_frames in [1, max_inflight]. */
int cart_interpolate(cart_engine *engine, int n_frames, int16_t *disp, size_t step, size_t frame_stride,
                     int radius, int iterations, int min_disp16, int max_disp, void *stream);

/* replaces: ImageDisparityDerivativeModule::runInternal (src/modules/disparity/derivative.cu:151-184):
 * out = CV_16SC2-shaped (ch0 vertical, ch1 horizontal), hist = 1x256 CV_32SC2-shaped device
 * buffer (512 int32 per frame), overwritten.  out, out_step and out_frame_stride on 4 bytes (a pixel is written as one word). */
int cart_disparity_derivative(cart_engine *engine, int n_frames,
                              const int16_t *disp, size_t disp_step, size_t disp_frame_stride,
                              int16_t *out, size_t out_step, size_t out_frame_stride,
                              int32_t *hist512, void *stream);

/* replaces: calculateDerivatives + mergeHistogram (src/modules/planeseg/planeseg.cu:31-158, launch :282-283).
 * hist256 (device) is ADDED to: with hist_frame_stride_elems == 0 all frames accumulate into one
 * persistent histogram like the module's (planeseg.hpp:160-161); with 256 each frame gets its own. */
int cart_plane_derivative_hist(cart_engine *engine, int n_frames,
                               const int16_t *disp, size_t disp_step, size_t disp_frame_stride,
                               int16_t *out, size_t out_step, size_t out_frame_stride,
                               int32_t *hist256, size_t hist_frame_stride_elems, void *stream);

/* replaces: classifyPlanes, non-temporal (planeseg.cu:160-198, launch :349-350).
 * params: one entry per frame if params_per_frame != 0, else params[0] for all. */
int cart_plane_classify(cart_engine *engine, int n_frames,
                        const int16_t *deriv, size_t deriv_step, size_t deriv_frame_stride,
                        const cart_plane_params *params, int params_per_frame,
                        uint8_t *planes, size_t planes_step, size_t planes_frame_stride, void *stream);

/* cart_plane_derivative_hist / cart_plane_classify for frames in separate allocations (host arrays of n_frames device
 * pointers, read before the call returns; one step per image kind): what a module adapter uses to serve the frames that
 * wait inside DisparityPlaneSegmentationModule::runInternal at the same moment with one launch per stage -- a one-frame
 * launch of these kernels costs 25-55 us of GPU time, a 16-frame launch 16-23 us.  hist_frame_stride_elems as above
 * (0: every frame adds to the one persistent histogram); params_per_frame: 0 = params[0] for all, 1 = params[f]. */
int cart_plane_derivative_hist_multi(cart_engine *engine, int n_frames,
                                     const int16_t *const *disp, size_t disp_step, int16_t *const *out, size_t out_step,
                                     int32_t *hist256, size_t hist_frame_stride_elems, void *stream);
int cart_plane_classify_multi(cart_engine *engine, int n_frames,
                              const int16_t *const *deriv, size_t deriv_step,
                              const cart_plane_params *params, int params_per_frame,
                              uint8_t *const *planes, size_t planes_step, void *stream);

/* replaces: the temporal-voting branch of classifyPlanes (planeseg.cu:199-240) with the tables the module builds at
 * :303-347: prev_planes[k] = unsmoothed planes of frame id-(k+1), flows[k] = optical flow of frame id-k (CV_16SC2-shaped,
 * S10.5 fixed point, each image and its step on 4 bytes).  n_prev <= 8.  A label byte above CART_PLANE_UNKNOWN counts as UNKNOWN.
 * The pointer arrays are HOST arrays of DEVICE pointers.  Single frame: temporal
 * smoothing makes frames depend on each other, so it does not shard. */
#define CART_MAX_TEMPORAL 8
int cart_plane_temporal_vote(cart_engine *engine, const uint8_t *planes, size_t planes_step, int n_prev,
                             const uint8_t *const *prev_planes, const size_t *prev_steps,
                             const int16_t *const *flows, const size_t *flow_steps,
                             uint8_t *smoothed, size_t smoothed_step, void *stream);

/* New stage (no reference counterpart; BASELINE config 3 "plane CCL"): 4-connected components of
 * the label map over labels {0,1}; id = smallest linear index y*width+x of the component,
 * UNKNOWN pixels -> -1.  n_components (device, one int32 per frame) may be NULL.  n_frames in [1, max_inflight]; ids, ids_step
 * and ids_frame_stride on 4 bytes (the same for the two entry points below). */
int cart_plane_ccl(cart_engine *engine, int n_frames,
                   const uint8_t *planes, size_t planes_step, size_t planes_frame_stride,
                   int32_t *ids, size_t ids_step, size_t ids_frame_stride,
                   int32_t *n_components, void *stream);

/* Component table of a label map and its ids (same stage, SURVEY 8a-11 "per-component {label, area, bbox}"): one entry per
 * component in ascending id order, bounding box inclusive.  `table` = device [n_frames][max_components]; a frame with more
 * components gets its first max_components entries, n_components (device, may be NULL) always holds the true count. */
typedef struct cart_component {
    int32_t id;            /* smallest linear index y*width+x of the component */
    int32_t label;         /* CART_PLANE_HORIZONTAL or CART_PLANE_VERTICAL */
    int32_t area;          /* pixels */
    int32_t x0, y0, x1, y1;
} cart_component;
int cart_plane_ccl_stats(cart_engine *engine, int n_frames,
                         const uint8_t *planes, size_t planes_step, size_t planes_frame_stride,
                         const int32_t *ids, size_t ids_step, size_t ids_frame_stride,
                         cart_component *table, int max_components, int32_t *n_components, void *stream);
/* cart_plane_ccl + cart_plane_ccl_stats in one call (same ids, count and table): the pass that writes the final ids also gathers
 * the component statistics, four launches in all instead of three + two.  `ids` must be an id map made by cart_plane_ccl /
 * cart_plane_ccl_table for cart_plane_ccl_stats to describe it: ids that are not roots of their own map are ignored there. */
int cart_plane_ccl_table(cart_engine *engine, int n_frames,
                         const uint8_t *planes, size_t planes_step, size_t planes_frame_stride,
                         int32_t *ids, size_t ids_step, size_t ids_frame_stride,
                         cart_component *table, int max_components, int32_t *n_components, void *stream);

/* replaces: HistogramPeakPlaneParameterProvider::updatePlaneParameters (planeseg.cu:405-458) +
 * util::findPeaks (src/utils/peaks.cpp:12-72).  HOST function on a host histogram.  Returns 1 if
 * *inout was updated, 0 on the reference's early-outs (parameters kept), <0 on error. */
int cart_find_plane_params(const int32_t hist256[256], cart_plane_params *inout);

/* Device-side plane-parameter schedule for the batched-frame mode: the same bookkeeping as
 * DisparityPlaneSegmentationModule::updatePlaneParameters (planeseg.cu:379-403: cumulative histogram, refresh when
 * id % update_interval == 1, reset when id % (update_interval*reset_interval) == 1) + the histogram_peak provider
 * (planeseg.cu:405-458) + util::findPeaks (peaks.cpp:12-72), replayed in frame-id order by one small kernel so
 * that a batch needs no device->host round trip.  `hists` = per-frame histograms [n_frames][256] (device, e.g. from
 * cart_plane_derivative_hist with hist_frame_stride_elems = 256, all-gathered across ranks in id order);
 * `params_out` = [n_frames] cart_plane_params (device) the frames are to be classified with.
 * provider: 0 = static (params_out = initial for every frame), 1 = histogram_peak. */
typedef struct cart_plane_schedule cart_plane_schedule;
int cart_plane_schedule_create(cart_engine *engine, int provider, const cart_plane_params *initial, int update_interval,
                               int reset_interval, cart_plane_schedule **out);
void cart_plane_schedule_destroy(cart_plane_schedule *schedule);
int cart_plane_schedule_advance(cart_plane_schedule *schedule, int first_id, int n_frames, const int32_t *hists,
                                cart_plane_params *params_out, void *stream);
/* Synchronises and copies the schedule's current parameters / cumulative histogram to the host (tests). */
int cart_plane_schedule_read(cart_plane_schedule *schedule, cart_plane_params *params_host, int32_t cum_hist_host[256]);

/* cart_plane_classify with the per-frame parameters in DEVICE memory (output of cart_plane_schedule_advance);
 * params_stride = 1 -> params[frame], 0 -> params[0] for every frame. */
int cart_plane_classify_dev(cart_engine *engine, int n_frames,
                            const int16_t *deriv, size_t deriv_step, size_t deriv_frame_stride,
                            const cart_plane_params *params_dev, int params_stride,
                            uint8_t *planes, size_t planes_step, size_t planes_frame_stride, void *stream);

/* replaces: DepthModule::runInternal (src/modules/depth.cpp:9-25): disparity x16 -> float (1/16) and
 * cv::cuda::reprojectImageTo3D(Q, 3 channels).  Q = row-major 4x4 (HOST pointer, copied), out = CV_32FC3-shaped.
 * Floating point: results are within 1e-4 relative of the CPU restatement (the same single-precision operations in the same order,
 * built without contraction).  xyz, xyz_step and xyz_frame_stride on 4 bytes. */
int cart_reproject_depth(cart_engine *engine, int n_frames,
                         const int16_t *disp, size_t disp_step, size_t disp_frame_stride, const float Q[16],
                         float *xyz, size_t xyz_step, size_t xyz_frame_stride, void *stream);

/* ---- superpixels ------------------------------------------------------------------------------
 * replaces: contour::ContourRelaxation + contour::createBlockInitialization as driven by SuperPixelModule
 * (src/modules/superpixels.cu:19-118, src/modules/superpixels/contourrelaxation/contourrelaxation.cu:324-447,
 * initialization.cu:13-58, features/gaussian.cu, features/compactness.cu).  The object owns the persistent label
 * image (ContourRelaxation::labelImage, contourrelaxation.hpp:47) and the per-label statistics workspaces; the
 * features are the reference's three: compactness, disparity (2-channel derivative image), colour (YCrCb).  A weight
 * <= 0 leaves the feature out (contourrelaxation.hpp:55-61).  Defaults of the JSON factory: cartconfig.cpp:121-133.
 * Semantics: oracle S13/S14 (race-free Jacobi sweeps, statistics over the whole image, fixed log sequence). */
typedef struct cart_superpixel_params {
    double direct_clique_cost;              /* 0.5 */
    double diagonal_clique_cost;            /* direct / sqrt(2) */
    double compactness_weight;              /* 0.1 */
    double progressive_compactness_cost;    /* 0.0 */
    double image_weight;                    /* 1.5 */
    double disparity_weight;                /* 1.0 */
} cart_superpixel_params;
void cart_superpixel_default_params(cart_superpixel_params *p);

typedef struct cart_superpixels cart_superpixels;
/* Allocates the state for the engine's image size and runs the block initialisation (superpixels.cu:57-59):
 * label = (y / block_h) * ceil(w / block_w) + x / block_w, max_label_id = #blocks (must be < 16384). */
int cart_superpixels_create(cart_engine *engine, const cart_superpixel_params *params, int block_w, int block_h,
                            cart_superpixels **out);
/* Keeps the device and image size it was created with, so it may be destroyed after its engine (as the plane schedule may). */
void cart_superpixels_destroy(cart_superpixels *sp);
/* Re-runs the block initialisation (the reset every `reset_iterations` frames, superpixels.cu:104-112). */
int cart_superpixels_reset(cart_superpixels *sp, void *stream);
/* ContourRelaxation::setLabelImage (contourrelaxation.cu:332-335): replaces the state with the caller's CV_16UC1
 * label image; every label must be < max_label_id (checked; synchronises `stream`). */
int cart_superpixels_set_labels(cart_superpixels *sp, const uint16_t *labels, size_t labels_step, int max_label_id,
                                void *stream);
/* ContourRelaxation::relax (contourrelaxation.cu:337-447) including the YCrCb conversion the module does first
 * (superpixels.cu:75-82): `image` = the frame's reference image, 3-channel BGR (or 1-channel gray, treated as
 * B=G=R); `deriv2` = CV_16SC2 "disparity_derivative" (may be NULL iff disparity_weight <= 0).  Runs `iterations`
 * sweeps on the state and copies the resulting label image to labels_out (CV_16UC1; may be NULL).  Calls on one
 * object are serialised in call order (the reference locks a mutex, superpixels.cu:97-99). */
int cart_superpixels_relax(cart_superpixels *sp, const uint8_t *image, size_t image_step, int channels,
                           const int16_t *deriv2, size_t deriv2_step, int iterations,
                           uint16_t *labels_out, size_t labels_out_step, void *stream);
/* superpixels_max_label blackboard value (superpixels.hpp:12). */
int cart_superpixels_max_label(const cart_superpixels *sp);

/* replaces: performSuperPixelClassifications + classifyPlanes launches (sp_planeseg.cu:27-178, 327-328).
 * deriv2 = CV_16SC2 derivative image (channel 0 is classified), labels = CV_16UC1 superpixels, max_label =
 * superpixels_max_label; n_prev/prev_planes/flows = the temporal tables the module builds (sp_planeseg.cu:243-300,
 * same layout as cart_plane_temporal_vote; n_prev = 0 -> no temporal vote).  Outputs: planes_unsmoothed = per-pixel
 * class before any vote ("planes_unsmoothed"), planes = per-superpixel majority ("planes"). */
int cart_superpixel_plane_classify(cart_engine *engine, const int16_t *deriv2, size_t deriv2_step,
                                   const uint16_t *labels, size_t labels_step, int max_label,
                                   const cart_plane_params *params, int n_prev,
                                   const uint8_t *const *prev_planes, const size_t *prev_steps,
                                   const int16_t *const *flows, const size_t *flow_steps,
                                   uint8_t *planes_unsmoothed, size_t planes_unsmoothed_step,
                                   uint8_t *planes, size_t planes_step, void *stream);

/* ---- superpixel plane fitting: planefit / planecluster ----------------------------------------------
 * replaces: the host work of SuperPixelPlaneFitModule (src/modules/planefit.cu:223-445) and SuperPixelPlaneClusterModule
 * (src/modules/planecluster.cpp:19-177), and segmentPlane / getPlaneFromPoints (src/utils/plane.cpp:56-180).  The reference
 * downloads labels + depth every frame and runs a std::random_device-seeded RANSAC per superpixel under OpenMP; its output
 * cannot be reproduced, so the stages follow a deterministic spec:
 *   S17 per-label RANSAC plane: the label's points in raster order whose xyz passes `predicate`, widened to double; fewer
 *       than 16 points -> plane (0,0,0,0).  Hypothesis h (0..99) draws 4 distinct indices from the counter-based stream
 *       stream(1, frame_id, label, h) (splitmix64; uniform index = (hi32(draw) * n) >> 32), fits them with sequential sums,
 *       and scores count = #(|((a*x + b*y) + c*z) + d| < thr) and qerr = sum of floor(dist^2 / thr^2 * 2^24); the best
 *       maximises (count, -qerr, -h) over count >= 1.  Refit on its inliers with 64-lane strided sums + butterfly.  fp64.
 *   S18 planecluster merge (host, cart_plane_cluster): the reference's region growing with one thread, groups >= 32.
 *   S19 planefit loop (device): grid samples from stream(2, frame_id, iteration, slot), up to 100 iterations, inliers at
 *       0.02, acceptance > half the label's pixels, winner needs >= 16 labels; the count starts at the VALID regions
 *       (planefit.cu:390-396, kept literally: with >= 90 % valid regions the loop does not run). */
enum { CART_PLANE_PREDICATE_PLANEFIT = 0,       /* isfinite(z) && z <= 40 && z > 0      (planefit.cu:20)     */
       CART_PLANE_PREDICATE_PLANECLUSTER = 1 }; /* !(z <= 0 || z > 40), NaN z kept      (planecluster.cpp:35) */
#define CART_PLANEFIT_MAX_PLANES 100            /* planefit.cu:400 */
#define CART_PLANEFIT_THRESHOLD 0.01            /* segmentPlane default distance threshold (plane.hpp:7-12) */

typedef struct cart_planefit cart_planefit;
/* Workspaces for labels 0..max_label_capacity (<= 16383, cart_superpixels' limit) at the engine's image size. */
int cart_planefit_create(cart_engine *engine, int max_label_capacity, cart_planefit **out);
/* Keeps the device and image size it was created with, so it may be destroyed after its engine (as the plane schedule may). */
void cart_planefit_destroy(cart_planefit *pf);
/* S17 for every label 0..max_label (replaces planefit.cu:366-384 + plane.cpp:102-180, planecluster.cpp:31-67).  labels =
 * CV_16UC1, xyz = CV_32FC3 "depth" (device, steps in bytes; labels and its step on 2 bytes, xyz and its step on 4, each step
 * at least a row: "<name> and its step must be N-byte aligned", "<name>_step is below the row size"; the same for the labels
 * of cart_planefit_adjacency and cart_planefit_fit).  Keeps the per-label statistics, point lists and planes in the
 * object for cart_planefit_fit / cart_planefit_points.  Optional device outputs (NULL = not written): planes [max_label+1][4]
 * f64, npoints [max_label+1] (points passing the predicate), counts [max_label+1][2] (all pixels, pixels failing the
 * predicate; planefit.cu:39-77).  Labels > max_label are not counted and are reported by cart_planefit_status. */
int cart_planefit_label_planes(cart_planefit *pf, const uint16_t *labels, size_t labels_step, int max_label, const float *xyz,
                               size_t xyz_step, int predicate, double thr, uint64_t seed, uint64_t frame_id, double *planes,
                               int32_t *npoints, int32_t *counts, void *stream);
/* Test / diagnostic access: the point lists of the last label_planes call.  points = device [capacity][4] f32 (x, y, z, 0),
 * label-major, raster order inside a label; offsets = device [max_label+2].  Fails if capacity < the number of points
 * (synchronises `stream` to read it). */
int cart_planefit_points(cart_planefit *pf, float *points, size_t capacity, int32_t *offsets, void *stream);
/* 8-neighbour label sets (planecluster.cpp:72-96) in CSR form: offsets = device [max_label+2], neighbours = device int32,
 * ascending inside a label.  capacity must be >= min(8 * width * height, (max_label+1) * max_label), which bounds every
 * label image: no set is ever truncated. */
int cart_planefit_adjacency(cart_planefit *pf, const uint16_t *labels, size_t labels_step, int max_label, int32_t *offsets,
                            int32_t *neighbours, size_t capacity, void *stream);
/* S19 on the device (replaces planefit.cu:386-445 incl. attemptAssignment and selectRandomSuperpixels): uses the last
 * label_planes call, which must have used CART_PLANE_PREDICATE_PLANEFIT.  Device outputs: planes [100][4] f64 (the first
 * *n_planes rows are set), assignments [max_label+1] u64 (1 + plane index, 0 = none), n_planes (int32; -1 when the label
 * image of that label_planes call held a label > max_label: then assignments are all 0 and planes is not written.  The flag
 * belongs to the label_planes call and only the next label_planes call clears it; a cart_planefit_adjacency call in between
 * does not).  *launches (host, may be NULL) = kernel launches queued.  No host synchronisation. */
int cart_planefit_fit(cart_planefit *pf, const uint16_t *labels, size_t labels_step, uint64_t seed, uint64_t frame_id,
                      double *planes, uint64_t *assignments, int32_t *n_planes, int *launches, void *stream);
/* Synchronises the object's last stream; *bad_labels = 1 if the label image of the last label_planes / adjacency call held a
 * label above its max_label (those pixels were left out).  Each of the two calls clears this flag when it starts, so it speaks
 * of the most recent of them; what cart_planefit_fit reports through n_planes is kept apart (see there). */
int cart_planefit_status(cart_planefit *pf, int *bad_labels);
/* S18 on the HOST (replaces planecluster.cpp:44-177): planes = [max_label+1][4] S17 planes (CART_PLANE_PREDICATE_PLANECLUSTER),
 * offsets / neighbours = the adjacency CSR (host copies).  Outputs: planes_out [max_label+1][4] (the first *n_planes rows),
 * assignments [max_label+1] (1 + plane index, 0 = none).  glibc atan2 / sin / cos, no FMA contraction. */
int cart_plane_cluster(const double *planes, int max_label, const int32_t *offsets, const int32_t *neighbours, double *planes_out,
                       uint64_t *assignments, int *n_planes);

/* ---- ORB keypoints and descriptors: ImageFeatureDetectorModule -------------------------------------------
 * replaces: detectOrbFeatures (src/modules/features.cpp:48-66) = cv::cuda::ORB::create(CARTSLAM_OPTION_KEYPOINTS = 5000)
 * ->detectAndComputeAsync(image, noArray(), keypoints, descriptors) + orb->convert(keypoints, host vector).  cv::cuda::ORB
 * is not deterministic (atomic FAST append, unstable sort, fastAtan2), so the stage follows a deterministic spec with
 * cv::cuda::ORB's structure and defaults (scale 1.2, 8 levels, edge 31, patch 31, FAST 20, Harris, WTA_K 2, no blur):
 *   S20 pyramid level 0 = the image (S1 gray for 3 channels), level l = S16 of level l-1 to rint(w / 1.2^l) x rint(h / 1.2^l),
 *       built while both sides are >= 63; per-level quotas n_l of nfeatures (cv::cuda::ORB's, last level clipped at 0);
 *       FAST-9 score >= 20 on [31, w-31) x [31, h-31), strict 3x3 NMS, Harris R = 25 (ab - c^2) - (a+b)^2 (int64, 7x7);
 *       per level the first n_l under (R desc, y asc, x asc); intensity-centroid moments over the half-size-15 patch,
 *       quantised to 30 bins of 12 degrees by integer cross products; 256 steered point pairs drawn from the S17 stream.
 *       Descriptors are NOT interchangeable with OpenCV's (different pattern); angles are multiples of 12 degrees. */
#define CART_ORB_DEFAULT_FEATURES 5000   /* CARTSLAM_OPTION_KEYPOINTS, include/modules/features.hpp:11 */
#define CART_ORB_MAX_FEATURES 65536
#define CART_ORB_LEVELS 8
#define CART_ORB_DESCRIPTOR_BYTES 32

/* cv::KeyPoint's layout (28 B): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct cart_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} cart_keypoint;

typedef struct cart_orb cart_orb;
/* Workspaces (pyramids, candidate lists, counters, the steered pattern) for two images up to max_width x max_height and
 * nfeatures in [1, 65536]; nothing is allocated per call.  Works on an engine of any disparity setting (0 / 0 included). */
int cart_orb_create(cart_engine *engine, int max_width, int max_height, int nfeatures, cart_orb **out);
/* Keeps the device and image size it was created with, so it may be destroyed after its engine (as the plane schedule may). */
void cart_orb_destroy(cart_orb *orb);
/* Host only, no GPU (features.cpp's orb object's level layout): level sizes and quotas of all 8 levels into the arrays
 * (each CART_ORB_LEVELS long, any may be NULL).  Returns the number of levels built (0..8), or -1 on bad arguments. */
int cart_orb_levels(int width, int height, int nfeatures, int *level_w, int *level_h, int *level_n);
/* detectAndComputeAsync + convert for 1 or 2 images (the left and right image of a frame go through one launch sequence,
 * features.cpp:21-22).  images[i] = device u8, channels 1 (gray) or 3 (BGR), width x height <= the create size, rows
 * steps[i] bytes apart.  Device outputs per image: keypoints[i] = cart_keypoint [nfeatures] (4-byte aligned),
 * descriptors[i] = [nfeatures] rows of 32 bytes, descriptor_steps[i] bytes apart (NULL = 32), counts[i] = keypoints
 * written (int32, device).  Keypoints are ordered by level, then (response desc, y asc, x asc).  No host synchronisation. */
int cart_orb_detect(cart_orb *orb, int n_images, const uint8_t *const *images, const size_t *steps, int channels, int width,
                    int height, cart_keypoint *const *keypoints, uint8_t *const *descriptors, const size_t *descriptor_steps,
                    int32_t *counts, void *stream);
/* Test / diagnostic access to the last detect call: level `level` of image `image` (device dst, level_w x level_h u8,
 * dst_step bytes; NULL = not copied) and the number of NMS survivors of that level before selection (host int32, NULL =
 * not read; synchronises `stream`).  Fails for a level that call did not build. */
int cart_orb_debug_level(cart_orb *orb, int image, int level, uint8_t *dst, size_t dst_step, int32_t *n_candidates, void *stream);

/* ---- ORB descriptor matching: stereo and temporal correspondences (spec S22) --------------------------------
 * An extension: the reference's feature module only draws its keypoints.  Brute-force Hamming matching of two sets of 256-bit
 * descriptors (what cart_orb_detect writes), integer and deterministic:
 *   d(i, j) = popcount(Q_i xor T_j).  With use_gate, a pair (i, j) is admissible iff dx_min <= q.x - t.x <= dx_max, dy_min <=
 *   q.y - t.y <= dy_max (one float32 subtraction each, bounds inclusive, NaN fails) and max_octave_diff < 0 or
 *   |q.octave - t.octave| <= max_octave_diff (int32 arithmetic); without it every pair is.
 *   Forward: (d1, j1) of the minimum d * 65536 + j over the admissible j of query i (ties go to the lowest train index), d2 = the
 *   minimum d over admissible j != j1 (may equal d1), -1 without one; j1 = d1 = d2 = -1 without any admissible j.
 *   Backward: i1(j) = the i of the minimum d * 65536 + i over the admissible i of train j.
 *   Query i is accepted iff j1 >= 0, d1 <= max_distance, (ratio == 0 or d2 < 0 or 100 d1 < ratio d2) and (cross_check == 0 or
 *   i1(j1) == i). */
typedef struct cart_match {
    int32_t query, train, distance, second;   /* i, j1, d1, d2 */
} cart_match;
typedef struct cart_match_params {
    int32_t use_gate;                         /* 0 | 1 */
    float dx_min, dx_max, dy_min, dy_max;     /* inclusive bounds on q - t */
    int32_t max_octave_diff;                  /* < 0: no octave test */
    int32_t max_distance;                     /* 0..256 */
    int32_t ratio;                            /* 0..100, 0 = off */
    int32_t cross_check;                      /* 0 | 1 */
} cart_match_params;
void cart_match_default_params(cart_match_params *p); /* gate off, octave test off, 64, 80, 1 */

typedef struct cart_matcher cart_matcher;
/* Workspaces for sets of up to max_features (1..65536) descriptors each; nothing is allocated per call. */
int cart_matcher_create(cart_engine *engine, int max_features, cart_matcher **out);
/* Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_matcher_destroy(cart_matcher *matcher);
/* Query set q, train set t: descriptor rows of 32 bytes q_step / t_step (>= 32) bytes apart, cart_keypoint records (4-byte
 * aligned; may be NULL when use_gate is 0) and the set sizes as DEVICE int32 (what cart_orb_detect writes; clamped to [0,
 * max_features]; rows at or beyond a size are never read).  Device outputs: matches [max_features] = the accepted queries in
 * ascending query order, match_count = their number, forward (may be NULL) = int32 [max_features][4], of which the first
 * q_count rows are written: (j1, d1, d2, i1(j1)), entry 3 = -1 when cross_check is 0 or j1 < 0.  No host synchronisation. */
int cart_matcher_match(cart_matcher *matcher, const cart_match_params *params, const uint8_t *q_desc, size_t q_step,
                       const cart_keypoint *q_kp, const int32_t *q_count, const uint8_t *t_desc, size_t t_step,
                       const cart_keypoint *t_kp, const int32_t *t_count, cart_match *matches, int32_t *match_count,
                       int32_t *forward, void *stream);

/* ---- Stereo visual odometry: frame-to-frame ego-motion from the ORB matches (spec S23) ------------------------
 * An extension: the reference estimates no pose.  The stereo matches of a frame are triangulated into landmarks, the temporal
 * matches whose two ends have landmarks become 3-D / 3-D correspondences, seeded three-point (triad) hypotheses are scored by
 * their left-image reprojection inliers, and the best is refined by Gauss-Newton.  fp64 with + - * / sqrt only, integer scores,
 * every sum in a fixed order: deterministic, restated in tests/np_ego.py.  Pose convention: p_cur = R p_prev + t. */
typedef struct cart_ego_camera {
    double fx, fy, cx, cy, baseline;          /* fx, fy, baseline > 0 */
} cart_ego_camera;
typedef struct cart_ego_params {
    double min_disparity;                     /* a landmark needs left.x - right.x >= this (> 0) */
    double inlier_threshold;                  /* pixels (> 0) */
    int32_t hypotheses;                       /* 1..1024 */
    int32_t refine_iterations;                /* 0..16 */
} cart_ego_params;
void cart_ego_default_params(cart_ego_params *p); /* extension: 1.0, 2.0, 256, 4 */
#define CART_EGO_MAX_HYPOTHESES 1024
#define CART_EGO_MAX_REFINE 16
typedef struct cart_ego_result {
    double R[9], t[3];                        /* row-major rotation and translation; the identity when status is 0 */
    double rms;                               /* sqrt(mean squared reprojection error) of the final inliers, pixels */
    int32_t status;                           /* 1 = a pose was found */
    int32_t n_correspondences, n_inliers;
    int32_t best_hypothesis;                  /* -1 when status is 0 */
} cart_ego_result;
typedef struct cart_ego_hypothesis {
    uint64_t qerr;                            /* sum over the inliers of floor(e2 / thr^2 * 2^24) */
    int32_t count, skipped;                   /* inliers; 1 = degenerate sample, not scored */
} cart_ego_hypothesis;

typedef struct cart_ego cart_ego;
/* Extension.  Workspaces for lists of up to max_features (1..65536) keypoints / matches; nothing is allocated per call. */
int cart_ego_create(cart_engine *engine, int max_features, cart_ego **out);
/* Extension.  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_ego_destroy(cart_ego *ego);
/* Extension.  Landmarks of one frame: kpL / kpR = the cart_keypoint records of the left and right image, left_count = the number of
 * left keypoints, stereo_matches / stereo_count = a match list with query = left, train = right and distinct queries (what
 * cart_matcher_match writes); all device memory, the counts DEVICE int32 clamped to [0, max_features].  landmarks = device double
 * [max_features][4] (8-byte aligned): (X, Y, Z, 1.0) for a left index with an accepted match, four zeros for every other
 * index below left_count; rows from left_count on are not written.  A match with an index outside [0, left_count) x
 * [0, max_features) is ignored.  No host synchronisation. */
int cart_ego_triangulate(cart_ego *ego, const cart_ego_camera *camera, const cart_ego_params *params, const cart_keypoint *kpL,
                         const cart_keypoint *kpR, const int32_t *left_count, const cart_match *stereo_matches,
                         const int32_t *stereo_count, double *landmarks, void *stream);
/* Extension.  Relative pose between two frames: cur_landmarks / cur_kpL of the current frame, prev_landmarks of the previous one
 * (each what cart_ego_triangulate wrote), temporal_matches / temporal_count = matches with query = current left, train =
 * previous left (device; the count a DEVICE int32, clamped to [0, max_features]).  Device outputs: result (8-byte aligned) and
 * inlier_mask (may be NULL) = int32 [max_features], entry k = 1 iff temporal match k is a final inlier (all max_features entries
 * are written).  The draws of hypothesis h come from the S17 stream (seed, 3, frame_id, h, 0).  No host synchronisation. */
int cart_ego_estimate(cart_ego *ego, const cart_ego_camera *camera, const cart_ego_params *params, const double *cur_landmarks,
                      const cart_keypoint *cur_kpL, const double *prev_landmarks, const cart_match *temporal_matches,
                      const int32_t *temporal_count, uint64_t seed, uint64_t frame_id, cart_ego_result *result,
                      int32_t *inlier_mask, void *stream);
/* Extension.  Test / diagnostic access to the last cart_ego_estimate call: the per-hypothesis table into host_dst (HOST, `capacity`
 * records; the first *n_hypotheses = that call's params.hypotheses are written).  Synchronises `stream`. */
int cart_ego_debug_hypotheses(cart_ego *ego, cart_ego_hypothesis *host_dst, int capacity, int *n_hypotheses, void *stream);

/* ---- World-frame bird's-eye plane map (spec S24) -----------------------------------------------------------------
 * An extension: the headless, race-free, accumulated form of the reference's paintBEVPlanes (planeseg_vis.cu:58-107).  A rolling
 * grid of cells_x x cells_z cells in the world's X-Z plane; every frame's disparity + plane labels vote into it through the frame's
 * camera-to-world pose.  fp64 with + - * / floor only and integer atomics: independent of execution order, restated in
 * tests/np_planemap.py.
 *   Window: c = floor(t / cell_size) per axis (t_x = pose[3], t_z = pose[11]), origin o = 16 floor_div(c - N / 2, 16) in absolute
 *   cells.  The first update after create / clear starts an empty window; afterwards the cells of the new window that the old one
 *   did not hold are empty before the frame's votes, and cells that leave are forgotten.
 *   Vote of pixel (x, y), disparity s, label l, in this order: l in {0, 1}; s != -32768; d = s / 16.0 >= min_disparity;
 *   Z = (fx baseline) / d <= max_depth; X = ((x - cx) Z) / fx in [-max_lateral, max_lateral]; Y = ((y - cy) Z) / fy;
 *   p_w[r] = ((P[4r] X + P[4r+1] Y) + P[4r+2] Z) + P[4r+3]; gx = floor(Xw / cell_size), gz = floor(Zw / cell_size); inside the
 *   window (compared as doubles) the cell's `horizontal` (l = 0) or `vertical` (l = 1) count grows by one, and for l = 1
 *   y_min / y_max take q = (int32) clamp(floor(Yw / height_quantum), -2^30, 2^30).  Votes outside the window are dropped.
 *   At the defaults the depth gate also removes the invalid marker of a range-fixed disparity, (min_disp - 1) * 16: with
 *   min_disp = 4 that is d = 3, Z = fx baseline / 3 > 20 m for any fx baseline > 60 (KITTI: 386).  When max_depth is raised,
 *   set min_disparity to the disparity module's own minimum. */
typedef struct cart_plane_map_cell {
    uint32_t horizontal, vertical;            /* votes */
    int32_t y_min, y_max;                     /* quantised world Y extent of the vertical votes */
} cart_plane_map_cell;                        /* the empty cell is (0, 0, INT32_MAX, INT32_MIN) */
typedef struct cart_plane_map_params {
    double cell_size;                         /* metres, >= 0.01 */
    double min_disparity;                     /* pixels, > 0 */
    double max_depth;                         /* metres, > 0; the reference's 20 */
    double max_lateral;                       /* metres, > 0; the reference's 10 */
    double height_quantum;                    /* metres, >= 0.001 */
} cart_plane_map_params;
void cart_plane_map_default_params(cart_plane_map_params *p); /* extension: 0.25, 1.0, 20.0, 10.0, 0.05 */

typedef struct cart_plane_map cart_plane_map;
/* Extension.  cells_x, cells_z: multiples of 16 in 32..4096.  The parameters are fixed for the object's life.  Stateful like
 * cart_superpixels: calls on one object must be issued in frame order.  cells_x, cells_z and params are checked before the engine,
 * so a configuration can be validated without a device. */
int cart_plane_map_create(cart_engine *engine, int cells_x, int cells_z, const cart_plane_map_params *params, cart_plane_map **out);
/* Extension.  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_plane_map_destroy(cart_plane_map *map);
/* Extension.  Empties the grid: the next update starts a new window.  No device work. */
int cart_plane_map_clear(cart_plane_map *map);
/* Extension.  One frame: pose = HOST double [12], the 3 x 4 camera-to-world matrix in KITTI row order (all finite, |R entries| <= 2,
 * |t entries| <= 1e6); disparity = device int16 x16 (2-byte aligned, step a multiple of 2), planes = device u8 labels, both
 * width x height (1..16384 each), steps in bytes.  Moves the window, clears what entered it, votes.  The camera, the pose and the
 * sizes are checked before the map and the images.  No host synchronisation. */
int cart_plane_map_update(cart_plane_map *map, const cart_ego_camera *camera, const double *pose, const int16_t *disparity,
                          size_t disparity_step, const uint8_t *planes, size_t planes_step, int width, int height, void *stream);
/* Extension.  HOST getter: the window origin in absolute cells and whether a window exists (0 after create / clear). */
int cart_plane_map_window(cart_plane_map *map, int64_t *origin_x, int64_t *origin_z, int *valid);
/* Extension.  Test / dump access: synchronises `stream` and copies the cells in window order (row gz - oz, column gx - ox) into
 * host_cells (HOST, cells_z * cells_x records); without a window every cell is empty and the origin is (0, 0). */
int cart_plane_map_read(cart_plane_map *map, cart_plane_map_cell *host_cells, int64_t *origin_x, int64_t *origin_z, void *stream);
/* Extension.  Classes of the window into classes (device u8 [cells_z][cells_x], classes_step bytes per row), with the Plane enum's
 * values: n = horizontal + vertical (uint64); n < min_votes (>= 1) -> 2 (UNKNOWN), else vertical * 100 >= obstacle_percent
 * (1..100) * n -> 1 (VERTICAL = obstacle), else 0 (HORIZONTAL = free).  No host synchronisation. */
int cart_plane_map_classify(cart_plane_map *map, int min_votes, int obstacle_percent, uint8_t *classes, size_t classes_step, void *stream);

/* ---- Rebuilding the plane map after a pose correction (spec S30) ------------------------------------------------
 * An extension.  A store keeps the disparity and label images of keyframes on the device; cart_plane_map_rebuild empties the map's
 * window and votes every stored frame that is named again, each through a NEW pose, in one launch sequence.  S24's votes are integer
 * sums, minima and maxima, so the rebuilt cells equal, byte for byte, an empty window at that origin plus each used entry's S24 votes
 * in any order; restated in tests/np_planemap_rebuild.py.
 *   Store: a ring of `capacity` frames of exactly width x height, each the int16 x16 disparity image and the u8 label image, tightly
 *   packed and copied verbatim: no gate is applied at insertion, so a store is independent of any map, camera or parameter set.
 *   Insertion number n (counted from 0 since create / clear) goes to slot n mod capacity and evicts what was there.  Every slot
 *   remembers the caller's frame_id; the id table is host state.  Ids are looked up newest first, so a repeated id names its latest
 *   insertion.
 *   Rebuild: the window origin is S24's, taken from window_pose (t_x = P[3], t_z = P[11]); every cell of the window is emptied; every
 *   entry (frame_id, pose) whose id is in the store votes by S24's Vote rule into that fixed window through its own pose, with the
 *   map's own params; votes outside the window are dropped.  Entries whose id is not in the store (evicted or never inserted) are
 *   skipped and counted: used = count - skipped.  An id may appear more than once and then votes once per appearance.  count = 0
 *   leaves an empty window at the new origin.  Afterwards the map is valid with that origin and cart_plane_map_update continues on it
 *   as after any update. */
typedef struct cart_plane_store cart_plane_store;
/* Extension (S30).  width, height in 1..16384, capacity in 1..1024, all checked before the engine.  Device footprint:
 * 3 * width * height * capacity bytes for the images plus 4096 records of 104 bytes for the entries of a rebuild:
 * 1242 x 375 x 256 is about 358 MB. */
int cart_plane_store_create(cart_engine *engine, int width, int height, int capacity, cart_plane_store **out);
/* Extension (S30).  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_plane_store_destroy(cart_plane_store *store);
/* Extension (S30).  Forgets every frame; the next insertion is number 0 again.  HOST only, no device work. */
int cart_plane_store_clear(cart_plane_store *store);
/* Extension (S30).  HOST getter: the number of frames held (at most capacity) and the capacity; either pointer may be NULL. */
int cart_plane_store_size(cart_plane_store *store, int *frames, int *capacity);
/* Extension (S30).  One frame into the ring under frame_id: disparity = device int16 x16 (2-byte aligned, step a multiple of 2),
 * planes = device u8 labels, steps in bytes, both width x height, which must equal the store's.  The sizes are checked before the
 * store and the images.  One copy kernel; no host synchronisation. */
int cart_plane_store_insert(cart_plane_store *store, uint64_t frame_id, const int16_t *disparity, size_t disparity_step,
                            const uint8_t *planes, size_t planes_step, int width, int height, void *stream);
/* Extension (S30).  HOST getter: the slot that holds frame_id's latest insertion, or -1. */
int cart_plane_store_contains(cart_plane_store *store, uint64_t frame_id, int *slot_or_minus_1);
/* Extension (S30).  ids = HOST uint64 [count], poses = HOST double [count][12] (3 x 4 camera-to-world, as cart_plane_map_update's),
 * count in 0..4096, window_pose = HOST double [12]; used_out (HOST, may be NULL) receives the number of entries that voted.  count,
 * the camera, window_pose and every poses[k] are checked before the map and the store, so a configuration can be validated without
 * a device; map and store must be on one device.  The entries travel through a pinned buffer of the store: a rebuild that follows
 * another waits on the host for that earlier upload alone (not for its kernels) before it rewrites the buffer.  No other host
 * synchronisation.  Holds the map, then the store. */
int cart_plane_map_rebuild(cart_plane_map *map, cart_plane_store *store, const cart_ego_camera *camera, const uint64_t *ids,
                           const double *poses, int count, const double *window_pose, int *used_out, void *stream);

/* ---- Motion segmentation from flow, disparity and ego-motion (spec S25) ------------------------------------------
 * An extension: the reference has no such stage.  A pixel moves on its own if the point seen there in frame t-1 (through the flow and
 * the previous disparity), carried through the relative pose and projected back, does not land where the image and the disparity of
 * frame t see it.  fp64 with + - * / floor only, every sum in the written order, no atomics: restated in tests/np_motion.py.
 *   Raw label of pixel (x, y); the first failing gate makes it 2 (UNKNOWN):
 *     1. s_c = disp_cur[y][x] != -32768 and d_c = s_c / 16.0 >= min_disparity;
 *     2. xp = x - (flow.x >> 5), yp = y - (flow.y >> 5) (arithmetic shifts of the S10.5 components) lie inside the image;
 *     3. s_p = disp_prev[yp][xp] passes the gate of step 1, giving d_p;
 *     4. Zp = (fx baseline) / d_p, Xp = ((xp - cx) Zp) / fx, Yp = ((yp - cy) Zp) / fy,
 *        q[r] = ((rel[4r] Xp + rel[4r+1] Yp) + rel[4r+2] Zp) + rel[4r+3], and q.z > 0.
 *   Then eu = ((fx q.x) / q.z + cx) - x, ev = ((fy q.y) / q.z + cy) - y, ed = (fx baseline) / q.z - d_c, and the label is 1 (MOVING)
 *   iff eu eu + ev ev > flow_threshold^2 or ed ed > disparity_threshold^2, else 0 (STATIC).  The three values are the Plane enum's, so
 *   cart_plane_ccl_table works on a motion label image unchanged.
 *   Residual record (int16 x 4): (Q(eu), Q(ev), Q(ed), raw label) with Q(e) = clamp(floor(16 e + 0.5), -32767, 32767) and Q(NaN) = -32767 (reachable only where a camera's fx baseline overflows); an UNKNOWN
 *   pixel holds (-32768, -32768, -32768, 2).
 *   Filtered label: raw 2 stays 2; else with n_m / n_s the raw 1 / raw 0 pixels of the (2 radius + 1)^2 window clipped to the image,
 *   the pixel itself included, 1 iff n_m 100 >= support_percent (n_m + n_s), else 0.  radius = 0: filtered = raw.
 *   Static planes: planes_static = (filtered == 1) ? 2 : planes. */
typedef struct cart_motion_params {
    double min_disparity;                     /* pixels, > 0 */
    double flow_threshold;                    /* pixels, > 0 */
    double disparity_threshold;               /* pixels, > 0 */
    int32_t radius;                           /* 0..4 */
    int32_t support_percent;                  /* 1..100 */
} cart_motion_params;
void cart_motion_default_params(cart_motion_params *p); /* extension: 1.0, 2.0, 1.0, 2, 50 (build-owned, untuned) */
/* Extension.  One frame, stateless: every buffer is the caller's device memory, width x height (1..16384 each), steps in bytes.
 * rel = HOST double [12], the 3 x 4 (R | t) in row order with p_cur = R p_prev + t (cart_ego_result's R and t as a KITTI pose row; all
 * finite, |R entries| <= 2, |t entries| <= 1e6).  disp_cur / disp_prev = int16 x16 (2-byte aligned), flow = int16 x 2 in S10.5 of the
 * current frame against the previous one (4-byte aligned), residual = int16 x 4 (8-byte aligned; may be NULL), raw / labels = u8;
 * planes (may be NULL) / planes_static (NULL iff planes is) = u8.  Steps are multiples of the alignment.  No output (residual, raw,
 * labels, planes_static) may overlap another output or an input: each such pair is refused by name.  Checked in this order, all before any device call: params, camera, rel, sizes, engine, then
 * pointers, alignment and steps; a refused call touches no output.  Asynchronous on `stream`, no host synchronisation. */
int cart_motion_segment(cart_engine *engine, const cart_ego_camera *camera, const double *rel, const cart_motion_params *params,
                        const int16_t *disp_cur, size_t disp_cur_step, const int16_t *disp_prev, size_t disp_prev_step,
                        const int16_t *flow, size_t flow_step, int width, int height, int16_t *residual, size_t residual_step,
                        uint8_t *raw, size_t raw_step, uint8_t *labels, size_t labels_step, const uint8_t *planes, size_t planes_step,
                        uint8_t *planes_static, size_t planes_static_step, void *stream);

/* ---- Dense ego-motion refinement from flow and disparity (spec S26) ----------------------------------------------
 * An extension: the reference estimates no pose.  Gauss-Newton refinement of a relative pose (cart_ego_result's, p_cur = R p_prev + t)
 * over every static pixel: the inputs are cart_motion_segment's.  fp64 with + - * / sqrt only, every sum in a fixed two-level order,
 * no floating-point atomics: restated in tests/np_dense_ego.py.
 *   Sample grid: pixels (x, y) = (i stride, j stride) inside the image.  A pixel is a candidate (independent of the pose) iff it passes
 *   gates 1-3 of S25 (giving d_c, xp, yp, d_p) and mask is NULL or mask[y][x] != 1 (MOVING).
 *   At the pose (R, t): Zp, Xp, Yp and q as S25's gate 4 with rel[4r + c] = R[3r + c], rel[4r + 3] = t[r]; eu, ev, ed as S25.  A
 *   candidate contributes iff q.z > 0, eu eu + ev ev < flow_threshold^2 and ed ed < disparity_threshold^2.
 *   Rows: a = fx / q.z, b = -((fx q.x) / (q.z q.z)), c = fy / q.z, d = -((fy q.y) / (q.z q.z)), g = -((fx baseline) / (q.z q.z)),
 *     Ju = (b q.y, a q.z - b q.x, -(a q.y), a, 0, b), Jv = (d q.y - c q.z, -(d q.x), c q.x, 0, c, d) (S23), Jd = (g q.y, -(g q.x), 0, 0, 0, g);
 *     H_ij = (Ju_i Ju_j + Jv_i Jv_j) + wd (Jd_i Jd_j) for i <= j, g_i = (Ju_i eu + Jv_i ev) + wd (Jd_i ed),
 *     e2 = (eu eu + ev ev) + wd (ed ed), wd = disparity_weight: 28 sums and an integer count.
 *   Order of every sum: for sampled row j, virtual lane l of 256 starts at +0.0 and adds its contributing pixels of sampled columns
 *   l, l + 256, ... in ascending order, then v[l] += v[l ^ o] for o = 1, 2, 4 .. 128 and lane 0 holds the row's partial; virtual lane l
 *   then adds the partials of sampled rows l, l + 256, ... (every row, ascending) and the same butterfly follows.
 *   Iteration: (R, t) = rel0; an evaluation there gives n_initial and rms_initial; up to `iterations` times: evaluate, stop if the count
 *   is below min_inliers, solve H delta = -g by S23's unpivoted Cholesky (stop at a pivot that is not > 0), update the pose as S23
 *   does, steps += 1; a last evaluation gives n_inliers and rms = sqrt(sum e2 / n) (0.0 at n = 0).
 *   Acceptance is the consumer's: take (R, t) iff status == 1, all 12 entries are finite and n_inliers >= n_initial, else keep rel0. */
typedef struct cart_dense_ego_params {
    double min_disparity;                     /* pixels, finite, > 0 */
    double flow_threshold;                    /* pixels, finite, > 0 */
    double disparity_threshold;               /* pixels, finite, > 0 */
    double disparity_weight;                  /* finite, >= 0 */
    int32_t iterations;                       /* 0..16 */
    int32_t stride;                           /* 1..16 */
    int32_t min_inliers;                      /* 6..2^30 */
} cart_dense_ego_params;
void cart_dense_ego_default_params(cart_dense_ego_params *p); /* extension: 1.0, 2.0, 1.0, 1.0, 4, 1, 1024 (build-owned, untuned) */
#define CART_DENSE_EGO_MAX_ITERATIONS 16
typedef struct cart_dense_ego_result {
    double R[9], t[3];                        /* the pose after `steps` updates; rel0's when status is 0 */
    double rms_initial, rms;                  /* sqrt(sum e2 / n) at rel0 and at (R, t) */
    int32_t status;                           /* 1 iff steps > 0 */
    int32_t n_candidates;                     /* the pose-independent count */
    int32_t n_initial, n_inliers;             /* contributing pixels at rel0 and at (R, t) */
    int32_t steps, reserved;
} cart_dense_ego_result;

typedef struct cart_dense_ego cart_dense_ego;
/* Extension.  The workspace for frames of up to max_width x max_height (1..16384 each): one row partial per image row and the pose
 * state; nothing is allocated per call.  The sizes are checked before the engine. */
int cart_dense_ego_create(cart_engine *engine, int max_width, int max_height, cart_dense_ego **out);
/* Extension.  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_dense_ego_destroy(cart_dense_ego *obj);
/* Extension.  One frame: rel0 = HOST double [12] as cart_motion_segment's rel (all finite, |R entries| <= 2, |t entries| <= 1e6);
 * disp_cur / disp_prev = device int16 x16 (2-byte aligned), flow = device int16 x 2 in S10.5 (4-byte aligned), mask = device u8 labels
 * of cart_motion_segment or NULL, all width x height (1..16384 each and within the object's maxima), steps in bytes and multiples of
 * the alignment.  result = DEVICE record (8-byte aligned, overlapping no input).  Checked in this order, all before any device call:
 * params, camera, rel0, sizes, object, then pointers, alignment and steps; a refused call touches no output.  2 (iterations + 1) plain
 * launches on `stream`, no host synchronisation: the pose stays on the device between them, and after a stop the later launches leave
 * at once. */
int cart_dense_ego_refine(cart_dense_ego *obj, const cart_ego_camera *camera, const double *rel0, const cart_dense_ego_params *params,
                          const int16_t *disp_cur, size_t disp_cur_step, const int16_t *disp_prev, size_t disp_prev_step,
                          const int16_t *flow, size_t flow_step, const uint8_t *mask, size_t mask_step, int width, int height,
                          cart_dense_ego_result *result, void *stream);

/* ---- Place recognition over an ORB keyframe database (spec S27) --------------------------------------------------
 * An extension: the reference has no such stage.  A device-resident ring of stored frames (descriptors, keypoints, optional landmarks)
 * and one call that scores the current frame's descriptors against every stored frame.  Integer and deterministic, restated in
 * tests/np_place.py.
 *   Ring: `capacity` slots of up to max_features features; insert number m (from 0 since create / clear) replaces slot m mod capacity.
 *   Eligible: slot k is occupied and frame_id_k + min_gap <= frame_id of the query (uint64; a sum that wraps is not eligible).
 *   Vote: for query i < nq, (j1, d1, d2) = S22's forward record over all j < n_k without a gate; i votes for k iff j1 >= 0, d1 <=
 *   max_distance and (ratio == 0 or d2 < 0 or 100 d1 < ratio d2).  No cross-check.  score_k = the number of votes (0 for an empty slot).
 *   scores[k] = score_k for an eligible slot, -1 for every other slot below capacity.
 *   Candidates: the eligible slots with score >= min_score under (score descending, frame id ascending, slot ascending), the first
 *   max_candidates of them. */
typedef struct cart_place_params {
    int32_t max_distance;                     /* 0..256 */
    int32_t ratio;                            /* 0..100, 0 = off */
    int32_t min_score;                        /* 0..65536 */
    int32_t max_candidates;                   /* 1..16 */
    uint64_t min_gap;                         /* frames between a stored frame and a query that may find it */
} cart_place_params;
void cart_place_default_params(cart_place_params *p); /* extension: 64, 80, 30, 4, 50 (build-owned, untuned) */
#define CART_PLACE_MAX_CAPACITY 1024
#define CART_PLACE_MAX_CANDIDATES 16
typedef struct cart_place_candidate {
    int32_t slot, score;
    uint64_t frame_id;
} cart_place_candidate;

typedef struct cart_place_db cart_place_db;
/* Extension.  The ring and the query's workspace for max_features in 1..65536 and capacity in 1..1024, all allocated here: 92 bytes
 * (32 descriptor + 28 keypoint + 32 landmark) x max_features x capacity, 16 bytes per slot and a partial table of 4 bytes x capacity x
 * ceil(max_features / 128).  The sizes are checked before the engine. */
int cart_place_create(cart_engine *engine, int max_features, int capacity, cart_place_db **out);
/* Extension.  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_place_destroy(cart_place_db *db);
/* Extension.  Empties every slot on `stream`; the next insert is number 0. */
int cart_place_clear(cart_place_db *db, void *stream);
/* Extension.  Stores a frame: desc = device rows of 32 bytes desc_step (>= 32) apart, kp = device cart_keypoint records (4-byte
 * aligned), landmarks = device double [..][4] as cart_ego_triangulate writes them (8-byte aligned) or NULL, count = DEVICE int32,
 * clamped to [0, max_features] on the device; rows at or beyond it are never read.  slot_out (HOST, may be NULL) = the slot taken.
 * One launch on `stream`, no host synchronisation; the slot's header (count, frame id) is written by that launch, so a query queued
 * behind it sees the frame and a query queued before it does not. */
int cart_place_insert(cart_place_db *db, const uint8_t *desc, size_t desc_step, const cart_keypoint *kp, const double *landmarks,
                      const int32_t *count, uint64_t frame_id, int32_t *slot_out, void *stream);
/* Extension.  Scores the query set (q_desc rows q_step >= 32 bytes apart, q_count = DEVICE int32 clamped to [0, max_features]) of
 * frame frame_id against every slot.  Device outputs: scores = int32 [capacity] (may be NULL), candidates = [params->max_candidates]
 * records (8-byte aligned) of which the first *n_candidates are written, n_candidates = their number.  No output may overlap another
 * or the query descriptors, whose extent this check takes as max_features rows whatever the count.  Checked in this order, all before any device call: params, object, then pointers, alignment and steps; a
 * refused call touches no output.  Two launches on `stream` whatever the capacity, no host synchronisation. */
int cart_place_query(cart_place_db *db, const cart_place_params *params, const uint8_t *q_desc, size_t q_step, const int32_t *q_count,
                     uint64_t frame_id, int32_t *scores, cart_place_candidate *candidates, int32_t *n_candidates, void *stream);
/* Extension.  HOST getter, no device work: device pointers into slot `slot` -- its descriptor rows (32 bytes apart), keypoints,
 * landmarks (NULL if the insert gave none) and count -- for cart_matcher_match and cart_ego_estimate; each of the four may be NULL (not
 * asked for).  They stay valid until the object is destroyed and describe the stored frame until the slot is overwritten or
 * cleared.  Fails for a slot that no insert has taken since create / clear. */
int cart_place_slot(cart_place_db *db, int slot, const uint8_t **desc, const cart_keypoint **kp, const double **landmarks,
                    const int32_t **count);

/* ---- Temporal disparity fusion through ego-motion (spec S28) ------------------------------------------------------
 * An extension: the reference has no such stage.  The previous call's fused disparity is forward-projected through the relative pose
 * into a z-buffer of this frame and fused with this frame's disparity; an age channel counts how long a pixel's depth has been
 * confirmed.  No optical flow.  fp64 with + - * / floor only (ceil(a) = -floor(-a)), every sum in the written order, integers after
 * the projection, the only atomics are integer maxima and counter additions: restated in tests/np_fusion.py.
 *   Source: previous pixel (xp, yp) with a_p = prev_age >= 1, s_p = prev_disp != -32768, d_p = s_p / 16.0 >= min_disparity and
 *   mask_prev absent or != 1.  Zp, Xp, Yp and q as S25's gate 4, q.z > 0; u = (fx q.x) / q.z + cx, v = (fy q.y) / q.z + cy,
 *   sw = floor(((fx baseline) / q.z) 16.0 + 0.5), kept iff 1 <= sw <= 32767 (as doubles; a NaN drops the source).
 *   Targets: columns x0 = ceil(u - r) and x1 = floor(u + r) (once when they are equal, none when x0 > x1), rows y0, y1 from v likewise,
 *   r = splat_radius; each is tested against the image as a double before it is converted.  To every target (x, y) inside the image:
 *     key = ((sw >> 4) << 16) | (c << 12) | ((sw & 15) << 8) | a_p,  c = 15 - min(15, floor(16 max(|x - u|, |y - v|)))
 *   and the z-buffer (uint32 per pixel, 0 = empty) keeps the maximum key: the whole-pixel disparity decides occlusion, then the
 *   closeness to the pixel centre, then the fraction, then the age.
 *   Fusion at (x, y): P = the z-buffer key, 0 where mask_cur == 1; s_w = ((P >> 16) << 4) | ((P >> 8) & 15), a_w = P & 255; the current
 *   pixel is valid iff s_c = disp_cur != -32768 and s_c / 16.0 >= min_disparity.
 *     valid, P == 0                                   -> fused s_c, age 1, source 1 (MEASURED)
 *     valid, e = (double)(s_c - s_w) / 16.0, e e <= agree_threshold^2
 *                                                     -> fused (w s_w + s_c + (w + 1) / 2) / (w + 1) in integer division with
 *                                                        w = min(a_w, max_weight), age min(a_w + 1, 255), source 2 (AGREED)
 *     valid, otherwise                                -> fused s_c, age 1, source 3 (REPLACED)
 *     invalid, P != 0, a_w >= min_age                 -> fused s_w, age a_w - 1, source 4 (PREDICTED)
 *     else                                            -> fused s_c unchanged, age 0, source 0 (NONE) */
typedef struct cart_fusion_params {
    double min_disparity;                     /* pixels, finite, > 0 */
    double agree_threshold;                   /* pixels, finite, > 0 */
    double splat_radius;                      /* pixels, finite, 0.5 <= r < 1 */
    int32_t max_weight;                       /* 1..255 */
    int32_t min_age;                          /* 1..255 */
} cart_fusion_params;
void cart_fusion_default_params(cart_fusion_params *p); /* extension: 1.0, 1.0, 0.75, 4, 2 (build-owned, untuned) */
#define CART_FUSION_NONE 0
#define CART_FUSION_MEASURED 1
#define CART_FUSION_AGREED 2
#define CART_FUSION_REPLACED 3
#define CART_FUSION_PREDICTED 4

typedef struct cart_fusion cart_fusion;
/* Extension.  The z-buffer (4 bytes per pixel) and the counters for frames of up to max_width x max_height (1..16384 each), zeroed
 * here once: every call leaves them all zero again.  The sizes are checked before the engine. */
int cart_fusion_create(cart_engine *engine, int max_width, int max_height, cart_fusion **out);
/* Extension.  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_fusion_destroy(cart_fusion *obj);
/* Extension.  One frame, width x height (1..16384 each and within the object's maxima), every image the caller's device memory with its
 * step in bytes.  rel = HOST double [12] as cart_motion_segment's (all finite, |R entries| <= 2, |t entries| <= 1e6); it may be NULL
 * only when prev_disp and prev_age are.  disp_cur = int16 x16; prev_disp (int16 x16) and prev_age (u8) = the previous call's fused and
 * age, both NULL for a frame without a predecessor (nothing is predicted, mask_prev is not read, one launch); mask_prev / mask_cur =
 * u8 labels of cart_motion_segment or NULL.  Outputs: fused int16 x16, age u8, source u8 (may be NULL), counts = DEVICE int32 [5], the
 * pixels per source class (4-byte aligned, may be NULL).  int16 images and their steps are 2-byte aligned.  No output may overlap
 * another output or an input: each such pair is refused by name.  Checked in this order, all before any device call: params, camera,
 * rel, sizes (also against the object's), object, then pointers, alignment, steps and overlaps; a refused call touches no output.  At
 * most two plain launches on `stream`, no host synchronisation. */
int cart_fusion_update(cart_fusion *obj, const cart_ego_camera *camera, const double *rel, const cart_fusion_params *params,
                       const int16_t *disp_cur, size_t disp_cur_step, const int16_t *prev_disp, size_t prev_disp_step,
                       const uint8_t *prev_age, size_t prev_age_step, const uint8_t *mask_prev, size_t mask_prev_step,
                       const uint8_t *mask_cur, size_t mask_cur_step, int width, int height, int16_t *fused, size_t fused_step,
                       uint8_t *age, size_t age_step, uint8_t *source, size_t source_step, int32_t *counts, void *stream);

/* ---- Pose-graph optimisation over keyframes (spec S29) -------------------------------------------------------------
 * An extension: the reference optimises no trajectory.  Nodes are camera-to-world poses (3 x 4, KITTI row order) in insertion order,
 * odometry edges join consecutive nodes, loop edges any two; Gauss-Newton over all nodes but node 0 with an exact step: the odometry
 * edges give a block-tridiagonal matrix that is factored in node order, the loop edges enter as a low-rank term (Woodbury).  fp64 with
 * + - * / sqrt only, every sum in one written order, no atomics: restated in tests/np_posegraph.py, byte for byte.
 *   Node n: odom_n = the pose handed in, est_n = the estimate; est_0 = odom_0 and never moves; est_n = est_{n-1} (odom_{n-1}^-1 odom_n)
 *   at insertion, inv = (R^T, -(R^T t)).
 *   Edge (a, b, M = (R_m, t_m), w_rot, w_trans): p_b = R_m p_a + t_m (cart_ego_result's convention).  The odometry edge (n-1, n) has
 *   M = odom_n^-1 odom_{n-1} and the weights given with node n.
 *   Residual: E = M (est_a^-1 est_b) = (R_e, t_e), rho = 0.5 (R_e[2,1] - R_e[1,2], R_e[0,2] - R_e[2,0], R_e[1,0] - R_e[0,1]), tau = t_e;
 *   cost = sum over the edges, odometry first, of w_rot rho.rho + w_trans tau.tau (S23's 256 virtual lanes).
 *   Update: R_i <- R_i Rq(omega_i), t_i <- t_i + R_i upsilon_i with S23's Rq.  The Jacobians, the step and every operation order:
 *   DESIGN.md 7.11.  A pivot that is not > 0 in either factorisation ends the call with status 0 and every estimate as it was. */
typedef struct cart_pose_graph_params {
    int32_t iterations;                       /* 0..16 Gauss-Newton steps, no early exit */
} cart_pose_graph_params;
void cart_pose_graph_default_params(cart_pose_graph_params *p); /* extension: 4 (build-owned) */
#define CART_POSE_GRAPH_MAX_NODES 4096
#define CART_POSE_GRAPH_MAX_LOOPS 64
#define CART_POSE_GRAPH_MAX_ITERATIONS 16
typedef struct cart_pose_graph_result {
    int32_t status;                           /* 1 = optimised (or nothing to do), 0 = a pivot was not > 0: nothing moved */
    int32_t n_nodes, n_loops, iterations;     /* what the call saw */
    double cost_before, cost_after;           /* both 0 for a graph without an edge; cost_after = cost_before with status 0 */
} cart_pose_graph_result;

typedef struct cart_pose_graph cart_pose_graph;
/* Extension.  Everything for max_nodes in 1..4096 and max_loops in 0..64 is allocated here: 96 + 96 + 96 bytes per node (odom, estimate,
 * snapshot), 128 per edge, 960 + 640 per node for the linearisation and the factor, the column workspace of max_nodes x 6 x (1 + 6
 * max_loops) doubles (19 MB at 1024 / 64) and the loop system, about 2 (6 max_loops + 1)^2 doubles.  The sizes are checked before the engine. */
int cart_pose_graph_create(cart_engine *engine, int max_nodes, int max_loops, cart_pose_graph **out);
/* Extension.  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_pose_graph_destroy(cart_pose_graph *pg);
/* Extension.  Forgets every node and loop; ordered on `stream` like every other call.  The object is stateful in call order. */
int cart_pose_graph_clear(cart_pose_graph *pg, void *stream);
/* Extension.  HOST getter, no device work: the node and loop counts (either pointer may be NULL). */
int cart_pose_graph_size(cart_pose_graph *pg, int *nodes, int *loops);
/* Extension.  Appends a node: pose = HOST double [12] (all finite, |R entries| <= 2, |t entries| <= 1e6), the weights of the odometry
 * edge to the previous node finite and > 0 (checked for node 0 too, where they are not used).  node_out (HOST, may be NULL) = its index.
 * The pose travels as kernel arguments: one launch on `stream`, no host synchronisation.  A full table is refused and touches nothing. */
int cart_pose_graph_add_node(cart_pose_graph *pg, const double *pose, double w_rot, double w_trans, int32_t *node_out, void *stream);
/* Extension.  Appends the loop edge (a, b, (R, t)) with p_b = R p_a + t: R = HOST double [9], t = HOST double [3], all finite; a != b,
 * both below the node count; weights finite and > 0.  One launch, no host synchronisation.  A full loop table is refused. */
int cart_pose_graph_add_loop(cart_pose_graph *pg, int a, int b, const double *R, const double *t, double w_rot, double w_trans, void *stream);
/* Extension.  params->iterations Gauss-Newton steps over the graph as it stands.  result = DEVICE record (8-byte aligned) or NULL.
 * One launch on `stream` whatever the node and loop counts, no host synchronisation.  Checked in this order, all before any device
 * call: params, object, then the pointer. */
int cart_pose_graph_optimize(cart_pose_graph *pg, const cart_pose_graph_params *params, cart_pose_graph_result *result, void *stream);
/* Extension.  Copies the estimates of nodes [first, first + count) as 12 doubles each to out = DEVICE memory (8-byte aligned) on `stream`;
 * count = 0 copies nothing. */
int cart_pose_graph_poses(cart_pose_graph *pg, int first, int count, double *out, void *stream);
/* Extension.  The same into HOST memory, after every call queued on the object so far; synchronises.  For tests and dumps. */
int cart_pose_graph_read(cart_pose_graph *pg, int first, int count, double *out_host);

/* ---- Moving-object tracks from the motion components (spec S31) ----------------------------------------------------
 * An extension: the reference has no such stage.  Every MOVING component of cart_plane_ccl_table (run on the labels of
 * cart_motion_segment) that is large enough becomes an object: where its surface is in metres, how large, which way and how fast it
 * moves beyond the camera's own motion, and, through a small tracker in the world frame, that it is the object of the last frame.
 * fp64 with + - * / floor only, every expression in the written order, the only atomics are integer additions, minima and maxima:
 * restated in tests/np_objects.py, byte for byte.
 *   Selection: table entries k = 0 .. min(n_components, max_components) - 1 in table order; entry k is selected iff label == 1 and
 *   area >= min_area; the j-th selected entry is object j, objects j >= max_objects are dropped (n_selected keeps the true count).
 *   Pass 1: a pixel whose id is object j's contributes iff s_c = disp_cur != -32768 and s_c / 16.0 >= min_disparity; it adds one to bin
 *   min(s_c >> 4, 511) of the object's histogram (CART_OBJECT_BINS bins).  n_hist = the total, B_j = the smallest bin whose cumulative
 *   count is >= (n_hist + 1) >> 1, -1 at n_hist = 0.
 *   Pass 2: with band16 = (int)floor(disparity_band 16.0), a pixel of object j that passes pass 1's gate is a point iff
 *   |s_c - (16 B_j + 8)| <= band16.  A point: P = back-projection of (x, y, s_c / 16.0) as S25's; n_points += 1, sum[i] += Qp(P_i),
 *   lo[i] / hi[i] = min / max of Qp(P_i), the pixel box x0..y1 grows; Qp(v) = (int64) clamp(floor(v 1024.0 + 0.5), -2147483647,
 *   2147483647), a NaN gives the lower bound.  The point carries flow iff S25's gates 2-4 pass ((xp, yp) = p - (flow >> 5) inside the
 *   image, disp_prev there valid and >= min_disparity, q = rel applied to the previous point with q.z > 0) and f = P - q has
 *   (f.x f.x + f.y f.y) + f.z f.z <= max_speed max_speed; then n_flow += 1, flow_sum[i] += Qp(f_i).
 *   Derive: valid = n_points >= min_points; c_i = ((double)sum[i] / 1024.0) / (double)n_points, centroid = pose applied to c,
 *   extent_i = (double)(hi[i] - lo[i]) / 1024.0 (camera axes); has_velocity = valid and n_flow >= min_points, v_i = ((double)flow_sum[i]
 *   / 1024.0) / (double)n_flow, velocity[r] = (pose[4r] v.x + pose[4r+1] v.y) + pose[4r+2] v.z (world, metres per frame).  The three
 *   of an invalid object, and the velocity of one without, are +0.0.
 *   Tracks (max_tracks slots, state 0 = free, a device next_id that starts at 1), per frame over the valid objects and live tracks:
 *   pred = position + velocity; d2 = (dx dx + dy dy) + dz dz between centroid and pred (d = centroid - pred), admissible iff d2 <=
 *   gate gate; greedy: the admissible pair with both ends free and the smallest d2 is matched, ties to the smaller slot, then the
 *   smaller object, until none is left.  Matched: m = has_velocity ? the object's velocity : centroid - position (the old one),
 *   velocity += g (m - velocity) with g = gain_percent / 100.0, position = centroid, extent = the object's, age += 1, missed = 0,
 *   object / component set, state = age >= min_age ? 2 : 1.  Unmatched: position = pred, missed += 1, object = component = -1, freed
 *   when missed > max_missed.  Then every unmatched valid object in ascending index takes the lowest free slot (those just freed
 *   included): id = next_id++, age 1, missed 0, state = min_age <= 1 ? 2 : 1, velocity the object's (or 0); without a free slot it is
 *   dropped and counted. */
#define CART_OBJECT_BINS 512
#define CART_OBJECT_MAX_OBJECTS 256
#define CART_OBJECT_MAX_TRACKS 256
typedef struct cart_object_params {
    double min_disparity;                     /* pixels, finite, > 0 */
    double disparity_band;                    /* pixels, finite, 0.5..64 */
    double max_speed;                         /* metres per frame, finite, > 0 */
    double gate;                              /* metres, finite, > 0 */
    int32_t min_area;                         /* pixels of a component, 1..2^30 */
    int32_t min_points;                       /* 1..2^30 */
    int32_t gain_percent;                     /* 0..100 */
    int32_t max_missed;                       /* 0..255 */
    int32_t min_age;                          /* 1..255 */
} cart_object_params;
/* Extension (S31): 1.0, 2.0, 5.0, 2.0, 64, 16, 50, 3, 3 (build-owned, no data set has tuned them). */
void cart_object_default_params(cart_object_params *p);
typedef struct cart_object {                  /* S31; 192 bytes, 8-byte aligned */
    int32_t component, area;                  /* the table entry's id and area */
    int32_t x0, y0, x1, y1;                   /* the pixel box of the object's POINTS, inclusive (not the table's box, which holds the
                                                 occlusion rim as well); 0, 0, -1, -1 without a point */
    int32_t median_bin, n_hist, n_points, n_flow;
    int32_t lo[3], hi[3];                     /* of Qp(P_i); all 0 without a point */
    int64_t sum[3], flow_sum[3];
    double centroid[3], velocity[3], extent[3];   /* world, world per frame, camera axes */
    int32_t valid, has_velocity;
} cart_object;
typedef struct cart_track {                   /* S31; 96 bytes, 8-byte aligned */
    uint32_t id;                              /* 0 in a free slot; never repeats */
    int32_t state;                            /* 0 free, 1 tentative, 2 confirmed */
    int32_t age, missed;
    int32_t object, component;                /* this frame's object index and its component id, -1 when unmatched or free */
    double position[3], velocity[3], extent[3];
} cart_track;

typedef struct cart_object_tracker cart_object_tracker;
/* Extension (S31).  The histograms, the accumulators, the id -> object scratch image (4 bytes per pixel) and the tracks for frames of up
 * to max_width x max_height (1..16384 each), max_objects and max_tracks in 1..256; no call allocates.  The sizes are checked before the
 * engine. */
int cart_object_tracker_create(cart_engine *engine, int max_width, int max_height, int max_objects, int max_tracks, cart_object_tracker **out);
/* Extension (S31).  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_object_tracker_destroy(cart_object_tracker *obj);
/* Extension (S31).  Frees every track and sets next_id = 1; ordered on `stream` like every other call. */
int cart_object_tracker_reset(cart_object_tracker *obj, void *stream);
/* Extension (S31).  One frame, width x height (1..16384 each and within the object's maxima), every image the caller's device memory
 * followed by its step in bytes: ids = the int32 image and table = the DEVICE cart_component [max_components] of cart_plane_ccl_table
 * run on cart_motion_segment's labels, n_components = its DEVICE int32 count (it may exceed max_components; max_components >= 1);
 * disp_cur / disp_prev int16 x16, flow int16 x2 in S10.5 as cart_motion_segment's.  rel = HOST double [12] as cart_motion_segment's,
 * pose = HOST double [12], camera-to-world of this frame as cart_plane_map_update's.  Outputs: objects_out = DEVICE cart_object
 * [max_objects] (rows past the frame's objects all zero; may be NULL), tracks_out = DEVICE cart_track [max_tracks], every slot,
 * counts_out = DEVICE int32 [8]: {table entries walked, n_selected, n_objects, n_valid, n_matched, n_born, n_dropped, n_live}.  The
 * records are 8-byte aligned, counts_out and the int32 inputs 4-byte.  No output may overlap another output or an input: each such pair
 * is refused by name.  Checked in this order, all before any device call: params, camera, rel, pose, sizes, object (and the sizes
 * against it), then pointers, alignment, steps and overlaps; a refused call launches nothing and touches no output or track.  Five
 * plain launches on `stream`, no host synchronisation. */
int cart_object_tracker_update(cart_object_tracker *obj, const cart_ego_camera *camera, const double *rel, const double *pose,
                               const cart_object_params *params, const int32_t *ids, size_t ids_step, const cart_component *table,
                               int max_components, const int32_t *n_components, const int16_t *disp_cur, size_t disp_cur_step,
                               const int16_t *disp_prev, size_t disp_prev_step, const int16_t *flow, size_t flow_step, int width, int height,
                               cart_object *objects_out, cart_track *tracks_out, int32_t *counts_out, void *stream);

/* ---- Windowed bundle adjustment over the last frames (spec S32) -------------------------------------------------
 * An extension: the reference refines no trajectory.  The object keeps the last `window` frames (their camera-to-world poses as handed
 * in and as estimated), the points those frames share and one stereo observation (u, v, u_right) per point and frame.  push() builds
 * the tracks from the frame's keypoints and match lists (integer logic and one back-projection per new point); optimize() runs
 * Gauss-Newton with a Huber weight over the poses of all frames but the oldest and over every point with enough observations: the
 * points are eliminated (Schur complement), the reduced system of order 6 (frames - 1) <= 90 is solved by an unpivoted Cholesky.  fp64
 * with + - * / sqrt only, every sum in one written order (S23's 256 virtual lanes over the point slots), no floating-point atomics:
 * restated in tests/np_localba.py, byte for byte.
 *   Ring: push number n (from 0 after a clear) goes to slot n mod window; a full ring drops the frame in that slot (no marginalisation)
 *   and frees every point that loses its last observation.  est_new = est_prev (odom_prev^-1 odom_new) with S29's products.
 *   Observation of left index i with stereo match (i, j): u = kpL[i].x, v = kpL[i].y, ur = kpR[j].x, valid iff (double)u - (double)ur >=
 *   min_disparity.  i continues point p iff it has a valid observation, a temporal match (i, j) and track_of_prev[j] = p is alive; of
 *   several i that name one p the smallest wins.  Every other valid i is a new point: ascending i take the free slots in ascending
 *   order, X = est_new applied to the back-projection of (u, v, u - ur); without a free slot the keypoint is dropped.
 *   Residual of X in a frame with est = (R, t): q = R^T (X - t), skipped unless q.z > 0; eu = ((fx q.x) / q.z + cx) - u, ev likewise,
 *   er = ((fx (q.x - baseline)) / q.z + cx) - ur; n2 = (eu eu + ev ev) + er er; w = 1 where n2 <= huber^2, else huber / sqrt(n2).
 *   Update: R <- R Rq(omega), t <- t + R upsilon (S29's), X <- X + dX.  The Jacobians, the elimination, the held frames and every
 *   operation order: DESIGN.md 7.14.  A pivot of the reduced system that is not > 0 ends the call with status 0 and everything as it was. */
typedef struct cart_local_ba_params {
    double min_disparity;                     /* pixels, finite, > 0: S23's test of a stereo observation */
    double huber;                             /* pixels, finite, > 0 */
    double damping;                           /* finite, >= 0: added to every diagonal entry of the pose and the point blocks */
    int32_t iterations;                       /* 0..16 Gauss-Newton steps, no early exit */
    int32_t min_observations;                 /* 1..16: a point with fewer observations in the window neither contributes nor moves */
    int32_t min_frame_observations;           /* 0..65536: a free frame with fewer usable observations in a step is held for that step */
} cart_local_ba_params;
/* Extension (S32): 1.0, 2.0, 0.0, 4, 2, 6 (build-owned, no data set has tuned them). */
void cart_local_ba_default_params(cart_local_ba_params *p);
#define CART_LOCAL_BA_MAX_WINDOW 16
#define CART_LOCAL_BA_MAX_POINTS 65536
#define CART_LOCAL_BA_MAX_ITERATIONS 16
typedef struct cart_local_ba_result {         /* S32; 40 bytes, 8-byte aligned */
    int32_t status;                           /* 1 = optimised (or nothing to do), 0 = a pivot was not > 0: nothing moved */
    int32_t n_frames, n_points_active;        /* frames in the window; points with >= min_observations observations */
    int32_t n_observations;                   /* observations of those points with q.z > 0, before the first step */
    int32_t n_held;                           /* held frames, added up over the steps */
    int32_t iterations;
    double cost_before, cost_after;           /* sum of the Huber costs; cost_after = cost_before with status 0 or nothing to do */
} cart_local_ba_result;

typedef struct cart_local_ba cart_local_ba;
/* Extension (S32).  Everything for keypoint lists of up to max_features (1..65536), window in 2..16 frames and max_points in 64..65536
 * is allocated here: per point 16 window bytes of observations, 48 for the position and its snapshot, 96 for the blocks of a step and
 * 20 of bookkeeping (2.4 MB at 8 / 8192, 28 MB at 16 / 65536), 28 bytes per feature, 392 per frame and the reduced system of at most
 * 91 x 90 doubles.  No call allocates.  The sizes are checked before the engine. */
int cart_local_ba_create(cart_engine *engine, int max_features, int window, int max_points, cart_local_ba **out);
/* Extension (S32).  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_local_ba_destroy(cart_local_ba *ba);
/* Extension (S32).  Forgets every frame and point; ordered on `stream` like every other call.  The object is stateful in call order. */
int cart_local_ba_clear(cart_local_ba *ba, void *stream);
/* Extension (S32).  HOST getter, no device work: the frames in the window and max_points (either pointer may be NULL). */
int cart_local_ba_size(cart_local_ba *ba, int *frames, int *points_capacity);
/* Extension (S32).  One frame: pose = HOST double [12], camera-to-world (all finite, |R entries| <= 2, |t entries| <= 1e6); kpL / kpR
 * = the cart_keypoint records of the left and right image, left_count = the number of left keypoints, stereo_matches with query =
 * left, train = right, temporal_matches with query = this frame's left, train = the previously pushed frame's left, both with
 * distinct queries (what cart_matcher_match writes); all DEVICE memory, 4-byte aligned, the counts DEVICE int32 clamped to [0,
 * max_features]; a match with an index outside [0, left_count) x [0, max_features) is ignored.  The first push after a clear ignores
 * the temporal list.  counts_out = DEVICE int32 [8] or NULL: {left keypoints, stereo-valid, continued, born, dropped, freed, live
 * points, frames in window}; it may overlap no input.  Of params only min_disparity is used, all are checked.  Checked in this order,
 * all before any device call: params, camera, pose, object, then pointers, alignment and overlaps; a refused call launches nothing and
 * touches no state.  Four launches on `stream`, no host synchronisation. */
int cart_local_ba_push(cart_local_ba *ba, const cart_ego_camera *camera, const cart_local_ba_params *params, uint64_t frame_id,
                       const double *pose, const cart_keypoint *kpL, const cart_keypoint *kpR, const int32_t *left_count,
                       const cart_match *stereo_matches, const int32_t *stereo_count, const cart_match *temporal_matches,
                       const int32_t *temporal_count, int32_t *counts_out, void *stream);
/* Extension (S32).  params->iterations Gauss-Newton steps over the window as it stands.  result = DEVICE record (8-byte aligned) or
 * NULL.  2 + 5 iterations launches on `stream` whatever the counts, no host synchronisation.  Checked in this order: params, camera,
 * object, then the pointer. */
int cart_local_ba_optimize(cart_local_ba *ba, const cart_ego_camera *camera, const cart_local_ba_params *params,
                           cart_local_ba_result *result, void *stream);
/* Extension (S32).  The window in age order, oldest first: out = DEVICE double [window][12] (8-byte aligned), ids_out = DEVICE uint64
 * [window] (8-byte aligned, may be NULL); rows past the frames in the window are zero.  The two may not overlap. */
int cart_local_ba_poses(cart_local_ba *ba, double *out, uint64_t *ids_out, void *stream);
/* Extension (S32).  Every point slot: out = DEVICE double [max_points][4] (8-byte aligned) = (X, Y, Z, n_obs), zeros in a free slot. */
int cart_local_ba_points(cart_local_ba *ba, double *out, void *stream);
/* Extension (S32).  The point slot of every left index of the newest frame, -1 without: out = DEVICE int32 [max_features] (4-byte
 * aligned). */
int cart_local_ba_track_of(cart_local_ba *ba, int32_t *out, void *stream);

/* ---- Rolling TSDF voxel map with model raycast (spec S33) ----------------------------------------------------------
 * An extension: the reference keeps no three-dimensional model.  A rolling window of Nx x Ny x Nz voxels in the world frame; every
 * frame's disparity is averaged into it as a truncated signed distance through the frame's camera-to-world pose, and a raycast from any
 * pose gives a model disparity in the format of the disparity image.  fp64 with + - * / floor only, every expression in the written
 * order, integers after the projection, no floating-point atomic and no atomic on the volume (one lane owns a voxel for a whole call):
 * restated in tests/np_voxelmap.py, byte for byte.
 *   Voxel: {int16 tsdf (units of 1 / 32767 of the truncation distance), uint16 weight}, empty = (0, 0).  Global voxel g is stored at
 *   (gx mod Nx, gy mod Ny, gz mod Nz) (floor modulo), x fastest, whatever the window: a window move copies nothing.
 *   Window (host, int64, floor division): c_a = floor((t_a + lookahead P[4a + 2]) / voxel_size) per axis a (t_a = P[4a + 3]; the third
 *   column of R is the optical axis), o_a = 8 floor_div(c_a - N_a / 2, 8).  The first integrate after create / clear starts at o with every
 *   voxel empty; afterwards the voxels that enter are emptied before the frame is integrated and those that leave are forgotten; a move
 *   of >= N_a on an axis empties everything.
 *   Integrate, for every voxel g of the new window, the gates in this order:
 *     1. p_a = ((double)g_a + 0.5) voxel_size, d = p - t, q_c = (P[c] d_0 + P[4 + c] d_1) + P[8 + c] d_2; q_z >= min_depth
 *     2. u = (fx q_x) / q_z + cx, v = (fy q_y) / q_z + cy, x = floor(u + 0.5), y = floor(v + 0.5), both inside the image (compared as
 *        doubles before the conversion; a NaN fails)
 *     3. s = disp[y][x] != -32768, d = s / 16.0 >= min_disparity, Z = (fx baseline) / d <= max_depth, mask absent or mask[y][x] != 1
 *     4. tr = truncation + disparity_sigma ((Z Z) / (fx baseline)), sdf = Z - q_z >= -tr
 *     5. f = sdf / tr, 1.0 where it is larger; obs = (int)floor(f 32767.0 + 0.5)
 *     6. with the stored (t, w), in int64: t' = floor_div(2 (w t + obs) + (w + 1), 2 (w + 1)), w' = min(w + 1, max_weight)
 *   A voxel that fails a gate is neither read nor written.
 *   Raycast of pixel (x, y): K = (int)floor((max_depth - min_depth) / march_step); for k = 0..K, z_k = min_depth + (double)k march_step,
 *   X = ((x - cx) z_k) / fx, Y = ((y - cy) z_k) / fy, p_w[r] = ((P[4r] X + P[4r+1] Y) + P[4r+2] z_k) + P[4r+3]; per axis a = p_w /
 *   voxel_size - 0.5, i0 = floor(a), fr = a - i0.  The sample is known iff a window exists, all eight corners i0 + {0,1}^3 lie in it
 *   (compared as doubles) and each has weight >= min_weight.  F = trilinear in fp64 of the eight tsdf integers: along x
 *   c = t0 + fr_x (t1 - t0) (the difference in integers), then e0 = c[0][0] + fr_y (c[1][0] - c[0][0]), e1 = c[0][1] + fr_y (c[1][1] -
 *   c[0][1]) with c[dy][dz], then F = e0 + fr_z (e1 - e0).  An unknown sample forgets the previous one; a known F <= 0 after a known
 *   previous F_p > 0 is a hit at z* = z_p + (march_step F_p) / (F_p - F) and ends the ray; a known F <= 0 otherwise ends it as INSIDE;
 *   a known F > 0 becomes the previous sample.  A hit with sw = floor(((fx baseline) / z*) 16.0 + 0.5) in 1..32767 writes sw, status
 *   HIT and the minimum weight of the eight corners of the sample that closed it; an INSIDE ray writes -32768, weight 0, status INSIDE;
 *   every other ray -32768, weight 0, status NONE. */
typedef struct cart_voxel {
    int16_t tsdf;
    uint16_t weight;
} cart_voxel;                                 /* the empty voxel is (0, 0) */
typedef struct cart_voxel_map_params {
    double voxel_size;                        /* metres, finite, >= 0.01 */
    double min_disparity;                     /* pixels, finite, > 0 */
    double min_depth;                         /* metres, finite, > 0 */
    double max_depth;                         /* metres, finite, > min_depth */
    double truncation;                        /* metres, finite, > 0 */
    double disparity_sigma;                   /* pixels, finite, >= 0: the truncation grows by sigma Z^2 / (fx baseline) */
    double lookahead;                         /* metres, finite, |.| <= 1000: the window's centre lies this far along the optical axis */
    double march_step;                        /* metres, finite, 0 < march_step <= truncation, at most 8192 steps */
    int32_t max_weight;                       /* 1..65535 */
    int32_t min_weight;                       /* 1..65535 */
} cart_voxel_map_params;
/* extension: 0.125, 1.0, 0.5, 16.0, 0.25, 0.5, 8.0, 0.125, 64, 1 (build-owned, untuned) */
void cart_voxel_map_default_params(cart_voxel_map_params *p);
#define CART_VOXEL_RAY_NONE 0
#define CART_VOXEL_RAY_HIT 1
#define CART_VOXEL_RAY_INSIDE 2

typedef struct cart_voxel_map cart_voxel_map;
/* Extension.  cells_x, cells_y, cells_z: multiples of 8 in 16..1024 with a product of at most 2^26 (4 bytes per voxel).  The parameters
 * are fixed for the object's life.  Stateful: calls on one object must be issued in frame order.  The sizes and params are checked
 * before the engine, so a configuration can be validated without a device. */
int cart_voxel_map_create(cart_engine *engine, int cells_x, int cells_y, int cells_z, const cart_voxel_map_params *params,
                          cart_voxel_map **out);
/* Extension.  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_voxel_map_destroy(cart_voxel_map *map);
/* Extension.  Forgets the window: the next integrate starts an empty one.  No device work. */
int cart_voxel_map_clear(cart_voxel_map *map);
/* Extension.  HOST getter: origin3 = int64 [3] (absolute voxels, zeros without a window), shape3 = int32 [3] (cells_x, cells_y,
 * cells_z), *valid = 0 after create / clear. */
int cart_voxel_map_window(cart_voxel_map *map, int64_t *origin3, int32_t *shape3, int *valid);
/* Extension.  One frame: pose = HOST double [12] (3 x 4 camera-to-world as cart_plane_map_update's); disp = device int16 x16, mask =
 * device u8 labels of cart_motion_segment or NULL, both width x height (1..16384 each), steps in bytes; counts = DEVICE int32 [2]
 * (4-byte aligned, may be NULL: then no counter is touched) = voxels updated, of them with f < 1.  Moves the window, empties what
 * entered it (at most one launch per axis that moved, or one for the whole grid), integrates (one launch).  Checked in this order, all
 * before any device call: camera, pose, sizes, the object, then pointers, alignment, steps and overlaps (counts against disp and mask); a
 * refused call launches nothing and leaves the window where it was.  No host synchronisation. */
int cart_voxel_map_integrate(cart_voxel_map *map, const cart_ego_camera *camera, const double *pose, const int16_t *disp,
                             size_t disp_step, int width, int height, const uint8_t *mask, size_t mask_step, int32_t *counts,
                             void *stream);
/* Extension.  The model seen from `pose` at width x height: disp_model = device int16 x16; weight_model = device uint16, status =
 * device u8 (CART_VOXEL_RAY_*), counts = DEVICE int32 [3] = rays NONE, HIT, INSIDE; the last three may be NULL.  Reads the volume only:
 * the window does not move.  No output may overlap another: each pair is refused by name.  Checked in the order of
 * cart_voxel_map_integrate.  One launch, no host synchronisation. */
int cart_voxel_map_raycast(cart_voxel_map *map, const cart_ego_camera *camera, const double *pose, int width, int height,
                           int16_t *disp_model, size_t disp_model_step, uint16_t *weight_model, size_t weight_model_step,
                           uint8_t *status, size_t status_step, int32_t *counts, void *stream);
/* Extension.  Test / dump access: synchronises `stream` and copies the window's voxels in window order [cells_z][cells_y][cells_x]
 * into host_voxels (HOST); without a window every voxel is empty and the origin is (0, 0, 0).  origin3 = int64 [3]. */
int cart_voxel_map_read(cart_voxel_map *map, cart_voxel *host_voxels, int64_t *origin3, void *stream);

/* ---- Rebuilding the TSDF volume after a pose correction (spec S35) -------------------------------------------------
 * An extension.  The frames of a cart_plane_store (S30, as it is: the int16 x16 disparity and a u8 plane per keyframe) integrated again,
 * each through a NEW pose, into one fixed window, in one launch.  S33's running average depends on the order of the observations (floor
 * division, and a weight cap that turns the mean into an exponential one), so the order is part of the spec: the caller's list order.
 * S33's arithmetic to the letter; restated in tests/np_voxelmap_rebuild.py, byte for byte.
 *   1. The window origin is S33's Window arithmetic applied to window_pose, with the map's own lookahead and voxel_size.
 *   2. Every voxel of that window starts empty, (0, 0).
 *   3. For k = 0 .. count - 1 in that order, an entry (ids[k], poses[k]) whose id the store holds (looked up newest first) is integrated
 *      into that fixed window by S33's Integrate rule, gates 1 to 6 unchanged, with the map's own params: the image is the stored frame,
 *      width x height of the store; with use_mask = 1 the stored u8 plane is integrate's mask (gate 3 passes where it is != 1), with
 *      use_mask = 0 it is not read.  The window does not move between entries; voxels outside it do not exist.
 *   4. Entries whose id is not in the store are skipped and counted: used = count - skipped.  An id listed twice is integrated twice.
 *      count = 0 leaves an empty valid window at the new origin.
 *   5. counts = the voxel updates summed over all used entries, and how many of them had f < 1.
 * Afterwards the map is valid at that origin; cart_voxel_map_integrate, _raycast, _read and cart_model_track_refine continue on it as
 * after any integrate.  The rebuilt volume equals cart_voxel_map_clear followed by one cart_voxel_map_integrate per used entry in list
 * order, provided every entry's own pose yields the rebuild's window origin.
 *
 * ids = HOST uint64 [count], poses = HOST double [count][12], count in 0..4096, window_pose = HOST double [12]; used_out (HOST, may be
 * NULL); counts = DEVICE int64 [2] (8-byte aligned, may be NULL: then no counter is touched; int64 because 4096 entries x 2^26 voxels pass
 * int32).  Checked in this order, everything up to the objects without a device: count and use_mask, the camera, window_pose and every
 * poses[k], the map, the store (on the map's device), the alignment of counts.  A refused call launches nothing and changes nothing.  The
 * entries travel through the store's pinned buffer as in cart_plane_map_rebuild: the only host synchronisation is the wait for the
 * previous rebuild's upload.  Holds the map, then the store. */
int cart_voxel_map_rebuild(cart_voxel_map *map, cart_plane_store *store, const cart_ego_camera *camera, const uint64_t *ids,
                           const double *poses, int count, const double *window_pose, int use_mask, int *used_out, int64_t *counts,
                           void *stream);

/* ---- Surface mesh of the TSDF volume (spec S36) --------------------------------------------------------------------
 * An extension.  The surface of the current window as an indexed quad mesh with per-vertex normals, by naive surface nets: one vertex per
 * cell the surface passes through, one quad per voxel edge the surface crosses.  S33's arithmetic rules: fp64 with + - * / floor sqrt,
 * every expression in the written association order; no atomic decides where a record lands.  Restated in tests/np_voxelmesh.py, byte
 * for byte.
 *   Cells: with a window of Nx x Ny x Nz voxels at origin o, cell c = (cx, cy, cz) exists for 0 <= c_a <= N_a - 2 (window-local indices:
 *   the window's last and first voxel are not neighbours, although they are adjacent in the toroidal storage).  Its corners are the window
 *   voxels c + (dx, dy, dz), d in {0,1}^3, with corner tsdf t[dy][dz][dx].  mw = the call's min_weight, or the map's own when that is 0.
 *   A cell is known iff all eight corners have weight >= mw; a corner is inside iff tsdf <= 0 (the raycast's F <= 0); a cell is active
 *   iff it is known and its corners are neither all inside nor all outside.
 *   Vertex of an active cell: the twelve cell edges in this order: the four x-edges (dy, dz) = (0,0), (1,0), (0,1), (1,1), the four y-edges
 *   (dx, dz) in the same order, the four z-edges (dx, dy) in the same order.  An edge from corner a (lower) to corner b (upper along its
 *   axis) crosses iff exactly one of them is inside; then f = (double)t_a / (double)(t_a - t_b) (the subtraction in integers, never zero
 *   on a crossing edge), and the edge contributes f along its own axis and (double)d along the other two.  Three sums s_x, s_y, s_z start
 *   at 0.0 and take the contributions in edge order; n counts the crossings.  l_a = s_a / (double)n, p_a = (((double)c_a + 0.5) + l_a)
 *   voxel_size: metres relative to the window origin; the world position is o_a voxel_size + p_a.
 *   Normal: (gx, gy, gz) = the gradient of S34's trilinear sample of the cell's eight corners at fr = (l_x, l_y, l_z); n2 = (gx gx + gy gy)
 *   + gz gz; the normal is g_a / sqrt(n2) where n2 > 0, else (0, 0, 0).  It points towards positive tsdf: free space, the cameras' side.
 *   Vertex record: position and normal, each component the fp64 value converted once to fp32; vertices are ordered by ascending cell index
 *   (cz (Ny - 1) + cy) (Nx - 1) + cx.
 *   Quads: voxel (i, j, k) owns the three edges that leave it in +x, +y, +z, taken in that axis order.  An edge emits a quad iff its upper
 *   voxel is in the window, the edge crosses, and the four cells around it all exist and are known (they are then active):
 *     x-edge: (i, j-1, k-1), (i, j, k-1), (i, j, k), (i, j-1, k)
 *     y-edge: (i-1, j, k-1), (i-1, j, k), (i, j, k), (i, j, k-1)
 *     z-edge: (i-1, j-1, k), (i, j-1, k), (i, j, k), (i-1, j, k)
 *   The record holds the four cells' vertex indices, in the listed order when the lower voxel is inside and reversed (4th, 3rd, 2nd, 1st)
 *   when it is outside: (p2 - p0) x (p3 - p1) then points to free space.  Quads are ordered by ascending (cell index of (i, j, k), axis).
 *   Capacity: the first max_vertices vertices and the first max_quads quads in these orders are written and nothing beyond them is touched;
 *   after a truncation a quad may name a vertex that was not written: a consumer takes the mesh iff found == written for both.
 * Limits: no colour in the records themselves (cart_voxel_color_vertices, S37 below, colours them from a colour volume), no decimation; surface nets round sharp edges and can be non-manifold where two surfaces meet within a cell; a mesh
 * covers the current window only. */
typedef struct cart_mesh_vertex {
    float position[3];                        /* metres, relative to the window origin */
    float normal[3];                          /* unit length, or (0, 0, 0) */
} cart_mesh_vertex;                           /* 24 bytes */
typedef struct cart_mesh_quad {
    int32_t v[4];                             /* vertex indices */
} cart_mesh_quad;
/* Extension.  min_weight = 0 (the map's own) or 1..65535; vertices = DEVICE cart_mesh_vertex [max_vertices], quads = DEVICE cart_mesh_quad
 * [max_quads], both 4-byte aligned, capacities in 1..2^26; counts = DEVICE int32 [4] (4-byte aligned) = vertices found, quads found,
 * vertices written, quads written: all 0 without a window.  origin3 = HOST int64 [3] or NULL: the window origin the mesh belongs to, written
 * under the map's lock as cart_voxel_map_window does (zeros without a window).  Reads the volume only.  Checked in this order, all before
 * any device call: min_weight, the capacities, the object, then pointers, alignment and overlaps (no output may overlap another).  Five
 * launches, no host synchronisation, except that the first call on a map allocates its workspace: one 4-byte word per voxel plus two
 * 4-byte words per 1024 voxels, 4.01 bytes per voxel, as much as the volume itself, kept until the map is destroyed. */
int cart_voxel_map_mesh(cart_voxel_map *map, int min_weight, cart_mesh_vertex *vertices, int max_vertices, cart_mesh_quad *quads,
                        int max_quads, int32_t *counts, int64_t *origin3, void *stream);
/* Extension.  The counterpart of cart_voxel_map_read: host_voxels (HOST, window order [cells_z][cells_y][cells_x]) become the window at
 * origin3 = HOST int64 [3], each component a multiple of 8 with |o_a| <= 2^27 (every origin the window arithmetic can produce).  Checked
 * before any device call: origin3, the object, host_voxels.  Synchronises `stream`, as _read does.  Afterwards the map is valid at that
 * origin; cart_voxel_map_integrate, _raycast, _read, _mesh and cart_model_track_refine continue on it as after any integrate. */
int cart_voxel_map_write(cart_voxel_map *map, const cart_voxel *host_voxels, const int64_t *origin3, void *stream);

/* ---- Colour for the TSDF volume (spec S37) -----------------------------------------------------------------------
 * An extension.  cart_voxel_color is a companion of one cart_voxel_map; it does not extend that map's voxel: the 4-byte cart_voxel,
 * cart_voxel_map_read / _write and every S33 - S36 kernel stay as they are.  The colour object copies cells_x/y/z and the map's
 * cart_voxel_map_params at create and owns a second volume of 4-byte words cart_voxel_rgb, stored as b | g << 8 | r << 16 | weight << 24
 * (the empty word is 0) in S33's toroidal storage (global voxel g at g mod N per axis, x fastest), its own window origin (int64) and
 * valid flag, and one parameter: max_weight (1..255, default 64, build-owned and untuned).  S33's arithmetic rules: fp64 with + - * /
 * floor only, every expression in the written order, integers after the projection, no atomic on the volume.  Restated in
 * tests/np_voxelcolor.py, byte for byte.
 *   Window: none of its own.  cart_voxel_color_integrate takes the MAP's current origin, read under the map's lock (lock order: map,
 *   then colour).  If the colour object has no window, or the origin moved by >= N on any axis, every colour voxel is emptied; otherwise
 *   the slabs that entered are emptied by S33's move rule.  Voxels that stay keep their colour: they are anchored in the world.  After
 *   cart_voxel_map_rebuild, _write or a jump the same rule applies at the next colour integrate.
 *   Integrate: called after cart_voxel_map_integrate of the same frame with the same camera, pose, disparity and mask, plus the frame's
 *   image: width x height of channels = 1 (gray) or 3 (B, G, R) bytes per pixel.  For every voxel of the window: gates 1 - 5 of S33 to the
 *   letter with the map's parameters, then f < 1.0 on the unclamped f of gate 5 (the voxels S33 counts in counts[1]: -tr <= sdf < tr).  A
 *   voxel that passes takes obs_c = the byte of channel c at pixel (x, y) (b = g = r for one channel) and, with its stored (c, w) in
 *   integers, c' = (2 (w c + obs_c) + (w + 1)) / (2 (w + 1)) (plain integer division of non-negative terms: rounds half up), w' = min(w +
 *   1, max_weight).  A voxel that fails a gate is neither read nor written; nothing of the TSDF volume is read.  counts = {voxels
 *   coloured, of them with w = 0 before}.
 *   Hand-worked (S33's case: identity pose, fx = fy = 256, cx = 8, cy = 4, baseline 0.5, disparity 64 px, voxel_size 0.25): voxel (0, 0,
 *   7) projects to pixel (25, 21), f = 0.125 / 0.265625 < 1; gray 200 leaves (200, 200, 200, 1); a second frame with 101 there gives
 *   604 / 4 = 151, weight 2; a third with 0 gives 607 / 6 = 101, weight 3.
 *   Sample rule, for a world point p in metres: per axis a = p / voxel_size - 0.5, i0 = floor(a); the eight corners i0 + {0,1}^3 must all
 *   lie in the colour window (compared as doubles: a NaN fails).  W = sum w_k and S_c = sum w_k c_k over the eight corners, in integers.
 *   Without a window, with a corner outside or with W = 0 the sample is (0, 0, 0, 0); otherwise c = (2 S_c + W) / (2 W) per channel and
 *   alpha = min(W, 255).  Hand-worked: corners (b = 10, w = 1) and (b = 20, w = 3) and six empty ones give W = 4, b = (140 + 4) / 8 = 18.
 *   Vertex colours: for vertex k < min(*n_vertices, max_vertices) of a cart_mesh_vertex array with its mesh origin o: a = (double)
 *   position_a / voxel_size - 0.5 (the fp32 record, as S36 wrote it), absolute corner index = o_a + floor(a) (a double sum), then the
 *   sample rule.  The rule is defined on the record, not on the cell that produced it: a position that fp32 rounding put on a cell face
 *   takes the neighbouring cell.  colors[k] for k beyond that count is not touched.
 *   Render: for pixel (x, y) of a disparity image in the format of `disparity` (the purpose is cart_voxel_map_raycast's model disparity):
 *   s != -32768 and s >= 1, d = s / 16.0, Z = (fx baseline) / d, p = the pose applied to (((x - cx) Z) / fx, ((y - cy) Z) / fy, Z) in S33's
 *   carry order, then the sample rule: B, G, R into an 8UC3 image and alpha into an optional u8 image; every other pixel gets zeros.
 *   counts = {pixels with alpha > 0}.
 * Memory: 4 bytes per voxel, as much as the map itself.  Limits: cart_voxel_map_rebuild restores no colour (the store keeps no images);
 * the colour pass is a launch of its own; the read-outs are weight-weighted integer means of eight voxels, not trilinear; no exposure
 * compensation. */
typedef struct cart_voxel_rgb { uint8_t b, g, r, weight; } cart_voxel_rgb;   /* 4 bytes */
typedef struct cart_voxel_color cart_voxel_color;
#define CART_VOXEL_COLOR_DEFAULT_MAX_WEIGHT 64
/* Extension.  max_weight in 1..255.  The object keeps the map's shape and parameters and the device it was created on, not the map: it
 * may outlive it.  Checked in this order: max_weight, engine and out ("bad arguments"), map, the map's device. */
int cart_voxel_color_create(cart_engine *engine, cart_voxel_map *map, int max_weight, cart_voxel_color **out);
void cart_voxel_color_destroy(cart_voxel_color *color);
/* Host only: the next integrate empties the colour volume on its stream; until then the read-outs give zeros. */
int cart_voxel_color_clear(cart_voxel_color *color);
/* Host getter, as cart_voxel_map_window: origin3 = zeros and *valid = 0 without a window. */
int cart_voxel_color_window(cart_voxel_color *color, int64_t *origin3, int32_t *shape3, int *valid);
/* Extension.  disp, image and mask are DEVICE images with steps in bytes (disp and its step 2-byte aligned; image_step >= channels width);
 * mask may be NULL; counts = DEVICE int32 [2] (4-byte aligned) or NULL.  Checked in this order, all before any device call: channels,
 * camera, pose, width and height, the colour object, the map, their devices and shapes, then pointers, alignment, steps and overlaps
 * (counts may overlap no input); the map's window under its lock.  A refused call launches nothing and changes nothing.  One or more
 * emptying launches and one integrate launch; no host synchronisation. */
int cart_voxel_color_integrate(cart_voxel_color *color, cart_voxel_map *map, const cart_ego_camera *camera, const double *pose,
                               const int16_t *disp, size_t disp_step, const uint8_t *image, size_t image_step, int channels, int width,
                               int height, const uint8_t *mask, size_t mask_step, int32_t *counts, void *stream);
/* Extension.  vertices = DEVICE cart_mesh_vertex [max_vertices], n_vertices = DEVICE int32 (both as cart_voxel_map_mesh wrote them: pass
 * counts + 2), max_vertices in 1..2^26, origin3 = HOST int64 [3] with |o_a| <= 2^27 (the mesh's origin), colors = DEVICE cart_voxel_rgb
 * [max_vertices] whose weight byte holds alpha.  Checked in this order: max_vertices, origin3, the object, then pointers, 4-byte
 * alignment and overlaps (colors may overlap neither input).  One launch, no host synchronisation. */
int cart_voxel_color_vertices(cart_voxel_color *color, const cart_mesh_vertex *vertices, const int32_t *n_vertices, int max_vertices,
                              const int64_t *origin3, cart_voxel_rgb *colors, void *stream);
/* Extension.  disp = DEVICE int16 image; image_bgr = DEVICE 8UC3 image (image_step >= 3 width), alpha = DEVICE u8 image or NULL, counts =
 * DEVICE int32 [1] (4-byte aligned) or NULL.  Checked in this order: camera, pose, width and height, the object, then pointers, alignment,
 * steps and overlaps (no output may overlap disp or another output).  One launch, no host synchronisation. */
int cart_voxel_color_render(cart_voxel_color *color, const cart_ego_camera *camera, const double *pose, const int16_t *disp,
                            size_t disp_step, int width, int height, uint8_t *image_bgr, size_t image_step, uint8_t *alpha,
                            size_t alpha_step, int32_t *counts, void *stream);
/* Extension.  As cart_voxel_map_read / _write, on HOST cart_voxel_rgb [cells_z][cells_y][cells_x] in window order; both synchronise
 * `stream`.  _read gives zeros and a zero origin without a window.  _write takes the origins cart_voxel_map_write takes (multiples of 8
 * within 2^27; checked first, then the object, then host_voxels) and leaves the object valid at that origin: a saved map restores with
 * its colours, and tests can sample arbitrary volumes. */
int cart_voxel_color_read(cart_voxel_color *color, cart_voxel_rgb *host_voxels, int64_t *origin3, void *stream);
int cart_voxel_color_write(cart_voxel_color *color, const cart_voxel_rgb *host_voxels, const int64_t *origin3, void *stream);

/* ---- Frame-to-model pose tracking against the TSDF volume (spec S34) ---------------------------------------------
 * An extension: the reference estimates no pose.  Gauss-Newton refinement of a camera-to-world pose P (3 x 4 as cart_voxel_map_raycast
 * takes it) so that the frame's back-projected pixels lie on the zero level set of a cart_voxel_map: minimises sum F(P p)^2.  fp64 with
 * + - * / floor sqrt only, every expression in the written order, no floating-point atomic: restated in tests/np_modeltrack.py, byte
 * for byte over the whole result record.  The depth, disparity and weight gates are the map's own cart_voxel_map_params.
 *   Sample grid: pixels (x, y) = (i stride, j stride) inside the image.  One evaluation at P, per sampled pixel:
 *   1. s = disp[y][x] != -32768, d = s / 16.0 >= min_disparity, Z = (fx baseline) / d with min_depth <= Z <= max_depth, mask NULL or
 *      mask[y][x] != 1 (MOVING): exactly the pixels cart_voxel_map_integrate could have used.
 *   2. p = P applied to (((x - cx) Z) / fx, ((y - cy) Z) / fy, Z) in S33's carry order.  The sample at p is known by the raycast's rule
 *      to the letter: a = p / voxel_size - 0.5, i0 = floor(a), fr = a - i0 per axis; a window exists, all eight corners i0 + {0,1}^3 lie
 *      in it (compared as doubles; a NaN fails) and each has weight >= min_weight.  A pixel with a known sample is a candidate.
 *   3. With t[dz][dy][dx] the eight tsdf integers: c[dy][dz], e0, e1 and F as the raycast's; g_z = e1 - e0; g_y = h0 + fr_z (h1 - h0)
 *      with h0 = c[1][0] - c[0][0], h1 = c[1][1] - c[0][1]; g_x = a0 + fr_z (a1 - a0) with a0 = D[0][0] + fr_y (D[1][0] - D[0][0]),
 *      a1 = D[0][1] + fr_y (D[1][1] - D[0][1]), D[dy][dz] = (double)(t[dz][dy][1] - t[dz][dy][0]).
 *   4. r = F / 32767.0; the candidate is an inlier iff |r| < residual_gate (saturated free space, where the gradient vanishes, drops out).
 *   5. G = g / (32767.0 voxel_size) (the product first), J = (p_y G_z - p_z G_y, p_z G_x - p_x G_z, p_x G_y - p_y G_x, G_x, G_y, G_z):
 *      the row of the left update p <- Rq p + upsilon.
 *   6. Sums in S26's layout: the 21 upper J_i J_j, the 6 J_i r, r r, the inlier count and the candidate count.
 *   Order of every sum: S26's, word for word (cart_dense_ego_params above): for sampled row j, virtual lane l of 256 starts at +0.0 and
 *   adds its inliers of sampled columns l, l + 256, ... in ascending order, then v[l] += v[l ^ o] for o = 1, 2, 4 .. 128 and lane 0 holds
 *   the row's partial; virtual lane l then adds the partials of sampled rows l, l + 256, ... (every row, ascending), the same butterfly.
 *   Iteration (S26's state machine): P = pose0; iterations + 1 evaluations, the last one only measures.  The first gives n_initial and
 *   rms_initial.  Up to `iterations` times: evaluate, stop if the inlier count cnt < min_inliers, H[i][i] = H[i][i] + damping (double)cnt,
 *   solve H delta = -g by S23's unpivoted Cholesky (stop at a pivot that is not > 0), update the pose as S23 does (R <- Rq R,
 *   t <- Rq t + upsilon), steps += 1.  The evaluation that stops gives n_inliers, n_candidates and rms = sqrt(sum r r / cnt) (0.0 at 0).
 *   Without a window there is no candidate: status 0 and the input pose.
 *   Acceptance is the consumer's: take the pose iff status == 1, every number of the record is finite, rms <= rms_initial and
 *   n_inliers >= min_inliers, else keep pose0. */
typedef struct cart_model_track_params {
    double residual_gate;                     /* fraction of the truncation, finite, 0 < . <= 1 */
    double damping;                           /* finite, >= 0: added to H's diagonal times the inlier count */
    int32_t iterations;                       /* 0..16 */
    int32_t stride;                           /* 1..16 */
    int32_t min_inliers;                      /* 6..2^30 */
} cart_model_track_params;
void cart_model_track_default_params(cart_model_track_params *p); /* extension: 0.9, 0.01, 4, 1, 1024 (build-owned, untuned) */
#define CART_MODEL_TRACK_MAX_ITERATIONS 16
typedef struct cart_model_track_result {      /* the layout of cart_dense_ego_result */
    double R[9], t[3];                        /* the pose after `steps` updates; pose0's when status is 0 */
    double rms_initial, rms;                  /* sqrt(sum r r / n) at pose0 and at (R, t) */
    int32_t status;                           /* 1 iff steps > 0 */
    int32_t n_candidates;                     /* pixels with a known sample at (R, t) */
    int32_t n_initial, n_inliers;             /* inliers at pose0 and at (R, t) */
    int32_t steps, reserved;
} cart_model_track_result;

typedef struct cart_model_track cart_model_track;
/* Extension.  The workspace for frames of up to max_width x max_height (1..16384 each): one row partial per image row and the pose
 * state; nothing is allocated per call.  The sizes are checked before the engine. */
int cart_model_track_create(cart_engine *engine, int max_width, int max_height, cart_model_track **out);
/* Extension.  Keeps the device it was created on, so it may be destroyed after its engine. */
void cart_model_track_destroy(cart_model_track *obj);
/* Extension.  One frame against `map`: pose0 = HOST double [12] (3 x 4 camera-to-world as cart_voxel_map_raycast's; all finite,
 * |R entries| <= 2, |t entries| <= 1e6); disp = device int16 x16 (2-byte aligned), mask = device u8 labels of cart_motion_segment or
 * NULL, both width x height (1..16384 each and within the object's maxima), steps in bytes.  result = DEVICE record (8-byte aligned,
 * overlapping no input).  Checked in this order, all before any device call: params, camera, pose0, sizes, the object, the map, then
 * pointers, alignment and steps; a refused call touches no output.  Reads the volume only and never moves the window.  Takes the
 * object, then the map: the call is ordered after earlier calls on either, whatever their streams.  2 (iterations + 1) plain launches
 * on `stream`, no host synchronisation. */
int cart_model_track_refine(cart_model_track *obj, cart_voxel_map *map, const cart_ego_camera *camera, const double *pose0,
                            const cart_model_track_params *params, const int16_t *disp, size_t disp_step, const uint8_t *mask,
                            size_t mask_step, int width, int height, cart_model_track_result *result, void *stream);

/* Extension: colour-aided frame-to-model tracking (spec S38).  S34's evaluation, to the letter, plus a photometric term
 * read from the colour companion of the volume (cart_voxel_color, S37), for every geometric inlier and only if photo_weight > 0:
 *   7. L_obs = b + 2 g + r of the frame's pixel (x, y) in integers (0 .. 1020; 4 v for one channel).
 *   8. The colour sample at p against the colour object's OWN grid and origin: a = p / voxel_size - 0.5, i0 = floor(a), fr = a - i0; known
 *      iff a colour window exists, all eight corners lie in it (compared as doubles) and each has weight >= color_min_weight.  With
 *      t[dz][dy][dx] = b + 2 g + r of the corner word, the value C and the gradient gc are step 3's expressions on these integers.
 *   9. rc = (C - (double)L_obs) / 1020.0; the pixel is a photometric inlier iff |rc| < photo_gate.
 *  10. Gc = gc / (1020.0 voxel_size) (the product first), Jc = (p_y Gc_z - p_z Gc_y, p_z Gc_x - p_x Gc_z, p_x Gc_y - p_y Gc_x, Gc).
 *  11. After the pixel's geometric terms: the 21 upper sums += (photo_weight Jc_i) Jc_j, the 6 += (photo_weight Jc_i) rc, a 29th sum
 *      += rc rc (unweighted; sum 27 stays the geometric r r), and a third count n_photo.
 *   Order of every sum: S34's two-level lane order over 29 sums and three counts.  The step is S34's: stop at cnt < min_inliers or at a
 *   pivot that is not > 0; H[i][i] += damping (double)cnt with the geometric count.
 *   cost = sqrt((sum r r + photo_weight sum rc rc) / ((double)cnt + photo_weight (double)n_photo)), 0.0 at a zero denominator.
 *   Acceptance is the consumer's: take the pose iff status == 1, every number of the record is finite, cost <= cost_initial and
 *   n_inliers >= min_inliers, else keep pose0.  With photo_weight == 0 neither the image nor the colour volume is read, and the first
 *   136 bytes of the record are cart_model_track_refine's on the same inputs. */
typedef struct cart_model_track_color_params {
    double photo_weight;                      /* finite, >= 0: the weight of the photometric term */
    double photo_gate;                        /* finite, 0 < . <= 1: inlier gate on |rc| */
    int32_t color_min_weight;                 /* 1..255: least weight of each colour corner */
    int32_t reserved;                         /* must be 0 */
} cart_model_track_color_params;
void cart_model_track_color_default_params(cart_model_track_color_params *p); /* extension: 64, 0.25, 1, 0 (build-owned, untuned) */
typedef struct cart_model_track_color_result { /* 176 bytes; the first 136 have cart_model_track_result's layout and meaning */
    double R[9], t[3];
    double rms_initial, rms;                  /* the geometric rms */
    int32_t status, n_candidates, n_initial, n_inliers, steps, reserved;
    double rms_photo_initial, rms_photo;      /* sqrt(sum rc rc / n_photo) at pose0 and at (R, t); 0.0 at n_photo == 0 */
    double cost_initial, cost;                /* the weighted mean residual at pose0 and at (R, t) */
    int32_t n_photo_initial, n_photo;         /* photometric inliers at pose0 and at (R, t) */
} cart_model_track_color_result;
/* Extension.  cart_model_track_refine's arguments plus `color` (made for a map of `map`'s shape, on the object's device), its parameters
 * and the frame's image: device u8, width x height of `channels` (1 = gray, 3 = B, G, R) bytes per pixel, image_step in bytes, as
 * cart_voxel_color_integrate takes it.  Checked in this order, all before any device call: params, color_params, channels, camera,
 * pose0, sizes, the object, the map, the colour object (NULL, devices, shape), then pointers, alignment, steps and overlaps; a refused
 * call touches no output.  result = DEVICE record (8-byte aligned, overlapping no input).  Reads both volumes only.  Takes the object,
 * then the map, then the colour object.  2 (iterations + 1) plain launches on `stream`, no host synchronisation. */
int cart_model_track_refine_color(cart_model_track *obj, cart_voxel_map *map, cart_voxel_color *color, const cart_ego_camera *camera,
                                  const double *pose0, const cart_model_track_params *params,
                                  const cart_model_track_color_params *color_params, const int16_t *disp, size_t disp_step,
                                  const uint8_t *image, size_t image_step, int channels, const uint8_t *mask, size_t mask_step, int width,
                                  int height, cart_model_track_color_result *result, void *stream);

/* Stand-in for ImageOpticalFlowModule's device work (src/modules/optflow.cpp:96-140: cvtColor x2 +
 * cv::cuda::NvidiaOpticalFlow_2_0::calc(current, previous), NVIDIA fixed-function hardware): dense census block
 * matching (oracle S15).  cur / prev = the reference images of frame id and id-1 (1-channel gray or 3-channel BGR),
 * flow = CV_16SC2 in S10.5 like the reference's (include/modules/optflow.hpp:16); previous position = p - (flow >> 5).
 * radius = search range in pixels (1..16), block = half window (1..3 -> 3x3, 5x5, 7x7). */
int cart_optical_flow(cart_engine *engine, const uint8_t *cur, size_t cur_step, const uint8_t *prev, size_t prev_step,
                      int channels, int radius, int block, int16_t *flow, size_t flow_step, void *stream);

/* Coarse-to-fine form of the same stand-in (spec S21): a 2x2-mean pyramid of both frames, S2 census per level, S15 at
 * the coarsest level (radius, block), then per finer level a search of (2 refine_radius + 1)^2 candidates around twice the coarser
 * level's flow, optionally a 3x3 median of each flow component per level.  Integer only; reach radius * 2^(L-1) + refine_radius *
 * (2^(L-1) - 1) pixels, no sub-pixel step (the consumers floor flow >> 5).  levels = 1, median = 0 is cart_optical_flow bit for bit. */
typedef struct cart_flow_params {
    int levels;         /* 1..6 requested; a level is built only while it is at least 24 x 16 */
    int radius;         /* 1..16, full search at the coarsest level */
    int refine_radius;  /* 1..4 */
    int block;          /* 1..3 */
    int median;         /* 0 | 1 */
} cart_flow_params;
void cart_flow_default_params(cart_flow_params *p); /* 4, 4, 2, 2, 1 */
/* HOST only: sizes of the levels S21 builds for a width x height frame (level_w / level_h: `levels` entries, may be NULL).
 * Returns levels_used <= levels, or -1 on bad arguments. */
int cart_flow_pyramid_levels(int width, int height, int levels, int *level_w, int *level_h);
/* Arguments as cart_optical_flow.  One workspace slot per call, nothing allocated after an engine's first call, asynchronous on `stream`. */
int cart_optical_flow_pyramid(cart_engine *engine, const uint8_t *cur, size_t cur_step, const uint8_t *prev, size_t prev_step,
                              int channels, const cart_flow_params *params, int16_t *flow, size_t flow_step, void *stream);
/* Test access to the calling thread's last cart_optical_flow_pyramid call (synchronises the device): what = 0 level image of cur,
 * 1 of prev (u8 [h_l][w_l]), 2 level flow (s16 [h_l][w_l][2], whole pixels, after the median when it is on).  host_dst is a HOST
 * buffer of exactly `bytes` = the level's size.  Fails for a level that call did not build. */
int cart_flow_debug_level(cart_engine *engine, int level, int what, void *host_dst, size_t bytes);

/* replaces: cv::cuda::resize(src, dst, size, 0, 0, cv::INTER_LINEAR) as KITTIDataSource::getNextInternal applies it when the
 * configured image size differs from the files' (src/sources/kitti.cpp:169-172); oracle S16.  8-bit, channels = 1 | 3,
 * device pointers, steps in bytes; needs no engine (no workspace).  device_id selects the GPU. */
int cart_resize_linear(int device_id, const uint8_t *src, size_t src_step, int src_width, int src_height, int channels,
                       uint8_t *dst, size_t dst_step, int dst_width, int dst_height, void *stream);

/* Copy between two device-visible buffers (16-byte aligned; e.g. a module output in HBM -> host memory that is mapped into
 * the device's address space, hipHostMalloc / a pinned allocation) by a kernel of `workgroups` workgroups (0 = 8).  This is
 * how a caller that wants disparity / planes in HOST memory -- the reference's consumers read cv::cuda::GpuMat, i.e. device
 * memory, so this is an extension -- gets them without a full-width copy kernel taking CUs from the compute kernels that
 * run beside it.  Asynchronous on `stream`. */
int cart_copy_narrow(cart_engine *engine, void *dst, const void *src, size_t bytes, int workgroups, void *stream);

/* replaces: util::findPeaks (peaks.cpp:12-72). HOST. Arrays hold n entries; returns #peaks, sorted by persistence. */
int cart_find_peaks(const int32_t *data, int n, int *born, int *died, int *left, int *right);

/* Test/diagnostic access to the workspace of the most recent compute call of the calling thread's
 * lease (synchronises the device).  `what`: */
enum {
    CART_DBG_GRAY_L = 0, CART_DBG_GRAY_R = 1,     /* u8  [h][w]              */
    CART_DBG_CENSUS_L = 2, CART_DBG_CENSUS_R = 3, /* u32 [h][w]              */
    CART_DBG_PATH0 = 16,                          /* +r: u8 [h][w][D], r<paths; path 1 ("up") is not materialised by
                                                     batches that take the fused WTA (D=256) */
    CART_DBG_WTA_L = 32, CART_DBG_WTA_R = 33      /* u16 [h][w]              */
};
int cart_debug_read(cart_engine *engine, int frame_slot, int what, void *host_dst, size_t bytes);

/* Test access to the integer form of the uniqueness test.  The WTA kernels replace the float compare
 * (float)S * u >= (float)best (u = (100 - uniqueness_ratio) / 100.0f) by S >= T(best); this returns T for every
 * best = 0..2047 (sums of <= 8 paths of <= 255 stay below 2048), clamped to 4095 where no reachable S passes.
 * engine != NULL: computed on its GPU by the kernels' own device function; engine == NULL: the same function
 * compiled for the host.  out2048 is a HOST array. */
int cart_debug_uniq_table(cart_engine *engine, int uniqueness_ratio, uint16_t *out2048);

/* Test / diagnostic access to the layout of the cost-slab workspace: the slots are cut into groups, each group one
 * device allocation of at most 8 GiB - 64 MiB.  Any pointer may be NULL.  group_bytes: bytes of a full group (the last one may be smaller). */
int cart_debug_slab_layout(cart_engine *engine, int *group_slots, int *n_groups, size_t *slot_bytes, size_t *group_bytes);
/* Test access: synchronises and counts the non-zero words of the component-table scratch (every table call must hand it back all
 * zeros: cart_plane_ccl_table / cart_plane_ccl_stats collect exactly what they accumulated).  *nonzero = 0 also when no table call
 * has allocated the scratch yet. */
int cart_debug_ccl_scratch_nonzero(cart_engine *engine, size_t *nonzero);

/* Per-stage device time (hipEvents recorded on the caller's stream around each stage of
 * cart_compute_disparity[_batch]).  set_timing(1) enables recording and clears the record ring
 * (the last 256 recorded calls are kept); set_timing(k), k > 1, records every k-th call only (the events
 * cost ~0.02 ms of a call's stream time: a throughput measurement that wants live stage times but not
 * their cost on every step samples); set_timing(0) stops.  collect_timing() synchronises the device and returns, per stage,
 * the MEAN milliseconds per call over the recorded calls (names are static strings).  Returns the
 * number of stages written (<= cap) and the number of calls averaged in *n_calls. */
int cart_engine_set_timing(cart_engine *engine, int enabled);
int cart_engine_collect_timing(cart_engine *engine, const char **names, float *mean_ms, int cap, int *n_calls);

/* Library / build identification ("cart_engine gfx950 <n kernels>"). */
const char *cart_engine_version(void);

#ifdef __cplusplus
}
#endif
#endif

// disparity.cpp -- the engine handle, frame coalescing and the three disparity modules (disparity, derivative, depth) on top of the C ABI (include/cart_engine.h).
#include <algorithm>
#include <cstdio>

#include "cartslam_amd/coalescer.hpp"
#include "cartslam_amd/modules/depth.hpp"
#include "module_support.hpp"

namespace cart {
StreamPool &StreamPool::instance() { static StreamPool p; return p; }

namespace {
// CARTSLAM_PLACEMENT_TRIES = placements of the slab workspace cart_engine_tune_placement may try.  Default 1 = keep the allocation the
// engine was created with: a module constructor does not go looking for device memory on its own.  A deployment that wants the 2-4 %
// (include/cart_engine.h) sets it to 2..10; the search then holds at most two units of slab memory beyond the workspace (the call's
// default cap) and logs what it found.
int placementTries() {
    const char *env = std::getenv("CARTSLAM_PLACEMENT_TRIES");
    return env ? std::max(1, std::atoi(env)) : 1;
}
}  // namespace

cart_engine_params paramsFor(Size res, int minDisparity, int numDisparities, int radius, int iterations, int paths, int p1, int p2, int uniq) {
    cart_engine_params p;
    cart_engine_default_params(&p);
    p.width = res.width; p.height = res.height;
    p.min_disparity = minDisparity; p.num_disparities = numDisparities; p.paths = paths; p.p1 = p1; p.p2 = p2;
    p.uniqueness_ratio = uniq; p.smoothing_radius = radius; p.smoothing_iterations = iterations;
    p.max_inflight = (int)concurrentRunLimit();
    return p;
}

EngineHandle::EngineHandle(Size, const cart_engine_params &params) {
    if (cart_engine_create(&params, &engine) != 0) throw std::runtime_error(std::string("cart_engine_create: ") + cart_last_error(nullptr));
    // Opt-in (CARTSLAM_PLACEMENT_TRIES > 1): pick the fastest of a few physical placements of the cost-slab workspace (include/cart_engine.h,
    // cart_engine_tune_placement: the aggregation launch runs 8-9 % faster on some).  Not fatal: a failed probe leaves the first placement.
    if (params.num_disparities > 0 && placementTries() > 1) {
        cart_placement_report rep;
        static const char *const modes[] = {"unknown", "fast", "mixed", "uniform"};
        if (cart_engine_tune_placement(engine, std::min(params.max_inflight, 16), placementTries(), /*max_extra_bytes: default cap*/ 0, &rep) != 0)
            std::fprintf(stderr, "[cartslam_amd] placement tuning failed (%s); keeping the first placement\n", cart_last_error(engine));
        else
            std::fprintf(stderr, "[cartslam_amd] placement tuning: launch pair %.3f -> %.3f ms, %d placements timed in %.2f s, mode %s\n", rep.ms_first, rep.ms_kept,
                         rep.candidates, rep.seconds, modes[rep.mode & 3]);
    }
}
EngineHandle::~EngineHandle() { cart_engine_destroy(engine); }
void EngineHandle::fail(const char *what) const { throw std::runtime_error(std::string(what) + ": " + cart_last_error(engine)); }

// ---------------------------------------------------------------- frame coalescing (cartslam_amd/coalescer.hpp)
// CARTSLAM_COALESCE = frame groups of one module allowed on the GPU at once; 0 = one launch sequence per frame.
// Default 1: while a group is on the GPU the next one collects every frame that arrives, so the groups are as large as
// the frames in flight allow (12 in flight: 5.6 frames per launch and 4.98 k pairs/s at D=128 / 8 paths, against 3.7 and
// 4.58 k with two groups and 2.5 / 4.56 k with three -- profiles/tools/r02_coalesce.sh; a launch of 3 frames is far from
// filling the chip, and two of them side by side do not make up for it).
int coalesceGroups() {
    const char *env = std::getenv("CARTSLAM_COALESCE");
    return env ? std::atoi(env) : 1;
}
int coalesceMaxGroup() { return (int)std::min<size_t>(concurrentRunLimit(), 16); }  // 16 = frames per launch sequence
// CARTSLAM_COALESCE_AHEAD = requests that must have gathered before a group is queued behind a running one (with CARTSLAM_COALESCE >= 2)
int coalesceMinAhead() {
    const char *env = std::getenv("CARTSLAM_COALESCE_AHEAD");
    return env ? std::max(1, std::atoi(env)) : std::max(2, (int)std::min<size_t>(concurrentRunLimit(), 32) / 2);
}

// ---------------------------------------------------------------- disparity (disparity.cu:49-80)
struct DisparityRequest : CoalescedRequest {
    const uint8_t *left, *right; size_t leftStep, rightStep; int channels;
    int16_t *out; size_t outStep;
};
class DisparityCoalescer : public FrameCoalescer<DisparityRequest> {
   public:
    using FrameCoalescer<DisparityRequest>::FrameCoalescer;
};

ImageDisparityModule::ImageDisparityModule(const Size imageRes, int minDisparity, int numDisparities, int /*blockSize: ignored by the CUDA SGM too*/,
                                           int smoothingRadius, int smoothingIterations, int paths, int p1, int p2, int uniquenessRatio)
    : SyncWrapperSystemModule("ImageDisparity"), imageRes(imageRes) {
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY);
    engine = std::make_shared<EngineHandle>(imageRes, paramsFor(imageRes, minDisparity, numDisparities, smoothingRadius, smoothingIterations, paths, p1, p2, uniquenessRatio));
    if (coalesceGroups() > 0) {
        auto eng = engine;
        coalescer = std::make_shared<DisparityCoalescer>(
            coalesceMaxGroup(), coalesceGroups(),
            [](const DisparityRequest &a, const DisparityRequest &b) {
                return a.channels == b.channels && a.leftStep == b.leftStep && a.rightStep == b.rightStep && a.outStep == b.outStep;
            },
            [eng](const std::vector<DisparityRequest *> &group) {
                std::vector<const uint8_t *> lefts, rights;
                std::vector<int16_t *> outs;
                for (const DisparityRequest *q : group) { lefts.push_back(q->left); rights.push_back(q->right); outs.push_back(q->out); }
                const DisparityRequest &rq = *group[0];
                ScopedStream stream(true);
                if (cart_compute_disparity_multi(eng->get(), (int)group.size(), lefts.data(), rq.leftStep, rights.data(), rq.rightStep, rq.channels,
                                                 outs.data(), rq.outStep, stream.s) != 0)
                    eng->fail("cart_compute_disparity_multi");
                stream.wait();  // stream.waitForCompletion(), disparity.cu:77
            },
            coalesceMinAhead());
    }
}

double ImageDisparityModule::meanFramesPerLaunch() const { return coalescer ? coalescer->meanGroup() : 1.0; }

system_data_t ImageDisparityModule::runInternal(System &, SystemRunData &data) {
    if (data.dataElement->type != DataElementType::STEREO) throw std::runtime_error("ImageDisparityModule requires StereoDataElement");
    auto stereo = std::static_pointer_cast<StereoDataElement>(data.dataElement);
    const image_t &l = stereo->left, &r = stereo->right;
    const int channels = l.type() == CV_8UC3 ? 3 : 1;
    if ((l.type() != CV_8UC3 && l.type() != CV_8UC1) || r.type() != l.type()) throw std::runtime_error("ImageDisparityModule requires CV_8UC1 or CV_8UC3 images");
    // the engine's workspaces are sized for the resolution given to the constructor (disparity.hpp:26): anything else would run past them
    if (l.cols != imageRes.width || l.rows != imageRes.height || r.cols != l.cols || r.rows != l.rows)
        throw std::runtime_error("ImageDisparityModule: image size " + std::to_string(l.cols) + "x" + std::to_string(l.rows) + " does not match the module's " +
                                 std::to_string(imageRes.width) + "x" + std::to_string(imageRes.height));
    auto disparity = std::make_shared<image_t>(l.rows, l.cols, CV_16SC1);
    if (coalescer) {
        DisparityRequest rq;
        rq.left = l.ptr<uint8_t>(); rq.right = r.ptr<uint8_t>(); rq.leftStep = l.step; rq.rightStep = r.step; rq.channels = channels;
        rq.out = disparity->ptr<int16_t>(); rq.outStep = disparity->step;
        coalescer->run(rq);
        return MODULE_RETURN(CARTSLAM_KEY_DISPARITY, disparity);
    }
    ScopedStream stream(true);
    if (cart_compute_disparity(engine->get(), l.ptr<uint8_t>(), l.step, r.ptr<uint8_t>(), r.step, channels, disparity->ptr<int16_t>(), disparity->step, stream.s) != 0)
        engine->fail("cart_compute_disparity");
    stream.wait();  // stream.waitForCompletion(), disparity.cu:77
    return MODULE_RETURN(CARTSLAM_KEY_DISPARITY, disparity);
}

// ---------------------------------------------------------------- derivative (derivative.cu:151-184)
ImageDisparityDerivativeModule::ImageDisparityDerivativeModule() : SyncWrapperSystemModule("ImageDisparityDerivative") {
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY));
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_DERIVATIVE);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_DERIVATIVE_HISTOGRAM);
}

std::shared_ptr<EngineHandle> postEngine(std::mutex &mu, std::shared_ptr<EngineHandle> &slot, const image_t &disp) {
    std::lock_guard<std::mutex> lk(mu);
    if (!slot) {  // the post stages only need the geometry: num_disparities = paths = 0 -> no SGM workspaces
        Size res; res.width = disp.cols; res.height = disp.rows;
        cart_engine_params p = paramsFor(res, 0, 0, -1, 0, 0, 10, 120, 12);
        slot = std::make_shared<EngineHandle>(res, p);
    }
    return slot;
}

system_data_t ImageDisparityDerivativeModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(CARTSLAM_KEY_DISPARITY);
    if (disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    auto eng = postEngine(engineMutex, engine, *disparity);
    auto derivatives = std::make_shared<image_t>(disparity->rows, disparity->cols, CV_16SC2);
    auto histogram = std::make_shared<image_t>(1, 256, CV_32SC2);
    ScopedStream stream;
    if (cart_disparity_derivative(eng->get(), 1, disparity->ptr<int16_t>(), disparity->step, 0, derivatives->ptr<int16_t>(), derivatives->step, 0,
                                  histogram->ptr<int32_t>(), stream.s) != 0)
        eng->fail("cart_disparity_derivative");
    stream.wait();
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_DISPARITY_DERIVATIVE, derivatives),
                             MODULE_PAIR(CARTSLAM_KEY_DISPARITY_DERIVATIVE_HISTOGRAM, histogram));
}

// ---------------------------------------------------------------- depth (depth.cpp:9-25)
system_data_t DepthModule::runInternal(System &system, SystemRunData &data) {
    auto disparity = data.getData<image_t>(CARTSLAM_KEY_DISPARITY);
    if (disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    auto eng = postEngine(engineMutex, engine, *disparity);
    const CameraIntrinsics K = system.getDataSource()->getCameraIntrinsics();
    auto depth = std::make_shared<image_t>(disparity->rows, disparity->cols, CV_32FC3);
    ScopedStream stream;
    if (cart_reproject_depth(eng->get(), 1, disparity->ptr<int16_t>(), disparity->step, 0, K.Q, depth->ptr<float>(), depth->step, 0, stream.s) != 0)
        eng->fail("cart_reproject_depth");
    stream.wait();
    return MODULE_RETURN(CARTSLAM_KEY_DEPTH, depth);
}
}  // namespace cart

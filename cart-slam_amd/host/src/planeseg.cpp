// planeseg.cpp -- the two plane-segmentation modules and the plane parameter providers (cartslam_amd/modules/planeseg.hpp).
#include "cartslam_amd/coalescer.hpp"
#include "cartslam_amd/modules/planeseg.hpp"
#include "module_support.hpp"

namespace cart {
// ---------------------------------------------------------------- plane labels (planeseg.cu:246-458)
DisparityPlaneSegmentationModule::DisparityPlaneSegmentationModule(std::shared_ptr<PlaneParameterProvider> provider, const int updateInterval, const int resetInterval,
                                                                   const bool useTemporalSmoothing, const unsigned int temporalSmoothingDistance, const bool labelComponents)
    : SyncWrapperSystemModule("PlaneSegmentation"), useTemporalSmoothing(useTemporalSmoothing), temporalSmoothingDistance(temporalSmoothingDistance),
      updateInterval(updateInterval), resetInterval(resetInterval), labelComponents(labelComponents), planeParameterProvider(provider) {
    if (useTemporalSmoothing && (temporalSmoothingDistance < 1 || temporalSmoothingDistance > CART_MAX_TEMPORAL))
        throw std::runtime_error("temporal_smoothing_distance must be in [1, 8]");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY));
    if (useTemporalSmoothing) {  // planeseg.hpp:128-137: optical flow and the earlier frames' unsmoothed planes
        this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_OPTFLOW));
        for (size_t i = 1; i <= this->temporalSmoothingDistance; i++) {
            this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_PLANES_UNSMOOTHED, -(int)i));
            if ((i + 1) <= this->temporalSmoothingDistance) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_OPTFLOW, -(int)i));
        }
    }
    this->providesData.push_back(CARTSLAM_KEY_PLANES);
    if (useTemporalSmoothing) this->providesData.push_back(CARTSLAM_KEY_PLANES_UNSMOOTHED);
    if (labelComponents) {
        this->providesData.push_back(CARTSLAM_KEY_PLANE_COMPONENTS);
        this->providesData.push_back(CARTSLAM_KEY_PLANE_COMPONENT_TABLE);
        this->providesData.push_back(CARTSLAM_KEY_PLANE_COMPONENT_COUNT);
    }
}

DisparityPlaneSegmentationModule::~DisparityPlaneSegmentationModule() {
    if (derivativeHistogram) (void)hipFree(derivativeHistogram);
}

struct PlaneRequest : CoalescedRequest {
    const int16_t *disparity; size_t disparityStep;
    int16_t *derivatives; size_t derivativesStep;
    uint8_t *planes; size_t planesStep;
};
class PlaneCoalescer : public FrameCoalescer<PlaneRequest> {
   public:
    using FrameCoalescer<PlaneRequest>::FrameCoalescer;
};

void DisparityPlaneSegmentationModule::ensureHistogram() {
    static std::mutex createMutex;
    std::lock_guard<std::mutex> lk(createMutex);
    if (!derivativeHistogram) {
        hipCheck(hipMalloc(reinterpret_cast<void **>(&derivativeHistogram), 256 * sizeof(int32_t)), "hipMalloc");
        hipCheck(hipMemset(derivativeHistogram, 0, 256 * sizeof(int32_t)), "hipMemset");
    }
}

system_data_t DisparityPlaneSegmentationModule::runInternal(System &system, SystemRunData &data) {
    auto disparity = data.getData<image_t>(CARTSLAM_KEY_DISPARITY);
    if (disparity->empty()) return MODULE_NO_RETURN_VALUE;  // planeseg.cu:250-253
    if (disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    auto eng = postEngine(engineMutex, engine, *disparity);
    auto derivatives = std::make_shared<image_t>(disparity->rows, disparity->cols, CV_16SC1);
    const bool updateFrame = (int)(data.id % (uint32_t)this->updateInterval) == 1;
    // Frames that neither refresh the parameters nor need per-frame extras go through the coalescer: the frames waiting
    // here together get one derivative launch (all adding to the cumulative histogram, like concurrent frames of the
    // reference do) and one classify launch with the parameters current at that moment.
    if (!updateFrame && !this->useTemporalSmoothing && !this->labelComponents && coalesceGroups() > 0) {
        {
            std::lock_guard<std::mutex> lk(engineMutex);
            if (!coalescer) {
                coalescer = std::make_shared<PlaneCoalescer>(
                    coalesceMaxGroup(), coalesceGroups(),
                    [](const PlaneRequest &a, const PlaneRequest &b) {
                        return a.disparityStep == b.disparityStep && a.derivativesStep == b.derivativesStep && a.planesStep == b.planesStep;
                    },
                    [this, eng](const std::vector<PlaneRequest *> &group) {
                        std::shared_lock<std::shared_mutex> histogramLock(derivativeHistogramMutex);  // until the group's kernels have finished
                        ensureHistogram();
                        std::vector<const int16_t *> disps, derivsIn;
                        std::vector<int16_t *> derivs;
                        std::vector<uint8_t *> labels;
                        for (const PlaneRequest *q : group) { disps.push_back(q->disparity); derivs.push_back(q->derivatives); derivsIn.push_back(q->derivatives); labels.push_back(q->planes); }
                        const PlaneRequest &rq = *group[0];
                        ScopedStream stream;
                        if (cart_plane_derivative_hist_multi(eng->get(), (int)group.size(), disps.data(), rq.disparityStep, derivs.data(), rq.derivativesStep,
                                                             derivativeHistogram, 0, stream.s) != 0)
                            eng->fail("cart_plane_derivative_hist_multi");
                        const PlaneParameters pp = planeParameterProvider->getPlaneParameters();
                        cart_plane_params cp{pp.horizontalRange.first, pp.horizontalRange.second, pp.verticalRange.first, pp.verticalRange.second, pp.horizontalCenter, pp.verticalCenter};
                        if (cart_plane_classify_multi(eng->get(), (int)group.size(), derivsIn.data(), rq.derivativesStep, &cp, 0, labels.data(), rq.planesStep, stream.s) != 0)
                            eng->fail("cart_plane_classify_multi");
                        stream.wait();
                    },
                    coalesceMinAhead());
            }
        }
        auto planes = std::make_shared<image_t>(disparity->rows, disparity->cols, CV_8UC1);
        PlaneRequest rq;
        rq.disparity = disparity->ptr<int16_t>(); rq.disparityStep = disparity->step;
        rq.derivatives = derivatives->ptr<int16_t>(); rq.derivativesStep = derivatives->step;
        rq.planes = planes->ptr<uint8_t>(); rq.planesStep = planes->step;
        coalescer->run(rq);
        return MODULE_RETURN(CARTSLAM_KEY_PLANES, planes);
    }
    // Read-lock section, planeseg.cu:269-288: the histogram download of an update frame (unique lock) must not overlap a
    // derivative kernel that is still adding to it.  An update frame (id % updateInterval == 1) synchronises and
    // releases the lock right after its derivative kernel, like the reference; every other frame has nothing to do
    // between the two kernels, keeps the lock and enqueues the rest of the module behind the derivative kernel on the
    // same stream: one stream synchronisation per frame instead of two.
    std::shared_lock<std::shared_mutex> histogramLock(derivativeHistogramMutex);
    ensureHistogram();
    ScopedStream stream;
    if (cart_plane_derivative_hist(eng->get(), 1, disparity->ptr<int16_t>(), disparity->step, 0, derivatives->ptr<int16_t>(), derivatives->step, 0,
                                   derivativeHistogram, 0, stream.s) != 0)
        eng->fail("cart_plane_derivative_hist");
    if (updateFrame) {
        stream.wait();
        histogramLock.unlock();
        this->updatePlaneParameters(system, data);
    }

    auto planes = std::make_shared<image_t>(disparity->rows, disparity->cols, CV_8UC1);
    const PlaneParameters pp = planeParameterProvider->getPlaneParameters();
    cart_plane_params cp{pp.horizontalRange.first, pp.horizontalRange.second, pp.verticalRange.first, pp.verticalRange.second, pp.horizontalCenter, pp.verticalCenter};
    if (cart_plane_classify(eng->get(), 1, derivatives->ptr<int16_t>(), derivatives->step, 0, &cp, 0, planes->ptr<uint8_t>(), planes->step, 0, stream.s) != 0)
        eng->fail("cart_plane_classify");
    std::shared_ptr<image_t> smoothed;
    std::vector<std::shared_ptr<image_t>> keepAlive;
    if (this->useTemporalSmoothing && data.id > 1) {  // planeseg.cu:303-347
        smoothed = std::make_shared<image_t>(disparity->rows, disparity->cols, CV_8UC1);
        const uint8_t *prevPlanes[CART_MAX_TEMPORAL];
        size_t prevSteps[CART_MAX_TEMPORAL];
        const int16_t *flows[CART_MAX_TEMPORAL];
        size_t flowSteps[CART_MAX_TEMPORAL];
        int previousPlaneCount = 0;
        auto optFlowCurr = data.getData<image_t>(CARTSLAM_KEY_OPTFLOW);
        keepAlive.push_back(optFlowCurr);
        flows[0] = optFlowCurr->ptr<int16_t>(); flowSteps[0] = optFlowCurr->step;
        for (int i = 1; i <= (int)this->temporalSmoothingDistance; i++) {
            if ((int64_t)data.id - i <= 0) break;
            auto relativeRun = data.getRelativeRun((int8_t)-i);
            auto prev = relativeRun->getData<image_t>(CARTSLAM_KEY_PLANES_UNSMOOTHED);
            keepAlive.push_back(prev);
            prevPlanes[previousPlaneCount] = prev->ptr<uint8_t>(); prevSteps[previousPlaneCount] = prev->step;
            previousPlaneCount++;
            if (relativeRun->id > 1 && previousPlaneCount < (int)this->temporalSmoothingDistance) {
                auto optFlow = relativeRun->getData<image_t>(CARTSLAM_KEY_OPTFLOW);
                keepAlive.push_back(optFlow);
                flows[previousPlaneCount] = optFlow->ptr<int16_t>(); flowSteps[previousPlaneCount] = optFlow->step;
            }
        }
        if (cart_plane_temporal_vote(eng->get(), planes->ptr<uint8_t>(), planes->step, previousPlaneCount, prevPlanes, prevSteps, flows, flowSteps,
                                     smoothed->ptr<uint8_t>(), smoothed->step, stream.s) != 0)
            eng->fail("cart_plane_temporal_vote");
    }
    std::shared_ptr<image_t> components, componentTable, componentCount;
    if (labelComponents) {
        components = std::make_shared<image_t>(disparity->rows, disparity->cols, CV_32SC1);
        componentTable = std::make_shared<image_t>(CARTSLAM_PLANE_COMPONENT_TABLE_ROWS, 7, CV_32SC1);
        componentCount = std::make_shared<image_t>(1, 1, CV_32SC1);
        static_assert(sizeof(cart_component) == 7 * sizeof(int32_t), "table rows are 7 x int32");
        if (componentTable->step != 7 * sizeof(int32_t)) {  // DeviceImage pads rows to 256 B: the table wants tight rows
            componentTable = std::make_shared<image_t>(1, CARTSLAM_PLANE_COMPONENT_TABLE_ROWS * 7, CV_32SC1);
        }
        // ids, count and table in one call: the pass that writes the final ids also gathers the component statistics (four launches)
        if (cart_plane_ccl_table(eng->get(), 1, planes->ptr<uint8_t>(), planes->step, 0, components->ptr<int32_t>(), components->step, 0,
                                 componentTable->ptr<cart_component>(), CARTSLAM_PLANE_COMPONENT_TABLE_ROWS, componentCount->ptr<int32_t>(), stream.s) != 0)
            eng->fail("cart_plane_ccl_table");
    }
    stream.wait();
    system_data_t out;
    if (this->useTemporalSmoothing) {  // planeseg.cu:361-374: frame 1 returns the same image under both keys
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_PLANES, data.id == 1 ? planes : smoothed));
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_PLANES_UNSMOOTHED, planes));
    } else {
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_PLANES, planes));
    }
    if (labelComponents) {
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_PLANE_COMPONENTS, components));
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_PLANE_COMPONENT_TABLE, componentTable));
        out.push_back(MODULE_PAIR(CARTSLAM_KEY_PLANE_COMPONENT_COUNT, componentCount));
    }
    return out;
}

void DisparityPlaneSegmentationModule::updatePlaneParameters(System &system, SystemRunData &data) {
    if ((int)(data.id % (uint32_t)this->updateInterval) != 1) return;  // planeseg.cu:381-383
    std::vector<int32_t> histogram(256);
    {
        std::unique_lock<std::shared_mutex> lock(derivativeHistogramMutex);
        hipCheck(hipMemcpy(histogram.data(), derivativeHistogram, 256 * sizeof(int32_t), hipMemcpyDeviceToHost), "hipMemcpy");
        if ((int)(data.id % (uint32_t)(this->updateInterval * this->resetInterval)) == 1)
            hipCheck(hipMemset(derivativeHistogram, 0, 256 * sizeof(int32_t)), "hipMemset");  // reset to avoid overflow (:391-394)
    }
    this->planeParameterProvider->updatePlaneParameters(system, data, histogram);
    system.insertGlobalData(CARTSLAM_KEY_PLANE_PARAMETERS, std::make_shared<PlaneParameters>(this->planeParameterProvider->getPlaneParameters()));
    system.insertGlobalData(CARTSLAM_KEY_DISPARITY_DERIVATIVE_HIST, std::make_shared<std::vector<int32_t>>(histogram));
}

// ---------------------------------------------------------------- superpixel plane labels (sp_planeseg.cu:180-388)
SuperPixelDisparityPlaneSegmentationModule::SuperPixelDisparityPlaneSegmentationModule(std::shared_ptr<PlaneParameterProvider> provider, const int updateInterval,
                                                                                       const int resetInterval, const bool useTemporalSmoothing,
                                                                                       const unsigned int temporalSmoothingDistance)
    : SyncWrapperSystemModule("SPPlaneSegmentation"), useTemporalSmoothing(useTemporalSmoothing), temporalSmoothingDistance(temporalSmoothingDistance),
      updateInterval(updateInterval), resetInterval(resetInterval), planeParameterProvider(provider) {
    if (useTemporalSmoothing && (temporalSmoothingDistance < 1 || temporalSmoothingDistance > CART_MAX_TEMPORAL))
        throw std::runtime_error("temporal_smoothing_distance must be in [1, 8]");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_SUPERPIXELS));  // sp_planeseg.cu:191-194
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY_DERIVATIVE));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY_DERIVATIVE_HISTOGRAM));
    if (useTemporalSmoothing) {  // :196-205
        this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_OPTFLOW));
        for (size_t i = 1; i <= this->temporalSmoothingDistance; i++) {
            this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_PLANES_UNSMOOTHED, -(int)i));
            if ((i + 1) <= this->temporalSmoothingDistance) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_OPTFLOW, -(int)i));
        }
    }
    this->providesData.push_back(CARTSLAM_KEY_PLANES);
    if (useTemporalSmoothing) this->providesData.push_back(CARTSLAM_KEY_PLANES_UNSMOOTHED);
}

system_data_t SuperPixelDisparityPlaneSegmentationModule::runInternal(System &system, SystemRunData &data) {
    auto derivatives = data.getData<image_t>(CARTSLAM_KEY_DISPARITY_DERIVATIVE);
    if (derivatives->empty()) return MODULE_NO_RETURN_VALUE;  // sp_planeseg.cu:223-226
    if (derivatives->type() != CV_16SC2) throw std::runtime_error("Disparity must be of type CV_16SC2");  // :228-231
    Size res; res.width = derivatives->cols; res.height = derivatives->rows;
    std::shared_ptr<EngineHandle> eng;
    {
        std::lock_guard<std::mutex> lk(engineMutex);
        if (!engine) engine = std::make_shared<EngineHandle>(res, paramsFor(res, 0, 0, -1, 0, 0, 10, 120, 12));
        eng = engine;
    }
    cart_plane_params cp;
    {
        FrameOrder::Turn turn(order, data.id);
        this->updatePlaneParameters(system, data);  // :237
        const PlaneParameters pp = planeParameterProvider->getPlaneParameters();
        cp = cart_plane_params{pp.horizontalRange.first, pp.horizontalRange.second, pp.verticalRange.first, pp.verticalRange.second, pp.horizontalCenter, pp.verticalCenter};
    }
    auto planes = std::make_shared<image_t>(derivatives->rows, derivatives->cols, CV_8UC1);
    auto smoothed = std::make_shared<image_t>(derivatives->rows, derivatives->cols, CV_8UC1);
    const uint8_t *prevPlanes[CART_MAX_TEMPORAL];
    size_t prevSteps[CART_MAX_TEMPORAL];
    const int16_t *flows[CART_MAX_TEMPORAL];
    size_t flowSteps[CART_MAX_TEMPORAL];
    int previousPlaneCount = 0;
    std::vector<std::shared_ptr<image_t>> keepAlive;
    if (this->useTemporalSmoothing && data.id > 1) {  // :250-300
        auto optFlowCurr = data.getData<image_t>(CARTSLAM_KEY_OPTFLOW);
        keepAlive.push_back(optFlowCurr);
        flows[0] = optFlowCurr->ptr<int16_t>(); flowSteps[0] = optFlowCurr->step;
        for (int i = 1; i <= (int)this->temporalSmoothingDistance; i++) {
            if ((int64_t)data.id - i <= 0) break;
            auto relativeRun = data.getRelativeRun((int8_t)-i);
            std::shared_ptr<image_t> prev;
            try { prev = relativeRun->getData<image_t>(CARTSLAM_KEY_PLANES_UNSMOOTHED); } catch (const std::exception &) { break; }  // :270-275
            keepAlive.push_back(prev);
            prevPlanes[previousPlaneCount] = prev->ptr<uint8_t>(); prevSteps[previousPlaneCount] = prev->step;
            previousPlaneCount++;
            if (relativeRun->id > 1 && previousPlaneCount < (int)this->temporalSmoothingDistance) {
                std::shared_ptr<image_t> optFlow;
                try { optFlow = relativeRun->getData<image_t>(CARTSLAM_KEY_OPTFLOW); } catch (const std::exception &) { break; }  // :289-294
                keepAlive.push_back(optFlow);
                flows[previousPlaneCount] = optFlow->ptr<int16_t>(); flowSteps[previousPlaneCount] = optFlow->step;
            }
        }
    }
    auto labels = data.getData<image_t>(CARTSLAM_KEY_SUPERPIXELS);
    const contour::label_t maxLabel = *data.getData<contour::label_t>(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL);
    if (labels->type() != CV_16UC1) throw std::runtime_error("Superpixels must be of type CV_16UC1");
    if (((size_t)maxLabel + 1) * 3 * sizeof(uint16_t) > 32768)  // the reference's shared-memory bound (:317-321), kept as the accepted range
        throw std::runtime_error("Shared memory size exceeds maximum. Reduce image size or increase block size.");
    ScopedStream stream;
    if (cart_superpixel_plane_classify(eng->get(), derivatives->ptr<int16_t>(), derivatives->step, labels->ptr<uint16_t>(), labels->step, (int)maxLabel, &cp,
                                       previousPlaneCount, prevPlanes, prevSteps, flows, flowSteps, planes->ptr<uint8_t>(), planes->step, smoothed->ptr<uint8_t>(),
                                       smoothed->step, stream.s) != 0)
        eng->fail("cart_superpixel_plane_classify");
    stream.wait();
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_PLANES, smoothed),  // :341-343: both keys, always
                             MODULE_PAIR(CARTSLAM_KEY_PLANES_UNSMOOTHED, planes));
}

void SuperPixelDisparityPlaneSegmentationModule::updatePlaneParameters(System &system, SystemRunData &data) {
    // channel 0 (vertical derivative) of the frame's CV_32SC2 1x256 histogram (sp_planeseg.cu:350-356)
    auto histImage = data.getData<image_t>(CARTSLAM_KEY_DISPARITY_DERIVATIVE_HISTOGRAM);
    std::vector<uint8_t> raw = histImage->downloadTight();
    const int32_t *two = reinterpret_cast<const int32_t *>(raw.data());
    std::vector<int32_t> histogram(256);
    for (int i = 0; i < 256; ++i) histogram[i] = two[2 * i];
    if (this->derivativeHistogram.empty()) {
        this->derivativeHistogram.assign(256, 0);  // :360-361: the first frame starts the running total at ZERO and is itself not added
    } else {
        for (int i = 0; i < 256; ++i) this->derivativeHistogram[i] += histogram[i];  // :363-365
        histogram = this->derivativeHistogram;
    }
    if ((int)(data.id % (uint32_t)(this->updateInterval * this->resetInterval)) == 1) this->derivativeHistogram.assign(256, 0);  // :368-371
    if ((int)(data.id % (uint32_t)this->updateInterval) != 1) return;  // :374-376
    this->planeParameterProvider->updatePlaneParameters(system, data, histogram);
    system.insertGlobalData(CARTSLAM_KEY_PLANE_PARAMETERS, std::make_shared<PlaneParameters>(this->planeParameterProvider->getPlaneParameters()));
    system.insertGlobalData(CARTSLAM_KEY_DISPARITY_DERIVATIVE_HIST, std::make_shared<std::vector<int32_t>>(histogram));
}

void HistogramPeakPlaneParameterProvider::updatePlaneParameters(System &, SystemRunData &, const std::vector<int32_t> &histogram) {
    cart_plane_params p{horizontalRange.first, horizontalRange.second, verticalRange.first, verticalRange.second, horizontalCenter, verticalCenter};
    if (cart_find_plane_params(histogram.data(), &p) < 0) throw std::runtime_error(std::string("cart_find_plane_params: ") + cart_last_error(nullptr));
    horizontalRange = std::make_pair(p.horizontal_min, p.horizontal_max);
    verticalRange = std::make_pair(p.vertical_min, p.vertical_max);
    horizontalCenter = p.horizontal_center;
    verticalCenter = p.vertical_center;
}
}  // namespace cart

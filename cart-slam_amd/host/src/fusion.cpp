// fusion.cpp -- TemporalFusionModule (cartslam_amd/modules/fusion.hpp): temporal disparity fusion through ego-motion, spec DESIGN.md S28.
#include "cartslam_amd/modules/fusion.hpp"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/motionseg.hpp"

namespace cart {
namespace {
[[noreturn]] void failAbi(const char *what) { throw std::runtime_error(std::string(what) + ": " + cart_last_error(nullptr)); }
void hipCheck(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
cart_fusion_params paramsOf(const TemporalFusionOptions &o) {
    return cart_fusion_params{o.minDisparity, o.agreeThreshold, o.splatRadius, o.maxWeight, o.minAge};
}
}  // namespace

TemporalFusionModule::TemporalFusionModule(const TemporalFusionOptions &options) : SyncWrapperSystemModule("TemporalFusion"), options(options) {
    const auto positive = [](double v) { return v > 0 && std::isfinite(v); };
    if (!positive(options.fx)) throw std::invalid_argument("fx must be a positive number (a source without calibration needs the camera keys)");
    if (!positive(options.fy)) throw std::invalid_argument("fy must be a positive number");
    if (!std::isfinite(options.cx)) throw std::invalid_argument("cx must be finite");
    if (!std::isfinite(options.cy)) throw std::invalid_argument("cy must be finite");
    if (!positive(options.baseline)) throw std::invalid_argument("baseline must be a positive number");
    // the library's own checks, without a device: everything valid gets as far as the missing object
    const cart_ego_camera cam{options.fx, options.fy, options.cx, options.cy, options.baseline};
    const cart_fusion_params p = paramsOf(options);
    (void)cart_fusion_update(nullptr, &cam, nullptr, &p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 1, 1, nullptr, 0, nullptr, 0, nullptr, 0, nullptr,
                             nullptr);
    if (std::strcmp(cart_last_error(nullptr), "bad arguments") != 0) throw std::invalid_argument(cart_last_error(nullptr));
    if (options.poseKey.empty()) throw std::invalid_argument("pose_key must name a blackboard pose");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY));
    this->requiresData.push_back(module_dependency_t(options.poseKey));
    if (options.useMotion) {
        this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION));
        this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION, -1));
    }
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY_FUSED, -1));   // one frame at a time, in order
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_FUSED);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_AGE);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_SOURCE);
    this->providesData.push_back(CARTSLAM_KEY_DISPARITY_FUSION_COUNTS);
}

TemporalFusionModule::~TemporalFusionModule() {
    cart_fusion_destroy(object);
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    if (stream) (void)hipStreamDestroy(static_cast<hipStream_t>(stream));
}

system_data_t TemporalFusionModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(CARTSLAM_KEY_DISPARITY);
    if (disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    const int rows = disparity->rows, cols = disparity->cols;
    auto ego = data.getData<EgoMotion>(options.poseKey);
    // Frame 1 has no predecessor, and a frame without an estimate keeps the previous pose: a kept pose must not warp, so the memory is dropped.
    const bool carry = data.id > 1 && ego->result.status != 0;
    std::shared_ptr<image_t> prevFused, prevAge, maskPrev, maskCur;
    const auto sized = [&](const std::shared_ptr<image_t> &m, int type) { return m && !m->empty() && m->type() == type && m->rows == rows && m->cols == cols; };
    if (carry) {
        auto before = data.getRelativeRun(-1);
        prevFused = before->getData<image_t>(CARTSLAM_KEY_DISPARITY_FUSED);
        prevAge = before->getData<image_t>(CARTSLAM_KEY_DISPARITY_AGE);
        if (!sized(prevFused, CV_16SC1) || !sized(prevAge, CV_8UC1))
            throw std::runtime_error("TemporalFusionModule: the previous frame's fused disparity is missing or of another size");
        if (options.useMotion) {
            maskPrev = before->getData<image_t>(CARTSLAM_KEY_MOTION);
            if (!sized(maskPrev, CV_8UC1)) throw std::runtime_error("TemporalFusionModule: the previous frame's motion must be a CV_8UC1 image of the disparity's size");
        }
    }
    if (options.useMotion) {
        maskCur = data.getData<image_t>(CARTSLAM_KEY_MOTION);
        if (!sized(maskCur, CV_8UC1)) throw std::runtime_error("TemporalFusionModule: motion must be a CV_8UC1 image of the disparity's size");
    }
    auto fused = std::make_shared<image_t>(rows, cols, CV_16SC1);
    auto age = std::make_shared<image_t>(rows, cols, CV_8UC1);
    auto source = std::make_shared<image_t>(rows, cols, CV_8UC1);
    auto counts = std::make_shared<FusionCounts>();
    std::lock_guard<std::mutex> lock(mutex);
    if (!object) {   // the object keeps the device of the engine it is made on, not the engine
        cart_engine_params ep;
        cart_engine_default_params(&ep);
        ep.width = cols; ep.height = rows; ep.num_disparities = 0; ep.paths = 0; ep.max_inflight = 1;
        cart_engine *engine = nullptr;
        if (cart_engine_create(&ep, &engine) != 0) failAbi("cart_engine_create");
        const int rc = cart_fusion_create(engine, cols, rows, &object);
        const std::string error = rc ? cart_last_error(nullptr) : "";
        cart_engine_destroy(engine);
        if (rc) throw std::runtime_error("cart_fusion_create: " + error);
        hipStream_t s = nullptr;
        hipCheck(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreateWithFlags");
        stream = s;
        hipCheck(hipMalloc(&dev, sizeof(FusionCounts)), "hipMalloc");
        hipCheck(hipHostMalloc(&host, sizeof(FusionCounts), hipHostMallocDefault), "hipHostMalloc");
    }
    const cart_ego_camera cam{options.fx, options.fy, options.cx, options.cy, options.baseline};
    const cart_fusion_params p = paramsOf(options);
    double rel[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) rel[4 * r + c] = ego->result.R[3 * r + c];
        rel[4 * r + 3] = ego->result.t[r];
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (cart_fusion_update(object, &cam, carry ? rel : nullptr, &p, disparity->ptr<int16_t>(), disparity->step, carry ? prevFused->ptr<int16_t>() : nullptr,
                           carry ? prevFused->step : 0, carry ? prevAge->ptr<uint8_t>() : nullptr, carry ? prevAge->step : 0,
                           maskPrev ? maskPrev->ptr<uint8_t>() : nullptr, maskPrev ? maskPrev->step : 0, maskCur ? maskCur->ptr<uint8_t>() : nullptr,
                           maskCur ? maskCur->step : 0, cols, rows, fused->ptr<int16_t>(), fused->step, age->ptr<uint8_t>(), age->step, source->ptr<uint8_t>(),
                           source->step, static_cast<int32_t *>(dev), s) != 0)
        failAbi("cart_fusion_update");
    hipCheck(hipMemcpyAsync(host, dev, sizeof(FusionCounts), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the fusion counts");
    hipCheck(hipStreamSynchronize(s), "hipStreamSynchronize");   // the frame's only blocking synchronisation
    std::memcpy(counts.get(), host, sizeof(FusionCounts));
    system_data_t out;
    out.push_back(std::make_pair(std::string(CARTSLAM_KEY_DISPARITY_FUSED), std::shared_ptr<void>(fused)));
    out.push_back(std::make_pair(std::string(CARTSLAM_KEY_DISPARITY_AGE), std::shared_ptr<void>(age)));
    out.push_back(std::make_pair(std::string(CARTSLAM_KEY_DISPARITY_SOURCE), std::shared_ptr<void>(source)));
    out.push_back(std::make_pair(std::string(CARTSLAM_KEY_DISPARITY_FUSION_COUNTS), std::shared_ptr<void>(counts)));
    return out;
}
}  // namespace cart

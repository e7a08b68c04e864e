// fusion.cpp -- TemporalFusionModule (cartslam_amd/modules/fusion.hpp): temporal disparity fusion through ego-motion, spec DESIGN.md S28.
#include "cartslam_amd/modules/fusion.hpp"

#include <cmath>
#include <cstring>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/motionseg.hpp"
#include "module_support.hpp"

namespace cart {
namespace {
cart_fusion_params paramsOf(const TemporalFusionOptions &o) {
    return cart_fusion_params{o.minDisparity, o.agreeThreshold, o.splatRadius, o.maxWeight, o.minAge};
}
}  // namespace

TemporalFusionModule::TemporalFusionModule(const TemporalFusionOptions &options) : SyncWrapperSystemModule("TemporalFusion"), options(options) {
    checkCamera(options);
    // the library's own checks, without a device: everything valid gets as far as the missing object
    const cart_ego_camera cam = cameraOf(options);
    const cart_fusion_params p = paramsOf(options);
    (void)cart_fusion_update(nullptr, &cam, nullptr, &p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 1, 1, nullptr, 0, nullptr, 0, nullptr, 0, nullptr,
                             nullptr);
    requireLibraryAccepts();
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

TemporalFusionModule::~TemporalFusionModule() { cart_fusion_destroy(object); }

system_data_t TemporalFusionModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(CARTSLAM_KEY_DISPARITY);
    if (disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    const int rows = disparity->rows, cols = disparity->cols;
    auto ego = data.getData<EgoMotion>(options.poseKey);
    // Frame 1 has no predecessor, and a frame without an estimate keeps the previous pose: a kept pose must not warp, so the memory is dropped.
    const bool carry = data.id > 1 && ego->result.status != 0;
    std::shared_ptr<image_t> prevFused, prevAge, maskPrev, maskCur;
    if (carry) {
        auto before = data.getRelativeRun(-1);
        prevFused = before->getData<image_t>(CARTSLAM_KEY_DISPARITY_FUSED);
        prevAge = before->getData<image_t>(CARTSLAM_KEY_DISPARITY_AGE);
        requireImage(prevFused, CV_16SC1, rows, cols, "TemporalFusionModule: the previous frame's fused disparity is missing or of another size");
        requireImage(prevAge, CV_8UC1, rows, cols, "TemporalFusionModule: the previous frame's fused disparity is missing or of another size");
        if (options.useMotion) {
            maskPrev = before->getData<image_t>(CARTSLAM_KEY_MOTION);
            requireImage(maskPrev, CV_8UC1, rows, cols, "TemporalFusionModule: the previous frame's motion must be a CV_8UC1 image of the disparity's size");
        }
    }
    if (options.useMotion) {
        maskCur = data.getData<image_t>(CARTSLAM_KEY_MOTION);
        requireImage(maskCur, CV_8UC1, rows, cols, "TemporalFusionModule: motion must be a CV_8UC1 image of the disparity's size");
    }
    auto fused = std::make_shared<image_t>(rows, cols, CV_16SC1);
    auto age = std::make_shared<image_t>(rows, cols, CV_8UC1);
    auto source = std::make_shared<image_t>(rows, cols, CV_8UC1);
    auto counts = std::make_shared<FusionCounts>();
    std::lock_guard<std::mutex> lock(mutex);
    if (!object) {   // the object keeps the device of the engine it is made on, not the engine
        makeOnPostEngine(cols, rows, [&](cart_engine *e) { return cart_fusion_create(e, cols, rows, &object) ? "cart_fusion_create" : nullptr; });
        scratch.create();
        scratch.reserve(sizeof(FusionCounts), sizeof(FusionCounts));
    }
    const cart_ego_camera cam = cameraOf(options);
    const cart_fusion_params p = paramsOf(options);
    double rel[12];
    pose12(ego->result, rel);
    hipStream_t s = scratch.stream();
    if (cart_fusion_update(object, &cam, carry ? rel : nullptr, &p, disparity->ptr<int16_t>(), disparity->step, carry ? prevFused->ptr<int16_t>() : nullptr,
                           carry ? prevFused->step : 0, carry ? prevAge->ptr<uint8_t>() : nullptr, carry ? prevAge->step : 0,
                           maskPrev ? maskPrev->ptr<uint8_t>() : nullptr, maskPrev ? maskPrev->step : 0, maskCur ? maskCur->ptr<uint8_t>() : nullptr,
                           maskCur ? maskCur->step : 0, cols, rows, fused->ptr<int16_t>(), fused->step, age->ptr<uint8_t>(), age->step, source->ptr<uint8_t>(),
                           source->step, scratch.dev<int32_t>(), s) != 0)
        failAbi("cart_fusion_update");
    hipCheck(hipMemcpyAsync(scratch.host(), scratch.dev(), sizeof(FusionCounts), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the fusion counts");
    scratch.wait();   // the frame's only blocking synchronisation
    std::memcpy(counts.get(), scratch.host(), sizeof(FusionCounts));
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_DISPARITY_FUSED, fused), MODULE_PAIR(CARTSLAM_KEY_DISPARITY_AGE, age),
                             MODULE_PAIR(CARTSLAM_KEY_DISPARITY_SOURCE, source), MODULE_PAIR(CARTSLAM_KEY_DISPARITY_FUSION_COUNTS, counts));
}
}  // namespace cart

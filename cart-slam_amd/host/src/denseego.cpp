// denseego.cpp -- DenseEgoModule (cartslam_amd/modules/denseego.hpp): dense refinement of the relative pose, spec DESIGN.md S26.
#include "cartslam_amd/modules/denseego.hpp"

#include <cmath>
#include <cstring>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/motionseg.hpp"
#include "cartslam_amd/modules/planeseg.hpp"
#include "module_support.hpp"

namespace cart {
namespace {
cart_dense_ego_params paramsOf(const DenseEgoOptions &o) {
    return cart_dense_ego_params{o.minDisparity, o.flowThreshold, o.disparityThreshold, o.disparityWeight, o.iterations, o.stride, o.minInliers};
}
}  // namespace

bool acceptDenseEgo(const cart_dense_ego_result &r) {
    if (r.status != 1 || r.n_inliers < r.n_initial) return false;
    for (double v : r.R)
        if (!std::isfinite(v)) return false;
    for (double v : r.t)
        if (!std::isfinite(v)) return false;
    return true;
}

bool acceptModelTrack(const cart_model_track_result &r, int minInliers) {
    if (r.status != 1 || r.n_inliers < minInliers || !(r.rms <= r.rms_initial) || !std::isfinite(r.rms) || !std::isfinite(r.rms_initial)) return false;
    for (double v : r.R)
        if (!std::isfinite(v)) return false;
    for (double v : r.t)
        if (!std::isfinite(v)) return false;
    return true;
}

bool acceptModelTrackColor(const cart_model_track_color_result &r, int minInliers) {
    if (r.status != 1 || r.n_inliers < minInliers || !(r.cost <= r.cost_initial)) return false;
    for (double v : {r.rms_initial, r.rms, r.rms_photo_initial, r.rms_photo, r.cost_initial, r.cost})
        if (!std::isfinite(v)) return false;
    for (double v : r.R)
        if (!std::isfinite(v)) return false;
    for (double v : r.t)
        if (!std::isfinite(v)) return false;
    return true;
}

DenseEgoModule::DenseEgoModule(const DenseEgoOptions &options) : SyncWrapperSystemModule("DenseEgo"), options(options) {
    checkCamera(options);
    // the library's own checks, without a device: everything valid gets as far as the missing object
    const cart_ego_camera cam = cameraOf(options);
    const cart_dense_ego_params p = paramsOf(options);
    (void)cart_dense_ego_refine(nullptr, &cam, kIdentityPose, &p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 1, 1, nullptr, nullptr);
    requireLibraryAccepts();
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY, -1));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_OPTFLOW));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_EGO_MOTION));
    if (options.useMotion) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DENSE_EGO, -1));   // the pose chains on the previous frame's
    this->providesData.push_back(CARTSLAM_KEY_DENSE_EGO);
    this->providesData.push_back(CARTSLAM_KEY_DENSE_EGO_RESULT);
}

DenseEgoModule::~DenseEgoModule() { cart_dense_ego_destroy(object); }

system_data_t DenseEgoModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(CARTSLAM_KEY_DISPARITY);
    if (disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    const int rows = disparity->rows, cols = disparity->cols;
    auto ego = data.getData<EgoMotion>(CARTSLAM_KEY_EGO_MOTION);
    std::shared_ptr<EgoMotion> before;
    if (data.id > 1) before = data.getRelativeRun(-1)->getData<EgoMotion>(CARTSLAM_KEY_DENSE_EGO);
    auto dense = std::make_shared<cart_dense_ego_result>();   // status 0 with ego_motion's pose for a frame without an estimate
    std::memset(dense.get(), 0, sizeof(*dense));
    std::memcpy(dense->R, ego->result.R, sizeof(dense->R));
    std::memcpy(dense->t, ego->result.t, sizeof(dense->t));
    if (data.id > 1 && ego->result.status != 0) {
        auto previous = data.getRelativeRun(-1)->getData<image_t>(CARTSLAM_KEY_DISPARITY);
        auto flow = data.getData<image_t>(CARTSLAM_KEY_OPTFLOW);
        requireImage(previous, CV_16SC1, rows, cols, "DenseEgoModule: the previous frame's disparity is missing or of another size");
        requireImage(flow, CV_16SC2, rows, cols, "DenseEgoModule: optflow must be a CV_16SC2 image of the disparity's size");
        std::shared_ptr<image_t> mask;
        if (options.useMotion) {
            mask = data.getData<image_t>(CARTSLAM_KEY_MOTION);
            requireImage(mask, CV_8UC1, rows, cols, "DenseEgoModule: motion must be a CV_8UC1 image of the disparity's size");
        }
        std::lock_guard<std::mutex> lock(mutex);
        if (!object) {   // the object keeps the device of the engine it is made on, not the engine
            makeOnPostEngine(cols, rows, [&](cart_engine *e) { return cart_dense_ego_create(e, cols, rows, &object) ? "cart_dense_ego_create" : nullptr; });
            scratch.create();
            scratch.reserve(sizeof(cart_dense_ego_result), sizeof(cart_dense_ego_result));
        }
        const cart_ego_camera cam = cameraOf(options);
        const cart_dense_ego_params p = paramsOf(options);
        double rel0[12];
        pose12(ego->result, rel0);
        hipStream_t s = scratch.stream();
        if (cart_dense_ego_refine(object, &cam, rel0, &p, disparity->ptr<int16_t>(), disparity->step, previous->ptr<int16_t>(), previous->step,
                                  flow->ptr<int16_t>(), flow->step, mask ? mask->ptr<uint8_t>() : nullptr, mask ? mask->step : 0, cols, rows,
                                  scratch.dev<cart_dense_ego_result>(), s) != 0)
            failAbi("cart_dense_ego_refine");
        hipCheck(hipMemcpyAsync(scratch.host(), scratch.dev(), sizeof(cart_dense_ego_result), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the dense ego-motion result");
        scratch.wait();   // the frame's only blocking synchronisation
        std::memcpy(dense.get(), scratch.host(), sizeof(*dense));
    }
    // what is chained: the accepted refined pose, else ego_motion's relative pose if it has one, else the pose is kept
    auto result = std::make_shared<EgoMotion>();
    result->result = ego->result;
    if (acceptDenseEgo(*dense)) {
        std::memcpy(result->result.R, dense->R, sizeof(dense->R));
        std::memcpy(result->result.t, dense->t, sizeof(dense->t));
    }
    chainPose(before ? before->pose : kIdentityPose, result->result, result->pose);
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_DENSE_EGO, result), MODULE_PAIR(CARTSLAM_KEY_DENSE_EGO_RESULT, dense));
}
}  // namespace cart

// denseego.cpp -- DenseEgoModule (cartslam_amd/modules/denseego.hpp): dense refinement of the relative pose, spec DESIGN.md S26.
#include "cartslam_amd/modules/denseego.hpp"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/motionseg.hpp"
#include "cartslam_amd/modules/planeseg.hpp"

namespace cart {
namespace {
[[noreturn]] void failAbi(const char *what) { throw std::runtime_error(std::string(what) + ": " + cart_last_error(nullptr)); }
void hipCheck(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
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

DenseEgoModule::DenseEgoModule(const DenseEgoOptions &options) : SyncWrapperSystemModule("DenseEgo"), options(options) {
    const auto positive = [](double v) { return v > 0 && std::isfinite(v); };
    if (!positive(options.fx)) throw std::invalid_argument("fx must be a positive number (a source without calibration needs the camera keys)");
    if (!positive(options.fy)) throw std::invalid_argument("fy must be a positive number");
    if (!std::isfinite(options.cx)) throw std::invalid_argument("cx must be finite");
    if (!std::isfinite(options.cy)) throw std::invalid_argument("cy must be finite");
    if (!positive(options.baseline)) throw std::invalid_argument("baseline must be a positive number");
    // the library's own checks, without a device: everything valid gets as far as the missing object
    const cart_ego_camera cam{options.fx, options.fy, options.cx, options.cy, options.baseline};
    const cart_dense_ego_params p = paramsOf(options);
    static const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    (void)cart_dense_ego_refine(nullptr, &cam, identity, &p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 1, 1, nullptr, nullptr);
    if (std::strcmp(cart_last_error(nullptr), "bad arguments") != 0) throw std::invalid_argument(cart_last_error(nullptr));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY, -1));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_OPTFLOW));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_EGO_MOTION));
    if (options.useMotion) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DENSE_EGO, -1));   // the pose chains on the previous frame's
    this->providesData.push_back(CARTSLAM_KEY_DENSE_EGO);
    this->providesData.push_back(CARTSLAM_KEY_DENSE_EGO_RESULT);
}

DenseEgoModule::~DenseEgoModule() {
    cart_dense_ego_destroy(object);
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    if (stream) (void)hipStreamDestroy(static_cast<hipStream_t>(stream));
}

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
        if (!previous || previous->type() != CV_16SC1 || previous->rows != rows || previous->cols != cols)
            throw std::runtime_error("DenseEgoModule: the previous frame's disparity is missing or of another size");
        if (!flow || flow->type() != CV_16SC2 || flow->rows != rows || flow->cols != cols)
            throw std::runtime_error("DenseEgoModule: optflow must be a CV_16SC2 image of the disparity's size");
        std::shared_ptr<image_t> mask;
        if (options.useMotion) {
            mask = data.getData<image_t>(CARTSLAM_KEY_MOTION);
            if (!mask || mask->type() != CV_8UC1 || mask->rows != rows || mask->cols != cols)
                throw std::runtime_error("DenseEgoModule: motion must be a CV_8UC1 image of the disparity's size");
        }
        std::lock_guard<std::mutex> lock(mutex);
        if (!object) {   // the object keeps the device of the engine it is made on, not the engine
            cart_engine_params ep;
            cart_engine_default_params(&ep);
            ep.width = cols; ep.height = rows; ep.num_disparities = 0; ep.paths = 0; ep.max_inflight = 1;
            cart_engine *engine = nullptr;
            if (cart_engine_create(&ep, &engine) != 0) failAbi("cart_engine_create");
            const int rc = cart_dense_ego_create(engine, cols, rows, &object);
            const std::string error = rc ? cart_last_error(nullptr) : "";
            cart_engine_destroy(engine);
            if (rc) throw std::runtime_error("cart_dense_ego_create: " + error);
            hipStream_t s = nullptr;
            hipCheck(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreateWithFlags");
            stream = s;
            hipCheck(hipMalloc(&dev, sizeof(cart_dense_ego_result)), "hipMalloc");
            hipCheck(hipHostMalloc(&host, sizeof(cart_dense_ego_result), hipHostMallocDefault), "hipHostMalloc");
        }
        const cart_ego_camera cam{options.fx, options.fy, options.cx, options.cy, options.baseline};
        const cart_dense_ego_params p = paramsOf(options);
        double rel0[12];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) rel0[4 * r + c] = ego->result.R[3 * r + c];
            rel0[4 * r + 3] = ego->result.t[r];
        }
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (cart_dense_ego_refine(object, &cam, rel0, &p, disparity->ptr<int16_t>(), disparity->step, previous->ptr<int16_t>(), previous->step,
                                  flow->ptr<int16_t>(), flow->step, mask ? mask->ptr<uint8_t>() : nullptr, mask ? mask->step : 0, cols, rows,
                                  static_cast<cart_dense_ego_result *>(dev), s) != 0)
            failAbi("cart_dense_ego_refine");
        hipCheck(hipMemcpyAsync(host, dev, sizeof(cart_dense_ego_result), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the dense ego-motion result");
        hipCheck(hipStreamSynchronize(s), "hipStreamSynchronize");   // the frame's only blocking synchronisation
        std::memcpy(dense.get(), host, sizeof(*dense));
    }
    // what is chained: the accepted refined pose, else ego_motion's relative pose if it has one, else the pose is kept
    auto result = std::make_shared<EgoMotion>();
    result->result = ego->result;
    if (acceptDenseEgo(*dense)) {
        std::memcpy(result->result.R, dense->R, sizeof(dense->R));
        std::memcpy(result->result.t, dense->t, sizeof(dense->t));
    }
    static const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    chainPose(before ? before->pose : identity, result->result, result->pose);
    system_data_t out;
    out.push_back(std::make_pair(std::string(CARTSLAM_KEY_DENSE_EGO), std::shared_ptr<void>(result)));
    out.push_back(std::make_pair(std::string(CARTSLAM_KEY_DENSE_EGO_RESULT), std::shared_ptr<void>(dense)));
    return out;
}
}  // namespace cart

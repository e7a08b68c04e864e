// egomotion.cpp -- EgoMotionModule and chainPose (cartslam_amd/modules/egomotion.hpp): stereo visual odometry, spec DESIGN.md S23.
#include <atomic>

#include "cartslam_amd/modules/egomotion.hpp"
#include "module_support.hpp"

namespace cart {
// ---------------------------------------------------------------- ego-motion (extension)
// The landmarks are a device buffer the frame owns (the next frame reads them there); the result comes to the host through the
// slot's pinned buffer.  The objects are made for the capacity of the first frame's feature sets.
class EgoPool : public DeviceObjectPool<cart_ego, cart_ego_destroy> {
   public:
    EgoPool() : DeviceObjectPool("cart_ego_create", [this](cart_engine *e, Size, cart_ego **g) { return cart_ego_create(e, capacity.load(), g); }) {}
    std::atomic<int> capacity{0};
};

void chainPose(const double previous[12], const cart_ego_result &rel, double out[12]) {
    if (!rel.status) {
        for (int k = 0; k < 12; ++k) out[k] = previous[k];
        return;
    }
    double Ri[9], ti[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ri[3 * r + c] = rel.R[3 * c + r];
    for (int r = 0; r < 3; ++r) ti[r] = -((Ri[3 * r] * rel.t[0] + Ri[3 * r + 1] * rel.t[1]) + Ri[3 * r + 2] * rel.t[2]);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = (previous[4 * r] * Ri[c] + previous[4 * r + 1] * Ri[3 + c]) + previous[4 * r + 2] * Ri[6 + c];
        out[4 * r + 3] = ((previous[4 * r] * ti[0] + previous[4 * r + 1] * ti[1]) + previous[4 * r + 2] * ti[2]) + previous[4 * r + 3];
    }
}

EgoMotionModule::EgoMotionModule(const EgoMotionOptions &options) : SyncWrapperSystemModule("EgoMotion"), options(options), pool(std::make_shared<EgoPool>()) {
    checkCamera(options);
    if (!positiveNumber(options.minDisparity)) throw std::invalid_argument("min_disparity must be a positive number");
    if (!positiveNumber(options.inlierThreshold)) throw std::invalid_argument("inlier_threshold must be a positive number");
    if (options.hypotheses < 1 || options.hypotheses > CART_EGO_MAX_HYPOTHESES) throw std::invalid_argument("hypotheses must be in [1, 1024]");
    if (options.refineIterations < 0 || options.refineIterations > CART_EGO_MAX_REFINE) throw std::invalid_argument("refine_iterations must be in [0, 16]");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_FEATURES));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_FEATURE_MATCHES));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_EGO_MOTION, -1));
    this->providesData.push_back(CARTSLAM_KEY_EGO_MOTION);
}
EgoMotionModule::~EgoMotionModule() = default;

system_data_t EgoMotionModule::runInternal(System &, SystemRunData &data) {
    typedef std::pair<ImageFeatures, ImageFeatures> features_t;
    auto features = data.getData<features_t>(CARTSLAM_KEY_FEATURES);
    auto matches = data.getData<FeatureMatches>(CARTSLAM_KEY_FEATURE_MATCHES);
    std::shared_ptr<EgoMotion> previous;
    if (data.id > 1) previous = data.getRelativeRun(-1)->getData<EgoMotion>(CARTSLAM_KEY_EGO_MOTION);
    const ImageFeatures &left = features->first, &right = features->second;
    if (!left.onDevice() || !right.onDevice() || !matches->onDevice())
        throw std::runtime_error("EgoMotionModule requires features and matches that are still on the device");
    const int n = left.deviceCapacity();
    int expected = 0;
    if (!pool->capacity.compare_exchange_strong(expected, n) && expected != n)
        throw std::runtime_error("EgoMotionModule: the feature capacity changed between frames");
    if (right.deviceCapacity() != n || matches->deviceCapacity() != n) throw std::runtime_error("EgoMotionModule: feature and match sets of different capacities");
    if (data.dataElement->type != DataElementType::STEREO) throw std::runtime_error("EgoMotionModule requires StereoDataElement");
    const image_t &image = std::static_pointer_cast<StereoDataElement>(data.dataElement)->left;   // sizes the pool's engine, as for the ORB pool
    auto eng = pool->engineFor(image);
    EgoPool::Lease lease{*pool, pool->acquire(image)};
    EgoPool::Slot &sl = *lease.slot;
    sl.reserve(sizeof(cart_ego_result), sizeof(cart_ego_result));
    const cart_ego_camera cam = cameraOf(options);
    const cart_ego_params p{options.minDisparity, options.inlierThreshold, options.hypotheses, options.refineIterations};
    auto result = std::make_shared<EgoMotion>();
    result->landmarks = image_t(1, (int)((size_t)n * 4 * sizeof(double)), CV_8UC1);
    ScopedStream stream;
    if (cart_ego_triangulate(sl.obj, &cam, &p, left.deviceKeypoints(), right.deviceKeypoints(), left.deviceCount(), matches->deviceMatches(0),
                             matches->deviceCount(0), result->landmarks.ptr<double>(), stream.s) != 0)
        eng->fail("cart_ego_triangulate");
    cart_ego_result rel{};
    rel.R[0] = rel.R[4] = rel.R[8] = 1.0;
    rel.best_hypothesis = -1;
    if (previous) {
        if (previous->landmarks.empty() || previous->landmarks.cols != result->landmarks.cols)
            throw std::runtime_error("EgoMotionModule: the previous frame's landmarks are missing or of another capacity");
        if (cart_ego_estimate(sl.obj, &cam, &p, result->landmarks.ptr<double>(), left.deviceKeypoints(), previous->landmarks.ptr<double>(),
                              matches->deviceMatches(1), matches->deviceCount(1), options.seed, data.id, sl.dev<cart_ego_result>(), nullptr,
                              stream.s) != 0)
            eng->fail("cart_ego_estimate");
        hipCheck(hipMemcpyAsync(sl.host(), sl.dev(), sizeof(cart_ego_result), hipMemcpyDeviceToHost, stream.s), "hipMemcpyAsync of the ego-motion result");
    }
    stream.wait();   // the frame's only blocking synchronisation
    if (previous) std::memcpy(&rel, sl.host(), sizeof(rel));
    result->result = rel;
    chainPose(previous ? previous->pose : kIdentityPose, rel, result->pose);
    return MODULE_RETURN(CARTSLAM_KEY_EGO_MOTION, result);
}
}  // namespace cart

// localba.cpp -- LocalBAModule (cartslam_amd/modules/localba.hpp): windowed bundle adjustment over the last frames, spec DESIGN.md S32.
#include "cartslam_amd/modules/localba.hpp"

#include <cstring>

#include "cartslam_amd/modules/denseego.hpp"
#include "module_support.hpp"

namespace cart {
namespace {
// the module's buffers: the result record and the counts (80 bytes with the padding), the window's poses before the optimise, after it, the ids
constexpr size_t kCountsAt = sizeof(cart_local_ba_result), kCarriedAt = sizeof(LocalBARecord);

// inv(a) b for (R | t) 3 x 4 in row order: inv = (R^T, -(R^T t)), every sum left to right (S29's products)
void relativePose(const double a[12], const double b[12], double R[9], double t[3]) {
    double inv[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) inv[4 * r + c] = a[4 * c + r];
    for (int r = 0; r < 3; ++r) inv[4 * r + 3] = -((inv[4 * r] * a[3] + inv[4 * r + 1] * a[7]) + inv[4 * r + 2] * a[11]);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (inv[4 * r] * b[c] + inv[4 * r + 1] * b[4 + c]) + inv[4 * r + 2] * b[8 + c];
        t[r] = ((inv[4 * r] * b[3] + inv[4 * r + 1] * b[7]) + inv[4 * r + 2] * b[11]) + inv[4 * r + 3];
    }
}
}  // namespace

LocalBAModule::LocalBAModule(const LocalBAOptions &options) : SyncWrapperSystemModule("LocalBA"), options(options) {
    checkCamera(options);
    // the library's own checks, without a device: everything valid gets as far as the missing engine / object
    cart_local_ba *none = nullptr;
    (void)cart_local_ba_create(nullptr, 1, options.window, options.maxPoints, &none);
    requireLibraryAccepts();
    const cart_ego_camera cam = cameraOf(options);
    const cart_local_ba_params p{options.minDisparity, options.huber, options.damping, options.iterations, options.minObservations, options.minFrameObservations};
    (void)cart_local_ba_optimize(nullptr, &cam, &p, nullptr, nullptr);
    requireLibraryAccepts("ba is NULL");
    if (options.interval < 1) throw std::invalid_argument("interval must be at least 1");
    if (options.poseKey != CARTSLAM_KEY_EGO_MOTION && options.poseKey != CARTSLAM_KEY_DENSE_EGO)
        throw std::invalid_argument("pose_key must be \"ego_motion\" or \"dense_ego\"");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_FEATURES));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_FEATURE_MATCHES));
    this->requiresData.push_back(module_dependency_t(options.poseKey));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_LOCAL_BA, -1));   // frames pass in order: the window grows in frame order
    this->providesData.push_back(CARTSLAM_KEY_LOCAL_BA);
    this->providesData.push_back(CARTSLAM_KEY_LOCAL_BA_RESULT);
    this->providesData.push_back(CARTSLAM_KEY_LOCAL_BA_WINDOW);
}

LocalBAModule::~LocalBAModule() { cart_local_ba_destroy(ba); }

system_data_t LocalBAModule::runInternal(System &, SystemRunData &data) {
    typedef std::pair<ImageFeatures, ImageFeatures> features_t;
    auto features = data.getData<features_t>(CARTSLAM_KEY_FEATURES);
    auto matches = data.getData<FeatureMatches>(CARTSLAM_KEY_FEATURE_MATCHES);
    auto source = data.getData<EgoMotion>(options.poseKey);
    const ImageFeatures &left = features->first, &right = features->second;
    if (!left.onDevice() || !right.onDevice() || !matches->onDevice())
        throw std::runtime_error("LocalBAModule requires features and matches that are still on the device");
    const int n = left.deviceCapacity();
    if (right.deviceCapacity() != n || matches->deviceCapacity() != n) throw std::runtime_error("LocalBAModule: feature and match sets of different capacities");
    const size_t w = (size_t)options.window, poseBytes = w * 12 * sizeof(double);
    const size_t finalAt = kCarriedAt + poseBytes, idsAt = finalAt + poseBytes, bytes = idsAt + w * sizeof(uint64_t);
    auto record = std::make_shared<LocalBARecord>();
    std::memset(record.get(), 0, sizeof(*record));
    auto window = std::make_shared<LocalBAWindow>();
    auto result = std::make_shared<EgoMotion>();
    result->result = source->result;
    result->landmarks = source->landmarks;
    std::lock_guard<std::mutex> lock(mutex);
    if (!ba) {   // the object keeps the device of the engine it is made on, not the engine
        makeOnPostEngine(64, 32, [&](cart_engine *e) { return cart_local_ba_create(e, n, options.window, options.maxPoints, &ba) ? "cart_local_ba_create" : nullptr; });
        capacity = n;
        scratch.create();
        scratch.reserve(bytes, bytes);
    } else if (capacity != n) {
        throw std::runtime_error("LocalBAModule: the feature capacity changed between frames");
    }
    hipStream_t s = scratch.stream();
    uint8_t *d = scratch.dev<uint8_t>(), *h = scratch.host<uint8_t>();
    const cart_ego_camera cam = cameraOf(options);
    const cart_local_ba_params p{options.minDisparity, options.huber, options.damping, options.iterations, options.minObservations, options.minFrameObservations};
    const bool restart = source->result.status == 0;   // no pose between this frame and the one before: the tracks cannot be continued
    if (restart && cart_local_ba_clear(ba, s) != 0) failAbi("cart_local_ba_clear");
    if (cart_local_ba_push(ba, &cam, &p, data.id, source->pose, left.deviceKeypoints(), right.deviceKeypoints(), left.deviceCount(), matches->deviceMatches(0),
                           matches->deviceCount(0), matches->deviceMatches(1), matches->deviceCount(1), reinterpret_cast<int32_t *>(d + kCountsAt), s) != 0)
        failAbi("cart_local_ba_push");
    if (cart_local_ba_poses(ba, reinterpret_cast<double *>(d + kCarriedAt), nullptr, s) != 0) failAbi("cart_local_ba_poses");
    const bool optimise = !restart && data.id % (uint32_t)options.interval == 0;
    if (optimise && cart_local_ba_optimize(ba, &cam, &p, reinterpret_cast<cart_local_ba_result *>(d), s) != 0) failAbi("cart_local_ba_optimize");
    if (cart_local_ba_poses(ba, reinterpret_cast<double *>(d + finalAt), reinterpret_cast<uint64_t *>(d + idsAt), s) != 0) failAbi("cart_local_ba_poses");
    const size_t from = optimise ? 0 : kCountsAt;
    hipCheck(hipMemcpyAsync(h + from, d + from, bytes - from, hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the local bundle adjustment's window");
    scratch.wait();   // the frame's only blocking synchronisation
    if (optimise) std::memcpy(&record->result, h, sizeof(record->result));
    std::memcpy(record->counts, h + kCountsAt, sizeof(record->counts));
    record->optimised = optimise ? 1 : 0;
    record->taken = optimise && record->result.status == 1 && record->result.cost_after <= record->result.cost_before ? 1 : 0;
    const double *poses = reinterpret_cast<const double *>(h + (record->taken ? finalAt : kCarriedAt));
    const int frames = record->counts[7];
    if (frames < 1 || frames > options.window) throw std::runtime_error("LocalBAModule: the window reports " + std::to_string(frames) + " frames");
    std::memcpy(result->pose, poses + (size_t)(frames - 1) * 12, sizeof(result->pose));
    if (!restart && frames >= 2) relativePose(result->pose, poses + (size_t)(frames - 2) * 12, result->result.R, result->result.t);
    const double *final = reinterpret_cast<const double *>(h + finalAt);
    const uint64_t *ids = reinterpret_cast<const uint64_t *>(h + idsAt);
    window->poses.assign(final, final + w * 12);
    window->ids.assign(ids, ids + w);
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_LOCAL_BA, result), MODULE_PAIR(CARTSLAM_KEY_LOCAL_BA_RESULT, record), MODULE_PAIR(CARTSLAM_KEY_LOCAL_BA_WINDOW, window));
}
}  // namespace cart

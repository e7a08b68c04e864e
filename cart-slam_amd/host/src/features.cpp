// features.cpp -- the ORB detector and matcher modules with their pools (cartslam_amd/modules/features.hpp, matches.hpp).
#include <atomic>

#include "cartslam_amd/modules/features.hpp"
#include "cartslam_amd/modules/matches.hpp"
#include "module_support.hpp"

namespace cart {
// ---------------------------------------------------------------- ORB features (features.cpp:10-66)
// The frame's counts and keypoints are written into a device buffer the frame owns (the matcher reads them there) and downloaded
// through the slot's pinned buffer; the descriptors are the frame's own output images, like every other module's outputs.
class OrbPool : public DeviceObjectPool<cart_orb, cart_orb_destroy> {
   public:
    explicit OrbPool(int nfeatures)
        : DeviceObjectPool("cart_orb_create",
                           [nfeatures](cart_engine *e, Size res, cart_orb **o) { return cart_orb_create(e, res.width, res.height, nfeatures, o); }),
          nfeatures(nfeatures) {}
    size_t bytes() const { return 16 + 2 * (size_t)nfeatures * sizeof(KeyPoint); }   // counts [2] int32 + 8 B padding | keypoints [2][nfeatures]
    const int nfeatures;
};

std::pair<ImageFeatures, ImageFeatures> detectOrbFeatures(OrbPool &pool, const image_t &left, const image_t &right) {
    const int channels = left.type() == CV_8UC3 ? 3 : 1;
    if ((left.type() != CV_8UC3 && left.type() != CV_8UC1) || right.type() != left.type() || right.cols != left.cols || right.rows != left.rows)
        throw std::runtime_error("ImageFeatureDetectorModule requires two CV_8UC1 or CV_8UC3 images of one size");
    auto eng = pool.engineFor(left);
    OrbPool::Lease lease{pool, pool.acquire(left)};
    OrbPool::Slot &sl = *lease.slot;
    sl.reserve(0, pool.bytes());
    const int n = pool.nfeatures;
    image_t desc[2] = {image_t(n, CART_ORB_DESCRIPTOR_BYTES, CV_8UC1), image_t(n, CART_ORB_DESCRIPTOR_BYTES, CV_8UC1)};
    image_t records(1, (int)pool.bytes(), CV_8UC1);
    int32_t *countsDev = records.ptr<int32_t>();
    KeyPoint *kpDev = reinterpret_cast<KeyPoint *>(records.ptr<uint8_t>() + 16);
    const uint8_t *images[2] = {left.ptr<uint8_t>(), right.ptr<uint8_t>()};
    const size_t steps[2] = {left.step, right.step}, descSteps[2] = {desc[0].step, desc[1].step};
    cart_keypoint *kps[2] = {kpDev, kpDev + n};
    uint8_t *descs[2] = {desc[0].ptr<uint8_t>(), desc[1].ptr<uint8_t>()};
    ScopedStream stream;
    if (cart_orb_detect(sl.obj, 2, images, steps, channels, left.cols, left.rows, kps, descs, descSteps, countsDev, stream.s) != 0)
        eng->fail("cart_orb_detect");
    hipCheck(hipMemcpyAsync(sl.host(), records.data, pool.bytes(), hipMemcpyDeviceToHost, stream.s), "hipMemcpyAsync of the keypoints");
    stream.wait();   // the frame's only blocking synchronisation (the reference's orb->convert)
    const int32_t *counts = sl.host<int32_t>();
    const KeyPoint *kpHost = reinterpret_cast<const KeyPoint *>(sl.host<uint8_t>() + 16);
    std::vector<ImageFeatures> out;
    for (int i = 0; i < 2; ++i) {
        if (counts[i] < 0 || counts[i] > n) throw std::runtime_error("cart_orb_detect: keypoint count out of range");
        desc[i].rows = counts[i];   // the first counts[i] rows are the descriptors
        out.emplace_back(std::vector<KeyPoint>(kpHost + (size_t)i * n, kpHost + (size_t)i * n + counts[i]), desc[i], records, (size_t)i * 4,
                         16 + (size_t)i * n * sizeof(KeyPoint), n);
    }
    return std::make_pair(out[0], out[1]);
}

ImageFeatureDetectorModule::ImageFeatureDetectorModule(int nfeatures) : SyncWrapperSystemModule("ImageFeatureDetector") {
    if (nfeatures < 1 || nfeatures > CART_ORB_MAX_FEATURES) throw std::invalid_argument("nfeatures must be in [1, 65536]");
    pool = std::make_shared<OrbPool>(nfeatures);
    this->providesData.push_back(CARTSLAM_KEY_FEATURES);
}
ImageFeatureDetectorModule::~ImageFeatureDetectorModule() = default;

system_data_t ImageFeatureDetectorModule::runInternal(System &, SystemRunData &data) {
    if (data.dataElement->type != DataElementType::STEREO) throw std::runtime_error("ImageFeatureDetectorModule requires StereoDataElement");
    auto stereo = std::static_pointer_cast<StereoDataElement>(data.dataElement);   // ImageFeatureDetectorVisitor::visitStereo
    auto result = std::make_shared<std::pair<ImageFeatures, ImageFeatures>>(detectOrbFeatures(*pool, stereo->left, stereo->right));
    return MODULE_RETURN(CARTSLAM_KEY_FEATURES, result);
}
// ---------------------------------------------------------------- ORB matches (extension)
// The frame's two match lists and their counts are written into a device buffer the frame owns (the ego-motion module reads them
// there) and downloaded through the slot's pinned buffer.  The matchers are made for the capacity of the first frame's feature sets (the "features" module's nfeatures).
class MatcherPool : public DeviceObjectPool<cart_matcher, cart_matcher_destroy> {
   public:
    MatcherPool() : DeviceObjectPool("cart_matcher_create", [this](cart_engine *e, Size, cart_matcher **m) { return cart_matcher_create(e, capacity.load(), m); }) {}
    size_t bytes(int n) const { return 16 + 2 * (size_t)n * sizeof(FeatureMatch); }   // counts [2] int32 + 8 B padding | matches [2][capacity]
    std::atomic<int> capacity{0};
};

FeatureMatcherModule::FeatureMatcherModule(const FeatureMatcherOptions &options)
    : SyncWrapperSystemModule("FeatureMatcher"), options(options), pool(std::make_shared<MatcherPool>()) {
    if (options.maxDistance < 0 || options.maxDistance > 256) throw std::invalid_argument("max_distance must be in [0, 256]");
    if (options.ratio < 0 || options.ratio > 100) throw std::invalid_argument("ratio must be in [0, 100]");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_FEATURES));
    if (options.temporal) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_FEATURES, -1));
    this->providesData.push_back(CARTSLAM_KEY_FEATURE_MATCHES);
}
FeatureMatcherModule::~FeatureMatcherModule() = default;

system_data_t FeatureMatcherModule::runInternal(System &, SystemRunData &data) {
    typedef std::pair<ImageFeatures, ImageFeatures> features_t;
    auto current = data.getData<features_t>(CARTSLAM_KEY_FEATURES);
    std::shared_ptr<features_t> previous;
    if (options.temporal && data.id > 1) previous = data.getRelativeRun(-1)->getData<features_t>(CARTSLAM_KEY_FEATURES);
    const ImageFeatures &left = current->first;
    if (!left.onDevice() || !current->second.onDevice() || (previous && !previous->first.onDevice()))
        throw std::runtime_error("FeatureMatcherModule requires features that are still on the device");
    const int n = left.deviceCapacity();
    int expected = 0;
    if (!pool->capacity.compare_exchange_strong(expected, n) && expected != n)
        throw std::runtime_error("FeatureMatcherModule: the feature capacity changed between frames");
    if (current->second.deviceCapacity() != n || (previous && previous->first.deviceCapacity() != n))
        throw std::runtime_error("FeatureMatcherModule: feature sets of different capacities");
    if (data.dataElement->type != DataElementType::STEREO) throw std::runtime_error("FeatureMatcherModule requires StereoDataElement");
    const image_t &image = std::static_pointer_cast<StereoDataElement>(data.dataElement)->left;   // sizes the pool's engine, as for the ORB pool
    auto eng = pool->engineFor(image);
    MatcherPool::Lease lease{*pool, pool->acquire(image)};
    MatcherPool::Slot &sl = *lease.slot;
    sl.reserve(0, pool->bytes(n));
    image_t records(1, (int)pool->bytes(n), CV_8UC1);
    int32_t *countsDev = records.ptr<int32_t>();
    FeatureMatch *matchesDev = reinterpret_cast<FeatureMatch *>(records.ptr<uint8_t>() + 16);
    cart_match_params p;
    cart_match_default_params(&p);
    p.use_gate = 1; p.max_octave_diff = 1;
    p.max_distance = options.maxDistance; p.ratio = options.ratio; p.cross_check = options.crossCheck ? 1 : 0;
    ScopedStream stream;
    hipCheck(hipMemsetAsync(countsDev, 0, 16, stream.s), "hipMemsetAsync of the match counts");
    auto match = [&](const ImageFeatures &q, const ImageFeatures &t, int list) {
        if (cart_matcher_match(sl.obj, &p, q.descriptors.ptr<uint8_t>(), q.descriptors.step, q.deviceKeypoints(), q.deviceCount(),
                               t.descriptors.ptr<uint8_t>(), t.descriptors.step, t.deviceKeypoints(), t.deviceCount(), matchesDev + (size_t)list * n,
                               countsDev + list, nullptr, stream.s) != 0)
            eng->fail("cart_matcher_match");
    };
    if (options.stereo) {
        p.dx_min = 0.f; p.dx_max = options.maxDisparity; p.dy_min = -options.maxDy; p.dy_max = options.maxDy;
        match(left, current->second, 0);
    }
    if (previous) {
        p.dx_min = p.dy_min = -options.searchRadius; p.dx_max = p.dy_max = options.searchRadius;
        match(left, previous->first, 1);
    }
    hipCheck(hipMemcpyAsync(sl.host(), records.data, pool->bytes(n), hipMemcpyDeviceToHost, stream.s), "hipMemcpyAsync of the matches");
    stream.wait();   // the frame's only blocking synchronisation
    const int32_t *counts = sl.host<int32_t>();
    const FeatureMatch *host = reinterpret_cast<const FeatureMatch *>(sl.host<uint8_t>() + 16);
    auto result = std::make_shared<FeatureMatches>();
    result->records = records;
    result->capacity = n;
    std::vector<FeatureMatch> *lists[2] = {&result->stereo, &result->temporal};
    for (int i = 0; i < 2; ++i) {
        if (counts[i] < 0 || counts[i] > n) throw std::runtime_error("cart_matcher_match: match count out of range");
        lists[i]->assign(host + (size_t)i * n, host + (size_t)i * n + counts[i]);
    }
    return MODULE_RETURN(CARTSLAM_KEY_FEATURE_MATCHES, result);
}
}  // namespace cart

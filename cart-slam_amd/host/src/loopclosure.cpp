// loopclosure.cpp -- LoopClosureModule (cartslam_amd/modules/loopclosure.hpp): place recognition and loop verification, spec DESIGN.md S27.
#include "cartslam_amd/modules/loopclosure.hpp"

#include <cmath>
#include <cstring>

#include "cartslam_amd/modules/denseego.hpp"
#include "cartslam_amd/modules/features.hpp"
#include "module_support.hpp"

namespace cart {
namespace {
cart_place_params placeParamsOf(const LoopClosureOptions &o) { return cart_place_params{o.maxDistance, o.ratio, o.minScore, o.maxCandidates, o.minGap}; }

// the module's device buffer: candidates [16] | n_candidates, match_count | cart_ego_result | matches [features]
constexpr size_t kCountsAt = CART_PLACE_MAX_CANDIDATES * sizeof(cart_place_candidate), kResultAt = kCountsAt + 16, kMatchesAt = kResultAt + 128;
static_assert(sizeof(cart_ego_result) <= 128, "cart_ego_result layout");
}  // namespace

LoopClosureModule::LoopClosureModule(const LoopClosureOptions &options) : SyncWrapperSystemModule("LoopClosure"), options(options) {
    checkCamera(options);
    // the library's own checks, without a device: everything valid gets as far as the missing object
    const cart_place_params p = placeParamsOf(options);
    (void)cart_place_query(nullptr, &p, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    requireLibraryAccepts();
    cart_place_db *none = nullptr;
    (void)cart_place_create(nullptr, 1, options.capacity, &none);
    requireLibraryAccepts();
    if (options.keyframeInterval < 1) throw std::invalid_argument("keyframe_interval must be at least 1");
    if (options.verify < 0 || options.verify > CART_PLACE_MAX_CANDIDATES) throw std::invalid_argument("verify must be in [0, 16]");
    if (options.minInliers < 0) throw std::invalid_argument("min_inliers must not be negative");
    if (!positiveNumber(options.minDisparity)) throw std::invalid_argument("min_disparity must be a positive number");
    if (!positiveNumber(options.inlierThreshold)) throw std::invalid_argument("inlier_threshold must be a positive number");
    if (options.hypotheses < 1 || options.hypotheses > CART_EGO_MAX_HYPOTHESES) throw std::invalid_argument("hypotheses must be in [1, 1024]");
    if (options.refineIterations < 0 || options.refineIterations > CART_EGO_MAX_REFINE) throw std::invalid_argument("refine_iterations must be in [0, 16]");
    if (options.poseKey != CARTSLAM_KEY_EGO_MOTION && options.poseKey != CARTSLAM_KEY_DENSE_EGO)
        throw std::invalid_argument("pose_key must be \"ego_motion\" or \"dense_ego\"");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_FEATURES));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_EGO_MOTION));
    if (options.poseKey != CARTSLAM_KEY_EGO_MOTION) this->requiresData.push_back(module_dependency_t(options.poseKey));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_LOOP_CLOSURE, -1));   // frames pass in order: the ring is filled in frame order
    this->providesData.push_back(CARTSLAM_KEY_LOOP_CLOSURE);
    keyframes.resize(options.capacity);
}

LoopClosureModule::~LoopClosureModule() {
    cart_place_destroy(db);
    cart_matcher_destroy(matcher);
    cart_ego_destroy(ego);
}

system_data_t LoopClosureModule::runInternal(System &, SystemRunData &data) {
    typedef std::pair<ImageFeatures, ImageFeatures> features_t;
    auto result = std::make_shared<LoopClosure>();
    std::memset(result.get(), 0, sizeof(*result));
    if (data.id % (uint32_t)options.keyframeInterval == 0) {
        auto features = data.getData<features_t>(CARTSLAM_KEY_FEATURES);
        auto landmarks = data.getData<EgoMotion>(CARTSLAM_KEY_EGO_MOTION);
        auto pose = data.getData<EgoMotion>(options.poseKey);
        const ImageFeatures &left = features->first;
        if (!left.onDevice()) throw std::runtime_error("LoopClosureModule requires features that are still on the device");
        const int n = left.deviceCapacity();
        if (landmarks->landmarks.empty() || (size_t)landmarks->landmarks.cols != (size_t)n * 4 * sizeof(double))
            throw std::runtime_error("LoopClosureModule: ego_motion's landmarks are missing or of another capacity than the features");
        std::lock_guard<std::mutex> lock(mutex);
        if (!db) {   // the objects keep the device of the engine they are made on, not the engine
            makeOnPostEngine(64, 32, [&](cart_engine *e) -> const char * {
                if (cart_place_create(e, n, options.capacity, &db) != 0) return "cart_place_create";
                if (cart_matcher_create(e, n, &matcher) != 0) return "cart_matcher_create";
                if (cart_ego_create(e, n, &ego) != 0) return "cart_ego_create";
                return nullptr;
            });
            featureCapacity = n;
            scratch.create();
            scratch.reserve(kMatchesAt + (size_t)n * sizeof(cart_match), kMatchesAt);
        }
        if (n != featureCapacity) throw std::runtime_error("LoopClosureModule: the feature capacity changed between frames");
        hipStream_t s = scratch.stream();
        uint8_t *d = scratch.dev<uint8_t>();
        const uint8_t *h = scratch.host<uint8_t>();
        cart_place_candidate *candidatesDev = reinterpret_cast<cart_place_candidate *>(d);
        int32_t *countsDev = reinterpret_cast<int32_t *>(d + kCountsAt);
        cart_ego_result *resultDev = reinterpret_cast<cart_ego_result *>(d + kResultAt);
        cart_match *matchesDev = reinterpret_cast<cart_match *>(d + kMatchesAt);
        const cart_place_params p = placeParamsOf(options);
        // 1. the query, 2. the candidate list through the pinned buffer
        if (cart_place_query(db, &p, left.descriptors.ptr<uint8_t>(), left.descriptors.step, left.deviceCount(), data.id, nullptr, candidatesDev, countsDev, s) != 0)
            failAbi("cart_place_query");
        hipCheck(hipMemcpyAsync(scratch.host(), d, kResultAt, hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the candidates");
        scratch.wait();
        const int found = *reinterpret_cast<const int32_t *>(h + kCountsAt);
        if (found < 0 || found > options.maxCandidates) throw std::runtime_error("cart_place_query: candidate count out of range");
        std::vector<cart_place_candidate> candidates(reinterpret_cast<const cart_place_candidate *>(h), reinterpret_cast<const cart_place_candidate *>(h) + found);
        // 3. verification: a cross-checked match against the stored frame, then the relative pose between the two frames' landmarks
        const cart_ego_camera cam = cameraOf(options);
        const cart_ego_params ep{options.minDisparity, options.inlierThreshold, options.hypotheses, options.refineIterations};
        cart_match_params mp;
        cart_match_default_params(&mp);
        mp.use_gate = 0; mp.max_distance = options.maxDistance; mp.ratio = options.ratio; mp.cross_check = 1;
        for (int c = 0; c < found && c < options.verify; ++c) {
            const cart_place_candidate &cand = candidates[c];
            if (cand.slot < 0 || cand.slot >= options.capacity) throw std::runtime_error("cart_place_query: candidate slot out of range");
            const uint8_t *slotDesc = nullptr;
            const cart_keypoint *slotKp = nullptr;
            const double *slotLandmarks = nullptr;
            const int32_t *slotCount = nullptr;
            if (cart_place_slot(db, cand.slot, &slotDesc, &slotKp, &slotLandmarks, &slotCount) != 0) failAbi("cart_place_slot");
            if (!slotLandmarks) throw std::runtime_error("LoopClosureModule: a stored keyframe has no landmarks");
            if (cart_matcher_match(matcher, &mp, left.descriptors.ptr<uint8_t>(), left.descriptors.step, left.deviceKeypoints(), left.deviceCount(), slotDesc,
                                   CART_ORB_DESCRIPTOR_BYTES, slotKp, slotCount, matchesDev, countsDev + 1, nullptr, s) != 0)
                failAbi("cart_matcher_match");
            if (cart_ego_estimate(ego, &cam, &ep, landmarks->landmarks.ptr<double>(), left.deviceKeypoints(), slotLandmarks, matchesDev, countsDev + 1, options.seed,
                                  data.id, resultDev, nullptr, s) != 0)
                failAbi("cart_ego_estimate");
            hipCheck(hipMemcpyAsync(scratch.host<uint8_t>() + kResultAt, resultDev, sizeof(cart_ego_result), hipMemcpyDeviceToHost, s),
                     "hipMemcpyAsync of the loop's relative pose");
            scratch.wait();
            cart_ego_result rel;
            std::memcpy(&rel, h + kResultAt, sizeof(rel));
            if (rel.status == 1 && rel.n_inliers >= options.minInliers) {
                const Keyframe &kf = keyframes[cand.slot];
                result->detected = 1;
                result->slot = cand.slot;
                result->score = cand.score;
                result->keyframeId = cand.frame_id;
                result->relative = rel;
                std::memcpy(result->poseKeyframe, kf.pose, sizeof(kf.pose));
                chainPose(kf.pose, rel, result->poseLoop);
                break;
            }
        }
        // 4. the frame itself, after the query: a frame never finds itself
        int32_t slot = -1;
        if (cart_place_insert(db, left.descriptors.ptr<uint8_t>(), left.descriptors.step, left.deviceKeypoints(), landmarks->landmarks.ptr<double>(), left.deviceCount(),
                              data.id, &slot, s) != 0)
            failAbi("cart_place_insert");
        scratch.wait();   // the frame's buffers may be released once the module returns
        keyframes[slot].id = data.id;
        std::memcpy(keyframes[slot].pose, pose->pose, sizeof(pose->pose));
    }
    return MODULE_RETURN(CARTSLAM_KEY_LOOP_CLOSURE, result);
}
}  // namespace cart

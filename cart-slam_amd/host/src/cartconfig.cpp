// cartconfig.cpp -- module / data-source factory. Type strings, keys and defaults are the reference's
// (src/cartconfig.cpp:56-80, :82-104, :144-152, :161-163, :198-206); GUI module types ("*_visualization") are
// accepted and skipped so that the reference's config files load unchanged; module types outside the hot path throw
// the reference's "Unknown module type" error.
#include "cartslam_amd/cartconfig.hpp"

#include <cmath>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "cartslam_amd/json.hpp"
#include "cartslam_amd/modules/depth.hpp"
#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/features.hpp"
#include "cartslam_amd/modules/matches.hpp"
#include "cartslam_amd/modules/denseego.hpp"
#include "cartslam_amd/modules/fusion.hpp"
#include "cartslam_amd/modules/objects.hpp"
#include "cartslam_amd/modules/loopclosure.hpp"
#include "cartslam_amd/modules/motionseg.hpp"
#include "cartslam_amd/modules/planefit.hpp"
#include "cartslam_amd/modules/planemap.hpp"
#include "cartslam_amd/modules/planeseg.hpp"
#include "cartslam_amd/modules/localba.hpp"
#include "cartslam_amd/modules/posegraph.hpp"
#include "cartslam_amd/modules/superpixels.hpp"
#include "cartslam_amd/modules/voxelmap.hpp"

#define CART_CONFIG_KEY_DATA_SOURCE "data_source"
#define CART_CONFIG_KEY_MODULES "modules"

namespace cart::config {
namespace {
using json::Value;

template <typename T>
T get(const Value &data, const std::string &key, const T &defaultValue) {
    if (!data.contains(key)) return defaultValue;
    return data.at(key).get<T>();
}
template <typename T>
T get(const Value &data, const std::string &key) { return data.at(key).get<T>(); }  // throws "Key <k> not found."

std::string slurp(const std::string &path) {
    std::string p = path;
    if (!p.empty() && p[0] == '~') if (const char *home = std::getenv("HOME")) p = std::string(home) + p.substr(1);
    std::ifstream file(p);
    if (!file.is_open()) throw std::runtime_error("Could not open file " + path + ": " + std::strerror(errno));
    std::stringstream ss;
    ss << file.rdbuf();
    return ss.str();
}

std::shared_ptr<PlaneParameterProvider> readParameterProvider(const Value &data) {
    if (!data.contains("type")) throw std::runtime_error("Parameter provider type not found.");
    const std::string providerType = data.at("type").get<std::string>();
    if (providerType == "static") {
        auto horizontalRange = std::make_pair(get<int>(data, "horizontal_range_min"), get<int>(data, "horizontal_range_max"));
        auto verticalRange = std::make_pair(get<int>(data, "vertical_range_min"), get<int>(data, "vertical_range_max"));
        const int horizontalCenter = (horizontalRange.first + horizontalRange.second) / 2;
        const int verticalCenter = (verticalRange.first + verticalRange.second) / 2;
        return std::make_shared<StaticPlaneParameterProvider>(horizontalCenter, verticalCenter, horizontalRange, verticalRange);
    }
    if (providerType == "histogram_peak") return std::make_shared<HistogramPeakPlaneParameterProvider>();
    throw std::runtime_error("Unknown parameter provider type.");
}

std::shared_ptr<DataSource> createDataSource(const Value &cfg) {
    if (!cfg.is_object()) throw std::runtime_error("Data source configuration is not an object.");
    const std::string sourcePath = cfg.at("path").get<std::string>();
    const std::string type = cfg.at("type").get<std::string>();
    // image_width / image_height are an extension: the reference's factory (cartconfig.cpp:95-98) never passes its ctor's imageSize
    if (type == "kitti")
        return std::make_shared<sources::KITTIDataSource>(sourcePath, get(cfg, "sequence", 0), Size{get(cfg, "image_width", 0), get(cfg, "image_height", 0)});
    if (type == "zed") throw std::runtime_error("Data source type zed needs the proprietary ZED SDK: not supported.");
    throw std::runtime_error("Unknown data source type.");
}

// The camera of a module: the configuration's keys, else Q as the source builds it (an uncalibrated source has fx = 0)
void readCamera(const Value &moduleConfig, const DataSource &dataSource, CameraOptions &o) {
    const CameraIntrinsics K = dataSource.getCameraIntrinsics();
    o.fx = get(moduleConfig, "fx", (double)K.Q[11]);
    o.fy = get(moduleConfig, "fy", (double)K.Q[11]);
    o.cx = get(moduleConfig, "cx", -(double)K.Q[3]);
    o.cy = get(moduleConfig, "cy", -(double)K.Q[7]);
    o.baseline = get(moduleConfig, "baseline", K.Q[14] != 0 ? std::fabs(1.0 / (double)K.Q[14]) : 0.0);
}

bool endsWith(const std::string &s, const std::string &suffix) { return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0; }

void applyModuleConfig(const Value &modulesConfig, std::shared_ptr<System> system) {
    if (!modulesConfig.is_array()) throw std::runtime_error("Modules configuration is not an array.");
    auto dataSource = system->getDataSource();
    int loopKeyframeInterval = 0;   // of the loop_closure module, once one is configured: pose_graph must use the same keyframes
    for (const auto &moduleConfig : modulesConfig.arr) {
        if (!moduleConfig.is_object()) throw std::runtime_error("Module configuration is not an object.");
        const std::string moduleType = moduleConfig.at("type").get<std::string>();
        if (moduleType == "disparity") {
            system->addModule<ImageDisparityModule>(dataSource->getImageSize(), get(moduleConfig, "min_disparity", 4), get(moduleConfig, "num_disparities", 256),
                                                    get(moduleConfig, "block_size", 3), get(moduleConfig, "smoothing_radius", -1),
                                                    get(moduleConfig, "smoothing_iterations", 5),
                                                    // extensions (not in the reference's JSON): OpenCV's createStereoSGM knobs
                                                    get(moduleConfig, "paths", 4), get(moduleConfig, "p1", 10), get(moduleConfig, "p2", 120),
                                                    get(moduleConfig, "uniqueness_ratio", 12));
        } else if (moduleType == "depth") {  // cartconfig.cpp:138-140
            system->addModule<DepthModule>();
        } else if (moduleType == "disparity_derivative") {
            system->addModule<ImageDisparityDerivativeModule>();
        } else if (moduleType == "disparity_planeseg") {
            const auto parameterProvider = readParameterProvider(moduleConfig.at("parameter_provider"));
            system->addModule<DisparityPlaneSegmentationModule>(parameterProvider, get(moduleConfig, "update_interval", 30), get(moduleConfig, "reset_interval", 10),
                                                                get(moduleConfig, "use_temporal_smoothing", false),
                                                                (unsigned)get(moduleConfig, "temporal_smoothing_distance", CARTSLAM_PLANE_TEMPORAL_DISTANCE_DEFAULT),
                                                                get(moduleConfig, "label_components", false));
        } else if (moduleType == "superpixels") {  // cartconfig.cpp:121-134
            const double direct = get(moduleConfig, "direct_clique_cost", 0.5);
            system->addModule<SuperPixelModule>(dataSource->getImageSize(), (unsigned)get(moduleConfig, "initial_iterations", 18), (unsigned)get(moduleConfig, "iterations", 6),
                                                (unsigned)get(moduleConfig, "block_size", 12), (unsigned)get(moduleConfig, "reset_iterations", 64), direct,
                                                get(moduleConfig, "diagonal_clique_cost", direct / std::sqrt(2.0)), get(moduleConfig, "compactness_weight", 0.1),
                                                get(moduleConfig, "progressive_compactness_cost", 0.0), get(moduleConfig, "image_weight", 1.5),
                                                get(moduleConfig, "disparity_weight", 1.0));
        } else if (moduleType == "superpixel_disparity_planeseg") {  // cartconfig.cpp:212-220
            const auto parameterProvider = readParameterProvider(moduleConfig.at("parameter_provider"));
            system->addModule<SuperPixelDisparityPlaneSegmentationModule>(parameterProvider, get(moduleConfig, "update_interval", 30), get(moduleConfig, "reset_interval", 10),
                                                                          get(moduleConfig, "use_temporal_smoothing", false),
                                                                          (unsigned)get(moduleConfig, "temporal_smoothing_distance", CARTSLAM_PLANE_TEMPORAL_DISTANCE_DEFAULT));
        } else if (moduleType == "optflow_file") {  // extension: replays flow fields from <sequence>/flow/%06d.bin
            system->addModule<OpticalFlowFileModule>();
        } else if (moduleType == "optflow") {  // cartconfig.cpp:183-185; every key is an extension.  pyramid_levels > 1: coarse-to-fine (spec S21)
            const int pyramidLevels = get(moduleConfig, "pyramid_levels", 1);
            system->addModule<ImageOpticalFlowModule>(dataSource->getImageSize(), get(moduleConfig, "search_radius", 8), get(moduleConfig, "block_radius", 2),
                                                      pyramidLevels, get(moduleConfig, "refine_radius", 2), get(moduleConfig, "median", pyramidLevels > 1));
        } else if (moduleType == "planefit") {  // extension key "seed" (default 0): the reference seeds from std::random_device
            system->addModule<SuperPixelPlaneFitModule>((uint64_t)get(moduleConfig, "seed", 0));
        } else if (moduleType == "planecluster") {
            system->addModule<SuperPixelPlaneClusterModule>((uint64_t)get(moduleConfig, "seed", 0));
        } else if (moduleType == "orb_features") {
            // the reference's "features" (cartconfig.cpp:167-179) under an extension name: tests/test_host.py uses "features" as
            // its example of an unknown module type, so renaming this to "features" is a follow-up together with that test.
            // "nfeatures" is an extension (the reference's is fixed at CARTSLAM_OPTION_KEYPOINTS).
            const std::string featureType = get<std::string>(moduleConfig, "feature_type", "orb");
            if (featureType != "orb") throw std::runtime_error("Unknown feature type.");
            system->addModule<ImageFeatureDetectorModule>(get(moduleConfig, "nfeatures", CARTSLAM_OPTION_KEYPOINTS));
        } else if (moduleType == "orb_matches") {  // extension (spec S22): stereo and temporal matches of the orb_features module's output
            FeatureMatcherOptions o;
            o.stereo = get(moduleConfig, "stereo", o.stereo);
            o.temporal = get(moduleConfig, "temporal", o.temporal);
            o.maxDistance = get(moduleConfig, "max_distance", o.maxDistance);
            o.ratio = get(moduleConfig, "ratio", o.ratio);
            o.crossCheck = get(moduleConfig, "cross_check", o.crossCheck);
            o.maxDisparity = (float)get(moduleConfig, "max_disparity", (double)o.maxDisparity);
            o.maxDy = (float)get(moduleConfig, "max_dy", (double)o.maxDy);
            o.searchRadius = (float)get(moduleConfig, "search_radius", (double)o.searchRadius);
            system->addModule<FeatureMatcherModule>(o);
        } else if (moduleType == "ego_motion") {  // extension (spec S23): frame-to-frame pose from the orb_matches module's output
            EgoMotionOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.inlierThreshold = get(moduleConfig, "inlier_threshold", o.inlierThreshold);
            o.hypotheses = get(moduleConfig, "hypotheses", o.hypotheses);
            o.refineIterations = get(moduleConfig, "refine_iterations", o.refineIterations);
            o.seed = (uint64_t)get(moduleConfig, "seed", 0);
            system->addModule<EgoMotionModule>(o);
        } else if (moduleType == "plane_map") {  // extension (spec S24): disparity + planes voted into a world-frame grid through the frame's pose
            PlaneMapOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.cellsX = get(moduleConfig, "cells_x", o.cellsX);
            o.cellsZ = get(moduleConfig, "cells_z", o.cellsZ);
            o.cellSize = get(moduleConfig, "cell_size", o.cellSize);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.maxDepth = get(moduleConfig, "max_depth", o.maxDepth);
            o.maxLateral = get(moduleConfig, "max_lateral", o.maxLateral);
            o.heightQuantum = get(moduleConfig, "height_quantum", o.heightQuantum);
            o.minVotes = get(moduleConfig, "min_votes", o.minVotes);
            o.obstaclePercent = get(moduleConfig, "obstacle_percent", o.obstaclePercent);
            o.poseFile = get<std::string>(moduleConfig, "pose_file", "");   // absent: the pose of the ego_motion module
            o.planesKey = get<std::string>(moduleConfig, "planes_key", o.planesKey);   // "planes_static": the static world only (motion_seg)
            o.poseKey = get<std::string>(moduleConfig, "pose_key", o.poseKey);         // "dense_ego": the refined trajectory
            o.disparityKey = get<std::string>(moduleConfig, "disparity_key", o.disparityKey);   // "disparity_fused": the temporally fused image (temporal_fusion)
            o.rebuild = get(moduleConfig, "rebuild", o.rebuild);   // S30: rebuild the grid from the stored keyframes when pose_graph optimised
            o.storeCapacity = get(moduleConfig, "store_capacity", o.storeCapacity);
            system->addModule<PlaneMapModule>(o);
        } else if (moduleType == "motion_seg") {  // extension (spec S25): which pixels moved on their own, from disparity, optflow and ego_motion
            MotionSegOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.flowThreshold = get(moduleConfig, "flow_threshold", o.flowThreshold);
            o.disparityThreshold = get(moduleConfig, "disparity_threshold", o.disparityThreshold);
            o.radius = get(moduleConfig, "radius", o.radius);
            o.supportPercent = get(moduleConfig, "support_percent", o.supportPercent);
            o.planes = get(moduleConfig, "planes", o.planes);
            o.components = get(moduleConfig, "components", o.components);
            system->addModule<MotionSegModule>(o);
        } else if (moduleType == "dense_ego") {  // extension (spec S26): ego_motion's relative pose refined over every static pixel
            DenseEgoOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.flowThreshold = get(moduleConfig, "flow_threshold", o.flowThreshold);
            o.disparityThreshold = get(moduleConfig, "disparity_threshold", o.disparityThreshold);
            o.disparityWeight = get(moduleConfig, "disparity_weight", o.disparityWeight);
            o.iterations = get(moduleConfig, "iterations", o.iterations);
            o.stride = get(moduleConfig, "stride", o.stride);
            o.minInliers = get(moduleConfig, "min_inliers", o.minInliers);
            o.useMotion = get(moduleConfig, "use_motion", o.useMotion);
            system->addModule<DenseEgoModule>(o);
        } else if (moduleType == "temporal_fusion") {  // extension (spec S28): the previous fused disparity carried through the pose and fused with this frame's
            TemporalFusionOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.agreeThreshold = get(moduleConfig, "agree_threshold", o.agreeThreshold);
            o.splatRadius = get(moduleConfig, "splat_radius", o.splatRadius);
            o.maxWeight = get(moduleConfig, "max_weight", o.maxWeight);
            o.minAge = get(moduleConfig, "min_age", o.minAge);
            o.useMotion = get(moduleConfig, "use_motion", o.useMotion);
            o.poseKey = get<std::string>(moduleConfig, "pose_key", o.poseKey);   // "dense_ego": the refined relative pose
            system->addModule<TemporalFusionModule>(o);
        } else if (moduleType == "moving_objects") {  // extension (spec S31): motion_seg's MOVING components as objects in metres and their tracks
            MovingObjectsOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.disparityBand = get(moduleConfig, "disparity_band", o.disparityBand);
            o.maxSpeed = get(moduleConfig, "max_speed", o.maxSpeed);
            o.gate = get(moduleConfig, "gate", o.gate);
            o.minArea = get(moduleConfig, "min_area", o.minArea);
            o.minPoints = get(moduleConfig, "min_points", o.minPoints);
            o.gainPercent = get(moduleConfig, "gain_percent", o.gainPercent);
            o.maxMissed = get(moduleConfig, "max_missed", o.maxMissed);
            o.minAge = get(moduleConfig, "min_age", o.minAge);
            o.maxObjects = get(moduleConfig, "max_objects", o.maxObjects);
            o.maxTracks = get(moduleConfig, "max_tracks", o.maxTracks);
            o.poseKey = get<std::string>(moduleConfig, "pose_key", o.poseKey);   // "dense_ego": the refined poses; "pose_graph" is refused
            system->addModule<MovingObjectsModule>(o);
        } else if (moduleType == "loop_closure") {  // extension (spec S27): keyframes recognised in a device-resident ring and verified by a relative pose
            LoopClosureOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.maxDistance = get(moduleConfig, "max_distance", o.maxDistance);
            o.ratio = get(moduleConfig, "ratio", o.ratio);
            o.minScore = get(moduleConfig, "min_score", o.minScore);
            o.maxCandidates = get(moduleConfig, "max_candidates", o.maxCandidates);
            o.minGap = (uint64_t)get(moduleConfig, "min_gap", (int)o.minGap);
            o.capacity = get(moduleConfig, "capacity", o.capacity);
            o.keyframeInterval = get(moduleConfig, "keyframe_interval", o.keyframeInterval);
            o.verify = get(moduleConfig, "verify", o.verify);
            o.minInliers = get(moduleConfig, "min_inliers", o.minInliers);
            o.seed = (uint64_t)get(moduleConfig, "seed", 0);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.inlierThreshold = get(moduleConfig, "inlier_threshold", o.inlierThreshold);
            o.hypotheses = get(moduleConfig, "hypotheses", o.hypotheses);
            o.refineIterations = get(moduleConfig, "refine_iterations", o.refineIterations);
            o.poseKey = get<std::string>(moduleConfig, "pose_key", o.poseKey);   // "dense_ego": keyframes are stored with the refined pose
            system->addModule<LoopClosureModule>(o);
            loopKeyframeInterval = o.keyframeInterval;
        } else if (moduleType == "pose_graph") {  // extension (spec S29): loop_closure's keyframes as a pose graph, optimised when a loop is accepted
            PoseGraphOptions o;
            o.keyframeInterval = get(moduleConfig, "keyframe_interval", o.keyframeInterval);
            o.loopClosureInterval = loopKeyframeInterval;
            o.maxNodes = get(moduleConfig, "max_nodes", o.maxNodes);
            o.maxLoops = get(moduleConfig, "max_loops", o.maxLoops);
            o.iterations = get(moduleConfig, "iterations", o.iterations);
            o.weightRotation = get(moduleConfig, "weight_rotation", o.weightRotation);
            o.weightTranslation = get(moduleConfig, "weight_translation", o.weightTranslation);
            o.loopWeight = get(moduleConfig, "loop_weight", o.loopWeight);
            o.poseKey = get<std::string>(moduleConfig, "pose_key", o.poseKey);   // "dense_ego": the refined trajectory is the odometry
            system->addModule<PoseGraphModule>(o);
        } else if (moduleType == "local_ba") {  // extension (spec S32): feature tracks over the last frames and a windowed bundle adjustment of their poses
            LocalBAOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.huber = get(moduleConfig, "huber", o.huber);
            o.damping = get(moduleConfig, "damping", o.damping);
            o.iterations = get(moduleConfig, "iterations", o.iterations);
            o.minObservations = get(moduleConfig, "min_observations", o.minObservations);
            o.minFrameObservations = get(moduleConfig, "min_frame_observations", o.minFrameObservations);
            o.window = get(moduleConfig, "window", o.window);
            o.maxPoints = get(moduleConfig, "max_points", o.maxPoints);
            o.interval = get(moduleConfig, "interval", o.interval);
            o.poseKey = get<std::string>(moduleConfig, "pose_key", o.poseKey);   // "dense_ego": the refined trajectory is the odometry
            system->addModule<LocalBAModule>(o);
        } else if (moduleType == "voxel_map") {  // extension (spec S33): disparity averaged into a rolling TSDF volume through the frame's pose, and its raycast
            VoxelMapOptions o;
            readCamera(moduleConfig, *dataSource, o);
            o.cellsX = get(moduleConfig, "cells_x", o.cellsX);
            o.cellsY = get(moduleConfig, "cells_y", o.cellsY);
            o.cellsZ = get(moduleConfig, "cells_z", o.cellsZ);
            o.voxelSize = get(moduleConfig, "voxel_size", o.voxelSize);
            o.minDisparity = get(moduleConfig, "min_disparity", o.minDisparity);
            o.minDepth = get(moduleConfig, "min_depth", o.minDepth);
            o.maxDepth = get(moduleConfig, "max_depth", o.maxDepth);
            o.truncation = get(moduleConfig, "truncation", o.truncation);
            o.disparitySigma = get(moduleConfig, "disparity_sigma", o.disparitySigma);
            o.lookahead = get(moduleConfig, "lookahead", o.lookahead);
            o.marchStep = get(moduleConfig, "march_step", o.marchStep);
            o.maxWeight = get(moduleConfig, "max_weight", o.maxWeight);
            o.minWeight = get(moduleConfig, "min_weight", o.minWeight);
            o.disparityKey = get<std::string>(moduleConfig, "disparity_key", o.disparityKey);   // "disparity_fused": the temporally fused image (temporal_fusion)
            o.poseKey = get<std::string>(moduleConfig, "pose_key", o.poseKey);                 // "dense_ego", "local_ba", "pose_graph": the refined trajectory
            o.useMotion = get(moduleConfig, "use_motion", o.useMotion);
            o.raycast = get(moduleConfig, "raycast", o.raycast);
            o.track = get(moduleConfig, "track", o.track);   // S34: the pose refined against the volume, published as "model_pose"
            o.rebuild = get(moduleConfig, "rebuild", o.rebuild);   // S35: the volume rebuilt from stored keyframes when the pose graph was optimised
            o.storeCapacity = get(moduleConfig, "store_capacity", o.storeCapacity);
            o.mesh = get(moduleConfig, "mesh", o.mesh);   // S36: the window's surface as a quad mesh, published as "voxel_mesh" every mesh_interval-th frame
            o.meshInterval = get(moduleConfig, "mesh_interval", o.meshInterval);
            o.meshMaxVertices = get(moduleConfig, "mesh_max_vertices", o.meshMaxVertices);
            o.meshMaxQuads = get(moduleConfig, "mesh_max_quads", o.meshMaxQuads);
            o.meshMinWeight = get(moduleConfig, "mesh_min_weight", o.meshMinWeight);
            o.color = get(moduleConfig, "color", o.color);   // S37: a colour volume beside the map; "image_model" with "raycast", "voxel_mesh_colors" with "mesh"
            o.colorMaxWeight = get(moduleConfig, "color_max_weight", o.colorMaxWeight);
            o.residualGate = get(moduleConfig, "residual_gate", o.residualGate);
            o.damping = get(moduleConfig, "damping", o.damping);
            o.iterations = get(moduleConfig, "iterations", o.iterations);
            o.stride = get(moduleConfig, "stride", o.stride);
            o.minInliers = get(moduleConfig, "min_inliers", o.minInliers);
            o.trackColor = get(moduleConfig, "track_color", o.trackColor);   // S38: "track" with a photometric term against the colour volume; needs "track" and "color"
            o.photoWeight = get(moduleConfig, "photo_weight", o.photoWeight);
            o.photoGate = get(moduleConfig, "photo_gate", o.photoGate);
            o.colorMinWeight = get(moduleConfig, "color_min_weight", o.colorMinWeight);
            system->addModule<VoxelMapModule>(o);
        } else if (endsWith(moduleType, "_visualization")) {
            std::cerr << "[cartconfig] skipping GUI module type " << moduleType << " (out of scope)\n";
        } else {
            throw std::runtime_error("Unknown module type " + moduleType + ".");
        }
    }
}
}  // namespace

std::shared_ptr<DataSource> readDataSourceConfig(const std::string path) { return createDataSource(json::parse(slurp(path))); }

void readModuleConfig(const std::string path, std::shared_ptr<System> system) { applyModuleConfig(json::parse(slurp(path)), system); }

void applyModuleConfigText(const std::string &text, std::shared_ptr<System> system) { applyModuleConfig(json::parse(text), system); }

std::shared_ptr<System> readSystemConfig(const std::string path) {
    const Value data = json::parse(slurp(path));
    if (!data.contains(CART_CONFIG_KEY_DATA_SOURCE)) throw std::runtime_error("Data source not found in configuration file.");
    if (!data.contains(CART_CONFIG_KEY_MODULES)) throw std::runtime_error("Modules not found in configuration file.");
    auto system = std::make_shared<System>(createDataSource(data.at(CART_CONFIG_KEY_DATA_SOURCE)));
    applyModuleConfig(data.at(CART_CONFIG_KEY_MODULES), system);
    return system;
}
}  // namespace cart::config

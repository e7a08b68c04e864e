// objects.cpp -- MovingObjectsModule (cartslam_amd/modules/objects.hpp): moving-object tracks from the motion components, spec DESIGN.md S31.
#include "cartslam_amd/modules/objects.hpp"

#include <cmath>
#include <cstring>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/motionseg.hpp"
#include "cartslam_amd/modules/planeseg.hpp"
#include "module_support.hpp"

namespace cart {
namespace {
cart_object_params paramsOf(const MovingObjectsOptions &o) {
    return cart_object_params{o.minDisparity, o.disparityBand, o.maxSpeed, o.gate, o.minArea, o.minPoints, o.gainPercent, o.maxMissed, o.minAge};
}
// the download: the counts, then every object record, then every track slot
size_t objectsAt() { return 8 * sizeof(int32_t); }
size_t tracksAt(const MovingObjectsOptions &o) { return objectsAt() + (size_t)o.maxObjects * sizeof(cart_object); }
size_t downloadBytes(const MovingObjectsOptions &o) { return tracksAt(o) + (size_t)o.maxTracks * sizeof(cart_track); }
}  // namespace

MovingObjectsModule::MovingObjectsModule(const MovingObjectsOptions &options) : SyncWrapperSystemModule("MovingObjects"), options(options) {
    checkCamera(options);
    // the library's own checks, without a device: everything valid gets as far as the missing object
    const cart_ego_camera cam = cameraOf(options);
    const cart_object_params p = paramsOf(options);
    (void)cart_object_tracker_update(nullptr, &cam, kIdentityPose, kIdentityPose, &p, nullptr, 0, nullptr, 1, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, 1, 1, nullptr,
                                     nullptr, nullptr, nullptr);
    requireLibraryAccepts();
    cart_object_tracker *none = nullptr;
    (void)cart_object_tracker_create(nullptr, 1, 1, options.maxObjects, options.maxTracks, &none);
    requireLibraryAccepts();
    if (options.poseKey.empty()) throw std::invalid_argument("pose_key must name a blackboard pose");
    if (options.poseKey == "pose_graph")
        throw std::invalid_argument("pose_key must not be pose_graph: a loop correction would move every world-frame track at once, which the tracker does not follow");
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION_COMPONENTS));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION_COMPONENT_TABLE));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOTION_COMPONENT_COUNT));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY, -1));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_OPTFLOW));
    this->requiresData.push_back(module_dependency_t(options.poseKey));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_MOVING_OBJECTS, -1));   // one frame at a time, in order
    this->providesData.push_back(CARTSLAM_KEY_MOVING_OBJECTS);
}

MovingObjectsModule::~MovingObjectsModule() { cart_object_tracker_destroy(object); }

system_data_t MovingObjectsModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(CARTSLAM_KEY_DISPARITY);
    if (disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    const int rows = disparity->rows, cols = disparity->cols;
    auto ego = data.getData<EgoMotion>(options.poseKey);
    // Frame 1 has no predecessor, and a frame without an estimate keeps the previous pose: neither can place an object, so the tracks are dropped.
    const bool estimate = data.id > 1 && ego->result.status != 0;
    auto out = std::make_shared<MovingObjects>();
    std::lock_guard<std::mutex> lock(mutex);
    if (!object) {   // the object keeps the device of the engine it is made on, not the engine
        makeOnPostEngine(cols, rows, [&](cart_engine *e) {
            return cart_object_tracker_create(e, cols, rows, options.maxObjects, options.maxTracks, &object) ? "cart_object_tracker_create" : nullptr;
        });
        scratch.create();
        scratch.reserve(downloadBytes(options), downloadBytes(options));
    }
    hipStream_t s = scratch.stream();
    if (!estimate) {
        if (cart_object_tracker_reset(object, s) != 0) failAbi("cart_object_tracker_reset");
        scratch.wait();
        return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_MOVING_OBJECTS, out));
    }
    auto ids = data.getData<image_t>(CARTSLAM_KEY_MOTION_COMPONENTS);
    auto table = data.getData<image_t>(CARTSLAM_KEY_MOTION_COMPONENT_TABLE);
    auto count = data.getData<image_t>(CARTSLAM_KEY_MOTION_COMPONENT_COUNT);
    auto previous = data.getRelativeRun(-1)->getData<image_t>(CARTSLAM_KEY_DISPARITY);
    auto flow = data.getData<image_t>(CARTSLAM_KEY_OPTFLOW);
    requireImage(ids, CV_32SC1, rows, cols, "MovingObjectsModule: motion_components must be a CV_32SC1 image of the disparity's size");
    requireImage(table, CV_32SC1, 1, CARTSLAM_PLANE_COMPONENT_TABLE_ROWS * 7, "MovingObjectsModule: motion_component_table is missing or of another size");
    requireImage(count, CV_32SC1, 1, 1, "MovingObjectsModule: motion_component_count is missing");
    requireImage(previous, CV_16SC1, rows, cols, "MovingObjectsModule: the previous frame's disparity is missing or of another size");
    requireImage(flow, CV_16SC2, rows, cols, "MovingObjectsModule: optflow must be a CV_16SC2 image of the disparity's size");
    const cart_ego_camera cam = cameraOf(options);
    const cart_object_params p = paramsOf(options);
    double rel[12];
    pose12(ego->result, rel);
    uint8_t *dev = scratch.dev<uint8_t>();
    if (cart_object_tracker_update(object, &cam, rel, ego->pose, &p, ids->ptr<int32_t>(), ids->step, table->ptr<cart_component>(), CARTSLAM_PLANE_COMPONENT_TABLE_ROWS,
                                   count->ptr<int32_t>(), disparity->ptr<int16_t>(), disparity->step, previous->ptr<int16_t>(), previous->step, flow->ptr<int16_t>(),
                                   flow->step, cols, rows, reinterpret_cast<cart_object *>(dev + objectsAt()), reinterpret_cast<cart_track *>(dev + tracksAt(options)),
                                   reinterpret_cast<int32_t *>(dev), s) != 0)
        failAbi("cart_object_tracker_update");
    hipCheck(hipMemcpyAsync(scratch.host(), dev, downloadBytes(options), hipMemcpyDeviceToHost, s), "hipMemcpyAsync of the moving objects");
    scratch.wait();   // the frame's only blocking synchronisation
    const uint8_t *host = scratch.host<uint8_t>();
    std::memcpy(out->counts, host, sizeof(out->counts));
    const cart_object *objects = reinterpret_cast<const cart_object *>(host + objectsAt());
    out->objects.assign(objects, objects + out->counts[2]);
    const cart_track *tracks = reinterpret_cast<const cart_track *>(host + tracksAt(options));
    for (int t = 0; t < options.maxTracks; ++t)
        if (tracks[t].state != 0) out->tracks.push_back(tracks[t]);
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_MOVING_OBJECTS, out));
}
}  // namespace cart

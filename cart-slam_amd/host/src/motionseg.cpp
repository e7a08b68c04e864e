// motionseg.cpp -- MotionSegModule (cartslam_amd/modules/motionseg.hpp): motion segmentation from flow, disparity and ego-motion, spec DESIGN.md S25.
#include "cartslam_amd/modules/motionseg.hpp"

#include <cmath>
#include <cstring>
#include <vector>

#include "cartslam_amd/modules/disparity.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/planeseg.hpp"
#include "module_support.hpp"

namespace cart {
MotionSegModule::MotionSegModule(const MotionSegOptions &options) : SyncWrapperSystemModule("MotionSeg"), options(options) {
    checkCamera(options);
    // the library's own checks, without a device: everything valid gets as far as the missing engine
    const cart_ego_camera cam = cameraOf(options);
    const cart_motion_params p{options.minDisparity, options.flowThreshold, options.disparityThreshold, options.radius, options.supportPercent};
    (void)cart_motion_segment(nullptr, &cam, kIdentityPose, &p, nullptr, 0, nullptr, 0, nullptr, 0, 1, 1, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr);
    requireLibraryAccepts();
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY, -1));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_OPTFLOW));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_EGO_MOTION));
    if (options.planes) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_PLANES));
    this->providesData.push_back(CARTSLAM_KEY_MOTION);
    this->providesData.push_back(CARTSLAM_KEY_MOTION_UNSMOOTHED);
    this->providesData.push_back(CARTSLAM_KEY_MOTION_RESIDUAL);
    if (options.planes) this->providesData.push_back(CARTSLAM_KEY_PLANES_STATIC);
    if (options.components) {
        this->providesData.push_back(CARTSLAM_KEY_MOTION_COMPONENTS);
        this->providesData.push_back(CARTSLAM_KEY_MOTION_COMPONENT_TABLE);
        this->providesData.push_back(CARTSLAM_KEY_MOTION_COMPONENT_COUNT);
    }
}

MotionSegModule::~MotionSegModule() {
    unknown.reset();
    cart_engine_destroy(engine);
}

void MotionSegModule::label(const Outputs &out) {   // the shapes disparity_planeseg publishes its own tables in
    static_assert(sizeof(cart_component) == 7 * sizeof(int32_t), "table rows are 7 x int32");
    if (cart_plane_ccl_table(engine, 1, out.labels->ptr<uint8_t>(), out.labels->step, 0, out.components->ptr<int32_t>(), out.components->step, 0,
                             out.componentTable->ptr<cart_component>(), CARTSLAM_PLANE_COMPONENT_TABLE_ROWS, out.componentCount->ptr<int32_t>(), scratch.stream()) != 0)
        failAbi("cart_plane_ccl_table");
}

system_data_t MotionSegModule::runInternal(System &, SystemRunData &data) {
    auto disparity = data.getData<image_t>(CARTSLAM_KEY_DISPARITY);
    if (disparity->empty() || disparity->type() != CV_16SC1) throw std::runtime_error("Disparity must be of type CV_16SC1");
    const int rows = disparity->rows, cols = disparity->cols;
    auto ego = data.getData<EgoMotion>(CARTSLAM_KEY_EGO_MOTION);
    std::shared_ptr<image_t> planes;
    if (options.planes) {
        planes = data.getData<image_t>(CARTSLAM_KEY_PLANES);
        requireImage(planes, CV_8UC1, rows, cols, "MotionSegModule: planes must be a CV_8UC1 image of the disparity's size");
    }
    const bool estimate = data.id > 1 && ego->result.status != 0;
    std::shared_ptr<image_t> previous, flow;
    if (estimate) {
        previous = data.getRelativeRun(-1)->getData<image_t>(CARTSLAM_KEY_DISPARITY);
        flow = data.getData<image_t>(CARTSLAM_KEY_OPTFLOW);
        requireImage(previous, CV_16SC1, rows, cols, "MotionSegModule: the previous frame's disparity is missing or of another size");
        requireImage(flow, CV_16SC2, rows, cols, "MotionSegModule: optflow must be a CV_16SC2 image of the disparity's size");
    }
    const auto make = [&] {
        Outputs o;
        o.labels = std::make_shared<image_t>(rows, cols, CV_8UC1);
        o.raw = std::make_shared<image_t>(rows, cols, CV_8UC1);
        o.residual = std::make_shared<image_t>(rows, cols, CV_16SC4);
        if (options.components) {
            o.components = std::make_shared<image_t>(rows, cols, CV_32SC1);
            o.componentTable = std::make_shared<image_t>(1, CARTSLAM_PLANE_COMPONENT_TABLE_ROWS * 7, CV_32SC1);   // tight rows
            o.componentCount = std::make_shared<image_t>(1, 1, CV_32SC1);
        }
        return o;
    };
    Outputs out;
    std::shared_ptr<image_t> planesStatic;
    std::unique_lock<std::mutex> lock(mutex);   // the lazy creation, the shared UNKNOWN images and the enqueue; not the wait
    if (!engine) {   // the geometry only: num_disparities = paths = 0 -> no SGM workspaces
        engine = createPostEngine(cols, rows);
        scratch.create();
    }
    if (!estimate) {   // frame 1, or no pose: all UNKNOWN, zero components, planes_static = planes; one set of images serves every such frame
        if (!unknown || unknown->labels->rows != rows || unknown->labels->cols != cols) {
            auto u = std::make_shared<Outputs>(make());
            u->labels->setTo(2);
            u->raw->setTo(2);
            std::vector<int16_t> record((size_t)rows * cols * 4);
            for (size_t i = 0; i < record.size(); ++i) record[i] = i % 4 == 3 ? 2 : -32768;
            u->residual->upload(record.data(), (size_t)cols * 4 * sizeof(int16_t));
            if (options.components) {
                label(*u);
                scratch.wait();
            }
            unknown = u;
        }
        out = *unknown;
        planesStatic = planes;
    } else {
        out = make();
        if (options.planes) planesStatic = std::make_shared<image_t>(rows, cols, CV_8UC1);
        const cart_ego_camera cam = cameraOf(options);
        const cart_motion_params p{options.minDisparity, options.flowThreshold, options.disparityThreshold, options.radius, options.supportPercent};
        double rel[12];
        pose12(ego->result, rel);
        if (cart_motion_segment(engine, &cam, rel, &p, disparity->ptr<int16_t>(), disparity->step, previous->ptr<int16_t>(), previous->step, flow->ptr<int16_t>(),
                                flow->step, cols, rows, out.residual->ptr<int16_t>(), out.residual->step, out.raw->ptr<uint8_t>(), out.raw->step,
                                out.labels->ptr<uint8_t>(), out.labels->step, planes ? planes->ptr<uint8_t>() : nullptr, planes ? planes->step : 0,
                                planesStatic ? planesStatic->ptr<uint8_t>() : nullptr, planesStatic ? planesStatic->step : 0, scratch.stream()) != 0)
            failAbi("cart_motion_segment");
        if (options.components) label(out);
        lock.unlock();   // the next frame may enqueue behind this one while this one waits
        scratch.wait();   // the frame's only blocking synchronisation
    }
    system_data_t result;
    result.push_back(MODULE_PAIR(CARTSLAM_KEY_MOTION, out.labels));
    result.push_back(MODULE_PAIR(CARTSLAM_KEY_MOTION_UNSMOOTHED, out.raw));
    result.push_back(MODULE_PAIR(CARTSLAM_KEY_MOTION_RESIDUAL, out.residual));
    if (options.planes) result.push_back(MODULE_PAIR(CARTSLAM_KEY_PLANES_STATIC, planesStatic));
    if (options.components) {
        result.push_back(MODULE_PAIR(CARTSLAM_KEY_MOTION_COMPONENTS, out.components));
        result.push_back(MODULE_PAIR(CARTSLAM_KEY_MOTION_COMPONENT_TABLE, out.componentTable));
        result.push_back(MODULE_PAIR(CARTSLAM_KEY_MOTION_COMPONENT_COUNT, out.componentCount));
    }
    return result;
}
}  // namespace cart

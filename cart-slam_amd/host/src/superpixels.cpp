// superpixels.cpp -- FrameOrder and SuperPixelModule (cartslam_amd/modules/superpixels.hpp).
#include "cartslam_amd/modules/superpixels.hpp"
#include "module_support.hpp"

namespace cart {
// ---------------------------------------------------------------- superpixels (superpixels.cu:19-118)
FrameOrder::Turn::Turn(FrameOrder &o, uint32_t id) : order(o), id(id) {
    std::unique_lock<std::mutex> lock(order.mutex);
    order.cv.wait(lock, [&] { return order.next >= id; });   // every earlier frame has finished, one way or the other
}
FrameOrder::Turn::~Turn() { order.finish(id); }

void FrameOrder::startAt(uint32_t id) {
    {
        std::lock_guard<std::mutex> lock(mutex);
        if (id <= next) return;
        next = id;
        while (!finishedAhead.empty() && *finishedAhead.begin() <= next) { if (*finishedAhead.begin() == next) ++next; finishedAhead.erase(finishedAhead.begin()); }
    }
    cv.notify_all();
}

void FrameOrder::finish(uint32_t id) {
    {
        std::lock_guard<std::mutex> lock(mutex);
        if (id < next) return;
        finishedAhead.insert(id);
        while (!finishedAhead.empty() && *finishedAhead.begin() == next) { finishedAhead.erase(finishedAhead.begin()); ++next; }
    }
    cv.notify_all();
}

SuperPixelModule::SuperPixelModule(const Size imageRes, const unsigned int initialIterations, const unsigned int iterations, const unsigned int blockSize,
                                   const unsigned int resetIterations, const double directCliqueCost, const double diagonalCliqueCost, const double compactnessWeight,
                                   const double progressiveCompactnessCost, const double imageWeight, const double disparityWeight)
    : SyncWrapperSystemModule("SuperPixelDetect"), initialIterations(initialIterations), iterations(iterations), resetIterations(resetIterations),
      blockSize(blockSize), requiresDisparityDerivative(disparityWeight > 0) {
    if (blockSize < 1) throw std::invalid_argument("blockSize must be more than 1");                                        // superpixels.cu:37-39
    if (directCliqueCost < 0) throw std::invalid_argument("directCliqueCost must be non-negative");                         // :41-43
    if (compactnessWeight < 0 || imageWeight < 0 || disparityWeight < 0) throw std::invalid_argument("weight must be non-negative");  // :45-47
    if (resetIterations < 1) throw std::invalid_argument("resetIterations must be at least 1");
    if (disparityWeight > 0) this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY_DERIVATIVE));
    this->providesData.push_back(CARTSLAM_KEY_SUPERPIXELS);
    this->providesData.push_back(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL);
    engine = std::make_shared<EngineHandle>(imageRes, paramsFor(imageRes, 0, 0, -1, 0, 0, 10, 120, 12));
    cart_superpixel_params p{directCliqueCost, diagonalCliqueCost, compactnessWeight, progressiveCompactnessCost, imageWeight, disparityWeight};
    if (cart_superpixels_create(engine->get(), &p, (int)blockSize, (int)blockSize, &contourRelaxation) != 0) engine->fail("cart_superpixels_create");
}

SuperPixelModule::~SuperPixelModule() { cart_superpixels_destroy(contourRelaxation); }

system_data_t SuperPixelModule::runInternal(System &, SystemRunData &data) {
    const image_t image = getReferenceImage(data.dataElement);  // the YCrCb conversion (superpixels.cu:81) happens inside cart_superpixels_relax
    if (image.type() != CV_8UC3 && image.type() != CV_8UC1) throw std::runtime_error("SuperPixelModule requires CV_8UC1 or CV_8UC3 images");
    std::shared_ptr<image_t> disparityDerivative;
    if (this->requiresDisparityDerivative) {
        disparityDerivative = data.getData<image_t>(CARTSLAM_KEY_DISPARITY_DERIVATIVE);
        if (disparityDerivative->type() != CV_16SC2) throw std::runtime_error("Disparity derivative must be of type CV_16SC2");
    }
    const unsigned int numIterations = (data.id == 1 || data.id % this->resetIterations == 0) ? this->initialIterations : this->iterations;  // :92
    auto relaxedLabelImage = std::make_shared<image_t>(image.rows, image.cols, CV_16UC1);
    int maxLabelId = 0;
    ScopedStream stream;
    {
        // The reference's mutex (:97-99), taken in frame order.  It covers the ENQUEUE only: cart_superpixels orders the
        // calls on the device (event of the previous call), so the next frame's sweeps queue up right behind this frame's
        // while this thread is still waiting for its own result -- the label state never leaves the GPU between frames.
        FrameOrder::Turn turn(order, data.id);
        if (data.id % this->resetIterations == 0)  // :104-112
            if (cart_superpixels_reset(contourRelaxation, stream.s) != 0) engine->fail("cart_superpixels_reset");
        if (cart_superpixels_relax(contourRelaxation, image.ptr<uint8_t>(), image.step, image.type() == CV_8UC3 ? 3 : 1,
                                   disparityDerivative ? disparityDerivative->ptr<int16_t>() : nullptr, disparityDerivative ? disparityDerivative->step : 0,
                                   (int)numIterations, relaxedLabelImage->ptr<uint16_t>(), relaxedLabelImage->step, stream.s) != 0)
            engine->fail("cart_superpixels_relax");
        maxLabelId = cart_superpixels_max_label(contourRelaxation);
    }
    stream.wait();
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_SUPERPIXELS, relaxedLabelImage),
                             MODULE_PAIR(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL, std::make_shared<contour::label_t>((contour::label_t)maxLabelId)));
}
}  // namespace cart

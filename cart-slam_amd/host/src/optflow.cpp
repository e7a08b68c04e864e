// optflow.cpp -- the two optical-flow modules (cartslam_amd/modules/planeseg.hpp).
#include <cstdio>

#include "cartslam_amd/modules/planeseg.hpp"
#include "module_support.hpp"

namespace cart {
// ---------------------------------------------------------------- optical flow (optflow.cpp:52-140)
ImageOpticalFlowModule::ImageOpticalFlowModule(const Size imageRes, int searchRadius, int blockRadius, int pyramidLevels, int refineRadius, bool median)
    : SyncWrapperSystemModule("ImageOpticalFlow"), searchRadius(searchRadius), blockRadius(blockRadius), pyramidLevels(pyramidLevels),
      refineRadius(refineRadius), median(median) {
    if (searchRadius < 1 || searchRadius > 16) throw std::invalid_argument("search_radius must be in [1, 16]");
    if (blockRadius < 1 || blockRadius > 3) throw std::invalid_argument("block_radius must be in [1, 3]");
    if (pyramidLevels < 1 || pyramidLevels > 6) throw std::invalid_argument("pyramid_levels must be in [1, 6]");
    if (refineRadius < 1 || refineRadius > 4) throw std::invalid_argument("refine_radius must be in [1, 4]");
    this->providesData.push_back(CARTSLAM_KEY_OPTFLOW);
    engine = std::make_shared<EngineHandle>(imageRes, paramsFor(imageRes, 0, 0, -1, 0, 0, 10, 120, 12));
}

system_data_t ImageOpticalFlowModule::runInternal(System &, SystemRunData &data) {
    if (data.id <= 1) return MODULE_RETURN(CARTSLAM_KEY_OPTFLOW, std::shared_ptr<void>());  // first run, no previous data (optflow.cpp:126-128)
    std::shared_ptr<SystemRunData> previousRun = data.getRelativeRun(-1);
    const image_t referenceCurrent = getReferenceImage(data.dataElement);
    const image_t referencePrevious = getReferenceImage(previousRun->dataElement);
    if ((referenceCurrent.type() != CV_8UC1 && referenceCurrent.type() != CV_8UC3) || referencePrevious.type() != referenceCurrent.type())
        throw std::runtime_error("ImageOpticalFlowModule requires CV_8UC1 or CV_8UC3 images");
    auto flow = std::make_shared<image_t>(referenceCurrent.rows, referenceCurrent.cols, CV_16SC2);
    ScopedStream stream;
    const int channels = referenceCurrent.type() == CV_8UC3 ? 3 : 1;
    if (pyramidLevels > 1) {
        const cart_flow_params params{pyramidLevels, searchRadius, refineRadius, blockRadius, median ? 1 : 0};
        if (cart_optical_flow_pyramid(engine->get(), referenceCurrent.ptr<uint8_t>(), referenceCurrent.step, referencePrevious.ptr<uint8_t>(),
                                      referencePrevious.step, channels, &params, flow->ptr<int16_t>(), flow->step, stream.s) != 0)
            engine->fail("cart_optical_flow_pyramid");
    } else if (cart_optical_flow(engine->get(), referenceCurrent.ptr<uint8_t>(), referenceCurrent.step, referencePrevious.ptr<uint8_t>(),
                                 referencePrevious.step, channels, searchRadius, blockRadius, flow->ptr<int16_t>(), flow->step, stream.s) != 0) {
        engine->fail("cart_optical_flow");
    }
    stream.wait();
    return MODULE_RETURN(CARTSLAM_KEY_OPTFLOW, flow);
}

system_data_t OpticalFlowFileModule::runInternal(System &system, SystemRunData &data) {
    const std::string dir = system.getDataSource()->getPath();
    const Size size = system.getDataSource()->getImageSize();
    char name[64];
    std::snprintf(name, sizeof(name), "/flow/%06u.bin", data.id - 1);
    std::vector<int16_t> host((size_t)size.width * size.height * 2);
    FILE *f = std::fopen((dir + name).c_str(), "rb");
    if (!f) throw std::runtime_error("Could not open optical flow file " + dir + name);
    const size_t got = std::fread(host.data(), sizeof(int16_t), host.size(), f);
    std::fclose(f);
    if (got != host.size()) throw std::runtime_error("Truncated optical flow file " + dir + name);
    auto flow = std::make_shared<image_t>(size.height, size.width, CV_16SC2);
    flow->upload(host.data(), (size_t)size.width * 4);
    return MODULE_RETURN(CARTSLAM_KEY_OPTFLOW, flow);
}
}  // namespace cart

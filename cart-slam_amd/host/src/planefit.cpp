// planefit.cpp -- superpixel plane fit and plane cluster (cartslam_amd/modules/planefit.hpp).
#include <algorithm>
#include <chrono>

#include "cartslam_amd/modules/planefit.hpp"
#include "cartslam_amd/modules/superpixels.hpp"
#include "module_support.hpp"

namespace cart {
// ---------------------------------------------------------------- superpixel plane fit / cluster (planefit.cu:182-445, planecluster.cpp:19-177)
class PlaneFitPool : public DeviceObjectPool<cart_planefit, cart_planefit_destroy> {
   public:
    PlaneFitPool() : DeviceObjectPool("cart_planefit_create", [](cart_engine *e, Size, cart_planefit **pf) { return cart_planefit_create(e, 16383, pf); }) {}
};

namespace {
struct PlaneInputs {
    std::shared_ptr<image_t> labels, depth;
    contour::label_t maxLabel;
};
PlaneInputs planeInputs(SystemRunData &data) {
    PlaneInputs in{data.getData<image_t>(CARTSLAM_KEY_SUPERPIXELS), data.getData<image_t>(CARTSLAM_KEY_DEPTH),
                   *data.getData<contour::label_t>(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL)};
    if (in.labels->type() != CV_16UC1) throw std::runtime_error("Superpixels must be of type CV_16UC1");
    requireImage(in.depth, CV_32FC3, in.labels->rows, in.labels->cols, "Depth must be CV_32FC3 of the superpixel image's size");
    return in;
}
}  // namespace

SuperPixelPlaneFitModule::SuperPixelPlaneFitModule(uint64_t seed) : SyncWrapperSystemModule("PlaneFit"), seed(seed), pool(std::make_shared<PlaneFitPool>()) {
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DEPTH));   // planefit.cu:182-187
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_SUPERPIXELS));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DISPARITY_DERIVATIVE));
    this->providesData.push_back(CARTSLAM_KEY_PLANES_EQ);
    this->providesData.push_back(CARTSLAM_KEY_PLANES_EQ_LABEL_PLANES);
}
SuperPixelPlaneFitModule::~SuperPixelPlaneFitModule() = default;

namespace {
std::vector<Vec4d> toPlanes(const double *p, size_t n) {
    std::vector<Vec4d> out(n);
    for (size_t k = 0; k < n; ++k) out[k] = Vec4d{p[k * 4], p[k * 4 + 1], p[k * 4 + 2], p[k * 4 + 3]};
    return out;
}
}  // namespace

system_data_t SuperPixelPlaneFitModule::runInternal(System &, SystemRunData &data) {
    const PlaneInputs in = planeInputs(data);
    auto eng = pool->engineFor(*in.labels);
    PlaneFitPool::Lease lease{*pool, pool->acquire(*in.labels)};
    PlaneFitPool::Slot &sl = *lease.slot;
    const size_t L1 = (size_t)in.maxLabel + 1;
    // output layout (device and host alike): label planes [L1][4] f64 | planes [100][4] f64 | assignments [L1] u64 | n_planes
    const size_t bytes = L1 * 32 + CART_PLANEFIT_MAX_PLANES * 32 + L1 * 8 + 8;
    sl.reserve(bytes, bytes);
    double *labelPlanesDev = sl.dev<double>();
    double *planesDev = labelPlanesDev + L1 * 4;
    uint64_t *assignDev = reinterpret_cast<uint64_t *>(planesDev + CART_PLANEFIT_MAX_PLANES * 4);
    int32_t *nDev = reinterpret_cast<int32_t *>(assignDev + L1);
    ScopedStream stream;
    if (cart_planefit_label_planes(sl.obj, in.labels->ptr<uint16_t>(), in.labels->step, (int)in.maxLabel, in.depth->ptr<float>(), in.depth->step,
                                   CART_PLANE_PREDICATE_PLANEFIT, CART_PLANEFIT_THRESHOLD, seed, data.id, labelPlanesDev, nullptr, nullptr, stream.s) != 0)
        eng->fail("cart_planefit_label_planes");
    if (cart_planefit_fit(sl.obj, in.labels->ptr<uint16_t>(), in.labels->step, seed, data.id, planesDev, assignDev, nDev, nullptr, stream.s) != 0)
        eng->fail("cart_planefit_fit");
    hipCheck(hipMemcpyAsync(sl.host(), sl.dev(), bytes, hipMemcpyDeviceToHost, stream.s), "hipMemcpyAsync of the planefit outputs");
    stream.wait();   // the frame's only blocking synchronisation
    const uint8_t *h = sl.host<uint8_t>();
    const int32_t n = *reinterpret_cast<const int32_t *>(h + L1 * 32 + CART_PLANEFIT_MAX_PLANES * 32 + L1 * 8);
    if (n < 0) throw std::runtime_error("superpixel label above superpixels_max_label");
    plane_fit_data_t out;
    out.planes = toPlanes(reinterpret_cast<const double *>(h + L1 * 32), (size_t)n);
    const uint64_t *as = reinterpret_cast<const uint64_t *>(h + L1 * 32 + CART_PLANEFIT_MAX_PLANES * 32);
    out.planeAssignments.assign(as, as + L1);
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_PLANES_EQ, std::make_shared<plane_fit_data_t>(std::move(out))),
                             MODULE_PAIR(CARTSLAM_KEY_PLANES_EQ_LABEL_PLANES, std::make_shared<std::vector<Vec4d>>(toPlanes(reinterpret_cast<const double *>(h), L1))));
}

SuperPixelPlaneClusterModule::SuperPixelPlaneClusterModule(uint64_t seed) : SyncWrapperSystemModule("PlaneCluster"), seed(seed), pool(std::make_shared<PlaneFitPool>()) {
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_DEPTH));   // planecluster.hpp:15-17
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_SUPERPIXELS));
    this->requiresData.push_back(module_dependency_t(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL));
    this->providesData.push_back(CARTSLAM_KEY_PLANES_EQ);
    this->providesData.push_back(CARTSLAM_KEY_PLANES_EQ_LABEL_PLANES);
}
SuperPixelPlaneClusterModule::~SuperPixelPlaneClusterModule() = default;

system_data_t SuperPixelPlaneClusterModule::runInternal(System &, SystemRunData &data) {
    const PlaneInputs in = planeInputs(data);
    auto eng = pool->engineFor(*in.labels);
    PlaneFitPool::Lease lease{*pool, pool->acquire(*in.labels)};
    PlaneFitPool::Slot &sl = *lease.slot;
    const size_t L1 = (size_t)in.maxLabel + 1;
    const size_t cap = std::max<size_t>(1, std::min<size_t>(8 * (size_t)in.labels->rows * in.labels->cols, L1 * (L1 - 1)));
    // layout: label planes [L1][4] f64 | offsets [L1 + 1] | neighbours [cap]; the host copy takes the head, then the neighbours
    const size_t head = L1 * 32 + (L1 + 1) * 4;
    sl.reserve(head + cap * 4, head + cap * 4);
    double *planesDev = sl.dev<double>();
    int32_t *offDev = reinterpret_cast<int32_t *>(planesDev + L1 * 4);
    int32_t *nbDev = offDev + L1 + 1;
    ScopedStream stream;
    if (cart_planefit_label_planes(sl.obj, in.labels->ptr<uint16_t>(), in.labels->step, (int)in.maxLabel, in.depth->ptr<float>(), in.depth->step,
                                   CART_PLANE_PREDICATE_PLANECLUSTER, CART_PLANEFIT_THRESHOLD, seed, data.id, planesDev, nullptr, nullptr, stream.s) != 0)
        eng->fail("cart_planefit_label_planes");
    if (cart_planefit_adjacency(sl.obj, in.labels->ptr<uint16_t>(), in.labels->step, (int)in.maxLabel, offDev, nbDev, cap, stream.s) != 0)
        eng->fail("cart_planefit_adjacency");
    hipCheck(hipMemcpyAsync(sl.host(), sl.dev(), head, hipMemcpyDeviceToHost, stream.s), "hipMemcpyAsync of the plane tables");
    stream.wait();
    uint8_t *h = sl.host<uint8_t>();
    const int32_t *off = reinterpret_cast<const int32_t *>(h + L1 * 32);
    if (off[0] != 0 || off[L1] < 0 || (size_t)off[L1] > cap) throw std::runtime_error("adjacency table out of range");
    int32_t *nb = reinterpret_cast<int32_t *>(h + head);
    if (off[L1] > 0) {
        hipCheck(hipMemcpyAsync(nb, nbDev, (size_t)off[L1] * 4, hipMemcpyDeviceToHost, stream.s), "hipMemcpyAsync of the adjacency");
        stream.wait();
    }
    int bad = 0;
    if (cart_planefit_status(sl.obj, &bad) != 0) eng->fail("cart_planefit_status");
    if (bad) throw std::runtime_error("superpixel label above superpixels_max_label");
    std::vector<double> planesOut(L1 * 4);
    std::vector<uint64_t> assign(L1);
    int n = 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (cart_plane_cluster(reinterpret_cast<const double *>(h), (int)L1 - 1, off, nb, planesOut.data(), assign.data(), &n) != 0)
        eng->fail("cart_plane_cluster");
    mergeNs.fetch_add((long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
    mergeCalls.fetch_add(1);
    plane_fit_data_t out;
    out.planes = toPlanes(planesOut.data(), (size_t)n);
    out.planeAssignments.assign(assign.begin(), assign.end());
    return MODULE_RETURN_ALL(MODULE_PAIR(CARTSLAM_KEY_PLANES_EQ, std::make_shared<plane_fit_data_t>(std::move(out))),
                             MODULE_PAIR(CARTSLAM_KEY_PLANES_EQ_LABEL_PLANES, std::make_shared<std::vector<Vec4d>>(toPlanes(reinterpret_cast<const double *>(h), L1))));
}

double SuperPixelPlaneClusterModule::meanMergeMs() const {
    const long n = mergeCalls.load();
    return n ? 1e-6 * (double)mergeNs.load() / (double)n : 0.0;
}
}  // namespace cart

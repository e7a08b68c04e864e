// modules/planefit.hpp -- mirrors include/modules/planefit.hpp + include/modules/planecluster.hpp: the two superpixel
// plane modules that read "depth" (src/modules/planefit.cu:182-445, src/modules/planecluster.cpp:19-177).  Their work
// runs behind cart_planefit_* / cart_plane_cluster (include/cart_engine.h), spec DESIGN.md S17-S19.
#pragma once
#include <array>
#include <atomic>
#include <mutex>
#include <vector>

#include "depth.hpp"
#include "superpixels.hpp"

#define CARTSLAM_KEY_PLANES_EQ "planes_eq"
// extension: the S17 plane of every label (std::vector<Vec4d>, max_label + 1 entries) the module computed on the way
#define CARTSLAM_KEY_PLANES_EQ_LABEL_PLANES "planes_eq_label_planes"

namespace cart {
typedef std::array<double, 4> Vec4d;   // cv::Vec4d: (a, b, c, d) of a*x + b*y + c*z + d = 0

struct plane_fit_data_t {
    std::vector<Vec4d> planes;
    std::vector<size_t> planeAssignments;   // [max_label + 1]: 1 + plane index, 0 = none
};

// Per-thread planefit workspaces of one module (the frames of a run may overlap).
class PlaneFitPool;

class SuperPixelPlaneFitModule : public SyncWrapperSystemModule {
   public:
    // `seed` is an extension: the reference seeds from std::random_device.  The frame id is the run id.
    explicit SuperPixelPlaneFitModule(uint64_t seed = 0);
    ~SuperPixelPlaneFitModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;

   private:
    const uint64_t seed;
    std::shared_ptr<PlaneFitPool> pool;
};

class SuperPixelPlaneClusterModule : public SyncWrapperSystemModule {
   public:
    explicit SuperPixelPlaneClusterModule(uint64_t seed = 0);
    ~SuperPixelPlaneClusterModule();
    system_data_t runInternal(System &system, SystemRunData &data) override;
    double meanMergeMs() const;   // host time of cart_plane_cluster per frame so far

   private:
    const uint64_t seed;
    std::shared_ptr<PlaneFitPool> pool;
    std::atomic<long long> mergeNs{0};
    std::atomic<long> mergeCalls{0};
};
}  // namespace cart

// module_support.hpp -- what the module files (disparity.cpp ... posegraph.cpp) share and no caller of the library sees: the HIP and C-ABI
// error checks, the stream pool, the device-object slot pool, the camera and pose helpers and the constructors' argument checks.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "cart_engine.h"
#include "cartslam_amd/modules/disparity.hpp"

namespace cart {
inline void hipCheck(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
[[noreturn]] inline void failAbi(const char *what) { throw std::runtime_error(std::string(what) + ": " + cart_last_error(nullptr)); }

// The reference creates and destroys one stream per invocation (disparity.cu:56, planeseg.cu:279-280,300-301); stream
// creation costs ~100 us here, so invocations borrow a stream from a pool instead (same concurrency, no churn).
// Two classes: the disparity module's launches fill the GPU for a millisecond at a time ("bulk", default priority);
// every other module enqueues short kernels, and on a default-priority stream their workgroups queue behind the whole
// remaining grid of whatever bulk kernel is resident (a 20 us classify kernel then takes 0.4-0.8 ms).  Those streams
// get the highest priority, so the dispatcher places their few workgroups as soon as any slot frees up.
// CARTSLAM_STREAM_PRIORITY=0 puts everything on default-priority streams.
class StreamPool {
   public:
    static StreamPool &instance();   // the process's one pool (disparity.cpp)
    hipStream_t acquire(bool bulk) {
        std::vector<hipStream_t> &idle = bulk ? idleBulk : idleShort;
        {
            std::lock_guard<std::mutex> lock(mutex);
            if (!idle.empty()) { hipStream_t s = idle.back(); idle.pop_back(); return s; }
        }
        static const bool usePriority = [] { const char *e = std::getenv("CARTSLAM_STREAM_PRIORITY"); return !e || std::atoi(e) != 0; }();
        int least = 0, greatest = 0;  // numerically: greatest priority = lowest number
        hipCheck(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
        hipStream_t s = nullptr;
        hipCheck(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, (bulk || !usePriority) ? least : greatest), "hipStreamCreateWithPriority");
        return s;
    }
    void release(hipStream_t s, bool bulk) { std::lock_guard<std::mutex> lock(mutex); (bulk ? idleBulk : idleShort).push_back(s); }

   private:
    std::mutex mutex;
    std::vector<hipStream_t> idleBulk, idleShort;
};

struct ScopedStream {
    hipStream_t s = nullptr;
    const bool bulk;
    explicit ScopedStream(bool bulk = false) : s(StreamPool::instance().acquire(bulk)), bulk(bulk), exceptionsAtEntry(std::uncaught_exceptions()) {}
    ~ScopedStream() {
        if (!s) return;
        // leaving through an exception with kernels still queued: drain them before the stream goes back to the pool and
        // before the images they touch (declared earlier, destroyed later) go back to theirs
        if (std::uncaught_exceptions() > exceptionsAtEntry) (void)hipStreamSynchronize(s);
        StreamPool::instance().release(s, bulk);
    }
    const int exceptionsAtEntry;
    void wait() { hipCheck(hipStreamSynchronize(s), "hipStreamSynchronize"); }
};

// ---------------------------------------------------------------- engines (disparity.cpp)
cart_engine_params paramsFor(Size res, int minDisparity, int numDisparities, int radius, int iterations, int paths, int p1, int p2, int uniq);
// the engine of the post stages, made for the first image's size and kept in `slot`
std::shared_ptr<EngineHandle> postEngine(std::mutex &mu, std::shared_ptr<EngineHandle> &slot, const image_t &disp);
// the frame-coalescing knobs (cartslam_amd/coalescer.hpp)
int coalesceGroups();
int coalesceMaxGroup();
int coalesceMinAhead();

// An engine of the geometry only, for one frame at a time: num_disparities = paths = 0 -> no SGM workspaces
inline cart_engine *createPostEngine(int cols, int rows) {
    cart_engine_params ep;
    cart_engine_default_params(&ep);
    ep.width = cols; ep.height = rows; ep.num_disparities = 0; ep.paths = 0; ep.max_inflight = 1;
    cart_engine *engine = nullptr;
    if (cart_engine_create(&ep, &engine) != 0) failAbi("cart_engine_create");
    return engine;
}
// Device objects keep the device of the engine they are made on, not the engine: `create(engine)` makes them on a throw-away
// post-only engine and returns NULL, or the name of the cart_*_create that failed, which is thrown with the library's error text.
template <typename F>
void makeOnPostEngine(int cols, int rows, F create) {
    cart_engine *engine = createPostEngine(cols, rows);
    const char *failed = create(engine);
    const std::string error = failed ? cart_last_error(nullptr) : "";
    cart_engine_destroy(engine);
    if (failed) throw std::runtime_error(std::string(failed) + ": " + error);
}

// ---------------------------------------------------------------- device-object slot pool (planefit / cluster, ORB)
// The engine and the device objects are made for the first frame's image size and kept: a free slot is leased per frame, so
// frames of one run may overlap.  Every slot owns one object, a device output buffer and a pinned host buffer for the download;
// both buffers only grow, and a slot is touched by one frame at a time (no allocation or free inside a frame once it has grown).
// The slots are destroyed before the engine they were made on.
template <typename T, void (*Destroy)(T *)>
class DeviceObjectPool {
   public:
    using Create = std::function<int(cart_engine *, Size, T **)>;
    struct Slot : DeviceScratch {   // the two buffers; no stream of its own, the frame borrows one from the StreamPool
        T *obj = nullptr;
        ~Slot() { Destroy(obj); }   // first the object, then the buffers
    };
    struct Lease {
        DeviceObjectPool &pool;
        Slot *slot;
        ~Lease() { std::lock_guard<std::mutex> lk(pool.mu); pool.idle.push_back(slot); }
    };
    DeviceObjectPool(const char *createName, Create create) : createName(createName), create(std::move(create)) {}
    std::shared_ptr<EngineHandle> engineFor(const image_t &image) { return postEngine(mu, engine, image); }
    Slot *acquire(const image_t &image) {
        auto eng = engineFor(image);
        std::lock_guard<std::mutex> lk(mu);
        if (!idle.empty()) { Slot *s = idle.back(); idle.pop_back(); return s; }
        if (all.empty()) { res.width = image.cols; res.height = image.rows; }
        auto s = std::make_unique<Slot>();
        if (create(eng->get(), res, &s->obj) != 0) eng->fail(createName);
        all.push_back(std::move(s));
        return all.back().get();
    }

   private:
    std::mutex mu;
    Size res;   // the first frame's: every object is made for it
    std::shared_ptr<EngineHandle> engine;
    std::vector<std::unique_ptr<Slot>> all;
    std::vector<Slot *> idle;
    const char *const createName;
    const Create create;
};

// ---------------------------------------------------------------- camera, poses, argument checks
inline cart_ego_camera cameraOf(const CameraOptions &o) { return cart_ego_camera{o.fx, o.fy, o.cx, o.cy, o.baseline}; }

inline bool positiveNumber(double v) { return v > 0 && std::isfinite(v); }

inline void checkCamera(const CameraOptions &o) {
    if (!positiveNumber(o.fx)) throw std::invalid_argument("fx must be a positive number (a source without calibration needs the camera keys)");
    if (!positiveNumber(o.fy)) throw std::invalid_argument("fy must be a positive number");
    if (!std::isfinite(o.cx)) throw std::invalid_argument("cx must be finite");
    if (!std::isfinite(o.cy)) throw std::invalid_argument("cy must be finite");
    if (!positiveNumber(o.baseline)) throw std::invalid_argument("baseline must be a positive number");
}

// The library's own argument checks, without a device: a constructor calls the C ABI with NULL objects, and everything valid gets
// as far as the missing object (`expected`); anything else is the library's message for the key that is out of range.
inline void requireLibraryAccepts(const char *expected = "bad arguments") {
    if (std::strcmp(cart_last_error(nullptr), expected) != 0) throw std::invalid_argument(cart_last_error(nullptr));
}

constexpr double kIdentityPose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// (R | t) of a relative pose as the 3 x 4 the pose-warp entry points take
inline void pose12(const cart_ego_result &r, double out[12]) {
    for (int row = 0; row < 3; ++row) {
        for (int c = 0; c < 3; ++c) out[4 * row + c] = r.R[3 * row + c];
        out[4 * row + 3] = r.t[row];
    }
}

// a blackboard image that is there, of `type` and rows x cols
inline bool isImage(const std::shared_ptr<image_t> &img, int type, int rows, int cols) {
    return img && !img->empty() && img->type() == type && img->rows == rows && img->cols == cols;
}
inline void requireImage(const std::shared_ptr<image_t> &img, int type, int rows, int cols, const char *message) {
    if (!isImage(img, type, rows, cols)) throw std::runtime_error(message);
}
}  // namespace cart

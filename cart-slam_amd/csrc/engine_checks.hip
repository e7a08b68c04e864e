// engine_checks.hip -- the argument checks the C-ABI entry points share (declared in engine_host.h).  Host code only: no launch, no HIP call.
// Every message is part of the interface (the tests compare them literally), and so is the order of the checks inside each function.

#include "engine_host.h"

namespace cart_amd {

int check_positive(const char *name, double v) {
    if (!(v > 0) || !std::isfinite(v)) return fail(std::string(name) + " must be a positive number");
    return 0;
}

int check_camera(const cart_ego_camera *cam) {
    if (!cam) return fail("camera is NULL");
    if (check_positive("fx", cam->fx) || check_positive("fy", cam->fy)) return -1;
    if (!std::isfinite(cam->cx)) return fail("cx must be finite");
    if (!std::isfinite(cam->cy)) return fail("cy must be finite");
    return check_positive("baseline", cam->baseline);
}

int check_pose(const char *name, const double *m) {
    if (!m) return fail(std::string(name) + " is NULL");
    for (int k = 0; k < 12; ++k) {
        const double bound = k % 4 == 3 ? 1e6 : 2.0;
        if (!std::isfinite(m[k]) || std::fabs(m[k]) > bound)
            return fail(std::string(name) + "[" + std::to_string(k) + "] must be finite and within " + (bound > 2.0 ? "1e6 (translation)" : "2 (rotation)"));
    }
    return 0;
}

static int check_size(const char *prefix, int w, int h) {
    if (w < 1 || w > 16384) return fail(std::string(prefix) + "width must be in [1, 16384]");
    if (h < 1 || h > 16384) return fail(std::string(prefix) + "height must be in [1, 16384]");
    return 0;
}
int check_frame_size(int w, int h) { return check_size("", w, h); }
int check_max_size(int max_width, int max_height) { return check_size("max_", max_width, max_height); }

int SizedObject::check_fits(int w, int h) const {
    if (w > max_width || h > max_height) return fail("width x height exceeds the object's " + std::to_string(max_width) + " x " + std::to_string(max_height));
    return 0;
}

int check_pitched(const Extent &x) {
    if ((x.begin() % x.elem) || (x.step % x.elem)) return fail(std::string(x.name) + " and its step must be " + std::to_string(x.elem) + "-byte aligned");
    if (x.step < x.row_bytes) return fail(std::string(x.name) + "_step is below the row size");
    return 0;
}

bool overlap(const Extent &a, const Extent &b) { return a.begin() < b.end() && b.begin() < a.end(); }

int check_outputs_apart(const Extent *all, int first_output, int n) {
    for (int i = first_output; i < n; ++i)
        for (int j = 0; all[i].ptr && j < i; ++j)
            if (all[j].ptr && overlap(all[j], all[i])) return fail(std::string(all[j].name) + " and " + all[i].name + " must not overlap");
    return 0;
}

}  // namespace cart_amd

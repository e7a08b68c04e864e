// engine_modeltrack.h -- the cart_model_track device object (spec S34), for the host translation units that use its workspaces:
// engine_modeltrack.hip, which owns it, and engine_modeltrack_color.hip (S38), which runs on the same object.  Private to csrc/.
#pragma once

#include "engine_host.h"

extern "C" {

struct cart_model_track : cart_amd::SizedObject {
    using cart_amd::SizedObject::SizedObject;
    double *partial = nullptr;                          // [kTrackColorWords][max_height]: cart_model_track_refine uses the first kDenseWords rows
    cart_amd::DenseEgoState *state = nullptr;
    cart_amd::ModelTrackColorState *color_state = nullptr;   // cart_model_track_refine_color's own pose state
};

}  // extern "C"

namespace cart_amd {

// cart_model_track_params as every call that takes them checks them, before anything else
inline int check_model_track_params(const cart_model_track_params *p) {
    if (!p) return fail("params is NULL");
    if (!(p->residual_gate > 0) || !(p->residual_gate <= 1)) return fail("residual_gate must be a number in (0, 1]");
    if (!(p->damping >= 0) || !std::isfinite(p->damping)) return fail("damping must be a number that is not negative");
    if (p->iterations < 0 || p->iterations > CART_MODEL_TRACK_MAX_ITERATIONS) return fail("iterations must be in [0, 16]");
    if (p->stride < 1 || p->stride > 16) return fail("stride must be in [1, 16]");
    if (p->min_inliers < 6 || p->min_inliers > (1 << 30)) return fail("min_inliers must be in [6, 2^30]");
    return 0;
}

}  // namespace cart_amd

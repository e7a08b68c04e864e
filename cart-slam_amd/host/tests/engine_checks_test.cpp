// engine_checks_test.cpp -- the shared argument checks of the C ABI (csrc/engine_checks.hip) on their edge extents, without a GPU.  Built by
// `make sanitize` under AddressSanitizer and UBSan together with engine_checks.hip as plain C++; the addresses below are only compared,
// never dereferenced.
#include <cassert>
#include <cstdio>
#include <limits>

#include "engine_host.h"

namespace cart_amd {
thread_local std::string g_last_error;
int fail(const std::string &msg) {
    g_last_error = msg;
    return -1;
}
}  // namespace cart_amd

using namespace cart_amd;

static bool failed_with(int rc, const char *msg) { return rc == -1 && g_last_error == msg; }

int main() {
    const auto at = [](uintptr_t a) { return reinterpret_cast<const void *>(a); };
    // a one-row image: its extent is the row, whatever the step
    const Extent row = Extent::image("row", at(0x1000), 0, 2, 100, 1);
    assert(row.end() == 0x1000 + 200);
    assert(failed_with(check_pitched(row), "row_step is below the row size"));
    assert(check_pitched(Extent::image("row", at(0x1000), 200, 2, 100, 1)) == 0);
    // the widest and tallest frame, 8-byte pixels, high in the address space
    const uintptr_t top = std::numeric_limits<uintptr_t>::max() - (uintptr_t)16384 * 16384 * 8;   // the extent ends just below the top
    const Extent big = Extent::image("big", at(top & ~(uintptr_t)7), (size_t)16384 * 8, 8, 16384, 16384);
    assert(check_pitched(big) == 0 && big.end() > big.begin());
    assert(failed_with(check_pitched(Extent::image("odd", at(0x1001), 64, 2, 16, 4)), "odd and its step must be 2-byte aligned"));
    assert(failed_with(check_pitched(Extent::image("odd", at(0x1000), 63, 2, 16, 4)), "odd and its step must be 2-byte aligned"));
    // 12-byte pixels on 4-byte alignment (CV_32FC3, built by hand as cart_planefit_label_planes does): the row is 12 * w, the alignment 4
    const auto xyz = [&](uintptr_t a, size_t step) { return Extent{"xyz", at(a), step, 4, (size_t)67 * 12, 9}; };
    assert(check_pitched(xyz(0x1004, 804)) == 0 && check_pitched(xyz(0x1000, 808)) == 0 && xyz(0x1004, 808).end() == 0x1004 + 8 * 808 + 804);
    assert(failed_with(check_pitched(xyz(0x1000, 800)), "xyz_step is below the row size"));
    assert(failed_with(check_pitched(xyz(0x1002, 804)), "xyz and its step must be 4-byte aligned"));
    assert(failed_with(check_pitched(xyz(0x1000, 806)), "xyz and its step must be 4-byte aligned"));
    // an output that ends exactly where an input begins does not overlap it; one byte further it does
    const Extent in = Extent::image("in", at(0x2000), 64, 1, 64, 4), none = Extent::image("none", nullptr, 0, 1, 64, 4);
    const Extent before = Extent::image("out", at(0x2000 - 4 * 64), 64, 1, 64, 4), into = Extent::image("out", at(0x2000 - 4 * 64 + 1), 64, 1, 64, 4);
    assert(before.end() == in.begin() && !overlap(before, in) && !overlap(in, before) && overlap(into, in) && overlap(in, into));
    const Extent apart[] = {in, none, before, none}, clash[] = {in, none, into, none};
    assert(check_outputs_apart(apart, 2, 4) == 0);
    assert(failed_with(check_outputs_apart(clash, 2, 4), "in and out must not overlap"));
    // sizes, numbers and poses
    assert(check_frame_size(1, 1) == 0 && check_frame_size(16384, 16384) == 0);
    assert(failed_with(check_frame_size(16385, 1), "width must be in [1, 16384]") && failed_with(check_frame_size(1, 0), "height must be in [1, 16384]"));
    assert(failed_with(check_max_size(0, 1), "max_width must be in [1, 16384]") && failed_with(check_max_size(1, 16385), "max_height must be in [1, 16384]"));
    assert(check_positive("v", 1e-300) == 0 && failed_with(check_positive("v", 0.0), "v must be a positive number"));
    assert(failed_with(check_positive("v", std::numeric_limits<double>::infinity()), "v must be a positive number"));
    assert(failed_with(check_positive("v", std::numeric_limits<double>::quiet_NaN()), "v must be a positive number"));
    double pose[12] = {1, 0, 0, 1e6, 0, 1, 0, -1e6, 0, 0, 1, 0};
    assert(check_pose("rel", pose) == 0 && failed_with(check_pose("rel", nullptr), "rel is NULL"));
    pose[5] = 2.5;
    assert(failed_with(check_pose("rel", pose), "rel[5] must be finite and within 2 (rotation)"));
    pose[5] = 1; pose[11] = std::numeric_limits<double>::quiet_NaN();
    assert(failed_with(check_pose("pose", pose), "pose[11] must be finite and within 1e6 (translation)"));
    const cart_ego_camera cam{700, 700, 600, 180, 0.5};
    cart_ego_camera bad = cam;
    bad.baseline = 0;
    assert(check_camera(&cam) == 0 && failed_with(check_camera(nullptr), "camera is NULL") && failed_with(check_camera(&bad), "baseline must be a positive number"));
    std::puts("engine_checks_test ok");
    return 0;
}

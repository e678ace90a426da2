// shutter_host.cpp — TEST INFRASTRUCTURE.  shutter_lerp and shutter_pose12 of take_amd/csrc/tk_shutter.h built for the
// host and run serially over placements, so that tests/test_shutter_cpu.py can hold the text the device runs
// (k_shutter_pose) to the numpy restatement (tests/shutter_ref.py) without a GPU.  Never loaded by the product.
#include <cstdint>

#include "tk_shutter.h"

extern "C" {
// marked, current: 12 doubles per placement; out: the same; ok: per placement 1 = the re-pose would take the pose, 0 =
// it would refuse it (singular or not finite).  0, or -1: a bad argument
int shutter_host_pose(const double *marked, const double *current, int32_t n, double t, double *out, int32_t *ok) {
    if (!marked || !current || !out || !ok || n < 0) return -1;
    for (int32_t i = 0; i < n; i++) ok[i] = tk::shutter_pose12(marked + 12 * (int64_t)i, current + 12 * (int64_t)i, t, out + 12 * (int64_t)i) ? 1 : 0;
    return 0;
}
double shutter_host_lerp(double t, double a, double b) { return tk::shutter_lerp(t, a, b); }
}

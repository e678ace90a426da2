// shutter_deform_host.cpp — TEST INFRASTRUCTURE.  shutter_lerp of take_amd/csrc/tk_shutter.h built for the host and run
// serially over an array, as k_shutter_vertices runs it per lane, so that tests/test_shutter_deform_cpu.py can hold the
// text the device runs to the numpy restatement (tests/shutter_deform_ref.py) without a GPU.  Never loaded by the product.
#include <cstdint>
#include <cstring>

#include "tk_shutter.h"

extern "C" {
// a, b, out: n doubles; *moved: 1 where any out[e] is not b[e] bit for bit, else 0.  0, or -1: a bad argument
int shutter_deform_host_vertices(const double *a, const double *b, int64_t n, double t, double *out, int32_t *moved) {
    if (!a || !b || !out || !moved || n < 0) return -1;
    *moved = 0;
    for (int64_t e = 0; e < n; e++) {
        out[e] = tk::shutter_lerp(t, a[e], b[e]);
        if (std::memcmp(&out[e], &b[e], sizeof(double)) != 0) *moved = 1;
    }
    return 0;
}
}

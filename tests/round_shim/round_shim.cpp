// round_shim.cpp — TEST INFRASTRUCTURE.  The outward double -> float rounding of take_amd/csrc/tk_round.h (what the
// device builder's boxes around double geometry rest on) built for the host, so that tests/test_build_info_cpu.py can
// drive it over the edge cases without a GPU.  Never loaded by the product.
#include <cstdint>

#include "tk_round.h"

extern "C" {
void round_shim_outward(const double *x, int64_t n, float *lo, float *hi) {
    for (int64_t i = 0; i < n; i++) lo[i] = tk::d2f_down(x[i]), hi[i] = tk::d2f_up(x[i]);
}
void round_shim_neighbours(const float *x, int64_t n, float *below, float *above) {
    for (int64_t i = 0; i < n; i++) below[i] = tk::f_below(x[i]), above[i] = tk::f_above(x[i]);
}
}

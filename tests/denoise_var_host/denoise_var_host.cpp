// denoise_var_host.cpp — TEST INFRASTRUCTURE.  The per-pixel functions of take_amd/csrc/tk_denoise_var.h built for the
// host (the C library's exp / expf) and run serially in the kernels' order — prologue, the levels ping-pong, the
// epilogue fused into the last — so that tests/test_denoise_var_cpu.py can hold the text the device runs to the numpy
// restatement (tests/denoise_var_ref.py) without a GPU.  Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <new>

#include "tk_denoise_var.h"

namespace {
template <class R>
int run(const void *rgb, const void *albedo, const void *normal, const void *depth, const int32_t *count, const double *m1, const double *m2, int32_t width,
        int32_t height, int32_t iterations, int32_t keep_albedo, const double *sigmas_floor, void *out, void *variance_out) {
    using namespace tk::dn;
    Params<R> P{};
    P.width = width, P.height = height;
    P.guides = (normal ? HAS_NORMAL : 0) | (depth ? HAS_DEPTH : 0) | (albedo && !keep_albedo ? DEMODULATE : 0);
    const double sc = sigmas_floor[0], sn = sigmas_floor[1], sd = sigmas_floor[2];
    P.inv_n = (R)(1.0 / (sn * sn)), P.inv_d = (R)(1.0 / (sd * sd)), P.albedo_floor = (R)sigmas_floor[3];
    const size_t npix = (size_t)width * height;
    // (operator new with an alignment: a record is 32 bytes in double)
    Rec4<R> *work = new (std::nothrow) Rec4<R>[3 * npix];
    if (!work) return -2;
    denoise_var_serial<R>(P, (const R *)rgb, (const R *)albedo, (const R *)normal, (const R *)depth, count, m1, m2, iterations, (R)(sc * sc), work, (R *)out,
                          (R *)variance_out);
    delete[] work;
    return 0;
}
}  // namespace

extern "C" {
// precision 0 float, 1 double; the guides and variance_out may be null; count int32, m1 and m2 double; sigmas_floor:
// sigma_color, sigma_normal, sigma_depth, albedo_floor (resolved: no defaults here); iterations 1..8.  out may be rgb.
// -> 0, -1 bad argument, -2 out of memory
int denoise_var_host(int32_t precision, const void *rgb, const void *albedo, const void *normal, const void *depth, const int32_t *count, const double *m1,
                     const double *m2, int32_t width, int32_t height, int32_t iterations, int32_t keep_albedo, const double *sigmas_floor, void *out,
                     void *variance_out) {
    if (!rgb || !out || !count || !m1 || !m2 || !sigmas_floor || width <= 0 || height <= 0 || iterations < 1 || iterations > tk::dn::MAX_ITERATIONS) return -1;
    if (precision == 1) return run<double>(rgb, albedo, normal, depth, count, m1, m2, width, height, iterations, keep_albedo, sigmas_floor, out, variance_out);
    if (precision == 0) return run<float>(rgb, albedo, normal, depth, count, m1, m2, width, height, iterations, keep_albedo, sigmas_floor, out, variance_out);
    return -1;
}
}

// rays_host.cpp — TEST INFRASTRUCTURE.  The two per-ray functions of take_amd/csrc/tk_rays.h (ray record -> initial path
// record, and back) built for the host and run serially, so that tests/test_rays_cpu.py can hold the text the device
// runs to its specification without a GPU.  Never loaded by the product.
#include <cstdint>

#include "take_hip.h"
#include "tk_rays.h"

namespace {
template <class R> int to_path(const void *rays, int64_t n, int32_t normalise, void *records) {
    const tk::PathState<R> st{(R *)records, n};
    for (int64_t i = 0; i < n; i++) tk::ray_to_path(((const tk::RayRec<R> *)rays)[i], normalise != 0, st, i);
    return 0;
}
template <class R> int to_ray(void *records, int64_t n, double tmin, void *rays) {
    const tk::PathState<R> st{(R *)records, n};
    for (int64_t i = 0; i < n; i++) ((tk::RayRec<R> *)rays)[i] = tk::path_to_ray(st, i, R(tmin));
    return 0;
}
}  // namespace

extern "C" {
// precision 0 float, 1 double.  rays: n records of 8 Reals (org3 tmin dir3 tmax); records: PATH_REC (32) Reals per path
// slot, slot i for ray i — ray_to_path writes its words of them, the others keep what the caller put there.
// 0, or -1: a bad argument
int rays_host_to_path(int32_t precision, const void *rays, int64_t n, int32_t normalise, void *records) {
    if (!rays || !records || n < 0) return -1;
    if (precision == 1) return to_path<double>(rays, n, normalise, records);
    if (precision == 0) return to_path<float>(rays, n, normalise, records);
    return -1;
}
// the inverse: the records' origins and directions -> n ray records with that tmin and tmax = +inf
int rays_host_to_ray(int32_t precision, void *records, int64_t n, double tmin, void *rays) {
    if (!rays || !records || n < 0) return -1;
    if (precision == 1) return to_ray<double>(records, n, tmin, rays);
    if (precision == 0) return to_ray<float>(records, n, tmin, rays);
    return -1;
}
int32_t rays_host_path_rec(void) { return tk::PATH_REC; }
int32_t rays_host_ray_bytes(int32_t precision) { return precision == 1 ? (int32_t)sizeof(tk::RayRec<double>) : (int32_t)sizeof(tk::RayRec<float>); }
}

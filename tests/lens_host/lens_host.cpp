// lens_host.cpp — TEST INFRASTRUCTURE.  The camera ray of take_amd/csrc/tk_lens.h as generate_path (tk_integrate.h)
// reaches it, built for the host and run serially over the path slots of one batch, so that tests/test_lens_cpu.py can
// hold the text the device runs to the numpy restatement (tests/lens_ref.py) without a GPU.  Never loaded by the product.
#include <cstdint>

#include "take_hip.h"
#include "tk_integrate.h"

namespace {
template <class R> int run(const void *cam_, int32_t width, int32_t height, int32_t spp, uint64_t seed, int32_t with_lens, void *records) {
    const R *c = (const R *)cam_;
    tk::DeviceScene<R> sc{};
    tk::CameraRec<R> cam{};  // (the lens members value-initialised: what a scene that never had a lens holds)
    for (int k = 0; k < 3; k++) cam.u[k] = c[k], cam.v[k] = c[3 + k], cam.w[k] = c[6 + k], cam.lookfrom[k] = c[9 + k];
    cam.viewport_width = c[12], cam.viewport_height = c[13], cam.width = width, cam.height = height;
    if (with_lens) cam.lens_radius = c[14], cam.focus = c[15];
    sc.cam = cam;
    tk::RenderParams<R> rp{};  // the whole image in one batch, as a render's first batch has it
    rp.width = width, rp.height = height, rp.n_local_rows = height, rp.npix = width * height;
    rp.inv_npix = 1.0 / (double)rp.npix, rp.inv_width = 1.0 / (double)width;
    rp.strip_first = 0, rp.strip_stride = 1, rp.spp = spp, rp.s0 = 0, rp.spb = spp, rp.seed = seed;
    const int64_t slots = (int64_t)spp * rp.npix;
    const tk::PathState<R> st{(R *)records, slots};
    for (int64_t s = 0; s < slots; s++) tk::generate_path(sc, rp, st, s);
    return 0;
}
}  // namespace

extern "C" {
// precision 0 float, 1 double.  cam: 16 Reals — u, v, w, lookfrom, viewport_width, viewport_height, lens_radius, focus
// (the last two read only where with_lens != 0).  records: PATH_REC (32) Reals per path slot, slot = sample * width *
// height + y * width + x with y = 0 the BOTTOM image row; generate_path writes its words of them, the others keep what
// the caller put there.  0, or -1: a bad argument
int lens_host_generate(int32_t precision, const void *cam, int32_t width, int32_t height, int32_t spp, uint64_t seed, int32_t with_lens, void *records) {
    if (!cam || !records || width <= 0 || height <= 0 || spp <= 0) return -1;
    if (precision == 1) return run<double>(cam, width, height, spp, seed, with_lens, records);
    if (precision == 0) return run<float>(cam, width, height, spp, seed, with_lens, records);
    return -1;
}
int32_t lens_host_path_rec(void) { return tk::PATH_REC; }
}

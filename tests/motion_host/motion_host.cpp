// motion_host.cpp — TEST INFRASTRUCTURE.  The per-pixel function of take_amd/csrc/tk_motion_pixel.h (the motion pass
// that follows moved vertices) built for the host and run serially over synthetic hit records, so that
// tests/test_motion_track_cpu.py can hold the text the device runs to the numpy restatement (tests/motion_ref.py)
// without a GPU.  Never loaded by the product.
#include <cstdint>

#include "take_hip.h"
#include "tk_motion_pixel.h"

namespace {
template <class R>
int run(const void *cam_, int32_t width, int32_t height, int64_t n, const int32_t *kind, const void *ro_, const void *rd_, const void *t_, const void *u_,
        const void *v_, const void *words_, const void *inv_, const double *fwd, const int32_t *placed, void *xy_, void *pd_) {
    const R *c = (const R *)cam_, *ro = (const R *)ro_, *rd = (const R *)rd_, *t = (const R *)t_, *u = (const R *)u_, *v = (const R *)v_;
    const R *words = (const R *)words_, *inv = (const R *)inv_;
    R *xy = (R *)xy_, *pd = (R *)pd_;
    tk::CameraRec<R> cam{};
    for (int k = 0; k < 3; k++) cam.u[k] = c[k], cam.v[k] = c[3 + k], cam.w[k] = c[6 + k], cam.lookfrom[k] = c[9 + k];
    cam.viewport_width = c[12], cam.viewport_height = c[13], cam.width = width, cam.height = height;
    for (int64_t i = 0; i < n; i++) {
        tk::MotionHit<R> h{};
        h.kind = kind[i];
        h.ro = {ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]}, h.rd = {rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]};
        h.t = t[i], h.u = u[i], h.v = v[i];
        h.words = words + 9 * i;
        if (placed[i]) h.inv = inv + 12 * i, h.fwd = fwd + 12 * i;
        tk::tracked_pixel(cam, h, xy[2 * i], xy[2 * i + 1], pd[i]);
    }
    return 0;
}
}  // namespace

extern "C" {
// precision 0 float, 1 double.  cam: 14 Reals — u, v, w, lookfrom, viewport_width, viewport_height — of the marked
// camera; per record i of n: kind (tk::MotionKind), ro / rd (3 Reals each), t, u, v, words (9 Reals), inv (12 Reals) and
// fwd (12 doubles) read where placed[i] != 0.  -> xy (2 Reals per record), pd (1).  0, or -1: a bad argument
int motion_host(int32_t precision, const void *cam, int32_t width, int32_t height, int64_t n, const int32_t *kind, const void *ro, const void *rd, const void *t,
                const void *u, const void *v, const void *words, const void *inv, const double *fwd, const int32_t *placed, void *xy, void *pd) {
    if (!cam || n < 0 || !kind || !ro || !rd || !t || !u || !v || !words || !inv || !fwd || !placed || !xy || !pd) return -1;
    if (precision == 1) return run<double>(cam, width, height, n, kind, ro, rd, t, u, v, words, inv, fwd, placed, xy, pd);
    if (precision == 0) return run<float>(cam, width, height, n, kind, ro, rd, t, u, v, words, inv, fwd, placed, xy, pd);
    return -1;
}
}

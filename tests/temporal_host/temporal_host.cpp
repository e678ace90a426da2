// temporal_host.cpp — TEST INFRASTRUCTURE.  The per-pixel function of take_amd/csrc/tk_temporal.h built for the host
// and run serially over the image, so that tests/test_temporal_cpu.py can hold the text the device runs to the numpy
// restatement (tests/temporal_ref.py) without a GPU.  Never loaded by the product.
#include <cmath>
#include <cstdint>

#include "tk_temporal.h"

namespace {
// a frame as six pointers in the order of TakeTemporalFrame: rgb, count, m1, m2, depth, shape_id
template <class R> tk::tp::Frame<R> frame(void *const *f) {
    if (!f) return {};
    return {(R *)f[0], (int32_t *)f[1], (double *)f[2], (double *)f[3], (R *)f[4], (int32_t *)f[5]};
}
template <class R>
int run(void *const *cur, void *const *hist, const void *prev_xy, const void *prev_depth, int32_t width, int32_t height, int32_t max_history, double depth_tol,
        void *const *out) {
    tk::tp::Params<R> P{};
    P.width = width, P.height = height, P.max_history = max_history, P.has_history = hist ? 1 : 0, P.depth_tol = (R)depth_tol;
    tk::tp::accumulate_serial<R>(P, frame<R>(cur), frame<R>(hist), (const R *)prev_xy, (const R *)prev_depth, frame<R>(out));
    return 0;
}
}  // namespace

extern "C" {
// precision 0 float, 1 double; cur / hist / out: six pointers each (hist may be null = no history; depth and shape_id
// may be null); max_history and depth_tol resolved (no defaults here).  out may be cur.  -> 0, -1 bad argument
int temporal_host(int32_t precision, void *const *cur, void *const *hist, const void *prev_xy, const void *prev_depth, int32_t width, int32_t height,
                  int32_t max_history, double depth_tol, void *const *out) {
    if (!cur || !out || !prev_xy || width <= 0 || height <= 0 || max_history <= 0) return -1;
    for (int k = 0; k < 4; k++)
        if (!cur[k] || !out[k] || (hist && !hist[k])) return -1;
    if (precision == 1) return run<double>(cur, hist, prev_xy, prev_depth, width, height, max_history, depth_tol, out);
    if (precision == 0) return run<float>(cur, hist, prev_xy, prev_depth, width, height, max_history, depth_tol, out);
    return -1;
}
}

// tk_temporal.h — temporal accumulation: the temporal half of SVGF (Schied et al. 2017) on the planes an adaptive
// render leaves (include/take_hip.h: take_hip_temporal_accumulate*; specification: DESIGN.md §4i).  Per pixel the
// history is fetched through the motion vector of the motion pass (tk_motion.h) with a bilinear footprint whose taps
// are tested one by one — inside the image, holding samples, the same surface id, a depth that matches where the
// point was — and blended with the current frame sample count by sample count, so that the result is again a mean
// with its count and moments: the input of the variance-guided filter (tk_denoise_var.h) and the next frame's history.
// The per-pixel function below is TK_HD and written once: the kernel at the end of this file runs it on the device,
// tests/temporal_host runs the same text on the host, tests/temporal_ref.py restates it in numpy.  Launched from
// tk_denoise.hip.
//
// Arithmetic: every + - * / is one operation in the order written (-ffp-contract=off).  The footprint, the weights,
// their sum W, the depth test and the colour are Real; the moments and the history length are double, with (double)w
// and (double)W.  Taps in the order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1); every sum starts from the
// first tap that counts and adds the later ones in that order.  depth_tol is rounded to Real once.
#pragma once
#include <cstdint>

#include "tk_common.h"

namespace tk {
namespace tp {

constexpr int TP_BX = 64, TP_BY = 4;  // the denoiser's block: a wave covers 64 consecutive x of one row

// one frame's planes for Reals of precision R (TakeTemporalFrame): depth and shape_id may be null
template <class R> struct Frame {
    R *rgb;
    int32_t *count;
    double *m1, *m2;
    R *depth;
    int32_t *shape_id;
};

// what every pixel of a call shares
template <class R> struct Params {
    int32_t width, height;
    int32_t max_history;
    int32_t has_history;  // 0: the output is the current frame
    R depth_tol;
};

// Pixel (x, y): cur (+ hist seen through prev_xy) -> out.  out may be cur (only pixel p of cur is read, before p of
// out is written); out must not be hist.  prev_depth may be null (the depth test is then off, as with a history
// without a depth plane); the id test is on when both frames have ids.
template <class R>
TK_HD void accumulate_pixel(const Params<R> &P, const Frame<R> &cur, const Frame<R> &hist, const R *prev_xy, const R *prev_depth, int x, int y,
                            const Frame<R> &out) {
    const int64_t p = (int64_t)y * P.width + x;
    const R cr = cur.rgb[3 * p], cg = cur.rgb[3 * p + 1], cb = cur.rgb[3 * p + 2];
    const int32_t c = cur.count[p];
    const double cm1 = cur.m1[p], cm2 = cur.m2[p];
    const int32_t id = cur.shape_id ? cur.shape_id[p] : -1;
    R W = R(0), hr = R(0), hg = R(0), hb = R(0);
    double a = 0, b = 0, nr = 0;
    if (P.has_history) {
        const R fx = prev_xy[2 * p] - R(0.5), fy = prev_xy[2 * p + 1] - R(0.5);
        // (a footprint with a tap inside has x0 in [-1, width - 1]; the comparison is false for a NaN, and keeps the
        // conversion to int in range)
        if (fx >= R(-1) && fx < R(P.width) && fy >= R(-1) && fy < R(P.height)) {
            const R flx = tk_floor(fx), fly = tk_floor(fy);
            const R tx = fx - flx, ty = fy - fly;
            const int x0 = (int)flx, y0 = (int)fly;
            const bool ids = cur.shape_id != nullptr && hist.shape_id != nullptr;
            const bool depths = hist.depth != nullptr && prev_depth != nullptr;
            const R pd = depths ? prev_depth[p] : R(0);
            const R wx[2] = {R(1) - tx, tx}, wy[2] = {R(1) - ty, ty};
            for (int j = 0; j < 2; j++)
                for (int i = 0; i < 2; i++) {
                    const R w = wx[i] * wy[j];
                    const int qx = x0 + i, qy = y0 + j;
                    if (!(w > R(0)) || qx < 0 || qx >= P.width || qy < 0 || qy >= P.height) continue;
                    const int64_t q = (int64_t)qy * P.width + qx;
                    const int32_t nq = hist.count[q];
                    if (nq <= 0) continue;
                    if (ids && hist.shape_id[q] != id) continue;
                    if (depths && !(tk_fabs(hist.depth[q] - pd) <= P.depth_tol * pd)) continue;
                    const double wd = (double)w, nd = (double)nq;
                    hr = hr + w * hist.rgb[3 * q], hg = hg + w * hist.rgb[3 * q + 1], hb = hb + w * hist.rgb[3 * q + 2];
                    a = a + wd * (hist.m1[q] / nd);
                    b = b + wd * (hist.m2[q] / nd);
                    nr = nr + wd * nd;
                    W = W + w;
                }
        }
    }
    R orr = cr, og = cg, ob = cb;
    int32_t n = c;
    double m1 = cm1, m2 = cm2;
    if (W > R(0)) {  // (otherwise the current frame bit for bit)
        const double Wd = (double)W;
        hr = hr / W, hg = hg / W, hb = hb / W;
        a = a / Wd, b = b / Wd, nr = nr / Wd;
        const double rounded = floor(nr + 0.5);
        const int32_t nh = rounded < (double)P.max_history ? (int32_t)rounded : P.max_history;
        n = nh + c;
        const R Rh = (R)nh, Rc = (R)c, Rn = (R)n;
        orr = (hr * Rh + cr * Rc) / Rn, og = (hg * Rh + cg * Rc) / Rn, ob = (hb * Rh + cb * Rc) / Rn;
        m1 = a * (double)nh + cm1;
        m2 = b * (double)nh + cm2;
    }
    out.rgb[3 * p] = orr, out.rgb[3 * p + 1] = og, out.rgb[3 * p + 2] = ob;
    out.count[p] = n;
    out.m1[p] = m1, out.m2[p] = m2;
    if (out.depth && cur.depth) out.depth[p] = cur.depth[p];
    if (out.shape_id && cur.shape_id) out.shape_id[p] = id;
}

// the call as the kernel runs it, serially (the host build of tests/temporal_host)
template <class R>
inline void accumulate_serial(const Params<R> &P, const Frame<R> &cur, const Frame<R> &hist, const R *prev_xy, const R *prev_depth, const Frame<R> &out) {
    for (int y = 0; y < P.height; y++)
        for (int x = 0; x < P.width; x++) accumulate_pixel(P, cur, hist, prev_xy, prev_depth, x, y, out);
}

#if defined(__HIPCC__)
// One thread per pixel on the denoiser's block.  Every load of the current frame and every store is plane-wise and
// contiguous along the wave; the four taps are the only gather, and for real motion neighbouring pixels' footprints
// overlap, so they come from lines the wave has just touched.  No LDS tile, for tk_denoise.h's reason: the footprint
// of a block is not known before prev_xy is read.
template <class R>
__global__ __launch_bounds__(TP_BX *TP_BY) void k_temporal_accumulate(Params<R> P, Frame<R> cur, Frame<R> hist, const R *prev_xy, const R *prev_depth,
                                                                      Frame<R> out) {
    const unsigned ux = blockIdx.x * TP_BX + threadIdx.x;
    if (ux >= (unsigned)P.width) return;
    for (int y = blockIdx.y * TP_BY + threadIdx.y; y < P.height; y += gridDim.y * TP_BY) accumulate_pixel(P, cur, hist, prev_xy, prev_depth, (int)ux, y, out);
}
#endif  // __HIPCC__

}  // namespace tp
}  // namespace tk

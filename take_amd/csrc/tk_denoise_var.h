// tk_denoise_var.h — the variance-guided denoiser: the spatial half of SVGF (Schied et al. 2017) on a render, its
// first-hit feature buffers and the moment planes of the adaptive sampler (include/take_hip.h:
// take_hip_denoise_variance*; specification: DESIGN.md §4h).  The A-trous levels of tk_denoise.h, but the colour term of
// a tap is the squared luminance difference over sigma_color^2 times the pixel's own variance estimate — a 3 x 3 blur
// of a variance plane that is filtered along with the colour (weights squared), so that later levels stop blurring once
// the estimate is clean.  The per-pixel functions below are TK_HD and written once: the kernels at the end of this file
// run them on the device, tests/denoise_var_host runs the same text on the host, tests/denoise_var_ref.py restates them
// in numpy.  Launched from tk_denoise.hip.
//
// Arithmetic: as tk_denoise.h — every + - * / is one operation in the order written (-ffp-contract=off), the constants
// (sigma_color^2, 1 / sigma_normal^2, 1 / sigma_depth^2, the albedo floor, 1 / 3) are computed in double and rounded to
// Real once, exp is the library's.  The initial variance is computed in double, with the operations of the adaptive
// rule (tk_adaptive.h), and rounded to Real once.  Non-finite inputs are taken as they are.
//
// Working image: still two records of four Reals per pixel, a tap still two aligned vector loads: colour {C.r, C.g,
// C.b, V} (ping-pong between the levels) and guide {N.x, N.y, N.z, D} (written once by the prologue: the depth never
// changes, so it left the ping-pong record and made room for the variance).
#pragma once
#include <cstdint>

#include "tk_denoise.h"

namespace tk {
namespace dn {

// The variance of the pixel's mean from the adaptive sampler's planes: count samples, m1 = sum of L_s, m2 = sum of
// L_s^2.  A single sample counts as 100 % relative error; count <= 0 gives 0 / 0 = NaN, which is taken as it is.
TK_HD double mean_variance(int32_t count, double m1, double m2) {
    const double n = (double)count;
    const double mean = m1 / n;
    double v = m2 / n - mean * mean;
    v = v > 0 ? v : 0;
    return count >= 2 ? v / (n - 1) : mean * mean;
}

// Am = the mean of A = max(albedo, floor): what a luminance is divided by when its channels are divided by A
template <class R> TK_HD R albedo_mean(const R A[3]) { return ((A[0] + A[1]) + A[2]) * (R)(1.0 / 3.0); }

// Prologue of pixel p: the initial variance, demodulate, pack.  (A missing normal or depth packs as 0 and is never read.)
template <class R>
TK_HD void var_pack_pixel(const Params<R> &P, const R *rgb, const R *albedo, const R *normal, const R *depth, const int32_t *count, const double *m1,
                          const double *m2, int64_t p, Rec4<R> &colour, Rec4<R> &guide) {
    R c[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
    R V = (R)mean_variance(count[p], m1[p], m2[p]);
    if (P.guides & DEMODULATE) {
        R A[3];
        albedo_of(albedo, p, P.albedo_floor, A);
        for (int k = 0; k < 3; k++) c[k] = c[k] / A[k];
        const R Am = albedo_mean(A);
        V = V / (Am * Am);
    }
    colour.v[0] = c[0], colour.v[1] = c[1], colour.v[2] = c[2], colour.v[3] = V;
    for (int k = 0; k < 3; k++) guide.v[k] = (P.guides & HAS_NORMAL) ? normal[3 * p + k] : R(0);
    guide.v[3] = (P.guides & HAS_DEPTH) ? depth[p] : R(0);
}

// One level at pixel (x, y): the 3 x 3 blur of the variance at unit spacing, then the 5 x 5 taps at distance `step`,
// dy outer and dx inner, taps outside the image skipped -> C_{i+1}(p) in out[0..2], V_{i+1}(p) in out[3].  sl2 =
// sigma_color^2.  The centre tap has weight 9/64 (its colour distance is 0), so the denominator is never 0; a colour
// term that overflows to +inf gives weight 0.
template <class R>
TK_HD void var_level_pixel(const Params<R> &P, const Rec4<R> *colour, const Rec4<R> *guide, int x, int y, int step, R sl2, R out[4]) {
    const R h[3] = {R(0.375), R(0.25), R(0.0625)}, g[2] = {R(0.5), R(0.25)};
    const int64_t p = (int64_t)y * P.width + x;
    R gn = R(0), gd = R(0);
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= P.height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= P.width) continue;
            const R k3 = g[dx < 0 ? -dx : dx] * g[dy < 0 ? -dy : dy];
            gn += k3 * colour[(int64_t)qy * P.width + qx].v[3];
            gd += k3;
        }
    }
    const R gv = gn / gd;
    const R inv_c = R(1) / (sl2 * gv + Tiny<R>::value);
    const bool guided = (P.guides & (HAS_NORMAL | HAS_DEPTH)) != 0;
    const Rec4<R> cp = colour[p];
    Rec4<R> gp{};
    if (guided) gp = guide[p];
    const R lp = (cp.v[0] + cp.v[1]) + cp.v[2];
    R num[3] = {R(0), R(0), R(0)}, nv = R(0), den = R(0);
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)step * dy;
        if (qy < 0 || qy >= P.height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)step * dx;
            if (qx < 0 || qx >= P.width) continue;
            const int64_t q = qy * P.width + qx;
            const Rec4<R> cq = colour[q];
            const R k = h[dx < 0 ? -dx : dx] * h[dy < 0 ? -dy : dy];
            const R dl = lp - ((cq.v[0] + cq.v[1]) + cq.v[2]);
            R e = (dl * dl) * inv_c;
            if (guided) {
                const Rec4<R> gq = guide[q];
                if (P.guides & HAS_NORMAL) {
                    const R n0 = gp.v[0] - gq.v[0], n1 = gp.v[1] - gq.v[1], n2 = gp.v[2] - gq.v[2];
                    e = e + ((n0 * n0 + n1 * n1) + n2 * n2) * P.inv_n;
                }
                if (P.guides & HAS_DEPTH) {
                    const R m = tk_fmax(tk_fmax(tk_fabs(gp.v[3]), tk_fabs(gq.v[3])), Tiny<R>::value);
                    const R r = (gp.v[3] - gq.v[3]) / m;
                    e = e + (r * r) * P.inv_d;
                }
            }
            const R w = k * tk_exp(-e);
            num[0] += w * cq.v[0], num[1] += w * cq.v[1], num[2] += w * cq.v[2];
            nv += (w * w) * cq.v[3];
            den += w;
        }
    }
    out[0] = num[0] / den, out[1] = num[1] / den, out[2] = num[2] / den;
    out[3] = nv / (den * den);
}

// Epilogue of pixel p: remodulate the last level's colour and variance c[0..3] into the caller's layout; variance_out
// may be null
template <class R> TK_HD void var_store_pixel(const Params<R> &P, const R c[4], const R *albedo, int64_t p, R *out, R *variance_out) {
    R A[3] = {R(1), R(1), R(1)};
    const bool demod = (P.guides & DEMODULATE) != 0;
    if (demod) albedo_of(albedo, p, P.albedo_floor, A);
    for (int k = 0; k < 3; k++) out[3 * p + k] = demod ? c[k] * A[k] : c[k];
    if (variance_out) {
        const R Am = albedo_mean(A);
        variance_out[p] = demod ? c[3] * (Am * Am) : c[3];
    }
}

// The filter as the kernels run it, serially: prologue, `iterations` levels (ping-pong), the epilogue fused into the
// last one.  work: three images of width * height records (colour, colour, guide).  (The host build of
// tests/denoise_var_host; the device launches are tk_denoise.hip's.)
template <class R>
inline void denoise_var_serial(const Params<R> &P, const R *rgb, const R *albedo, const R *normal, const R *depth, const int32_t *count, const double *m1,
                               const double *m2, int iterations, R sl2, Rec4<R> *work, R *out, R *variance_out) {
    const int64_t npix = (int64_t)P.width * P.height;
    Rec4<R> *colour[2] = {work, work + npix}, *guide = work + 2 * npix;
    for (int64_t p = 0; p < npix; p++) var_pack_pixel(P, rgb, albedo, normal, depth, count, m1, m2, p, colour[0][p], guide[p]);
    for (int i = 0; i < iterations; i++) {
        const Rec4<R> *src = colour[i & 1];
        Rec4<R> *dst = colour[(i + 1) & 1];
        for (int y = 0; y < P.height; y++)
            for (int x = 0; x < P.width; x++) {
                const int64_t p = (int64_t)y * P.width + x;
                R c[4];
                var_level_pixel(P, src, guide, x, y, 1 << i, sl2, c);
                if (i == iterations - 1)
                    var_store_pixel(P, c, albedo, p, out, variance_out);
                else
                    dst[p] = Rec4<R>{{c[0], c[1], c[2], c[3]}};
            }
    }
}

#if defined(__HIPCC__)
// Launch geometry: k_denoise_level's (a block is 64 x 4 threads, a wave 64 consecutive x of one row).  The eight extra
// loads of the blur come from the rows y - 1 .. y + 1, which the level's own taps bring into L1 at level 0; no LDS
// tile, for tk_denoise.h's reason.
template <class R>
__global__ __launch_bounds__(256) void k_denoise_var_pack(Params<R> P, const R *rgb, const R *albedo, const R *normal, const R *depth, const int32_t *count,
                                                          const double *m1, const double *m2, Rec4<R> *colour, Rec4<R> *guide) {
    const int64_t npix = (int64_t)P.width * P.height;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        Rec4<R> c, g;
        var_pack_pixel(P, rgb, albedo, normal, depth, count, m1, m2, p, c, g);
        colour[p] = c, guide[p] = g;
    }
}

// one level; LAST: the epilogue instead of the packed store (dst is then unused)
template <class R, bool LAST>
__global__ __launch_bounds__(DN_BX *DN_BY) void k_denoise_var_level(Params<R> P, const Rec4<R> *src, const Rec4<R> *guide, int step, R sl2, Rec4<R> *dst,
                                                                      const R *albedo, R *out, R *variance_out) {
    const unsigned ux = blockIdx.x * DN_BX + threadIdx.x;
    if (ux >= (unsigned)P.width) return;
    const int x = (int)ux;
    for (int y = blockIdx.y * DN_BY + threadIdx.y; y < P.height; y += gridDim.y * DN_BY) {
        const int64_t p = (int64_t)y * P.width + x;
        R c[4];
        var_level_pixel(P, src, guide, x, y, step, sl2, c);
        if (LAST)
            var_store_pixel(P, c, albedo, p, out, variance_out);
        else
            dst[p] = Rec4<R>{{c[0], c[1], c[2], c[3]}};
    }
}
#endif  // __HIPCC__

}  // namespace dn
}  // namespace tk

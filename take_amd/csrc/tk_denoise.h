// tk_denoise.h — the image-space denoiser: the edge-avoiding A-trous wavelet filter of Dammertz et al. 2010 on a
// render and its first-hit feature buffers (include/take_hip.h: take_hip_denoise*; specification: DESIGN.md §4f).
// The per-pixel functions below are TK_HD and written once: the kernels at the end of this file run them on the
// device, tests/denoise_host runs the same text on the host (the C library's exp), tests/denoise_ref.py restates
// them in numpy.  Launched from tk_denoise.hip.
//
// Arithmetic: every + - * / is one operation in the order written (-ffp-contract=off); the constants (the level's
// 4^i / sigma_color^2, 1 / sigma_normal^2, 1 / sigma_depth^2, the albedo floor) are computed in double on the host and
// rounded to Real once; exp is the library's exp / expf.  Non-finite inputs are taken as they are: a NaN or an
// infinity in a plane spreads through every pixel whose footprint holds it.
//
// Working image: two records of four Reals per pixel, so that a tap — seven Reals — is two aligned vector loads (16
// bytes each in f32, 32 in f64): colour {C.r, C.g, C.b, D} (ping-pong between the levels; D, the depth, is carried
// along unchanged) and guide {N.x, N.y, N.z, 0} (written once by the prologue, read-only afterwards).
#pragma once
#include <cstdint>

#include "tk_common.h"

namespace tk {
namespace dn {

template <class R> struct alignas(4 * sizeof(R)) Rec4 {
    R v[4];
};
static_assert(sizeof(Rec4<float>) == 16 && sizeof(Rec4<double>) == 32, "a tap is two aligned vector loads");

template <class R> struct Tiny;  // the smallest normal Real
template <> struct Tiny<float> {
    static constexpr float value = 1.17549435e-38f;
};
template <> struct Tiny<double> {
    static constexpr double value = 2.2250738585072014e-308;
};

// the library's exp of Real (a few ulp), never a reduced-precision intrinsic: the bars of the tests assume it
TK_HD float tk_exp(float x) { return expf(x); }
TK_HD double tk_exp(double x) { return exp(x); }

constexpr int MAX_ITERATIONS = 8;
enum : int32_t { HAS_NORMAL = 1, HAS_DEPTH = 2, DEMODULATE = 4 };  // which planes the caller gave / what the prologue did

// what every pixel of a call shares
template <class R> struct Params {
    int32_t width, height;
    int32_t guides;  // HAS_* | DEMODULATE
    R inv_n, inv_d;  // 1 / sigma_normal^2, 1 / sigma_depth^2
    R albedo_floor;
};

// A = max(albedo, floor) per channel: what the prologue divides by and the epilogue multiplies with
template <class R> TK_HD void albedo_of(const R *albedo, int64_t p, R floor, R A[3]) {
    for (int c = 0; c < 3; c++) A[c] = tk_fmax(albedo[3 * p + c], floor);
}

// Prologue of pixel p: demodulate and pack.  (A missing normal or depth packs as 0 and is never read.)
template <class R>
TK_HD void pack_pixel(const Params<R> &P, const R *rgb, const R *albedo, const R *normal, const R *depth, int64_t p, Rec4<R> &colour, Rec4<R> &guide) {
    R c[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
    if (P.guides & DEMODULATE) {
        R A[3];
        albedo_of(albedo, p, P.albedo_floor, A);
        for (int k = 0; k < 3; k++) c[k] = c[k] / A[k];
    }
    colour.v[0] = c[0], colour.v[1] = c[1], colour.v[2] = c[2];
    colour.v[3] = (P.guides & HAS_DEPTH) ? depth[p] : R(0);
    for (int k = 0; k < 3; k++) guide.v[k] = (P.guides & HAS_NORMAL) ? normal[3 * p + k] : R(0);
    guide.v[3] = R(0);
}

// One A-trous level at pixel (x, y): the 5 x 5 taps at distance `step`, dy outer and dx inner, taps outside the image
// skipped -> C_{i+1}(p) in out[0..2].  inv_c = 4^i / sigma_color^2 of this level.  The centre tap has weight 9/64, so
// the denominator is never 0.
template <class R>
TK_HD void level_pixel(const Params<R> &P, const Rec4<R> *colour, const Rec4<R> *guide, int x, int y, int step, R inv_c, R out[3]) {
    const R h[3] = {R(0.375), R(0.25), R(0.0625)};
    const int64_t p = (int64_t)y * P.width + x;
    const Rec4<R> cp = colour[p];
    Rec4<R> np{};
    if (P.guides & HAS_NORMAL) np = guide[p];
    R num[3] = {R(0), R(0), R(0)}, den = R(0);
    for (int dy = -2; dy <= 2; dy++) {
        const int64_t qy = (int64_t)y + (int64_t)step * dy;
        if (qy < 0 || qy >= P.height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int64_t qx = (int64_t)x + (int64_t)step * dx;
            if (qx < 0 || qx >= P.width) continue;
            const int64_t q = qy * P.width + qx;
            const Rec4<R> cq = colour[q];
            const R k = h[dx < 0 ? -dx : dx] * h[dy < 0 ? -dy : dy];
            const R d0 = cp.v[0] - cq.v[0], d1 = cp.v[1] - cq.v[1], d2 = cp.v[2] - cq.v[2];
            R e = ((d0 * d0 + d1 * d1) + d2 * d2) * inv_c;
            if (P.guides & HAS_NORMAL) {
                const Rec4<R> nq = guide[q];
                const R n0 = np.v[0] - nq.v[0], n1 = np.v[1] - nq.v[1], n2 = np.v[2] - nq.v[2];
                e = e + ((n0 * n0 + n1 * n1) + n2 * n2) * P.inv_n;
            }
            if (P.guides & HAS_DEPTH) {
                const R m = tk_fmax(tk_fmax(tk_fabs(cp.v[3]), tk_fabs(cq.v[3])), Tiny<R>::value);
                const R r = (cp.v[3] - cq.v[3]) / m;
                e = e + (r * r) * P.inv_d;
            }
            const R w = k * tk_exp(-e);
            num[0] += w * cq.v[0], num[1] += w * cq.v[1], num[2] += w * cq.v[2];
            den += w;
        }
    }
    out[0] = num[0] / den, out[1] = num[1] / den, out[2] = num[2] / den;
}

// Epilogue of pixel p: remodulate the last level's colour c into the caller's layout
template <class R> TK_HD void store_pixel(const Params<R> &P, const R c[3], const R *albedo, int64_t p, R *out) {
    R A[3] = {R(1), R(1), R(1)};
    const bool demod = (P.guides & DEMODULATE) != 0;
    if (demod) albedo_of(albedo, p, P.albedo_floor, A);
    for (int k = 0; k < 3; k++) out[3 * p + k] = demod ? c[k] * A[k] : c[k];
}

// The filter as the kernels run it, serially: prologue, `iterations` levels (ping-pong), the epilogue fused into the
// last one.  work: three images of width * height records (colour, colour, guide).  inv_c[i]: the levels' constants.
// (The host build of tests/denoise_host; the device launches are tk_denoise.hip's.)
template <class R>
inline void denoise_serial(const Params<R> &P, const R *rgb, const R *albedo, const R *normal, const R *depth, int iterations, const R *inv_c,
                           Rec4<R> *work, R *out) {
    const int64_t npix = (int64_t)P.width * P.height;
    Rec4<R> *colour[2] = {work, work + npix}, *guide = work + 2 * npix;
    for (int64_t p = 0; p < npix; p++) pack_pixel(P, rgb, albedo, normal, depth, p, colour[0][p], guide[p]);
    for (int i = 0; i < iterations; i++) {
        const Rec4<R> *src = colour[i & 1];
        Rec4<R> *dst = colour[(i + 1) & 1];
        for (int y = 0; y < P.height; y++)
            for (int x = 0; x < P.width; x++) {
                const int64_t p = (int64_t)y * P.width + x;
                R c[3];
                level_pixel(P, src, guide, x, y, 1 << i, inv_c[i], c);
                if (i == iterations - 1)
                    store_pixel(P, c, albedo, p, out);
                else
                    dst[p] = Rec4<R>{{c[0], c[1], c[2], src[p].v[3]}};
            }
    }
}

#if defined(__HIPCC__)
// Launch geometry: a block is 64 x 4 threads, a wave 64 consecutive x of one row — every tap load of a wave is one
// contiguous line of 1 KiB (f32) or 2 KiB (f64), and the row test of a tap is wave-uniform.  No LDS tile: the halo of
// level i is 2 * 2^i pixels, so a tile pays only for the first two or three levels, and at 1920 x 1080 the working set
// (three images: 100 MB in f32) stays in the Infinity Cache between the levels (DESIGN.md §4f has the measurement).
constexpr int DN_BX = 64, DN_BY = 4;

template <class R>
__global__ __launch_bounds__(256) void k_denoise_pack(Params<R> P, const R *rgb, const R *albedo, const R *normal, const R *depth, Rec4<R> *colour,
                                                      Rec4<R> *guide) {
    const int64_t npix = (int64_t)P.width * P.height;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        Rec4<R> c, g;
        pack_pixel(P, rgb, albedo, normal, depth, p, c, g);
        colour[p] = c, guide[p] = g;
    }
}

// one level; LAST: the epilogue instead of the packed store (dst is then unused)
template <class R, bool LAST>
__global__ __launch_bounds__(DN_BX *DN_BY) void k_denoise_level(Params<R> P, const Rec4<R> *src, const Rec4<R> *guide, int step, R inv_c, Rec4<R> *dst,
                                                                  const R *albedo, R *out) {
    const unsigned ux = blockIdx.x * DN_BX + threadIdx.x;
    if (ux >= (unsigned)P.width) return;
    const int x = (int)ux;
    for (int y = blockIdx.y * DN_BY + threadIdx.y; y < P.height; y += gridDim.y * DN_BY) {
        const int64_t p = (int64_t)y * P.width + x;
        R c[3];
        level_pixel(P, src, guide, x, y, step, inv_c, c);
        if (LAST)
            store_pixel(P, c, albedo, p, out);
        else
            dst[p] = Rec4<R>{{c[0], c[1], c[2], src[p].v[3]}};
    }
}
#endif  // __HIPCC__

}  // namespace dn
}  // namespace tk

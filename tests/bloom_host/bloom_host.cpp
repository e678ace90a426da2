// bloom_host.cpp — TEST INFRASTRUCTURE.  The per-pixel functions of take_amd/csrc/tk_bloom.h built for the host and run
// serially over whole images, so that tests/test_bloom_cpu.py can hold the text the device runs to the numpy restatement
// (tests/bloom_ref.py) without a GPU.  Never loaded by the product.
#include <cstdint>
#include <vector>

#include "tk_bloom.h"

namespace {
using namespace tk;

template <class R> void down_level(const bl::Params<R> &P, bool first, const R *src, int sw, int sh, R *dst, int dw, int dh) {
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            R v[3][6][6];
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) {
                    const R *px = src + ((int64_t)bl::clampi(2 * y - 2 + i, 0, sh - 1) * sw + bl::clampi(2 * x - 2 + j, 0, sw - 1)) * 3;
                    R b[3] = {px[0], px[1], px[2]};
                    if (first) bl::bright_pixel(P, px, b);
                    for (int ch = 0; ch < 3; ch++) v[ch][i][j] = b[ch];
                }
            for (int ch = 0; ch < 3; ch++) dst[((int64_t)y * dw + x) * 3 + ch] = bl::down13(v[ch]);
        }
}

// steps 1 to 5 -> U_0 (level 0's size), and the pyramid it was made in
template <class R> std::vector<R> u0_of(const bl::Params<R> &P, const R *rgb, int w, int h, const bl::Pyramid &pyr) {
    std::vector<std::vector<R>> L(pyr.n);
    for (int k = 0; k < pyr.n; k++) {
        L[k].resize((size_t)pyr.w[k] * pyr.h[k] * 3);
        if (k == 0)
            down_level(P, true, rgb, w, h, L[0].data(), pyr.w[0], pyr.h[0]);
        else
            down_level(P, false, (const R *)L[k - 1].data(), pyr.w[k - 1], pyr.h[k - 1], L[k].data(), pyr.w[k], pyr.h[k]);
    }
    for (int k = pyr.n - 2; k >= 0; k--)
        for (int y = 0; y < pyr.h[k]; y++)
            for (int x = 0; x < pyr.w[k]; x++)
                for (int ch = 0; ch < 3; ch++) {
                    R &d = L[k][((size_t)y * pyr.w[k] + x) * 3 + ch];
                    d = d + bl::up_pixel((const R *)L[k + 1].data(), pyr.w[k + 1], pyr.h[k + 1], x, y, ch);
                }
    return L[0];
}

template <class R> bl::Params<R> params(double exposure, double threshold, double knee, double intensity, const bl::Pyramid &pyr) {
    return bl::Params<R>{(R)exposure, (R)threshold, (R)knee, (R)(intensity / (double)pyr.n)};
}

template <class R> void layer(const void *rgb, int w, int h, double exposure, double threshold, double knee, double intensity, int levels, void *out) {
    const bl::Pyramid pyr = bl::pyramid_of(w, h, levels);
    const bl::Params<R> P = params<R>(exposure, threshold, knee, intensity, pyr);
    const std::vector<R> u0 = u0_of(P, (const R *)rgb, w, h, pyr);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int ch = 0; ch < 3; ch++) ((R *)out)[((int64_t)y * w + x) * 3 + ch] = P.gain * bl::up_pixel(u0.data(), pyr.w[0], pyr.h[0], x, y, ch);
}

template <class R>
void tonemap(const void *rgb, int w, int h, double exposure, double white, int32_t op, int32_t transfer, int32_t format, double threshold, double knee, double intensity,
             int levels, void *out) {
    const bl::Pyramid pyr = bl::pyramid_of(w, h, levels);
    const bl::Params<R> P = params<R>(exposure, threshold, knee, intensity, pyr);
    const dp::Params<R> T{(R)exposure, (R)(1.0 / (white * white)), op, transfer};
    const std::vector<R> u0 = u0_of(P, (const R *)rgb, w, h, pyr);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            R c[3];
            bl::composite_pixel(T, P.gain, (const R *)rgb, w, x, y, u0.data(), pyr.w[0], pyr.h[0], c);
            const int64_t p = (int64_t)y * w + x;
            if (format == TAKE_DISPLAY_RGBA)
                ((uint32_t *)out)[p] = dp::quantise(c[0]) | (dp::quantise(c[1]) << 8) | (dp::quantise(c[2]) << 16) | (255u << 24);
            else
                for (int ch = 0; ch < 3; ch++) ((R *)out)[3 * p + ch] = c[ch];
        }
}
bool bad(int32_t precision, const void *rgb, int w, int h, const void *out) { return !rgb || !out || w <= 0 || h <= 0 || (precision != 0 && precision != 1); }
}  // namespace

extern "C" {
// precision 0 float, 1 double; the options resolved (no defaults here).  -> 0, -1 bad argument
// the sizes of the pyramid -> the number of levels; w_out, h_out: TAKE_BLOOM_MAX_LEVELS ints each
int bloom_pyramid(int w, int h, int levels, int32_t *w_out, int32_t *h_out) {
    if (w <= 0 || h <= 0 || !w_out || !h_out) return -1;
    const tk::bl::Pyramid pyr = tk::bl::pyramid_of(w, h, levels);
    for (int k = 0; k < pyr.n; k++) w_out[k] = pyr.w[k], h_out[k] = pyr.h[k];
    return pyr.n;
}
// the full-resolution layer, h * w * 3 Reals (out may be rgb)
int bloom_layer(int32_t precision, const void *rgb, int w, int h, double exposure, double threshold, double knee, double intensity, int levels, void *out) {
    if (bad(precision, rgb, w, h, out)) return -1;
    precision ? layer<double>(rgb, w, h, exposure, threshold, knee, intensity, levels, out) : layer<float>(rgb, w, h, exposure, threshold, knee, intensity, levels, out);
    return 0;
}
// the composite; out: h * w * 4 bytes (RGBA) or h * w * 3 Reals (REAL, may be rgb)
int bloom_tonemap(int32_t precision, const void *rgb, int w, int h, double exposure, double white, int32_t op, int32_t transfer, int32_t format, double threshold,
                  double knee, double intensity, int levels, void *out) {
    if (bad(precision, rgb, w, h, out)) return -1;
    precision ? tonemap<double>(rgb, w, h, exposure, white, op, transfer, format, threshold, knee, intensity, levels, out)
              : tonemap<float>(rgb, w, h, exposure, white, op, transfer, format, threshold, knee, intensity, levels, out);
    return 0;
}
}

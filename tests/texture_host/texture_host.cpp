// texture_host.cpp — TEST INFRASTRUCTURE.  eval_texture<float|double> of take_amd/csrc/tk_shade.h built for the host, on a
// caller's pool of images and rows (u, v, uscale, vscale, uoffset, voffset), so that tests/test_texture_cpu.py can hold
// it to the exact reference of tests/texture_ref.py without a GPU.  With -DTEXTURE_HOST_MAIN a stand-alone program (the
// sanitizer build of the Makefile): every image shape, alone in an allocation of exactly 3 * W * H elements and in a
// pool where image k is directly followed by image k + 1, against its own list of edge-case bit patterns — denormal
// coordinates included — each result compared with a long double restatement.  Never loaded by the product.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "take_hip.h"
#include "tk_shade.h"

namespace {
using namespace tk;

// images: (width, height) pairs, laid out one after the other in `texels`; the rows go through image `image`
template <class R> void eval(int n_images, const int32_t *dims, int image, const R *texels, const double *rows, int64_t n, double *out) {
    std::vector<ImageInfo> info;
    int64_t at = 0;
    for (int k = 0; k < n_images; k++) {
        info.push_back(ImageInfo{dims[2 * k], dims[2 * k + 1], at});
        at += (int64_t)dims[2 * k] * dims[2 * k + 1];
    }
    DeviceScene<R> sc{};
    sc.images = info.data(), sc.texels = texels;
    for (int64_t r = 0; r < n; r++) {
        const double *p = rows + 6 * r;
        MaterialRec<R> m{};
        m.tex_kind = 1, m.tex_image = image;
        m.uscale = R(p[2]), m.vscale = R(p[3]), m.uoffset = R(p[4]), m.voffset = R(p[5]);
        const Vec3<R> c = eval_texture(sc, m, Vec2<R>{R(p[0]), R(p[1])});
        out[3 * r] = (double)c.x, out[3 * r + 1] = (double)c.y, out[3 * r + 2] = (double)c.z;
    }
}
}  // namespace

extern "C" {
// real: 0 float, 1 double; dims: n_images (width, height) pairs; texels: the pool in that Real, image k + 1 directly
// behind image k; rows: n x 6 doubles; out: n x 3 doubles.  -> 0, or -1 for a bad argument
int texture_host_eval(int real, int n_images, const int32_t *dims, int image, const void *texels, const double *rows, int64_t n, double *out) {
    if (!dims || !texels || !rows || !out || n < 0 || image < 0 || image >= n_images) return -1;
    if (real) eval<double>(n_images, dims, image, (const double *)texels, rows, n, out);
    else eval<float>(n_images, dims, image, (const float *)texels, rows, n, out);
    return 0;
}
}

#ifdef TEXTURE_HOST_MAIN
namespace {
// the edge classes as bit patterns: a in the window where r + 1 rounds to 1 (-2^-26, -2^-30, -2^-100, the tie -2^-25),
// -2^-24 just outside it, signed zeros, +2^-26, pred(1), 1, succ(1), -1, pred(-1), -3, 2, 2^20, the boundaries k/8 with
// both neighbours, and denormals: the smallest and the largest of either sign, and the smallest normal below zero
const uint32_t EDGES32[] = {
    0xB2800000u, 0xB0800000u, 0x8D800000u, 0xB3000000u, 0xB3800000u, 0x80000000u, 0x00000000u, 0x32800000u, 0x3F7FFFFFu, 0x3F800000u, 0x3F800001u,
    0xBF800000u, 0xBF800001u, 0xC0400000u, 0x40000000u, 0x49800000u, 0x3F000000u, 0x3EFFFFFFu, 0x3F000001u, 0x3E800000u, 0x3E7FFFFFu, 0x3E800001u,
    0x3F400000u, 0x3F3FFFFFu, 0x3F400001u, 0x3E000000u, 0x3DFFFFFFu, 0x3E000001u, 0x3EC00000u, 0x3EBFFFFFu, 0x3EC00001u, 0x3F200000u, 0x3F1FFFFFu,
    0x3F200001u, 0x3F600000u, 0x3F5FFFFFu, 0x3F600001u, 0x00000001u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu, 0x80800000u};
// the same in f64, with its own window: -2^-54 (the tie), -2^-60, -2^-1000
const uint64_t EDGES64[] = {
    0xBE50000000000000ull, 0xBE10000000000000ull, 0xB9B0000000000000ull, 0xBE60000000000000ull, 0xBE70000000000000ull, 0xBC90000000000000ull,
    0xBC30000000000000ull, 0x8170000000000000ull, 0x8000000000000000ull, 0x0000000000000000ull, 0x3E50000000000000ull, 0x3FEFFFFFFFFFFFFFull,
    0x3FF0000000000000ull, 0x3FF0000020000000ull, 0xBFF0000000000000ull, 0xBFF0000020000000ull, 0xC008000000000000ull, 0x4000000000000000ull,
    0x4130000000000000ull, 0x3FE0000000000000ull, 0x3FF0000000000001ull, 0x3FDFFFFFFFFFFFFFull, 0x3FE0000000000001ull, 0x3FD0000000000000ull,
    0x3FCFFFFFFFFFFFFFull, 0x3FD0000000000001ull, 0x3FE8000000000000ull, 0x3FE7FFFFFFFFFFFFull, 0x3FE8000000000001ull, 0x3FC0000000000000ull,
    0x3FBFFFFFFFFFFFFFull, 0x3FC0000000000001ull, 0x3FD8000000000000ull, 0x3FD7FFFFFFFFFFFFull, 0x3FD8000000000001ull, 0x3FE4000000000000ull,
    0x3FE3FFFFFFFFFFFFull, 0x3FE4000000000001ull, 0x3FEC000000000000ull, 0x3FEBFFFFFFFFFFFFull, 0x3FEC000000000001ull, 0x0000000000000001ull,
    0x8000000000000001ull, 0x000FFFFFFFFFFFFFull, 0x800FFFFFFFFFFFFFull, 0x8010000000000000ull};
const int32_t DIMS[] = {1, 1, 1, 6, 6, 1, 2, 2, 5, 4, 8, 4};  // (width, height)
constexpr int N_IMAGES = 6;

std::vector<float> edges(float) {
    std::vector<float> out;
    for (uint32_t b : EDGES32) {
        float f;
        std::memcpy(&f, &b, 4);
        out.push_back(f);
    }
    return out;
}
std::vector<double> edges(double) {
    std::vector<double> out;
    for (uint64_t b : EDGES64) {
        double f;
        std::memcpy(&f, &b, 8);
        out.push_back(f);
    }
    return out;
}

// texel values that occur once in the whole pool and are not affine in (x, y): a multiplicative permutation of 1..210
double texel_value(int64_t k) { return (double)((k + 1) * 89 % 211) / 211.0; }

// src/texture.cpp:3-25 in long double; the wrap is a - floor(a), held below 1
template <class R> void restate(const R *tx, int W, int H, const double *p, long double *out) {
    auto wrap = [](long double a) {
        const long double w = a - floorl(a);
        return w < 1.0L ? w : 1.0L - LDBL_EPSILON / 2;
    };
    // (the inputs as the Real holds them; a product and a sum of two such values are exact or far inside the bar)
    const long double x = W * wrap((long double)R(p[2]) * R(p[0]) + R(p[4])), y = H * wrap((long double)R(p[3]) * R(p[1]) + R(p[5]));
    int x1 = (int)floorl(x), y1 = (int)floorl(y);
    int x2 = x1 + 1 == W ? 0 : x1 + 1, y2 = y1 + 1 == H ? 0 : y1 + 1;
    const R *q11 = tx + 3 * ((int64_t)y1 * W + x1), *q12 = tx + 3 * ((int64_t)y2 * W + x1), *q21 = tx + 3 * ((int64_t)y1 * W + x2), *q22 = tx + 3 * ((int64_t)y2 * W + x2);
    if (x1 == x2) x2 += 1;
    if (y1 == y2) y2 += 1;
    for (int c = 0; c < 3; c++)
        out[c] = (q11[c] * (x2 - x) * (y2 - y) + q21[c] * (x - x1) * (y2 - y) + q12[c] * (x2 - x) * (y - y1) + q22[c] * (x - x1) * (y - y1)) / ((x2 - x1) * (y2 - y1));
}

template <class R> void run(int &cases, int &bad) {
    const bool f64 = sizeof(R) == 8;
    const double rtol = f64 ? 1e-11 : 5e-4, atol = f64 ? 1e-13 : 2e-5;  // the project's bars for table rows
    const std::vector<R> e = edges(R());
    const double other = 0.3125;
    std::vector<double> rows;
    auto row = [&](double u, double v, double us, double vs, double uo, double vo) { rows.insert(rows.end(), {u, v, us, vs, uo, vo}); };
    for (R a : e) {
        row(a, other, 1, 1, 0, 0), row(other, a, 1, 1, 0, 0), row(a, a, 1, 1, 0, 0);
        row(-(double)a, -(double)a, -1, -1, 0, 0);                            // the same a through a scale of -1
        if (R(R(a / 2) * 2) == a) row((double)a / 2, (double)a / 2, 2, 2, 0, 0);  // and of 2, where a / 2 is exact
        if ((double)R((double)a + 0.5) == (double)a + 0.5) row((double)a + 0.5, (double)a + 0.5, 1, 1, -0.5, -0.5);  // and an offset
    }
    row(0.5 - (f64 ? ldexp(1.0, -54) : ldexp(1.0, -25)), 0.5 - (f64 ? ldexp(1.0, -54) : ldexp(1.0, -25)), 1, 1, -0.5, -0.5);  // a = the tie
    const int64_t n = (int64_t)rows.size() / 6;
    std::vector<double> got(3 * (size_t)n);
    // 1. every image alone, in exactly 3 * W * H elements
    int64_t first = 0;
    std::vector<R> pool;
    for (int k = 0; k < N_IMAGES; k++) {
        const int W = DIMS[2 * k], H = DIMS[2 * k + 1];
        std::vector<R> img(3 * (size_t)W * H);
        for (size_t i = 0; i < img.size(); i++) img[i] = R(texel_value(first + (int64_t)i));
        first += (int64_t)img.size();
        pool.insert(pool.end(), img.begin(), img.end());
        texture_host_eval(f64, 1, DIMS + 2 * k, 0, img.data(), rows.data(), n, got.data());
        for (int64_t r = 0; r < n; r++, cases++) {
            long double want[3];
            restate(img.data(), W, H, rows.data() + 6 * r, want);
            for (int c = 0; c < 3; c++)
                if (!(fabsl(got[3 * r + c] - want[c]) <= atol + rtol * fabsl(want[c]))) {
                    if (bad++ < 20) std::printf("MISMATCH f%d alone %dx%d row %lld (u %a v %a) channel %d: %.17g, want %.17Lg\n", f64 ? 64 : 32, W, H, (long long)r, rows[6 * r], rows[6 * r + 1], c, got[3 * r + c], want[c]);
                    break;
                }
        }
    }
    // 2. the pool: image k directly followed by image k + 1, exactly sum 3 * W * H elements
    int64_t at = 0;
    for (int k = 0; k < N_IMAGES; k++) {
        const int W = DIMS[2 * k], H = DIMS[2 * k + 1];
        texture_host_eval(f64, N_IMAGES, DIMS, k, pool.data(), rows.data(), n, got.data());
        for (int64_t r = 0; r < n; r++, cases++) {
            long double want[3];
            restate(pool.data() + at, W, H, rows.data() + 6 * r, want);
            for (int c = 0; c < 3; c++)
                if (!(fabsl(got[3 * r + c] - want[c]) <= atol + rtol * fabsl(want[c]))) {
                    if (bad++ < 20) std::printf("MISMATCH f%d pooled %dx%d row %lld (u %a v %a) channel %d: %.17g, want %.17Lg\n", f64 ? 64 : 32, W, H, (long long)r, rows[6 * r], rows[6 * r + 1], c, got[3 * r + c], want[c]);
                    break;
                }
        }
        at += 3 * (int64_t)W * H;
    }
}
}  // namespace

int main() {
    int cases = 0, bad = 0;
    run<float>(cases, bad);
    run<double>(cases, bad);
    std::printf("texture_host: %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif

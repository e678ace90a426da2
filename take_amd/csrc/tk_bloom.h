// tk_bloom.h — bloom for the display transform: a bright pass, a pyramid of 13-tap downsamples, bilinear upsamples
// summed back, and the layer added between tk_display.h's exposure and its tone operator (include/take_hip.h:
// take_hip_bloom_layer*, take_hip_tonemap_bloom*; specification: DESIGN.md §4m).  The per-pixel functions below are
// TK_HD and written once: the kernels at the end of this file run them on the device, tests/bloom_host runs the same
// text on the host, tests/bloom_ref.py restates them in numpy.  Launched from tk_bloom.hip.
//
// Arithmetic: every + - * / is one operation in the order written (-ffp-contract=off); the constants are doubles
// rounded to Real once; every filter weight is a power of two or 3 or 9 times one.  No pow, no log: everything up to
// the tone operator's transfer is exactly reproducible.  The orders of additions this file fixes (§4m restates them):
//   a 2 x 2 mean      M = ((s00 + s11) + (s01 + s10)) * 0.25          (s[row][column]: the diagonals are paired)
//   a downsample      ((0.125 * ((C00 + C11) + (C01 + C10)) + 0.125 * B11) + 0.0625 * ((B01 + B21) + (B10 + B12)))
//                         + 0.03125 * ((B00 + B22) + (B02 + B20))      (B[row][column], C[row][column])
//   an upsample       (0.5625 * nn + 0.0625 * ff) + (0.1875 * nf + 0.1875 * fn)   (first letter the row: near or far)
// Every pair is one that a mirror image or a transposition maps to itself or to the other pair of its sum, so that —
// a + b being b + a — a mirrored or transposed image gives the mirrored or transposed result bit for bit.
#pragma once
#include <cstdint>

#include "take_hip.h"
#include "tk_common.h"
#include "tk_display.h"

namespace tk {
namespace bl {

constexpr int MAX_LEVELS = TAKE_BLOOM_MAX_LEVELS;

// The pyramid of a W x H image (step 3): n levels, level 0 the ceil-halving of the image, each further one of the one
// before, until both axes are 1; at most MAX_LEVELS, and at most `levels` if that is positive
struct Pyramid {
    int n;
    int w[MAX_LEVELS], h[MAX_LEVELS];
    int64_t pixels() const {
        int64_t s = 0;
        for (int k = 0; k < n; k++) s += (int64_t)w[k] * h[k];
        return s;
    }
};
inline Pyramid pyramid_of(int W, int H, int levels) {
    Pyramid p{};
    const int cap = levels > 0 && levels < MAX_LEVELS ? levels : MAX_LEVELS;
    while (p.n < cap) {
        W = (W + 1) / 2, H = (H + 1) / 2;
        p.w[p.n] = W, p.h[p.n] = H, p.n++;
        if (W == 1 && H == 1) break;
    }
    return p;
}

// what every pixel of a bloom call shares
template <class R> struct Params {
    R exposure;         // E
    R threshold, knee;  // t, k: 0 <= k <= t
    R gain;             // intensity / L
};

TK_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// steps 1 and 2: the raw pixel px[3] -> its bright part b[3]
template <class R> TK_HD void bright_pixel(const Params<R> &P, const R *px, R *b) {
    const R xr = tk_fmin(dp::expose_channel(P.exposure, px[0]), R(65504));
    const R xg = tk_fmin(dp::expose_channel(P.exposure, px[1]), R(65504));
    const R xb = tk_fmin(dp::expose_channel(P.exposure, px[2]), R(65504));
    const R Y = dp::luminance(xr, xg, xb);
    const R t = P.threshold, k = P.knee;
    R s = Y - (t - k);
    s = tk_fmin(tk_fmax(s, R(0)), R(2) * k);
    s = k > R(0) ? (s * s) / (R(4) * k) : R(0);
    const R m = tk_fmax(s, Y - t);
    const R w = m > R(0) ? m / Y : R(0);
    b[0] = xr * w, b[1] = xg * w, b[2] = xb * w;
}

// step 4: v[i][j] = the source at row 2 y - 2 + i, column 2 x - 2 + j (clamped) -> the destination pixel
template <class R> TK_HD R mean4(R s00, R s01, R s10, R s11) { return ((s00 + s11) + (s01 + s10)) * R(0.25); }
template <class R> TK_HD R down13(const R (&v)[6][6]) {
#define TK_BLOOM_M(i, j) mean4(v[i][j], v[i][(j) + 1], v[(i) + 1][j], v[(i) + 1][(j) + 1])
    const R B00 = TK_BLOOM_M(0, 0), B01 = TK_BLOOM_M(0, 2), B02 = TK_BLOOM_M(0, 4);
    const R B10 = TK_BLOOM_M(2, 0), B11 = TK_BLOOM_M(2, 2), B12 = TK_BLOOM_M(2, 4);
    const R B20 = TK_BLOOM_M(4, 0), B21 = TK_BLOOM_M(4, 2), B22 = TK_BLOOM_M(4, 4);
    const R C00 = TK_BLOOM_M(1, 1), C01 = TK_BLOOM_M(1, 3), C10 = TK_BLOOM_M(3, 1), C11 = TK_BLOOM_M(3, 3);
#undef TK_BLOOM_M
    const R centre = R(0.125) * ((C00 + C11) + (C01 + C10)) + R(0.125) * B11;
    return (centre + R(0.0625) * ((B01 + B21) + (B10 + B12))) + R(0.03125) * ((B00 + B22) + (B02 + B20));
}

// step 5: channel ch of up(src) at destination (x, y); src: sw x sh pixels of three Reals, the ceil-halving of the
// destination's size (so that the near pixel always exists; the far one is clamped)
template <class R> TK_HD R up_pixel(const R *src, int sw, int sh, int x, int y, int ch) {
    const int nx = x >> 1, fx = (x & 1) ? (nx + 1 < sw ? nx + 1 : sw - 1) : (nx > 0 ? nx - 1 : 0);
    const int ny = y >> 1, fy = (y & 1) ? (ny + 1 < sh ? ny + 1 : sh - 1) : (ny > 0 ? ny - 1 : 0);
    const R nn = src[((int64_t)ny * sw + nx) * 3 + ch], nf = src[((int64_t)ny * sw + fx) * 3 + ch];
    const R fn = src[((int64_t)fy * sw + nx) * 3 + ch], ff = src[((int64_t)fy * sw + fx) * 3 + ch];
    return (R(0.5625) * nn + R(0.0625) * ff) + (R(0.1875) * nf + R(0.1875) * fn);
}

// step 6: pixel (x, y) of the W-wide image -> y[3] in [0, 1]; u0: level 0 after the upsamples, sw x sh
template <class R> TK_HD void composite_pixel(const dp::Params<R> &P, R gain, const R *rgb, int W, int x, int y, const R *u0, int sw, int sh, R *out) {
    const int64_t p = (int64_t)y * W + x;
    for (int ch = 0; ch < 3; ch++) {
        const R xx = tk_fmin(dp::expose_channel(P.exposure, rgb[3 * p + ch]), R(65504));
        const R layer = gain * up_pixel(u0, sw, sh, x, y, ch);
        out[ch] = dp::tone_tail(P, xx + layer);
    }
}

#if defined(__HIPCC__)
// Launch geometry: 2-D.  The downsample runs one 16 x 16 block per 16 x 16 destination tile; the pixel-wise kernels run
// 64 x 4 blocks, a wave on 64 consecutive pixels of a row.  grid.y is capped and the kernels stride over it.
constexpr int TILE = 16, SRC = 2 * TILE + 4, ROW_X = 64, ROW_Y = 4, MAX_GRID_Y = 32768;

template <class R> struct Pair;
template <> struct Pair<float> { typedef float2 type; };
template <> struct Pair<double> { typedef double2 type; };

// dst (dw x dh) = the 13-tap downsample of src (sw x sh), dw = ceil(sw / 2), dh = ceil(sh / 2).  A block stages the
// 36 x 36 source pixels its tile reads — the tile's 32 x 32 and a halo of 2, coordinates clamped to the source — in LDS
// once, one plane per channel: consecutive lanes load consecutive pixels of a source row (12 or 24 contiguous bytes
// each) and write consecutive words of a plane.  FIRST: src is the image, and what is staged is its bright pass (steps
// 1 and 2), which is never stored.  Each thread then reads its 6 x 6 neighbourhood as 18 aligned pairs per channel (the
// column 2 tx + 2 p is even, a row has 36 Reals).
template <class R, bool FIRST> __global__ __launch_bounds__(TILE *TILE) void k_bloom_down(Params<R> P, const R *src, int sw, int sh, R *dst, int dw, int dh) {
    __shared__ __attribute__((aligned(16))) R tile[3][SRC][SRC];
    typedef typename Pair<R>::type R2;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * TILE + tx;
    const int tiles_y = (dh + TILE - 1) / TILE;
    for (int by = blockIdx.y; by < tiles_y; by += gridDim.y) {
        const int ox = (int)blockIdx.x * 2 * TILE - 2, oy = by * 2 * TILE - 2;
        for (int e = tid; e < SRC * SRC; e += TILE * TILE) {
            const int r = e / SRC, c = e - r * SRC;
            const R *px = src + ((int64_t)clampi(oy + r, 0, sh - 1) * sw + clampi(ox + c, 0, sw - 1)) * 3;
            R v[3];
            if (FIRST)
                bright_pixel(P, px, v);
            else
                v[0] = px[0], v[1] = px[1], v[2] = px[2];
            tile[0][r][c] = v[0], tile[1][r][c] = v[1], tile[2][r][c] = v[2];
        }
        __syncthreads();
        const int x = (int)blockIdx.x * TILE + tx, y = by * TILE + ty;
        if (x < dw && y < dh) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                R v[6][6];
#pragma unroll
                for (int i = 0; i < 6; i++)
#pragma unroll
                    for (int p = 0; p < 3; p++) {
                        const R2 two = *reinterpret_cast<const R2 *>(&tile[ch][2 * ty + i][2 * tx + 2 * p]);
                        v[i][2 * p] = two.x, v[i][2 * p + 1] = two.y;
                    }
                dst[((int64_t)y * dw + x) * 3 + ch] = down13(v);
            }
        }
        __syncthreads();  // (before the next tile is staged over this one)
    }
}

// One destination pixel (w x h) per lane from src (sw x sh, the ceil-halving).  LAYER: out = gain * up(src), the
// full-resolution layer; else out = d + up(src), U_k from D_k — out may be d: a pixel's d is read before it is written
// and src is another level.
template <class R, bool LAYER> __global__ __launch_bounds__(ROW_X *ROW_Y) void k_bloom_up(const R *d, const R *src, int sw, int sh, R *out, int w, int h, R gain) {
    const int x = (int)blockIdx.x * ROW_X + threadIdx.x;
    if (x >= w) return;
    for (int y = (int)blockIdx.y * ROW_Y + threadIdx.y; y < h; y += (int)gridDim.y * ROW_Y) {
        const int64_t q = ((int64_t)y * w + x) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const R u = up_pixel(src, sw, sh, x, y, ch);
            out[q + ch] = LAYER ? gain * u : d[q + ch] + u;
        }
    }
}

// dp::k_tonemap with the four taps of U_0 and the add.  RGBA: one 32-bit store per pixel; else three Reals per pixel
// (out may be rgb).
template <class R, bool RGBA> __global__ __launch_bounds__(ROW_X *ROW_Y) void k_tonemap_bloom(dp::Params<R> P, R gain, const R *rgb, int w, int h, const R *u0, int sw, int sh, void *out) {
    const int x = (int)blockIdx.x * ROW_X + threadIdx.x;
    if (x >= w) return;
    for (int y = (int)blockIdx.y * ROW_Y + threadIdx.y; y < h; y += (int)gridDim.y * ROW_Y) {
        R c[3];
        composite_pixel(P, gain, rgb, w, x, y, u0, sw, sh, c);
        const int64_t p = (int64_t)y * w + x;
        if (RGBA)
            ((uint32_t *)out)[p] = dp::quantise(c[0]) | (dp::quantise(c[1]) << 8) | (dp::quantise(c[2]) << 16) | (255u << 24);
        else
            ((R *)out)[3 * p] = c[0], ((R *)out)[3 * p + 1] = c[1], ((R *)out)[3 * p + 2] = c[2];
    }
}
#endif  // __HIPCC__

}  // namespace bl
}  // namespace tk

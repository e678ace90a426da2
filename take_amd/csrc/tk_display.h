// tk_display.h — the display transform: a luminance histogram for the auto-exposure, and the fused pass exposure ->
// tone operator -> sRGB transfer -> RGBA8 (include/take_hip.h: take_hip_luminance_histogram*, take_hip_tonemap*;
// specification: DESIGN.md §4j).  The per-pixel functions below are TK_HD and written once: the kernels at the end of
// this file run them on the device, tests/display_host runs the same text on the host (the C library's pow),
// tests/display_ref.py restates them in numpy.  Launched from tk_display.hip.
//
// Arithmetic: every + - * / is one operation in the order written (-ffp-contract=off); the constants (the Rec.709
// weights, the exposure, 1 / white^2, the operators' and the transfer's coefficients) are doubles rounded to Real once;
// pow is the library's pow / powf (tk_common.h's tk_pow: a few ulp, never a reduced-precision intrinsic — the bars of
// the tests assume it).  The histogram bin is integer work on the bits of the luminance rounded to float: there is no
// log anywhere, so the counts are exactly reproducible.
#pragma once
#include <cstdint>

#include "take_hip.h"
#include "tk_common.h"

namespace tk {
namespace dp {

constexpr int BINS = TAKE_LUMINANCE_BINS, SLOTS = TAKE_LUMINANCE_SLOTS;
constexpr int NONPOSITIVE = BINS, NONFINITE = BINS + 1;  // the two slots behind the bins
static_assert(SLOTS == BINS + 2 && BINS == 8 * 48, "8 bins per octave over [2^-24, 2^24), then the two extra slots");

TK_HD uint32_t float_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// Y = ((wr * r) + (wg * g)) + (wb * b) with the Rec.709 weights rounded to Real
template <class R> TK_HD R luminance(R r, R g, R b) { return ((R(0.2126) * r) + (R(0.7152) * g)) + (R(0.0722) * b); }

// The slot of a luminance: Y rounded to float (nearest even; a double beyond float's range becomes an infinity), then
// NaN or an infinity -> NONFINITE; <= 0 (either zero, any negative) -> NONPOSITIVE; otherwise the 8 exponent bits and
// the top 3 mantissa bits, counted from 2^-24 and clamped to the end bins.  Integer work on the bits only.
template <class R> TK_HD int luminance_slot(R Y) {
    const uint32_t u = float_bits((float)Y);
    if ((u & 0x7f800000u) == 0x7f800000u) return NONFINITE;
    if ((u >> 31) != 0 || u == 0) return NONPOSITIVE;
    const int k = (int)(u >> 20) - 8 * (127 - 24);
    return k < 0 ? 0 : (k > BINS - 1 ? BINS - 1 : k);
}
template <class R> TK_HD int pixel_slot(const R *rgb, int64_t p) { return luminance_slot(luminance(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2])); }

// what every pixel of a tone-mapping call shares
template <class R> struct Params {
    R exposure;  // E
    R inv_w2;    // REINHARD: 1 / white^2
    int32_t op, transfer;  // TAKE_TONEMAP_*, TAKE_TRANSFER_*
};

// One channel in two halves, so that the bloom composite (tk_bloom.h) can add its layer between them.  The head:
// exposure, NaN and negatives to 0
template <class R> TK_HD R expose_channel(R E, R c) {
    R x = c * E;
    if (!(x > R(0))) x = R(0);
    return x;
}
// The tail, from x >= 0: clamp to 65504 (every operator then stays finite in f32), the operator, clamp to 1, the
// transfer -> y in [0, 1]
template <class R> TK_HD R tone_tail(const Params<R> &P, R x) {
    x = tk_fmin(x, R(65504));
    R y = x;
    if (P.op == TAKE_TONEMAP_REINHARD)
        y = x * (R(1) + x * P.inv_w2) / (R(1) + x);
    else if (P.op == TAKE_TONEMAP_ACES)  // Narkowicz's rational fit
        y = (x * (R(2.51) * x + R(0.03))) / (x * (R(2.43) * x + R(0.59)) + R(0.14));
    y = tk_fmin(y, R(1));
    if (P.transfer == TAKE_TRANSFER_SRGB) y = y <= R(0.0031308) ? R(12.92) * y : R(1.055) * tk_pow(y, R(1.0 / 2.4)) - R(0.055);
    return y;
}
template <class R> TK_HD R tone_channel(const Params<R> &P, R c) { return tone_tail(P, expose_channel(P.exposure, c)); }
// the 8-bit code of y in [0, 1]
template <class R> TK_HD uint32_t quantise(R y) { return (uint32_t)(int)(y * R(255) + R(0.5)); }

// Pixel p -> three Reals (out may be rgb: the pixel is read before it is written)
template <class R> TK_HD void tone_pixel_real(const Params<R> &P, const R *rgb, int64_t p, R *out) {
    const R r = tone_channel(P, rgb[3 * p]), g = tone_channel(P, rgb[3 * p + 1]), b = tone_channel(P, rgb[3 * p + 2]);
    out[3 * p] = r, out[3 * p + 1] = g, out[3 * p + 2] = b;
}
// Pixel p -> the bytes R, G, B, 255 as one little-endian 32-bit word
template <class R> TK_HD uint32_t tone_pixel_rgba(const Params<R> &P, const R *rgb, int64_t p) {
    const uint32_t r = quantise(tone_channel(P, rgb[3 * p])), g = quantise(tone_channel(P, rgb[3 * p + 1])), b = quantise(tone_channel(P, rgb[3 * p + 2]));
    return r | (g << 8) | (b << 16) | (255u << 24);
}

// The kernels, for the one unit that launches them: tk_display.hip defines TK_DISPLAY_KERNELS before it includes this file;
// tk_bloom.hip includes it for the per-pixel functions above only.
#if defined(__HIPCC__) && defined(TK_DISPLAY_KERNELS)
// Launch geometry of all three kernels over the pixels: 256-thread blocks, at most MAX_BLOCKS of them, grid-stride.
constexpr int BLOCK = 256, WAVES = BLOCK / 64, MAX_BLOCKS = 2048;

// The histogram of one block's pixels -> row blockIdx.x of slab[gridDim.x][SLOTS], plain stores.  Counts are uint32 in
// LDS, one private histogram per wave so that the four waves do not hit one word; no global atomics.  The loop is
// uniform per wave (all 64 lanes share `base`), so the wave can look at itself: when every lane with a pixel falls into
// one slot — flat regions, constant images — one lane adds the lane count once instead of 64 adds serialising on a word.
template <class R> __global__ __launch_bounds__(BLOCK) void k_luminance_histogram(const R *rgb, int64_t npix, uint32_t *slab) {
    __shared__ uint32_t h[WAVES][SLOTS];
    for (int s = threadIdx.x; s < WAVES * SLOTS; s += BLOCK) (&h[0][0])[s] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    uint32_t *mine = h[threadIdx.x >> 6];
    for (int64_t base = (int64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63); base < npix; base += (int64_t)gridDim.x * BLOCK) {
        const int64_t p = base + lane;
        const bool valid = p < npix;
        const int slot = valid ? pixel_slot(rgb, p) : -1;
        const uint64_t active = __ballot(valid);  // (never 0: base < npix)
        const int first = __ffsll((unsigned long long)active) - 1;
        const int s0 = __shfl(slot, first);
        if (__ballot(valid && slot == s0) == active) {
            if (lane == first) atomicAdd(&mine[s0], (uint32_t)__popcll(active));
        } else if (valid) {
            atomicAdd(&mine[slot], 1u);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < SLOTS; s += BLOCK) {
        uint32_t c = 0;
        for (int w = 0; w < WAVES; w++) c += h[w][s];
        slab[(size_t)blockIdx.x * SLOTS + s] = c;
    }
}

// slab[blocks][SLOTS] -> hist[SLOTS] as int64.  A block is SUM_SLOTS slots x SUM_ROWS row groups: thread (x, y) sums the
// rows y, y + SUM_ROWS, ... of its slot (a wave reads two rows' 128 contiguous bytes), eight loads in flight at a time,
// then row group 0 adds the partial sums in fixed order.  (Integer sums do not depend on the order; the row groups and
// the unrolling only shorten the chain of dependent loads — with one thread per slot over 2048 rows the sum took five
// times as long as the histogram it follows.)
constexpr int SUM_SLOTS = 32, SUM_ROWS = 32;
__global__ __launch_bounds__(SUM_SLOTS *SUM_ROWS) void k_luminance_sum(const uint32_t *slab, int blocks, int64_t *hist) {
    __shared__ int64_t part[SUM_ROWS][SUM_SLOTS];
    const int s = blockIdx.x * SUM_SLOTS + threadIdx.x;
    int64_t acc = 0;
    if (s < SLOTS) {
        int b = threadIdx.y;
        for (; b + 7 * SUM_ROWS < blocks; b += 8 * SUM_ROWS) {
            uint32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = slab[(size_t)(b + k * SUM_ROWS) * SLOTS + s];
#pragma unroll
            for (int k = 0; k < 8; k++) acc += v[k];
        }
        for (; b < blocks; b += SUM_ROWS) acc += slab[(size_t)b * SLOTS + s];
    }
    part[threadIdx.y][threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.y == 0 && s < SLOTS) {
        int64_t t = 0;
        for (int k = 0; k < SUM_ROWS; k++) t += part[k][threadIdx.x];
        hist[s] = t;
    }
}

// The fused pass.  RGBA: one 32-bit store per pixel (a wave writes 256 contiguous bytes); else three Reals per pixel.
template <class R, bool RGBA> __global__ __launch_bounds__(BLOCK) void k_tonemap(Params<R> P, const R *rgb, int64_t npix, void *out) {
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < npix; p += (int64_t)gridDim.x * BLOCK) {
        if (RGBA)
            ((uint32_t *)out)[p] = tone_pixel_rgba(P, rgb, p);
        else
            tone_pixel_real(P, rgb, p, (R *)out);
    }
}
#endif  // __HIPCC__ && TK_DISPLAY_KERNELS

}  // namespace dp
}  // namespace tk

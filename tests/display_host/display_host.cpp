// display_host.cpp — TEST INFRASTRUCTURE.  The per-pixel functions of take_amd/csrc/tk_display.h built for the host (the
// C library's pow / powf) and run serially, so that tests/test_display_cpu.py can hold the text the device runs to the
// numpy restatement (tests/display_ref.py) without a GPU.  Never loaded by the product.
#include <cstdint>

#include "tk_display.h"

namespace {
template <class R> void slots(const void *rgb, int64_t npix, int32_t *out) {
    for (int64_t p = 0; p < npix; p++) out[p] = tk::dp::pixel_slot((const R *)rgb, p);
}
template <class R> void luminance_slots(const void *y, int64_t n, int32_t *out) {
    for (int64_t p = 0; p < n; p++) out[p] = tk::dp::luminance_slot(((const R *)y)[p]);
}
template <class R> void tonemap(const void *rgb, int64_t npix, double exposure, double white, int32_t op, int32_t transfer, int32_t format, void *out) {
    const tk::dp::Params<R> P{(R)exposure, (R)(1.0 / (white * white)), op, transfer};
    for (int64_t p = 0; p < npix; p++) {
        if (format == TAKE_DISPLAY_RGBA)
            ((uint32_t *)out)[p] = tk::dp::tone_pixel_rgba(P, (const R *)rgb, p);
        else
            tk::dp::tone_pixel_real(P, (const R *)rgb, p, (R *)out);
    }
}
}  // namespace

extern "C" {
// precision 0 float, 1 double.  -> 0, -1 bad argument
// the slot (bin, 384 non-positive, 385 non-finite) of each of npix pixels
int display_slots(int32_t precision, const void *rgb, int64_t npix, int32_t *out) {
    if (!rgb || !out || npix < 0 || (precision != 0 && precision != 1)) return -1;
    precision ? slots<double>(rgb, npix, out) : slots<float>(rgb, npix, out);
    return 0;
}
// the slot of each of n luminances (so that a test can put one exactly on a bin's edge)
int display_luminance_slots(int32_t precision, const void *y, int64_t n, int32_t *out) {
    if (!y || !out || n < 0 || (precision != 0 && precision != 1)) return -1;
    precision ? luminance_slots<double>(y, n, out) : luminance_slots<float>(y, n, out);
    return 0;
}
// exposure and white resolved (no defaults, no auto-exposure here); out: npix * 4 bytes (RGBA) or npix * 3 Reals (REAL,
// may be rgb)
int display_tonemap(int32_t precision, const void *rgb, int64_t npix, double exposure, double white, int32_t op, int32_t transfer, int32_t format, void *out) {
    if (!rgb || !out || npix < 0 || (precision != 0 && precision != 1)) return -1;
    precision ? tonemap<double>(rgb, npix, exposure, white, op, transfer, format, out) : tonemap<float>(rgb, npix, exposure, white, op, transfer, format, out);
    return 0;
}
}

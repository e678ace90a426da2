// tk_display_host.h — what tk_display.hip (the display transform) shares with tk_bloom.hip (its bloom variant): the
// resolved options, the argument checks, the histogram launches and the auto-exposure.  Defined in tk_display.hip; the
// kernels of tk_display.h are compiled there only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "take_hip.h"

namespace tk_display {

// TakeExposureOpts with the defaults filled in
struct ExposureOpts {
    double key = 0.18, low_fraction = 0.05, high_fraction = 0.95, min_exposure = 1.0 / 65536.0, max_exposure = 65536.0, prev_exposure = 0.0, rate = 1.0;
};
// TakeTonemapOpts with the defaults filled in
struct TonemapOpts {
    double exposure = 0.0, white = 4.0;  // exposure <= 0: automatic
    int op = TAKE_TONEMAP_ACES, transfer = TAKE_TRANSFER_SRGB, format = TAKE_DISPLAY_RGBA;
    ExposureOpts auto_opts;
};

inline size_t real_bytes(int32_t precision) { return precision == TAKE_PRECISION_F64 ? 8 : 4; }
// steps 1 to 8 of take_hip_auto_exposure (include/take_hip.h), in double; hist: no negative count
double auto_exposure(const int64_t *hist, const ExposureOpts &o);
// what both tone-mapping calls (and their bloom variants) refuse, before a device is looked for
int check_tonemap_args(const void *rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts, const void *out, TonemapOpts &o);
// the uint32 words the histogram's slab needs for npix pixels: the blocks' rows, then the sums
size_t histogram_slab_words(int64_t npix);
// The two histogram launches and the copy to the host, on `stream`, drained.  The device is there.  slab: device
// memory of histogram_slab_words(width * height) words, 8-byte aligned, or null = allocated here and freed on return.
int histogram_on_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, int64_t *hist_out_host, hipStream_t stream, uint32_t *slab = nullptr);

}  // namespace tk_display

// tk_display.hip — the C entry points of the display transform (include/take_hip.h: take_hip_luminance_histogram*,
// take_hip_auto_exposure, take_hip_tonemap*) and the only unit that compiles the kernels of tk_display.h.  Scene-free,
// as the scene-free denoiser calls of tk_denoise.hip: the block histograms are allocated per call, the host twins stage
// their planes through StagedPlanes.  The auto-exposure is host arithmetic in double and needs no device.  What the
// bloom variant of the transform (tk_bloom.hip) shares is declared in tk_display_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "take_hip.h"
#include "tk_host.h"
#define TK_DISPLAY_KERNELS  // this unit compiles tk_display.h's kernels
#include "tk_display.h"
#include "tk_display_host.h"

using namespace tk;
using namespace tk_host;
using namespace tk_display;

namespace {
int resolve_exposure(const TakeExposureOpts *o, ExposureOpts &r) {
    r = ExposureOpts{};
    if (!o) return TAKE_OK;
    for (double v : {o->key, o->low_fraction, o->high_fraction, o->min_exposure, o->max_exposure, o->prev_exposure, o->rate})
        if (!std::isfinite(v)) return fail(TAKE_E_INVALID, "the exposure options must be finite");
    if (o->key > 0) r.key = o->key;
    if (o->low_fraction >= 0) r.low_fraction = o->low_fraction;
    if (o->high_fraction > 0) r.high_fraction = o->high_fraction;
    if (o->min_exposure > 0) r.min_exposure = o->min_exposure;
    if (o->max_exposure > 0) r.max_exposure = o->max_exposure;
    if (o->prev_exposure > 0) r.prev_exposure = o->prev_exposure;
    if (o->rate > 0) r.rate = o->rate;
    if (r.high_fraction > 1) return fail(TAKE_E_INVALID, "high_fraction must be at most 1");
    if (r.low_fraction >= r.high_fraction) return fail(TAKE_E_INVALID, "low_fraction must be below high_fraction");
    if (r.rate > 1) return fail(TAKE_E_INVALID, "rate must be at most 1");
    if (r.min_exposure > r.max_exposure) return fail(TAKE_E_INVALID, "min_exposure must be at most max_exposure");
    return TAKE_OK;
}
}  // namespace

double tk_display::auto_exposure(const int64_t *hist, const ExposureOpts &o) {
    int64_t N = 0;
    for (int b = 0; b < dp::BINS; b++) N += hist[b];
    double target = 1.0;
    if (N > 0) {
        const double a = o.low_fraction * (double)N, z = o.high_fraction * (double)N;
        double sw = 0.0, swl = 0.0, sn = 0.0, snl = 0.0;  // between the percentiles; all bins
        int64_t cum = 0;
        for (int b = 0; b < dp::BINS; b++) {
            const double c0 = (double)cum;
            cum += hist[b];
            const double c1 = (double)cum;
            const double w = std::max(0.0, std::min(c1, z) - std::max(c0, a));
            const double l = (double)(b / 8 - 24) + std::log2(1.0 + ((double)(b % 8) + 0.5) / 8.0);
            sw = sw + w, swl = swl + w * l;
            sn = sn + (double)hist[b], snl = snl + (double)hist[b] * l;
        }
        const double mean = sw > 0.0 ? swl / sw : snl / sn;
        target = o.key / std::exp2(mean);
    }
    double E = target;
    if (o.prev_exposure > 0) {
        const double lp = std::log2(o.prev_exposure);
        E = std::exp2(lp + o.rate * (std::log2(target) - lp));
    }
    return std::min(std::max(E, o.min_exposure), o.max_exposure);
}

namespace {
int resolve_tonemap(const TakeTonemapOpts *o, TonemapOpts &r) {
    r = TonemapOpts{};
    if (!o) return TAKE_OK;
    if (o->op != TAKE_TONEMAP_LINEAR && o->op != TAKE_TONEMAP_REINHARD && o->op != TAKE_TONEMAP_ACES) return fail(TAKE_E_INVALID, "unknown tone operator");
    if (o->transfer != TAKE_TRANSFER_SRGB && o->transfer != TAKE_TRANSFER_LINEAR) return fail(TAKE_E_INVALID, "unknown transfer");
    if (o->format != TAKE_DISPLAY_RGBA && o->format != TAKE_DISPLAY_REAL) return fail(TAKE_E_INVALID, "unknown output format");
    if (o->reserved != 0) return fail(TAKE_E_INVALID, "reserved must be 0");
    if (!std::isfinite(o->exposure) || !std::isfinite(o->white)) return fail(TAKE_E_INVALID, "exposure and white must be finite");
    r.op = o->op, r.transfer = o->transfer, r.format = o->format;
    if (o->exposure > 0) r.exposure = o->exposure;
    if (o->white > 0) r.white = o->white;
    return resolve_exposure(&o->auto_opts, r.auto_opts);
}
}  // namespace

int tk_display::check_tonemap_args(const void *rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts, const void *out, TonemapOpts &o) {
    if (!rgb || !out) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_image(precision, width, height)) return rc;
    if (int rc = resolve_tonemap(opts, o)) return rc;
    if (o.format == TAKE_DISPLAY_RGBA) {
        const size_t npix = (size_t)width * height;
        const char *a = (const char *)rgb, *b = (const char *)out;
        if (a < b + 4 * npix && b < a + 3 * real_bytes(precision) * npix) return fail(TAKE_E_INVALID, "RGBA output must not overlap the input");
        if ((uintptr_t)out % 4) return fail(TAKE_E_INVALID, "RGBA output must be 4-byte aligned");
    }
    return TAKE_OK;
}

namespace {
dim3 pixel_grid(int64_t npix) { return dim3((unsigned)std::min<int64_t>((npix + dp::BLOCK - 1) / dp::BLOCK, dp::MAX_BLOCKS)); }
}  // namespace

// the blocks' rows, then (8-byte aligned: SLOTS is even) the sums
size_t tk_display::histogram_slab_words(int64_t npix) { return ((size_t)pixel_grid(npix).x + 2) * dp::SLOTS; }

int tk_display::histogram_on_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, int64_t *hist_out_host, hipStream_t stream, uint32_t *slab) {
    const int64_t npix = (int64_t)width * height;
    const dim3 grid = pixel_grid(npix);
    DevBuf<uint32_t> own;
    if (!slab) {
        if (own.alloc(histogram_slab_words(npix)) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the block histograms");
        slab = own.p;
    }
    int64_t *d_hist = (int64_t *)(slab + (size_t)grid.x * dp::SLOTS);
    with_real(precision, [&](auto tag) {
        using R = decltype(tag);
        hipLaunchKernelGGL((dp::k_luminance_histogram<R>), grid, dim3(dp::BLOCK), 0, stream, (const R *)d_rgb, npix, slab);
        return 0;
    });
    hipLaunchKernelGGL(dp::k_luminance_sum, dim3((dp::SLOTS + dp::SUM_SLOTS - 1) / dp::SUM_SLOTS), dim3(dp::SUM_SLOTS, dp::SUM_ROWS), 0, stream, (const uint32_t *)slab, (int)grid.x, d_hist);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hist_out_host, d_hist, dp::SLOTS * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return TAKE_OK;
}

extern "C" {

int take_hip_luminance_histogram_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, int64_t *hist_out_host, void *stream) {
    if (!d_rgb || !hist_out_host) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_image(precision, width, height)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    return histogram_on_device(d_rgb, precision, width, height, hist_out_host, (hipStream_t)stream);
}

int take_hip_luminance_histogram(const void *rgb, int32_t precision, int32_t width, int32_t height, int64_t *hist_out) {
    if (!rgb || !hist_out) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_image(precision, width, height)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    StagedPlanes<1> st{{plane_in(rgb, 3 * real_bytes(precision))}};
    if (int rc = st.alloc((size_t)width * height, "out of device memory for the image")) return rc;
    if (int rc = st.upload()) return rc;
    return take_hip_luminance_histogram_device(st[0], precision, width, height, hist_out, nullptr);
}

int take_hip_auto_exposure(const int64_t *hist, const TakeExposureOpts *opts, double *exposure_out) {
    if (!hist || !exposure_out) return fail(TAKE_E_INVALID, "null argument");
    ExposureOpts o;
    if (int rc = resolve_exposure(opts, o)) return rc;
    for (int s = 0; s < dp::SLOTS; s++)
        if (hist[s] < 0) return fail(TAKE_E_INVALID, "negative histogram count");
    *exposure_out = auto_exposure(hist, o);
    return TAKE_OK;
}

int take_hip_tonemap_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts, void *d_out,
                            double *exposure_used, void *stream) {
    TonemapOpts o;
    if (int rc = check_tonemap_args(d_rgb, precision, width, height, opts, d_out, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    hipStream_t s = (hipStream_t)stream;
    double E = o.exposure;
    if (!(E > 0)) {
        int64_t hist[dp::SLOTS];
        if (int rc = histogram_on_device(d_rgb, precision, width, height, hist, s)) return rc;
        E = auto_exposure(hist, o.auto_opts);
    }
    const int64_t npix = (int64_t)width * height;
    with_real(precision, [&](auto tag) {
        using R = decltype(tag);
        const dp::Params<R> P{(R)E, (R)(1.0 / (o.white * o.white)), o.op, o.transfer};
        if (o.format == TAKE_DISPLAY_RGBA)
            hipLaunchKernelGGL((dp::k_tonemap<R, true>), pixel_grid(npix), dim3(dp::BLOCK), 0, s, P, (const R *)d_rgb, npix, d_out);
        else
            hipLaunchKernelGGL((dp::k_tonemap<R, false>), pixel_grid(npix), dim3(dp::BLOCK), 0, s, P, (const R *)d_rgb, npix, d_out);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (exposure_used) *exposure_used = E;
    return TAKE_OK;
}

int take_hip_tonemap(const void *rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts, void *out, double *exposure_used) {
    TonemapOpts o;
    if (int rc = check_tonemap_args(rgb, precision, width, height, opts, out, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const bool rgba = o.format == TAKE_DISPLAY_RGBA;
    const size_t real = real_bytes(precision);
    // REAL: rgb, transformed in place; RGBA: rgb, then the codes
    StagedPlanes<2> st{{rgba ? plane_in(rgb, 3 * real) : plane_inout(rgb, out, 3 * real), plane_out(rgba ? out : nullptr, 4)}};
    if (int rc = st.alloc((size_t)width * height, "out of device memory for the display transform's planes")) return rc;
    if (int rc = st.upload()) return rc;
    if (int rc = take_hip_tonemap_device(st[0], precision, width, height, opts, rgba ? st[1] : st[0], exposure_used, nullptr)) return rc;
    return st.download();
}

}  // extern "C"

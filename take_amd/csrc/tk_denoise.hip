// tk_denoise.hip — the C entry points of the image-space denoisers (include/take_hip.h: take_hip_denoise*,
// take_hip_render_denoised*; the variance-guided take_hip_denoise_variance*, take_hip_render_adaptive_denoised*) and the
// only unit that compiles the kernels of tk_denoise.h and tk_denoise_var.h.  The scene-free calls need no scene (as
// take_hip_pack_exr_scanlines does not) and allocate their working images per call; the scene-bound ones render, make
// the feature planes and filter on the device, with planes and working images in the handle's RenderWorkspace — they
// are the three public calls made by hand, through the same functions.  Also the temporal accumulation
// (take_hip_temporal_accumulate*, take_hip_render_temporal*: the kernel of tk_temporal.h), which feeds the same filter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>

#include "take_hip.h"
#include "tk_scene_handle.h"
#include "tk_denoise.h"
#include "tk_denoise_var.h"
#include "tk_temporal.h"

using namespace tk;
using namespace tk_host;

namespace {
// TakeDenoiseOpts with the defaults filled in
struct DenoiseOpts {
    int iterations = 5;
    bool keep_albedo = false;
    double sigma_color = 1.0, sigma_normal = 0.3, sigma_depth = 0.05, albedo_floor = 1e-3;
};
// what needs no device: TAKE_E_INVALID with a message, or TAKE_OK and the resolved options.  sigma_color: its default —
// a radiance for the fixed-sigma filter, a multiple of the pixel's standard deviation for the variance-guided one
constexpr double SIGMA_COLOR = 1.0, SIGMA_COLOR_VARIANCE = 4.0;
int resolve(const TakeDenoiseOpts *o, DenoiseOpts &r, double sigma_color = SIGMA_COLOR) {
    r = DenoiseOpts{};
    r.sigma_color = sigma_color;
    if (!o) return TAKE_OK;
    if (o->iterations > dn::MAX_ITERATIONS) return fail(TAKE_E_INVALID, "iterations must be at most " + std::to_string(dn::MAX_ITERATIONS));
    if (o->flags & ~TAKE_DENOISE_KEEP_ALBEDO) return fail(TAKE_E_INVALID, "unknown flag bits");
    if (!std::isfinite(o->sigma_color) || !std::isfinite(o->sigma_normal) || !std::isfinite(o->sigma_depth) || !std::isfinite(o->albedo_floor))
        return fail(TAKE_E_INVALID, "sigma_color, sigma_normal, sigma_depth and albedo_floor must be finite");
    if (o->iterations > 0) r.iterations = o->iterations;
    r.keep_albedo = (o->flags & TAKE_DENOISE_KEEP_ALBEDO) != 0;
    if (o->sigma_color > 0) r.sigma_color = o->sigma_color;
    if (o->sigma_normal > 0) r.sigma_normal = o->sigma_normal;
    if (o->sigma_depth > 0) r.sigma_depth = o->sigma_depth;
    if (o->albedo_floor > 0) r.albedo_floor = o->albedo_floor;
    return TAKE_OK;
}
int check_image(int32_t precision, int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return fail(TAKE_E_INVALID, "width and height must be positive");
    if (precision != TAKE_PRECISION_F32 && precision != TAKE_PRECISION_F64) return fail(TAKE_E_INVALID, "unknown precision");
    return TAKE_OK;
}

// Reals of working images per pixel: colour, colour, guide records
constexpr int WORK_REALS = 12;

// Prologue, the levels, the epilogue fused into the last: enqueued on `stream`, no synchronisation.  work: WORK_REALS *
// width * height Reals, aligned for Rec4<R>.  out may be rgb (the prologue has read rgb before the last level writes).
template <class R>
int denoise_enqueue(const R *rgb, const R *albedo, const R *normal, const R *depth, int32_t width, int32_t height, const DenoiseOpts &o, R *work, R *out,
                    hipStream_t stream) {
    const int64_t npix = (int64_t)width * height;
    dn::Params<R> P{};
    P.width = width, P.height = height;
    P.guides = (normal ? dn::HAS_NORMAL : 0) | (depth ? dn::HAS_DEPTH : 0) | (albedo && !o.keep_albedo ? dn::DEMODULATE : 0);
    P.inv_n = (R)(1.0 / (o.sigma_normal * o.sigma_normal)), P.inv_d = (R)(1.0 / (o.sigma_depth * o.sigma_depth));
    P.albedo_floor = (R)o.albedo_floor;
    dn::Rec4<R> *colour[2] = {(dn::Rec4<R> *)work, (dn::Rec4<R> *)work + npix}, *guide = (dn::Rec4<R> *)work + 2 * npix;
    const dim3 pack_grid((unsigned)std::min<int64_t>((npix + 255) / 256, 2048));
    hipLaunchKernelGGL((dn::k_denoise_pack<R>), pack_grid, dim3(256), 0, stream, P, rgb, albedo, normal, depth, colour[0], guide);
    const dim3 grid((unsigned)((width + dn::DN_BX - 1) / dn::DN_BX), (unsigned)std::min((height + dn::DN_BY - 1) / dn::DN_BY, 65535)), block(dn::DN_BX, dn::DN_BY);
    for (int i = 0; i < o.iterations; i++) {
        const R inv_c = (R)(std::ldexp(1.0, 2 * i) / (o.sigma_color * o.sigma_color));  // the colour sigma halves every level
        if (i == o.iterations - 1)
            hipLaunchKernelGGL((dn::k_denoise_level<R, true>), grid, block, 0, stream, P, colour[i & 1], guide, 1 << i, inv_c, (dn::Rec4<R> *)nullptr, albedo, out);
        else
            hipLaunchKernelGGL((dn::k_denoise_level<R, false>), grid, block, 0, stream, P, colour[i & 1], guide, 1 << i, inv_c, colour[(i + 1) & 1], albedo, (R *)nullptr);
    }
    HIP_TRY(hipGetLastError());
    return TAKE_OK;
}
int denoise_enqueue_any(int32_t precision, const void *rgb, const TakeFeatureBuffers *g, int32_t width, int32_t height, const DenoiseOpts &o, void *work,
                        void *out, hipStream_t stream) {
    const void *albedo = g ? g->albedo : nullptr, *normal = g ? g->normal : nullptr, *depth = g ? g->depth : nullptr;
    if (precision == TAKE_PRECISION_F64)
        return denoise_enqueue((const double *)rgb, (const double *)albedo, (const double *)normal, (const double *)depth, width, height, o, (double *)work, (double *)out, stream);
    return denoise_enqueue((const float *)rgb, (const float *)albedo, (const float *)normal, (const float *)depth, width, height, o, (float *)work, (float *)out, stream);
}

// The variance-guided filter (tk_denoise_var.h): the same shape of launches.  count / m1 / m2: the planes of
// TakeAdaptiveStats; variance_out may be null.  o.sigma_color is a multiple of the pixel's standard deviation.
template <class R>
int denoise_var_enqueue(const R *rgb, const R *albedo, const R *normal, const R *depth, const TakeAdaptiveStats &s, int32_t width, int32_t height,
                        const DenoiseOpts &o, R *work, R *out, R *variance_out, hipStream_t stream) {
    const int64_t npix = (int64_t)width * height;
    dn::Params<R> P{};
    P.width = width, P.height = height;
    P.guides = (normal ? dn::HAS_NORMAL : 0) | (depth ? dn::HAS_DEPTH : 0) | (albedo && !o.keep_albedo ? dn::DEMODULATE : 0);
    P.inv_n = (R)(1.0 / (o.sigma_normal * o.sigma_normal)), P.inv_d = (R)(1.0 / (o.sigma_depth * o.sigma_depth));
    P.albedo_floor = (R)o.albedo_floor;
    const R sl2 = (R)(o.sigma_color * o.sigma_color);
    dn::Rec4<R> *colour[2] = {(dn::Rec4<R> *)work, (dn::Rec4<R> *)work + npix}, *guide = (dn::Rec4<R> *)work + 2 * npix;
    const dim3 pack_grid((unsigned)std::min<int64_t>((npix + 255) / 256, 2048));
    hipLaunchKernelGGL((dn::k_denoise_var_pack<R>), pack_grid, dim3(256), 0, stream, P, rgb, albedo, normal, depth, (const int32_t *)s.count, (const double *)s.m1,
                       (const double *)s.m2, colour[0], guide);
    const dim3 grid((unsigned)((width + dn::DN_BX - 1) / dn::DN_BX), (unsigned)std::min((height + dn::DN_BY - 1) / dn::DN_BY, 65535)), block(dn::DN_BX, dn::DN_BY);
    for (int i = 0; i < o.iterations; i++) {
        if (i == o.iterations - 1)
            hipLaunchKernelGGL((dn::k_denoise_var_level<R, true>), grid, block, 0, stream, P, colour[i & 1], guide, 1 << i, sl2, (dn::Rec4<R> *)nullptr, albedo, out, variance_out);
        else
            hipLaunchKernelGGL((dn::k_denoise_var_level<R, false>), grid, block, 0, stream, P, colour[i & 1], guide, 1 << i, sl2, colour[(i + 1) & 1], albedo, (R *)nullptr,
                               (R *)nullptr);
    }
    HIP_TRY(hipGetLastError());
    return TAKE_OK;
}
// what the scene-free variance-guided calls refuse, before a device is looked for
int check_variance_args(const void *rgb, const TakeAdaptiveStats *stats, const void *out, int32_t precision, int32_t width, int32_t height,
                        const TakeDenoiseOpts *opts, DenoiseOpts &o) {
    if (!rgb || !out || !stats || !stats->count || !stats->m1 || !stats->m2) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_image(precision, width, height)) return rc;
    return resolve(opts, o, SIGMA_COLOR_VARIANCE);
}
// what the scene-bound variance-guided calls refuse, before a device is looked for: the adaptive part's, then the denoiser's
int check_adaptive_denoised_args(const TakeScene *ts, const TakeRenderOpts *ropts, const TakeAdaptiveOpts *aopts, const TakeDenoiseOpts *dopts, const void *out,
                                 DenoiseOpts &o) {
    if (!ts || !ropts || !out) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_adaptive_opts(aopts)) return rc;
    return resolve(dopts, o, SIGMA_COLOR_VARIANCE);
}

// ---- temporal accumulation (tk_temporal.h)
// TakeTemporalOpts with the defaults filled in
struct TemporalOpts {
    int max_history = 64;
    double depth_tol = 0.05;
};
int resolve_temporal(const TakeTemporalOpts *o, TemporalOpts &r) {
    r = TemporalOpts{};
    if (!o) return TAKE_OK;
    if (o->flags != 0) return fail(TAKE_E_INVALID, "unknown flag bits");
    if (!std::isfinite(o->depth_tol)) return fail(TAKE_E_INVALID, "depth_tol must be finite");
    if (o->max_history > 0) r.max_history = o->max_history;
    if (o->depth_tol > 0) r.depth_tol = o->depth_tol;
    return TAKE_OK;
}
// what the scene-free calls refuse, before a device is looked for
int check_temporal_args(const TakeTemporalFrame *cur, const TakeTemporalFrame *hist, const void *prev_xy, int32_t precision, int32_t width, int32_t height,
                        const TakeTemporalOpts *opts, const TakeTemporalFrame *out, TemporalOpts &o) {
    if (!cur || !out || !prev_xy || !cur->rgb || !cur->count || !cur->m1 || !cur->m2 || !out->rgb || !out->count || !out->m1 || !out->m2)
        return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_image(precision, width, height)) return rc;
    if (int rc = resolve_temporal(opts, o)) return rc;
    if (hist && (!hist->rgb || !hist->count || !hist->m1 || !hist->m2)) return fail(TAKE_E_INVALID, "incomplete history: rgb, count, m1 and m2 are all required");
    return TAKE_OK;
}
template <class R> tp::Frame<R> typed(const TakeTemporalFrame &f) { return {(R *)f.rgb, f.count, f.m1, f.m2, (R *)f.depth, f.shape_id}; }
// One launch, enqueued on `stream`, no synchronisation.  hist: null = none (the output is the current frame).
template <class R>
int temporal_enqueue(const tp::Frame<R> &cur, const tp::Frame<R> *hist, const R *prev_xy, const R *prev_depth, int32_t width, int32_t height, const TemporalOpts &o,
                     const tp::Frame<R> &out, hipStream_t stream) {
    tp::Params<R> P{};
    P.width = width, P.height = height, P.max_history = o.max_history, P.has_history = hist ? 1 : 0, P.depth_tol = (R)o.depth_tol;
    const dim3 grid((unsigned)((width + tp::TP_BX - 1) / tp::TP_BX), (unsigned)std::min((height + tp::TP_BY - 1) / tp::TP_BY, 65535)), block(tp::TP_BX, tp::TP_BY);
    hipLaunchKernelGGL((tp::k_temporal_accumulate<R>), grid, block, 0, stream, P, cur, hist ? *hist : tp::Frame<R>{}, prev_xy, prev_depth, out);
    HIP_TRY(hipGetLastError());
    return TAKE_OK;
}

// take_hip_render_temporal*: a frame in one of the handle's buffers — m1, m2, then rgb and depth, then count and
// shape_id (every plane aligned for its type whatever the pixel count); the current frame's buffer goes on with prev_xy
// and prev_depth
template <class R> constexpr int64_t temporal_frame_bytes() { return 16 + 4 * (int64_t)sizeof(R) + 8; }
template <class R> tp::Frame<R> frame_at(double *base, int64_t npix) {
    double *m1 = base, *m2 = m1 + npix;
    R *rgb = (R *)(m2 + npix), *depth = rgb + 3 * npix;
    int32_t *count = (int32_t *)(depth + npix), *shape_id = count + npix;
    return {rgb, count, m1, m2, depth, shape_id};
}
// what the scene-bound temporal calls refuse, before a device is looked for: the adaptive part's, the temporal part's, the denoiser's
int check_render_temporal_args(const TakeScene *ts, const TakeRenderOpts *ropts, const TakeAdaptiveOpts *aopts, const TakeTemporalOpts *topts,
                               const TakeDenoiseOpts *dopts, const void *out, TemporalOpts &t, DenoiseOpts &o) {
    if (!ts || !ropts || !out) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_adaptive_opts(aopts)) return rc;
    if (int rc = resolve_temporal(topts, t)) return rc;
    return resolve(dopts, o, SIGMA_COLOR_VARIANCE);
}
}  // namespace

extern "C" {

int take_hip_denoise_device(const void *d_rgb, const TakeFeatureBuffers *d_guides, int32_t precision, int32_t width, int32_t height,
                            const TakeDenoiseOpts *opts, void *d_out, void *stream) {
    if (!d_rgb || !d_out) return fail(TAKE_E_INVALID, "null argument");
    DenoiseOpts o;
    if (int rc = check_image(precision, width, height)) return rc;
    if (int rc = resolve(opts, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const size_t real = precision == TAKE_PRECISION_F64 ? 8 : 4;
    DevBuf<char> work;
    if (work.alloc((size_t)width * height * WORK_REALS * real) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the denoiser's working images");
    if (int rc = denoise_enqueue_any(precision, d_rgb, d_guides, width, height, o, work.p, d_out, (hipStream_t)stream)) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return TAKE_OK;
}

int take_hip_denoise(const void *rgb, const TakeFeatureBuffers *guides, int32_t precision, int32_t width, int32_t height, const TakeDenoiseOpts *opts,
                     void *out) {
    if (!rgb || !out) return fail(TAKE_E_INVALID, "null argument");
    DenoiseOpts o;
    if (int rc = check_image(precision, width, height)) return rc;
    if (int rc = resolve(opts, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const size_t real = precision == TAKE_PRECISION_F64 ? 8 : 4, npix = (size_t)width * height;
    // rgb (filtered in place), then the guides that were given: (host pointer, Reals per pixel)
    const std::pair<const void *, size_t> planes[4] = {{rgb, 3}, {guides ? guides->albedo : nullptr, 3}, {guides ? guides->normal : nullptr, 3}, {guides ? guides->depth : nullptr, 1}};
    DevBuf<char> d_plane[4];
    for (int k = 0; k < 4; k++) {
        if (!planes[k].first) continue;
        if (d_plane[k].alloc(npix * planes[k].second * real) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the denoiser's planes");
        HIP_TRY(hipMemcpy(d_plane[k].p, planes[k].first, d_plane[k].bytes(), hipMemcpyHostToDevice));
    }
    const TakeFeatureBuffers d_guides{d_plane[1].p, d_plane[2].p, d_plane[3].p, nullptr, nullptr, nullptr};
    if (int rc = take_hip_denoise_device(d_plane[0].p, &d_guides, precision, width, height, opts, d_plane[0].p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_plane[0].p, d_plane[0].bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_render_denoised_device(TakeScene *ts, const TakeRenderOpts *ropts, const TakeDenoiseOpts *dopts, void *d_out, void *stream) {
    if (!ts || !ropts || !d_out) return fail(TAKE_E_INVALID, "null argument");
    DenoiseOpts o;
    if (int rc = resolve(dopts, o)) return rc;
    TAKE_ON_DEVICE(ts);
    TakeRenderOpts ro = *ropts;
    ro.strip_first = 0, ro.strip_stride = 1;  // the whole image, as take_hip_render_exr_scanlines
    const int W = ts->width(), H = ts->height();
    const int64_t npix = (int64_t)W * H;
    return on_primary(ts, [&](auto &sc, auto &work) {
        using R = std::remove_reference_t<decltype(*work.accum.p)>;
        // the working images, then albedo, normal and depth
        if (int rc = work.ensure_denoise((WORK_REALS + 7) * npix)) return rc;
        R *albedo = work.denoise.p + WORK_REALS * npix, *normal = albedo + 3 * npix, *depth = normal + 3 * npix;
        if (int rc = render_scene(ts, ro, d_out, (hipStream_t)stream)) return rc;
        const TakeFeatureBuffers planes{albedo, normal, depth, nullptr, nullptr, nullptr};
        if (int rc = render_features_scene(ts, ro, planes, (hipStream_t)stream)) return rc;
        if (int rc = denoise_enqueue((const R *)d_out, (const R *)albedo, (const R *)normal, (const R *)depth, W, H, o, work.denoise.p, (R *)d_out, (hipStream_t)stream)) return rc;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return (int)TAKE_OK;
    });
}

int take_hip_render_denoised(TakeScene *ts, const TakeRenderOpts *ropts, const TakeDenoiseOpts *dopts, void *rgb_out_host) {
    if (!ts || !ropts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    DenoiseOpts o;
    if (int rc = resolve(dopts, o)) return rc;
    TAKE_ON_DEVICE(ts);
    DevBuf<char> d_out;
    if (d_out.alloc((size_t)ts->width() * ts->height() * 3 * (ts->f64() ? 8 : 4)) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the denoised image");
    if (int rc = take_hip_render_denoised_device(ts, ropts, dopts, d_out.p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(rgb_out_host, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_denoise_variance_device(const void *d_rgb, const TakeFeatureBuffers *d_guides, const TakeAdaptiveStats *d_stats, int32_t precision, int32_t width,
                                     int32_t height, const TakeDenoiseOpts *opts, void *d_out, void *d_variance_out, void *stream) {
    DenoiseOpts o;
    if (int rc = check_variance_args(d_rgb, d_stats, d_out, precision, width, height, opts, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const size_t real = precision == TAKE_PRECISION_F64 ? 8 : 4;
    DevBuf<char> work;
    if (work.alloc((size_t)width * height * WORK_REALS * real) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the denoiser's working images");
    const void *albedo = d_guides ? d_guides->albedo : nullptr, *normal = d_guides ? d_guides->normal : nullptr, *depth = d_guides ? d_guides->depth : nullptr;
    int rc;
    if (precision == TAKE_PRECISION_F64)
        rc = denoise_var_enqueue((const double *)d_rgb, (const double *)albedo, (const double *)normal, (const double *)depth, *d_stats, width, height, o, (double *)work.p,
                                 (double *)d_out, (double *)d_variance_out, (hipStream_t)stream);
    else
        rc = denoise_var_enqueue((const float *)d_rgb, (const float *)albedo, (const float *)normal, (const float *)depth, *d_stats, width, height, o, (float *)work.p,
                                 (float *)d_out, (float *)d_variance_out, (hipStream_t)stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return TAKE_OK;
}

int take_hip_denoise_variance(const void *rgb, const TakeFeatureBuffers *guides, const TakeAdaptiveStats *stats, int32_t precision, int32_t width, int32_t height,
                              const TakeDenoiseOpts *opts, void *out, void *variance_out) {
    DenoiseOpts o;
    if (int rc = check_variance_args(rgb, stats, out, precision, width, height, opts, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const size_t real = precision == TAKE_PRECISION_F64 ? 8 : 4, npix = (size_t)width * height;
    // rgb (filtered in place), the guides that were given, the three statistics planes: (host pointer, bytes per pixel);
    // then the variance plane, if wanted
    const std::pair<const void *, size_t> planes[7] = {{rgb, 3 * real}, {guides ? guides->albedo : nullptr, 3 * real}, {guides ? guides->normal : nullptr, 3 * real},
                                                       {guides ? guides->depth : nullptr, real}, {stats->count, 4}, {stats->m1, 8}, {stats->m2, 8}};
    DevBuf<char> d_plane[7], d_variance;
    for (int k = 0; k < 7; k++) {
        if (!planes[k].first) continue;
        if (d_plane[k].alloc(npix * planes[k].second) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the denoiser's planes");
        HIP_TRY(hipMemcpy(d_plane[k].p, planes[k].first, d_plane[k].bytes(), hipMemcpyHostToDevice));
    }
    if (variance_out && d_variance.alloc(npix * real) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the denoiser's planes");
    const TakeFeatureBuffers d_guides{d_plane[1].p, d_plane[2].p, d_plane[3].p, nullptr, nullptr, nullptr};
    const TakeAdaptiveStats d_stats{(int32_t *)d_plane[4].p, (double *)d_plane[5].p, (double *)d_plane[6].p};
    if (int rc = take_hip_denoise_variance_device(d_plane[0].p, &d_guides, &d_stats, precision, width, height, opts, d_plane[0].p, d_variance.p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_plane[0].p, d_plane[0].bytes(), hipMemcpyDeviceToHost));
    if (variance_out) HIP_TRY(hipMemcpy(variance_out, d_variance.p, d_variance.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_render_adaptive_denoised_device(TakeScene *ts, const TakeRenderOpts *ropts, const TakeAdaptiveOpts *aopts, const TakeDenoiseOpts *dopts, void *d_out,
                                             const TakeAdaptiveStats *d_stats, void *d_variance_out, void *stream) {
    DenoiseOpts o;
    if (int rc = check_adaptive_denoised_args(ts, ropts, aopts, dopts, d_out, o)) return rc;
    TAKE_ON_DEVICE(ts);
    TakeRenderOpts ro = *ropts;
    ro.strip_first = 0, ro.strip_stride = 1;  // the whole image, as take_hip_render_denoised_device
    const int W = ts->width(), H = ts->height();
    const int64_t npix = (int64_t)W * H;
    return on_primary(ts, [&](auto &sc, auto &work) {
        using R = std::remove_reference_t<decltype(*work.accum.p)>;
        // the working images, then albedo, normal and depth, then — from the next multiple of 8 bytes on — the statistics
        // planes the caller did not ask for: m1, m2, count
        const int64_t real_planes = (WORK_REALS + 7) * npix, stats_at = (real_planes * (int64_t)sizeof(R) + 7) / 8 * 8;
        if (int rc = work.ensure_denoise((stats_at + 20 * npix + (int64_t)sizeof(R) - 1) / (int64_t)sizeof(R))) return rc;
        R *albedo = work.denoise.p + WORK_REALS * npix, *normal = albedo + 3 * npix, *depth = normal + 3 * npix;
        double *own_m1 = (double *)((char *)work.denoise.p + stats_at), *own_m2 = own_m1 + npix;
        TakeAdaptiveStats stats{(int32_t *)(own_m2 + npix), own_m1, own_m2};
        if (d_stats && d_stats->count) stats.count = d_stats->count;
        if (d_stats && d_stats->m1) stats.m1 = d_stats->m1;
        if (d_stats && d_stats->m2) stats.m2 = d_stats->m2;
        if (int rc = render_adaptive_scene(ts, ro, aopts, d_out, stats, (hipStream_t)stream)) return rc;
        TakeRenderOpts fo = ro;
        fo.spp = adaptive_min_spp(ro, aopts);  // the samples every pixel has: the guide pass does not grow with the maximum
        const TakeFeatureBuffers planes{albedo, normal, depth, nullptr, nullptr, nullptr};
        if (int rc = render_features_scene(ts, fo, planes, (hipStream_t)stream)) return rc;
        if (int rc = denoise_var_enqueue((const R *)d_out, (const R *)albedo, (const R *)normal, (const R *)depth, stats, W, H, o, work.denoise.p, (R *)d_out,
                                         (R *)d_variance_out, (hipStream_t)stream))
            return rc;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return (int)TAKE_OK;
    });
}

int take_hip_render_adaptive_denoised(TakeScene *ts, const TakeRenderOpts *ropts, const TakeAdaptiveOpts *aopts, const TakeDenoiseOpts *dopts, void *rgb_out_host,
                                      const TakeAdaptiveStats *host_stats, void *variance_out_host) {
    DenoiseOpts o;
    if (int rc = check_adaptive_denoised_args(ts, ropts, aopts, dopts, rgb_out_host, o)) return rc;
    TAKE_ON_DEVICE(ts);
    const size_t npix = (size_t)ts->width() * ts->height(), real = ts->f64() ? 8 : 4;
    // the image and the wanted planes in device memory, then copied out: (host pointer, bytes per pixel)
    const std::pair<void *, size_t> planes[5] = {{rgb_out_host, 3 * real}, {host_stats ? host_stats->count : nullptr, 4}, {host_stats ? host_stats->m1 : nullptr, 8},
                                                 {host_stats ? host_stats->m2 : nullptr, 8}, {variance_out_host, real}};
    DevBuf<char> d_plane[5];
    for (int k = 0; k < 5; k++)
        if (planes[k].first && d_plane[k].alloc(npix * planes[k].second) != hipSuccess)
            return fail(TAKE_E_NOMEM, "out of device memory for the denoised adaptive render's planes");
    const TakeAdaptiveStats d_stats{(int32_t *)d_plane[1].p, (double *)d_plane[2].p, (double *)d_plane[3].p};
    if (int rc = take_hip_render_adaptive_denoised_device(ts, ropts, aopts, dopts, d_plane[0].p, &d_stats, d_plane[4].p, nullptr)) return rc;
    for (int k = 0; k < 5; k++)
        if (d_plane[k].p) HIP_TRY(hipMemcpy(planes[k].first, d_plane[k].p, d_plane[k].bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_temporal_accumulate_device(const TakeTemporalFrame *d_cur, const TakeTemporalFrame *d_hist, const void *d_prev_xy, const void *d_prev_depth,
                                        int32_t precision, int32_t width, int32_t height, const TakeTemporalOpts *opts, const TakeTemporalFrame *d_out, void *stream) {
    TemporalOpts o;
    if (int rc = check_temporal_args(d_cur, d_hist, d_prev_xy, precision, width, height, opts, d_out, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    int rc;
    if (precision == TAKE_PRECISION_F64) {
        const tp::Frame<double> hist = d_hist ? typed<double>(*d_hist) : tp::Frame<double>{};
        rc = temporal_enqueue(typed<double>(*d_cur), d_hist ? &hist : nullptr, (const double *)d_prev_xy, (const double *)d_prev_depth, width, height, o,
                              typed<double>(*d_out), (hipStream_t)stream);
    } else {
        const tp::Frame<float> hist = d_hist ? typed<float>(*d_hist) : tp::Frame<float>{};
        rc = temporal_enqueue(typed<float>(*d_cur), d_hist ? &hist : nullptr, (const float *)d_prev_xy, (const float *)d_prev_depth, width, height, o,
                              typed<float>(*d_out), (hipStream_t)stream);
    }
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return TAKE_OK;
}

int take_hip_temporal_accumulate(const TakeTemporalFrame *cur, const TakeTemporalFrame *hist, const void *prev_xy, const void *prev_depth, int32_t precision,
                                 int32_t width, int32_t height, const TakeTemporalOpts *opts, const TakeTemporalFrame *out) {
    TemporalOpts o;
    if (int rc = check_temporal_args(cur, hist, prev_xy, precision, width, height, opts, out, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const size_t real = precision == TAKE_PRECISION_F64 ? 8 : 4, npix = (size_t)width * height;
    // the planes of a frame: bytes per pixel, in the order of TakeTemporalFrame's members
    const size_t per_pixel[6] = {3 * real, 4, 8, 8, real, 4};
    auto members = [](const TakeTemporalFrame &f, void *m[6]) { m[0] = f.rgb, m[1] = f.count, m[2] = f.m1, m[3] = f.m2, m[4] = f.depth, m[5] = f.shape_id; };
    // the current frame (accumulated in place) and the history, uploaded; then the motion planes
    DevBuf<char> d_cur[6], d_hist[6], d_xy, d_pd;
    void *h_cur[6], *h_hist[6] = {}, *h_out[6];
    members(*cur, h_cur), members(*out, h_out);
    if (hist) members(*hist, h_hist);
    for (int k = 0; k < 6; k++)
        for (int which = 0; which < 2; which++) {
            const void *src = which ? h_hist[k] : h_cur[k];
            DevBuf<char> &dst = which ? d_hist[k] : d_cur[k];
            if (!src) continue;
            if (dst.alloc(npix * per_pixel[k]) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the temporal accumulation's planes");
            HIP_TRY(hipMemcpy(dst.p, src, dst.bytes(), hipMemcpyHostToDevice));
        }
    if (d_xy.alloc(npix * 2 * real) != hipSuccess || (prev_depth && d_pd.alloc(npix * real) != hipSuccess))
        return fail(TAKE_E_NOMEM, "out of device memory for the temporal accumulation's planes");
    HIP_TRY(hipMemcpy(d_xy.p, prev_xy, d_xy.bytes(), hipMemcpyHostToDevice));
    if (prev_depth) HIP_TRY(hipMemcpy(d_pd.p, prev_depth, d_pd.bytes(), hipMemcpyHostToDevice));
    const TakeTemporalFrame dc{d_cur[0].p, (int32_t *)d_cur[1].p, (double *)d_cur[2].p, (double *)d_cur[3].p, d_cur[4].p, (int32_t *)d_cur[5].p};
    const TakeTemporalFrame dh{d_hist[0].p, (int32_t *)d_hist[1].p, (double *)d_hist[2].p, (double *)d_hist[3].p, d_hist[4].p, (int32_t *)d_hist[5].p};
    if (int rc = take_hip_temporal_accumulate_device(&dc, hist ? &dh : nullptr, d_xy.p, d_pd.p, precision, width, height, opts, &dc, nullptr)) return rc;
    for (int k = 0; k < 6; k++)
        if (h_out[k] && d_cur[k].p) HIP_TRY(hipMemcpy(h_out[k], d_cur[k].p, d_cur[k].bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_render_temporal_device(TakeScene *ts, const TakeRenderOpts *ropts, const TakeAdaptiveOpts *aopts, const TakeTemporalOpts *topts,
                                    const TakeDenoiseOpts *dopts, int32_t restart, void *d_out, void *stream) {
    TemporalOpts t;
    DenoiseOpts o;
    if (int rc = check_render_temporal_args(ts, ropts, aopts, topts, dopts, d_out, t, o)) return rc;
    TAKE_ON_DEVICE(ts);
    TakeRenderOpts ro = *ropts;
    ro.strip_first = 0, ro.strip_stride = 1;  // the whole image, as take_hip_render_denoised_device
    const int W = ts->width(), H = ts->height();
    const int64_t npix = (int64_t)W * H;
    const int rc = on_primary(ts, [&](auto &sc, auto &work) {
        using R = std::remove_reference_t<decltype(*work.accum.p)>;
        hipStream_t s = (hipStream_t)stream;
        // the two accumulated frames and the current one with its motion planes (allocated once: the pixel count is the
        // scene's), the filter's working images with albedo, normal and depth behind them
        const size_t frame_doubles = (size_t)(temporal_frame_bytes<R>() * npix + 7) / 8, cur_doubles = (size_t)((temporal_frame_bytes<R>() + 3 * (int64_t)sizeof(R)) * npix + 7) / 8;
        for (auto *b : {&work.temporal[0], &work.temporal[1]})
            if (b->n < frame_doubles) {
                ts->temporal_history = -1;  // (never taken: the buffers are sized by the first call)
                if (b->alloc(frame_doubles) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the accumulated frames");
            }
        if (work.temporal_cur.n < cur_doubles && work.temporal_cur.alloc(cur_doubles) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the accumulated frames");
        if (int rc = work.ensure_denoise((WORK_REALS + 7) * npix)) return rc;
        R *albedo = work.denoise.p + WORK_REALS * npix, *normal = albedo + 3 * npix, *depth = normal + 3 * npix;
        const tp::Frame<R> cur = frame_at<R>(work.temporal_cur.p, npix);
        R *prev_xy = (R *)(cur.shape_id + npix), *prev_depth = prev_xy + 2 * npix;
        // 1. the frame
        if (int rc = render_adaptive_scene(ts, ro, aopts, cur.rgb, TakeAdaptiveStats{cur.count, cur.m1, cur.m2}, s)) return rc;
        // 2. onto the history, through the motion pass (without one: depth and ids only, against the frame itself)
        const bool have = restart == 0 && ts->temporal_history >= 0 && ts->mark.set;
        const int into = have ? 1 - ts->temporal_history : 0;
        const tp::Frame<R> acc = frame_at<R>(work.temporal[into].p, npix);
        const TakeMotionBuffers motion{have ? prev_xy : nullptr, have ? prev_depth : nullptr, cur.depth, cur.shape_id};
        if (int rc = render_motion_scene(ts, ro, motion, have, s)) return rc;
        if (have) {
            const tp::Frame<R> hist = frame_at<R>(work.temporal[ts->temporal_history].p, npix);
            if (int rc = temporal_enqueue(cur, &hist, (const R *)prev_xy, (const R *)prev_depth, W, H, t, acc, s)) return rc;
        } else {
            HIP_TRY(hipMemcpyAsync(work.temporal[into].p, work.temporal_cur.p, (size_t)(temporal_frame_bytes<R>() * npix), hipMemcpyDeviceToDevice, s));
        }
        // 3. the result is the history from here on
        ts->temporal_history = into;
        // 4. the guides, and the filter on the accumulated image with the accumulated statistics
        TakeRenderOpts fo = ro;
        fo.spp = adaptive_min_spp(ro, aopts);
        const TakeFeatureBuffers planes{albedo, normal, depth, nullptr, nullptr, nullptr};
        if (int rc = render_features_scene(ts, fo, planes, s)) return rc;
        if (int rc = denoise_var_enqueue((const R *)acc.rgb, (const R *)albedo, (const R *)normal, (const R *)depth, TakeAdaptiveStats{acc.count, acc.m1, acc.m2}, W, H, o,
                                         work.denoise.p, (R *)d_out, (R *)nullptr, s))
            return rc;
        HIP_TRY(hipStreamSynchronize(s));
        return (int)TAKE_OK;
    });
    // 5. this frame is the next one's previous frame
    return rc ? rc : take_hip_scene_mark_frame(ts);
}

int take_hip_render_temporal(TakeScene *ts, const TakeRenderOpts *ropts, const TakeAdaptiveOpts *aopts, const TakeTemporalOpts *topts, const TakeDenoiseOpts *dopts,
                             int32_t restart, void *rgb_out_host) {
    TemporalOpts t;
    DenoiseOpts o;
    if (int rc = check_render_temporal_args(ts, ropts, aopts, topts, dopts, rgb_out_host, t, o)) return rc;
    TAKE_ON_DEVICE(ts);
    DevBuf<char> d_out;
    if (d_out.alloc((size_t)ts->width() * ts->height() * 3 * (ts->f64() ? 8 : 4)) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the filtered frame");
    if (int rc = take_hip_render_temporal_device(ts, ropts, aopts, topts, dopts, restart, d_out.p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(rgb_out_host, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

}  // extern "C"

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
// Reals of working images per pixel: colour, colour, guide records
constexpr int WORK_REALS = 12;

// the guide planes of a TakeFeatureBuffers (null: none were given) for Reals of precision R; each may be null
template <class R> struct Guides {
    R *albedo, *normal, *depth;
};
template <class R> Guides<R> typed(const TakeFeatureBuffers *g) { return g ? Guides<R>{(R *)g->albedo, (R *)g->normal, (R *)g->depth} : Guides<R>{}; }

// The launches both filters share — prologue, the levels, the epilogue fused into the last: enqueued on `stream`, no
// synchronisation.  work: WORK_REALS * width * height Reals, aligned for Rec4<R>.  pack(grid, block, P, colour, guide)
// launches the prologue, level(last, grid, block, P, i, src, guide, dst) level i from src to dst; last: std::true_type
// for the level that is the epilogue (dst is null: it writes the caller's planes), std::false_type before.
template <class R, class Pack, class Level>
int filter_enqueue(const Guides<R> &g, int32_t width, int32_t height, const DenoiseOpts &o, R *work, Pack &&pack, Level &&level) {
    const int64_t npix = (int64_t)width * height;
    dn::Params<R> P{};
    P.width = width, P.height = height;
    P.guides = (g.normal ? dn::HAS_NORMAL : 0) | (g.depth ? dn::HAS_DEPTH : 0) | (g.albedo && !o.keep_albedo ? dn::DEMODULATE : 0);
    P.inv_n = (R)(1.0 / (o.sigma_normal * o.sigma_normal)), P.inv_d = (R)(1.0 / (o.sigma_depth * o.sigma_depth));
    P.albedo_floor = (R)o.albedo_floor;
    dn::Rec4<R> *colour[2] = {(dn::Rec4<R> *)work, (dn::Rec4<R> *)work + npix}, *guide = (dn::Rec4<R> *)work + 2 * npix;
    pack(dim3((unsigned)std::min<int64_t>((npix + 255) / 256, 2048)), dim3(256), P, colour[0], guide);
    const dim3 grid((unsigned)((width + dn::DN_BX - 1) / dn::DN_BX), (unsigned)std::min((height + dn::DN_BY - 1) / dn::DN_BY, 65535)), block(dn::DN_BX, dn::DN_BY);
    for (int i = 0; i < o.iterations; i++) {
        if (i == o.iterations - 1)
            level(std::true_type{}, grid, block, P, i, colour[i & 1], guide, (dn::Rec4<R> *)nullptr);
        else
            level(std::false_type{}, grid, block, P, i, colour[i & 1], guide, colour[(i + 1) & 1]);
    }
    HIP_TRY(hipGetLastError());
    return TAKE_OK;
}

// The fixed-sigma filter (tk_denoise.h).  out may be rgb (the prologue has read rgb before the last level writes).
template <class R>
int denoise_enqueue(const R *rgb, const Guides<R> &g, int32_t width, int32_t height, const DenoiseOpts &o, R *work, R *out, hipStream_t stream) {
    return filter_enqueue(
        g, width, height, o, work,
        [&](dim3 grid, dim3 block, const dn::Params<R> &P, dn::Rec4<R> *colour, dn::Rec4<R> *guide) {
            hipLaunchKernelGGL((dn::k_denoise_pack<R>), grid, block, 0, stream, P, rgb, g.albedo, g.normal, g.depth, colour, guide);
        },
        [&](auto last, dim3 grid, dim3 block, const dn::Params<R> &P, int i, dn::Rec4<R> *src, dn::Rec4<R> *guide, dn::Rec4<R> *dst) {
            const R inv_c = (R)(std::ldexp(1.0, 2 * i) / (o.sigma_color * o.sigma_color));  // the colour sigma halves every level
            hipLaunchKernelGGL((dn::k_denoise_level<R, decltype(last)::value>), grid, block, 0, stream, P, src, guide, 1 << i, inv_c, dst, g.albedo, last ? out : (R *)nullptr);
        });
}

// The variance-guided filter (tk_denoise_var.h).  s: the planes of TakeAdaptiveStats; variance_out may be null.
// o.sigma_color is a multiple of the pixel's standard deviation.
template <class R>
int denoise_var_enqueue(const R *rgb, const Guides<R> &g, const TakeAdaptiveStats &s, int32_t width, int32_t height, const DenoiseOpts &o, R *work, R *out,
                        R *variance_out, hipStream_t stream) {
    const R sl2 = (R)(o.sigma_color * o.sigma_color);
    return filter_enqueue(
        g, width, height, o, work,
        [&](dim3 grid, dim3 block, const dn::Params<R> &P, dn::Rec4<R> *colour, dn::Rec4<R> *guide) {
            hipLaunchKernelGGL((dn::k_denoise_var_pack<R>), grid, block, 0, stream, P, rgb, g.albedo, g.normal, g.depth, s.count, s.m1, s.m2, colour, guide);
        },
        [&](auto last, dim3 grid, dim3 block, const dn::Params<R> &P, int i, dn::Rec4<R> *src, dn::Rec4<R> *guide, dn::Rec4<R> *dst) {
            hipLaunchKernelGGL((dn::k_denoise_var_level<R, decltype(last)::value>), grid, block, 0, stream, P, src, guide, 1 << i, sl2, dst, g.albedo, last ? out : (R *)nullptr,
                               last ? variance_out : (R *)nullptr);
        });
}

// A scene-free filter call, its arguments checked: the device, working images of the call's own, enqueue(them, as R *),
// the stream drained
template <class F> int filter_on_own_work(int32_t precision, int32_t width, int32_t height, hipStream_t stream, F &&enqueue) {
    const int nd = check_device();
    if (nd < 0) return nd;
    DevBuf<char> work;
    if (work.alloc((size_t)width * height * WORK_REALS * (precision == TAKE_PRECISION_F64 ? 8 : 4)) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for the denoiser's working images");
    if (int rc = with_real(precision, [&](auto tag) { return enqueue((decltype(tag) *)work.p); })) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
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

// ---- what the scene-bound calls share
// the whole image, as take_hip_render_exr_scanlines
TakeRenderOpts whole_image(const TakeRenderOpts &o) {
    TakeRenderOpts ro = o;
    ro.strip_first = 0, ro.strip_stride = 1;
    return ro;
}
// RenderWorkspace::denoise of a scene of npix pixels, `reals` Reals: the filter's working images, then albedo, normal
// and depth; then, if wanted — from the next multiple of 8 bytes on — statistics planes of its own: m1, m2, count
template <class R> struct DenoiseArena {
    int64_t reals;
    R *work;
    Guides<R> guides;
    TakeAdaptiveStats stats;  // (null without own_stats)
    TakeFeatureBuffers planes() const { return {guides.albedo, guides.normal, guides.depth, nullptr, nullptr, nullptr}; }
};
template <class R> int denoise_arena(RenderWorkspace<R> &w, int64_t npix, bool own_stats, DenoiseArena<R> &a) {
    const int64_t real_planes = (WORK_REALS + 7) * npix, stats_at = (real_planes * (int64_t)sizeof(R) + 7) / 8 * 8;
    a.reals = own_stats ? (stats_at + 20 * npix + (int64_t)sizeof(R) - 1) / (int64_t)sizeof(R) : real_planes;
    if (int rc = w.ensure_denoise(a.reals)) return rc;
    a.work = w.denoise.p;
    a.guides.albedo = a.work + WORK_REALS * npix, a.guides.normal = a.guides.albedo + 3 * npix, a.guides.depth = a.guides.normal + 3 * npix;
    a.stats = TakeAdaptiveStats{nullptr, nullptr, nullptr};
    if (own_stats) {
        double *m1 = (double *)((char *)a.work + stats_at), *m2 = m1 + npix;
        a.stats = TakeAdaptiveStats{(int32_t *)(m2 + npix), m1, m2};
    }
    return TAKE_OK;
}
// The tail of the adaptive pipelines: the guides from the samples every pixel has (the guide pass does not grow with the
// maximum), then the variance filter of (rgb, stats) into (out, variance_out); ro: the whole image.  Enqueued on
// `stream`, no synchronisation.
template <class R>
int guides_then_variance_filter(TakeScene *ts, const TakeRenderOpts &ro, const TakeAdaptiveOpts *aopts, const DenoiseArena<R> &a, const R *rgb,
                                const TakeAdaptiveStats &stats, const DenoiseOpts &o, R *out, R *variance_out, hipStream_t stream) {
    TakeRenderOpts fo = ro;
    fo.spp = adaptive_min_spp(ro, aopts);
    if (int rc = render_features_scene(ts, fo, a.planes(), stream)) return rc;
    return denoise_var_enqueue(rgb, a.guides, stats, ts->width(), ts->height(), o, a.work, out, variance_out, stream);
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
    return filter_on_own_work(precision, width, height, (hipStream_t)stream, [&](auto *work) {
        using R = std::remove_pointer_t<decltype(work)>;
        return denoise_enqueue((const R *)d_rgb, typed<R>(d_guides), width, height, o, work, (R *)d_out, (hipStream_t)stream);
    });
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
    // rgb (filtered in place), then the guides that were given
    StagedPlanes<4> st{{plane_inout(rgb, out, 3 * real), plane_in(guides ? guides->albedo : nullptr, 3 * real), plane_in(guides ? guides->normal : nullptr, 3 * real),
                        plane_in(guides ? guides->depth : nullptr, real)}};
    if (int rc = st.alloc(npix, "out of device memory for the denoiser's planes")) return rc;
    if (int rc = st.upload()) return rc;
    const TakeFeatureBuffers d_guides{st[1], st[2], st[3], nullptr, nullptr, nullptr};
    if (int rc = take_hip_denoise_device(st[0], &d_guides, precision, width, height, opts, st[0], nullptr)) return rc;
    return st.download();
}

int take_hip_render_denoised_device(TakeScene *ts, const TakeRenderOpts *ropts, const TakeDenoiseOpts *dopts, void *d_out, void *stream) {
    if (!ts || !ropts || !d_out) return fail(TAKE_E_INVALID, "null argument");
    DenoiseOpts o;
    if (int rc = resolve(dopts, o)) return rc;
    TAKE_ON_DEVICE(ts);
    const TakeRenderOpts ro = whole_image(*ropts);
    const int W = ts->width(), H = ts->height();
    return on_primary(ts, [&](auto &sc, auto &work) {
        using R = std::remove_reference_t<decltype(*work.accum.p)>;
        DenoiseArena<R> a;
        if (int rc = denoise_arena(work, (int64_t)W * H, false, a)) return rc;
        if (int rc = render_scene(ts, ro, d_out, (hipStream_t)stream)) return rc;
        if (int rc = render_features_scene(ts, ro, a.planes(), (hipStream_t)stream)) return rc;
        if (int rc = denoise_enqueue((const R *)d_out, a.guides, W, H, o, a.work, (R *)d_out, (hipStream_t)stream)) return rc;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        return (int)TAKE_OK;
    });
}

int take_hip_render_denoised(TakeScene *ts, const TakeRenderOpts *ropts, const TakeDenoiseOpts *dopts, void *rgb_out_host) {
    if (!ts || !ropts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    DenoiseOpts o;
    if (int rc = resolve(dopts, o)) return rc;
    TAKE_ON_DEVICE(ts);
    StagedPlanes<1> st{{plane_out(rgb_out_host, (size_t)3 * (ts->f64() ? 8 : 4))}};
    if (int rc = st.alloc((size_t)ts->width() * ts->height(), "out of device memory for the denoised image")) return rc;
    if (int rc = take_hip_render_denoised_device(ts, ropts, dopts, st[0], nullptr)) return rc;
    return st.download();
}

int take_hip_denoise_variance_device(const void *d_rgb, const TakeFeatureBuffers *d_guides, const TakeAdaptiveStats *d_stats, int32_t precision, int32_t width,
                                     int32_t height, const TakeDenoiseOpts *opts, void *d_out, void *d_variance_out, void *stream) {
    DenoiseOpts o;
    if (int rc = check_variance_args(d_rgb, d_stats, d_out, precision, width, height, opts, o)) return rc;
    return filter_on_own_work(precision, width, height, (hipStream_t)stream, [&](auto *work) {
        using R = std::remove_pointer_t<decltype(work)>;
        return denoise_var_enqueue((const R *)d_rgb, typed<R>(d_guides), *d_stats, width, height, o, work, (R *)d_out, (R *)d_variance_out, (hipStream_t)stream);
    });
}

int take_hip_denoise_variance(const void *rgb, const TakeFeatureBuffers *guides, const TakeAdaptiveStats *stats, int32_t precision, int32_t width, int32_t height,
                              const TakeDenoiseOpts *opts, void *out, void *variance_out) {
    DenoiseOpts o;
    if (int rc = check_variance_args(rgb, stats, out, precision, width, height, opts, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const size_t real = precision == TAKE_PRECISION_F64 ? 8 : 4, npix = (size_t)width * height;
    // rgb (filtered in place), the guides that were given, the three statistics planes; then the variance plane, if wanted
    StagedPlanes<8> st{{plane_inout(rgb, out, 3 * real), plane_in(guides ? guides->albedo : nullptr, 3 * real), plane_in(guides ? guides->normal : nullptr, 3 * real),
                        plane_in(guides ? guides->depth : nullptr, real), plane_in(stats->count, 4), plane_in(stats->m1, 8), plane_in(stats->m2, 8),
                        plane_out(variance_out, real)}};
    if (int rc = st.alloc(npix, "out of device memory for the denoiser's planes")) return rc;
    if (int rc = st.upload()) return rc;
    const TakeFeatureBuffers d_guides{st[1], st[2], st[3], nullptr, nullptr, nullptr};
    const TakeAdaptiveStats d_stats{(int32_t *)st[4], (double *)st[5], (double *)st[6]};
    if (int rc = take_hip_denoise_variance_device(st[0], &d_guides, &d_stats, precision, width, height, opts, st[0], st[7], nullptr)) return rc;
    return st.download();
}

int take_hip_render_adaptive_denoised_device(TakeScene *ts, const TakeRenderOpts *ropts, const TakeAdaptiveOpts *aopts, const TakeDenoiseOpts *dopts, void *d_out,
                                             const TakeAdaptiveStats *d_stats, void *d_variance_out, void *stream) {
    DenoiseOpts o;
    if (int rc = check_adaptive_denoised_args(ts, ropts, aopts, dopts, d_out, o)) return rc;
    TAKE_ON_DEVICE(ts);
    const TakeRenderOpts ro = whole_image(*ropts);
    return on_primary(ts, [&](auto &sc, auto &work) {
        using R = std::remove_reference_t<decltype(*work.accum.p)>;
        DenoiseArena<R> a;
        if (int rc = denoise_arena(work, (int64_t)ts->width() * ts->height(), true, a)) return rc;
        // the arena's statistics planes stand in for the ones the caller did not ask for
        TakeAdaptiveStats stats = a.stats;
        if (d_stats && d_stats->count) stats.count = d_stats->count;
        if (d_stats && d_stats->m1) stats.m1 = d_stats->m1;
        if (d_stats && d_stats->m2) stats.m2 = d_stats->m2;
        if (int rc = render_adaptive_scene(ts, ro, aopts, d_out, stats, (hipStream_t)stream)) return rc;
        if (int rc = guides_then_variance_filter(ts, ro, aopts, a, (const R *)d_out, stats, o, (R *)d_out, (R *)d_variance_out, (hipStream_t)stream)) return rc;
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
    // the image and the wanted planes in device memory, then copied out
    StagedPlanes<5> st{{plane_out(rgb_out_host, 3 * real), plane_out(host_stats ? host_stats->count : nullptr, 4), plane_out(host_stats ? host_stats->m1 : nullptr, 8),
                        plane_out(host_stats ? host_stats->m2 : nullptr, 8), plane_out(variance_out_host, real)}};
    if (int rc = st.alloc(npix, "out of device memory for the denoised adaptive render's planes")) return rc;
    const TakeAdaptiveStats d_stats{(int32_t *)st[1], (double *)st[2], (double *)st[3]};
    if (int rc = take_hip_render_adaptive_denoised_device(ts, ropts, aopts, dopts, st[0], &d_stats, st[4], nullptr)) return rc;
    return st.download();
}

int take_hip_temporal_accumulate_device(const TakeTemporalFrame *d_cur, const TakeTemporalFrame *d_hist, const void *d_prev_xy, const void *d_prev_depth,
                                        int32_t precision, int32_t width, int32_t height, const TakeTemporalOpts *opts, const TakeTemporalFrame *d_out, void *stream) {
    TemporalOpts o;
    if (int rc = check_temporal_args(d_cur, d_hist, d_prev_xy, precision, width, height, opts, d_out, o)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    const int rc = with_real(precision, [&](auto tag) {
        using R = decltype(tag);
        const tp::Frame<R> hist = d_hist ? typed<R>(*d_hist) : tp::Frame<R>{};
        return temporal_enqueue(typed<R>(*d_cur), d_hist ? &hist : nullptr, (const R *)d_prev_xy, (const R *)d_prev_depth, width, height, o, typed<R>(*d_out),
                                (hipStream_t)stream);
    });
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
    // member by member of TakeTemporalFrame, the current frame's plane (accumulated in place, copied out where `out`
    // has the member) and the history's; then the motion planes
    const TakeTemporalFrame none{}, &h = hist ? *hist : none;
    StagedPlanes<14> st{{plane_inout(cur->rgb, out->rgb, 3 * real), plane_in(h.rgb, 3 * real), plane_inout(cur->count, out->count, 4), plane_in(h.count, 4),
                         plane_inout(cur->m1, out->m1, 8), plane_in(h.m1, 8), plane_inout(cur->m2, out->m2, 8), plane_in(h.m2, 8),
                         plane_inout(cur->depth, out->depth, real), plane_in(h.depth, real), plane_inout(cur->shape_id, out->shape_id, 4), plane_in(h.shape_id, 4),
                         plane_in(prev_xy, 2 * real), plane_in(prev_depth, real)}};
    if (int rc = st.alloc(npix, "out of device memory for the temporal accumulation's planes")) return rc;
    if (int rc = st.upload()) return rc;
    const TakeTemporalFrame dc{st[0], (int32_t *)st[2], (double *)st[4], (double *)st[6], st[8], (int32_t *)st[10]};
    const TakeTemporalFrame dh{st[1], (int32_t *)st[3], (double *)st[5], (double *)st[7], st[9], (int32_t *)st[11]};
    if (int rc = take_hip_temporal_accumulate_device(&dc, hist ? &dh : nullptr, st[12], st[13], precision, width, height, opts, &dc, nullptr)) return rc;
    return st.download();
}

int take_hip_render_temporal_device(TakeScene *ts, const TakeRenderOpts *ropts, const TakeAdaptiveOpts *aopts, const TakeTemporalOpts *topts,
                                    const TakeDenoiseOpts *dopts, int32_t restart, void *d_out, void *stream) {
    TemporalOpts t;
    DenoiseOpts o;
    if (int rc = check_render_temporal_args(ts, ropts, aopts, topts, dopts, d_out, t, o)) return rc;
    TAKE_ON_DEVICE(ts);
    const TakeRenderOpts ro = whole_image(*ropts);
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
        DenoiseArena<R> a;
        if (int rc = denoise_arena(work, npix, false, a)) return rc;
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
        if (int rc = guides_then_variance_filter(ts, ro, aopts, a, (const R *)acc.rgb, TakeAdaptiveStats{acc.count, acc.m1, acc.m2}, o, (R *)d_out, (R *)nullptr, s)) return rc;
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
    StagedPlanes<1> st{{plane_out(rgb_out_host, (size_t)3 * (ts->f64() ? 8 : 4))}};
    if (int rc = st.alloc((size_t)ts->width() * ts->height(), "out of device memory for the filtered frame")) return rc;
    if (int rc = take_hip_render_temporal_device(ts, ropts, aopts, topts, dopts, restart, st[0], nullptr)) return rc;
    return st.download();
}

}  // extern "C"

// tk_api.hip — the C entry points of include/take_hip.h that work on an existing scene: rendering, tracing, feature
// buffers, the motion pass, accumulation, statistics and the test hook that reads a resident tree back.  Launches no
// kernel: tracing and rendering is tk_render.hip, reached through tk_scene_handle.h.  The entry points that CHANGE a
// resident scene (transforms, vertices, camera and lens, mark and track, the shutter) are tk_scene_update.hip, scene
// creation tk_create.hip, scene groups tk_group.hip, the mesh entry points (PLY, serialized, OBJ, compute_normals)
// tk_mesh.hip, the image-space denoiser tk_denoise.hip; the shared plumbing is tk_host.h.  There is no CPU rendering
// path in this library: without a HIP device every entry point returns TAKE_E_NO_GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"

using namespace tk;
using namespace tk_host;

namespace {
// what one side keeps in device memory of its tree: counts and sizes of the arrays the trace kernels read (sc.dev and
// the device buffers; nothing of sc.host)
template <class R> TakeDebugTreeInfo debug_tree_info(const SceneT<R> &sc) {
    TakeDebugTreeInfo o{};
    o.node_format = sc.trace.nodes == NodeFormat::Q8 ? 2 : (sc.trace.nodes == NodeFormat::Q4 ? 1 : 0);
    o.node_width = sc.trace.nodes == NodeFormat::Q8 ? 8 : 4;
    o.two_level = sc.trace.two_level ? 1 : 0;
    o.root_child = sc.dev.root_child;
    o.real_bytes = (int32_t)sizeof(R);
    o.node_bytes = (int32_t)node_bytes<R>(sc.trace.nodes), o.prim_bytes = (int32_t)sizeof(PrimRec<R>), o.inst_bytes = (int32_t)sizeof(InstTrace<R>);
    o.n_nodes = sc.dev.n_nodes, o.n_prims = (int64_t)sc.prims.n, o.n_instances = (int64_t)sc.inst_trace.n;
    for (int a = 0; a < 3; a++) o.grid_lo[a] = sc.dev.grid_lo[a], o.grid_step[a] = sc.dev.grid_step[a];
    return o;
}
template <class R> int debug_tree_copy(const SceneT<R> &sc, void *nodes, void *prims, void *inst_trace) {
    const TakeDebugTreeInfo o = debug_tree_info(sc);
    const void *d_nodes = sc.dev.qnodes8 ? (const void *)sc.dev.qnodes8 : (sc.dev.qnodes ? (const void *)sc.dev.qnodes : (const void *)sc.dev.nodes);
    if ((o.n_nodes > 0 && !nodes) || (o.n_prims > 0 && !prims) || (o.n_instances > 0 && !inst_trace)) return fail(TAKE_E_INVALID, "null argument");
    if (o.n_nodes > 0) HIP_TRY(hipMemcpy(nodes, d_nodes, (size_t)o.n_nodes * o.node_bytes, hipMemcpyDeviceToHost));
    if (o.n_prims > 0) HIP_TRY(hipMemcpy(prims, sc.dev.prims, (size_t)o.n_prims * o.prim_bytes, hipMemcpyDeviceToHost));
    if (o.n_instances > 0) HIP_TRY(hipMemcpy(inst_trace, sc.dev.inst_trace, (size_t)o.n_instances * o.inst_bytes, hipMemcpyDeviceToHost));
    return TAKE_OK;
}
// take_hip_render_rays* / take_hip_camera_rays*: what needs neither scene nor device
int check_first_sample(int32_t first_sample, int32_t spp) {
    if (first_sample < 0 || (int64_t)first_sample + (int64_t)spp > (int64_t)INT32_MAX)
        return fail(TAKE_E_INVALID, "first_sample must be >= 0 and first_sample + spp must fit int32");
    return TAKE_OK;
}
int check_ray_batch(const TakeScene *ts, const TakeRenderOpts *opts, const TakeRayBatch *b, const void *out) {
    if (!ts || !opts || !b || (b->n > 0 && (!b->rays || !out))) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_render_values(*opts)) return rc;
    if (b->n < 0 || b->n >= ((int64_t)1 << 30)) return fail(TAKE_E_INVALID, "n must be in [0, 2^30)");
    if (b->ray_sets != 1 && b->ray_sets != opts->spp) return fail(TAKE_E_INVALID, "ray_sets must be 1 or spp");
    if (int rc = check_first_sample(b->first_sample, opts->spp)) return rc;
    if (b->flags & ~TAKE_RAYS_NORMALIZE) return fail(TAKE_E_INVALID, "unknown flag bits");
    if (b->reserved != 0) return fail(TAKE_E_INVALID, "reserved must be 0");
    return TAKE_OK;
}
// the host entry's look at the rays: the first with a non-finite component, or a direction the call cannot use
template <class R> int check_host_rays(const void *rays, int64_t count, bool normalise) {
    const R *r = (const R *)rays;
    auto refuse = [](int64_t i, const char *why) { return fail(TAKE_E_INVALID, "ray " + std::to_string(i) + ": " + why); };
    for (int64_t i = 0; i < count; i++, r += 8) {
        for (int c : {0, 1, 2, 4, 5, 6})
            if (!std::isfinite(r[c])) return refuse(i, "org and dir must be finite");
        if (normalise) {
            const R l2 = r[4] * r[4] + r[5] * r[5] + r[6] * r[6];  // (in Real, as the device's normalize)
            if (!(l2 > R(0)) || !std::isfinite(l2)) return refuse(i, "the direction's length is zero or overflows: it cannot be normalised");
        } else {
            const double x = r[4], y = r[5], z = r[6];
            if (!(std::fabs(x * x + y * y + z * z - 1.0) <= 1e-3))
                return refuse(i, "the direction is not of unit length (| |dir|^2 - 1 | > 1e-3): normalise it, or pass TAKE_RAYS_NORMALIZE");
        }
    }
    return TAKE_OK;
}
bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

namespace tk_host {
int check_adaptive_opts(const TakeAdaptiveOpts *a) {
    if (!a) return TAKE_OK;
    if (!std::isfinite(a->threshold) || !std::isfinite(a->floor)) return fail(TAKE_E_INVALID, "threshold and floor must be finite");
    if (a->flags != 0) return fail(TAKE_E_INVALID, "unknown flag bits");
    return TAKE_OK;
}
int strip_set(const TakeScene *ts, int first, int stride, StripSet &s, int32_t *rows_out) {
    if (stride <= 0 || first < 0 || first >= stride) return fail(TAKE_E_INVALID, "strip_first must be in [0, strip_stride)");
    s.first = first, s.stride = stride;
    s.rows = rows_of(ts->height(), first, stride, rows_out);
    s.npix = (int64_t)s.rows * ts->width();
    return TAKE_OK;
}
}  // namespace tk_host

extern "C" {

const char *take_hip_last_error(void) { return g_error.c_str(); }
int take_hip_abi_version(void) { return TAKE_HIP_ABI_VERSION; }
int take_hip_device_count(void) { return check_device(); }

int take_hip_render_rows(const TakeScene *ts, int32_t strip_first, int32_t strip_stride, int32_t *rows_out) {
    if (!ts) return fail(TAKE_E_INVALID, "null scene");
    StripSet s;
    if (int rc = strip_set(ts, strip_first, strip_stride, s, rows_out)) return rc;
    return s.rows;
}

int take_hip_render_device(TakeScene *ts, const TakeRenderOpts *opts, void *d_rgb_out, void *stream) {
    if (!ts || !opts || !d_rgb_out) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    return render_scene(ts, *opts, d_rgb_out, (hipStream_t)stream);
}

// Progressive rendering (the per-pixel accumulate of src/render.cpp:68-78 kept resident between calls).
int take_hip_render_accumulate(TakeScene *ts, const TakeRenderOpts *opts, int32_t restart, void *d_rgb_out, void *stream) {
    if (!ts || !opts || !d_rgb_out) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    if (ts->acc_restart_needed && restart == 0)
        return fail(TAKE_E_INVALID, "take_hip_render_accumulate: the scene's placements, vertices or camera changed since the last call: pass restart = 1");
    const TakeRenderOpts &a = ts->acc_opts;
    const bool fresh = restart != 0 || ts->acc_samples == 0;
    // (mixed scenes: the exact rounds the samples were rendered with, <= 0 meaning the default; f32 / f64 ignore the field)
    auto exact = [ts](const TakeRenderOpts &o) {
        return ts->precision != TAKE_PRECISION_MIXED ? 0 : o.exact_bounces > 0 ? o.exact_bounces : TAKE_DEFAULT_EXACT_BOUNCES;
    };
    if (!fresh && (a.seed != opts->seed || a.max_depth != opts->max_depth || a.integrator != opts->integrator ||
                   a.strip_first != opts->strip_first || a.strip_stride != opts->strip_stride || a.ray_epsilon != opts->ray_epsilon ||
                   exact(a) != exact(*opts)))
        return fail(TAKE_E_INVALID, "take_hip_render_accumulate: options differ from the ones the accumulated samples were "
                                    "rendered with (seed, max_depth, integrator, strips, ray_epsilon, exact_bounces): pass restart = 1");
    const int64_t first = fresh ? 0 : ts->acc_samples;
    if (first + (int64_t)opts->spp >= ((int64_t)1 << 31)) return fail(TAKE_E_INVALID, "too many accumulated samples");
    // (a workspace grown for a bigger batch keeps the accumulator: RenderWorkspace::ensure only ever enlarges it, and the
    // strip set — hence the pixel count — is fixed for the sequence)
    const int rc = render_scene(ts, *opts, d_rgb_out, (hipStream_t)stream, first, !fresh);
    if (rc) {
        ts->acc_samples = 0;  // the accumulator may hold a partial batch: the sequence has to restart
        return rc;
    }
    ts->acc_samples = first + opts->spp;
    ts->acc_opts = *opts;
    ts->acc_restart_needed = false;
    return TAKE_OK;
}
int64_t take_hip_accumulated_samples(const TakeScene *ts) { return ts ? ts->acc_samples : 0; }

int take_hip_render(TakeScene *ts, const TakeRenderOpts *opts, void *rgb_out_host) {
    if (!ts || !opts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    StripSet s;
    if (int rc = strip_set(ts, *opts, s)) return rc;
    const size_t bytes = (size_t)s.npix * 3 * (ts->f64() ? 8 : 4);
    if (bytes == 0) return TAKE_OK;
    // render into the scene's own output buffer, then copy out
    const void *img = nullptr;
    const int rc = render_scene_to_out(ts, *opts, s.npix, img);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(rgb_out_host, img, bytes, hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_render_exr_scanlines(TakeScene *ts, const TakeRenderOpts *opts, uint16_t *out_host) {
    if (!ts || !opts || !out_host) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    const int W = ts->width(), H = ts->height();
    TakeRenderOpts o = *opts;
    o.strip_first = 0, o.strip_stride = 1;
    const void *d_img = nullptr;
    int rc = render_scene_to_out(ts, o, (int64_t)W * H, d_img);
    if (rc) return rc;
    DevBuf<uint16_t> halves;
    if (halves.alloc((size_t)W * H * 3) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the scanline buffer");
    rc = take_hip_pack_exr_scanlines(d_img, ts->precision, W, H, halves.p, nullptr);
    if (!rc && hipMemcpy(out_host, halves.p, halves.bytes(), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(TAKE_E_DEVICE, "scanline download failed");
    return rc;
}

// First-hit feature buffers (albedo, shading normal, depth, coverage, ids): tk_render.hip, features_impl.
int take_hip_render_features_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeFeatureBuffers *d_out, void *stream) {
    if (!ts || !opts || !d_out) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    return render_features_scene(ts, *opts, *d_out, (hipStream_t)stream);
}
int take_hip_render_features(TakeScene *ts, const TakeRenderOpts *opts, const TakeFeatureBuffers *host_out) {
    if (!ts || !opts || !host_out) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    StripSet s;
    if (int rc = strip_set(ts, *opts, s)) return rc;
    const size_t npix = (size_t)s.npix, real = ts->f64() ? 8 : 4;
    // the wanted planes in device memory, then copied out
    StagedPlanes<6> st{{plane_out(host_out->albedo, 3 * real), plane_out(host_out->normal, 3 * real), plane_out(host_out->depth, real),
                        plane_out(host_out->alpha, real), plane_out(host_out->shape_id, 4), plane_out(host_out->material_id, 4)}};
    if (int rc = st.alloc(npix, "out of device memory for the feature buffers")) return rc;
    const TakeFeatureBuffers d_out{st[0], st[1], st[2], st[3], (int32_t *)st[4], (int32_t *)st[5]};
    TakeFeatureBuffers asked = npix == 0 ? *host_out : d_out;  // (an empty strip set: the checks run on what was asked for)
    if (int rc = render_features_scene(ts, *opts, asked, nullptr)) return rc;
    return st.download();
}

// Adaptive sampling (stop pixels whose error estimate is below a threshold): tk_render.hip, adaptive_impl.
int take_hip_render_adaptive_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeAdaptiveOpts *adaptive, void *d_rgb_out,
                                    const TakeAdaptiveStats *d_stats, void *stream) {
    if (!ts || !opts || !d_rgb_out) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_adaptive_opts(adaptive)) return rc;
    TAKE_ON_DEVICE(ts);
    return render_adaptive_scene(ts, *opts, adaptive, d_rgb_out, d_stats ? *d_stats : TakeAdaptiveStats{nullptr, nullptr, nullptr}, (hipStream_t)stream);
}
int take_hip_render_adaptive(TakeScene *ts, const TakeRenderOpts *opts, const TakeAdaptiveOpts *adaptive, void *rgb_out_host,
                             const TakeAdaptiveStats *host_stats) {
    if (!ts || !opts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_adaptive_opts(adaptive)) return rc;
    TAKE_ON_DEVICE(ts);
    StripSet s;
    if (int rc = strip_set(ts, *opts, s)) return rc;
    const size_t npix = (size_t)s.npix;
    // the image and the wanted planes in device memory, then copied out
    StagedPlanes<4> st{{plane_out(rgb_out_host, (size_t)3 * (ts->f64() ? 8 : 4)), plane_out(host_stats ? host_stats->count : nullptr, 4),
                        plane_out(host_stats ? host_stats->m1 : nullptr, 8), plane_out(host_stats ? host_stats->m2 : nullptr, 8)}};
    if (int rc = st.alloc(npix, "out of device memory for the adaptive render's planes")) return rc;
    const TakeAdaptiveStats d_stats{(int32_t *)st[1], (double *)st[2], (double *)st[3]};
    // (an empty strip set: the checks run, nothing is written)
    if (int rc = render_adaptive_scene(ts, *opts, adaptive, npix ? st[0] : rgb_out_host, d_stats, nullptr)) return rc;
    return st.download();
}

int take_hip_trace_closest(TakeScene *ts, const void *rays, int64_t n, void *hits) {
    if (!ts || (n > 0 && (!rays || !hits))) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    return trace_rays_host(ts, rays, n, hits, nullptr, false);
}
int take_hip_trace_any(TakeScene *ts, const void *rays, int64_t n, int32_t *occluded) {
    if (!ts || (n > 0 && (!rays || !occluded))) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    return trace_rays_host(ts, rays, n, nullptr, occluded, true);
}
int take_hip_trace_closest_device(TakeScene *ts, const void *d_rays, int64_t n, void *d_hits, int32_t count_mode,
                                  void *stream) {
    if (!ts || (n > 0 && (!d_rays || !d_hits))) return fail(TAKE_E_INVALID, "null argument");
    if (n == 0) return TAKE_OK;
    TAKE_ON_DEVICE(ts);
    return trace_rays_device(ts, d_rays, n, d_hits, count_mode != 0, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ caller-supplied rays
// Path tracing of caller-supplied rays and the export of the scene's camera rays (include/take_hip.h):
// tk_render.hip, render_impl (FirstRays::CALLER) and camera_rays_impl.  What needs no device is looked at before one is looked for.
int take_hip_render_rays_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeRayBatch *batch, void *d_rgb_out, void *stream) {
    if (int rc = check_ray_batch(ts, opts, batch, d_rgb_out)) return rc;
    if (!aligned16(batch->rays)) return fail(TAKE_E_INVALID, "the rays must be 16-byte aligned");
    if (batch->n == 0) return TAKE_OK;
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    return render_rays_scene(ts, *opts, *batch, d_rgb_out, (hipStream_t)stream);
}
int take_hip_render_rays(TakeScene *ts, const TakeRenderOpts *opts, const TakeRayBatch *batch, void *rgb_out_host) {
    if (int rc = check_ray_batch(ts, opts, batch, rgb_out_host)) return rc;
    const int64_t count = (int64_t)batch->ray_sets * batch->n;
    const bool normalise = (batch->flags & TAKE_RAYS_NORMALIZE) != 0;
    if (int rc = ts->f64() ? check_host_rays<double>(batch->rays, count, normalise) : check_host_rays<float>(batch->rays, count, normalise)) return rc;
    if (batch->n == 0) return TAKE_OK;
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    const size_t real = ts->f64() ? 8 : 4;
    DevBuf<char> d_rays, d_out;
    if (d_rays.alloc((size_t)count * 8 * real) != hipSuccess || d_out.alloc((size_t)batch->n * 3 * real) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for the rays and their texels");
    if (hipMemcpy(d_rays.p, batch->rays, d_rays.bytes(), hipMemcpyHostToDevice) != hipSuccess) return fail(TAKE_E_DEVICE, "ray upload failed");
    TakeRayBatch d_batch = *batch;
    d_batch.rays = d_rays.p;
    if (int rc = render_rays_scene(ts, *opts, d_batch, d_out.p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(rgb_out_host, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}
int take_hip_camera_rays_device(TakeScene *ts, const TakeRenderOpts *opts, int32_t first_sample, void *d_rays_out, void *stream) {
    if (!ts || !opts || !d_rays_out) return fail(TAKE_E_INVALID, "null argument");
    if (opts->spp <= 0) return fail(TAKE_E_INVALID, "spp must be positive");
    if (int rc = check_first_sample(first_sample, opts->spp)) return rc;
    if (!aligned16(d_rays_out)) return fail(TAKE_E_INVALID, "the rays must be 16-byte aligned");
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    return camera_rays_scene(ts, *opts, first_sample, d_rays_out, (hipStream_t)stream);
}
int take_hip_camera_rays(TakeScene *ts, const TakeRenderOpts *opts, int32_t first_sample, void *rays_out_host) {
    if (!ts || !opts || !rays_out_host) return fail(TAKE_E_INVALID, "null argument");
    if (opts->spp <= 0) return fail(TAKE_E_INVALID, "spp must be positive");
    if (int rc = check_first_sample(first_sample, opts->spp)) return rc;
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    const size_t bytes = (size_t)opts->spp * (size_t)ts->width() * (size_t)ts->height() * 8 * (ts->f64() ? 8 : 4);
    if (bytes == 0) return TAKE_OK;
    DevBuf<char> d_rays;
    if (d_rays.alloc(bytes) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the camera rays");
    if (int rc = camera_rays_scene(ts, *opts, first_sample, d_rays.p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(rays_out_host, d_rays.p, bytes, hipMemcpyDeviceToHost));
    return TAKE_OK;
}

// The motion pass (where every pixel's surface point was in the marked frame): tk_render.hip, motion_impl.
static int check_motion_args(const TakeScene *ts, const TakeRenderOpts *opts, const TakeMotionBuffers *b) {
    if (!ts || !opts || !b) return fail(TAKE_E_INVALID, "null argument");
    if (!b->prev_xy && !b->prev_depth && !b->depth && !b->shape_id)
        return fail(TAKE_E_INVALID, "no motion buffer was asked for: every pointer of TakeMotionBuffers is NULL");
    return TAKE_OK;
}
int take_hip_render_motion_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeMotionBuffers *d_out, void *stream) {
    if (int rc = check_motion_args(ts, opts, d_out)) return rc;
    TAKE_ON_DEVICE(ts);
    return render_motion_scene(ts, *opts, *d_out, true, (hipStream_t)stream);
}
int take_hip_render_motion(TakeScene *ts, const TakeRenderOpts *opts, const TakeMotionBuffers *host_out) {
    if (int rc = check_motion_args(ts, opts, host_out)) return rc;
    TAKE_ON_DEVICE(ts);
    const size_t npix = (size_t)ts->width() * ts->height(), real = ts->f64() ? 8 : 4;
    // the wanted planes in device memory, then copied out
    StagedPlanes<4> st{{plane_out(host_out->prev_xy, 2 * real), plane_out(host_out->prev_depth, real), plane_out(host_out->depth, real), plane_out(host_out->shape_id, 4)}};
    if (int rc = st.alloc(npix, "out of device memory for the motion buffers")) return rc;
    const TakeMotionBuffers d_out{st[0], st[1], st[2], (int32_t *)st[3]};
    if (int rc = render_motion_scene(ts, *opts, d_out, true, nullptr)) return rc;
    return st.download();
}

int take_hip_get_counters(const TakeScene *ts, TakeCounters *out) {
    if (!ts || !out) return fail(TAKE_E_INVALID, "null argument");
    *out = ts->counters;
    return TAKE_OK;
}
int take_hip_set_instrumentation(TakeScene *ts, int32_t flags) {
    if (!ts) return fail(TAKE_E_INVALID, "null scene");
    ts->instrumentation = flags;
    return TAKE_OK;
}
int take_hip_scene_stats(const TakeScene *ts, int64_t *n_nodes, int64_t *n_prims, int32_t *depth,
                         int64_t *device_bytes) {
    if (!ts) return fail(TAKE_E_INVALID, "null scene");
    const WideBvhStats s = on_primary(ts, [](const auto &sc, const auto &) { return sc.host.stats; });
    if (n_nodes) *n_nodes = s.n_nodes;
    if (n_prims) *n_prims = s.n_prims;
    if (depth) *depth = s.depth;
    // (a side the scene's precision does not make is empty: 0 bytes)
    if (device_bytes) *device_bytes = (int64_t)(ts->d.scene_bytes() + ts->f.scene_bytes());
    return TAKE_OK;
}
int take_hip_scene_build_info(const TakeScene *ts, int32_t *f32_builder, int32_t *f64_builder) {
    if (!ts) return fail(TAKE_E_INVALID, "null scene");
    if (const int nd = check_device(); nd < 0) return nd;
    if (f32_builder) *f32_builder = !has_side(ts, TAKE_PRECISION_F32) ? -1 : (ts->f.built_on_device ? TAKE_BUILDER_DEVICE_LBVH : TAKE_BUILDER_HOST_SAH);
    if (f64_builder) *f64_builder = !has_side(ts, TAKE_PRECISION_F64) ? -1 : (ts->d.built_on_device ? TAKE_BUILDER_DEVICE_LBVH : TAKE_BUILDER_HOST_SAH);
    return TAKE_OK;
}

// ------------------------------------------------------------------------------------------------ test hook: the resident tree
int take_hip_debug_tree_info(const TakeScene *ts, int32_t side, TakeDebugTreeInfo *info) {
    if (!ts || !info) return fail(TAKE_E_INVALID, "null argument");
    if (const int nd = check_device(); nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    *info = on_side(ts, side, [](const auto &sc) { return debug_tree_info(sc); });
    return TAKE_OK;
}
int take_hip_debug_tree(const TakeScene *ts, int32_t side, void *nodes, void *prims, void *inst_trace) {
    if (!ts || !nodes || !prims) return fail(TAKE_E_INVALID, "null argument");
    if (const int nd = check_device(); nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    TAKE_ON_DEVICE(ts);
    HIP_TRY(hipDeviceSynchronize());
    return on_side(ts, side, [&](const auto &sc) { return debug_tree_copy(sc, nodes, prims, inst_trace); });
}

}  // extern "C"

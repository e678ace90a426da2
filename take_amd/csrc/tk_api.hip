// tk_api.hip — the C entry points of include/take_hip.h that work on an existing scene: rendering, tracing, feature
// buffers, accumulation, statistics, the changes of a resident scene (new transforms, vertices, camera) and the test
// hook that reads a resident tree back.  Launches no kernel: tracing and rendering is tk_render.hip, the device LBVH
// build tk_build.hip, both reached through tk_scene_handle.h.  Scene creation is tk_create.hip, scene groups
// tk_group.hip, the mesh entry points (PLY, serialized, OBJ, compute_normals) tk_mesh.hip, the image-space denoiser
// tk_denoise.hip; the shared plumbing is
// tk_host.h.  There is no CPU rendering path in this library: without a HIP device every entry point returns TAKE_E_NO_GPU.
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
// what take_hip_scene_set_instance_transforms accepts, checked before anything is read or made
int check_repose(const TakeScene *ts, int64_t n) {
    if (ts->n_placements <= 0) return fail(TAKE_E_INVALID, "the scene has no placements (none were given, or TAKE_INSTANCES_FLATTEN expanded them)");
    if (n != ts->n_placements) return fail(TAKE_E_INVALID, "n = " + std::to_string(n) + ", but the scene has " + std::to_string(ts->n_placements) + " placements");
    const bool plain = on_primary(ts, [&](const auto &sc, const auto &) {
        return sc.trace.two_level && sc.trace.nodes != NodeFormat::Q8 && (int64_t)sc.inst_trace.n == n && (int64_t)sc.host.placements.inst_proto.size() == n;
    });
    if (!plain) return fail(TAKE_E_INVALID, "unsupported: the scene was built under TAKE_HIP_BRAID > 1 or TAKE_HIP_NODES=q8");
    return TAKE_OK;
}
// New transforms (device memory the library owns, complete) for all placements of ts (check_repose passed); a
// successful call keeps them: they are the scene's current transforms from then on (TakeScene::xforms)
int set_instance_transforms(TakeScene *ts, DevBuf<double> &xforms, int64_t n) {
    try {
        const int rc = stage_then_commit<ReposeStage>(ts, [&](const auto &sc, auto &stage) { return repose_two_level_device(sc, xforms.p, n, stage); });
        if (!rc) ts->xforms = std::move(xforms);
        return rc;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while re-posing the placements");
    }
}

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
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    return render_rays_scene(ts, *opts, *batch, d_rgb_out, (hipStream_t)stream);
}
int take_hip_render_rays(TakeScene *ts, const TakeRenderOpts *opts, const TakeRayBatch *batch, void *rgb_out_host) {
    if (int rc = check_ray_batch(ts, opts, batch, rgb_out_host)) return rc;
    const int64_t count = (int64_t)batch->ray_sets * batch->n;
    const bool normalise = (batch->flags & TAKE_RAYS_NORMALIZE) != 0;
    if (int rc = ts->f64() ? check_host_rays<double>(batch->rays, count, normalise) : check_host_rays<float>(batch->rays, count, normalise)) return rc;
    if (batch->n == 0) return TAKE_OK;
    const int nd = check_device();
    if (nd < 0) return nd;
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
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    return camera_rays_scene(ts, *opts, first_sample, d_rays_out, (hipStream_t)stream);
}
int take_hip_camera_rays(TakeScene *ts, const TakeRenderOpts *opts, int32_t first_sample, void *rays_out_host) {
    if (!ts || !opts || !rays_out_host) return fail(TAKE_E_INVALID, "null argument");
    if (opts->spp <= 0) return fail(TAKE_E_INVALID, "spp must be positive");
    if (int rc = check_first_sample(first_sample, opts->spp)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    const size_t bytes = (size_t)opts->spp * (size_t)ts->width() * (size_t)ts->height() * 8 * (ts->f64() ? 8 : 4);
    if (bytes == 0) return TAKE_OK;
    DevBuf<char> d_rays;
    if (d_rays.alloc(bytes) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the camera rays");
    if (int rc = camera_rays_scene(ts, *opts, first_sample, d_rays.p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(rays_out_host, d_rays.p, bytes, hipMemcpyDeviceToHost));
    return TAKE_OK;
}

// ------------------------------------------------------------------------------------------------ a resident scene changes
int take_hip_scene_set_instance_transforms_device(TakeScene *ts, const double *d_xforms, int64_t n, void *stream) {
    if (!ts || !d_xforms) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    // (the build runs on the default stream, as scene_create's does: first whatever `stream` still has to write into d_xforms)
    const int rc = check_repose(ts, n);
    if (rc) return rc;
    if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    DevBuf<double> own;  // (a copy the scene can keep: the caller's memory stays the caller's)
    if (own.alloc(12 * (size_t)n) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the transforms");
    HIP_TRY(hipMemcpy(own.p, d_xforms, own.bytes(), hipMemcpyDeviceToDevice));
    return set_instance_transforms(ts, own, n);
}
int take_hip_scene_set_instance_transforms(TakeScene *ts, const double *xforms, int64_t n) {
    if (!ts || !xforms) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    const int rc = check_repose(ts, n);
    if (rc) return rc;
    DevBuf<double> d_xforms;
    if (d_xforms.alloc(12 * (size_t)n) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the transforms");
    HIP_TRY(hipMemcpy(d_xforms.p, xforms, d_xforms.bytes(), hipMemcpyHostToDevice));
    return set_instance_transforms(ts, d_xforms, n);
}
// New vertices for meshes of a resident scene (include/take_hip.h), in two parts: what the path does not support of a
// scene (check_update_scene), and the core that stages every side and commits every side (commit_mesh_update).
// update_meshes, below them, is the public symbols: the arguments that need no scene, the device, the arguments against
// the scene, then both parts and the mark's bookkeeping.  two_level_too: take_hip_scene_update_meshes — a scene with
// placements takes update_two_level_meshes_device, any other scene the one path both symbols share.
// What the update does not support, in its words (take_hip_render_shutter_meshes* refuses the same):
static int check_update_scene(const TakeScene *ts, bool two_level_too) {
    const bool two_level = ts->n_placements > 0;
    if (two_level && !two_level_too) return fail(TAKE_E_INVALID, "unsupported: a two-level scene (take_hip_scene_update_meshes moves the vertices of its meshes)");
    if (ts->flattened) return fail(TAKE_E_INVALID, "unsupported: the scene was flattened from instances");
    const bool q8 = ts->node_knob == "q8" || on_primary(ts, [&](const auto &sc, const auto &) { return sc.trace.nodes == NodeFormat::Q8; });
    if (q8) return fail(TAKE_E_INVALID, "unsupported: the scene was built under TAKE_HIP_NODES=q8");
    if (two_level) {
        if (const int rc = check_repose(ts, ts->n_placements)) return rc;  // (TAKE_HIP_BRAID > 1: "unsupported")
        if (!ts->xforms.p || (int64_t)ts->xforms.n != 12 * ts->n_placements) return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group");
        if (on_primary(ts, [&](const auto &sc, const auto &) { return (int64_t)sc.prims.n - sc.host.blas_prims != (int64_t)ts->shape_face.n; }))
            return fail(TAKE_E_INVALID, "unsupported: the scene does not have one primitive record per shape");
    } else {
        if (on_primary(ts, [&](const auto &sc, const auto &) { return sc.trace.two_level; })) return fail(TAKE_E_INVALID, "unsupported: a two-level scene");
        if (!ts->shape_face.p) return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group, or has no shapes");
        if (on_primary(ts, [&](const auto &sc, const auto &) { return sc.prims.n != ts->shape_face.n; }))
            return fail(TAKE_E_INVALID, "unsupported: the scene does not have one primitive record per shape");
    }
    return TAKE_OK;
}
static bool mesh_has_normals(const TakeScene *ts, int32_t mesh) {
    return on_primary(ts, [&](const auto &sc, const auto &) { return (size_t)mesh < sc.host.meshes.size() && sc.host.meshes[mesh].nbase >= 0; });
}
// The core of an update (check_update_scene passed): every side staged from `in`, then every side committed.  A scene
// with placements gets its top level under d_xforms; new_records: they are not the transforms its placement records
// were made from (a slice of take_hip_render_shutter_meshes*), which are made again with it.  The mark, vertex tracking
// and the current transforms are the caller's business.
static int commit_mesh_update(TakeScene *ts, const MeshUpdateInputs &in, const double *d_xforms, bool new_records) {
    if (ts->n_placements > 0)
        return stage_then_commit<ProtoUpdateStage>(ts, [&](const auto &sc, auto &stage) {
            return update_two_level_meshes_device(sc, in, ts->mesh_vertices, ts->shape_face.p, d_xforms, ts->max_leaf, new_records, stage);
        });
    const bool compressed_ok = compressed_nodes_supported() && ts->node_knob != "wide", compressed_forced = ts->node_knob == "q16";
    return stage_then_commit<MeshUpdateStage>(ts, [&](const auto &sc, auto &stage) {
        return update_mesh_vertices_device(sc, in, ts->mesh_vertices, ts->shape_face.p, ts->max_leaf, compressed_ok, compressed_forced, ts->num_cus, stage);
    });
}
static int update_meshes(TakeScene *ts, const TakeMeshUpdate *updates, int32_t n_updates, bool two_level_too) {
    if (!ts || !updates) return fail(TAKE_E_INVALID, "null argument");
    if (n_updates <= 0) return fail(TAKE_E_INVALID, "n_updates must be positive");
    try {
        std::vector<int32_t> ids((size_t)n_updates);
        for (int32_t i = 0; i < n_updates; i++) {
            const TakeMeshUpdate &u = updates[i];
            const std::string who = "update " + std::to_string(i) + ": ";
            if (u.mesh < 0) return fail(TAKE_E_INVALID, who + "mesh index out of range");
            if (u.flags & ~TAKE_MESH_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, who + "unknown flag bits");
            if (!u.positions) return fail(TAKE_E_INVALID, who + "positions is null");
            ids[i] = u.mesh;
        }
        std::sort(ids.begin(), ids.end());
        for (int32_t i = 1; i < n_updates; i++)
            if (ids[i] == ids[i - 1]) return fail(TAKE_E_INVALID, "mesh " + std::to_string(ids[i]) + " appears more than once");
        const int nd = check_device();
        if (nd < 0) return nd;
        for (int32_t i = 0; i < n_updates; i++) {
            const TakeMeshUpdate &u = updates[i];
            const std::string who = "update " + std::to_string(i) + ": ";
            if ((size_t)u.mesh >= ts->mesh_vertices.size()) return fail(TAKE_E_INVALID, who + "mesh index out of range");
            if (u.normals && !mesh_has_normals(ts, u.mesh)) return fail(TAKE_E_INVALID, who + "normals given for a mesh without vertex normals");
        }
        if (const int rc = check_update_scene(ts, two_level_too)) return rc;
        TAKE_ON_DEVICE(ts);
        MeshUpdateInputs in;
        int rc = in.upload(ts->mesh_vertices, updates, n_updates);
        if (rc) return rc;
        // take_hip_scene_track_vertices: the first update after a mark keeps the geometry words of the primary side's
        // records as they are now — staged with the update, and the handle's only when every side committed
        TakeScene::FrameMark kept;
        const bool keep = ts->track_flags && ts->mark.set && !ts->mark.updated && !ts->mark.has_geometry();
        if (keep) {
            rc = ts->f64() ? copy_marked_geometry(ts->d, kept.geom_d, kept.inst_first) : copy_marked_geometry(ts->f, kept.geom_f, kept.inst_first);
            if (rc) return rc;
        }
        rc = commit_mesh_update(ts, in, ts->xforms.p, false);
        if (rc) return rc;
        ts->mark.updated = true;
        if (keep) ts->mark.geom_f = std::move(kept.geom_f), ts->mark.geom_d = std::move(kept.geom_d), ts->mark.inst_first = std::move(kept.inst_first);
        return TAKE_OK;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while updating the meshes");
    } catch (const std::exception &e) {
        return fail(TAKE_E_INVALID, std::string("updating the meshes failed: ") + e.what());
    }
}
int take_hip_scene_set_mesh_vertices(TakeScene *ts, const TakeMeshUpdate *updates, int32_t n_updates) { return update_meshes(ts, updates, n_updates, false); }
int take_hip_scene_update_meshes(TakeScene *ts, const TakeMeshUpdate *updates, int32_t n_updates) { return update_meshes(ts, updates, n_updates, true); }
// the lens of the handle (ts->lens, ts->lens_focus) -> every side's camera record, each value rounded to Real once;
// radius 0 is the pinhole camera, whose record holds zeros there
static void apply_lens(TakeScene *ts) {
    const bool on = ts->lens.aperture_radius > 0;
    for_each_side(ts, [&](auto &sc) {
        using R = std::remove_reference_t<decltype(sc.host.cam.focus)>;
        sc.host.cam.lens_radius = on ? R(ts->lens.aperture_radius) : R(0), sc.host.cam.focus = on ? R(ts->lens_focus) : R(0);
        sc.dev.cam = sc.host.cam;
        return TAKE_OK;
    });
}
// > 0, and still finite where the scene has an f32 side
static bool lens_focus_usable(const TakeScene *ts, double focus) {
    return focus > 0 && std::isfinite(focus) && (ts->precision == TAKE_PRECISION_F64 || ((float)focus > 0 && std::isfinite((float)focus)));
}
int take_hip_scene_set_camera(TakeScene *ts, const TakeCamera *camera) {
    if (!ts || !camera) return fail(TAKE_E_INVALID, "null argument");
    if (camera->width != ts->width() || camera->height != ts->height())
        return fail(TAKE_E_INVALID, "the new camera is " + std::to_string(camera->width) + " x " + std::to_string(camera->height) + ", the scene " +
                                        std::to_string(ts->width()) + " x " + std::to_string(ts->height()) + ": the render buffers are sized at creation");
    // (the lens stays: make_camera leaves its two members alone; an automatic focus follows the new lookat)
    const double look = look_distance(*camera);
    const bool refocus = ts->lens.aperture_radius > 0 && !(ts->lens.focus_distance > 0);
    if (refocus && !lens_focus_usable(ts, look)) return fail(TAKE_E_INVALID, "the scene's lens focuses on lookat, and the new camera's lookat is not in front of its lookfrom");
    for_each_side(ts, [&](auto &sc) { return make_camera(*camera, sc.host.cam), sc.dev.cam = sc.host.cam, TAKE_OK; });
    ts->look_distance = look, ts->camera = *camera;
    if (!(ts->lens.focus_distance > 0)) ts->lens_focus = look;
    apply_lens(ts);
    ts->acc_samples = 0, ts->acc_restart_needed = true;
    return TAKE_OK;
}

// The thin lens (include/take_hip.h; tk_lens.h): two members of every side's camera record, which the launches pass by
// value — no device memory changes, so no device is looked for.
int take_hip_scene_set_lens(TakeScene *ts, const TakeLens *lens) {
    if (!ts || !lens) return fail(TAKE_E_INVALID, "null argument");
    if (!(lens->aperture_radius >= 0) || !std::isfinite(lens->aperture_radius)) return fail(TAKE_E_INVALID, "the aperture radius must be finite and >= 0");
    if (!std::isfinite(lens->focus_distance)) return fail(TAKE_E_INVALID, "the focus distance must be finite");
    if (lens->flags != 0 || lens->reserved != 0) return fail(TAKE_E_INVALID, "flags and reserved must be 0");
    const double focus = lens->focus_distance > 0 ? lens->focus_distance : ts->look_distance;
    if (lens->aperture_radius > 0 && !lens_focus_usable(ts, focus))
        return fail(TAKE_E_INVALID, "the effective focus distance must be > 0 (and finite in the scene's precision): focus_distance <= 0 asks for |lookat - lookfrom|");
    ts->lens = *lens, ts->lens_focus = focus;
    apply_lens(ts);
    ts->acc_samples = 0, ts->acc_restart_needed = true;
    return TAKE_OK;
}
int take_hip_scene_get_lens(const TakeScene *ts, TakeLens *out) {
    if (!ts || !out) return fail(TAKE_E_INVALID, "null argument");
    *out = ts->lens;
    out->focus_distance = ts->lens_focus;
    return TAKE_OK;
}
int take_hip_scene_focus_distance_at(TakeScene *ts, int32_t column, int32_t row, double *distance_out) {
    if (!ts || !distance_out) return fail(TAKE_E_INVALID, "null argument");
    if (column < 0 || column >= ts->width() || row < 0 || row >= ts->height())
        return fail(TAKE_E_INVALID, "pixel (" + std::to_string(column) + ", " + std::to_string(row) + ") is outside the " + std::to_string(ts->width()) + " x " +
                                        std::to_string(ts->height()) + " image");
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    return focus_distance_scene(ts, column, row, distance_out);
}

// "The previous frame" of the temporal accumulation (include/take_hip.h): every side's camera and a copy of the
// placements' current transforms.  The copy is made first: a failed call leaves the earlier mark whole.
int take_hip_scene_mark_frame(TakeScene *ts) {
    if (!ts) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    DevBuf<double> copy;
    if (ts->n_placements > 0) {
        if (!ts->xforms.p || (int64_t)ts->xforms.n != 12 * ts->n_placements) return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group");
        if (copy.alloc(ts->xforms.n) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the marked frame's transforms");
        HIP_TRY(hipMemcpy(copy.p, ts->xforms.p, copy.bytes(), hipMemcpyDeviceToDevice));
    }
    ts->mark.xforms = std::move(copy);
    ts->mark.drop_geometry(), ts->mark.updated = false;  // (the records are the marked ones again)
    ts->mark.cam_f = ts->f.dev.cam, ts->mark.cam_d = ts->d.dev.cam;  // (a side the scene does not have: never read)
    ts->mark.camera = ts->camera;
    ts->mark.set = true;
    return TAKE_OK;
}

// Following moved vertices in the motion pass (include/take_hip.h): a switch in the handle; what it holds is made by
// update_meshes and dropped by take_hip_scene_mark_frame.
int take_hip_scene_track_vertices(TakeScene *ts, int32_t flags) {
    if (!ts) return fail(TAKE_E_INVALID, "null argument");
    if (flags & ~TAKE_TRACK_VERTICES) return fail(TAKE_E_INVALID, "unknown flag bits");
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    if (!flags) ts->mark.drop_geometry();
    ts->track_flags = flags;
    return TAKE_OK;
}
int take_hip_scene_tracking_info(const TakeScene *ts, int32_t *flags, int64_t *marked_bytes) {
    if (!ts) return fail(TAKE_E_INVALID, "null argument");
    if (flags) *flags = ts->track_flags;
    if (marked_bytes) *marked_bytes = (int64_t)(ts->mark.geom_f.bytes() + ts->mark.geom_d.bytes() + ts->mark.inst_first.bytes());
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

// ------------------------------------------------------------------------------------------------ motion blur
// A render over a shutter between the marked and the current frame (include/take_hip.h): the plan, the
// pose at a time (tk_shutter.h; launched by tk_render.hip's shutter_pose_device) and the loop over the slices, which
// re-poses through set_instance_transforms' own path and renders through take_hip_render_accumulate's.  With deforming
// meshes (take_hip_render_shutter_meshes*) the same loop also lerps their vertices per slice
// (tk_shutter.h: k_shutter_vertices; tk_render.hip: shutter_vertices_launch) and takes them in through commit_mesh_update.
static int check_shutter(const TakeShutter &s) {
    if (!std::isfinite(s.open) || !std::isfinite(s.close) || !(0.0 <= s.open && s.open <= s.close && s.close <= 1.0))
        return fail(TAKE_E_INVALID, "the shutter must have 0 <= open <= close <= 1");
    if (s.flags != 0) return fail(TAKE_E_INVALID, "unknown flag bits");
    return TAKE_OK;
}
int take_hip_shutter_plan(int32_t spp, const TakeShutter *shutter, int32_t *slices_out, int32_t *first_sample, double *time) {
    if (!slices_out) return fail(TAKE_E_INVALID, "null argument");
    const TakeShutter s = shutter ? *shutter : TakeShutter{0.0, 1.0, 0, 0};
    if (int rc = check_shutter(s)) return rc;
    if (spp <= 0) return fail(TAKE_E_INVALID, "spp must be positive");
    const int32_t K = s.slices <= 0 ? std::min<int32_t>(spp, 16) : std::min(s.slices, spp);
    *slices_out = K;
    for (int32_t k = 0; first_sample && k <= K; k++) first_sample[k] = (int32_t)((int64_t)k * spp / K);
    for (int32_t k = 0; time && k < K; k++) time[k] = s.open + (s.close - s.open) * ((k + 0.5) / K);
    return TAKE_OK;
}
// what the shutter needs of the scene: a mark, and — with placements — what the re-pose accepts and both sets of transforms
static int check_shutter_scene(const TakeScene *ts) {
    if (!ts->mark.set) return fail(TAKE_E_INVALID, "no marked frame: take_hip_scene_mark_frame has not been called on this scene");
    if (ts->n_placements <= 0) return TAKE_OK;
    if (const int rc = check_repose(ts, ts->n_placements)) return rc;
    if (!ts->xforms.p || (int64_t)ts->xforms.n != 12 * ts->n_placements || (int64_t)ts->mark.xforms.n != 12 * ts->n_placements)
        return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group");
    return TAKE_OK;
}
static bool camera_usable(const TakeCamera &c) {
    bool finite = std::isfinite(c.vfov), apart = false;
    for (int a = 0; a < 3; a++) finite = finite && std::isfinite(c.lookfrom[a]) && std::isfinite(c.lookat[a]) && std::isfinite(c.up[a]), apart = apart || c.lookfrom[a] != c.lookat[a];
    return finite && apart;
}
static int bad_pose(int64_t first_bad, int64_t n) {
    return fail(TAKE_E_INVALID, "slice " + std::to_string(first_bad / n) + ": instance " + std::to_string(first_bad % n) + ": singular or non-finite transform");
}
int take_hip_shutter_pose(TakeScene *ts, double t, TakeCamera *camera_out, double *xforms_out) {
    if (!ts || !camera_out) return fail(TAKE_E_INVALID, "null argument");
    if (!(t >= 0.0 && t <= 1.0)) return fail(TAKE_E_INVALID, "t must be in [0, 1]");
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    if (const int rc = check_shutter_scene(ts)) return rc;
    const TakeCamera cam = shutter_camera(ts->mark.camera, ts->camera, t);
    if (!camera_usable(cam)) return fail(TAKE_E_INVALID, "slice 0: the interpolated camera is not finite, or its lookat coincides with its lookfrom");
    if (xforms_out && ts->n_placements > 0) {
        DevBuf<double> posed;
        int64_t first_bad = -1;
        std::vector<int> moved;
        if (const int rc = shutter_pose_device(ts->mark.xforms.p, ts->xforms.p, std::vector<double>{t}, ts->n_placements, posed, first_bad, moved)) return rc;
        if (first_bad >= 0) return bad_pose(first_bad, ts->n_placements);
        HIP_TRY(hipMemcpy(xforms_out, posed.p, posed.bytes(), hipMemcpyDeviceToHost));
    }
    *camera_out = cam;
    return TAKE_OK;
}
// every side's camera record from `cam`, lens members kept (take_hip_scene_set_camera's arithmetic; nothing else of the handle)
static void pose_camera(TakeScene *ts, const TakeCamera &cam) {
    for_each_side(ts, [&](auto &sc) { return make_camera(cam, sc.host.cam), sc.dev.cam = sc.host.cam, TAKE_OK; });
}
// take_hip_render_shutter_meshes* (DESIGN.md §4r): what it refuses of its motions without a scene
static int check_motions(const TakeMeshMotion *motions, int32_t n) {
    if (n < 0) return fail(TAKE_E_INVALID, "n must not be negative");
    if (n > 0 && !motions) return fail(TAKE_E_INVALID, "null argument");
    std::vector<int32_t> ids((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const TakeMeshMotion &m = motions[i];
        const std::string who = "motion " + std::to_string(i) + ": ";
        if (m.mesh < 0) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        if (m.flags & ~TAKE_MESH_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, who + "unknown flag bits");
        if (!m.positions0 || !m.positions1) return fail(TAKE_E_INVALID, who + "positions0 or positions1 is null");
        if (!m.normals0 != !m.normals1) return fail(TAKE_E_INVALID, who + "normals0 and normals1 must be given together");
        ids[i] = m.mesh;
    }
    std::sort(ids.begin(), ids.end());
    for (int32_t i = 1; i < n; i++)
        if (ids[i] == ids[i - 1]) return fail(TAKE_E_INVALID, "mesh " + std::to_string(ids[i]) + " appears more than once");
    return TAKE_OK;
}
// The deforming meshes of a render over the shutter, in device memory: per array of a motion its two ends (host arrays
// uploaded once, device arrays borrowed) and the buffer the slices' vertices are made in; the update's inputs over
// those buffers — the same for every slice — and over the current ends, which put the scene back.
struct SliceMeshes {
    struct Array {
        const double *a, *b;
        double *out;
        int64_t n;
    };
    std::vector<DevBuf<double>> owned;
    std::vector<Array> arrays;
    MeshUpdateInputs slice, current;
    DevBuf<int> moved;
    int make(const TakeScene *ts, const TakeMeshMotion *motions, int32_t n) {
        const char *nomem = "out of device memory for the meshes' vertices over the shutter";
        std::vector<TakeMeshUpdate> to_slice((size_t)n), to_current((size_t)n);
        auto resident = [&](const double *src, bool device, size_t words, const double *&dst) {
            if (device) return dst = src, (int)TAKE_OK;
            owned.emplace_back();
            if (owned.back().alloc(std::max<size_t>(words, 1)) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
            if (words) HIP_TRY(hipMemcpy(owned.back().p, src, words * sizeof(double), hipMemcpyHostToDevice));
            return dst = owned.back().p, (int)TAKE_OK;
        };
        for (int32_t i = 0; i < n; i++) {
            const TakeMeshMotion &m = motions[i];
            const size_t words = 3 * (size_t)ts->mesh_vertices[m.mesh];
            const bool device = (m.flags & TAKE_MESH_DEVICE_ARRAYS) != 0;
            const double *ends[2][2] = {{m.positions0, m.positions1}, {m.normals0, m.normals1}};
            const double *out[2] = {nullptr, nullptr}, *now[2] = {nullptr, nullptr};
            for (int k = 0; k < 2; k++) {
                if (!ends[k][0]) continue;
                Array arr{nullptr, nullptr, nullptr, (int64_t)words};
                if (const int rc = resident(ends[k][0], device, words, arr.a)) return rc;
                if (const int rc = resident(ends[k][1], device, words, arr.b)) return rc;
                owned.emplace_back();
                if (owned.back().alloc(std::max<size_t>(words, 1)) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
                arr.out = owned.back().p, out[k] = arr.out, now[k] = arr.b;
                arrays.push_back(arr);
            }
            to_slice[i] = TakeMeshUpdate{m.mesh, TAKE_MESH_DEVICE_ARRAYS, out[0], out[1]};
            to_current[i] = TakeMeshUpdate{m.mesh, TAKE_MESH_DEVICE_ARRAYS, now[0], now[1]};
        }
        if (moved.alloc(1) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
        if (const int rc = slice.upload(ts->mesh_vertices, to_slice.data(), n)) return rc;
        return current.upload(ts->mesh_vertices, to_current.data(), n);
    }
    // every array at time t -> its buffer (the default stream, as the update that reads them next); any: some vertex is
    // not the current one bit for bit
    int lerp(double t, int num_cus, bool &any) {
        HIP_TRY(hipMemsetAsync(moved.p, 0, sizeof(int), nullptr));
        for (const Array &x : arrays) shutter_vertices_launch(x.a, x.b, x.n, t, x.out, moved.p, num_cus, nullptr);
        HIP_TRY(hipGetLastError());
        int flag = 0;
        HIP_TRY(hipMemcpy(&flag, moved.p, sizeof(int), hipMemcpyDeviceToHost));
        any = flag != 0;
        return TAKE_OK;
    }
};
// The one loop over the slices: take_hip_render_shutter_device (n_motions = 0) and take_hip_render_shutter_meshes_device.
static int render_over_shutter(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n_motions,
                               void *d_rgb_out, void *stream) {
    if (!ts || !opts || !d_rgb_out) return fail(TAKE_E_INVALID, "null argument");
    int32_t K = 0;
    if (int rc = take_hip_shutter_plan(opts->spp, shutter, &K, nullptr, nullptr)) return rc;
    try {
        if (int rc = check_motions(motions, n_motions)) return rc;
        const int nd = check_device();
        if (nd < 0) return nd;
        TAKE_ON_DEVICE(ts);
        for (int32_t i = 0; i < n_motions; i++) {
            const std::string who = "motion " + std::to_string(i) + ": ";
            if ((size_t)motions[i].mesh >= ts->mesh_vertices.size()) return fail(TAKE_E_INVALID, who + "mesh index out of range");
            if (motions[i].normals0 && !mesh_has_normals(ts, motions[i].mesh)) return fail(TAKE_E_INVALID, who + "normals given for a mesh without vertex normals");
        }
        if (const int rc = check_shutter_scene(ts)) return rc;
        if (n_motions > 0)
            if (const int rc = check_update_scene(ts, true)) return rc;
        std::vector<int32_t> first((size_t)K + 1);
        std::vector<double> time((size_t)K);
        take_hip_shutter_plan(opts->spp, shutter, &K, first.data(), time.data());
        // every slice's pose, looked at before the first sample is rendered
        const int64_t n = ts->n_placements;
        std::vector<TakeCamera> cams;
        for (int32_t k = 0; k < K; k++) {
            cams.push_back(shutter_camera(ts->mark.camera, ts->camera, time[k]));
            if (!camera_usable(cams.back()))
                return fail(TAKE_E_INVALID, "slice " + std::to_string(k) + ": the interpolated camera is not finite, or its lookat coincides with its lookfrom");
        }
        DevBuf<double> posed;
        int64_t first_bad = -1;
        std::vector<int> moved;
        if (n > 0) {
            if (const int rc = shutter_pose_device(ts->mark.xforms.p, ts->xforms.p, time, n, posed, first_bad, moved)) return rc;
            if (first_bad >= 0) return bad_pose(first_bad, n);
        }
        // the deforming meshes: both ends and the slices' buffers in device memory before the first slice (the default
        // stream reads them: first whatever `stream` still has to write into device arrays)
        SliceMeshes meshes;
        if (n_motions > 0) {
            if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
            if (const int rc = meshes.make(ts, motions, n_motions)) return rc;
        }
        // the slices; whatever happens from here on, the scene goes back to its current pose.  `at`: the transforms the
        // placements are under — a slice whose pose is the current transforms bit for bit is rendered under those, and
        // placements that did not move since the mark are never re-posed at all.  `deformed`: the meshes are not at
        // their current vertices — a slice whose vertices are the current ones bit for bit, in a scene that is at them,
        // runs no update, and one that runs it makes the placements' records and the top level for its pose with it
        const bool restart_needed = ts->acc_restart_needed;  // (a re-pose sets it; a one-shot render leaves it alone, and so does this call)
        const double *at = ts->xforms.p;
        bool deformed = false, updated = false;
        auto repose_to = [&](const double *x) {
            if (x == at) return (int)TAKE_OK;
            const int rc = stage_then_commit<ReposeStage>(ts, [&](const auto &sc, auto &stage) { return repose_two_level_device(sc, x, n, stage); });
            if (!rc) at = x;
            return rc;
        };
        auto update_to = [&](const MeshUpdateInputs &in, const double *x, bool now_deformed) {
            const int rc = commit_mesh_update(ts, in, x, x != at);
            if (!rc) at = x, deformed = now_deformed, updated = true;
            return rc;
        };
        int rc = TAKE_OK;
        for (int32_t k = 0; k < K && !rc; k++) {
            pose_camera(ts, cams[k]);
            const double *x = n > 0 && moved[k] ? posed.p + 12 * n * (int64_t)k : ts->xforms.p;
            bool any = false;
            if (n_motions > 0) rc = meshes.lerp(time[k], ts->num_cus, any);
            if (!rc && (any || deformed)) {
                rc = update_to(meshes.slice, x, any);
                if (rc) rc = fail(rc, "slice " + std::to_string(k) + ": " + g_error);
            } else if (!rc && n > 0) {
                rc = repose_to(x);
            }
            TakeRenderOpts o = *opts;
            o.spp = first[k + 1] - first[k];
            if (!rc) rc = render_scene(ts, o, d_rgb_out, (hipStream_t)stream, first[k], k > 0, k + 1 == K);
        }
        const std::string why = g_error;
        pose_camera(ts, ts->camera);
        const int back = updated ? update_to(meshes.current, ts->xforms.p, false) : (n > 0 ? repose_to(ts->xforms.p) : (int)TAKE_OK);
        ts->acc_samples = 0, ts->acc_restart_needed = restart_needed || back != TAKE_OK;
        if (rc) return fail(rc, why);
        if (back) return fail(back, "the render is complete, but putting the scene back at its current pose failed: " + g_error);
        return TAKE_OK;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while rendering over the shutter");
    }
}
// the host entries: the image in device memory, then copied out
static int render_shutter_to_host(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n_motions,
                                  void *rgb_out_host) {
    if (!ts || !opts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    int32_t K = 0;
    if (int rc = take_hip_shutter_plan(opts->spp, shutter, &K, nullptr, nullptr)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    StripSet s;
    if (int rc = strip_set(ts, *opts, s)) return rc;
    const size_t bytes = (size_t)s.npix * 3 * (ts->f64() ? 8 : 4);
    if (bytes == 0) return TAKE_OK;
    DevBuf<char> img;
    if (img.alloc(bytes) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the image");
    if (int rc = render_over_shutter(ts, opts, shutter, motions, n_motions, img.p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(rgb_out_host, img.p, bytes, hipMemcpyDeviceToHost));
    return TAKE_OK;
}
int take_hip_render_shutter_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, void *d_rgb_out, void *stream) {
    return render_over_shutter(ts, opts, shutter, nullptr, 0, d_rgb_out, stream);
}
int take_hip_render_shutter(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, void *rgb_out_host) {
    return render_shutter_to_host(ts, opts, shutter, nullptr, 0, rgb_out_host);
}
int take_hip_render_shutter_meshes_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n,
                                          void *d_rgb_out, void *stream) {
    return render_over_shutter(ts, opts, shutter, motions, n, d_rgb_out, stream);
}
int take_hip_render_shutter_meshes(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n,
                                   void *rgb_out_host) {
    if (!ts || !opts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    int32_t K = 0;
    if (int rc = take_hip_shutter_plan(opts->spp, shutter, &K, nullptr, nullptr)) return rc;
    try {
        if (int rc = check_motions(motions, n)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while rendering over the shutter");
    }
    return render_shutter_to_host(ts, opts, shutter, motions, n, rgb_out_host);
}
// The vertices of a mesh at a time of the shutter, without a scene (include/take_hip.h; tk_shutter.h: k_shutter_vertices)
static int check_shutter_vertices(const void *a, const void *b, int64_t n, double t, const void *out) {
    if (!a || !b || !out) return fail(TAKE_E_INVALID, "null argument");
    if (n <= 0) return fail(TAKE_E_INVALID, "n must be positive");
    if (!(t >= 0.0 && t <= 1.0)) return fail(TAKE_E_INVALID, "t must be in [0, 1]");
    return TAKE_OK;
}
int take_hip_shutter_vertices_device(const double *d_a, const double *d_b, int64_t n, double t, double *d_out, int32_t *moved_host, void *stream) {
    if (int rc = check_shutter_vertices(d_a, d_b, n, t, d_out)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    int device = 0, num_cus = 0;
    HIP_TRY(hipGetDevice(&device));
    if (hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || num_cus <= 0) num_cus = 256;
    DevBuf<int> moved;
    if (moved.alloc(1) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the vertices at a time of the shutter");
    HIP_TRY(hipMemsetAsync(moved.p, 0, sizeof(int), (hipStream_t)stream));
    shutter_vertices_launch(d_a, d_b, n, t, d_out, moved.p, num_cus, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, moved.p, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (moved_host) *moved_host = flag;
    return TAKE_OK;
}
int take_hip_shutter_vertices(const double *a, const double *b, int64_t n, double t, double *out, int32_t *moved) {
    if (int rc = check_shutter_vertices(a, b, n, t, out)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    DevBuf<double> d_a, d_b, d_out;
    if (d_a.alloc((size_t)n) != hipSuccess || d_b.alloc((size_t)n) != hipSuccess || d_out.alloc((size_t)n) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for the vertices at a time of the shutter");
    HIP_TRY(hipMemcpy(d_a.p, a, d_a.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_b.p, b, d_b.bytes(), hipMemcpyHostToDevice));
    if (int rc = take_hip_shutter_vertices_device(d_a.p, d_b.p, n, t, d_out.p, moved, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
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
    const int nd = check_device();
    if (nd < 0) return nd;
    if (f32_builder) *f32_builder = !has_side(ts, TAKE_PRECISION_F32) ? -1 : (ts->f.built_on_device ? TAKE_BUILDER_DEVICE_LBVH : TAKE_BUILDER_HOST_SAH);
    if (f64_builder) *f64_builder = !has_side(ts, TAKE_PRECISION_F64) ? -1 : (ts->d.built_on_device ? TAKE_BUILDER_DEVICE_LBVH : TAKE_BUILDER_HOST_SAH);
    return TAKE_OK;
}

// ------------------------------------------------------------------------------------------------ test hook: the resident tree
int take_hip_debug_tree_info(const TakeScene *ts, int32_t side, TakeDebugTreeInfo *info) {
    if (!ts || !info) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    *info = on_side(ts, side, [](const auto &sc) { return debug_tree_info(sc); });
    return TAKE_OK;
}
int take_hip_debug_tree(const TakeScene *ts, int32_t side, void *nodes, void *prims, void *inst_trace) {
    if (!ts || !nodes || !prims) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    TAKE_ON_DEVICE(ts);
    HIP_TRY(hipDeviceSynchronize());
    return on_side(ts, side, [&](const auto &sc) { return debug_tree_copy(sc, nodes, prims, inst_trace); });
}

}  // extern "C"

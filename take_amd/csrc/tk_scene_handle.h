// tk_scene_handle.h — the scene handle and who owns what in it: TakeScene has one SceneT per precision side (the scene
// itself), each with the TraceState of its trace kernel instance, and ONE RenderWorkspace, of the primary side's precision.
// Then the walks over the sides (on_primary, for_each_side, on_side, stage_then_commit) and what tk_create.hip (scene
// creation), tk_group.hip (groups), tk_api.hip (the entry points that render and trace) and tk_scene_update.hip (those
// that change a resident scene) call of tk_render.hip (the only unit that compiles the kernels of tk_kernels.h) and of
// tk_build.hip (the device LBVH build: the only one that compiles tk_build_gpu.h's).  Includes no kernel source.
#pragma once
#include <chrono>
#include <cmath>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "tk_host.h"
#include "tk_host_scene.h"

namespace tk_host {
using namespace tk;

struct EventPool {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    EventPool() = default;
    EventPool(const EventPool &) = delete;
    EventPool &operator=(const EventPool &) = delete;
    ~EventPool() {
        for (auto e : ev) (void)hipEventDestroy(e);
    }
    hipEvent_t get() {
        if (used == ev.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;  // callers treat a null event as a failed timing call
            ev.push_back(e);
        }
        return ev[used++];
    }
    void reset() { used = 0; }
};

// Queue lengths read back WITHOUT stalling the launch loop (render_impl): a ring of pinned words + events, made by the
// first render.
struct PollRing {
    static constexpr int SIZE = 64;
    int32_t *word = nullptr;  // SIZE pinned words
    hipEvent_t ev[SIZE] = {};
    PollRing() = default;
    PollRing(const PollRing &) = delete;
    PollRing &operator=(const PollRing &) = delete;
    ~PollRing() {
        if (word) (void)hipHostFree(word);
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() {  // (a no-op once it has succeeded; after a failure the next call makes what is missing)
        hipError_t r = word ? hipSuccess : hipHostMalloc((void **)&word, sizeof(int32_t) * SIZE, hipHostMallocDefault);
        for (int i = 0; i < SIZE && r == hipSuccess; i++)
            if (!ev[i]) r = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        return r;
    }
};

// What the traversal of a scene is: set once from what upload_scene uploaded, copied by replicas.  The trace kernel
// instance, its node size and its block geometry all follow from it (tk_render.hip: with_trace_kernel).
enum class NodeFormat { WIDE /* Node4<R> */, Q4 /* QNode4, compressed */, Q8 /* QNode8, compressed 8-wide */ };
struct TraceKind {
    NodeFormat nodes = NodeFormat::WIDE;
    bool two_level = false;  // instances (InstTrace): the INST kernels
};
template <class R> constexpr size_t node_bytes(NodeFormat f) {
    return f == NodeFormat::Q8 ? sizeof(QNode8) : (f == NodeFormat::Q4 ? sizeof(QNode4) : sizeof(Node4<R>));
}

// The persistent trace grid of one side (alloc_trace_state).  Blocks per CU and spill levels are properties of the kernel
// instance the side's `trace` selects (a replica takes the former from its source), the grid is blocks per CU times the device's CUs.
struct TraceState {
    DevBuf<unsigned long long> spill;  // the stack levels beyond the LDS: [level][ray group of the grid]
    int blocks_per_cu = 0, spill_levels = 0;
    int trace_grid = 0;
    int64_t spill_stride = 0;  // ray groups in the persistent trace grid
    // blocks of a launch over a queue of at most n_bound rays: the grid, cut down when they cannot fill it (one block per 128 rays)
    unsigned grid_for(int64_t n_bound) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(trace_grid, (n_bound + 127) / 128)); }
};

// One precision side of a scene: what a replica copies, bind() points into and a stage replaces.
template <class R> struct SceneT {
    HostScene<R> host;  // kept: cheap relative to HBM copies, used for stats
    DevBuf<Node4<R>> nodes;
    DevBuf<QNode4> qnodes;
    DevBuf<QNode8> qnodes8;
    DevBuf<PrimRec<R>> prims;
    DevBuf<MeshInfo> meshes;
    DevBuf<int32_t> face_idx;
    DevBuf<R> normals, uvs, texels;
    DevBuf<MaterialRec<R>> materials;
    DevBuf<ImageInfo> images;
    DevBuf<LightRec<R>> lights;
    DevBuf<R> light_pmf, light_cdf;
    DevBuf<InstTrace<R>> inst_trace;
    DevBuf<InstShade<R>> inst_shade;
    DevBuf<R> env_marginal, env_conditional;
    DevBuf<int32_t> env_guide_m, env_guide_c;
    DeviceScene<R> dev{};
    bool built_on_device = false;
    TraceKind trace;         // which trace kernel instance traverses this scene
    TraceState trace_state;  // that instance's grid on the scene's device

    // The scene arrays: f(x.nodes...), f(x.qnodes...), ... for the scenes x, in the order replicate_t allocates them.
    template <class F, class... S> static void for_each_array(F &&f, S &...x) {
        f(x.nodes...), f(x.qnodes...), f(x.qnodes8...), f(x.prims...), f(x.meshes...), f(x.face_idx...), f(x.normals...);
        f(x.uvs...), f(x.texels...), f(x.materials...), f(x.images...), f(x.lights...), f(x.light_pmf...), f(x.light_cdf...);
        f(x.inst_trace...), f(x.inst_shade...), f(x.env_marginal...), f(x.env_conditional...), f(x.env_guide_m...), f(x.env_guide_c...);
    }
    // dev's pointers into this scene's arrays: null where an array is empty, and for the node formats not in use (only
    // the format the kernels traverse is allocated)
    void bind() {
        dev.nodes = nodes.p, dev.qnodes = qnodes.p, dev.qnodes8 = qnodes8.p, dev.prims = prims.p;
        dev.shapes = nullptr;  // (ShapeInfo stays on the host: every kernel reads the shading side of a primitive from its own record)
        dev.meshes = meshes.p, dev.face_idx = face_idx.p, dev.normals = normals.p, dev.uvs = uvs.p, dev.texels = texels.p;
        dev.materials = materials.p, dev.images = images.p, dev.lights = lights.p, dev.light_pmf = light_pmf.p, dev.light_cdf = light_cdf.p;
        dev.inst_trace = inst_trace.p, dev.inst_shade = inst_shade.p;
        dev.env.marginal = env_marginal.p, dev.env.conditional = env_conditional.p, dev.env.guide_m = env_guide_m.p, dev.env.guide_c = env_guide_c.p;
    }
    // device bytes of the scene (take_hip_scene_stats): the light-picking and environment-map tables have never been
    // counted in this figure
    size_t scene_bytes() const {
        size_t n = 0;
        for_each_array([&n](const auto &b) { n += b.bytes(); }, *this);
        return n - light_pmf.bytes() - light_cdf.bytes() - env_marginal.bytes() - env_conditional.bytes() - env_guide_m.bytes() - env_guide_c.bytes();
    }
};

// take_hip_render_adaptive*: the per-pixel state of the adaptive sampler (tk_adaptive.h), for the pixels of the call's
// strip set: samples received and the moments of the sample values (double whatever the scene's precision), the two
// lists of pixels still active (one read, one written by the compaction), and the compaction's scratch — one keep mask
// per 64 list entries, its scanned bit counts, the length of the next list.
struct AdaptiveState {
    DevBuf<int32_t> count;
    DevBuf<double> m1, m2;
    DevBuf<int32_t> list[2];
    DevBuf<uint64_t> mask;
    DevBuf<int32_t> base, n_next;
};

// The render workspace of a handle, in the precision R of its primary side: every render, feature pass and trace hook
// of the scene uses this one set (the f32 rounds of a mixed-precision render too: slot numbers and queue words do not
// depend on the precision of the records they point to).  Per-slot buffers and framebuffers grow on demand (ensure);
// queue words and counters are made once, with the handle (create).  Defined in tk_render.hip.
template <class R> struct RenderWorkspace {
    DevBuf<R> records;           // PATH_REC words per path slot
    DevBuf<float> records_f32;   // a mixed-precision render: the f32 record beside each f64 one
    DevBuf<int32_t> queue[2], shadow_queue, sorted_queue;
    DevBuf<uint8_t> sort_keys;             // one key byte per queue entry (material sort)
    DevBuf<int32_t> sort_hist, sort_base;  // [key][wave] counts and their exclusive scan
    DevBuf<R> accum, out;
    DevBuf<R> features;  // per-pixel sums of the feature pass (take_hip_render_features*): FEATURE_WORDS planes, its own — not accum
    // take_hip_render_denoised*: the filter's working images and the three guide planes (tk_denoise.hip); grows on
    // demand, is no per-slot buffer (release() leaves it, as it leaves accum, out and features) and goes with the handle
    DevBuf<R> denoise;
    int ensure_denoise(int64_t reals) {
        if ((int64_t)denoise.n >= reals || denoise.alloc((size_t)reals) == hipSuccess) return TAKE_OK;
        return fail(TAKE_E_NOMEM, "out of device memory for the denoiser's workspace");
    }
    // take_hip_render_temporal*: two accumulated frames that alternate (the history, and the one being made from it:
    // the taps gather, so a frame is never accumulated in place) and the current frame with its motion planes
    // (tk_denoise.hip has the layout); allocated by the first call, no per-slot buffers, go with the handle
    DevBuf<double> temporal[2], temporal_cur;
    // grows on demand as the denoiser's planes do, is no per-slot buffer and goes with the handle (defined in tk_render.hip)
    AdaptiveState adaptive;
    int ensure_adaptive(int64_t npix);
    DevBuf<int32_t> qwords;  // Q_NUM_WORDS + 2 * N_SORT_KEYS
    DevBuf<unsigned long long> counters;
    int64_t capacity = 0;  // path slots allocated
    hipError_t create();   // zeroed queue words and counters
    // Records and queues for `slots` paths, a framebuffer of npix pixels (0: left as it is), with f32_records one f32
    // record per slot.  A failed allocation leaves the handle WITHOUT per-slot buffers (release) and returns
    // TAKE_E_NOMEM: the next render allocates afresh instead of trusting a stale capacity over null pointers.
    int ensure(int64_t slots, int64_t npix, bool f32_records);
    void release();
};

}  // namespace tk_host

struct TakeScene {
    int precision = TAKE_PRECISION_F32;
    int device = 0;
    int num_cus = 256;
    // progressive rendering (take_hip_render_accumulate): samples per pixel summed in `accum` so far, under which options
    int64_t acc_samples = 0;
    TakeRenderOpts acc_opts{};
    bool acc_restart_needed = false;  // the scene changed (new transforms, a new camera): the next accumulate call has to restart
    int64_t n_placements = 0;         // TakeSceneDesc.n_instances of a two-level scene (0: none, or flattened at creation)
    // what take_hip_scene_set_mesh_vertices needs to know of the description the scene was created from (a replica of
    // a scene group knows none of it: groups take no updates)
    std::vector<int64_t> mesh_vertices;   // per mesh: its vertex count
    tk_host::DevBuf<int32_t> shape_face;  // TakeSceneDesc.shape_face in device memory (not of a flattened scene), shared by both sides
    // the placements' CURRENT transforms, 12 doubles each, in device memory (two-level scenes; one copy, shared by the
    // sides): written at creation and by every successful take_hip_scene_set_instance_transforms[_device].  Nothing
    // else holds them in double — take_hip_scene_update_meshes rebuilds the top level under them.
    tk_host::DevBuf<double> xforms;
    int max_leaf = 0;                     // the leaf size request the trees were built with (TakeBuildOpts / TAKE_HIP_MAX_LEAF)
    bool flattened = false;               // TAKE_INSTANCES_FLATTEN expanded placements: the meshes are no longer the caller's
    bool burley_lobes = false;            // TakeBuildOpts.burley_lobes at creation: take_hip_scene_set_materials remaps new materials the same way
    std::string node_knob;                // TAKE_HIP_NODES when the scene was built
    // take_hip_scene_mark_frame: "the previous frame" — the camera of every resident side and, in a two-level scene, a
    // copy of the placements' transforms (xforms) as they were then.  The changes of a resident scene leave it alone.
    struct FrameMark {
        bool set = false;
        tk::CameraRec<float> cam_f{};
        tk::CameraRec<double> cam_d{};
        TakeCamera camera{};  // as it was given (TakeScene::camera then): the shutter lerps the cameras, not their records
        tk_host::DevBuf<double> xforms;
        // take_hip_scene_track_vertices: the marked geometry (tk_motion_pixel.h: MarkedGeometry) of the primary side, in
        // its Real — made by the first mesh update after the mark (copy on write: until then the scene's records are the
        // marked ones), dropped by the next mark and by turning tracking off.  inst_first: per placement.
        tk_host::DevBuf<float> geom_f;
        tk_host::DevBuf<double> geom_d;
        tk_host::DevBuf<int32_t> inst_first;
        bool updated = false;  // a mesh update succeeded since the mark: the scene's records are no longer the marked ones
        bool has_geometry() const { return geom_f.p || geom_d.p; }
        void drop_geometry() { geom_f.release(), geom_d.release(), inst_first.release(); }
    } mark;
    // take_hip_scene_set_lens: the request as given, the focus distance in effect (0 until a lens is set) and what an
    // automatic focus follows — |lookat - lookfrom| of the current camera (creation, take_hip_scene_set_camera), in double
    TakeLens lens{};
    double lens_focus = 0.0, look_distance = 0.0;
    // the camera the scene was last given (creation, take_hip_scene_set_camera), as it was given: the sides keep only
    // the records derived from it, and take_hip_render_shutter* lerps the marked and the current one
    TakeCamera camera{};
    int track_flags = 0;  // take_hip_scene_track_vertices
    int temporal_history = -1;  // take_hip_render_temporal*: which of the workspace's two accumulated frames is the history (-1: none)
    int mem_share = 1;  // scenes of one group on this device: each sizes its path-state batch for 1/mem_share of the free HBM
    int instrumentation = 0;
    tk_host::SceneT<float> f;
    tk_host::SceneT<double> d;
    tk_host::RenderWorkspace<float> work_f;  // the one workspace of the handle: of an F32 scene
    tk_host::RenderWorkspace<double> work_d;  // ... of an F64 or MIXED one
    TakeCounters counters{};
    tk_host::EventPool events;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> timed;
    tk_host::PollRing poll;
    // records, images and trace hooks of a mixed-precision scene are the f64 ones (its f32 side finishes the paths)
    bool f64() const { return precision != TAKE_PRECISION_F32; }
    int width() const { return f64() ? d.host.cam.width : f.host.cam.width; }
    int height() const { return f64() ? d.host.cam.height : f.host.cam.height; }
};

namespace tk_host {

// |lookat - lookfrom| of a camera, in double: what an automatic focus (TakeLens::focus_distance <= 0) means
inline double look_distance(const TakeCamera &c) {
    const double x = c.lookat[0] - c.lookfrom[0], y = c.lookat[1] - c.lookfrom[1], z = c.lookat[2] - c.lookfrom[2];
    return std::sqrt(x * x + y * y + z * z);
}
// f(the scene's SceneT that renders, traces and reports, the handle's workspace): d for F64 and MIXED scenes, f for F32 ones
template <class TS, class F> decltype(auto) on_primary(TS *ts, F &&f) { return ts->f64() ? f(ts->d, ts->work_d) : f(ts->f, ts->work_f); }
// The sides a scene has: the f64 one (side = TAKE_PRECISION_F64) of F64 and MIXED scenes, the f32 one of F32 and MIXED ones.
// on_side: f(the named side).  for_each_side: f(every side), f64 first as creation makes them, and of `more` the same
// side with it; f returns a TAKE_* code, and the first that is not TAKE_OK ends the walk and is returned.
inline bool has_side(const TakeScene *ts, int32_t side) { return side == TAKE_PRECISION_F64 ? ts->f64() : side == TAKE_PRECISION_F32 && ts->precision != TAKE_PRECISION_F64; }
template <class TS, class F> decltype(auto) on_side(TS *ts, int32_t side, F &&f) { return side == TAKE_PRECISION_F64 ? f(ts->d) : f(ts->f); }
template <class TS, class F, class... S> int for_each_side(TS *ts, F &&f, S *...more) {
    const int rc = has_side(ts, TAKE_PRECISION_F64) ? f(ts->d, more->d...) : TAKE_OK;
    return rc || !has_side(ts, TAKE_PRECISION_F32) ? rc : f(ts->f, more->f...);
}
// A change of a resident scene (Stage = ReposeStage, MeshUpdateStage, ProtoUpdateStage): stage_side(sc, its stage) builds every side aside and leaves
// sc as it is; only when all succeeded commit() puts them in — a mixed scene gets both sides or neither — and a progressive sequence restarts.
template <template <class> class Stage, class F> int stage_then_commit(TakeScene *ts, F &&stage_side) {
    struct { Stage<double> d; Stage<float> f; } stages;  // (sides named as the scene's: for_each_side pairs them)
    if (const int rc = for_each_side(ts, stage_side, &stages)) return rc;
    ts->acc_samples = 0, ts->acc_restart_needed = true;
    return for_each_side(ts, [](auto &sc, auto &stage) { return stage.commit(sc); }, &stages);
}

// A scene lives on the device that was current when it was created; every entry point that touches it makes that
// device current for the duration of the call and restores the caller's afterwards.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};
#define TAKE_ON_DEVICE(ts)                                                                            \
    DeviceGuard guard_((ts)->device);                                                                 \
    if (!guard_.ok) return fail(TAKE_E_DEVICE, "cannot make the scene's device current")

// phase timer of scene_create (TAKE_HIP_VERBOSE=1 prints the phases to stderr)
struct PhaseClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    bool on = std::getenv("TAKE_HIP_VERBOSE") != nullptr;
    const char *side;  // "f32" / "f64": the side of the scene the phases belong to
    explicit PhaseClock(const char *side_) : side(side_) {}
    void lap(const char *what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[take_hip] scene_create: %s %-28s %8.1f ms\n", side, what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// ---- defined in tk_render.hip
// Lanes per ray of the trace kernels: one (TQ_GROUP).  Round 1 measured quad 143.6 / pair 121.5 / one ray per lane
// 128.8 ms of closest-hit time per 8.3 M samples on full-width nodes; on the 64-byte nodes one ray per lane is 9 %
// (f32) and 22 % (f64) ahead of the pair kernel.  The other group sizes stay behind -DTQ_GROUP for
// comparison builds; the quad kernel does not traverse compressed nodes.
bool compressed_nodes_supported();
// sc.trace_state: the persistent trace grid of a scene side on a device of num_cus CUs, the spill area.
template <class R> hipError_t alloc_trace_state(SceneT<R> &sc, int num_cus);
// image rows of the strips first, first + stride, ... (increasing; rows_out may be null) -> their number
int rows_of(int height, int first, int stride, int32_t *rows_out);
// first_sample / keep_accum: progressive rendering (render_impl); resolve = false: the samples are accumulated, d_out is not written
int render_scene(TakeScene *ts, const TakeRenderOpts &o, void *d_out, hipStream_t stream, int64_t first_sample = 0, bool keep_accum = false, bool resolve = true);
// a render of npix pixels into the scene's own output buffer (-> img)
int render_scene_to_out(TakeScene *ts, const TakeRenderOpts &o, int64_t npix, const void *&img);
// the first-hit feature buffers (include/take_hip.h: take_hip_render_features_device) into device memory
int render_features_scene(TakeScene *ts, const TakeRenderOpts &o, const TakeFeatureBuffers &d_out, hipStream_t stream);
// adaptive sampling (include/take_hip.h: take_hip_render_adaptive_device) into device memory; a: checked by the caller, or null
int render_adaptive_scene(TakeScene *ts, const TakeRenderOpts &o, const TakeAdaptiveOpts *a, void *d_out, const TakeAdaptiveStats &d_stats, hipStream_t stream);
// the samples every pixel of an adaptive render of o.spp > 0 samples at most gets before the first test: a's min_spp
// (null or <= 0: the default) clamped to o.spp
int adaptive_min_spp(const TakeRenderOpts &o, const TakeAdaptiveOpts *a);
// the motion pass (include/take_hip.h: take_hip_render_motion_device) into device memory, against the marked frame;
// marked = false (take_hip_render_temporal_device's first frame, which wants depth and ids only): against the current one
int render_motion_scene(TakeScene *ts, const TakeRenderOpts &o, const TakeMotionBuffers &d_out, bool marked, hipStream_t stream);
// what a render refuses of its options without looking at a scene: spp, max_depth, the integrator's range
int check_render_values(const TakeRenderOpts &o);
// path tracing of caller-supplied rays (include/take_hip.h: take_hip_render_rays_device) into device memory; d_batch:
// checked by the caller, its rays in device memory
int render_rays_scene(TakeScene *ts, const TakeRenderOpts &o, const TakeRayBatch &d_batch, void *d_out, hipStream_t stream);
// the scene's camera rays (include/take_hip.h: take_hip_camera_rays_device) into device memory; first_sample: checked by the caller
int camera_rays_scene(TakeScene *ts, const TakeRenderOpts &o, int32_t first_sample, void *d_rays_out, hipStream_t stream);
int trace_rays_host(TakeScene *ts, const void *rays, int64_t n, void *hits, int32_t *occ, bool any);
int trace_rays_device(TakeScene *ts, const void *d_rays, int64_t n, void *d_hits, bool count, hipStream_t stream);
// the distance along the view axis of what the centre ray of pixel (column, row; both inside the image) hits, 0 for a miss
int focus_distance_scene(TakeScene *ts, int32_t column, int32_t row, double *distance_out);
// the camera at scene time t between the marked and the current one (tk_shutter.h: shutter_lerp, component by component)
TakeCamera shutter_camera(const TakeCamera &marked, const TakeCamera &current, double t);
// take_hip_render_shutter* / take_hip_shutter_pose (tk_shutter.h: k_shutter_pose): the n placements' transforms, d_marked
// -> d_current (device memory, 12 doubles each), at the times[0 .. n_slices) of the shutter -> posed, n_slices * n * 12
// doubles, slice-major, allocated here; first_bad = slice * n + placement of the first pose the re-pose would refuse, -1:
// none; moved[slice] = 0 where the slice's pose is the current transforms bit for bit (no re-pose needed), 1 elsewhere
int shutter_pose_device(const double *d_marked, const double *d_current, const std::vector<double> &times, int64_t n, DevBuf<double> &posed, int64_t &first_bad,
                        std::vector<int> &moved);
// take_hip_shutter_vertices* / take_hip_render_shutter_meshes* (tk_shutter.h: k_shutter_vertices): n doubles of device
// memory, d_a (scene time 0) -> d_b (scene time 1), at time t -> d_out; *d_moved — a word of device memory, 0 before —
// becomes 1 where any of them is not d_b's bit for bit.  Launches on `stream` and returns; n <= 0 launches nothing.
void shutter_vertices_launch(const double *d_a, const double *d_b, int64_t n, double t, double *d_out, int *d_moved, int num_cus, hipStream_t stream);

// ---- defined in tk_api.hip
// what take_hip_render_adaptive* refuse of their options (null: the defaults), needing neither scene nor device
int check_adaptive_opts(const TakeAdaptiveOpts *a);
// The strips first, first + stride, ... of the scene's image a call covers, their rows and pixels: the one place that
// refuses a strip set (stride <= 0, first outside [0, stride)).  rows_out: as rows_of's.  From render options: a stride
// <= 0 means 1.
struct StripSet {
    int first = 0, stride = 1, rows = 0;
    int64_t npix = 0;
};
int strip_set(const TakeScene *ts, int first, int stride, StripSet &s, int32_t *rows_out = nullptr);
inline int strip_set(const TakeScene *ts, const TakeRenderOpts &o, StripSet &s) { return strip_set(ts, o.strip_first, o.strip_stride > 0 ? o.strip_stride : 1, s); }

// ---- defined in tk_build.hip
// The marked geometry of a side whose records are still the marked frame's (take_hip_scene_track_vertices; layout:
// tk_motion_pixel.h), made aside before a mesh update is staged: words = one entry per record of sc, inst_first = per
// placement record the first entry of its prototype (empty without placements).  TAKE_E_NOMEM with its own message.
template <class R> int copy_marked_geometry(const SceneT<R> &sc, DevBuf<R> &words, DevBuf<int32_t> &inst_first);

// What k_make_prims — and, in a two-level scene, k_make_proto_prims and k_placement_boxes — read of the caller's
// arrays, in device memory: the mesh positions as they are (double, one copy per mesh, no host staging) and the four
// shape arrays.  Uploaded once per scene: both sides of a mixed-precision scene make their records from these.
// device_positions: per mesh, positions that are in device memory already (a mesh take_hip_mesh_from_ply decoded; the
// description then holds host copies of what the host side validates and tabulates, not of these), or null
struct DeviceBuildInputs {
    DevBuf<double> pos;
    DevBuf<int32_t> kind, ref, face, area_light;
    std::vector<int64_t> pos_off;         // per mesh: its first vertex in pos
    const int32_t *face_idx = nullptr;    // the validated face indices on the device: the array of the side that uploaded them
    bool ready = false;
    int upload(const TakeSceneDesc &d, const double *const *device_positions);  // (a no-op for the second side)
    // (`face` stays: a scene keeps it resident for take_hip_scene_set_mesh_vertices / _update_meshes, 4 bytes per shape)
    void release() { pos.release(), kind.release(), ref.release(), area_light.release(); }
};
// Records and trees of one side of a new scene, made on the device (the LBVH builder, tk_build_gpu.h).  In: sc.host as
// prepare_scene(PREP_DEVICE_BUILD) leaves it; `in`: shared by the sides of the scene, uploaded by the first and released
// here by the last (last_side) — after the records of a scene without placements, so that it stays out of the build's
// peak; after the build of a two-level one, which reads the prototypes' positions.  Out: sc.prims in leaf order,
// sc.qnodes or sc.nodes, sc.face_idx, the stats, grid and placements' roots in sc.host.  compressed_ok / _forced: 64-byte
// nodes unless the grid is too coarse (Q_MAX_INFLATION) / even then.  Returns TAKE_OK, an error, or 1 = "use the host
// builder": a tree of fewer than two leaves, or too deep for the traversal stack.  Laps "mesh arrays -> HBM, records".
template <class R>
int build_side_on_device(SceneT<R> &sc, const TakeSceneDesc &d, DeviceBuildInputs &in, const double *const *device_positions, int max_leaf,
                         bool compressed_ok, bool compressed_forced, bool last_side, PhaseClock &clock);

// The three changes of a resident scene that rebuild trees, each built into a stage of its own (stage_then_commit) by a
// driver of tk_build.hip, where the steps they share are described.  A commit() returns a TAKE_* code and allocates nothing.

// What the node assembly of a resident two-level scene makes, in the node format the scene keeps: the new top-level
// tree's nodes, then the prototypes'; the top-level tree's grid (compressed nodes); the depth over both levels.
template <class R> struct ResidentNodes {
    DevBuf<Node4<R>> nodes;
    DevBuf<QNode4> qnodes;
    float grid_lo[3] = {0, 0, 0}, grid_step[3] = {1, 1, 1};
    int64_t n_nodes = 0, blas_nodes = 0;
    int depth = 0;
    std::vector<int64_t> node_first, node_count;  // per prototype, as HostScene::blas_node_first / _count
};
// The placements of a resident two-level scene under new transforms (take_hip_scene_set_instance_transforms): the
// top-level half of the device build entered a second time, reading only what the scene keeps.  d_xforms: 12 doubles
// per placement in device memory, complete; n = the scene's placements.  The prototypes' trees are copied, never
// rebuilt; who built the scene does not matter (the new top-level tree is an LBVH).  commit() copies the staged head
// records over the scene's — not every prototype's records — which fails only with a lost device.  Errors:
// TAKE_E_INVALID naming the first singular or non-finite transform, or starting with "unsupported" when the new
// top-level tree has fewer than two leaves or is too deep for the traversal stack.
template <class R> struct ReposeStage {
    ResidentNodes<R> tree;
    DevBuf<PrimRec<R>> head;     // the shapes' records in the new leaf order (the head of sc.prims)
    DevBuf<InstTrace<R>> inst_trace;
    DevBuf<InstShade<R>> inst_shade;
    int commit(SceneT<R> &sc);
};
template <class R> int repose_two_level_device(const SceneT<R> &sc, const double *d_xforms, int64_t n, ReposeStage<R> &out);

// New vertex positions (and vertex normals) for some meshes of a resident scene WITHOUT placements
// (take_hip_scene_set_mesh_vertices): the records are rewritten from what the scene keeps — its records, face_idx,
// MeshInfo, shape_face — and the tree is built again by creation's own tail (build_bvh_device), so the result is the
// bytes a fresh device build of the description with the new arrays leaves.
// MeshUpdateInputs: the new arrays in device memory, shared by the sides of the scene — host arrays uploaded (pinned in
// place, one buffer per updated array), device arrays borrowed — and per mesh of the scene a pointer or null.
struct MeshUpdateInputs {
    std::vector<DevBuf<double>> owned;
    std::vector<const double *> pos, nrm;  // per mesh: new positions / normals in device memory, null = keeps its own
    DevBuf<const double *> d_pos, d_nrm;   // the same tables in device memory
    int upload(const std::vector<int64_t> &mesh_vertices, const TakeMeshUpdate *updates, int32_t n_updates);
};
// Built into `out` (stage_then_commit).  Errors: TAKE_E_INVALID naming mesh and vertex of the first coordinate that is
// not finite, or starting with "unsupported" when the new tree has fewer than two leaves or is too deep for the
// traversal stack.  compressed_ok / _forced: as build_side_on_device.
template <class R> struct MeshUpdateStage {
    // a side of its own that creation's tail builds into: prims (leaf order), qnodes or nodes, lights and their tables,
    // host.stats / root_child / grid / q_inflation / lights / light_pmf / light_cdf, trace — and, when the node format
    // changed, the trace_state of the new kernel instance (alloc_trace_state).  (A side holds no workspace.)
    SceneT<R> built;
    // built.normals: with new normals, the scene's whole array copied and the named meshes' parts rewritten
    bool new_lights = false, new_normals = false, new_trace_state = false;
    int commit(SceneT<R> &sc);  // moves only: always TAKE_OK
};
template <class R>
int update_mesh_vertices_device(const SceneT<R> &sc, const MeshUpdateInputs &in, const std::vector<int64_t> &mesh_vertices, const int32_t *d_shape_face,
                                int max_leaf, bool compressed_ok, bool compressed_forced, int num_cus, MeshUpdateStage<R> &out);

// New vertex positions (and vertex normals) for meshes of a resident TWO-LEVEL scene (take_hip_scene_update_meshes):
// the records and tree of every prototype whose mesh is named are made again with the scene's leaf size request, the
// others' copied, and the top level is rebuilt under d_xforms — the scene's current transforms — by the resident path
// the re-pose takes.  The scene keeps its node format.  commit() only moves.  Errors: as update_mesh_vertices_device,
// the trees being the moved prototypes' and the top-level one, the depth both levels'.
// new_records (a slice of take_hip_render_shutter_meshes*): d_xforms are NOT the transforms the placements' records were
// made from — the records are made again under them, with the re-pose's refusal, so that the one top-level rebuild
// serves both the new vertices and the new pose.
template <class R> struct ProtoUpdateStage {
    // built.prims (all records), inst_trace (inst_shade: new_records), normals / lights and their tables when they change
    SceneT<R> built;
    ResidentNodes<R> tree;
    bool new_lights = false, new_normals = false;
    int blas_depth = 0;
    std::vector<int> depths;  // per prototype, as HostScene::blas_depths
    int commit(SceneT<R> &sc);  // moves only: always TAKE_OK
};
template <class R>
int update_two_level_meshes_device(const SceneT<R> &sc, const MeshUpdateInputs &in, const std::vector<int64_t> &mesh_vertices, const int32_t *d_shape_face,
                                   const double *d_xforms, int max_leaf, bool new_records, ProtoUpdateStage<R> &out);

}  // namespace tk_host

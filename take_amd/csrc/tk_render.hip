// tk_render.hip — the host side of tracing and rendering: the render workspace's allocations, the kernel launchers,
// the frame (Frame: what the launches of one call share; begin_frame / start / finish: what every call does before and
// after them), the batch step every path-traced call runs (run_batch: start_batch — the one place that decides who makes
// a batch's first rays, from the call's FirstRays — then run_rounds and accumulate_batch) and the calls that differ
// around it — the render of the camera's pixels or of caller-supplied rays (render_impl), the adaptive passes over the
// pixels still active, the feature pass and the export of the camera's rays (start_batch only), the motion pass, the
// trace hooks.
// The only unit that compiles the kernels of tk_kernels.h, tk_features.h, tk_motion.h, tk_adaptive.h, tk_shutter.h and tk_rays.h (as tk_build.hip is for tk_build_gpu.h);
// what tk_api.hip, tk_scene_update.hip, tk_create.hip and tk_group.hip (the C entry points, scene creation, groups) call here is declared
// in tk_scene_handle.h.  Host code only orchestrates: every per-sample operation runs in the kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"
#include "tk_kernels.h"
#include "tk_features.h"
#include "tk_motion.h"
#include "tk_adaptive.h"
#include "tk_shutter.h"
#include "tk_rays.h"

using namespace tk;
using namespace tk_host;

namespace {

enum TimedKernel { TK_CLOSEST, TK_SHADOW, TK_SHADE, TK_OTHER, TK_CLOSEST_TAIL /* mixed precision: closest hits of the f32 rounds */, TK_NUM };

// The trace kernel instance for (scene's traversal, any-hit, counting, Io): fn(kernel, its block geometry).  The one
// place that names an instance; the occupancy query, the launches and the spill size all come through here, so they
// cannot disagree.  Instantiated: every node format (the 8-wide one with one ray per lane only) for PathIo and HookIo;
// CameraIo for closest hits on compressed 4-wide nodes, not counting, only; CentreCameraIo (the motion pass, which has
// no generate pass to fall back on) for closest hits, not counting, on every node format.  A combination outside that
// runs nothing: false.
template <class R, bool ANY_HIT, bool COUNT, class Io, class Fn> bool with_trace_kernel(TraceKind kind, Fn &&fn) {
    constexpr bool centre = std::is_same<Io, CentreCameraIo<R>>::value;
    constexpr bool camera = std::is_same<Io, CameraIo<R>>::value || (centre && (ANY_HIT || COUNT));
    auto pick = [&](auto qn, auto width) {
        constexpr bool QN = decltype(qn)::value;
        constexpr int W = decltype(width)::value;
        if (kind.two_level) fn(k_trace_group<R, TQ_GROUP, ANY_HIT, COUNT, Io, QN, true, W>, GroupGeom<TQ_GROUP, W>{});
        else fn(k_trace_group<R, TQ_GROUP, ANY_HIT, COUNT, Io, QN, false, W>, GroupGeom<TQ_GROUP, W>{});
        return true;
    };
    if constexpr (!camera || (!ANY_HIT && !COUNT))
        if (kind.nodes == NodeFormat::Q4) return pick(std::true_type{}, std::integral_constant<int, 4>{});
    if constexpr (!camera) {
        if (kind.nodes == NodeFormat::WIDE) return pick(std::false_type{}, std::integral_constant<int, 4>{});
        if constexpr (TQ_GROUP == 1)
            if (kind.nodes == NodeFormat::Q8) return pick(std::true_type{}, std::integral_constant<int, 8>{});
    }
    return false;
}

__global__ void k_prep(int32_t *q, int next) {
    const int t = threadIdx.x;
    if (t == 0) {
        q[Q_HEAD_CLOSEST] = 0;
        q[Q_HEAD_SHADOW] = 0;
        q[Q_N_SHADOW] = 0;
        q[next ? Q_N_EXT1 : Q_N_EXT0] = 0;
    }
    if (t < 2 * N_SORT_KEYS) q[Q_NUM_WORDS + t] = 0;
}
__global__ void k_set_word(int32_t *q, int word, int32_t value) { q[word] = value; }

struct Timer {
    TakeScene *ts;
    hipStream_t stream;
    bool on;
    hipError_t err = hipSuccess;  // first failure of an event call; end_frame reports it instead of bogus times
    void begin(int which) {
        if (!on) return;
        hipEvent_t a = ts->events.get(), b = ts->events.get();
        const hipError_t e = (a && b) ? hipEventRecord(a, stream) : hipErrorOutOfMemory;
        if (e != hipSuccess && err == hipSuccess) err = e;
        ts->timed.push_back({which, {a, b}});
    }
    void end() {
        if (!on) return;
        const hipEvent_t b = ts->timed.back().second.second;
        const hipError_t e = b ? hipEventRecord(b, stream) : hipErrorOutOfMemory;
        if (e != hipSuccess && err == hipSuccess) err = e;
    }
};

// launch the trace kernel instance of a scene side for (any-hit, counting), with the side's spill area
template <class R, class Io>
hipError_t launch_trace(const SceneT<R> &sc, bool any, bool count, unsigned grid, hipStream_t stream, const Io &io, const int32_t *n_ptr,
                        int32_t n_direct, int32_t *head, unsigned long long *counters, int counter_word) {
    const TraceState &t = sc.trace_state;
    auto launch = [&](auto kernel, auto) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(TQ_BLOCK), 0, stream, sc.dev, io, n_ptr, n_direct, head, counters, counter_word,
                           StackSpill{t.spill.p, t.spill_stride});
    };
    const bool found = any ? (count ? with_trace_kernel<R, true, true, Io>(sc.trace, launch) : with_trace_kernel<R, true, false, Io>(sc.trace, launch))
                           : (count ? with_trace_kernel<R, false, true, Io>(sc.trace, launch) : with_trace_kernel<R, false, false, Io>(sc.trace, launch));
    return found ? hipSuccess : hipErrorInvalidDeviceFunction;
}

template <class R> struct ShadeArgs {
    DeviceScene<R> dev;
    RenderParams<R> rp;
    PathState<R> st;
    const int32_t *queue;
    const int32_t *n_cur;
    const int32_t *tag_count;
    int32_t *next_queue, *n_next, *shadow_queue, *n_shadow;
    int k;
    unsigned long long *counters;
    int grid;
    hipStream_t stream;
    float *to_f32;  // mixed precision, last exact round: the f32 records the continuing paths are converted into (else null)
    bool coop;      // the wave moves its paths' records as whole lines (tk_record_io.h); false: every lane its own record
};
template <class R, int TAG, bool ALT, bool COOP> void launch_shade_instance(const ShadeArgs<R> &a) {
    hipLaunchKernelGGL((k_shade<R, TAG, ALT, COOP>), dim3(a.grid), dim3(BLOCK), 0, a.stream, a.dev, a.rp, a.st, a.queue, a.n_cur, a.tag_count,
                       a.next_queue, a.n_next, a.shadow_queue, a.n_shadow, a.k, a.counters, a.to_f32);
}
template <class R, int TAG> void launch_shade_tag(const ShadeArgs<R> &a) {
    if (a.rp.integrator != 0) a.coop ? launch_shade_instance<R, TAG, true, true>(a) : launch_shade_instance<R, TAG, true, false>(a);
    else a.coop ? launch_shade_instance<R, TAG, false, true>(a) : launch_shade_instance<R, TAG, false, false>(a);
}
// the instance of a material tag 0 .. TAKE_MAT_COUNT - 1; any other tag: the miss segment's (TAG_MISS)
template <class R, int TAG = 0> void launch_shade(int tag, const ShadeArgs<R> &a) {
    if constexpr (TAG == TAKE_MAT_COUNT) launch_shade_tag<R, TAG_MISS>(a);
    else if (tag == TAG) launch_shade_tag<R, TAG>(a);
    else launch_shade<R, TAG + 1>(tag, a);
}

// Debug aid (TAKE_HIP_DUMP_SLOT=<slot>): print one path's state after every kernel of a round.
template <class R> void dump_slot(const PathState<R> &st, int64_t slot, const char *tag, int k, hipStream_t stream) {
    (void)hipStreamSynchronize(stream);
    std::fprintf(stderr, "[slot %lld] k=%d %s R:", (long long)slot, k, tag);
    R rec[PATH_REC];
    (void)hipMemcpy(rec, st.r + slot * PATH_REC, sizeof rec, hipMemcpyDeviceToHost);
    for (int c = 0; c < PATH_REC; c++)
        if (c != S_HIT && c != S_CTR && c != S_FLAGS) std::fprintf(stderr, " %.17g", (double)rec[c]);
    std::fprintf(stderr, " I:");
    for (int c : {(int)S_HIT, (int)S_CTR, (int)S_FLAGS}) std::fprintf(stderr, " %d", *reinterpret_cast<int32_t *>(&rec[c]));
    std::fprintf(stderr, "\n");
}

// What the launches of one call (a render, a feature pass, a trace hook) share: the primary side and the handle's
// workspace, the stream, timer and options, and what pick_strips / begin_frame (the calls over pixels) and start_frame
// set.  (The f32 rounds of a mixed-precision render launch on the f32 side with the same frame.)
template <class R> struct Frame {
    TakeScene *ts;
    SceneT<R> &sc;
    RenderWorkspace<R> &work;
    hipStream_t stream;
    Timer tm{ts, stream, (ts->instrumentation & 1) != 0};
    bool counting = (ts->instrumentation & 2) != 0;
    bool sort_materials = false;
    int64_t dump = -1;  // TAKE_HIP_DUMP_SLOT (or -1)
    bool shade_coop = true;  // the shade kernels' record moves (k_shade, COOP); TAKE_HIP_SHADE_COOP=0 turns it off (A/B runs)
    bool camera_in_trace = false;  // of the batch under way: round 0's trace launch makes the camera rays itself (start_batch decides, launch_closest obeys)
    int width = 0, height = 0;  // of what the call covers: the camera's image (pick_strips), or n texels in one row (pick_texels)
    int first = 0, stride = 1, n_rows = 0;  // the strips first, first + stride, ... of the image and their rows (pick_strips)
    int64_t npix = 0;                       // the pixels of those rows
    int spb = 0;                            // samples per batch
    int64_t slots = 0;                      // = spb * npix
    PathState<R> st{};
    RenderParams<R> rp{};
    int wide_grid = 0, pix_grid = 0;  // blocks of a launch over the slots / the pixels
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    unsigned long long raw[C_NUM_WORDS];  // the device counters of the call (end_frame), for the caller's own lines
};
// Round 0 of the default integrator on the default node format: no generate pass (CameraIo).  The counting instances,
// the other integrators (their shade rounds read the initial flag word) and the other node formats keep k_generate.
// So does a scene with a lens (lens: CameraRec::lens_radius > 0), whose rays k_generate_lens makes: CameraIo is the
// pinhole camera's.  TAKE_HIP_CAMERA_FUSED=0 turns it off (A/B runs).
bool camera_fused(TraceKind kind, int integrator, bool counting, bool lens) {
    static const bool enabled = !(std::getenv("TAKE_HIP_CAMERA_FUSED") && std::atoi(std::getenv("TAKE_HIP_CAMERA_FUSED")) == 0);
    return enabled && TQ_GROUP == 1 && !counting && integrator == 0 && kind.nodes == NodeFormat::Q4 && !lens;
}

// The closest hits of round k of a batch for the extend queue (k = 0: the batch's first rays — made by the launch that
// traces them where start_batch left it so, Frame::camera_in_trace).  tail: an f32 round of a mixed-precision render.
template <class RR, class R>
hipError_t launch_closest(Frame<R> &c, SceneT<RR> &sc, PathState<RR> st, const RenderParams<RR> &rp, int k, int64_t n_bound, bool tail) {
    Timer &tm = c.tm;
    int32_t *q = c.work.qwords.p;
    unsigned long long *counters = c.work.counters.p;
    const int cur = k & 1, next = cur ^ 1;
    int32_t *n_cur = q + (cur ? Q_N_EXT1 : Q_N_EXT0);
    const PathIo<RR> io_ext{sc.dev.prims, st, c.work.queue[cur].p, rp.ray_eps};
    const unsigned tgrid = sc.trace_state.grid_for(n_bound);
    hipError_t e;
    hipLaunchKernelGGL(k_prep, dim3(1), dim3(64), 0, c.stream, q, next);
    tm.begin(tail ? TK_CLOSEST_TAIL : TK_CLOSEST);
    if (k == 0 && c.camera_in_trace) {
        // (the camera rays are made by the launch that traces them: CameraIo, tk_kernels.h)
        CameraIo<RR> io_cam;
        static_cast<PathIo<RR> &>(io_cam) = io_ext;
        io_cam.cam = sc.dev.cam, io_cam.rp = rp;
        e = launch_trace(sc, false, false, tgrid, c.stream, io_cam, n_cur, 0, q + Q_HEAD_CLOSEST, counters, (int)C_RAYS_CLOSEST);
    } else {
        e = launch_trace(sc, false, c.counting, tgrid, c.stream, io_ext, n_cur, 0, q + Q_HEAD_CLOSEST, counters,
                         tail ? (int)C_RAYS_CLOSEST_TAIL : (int)C_RAYS_CLOSEST);
    }
    if (e != hipSuccess) return e;
    tm.end();
    return hipSuccess;
}

// One round k of a batch on the records of precision RR: closest hits of the extend queue, material sort, shade,
// shadow rays.  (Everything is enqueued; nothing waits.)  tail: an f32 round of a mixed-precision render; to_f32: see
// ShadeArgs.  (Long because it is the round, kernel by kernel in stream order.)
template <class RR, class R>
hipError_t launch_round(Frame<R> &c, SceneT<RR> &sc, PathState<RR> st, const RenderParams<RR> &rp, int k, int64_t n_bound, bool tail,
                        float *to_f32) {
    Timer &tm = c.tm;
    RenderWorkspace<R> &w = c.work;
    int32_t *q = w.qwords.p;
    int32_t *tag_count = q + Q_NUM_WORDS;
    const int cur = k & 1, next = cur ^ 1;
    int32_t *n_cur = q + (cur ? Q_N_EXT1 : Q_N_EXT0), *n_next = q + (next ? Q_N_EXT1 : Q_N_EXT0);
    const bool dump = !tail && c.dump >= 0 && c.dump < c.slots;  // (the slot's f64 record)
    const PathIo<RR> io_shadow{sc.dev.prims, st, w.shadow_queue.p, rp.ray_eps};
    hipError_t e = launch_closest(c, sc, st, rp, k, n_bound, tail);
    if (e != hipSuccess) return e;
    if (dump) dump_slot(st, c.dump, "after trace_closest", k, c.stream);
    const int32_t *shade_in = w.queue[cur].p;
    if (c.sort_materials) {
        tm.begin(TK_OTHER);
        // every wave of the sort gets >= 512 entries of the (bounded) queue: the one-block scan walks
        // 13 x waves counters, which must not dominate small rounds (it was 40 % of a 256x256 render)
        const int sort_grid = (int)std::max<int64_t>(1, std::min<int64_t>(c.wide_grid, (n_bound + 2047) / 2048));
        hipLaunchKernelGGL((k_sort_count<RR>), dim3(sort_grid), dim3(BLOCK), 0, c.stream, sc.dev.prims, sc.dev.inst_shade, st,
                           w.queue[cur].p, n_cur, w.sort_keys.p, w.sort_hist.p);
        hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(SORT_SCAN_THREADS), 0, c.stream, w.sort_hist.p, w.sort_base.p, tag_count,
                           sort_grid * (BLOCK / WAVE));
        hipLaunchKernelGGL(k_sort_scatter, dim3(sort_grid), dim3(BLOCK), 0, c.stream, w.queue[cur].p, n_cur, w.sort_keys.p, w.sort_base.p,
                           w.sorted_queue.p);
        tm.end();
        shade_in = w.sorted_queue.p;
    }
    tm.begin(TK_SHADE);
    {
        const int shade_grid = (int)((n_bound + BLOCK - 1) / BLOCK);
        ShadeArgs<RR> sa{sc.dev, rp, st, shade_in, n_cur, c.sort_materials ? tag_count : nullptr, w.queue[next].p,
                         n_next, w.shadow_queue.p, q + Q_N_SHADOW, k, w.counters.p, shade_grid, c.stream, to_f32, c.shade_coop};
        if (c.sort_materials) {
            // one specialised launch per material tag present in the scene + the miss segment
            for (int t = 0; t < TAKE_MAT_COUNT; t++)
                if (sc.host.tag_mask & (1u << t)) launch_shade<RR>(t, sa);
            launch_shade<RR>(TAG_MISS, sa);
        } else {
            launch_shade<RR>(sc.host.single_tag, sa);
        }
    }
    tm.end();
    if constexpr (sizeof(RR) == 8) {
        if (!TK_SHADE_RECORD && to_f32 != nullptr) {
            // mixed precision, last exact round, builds without the register copy of the record: the paths that go on
            // continue on f32 records from here — converted before this round's shadow rays, as k_shade does it
            tm.begin(TK_OTHER);
            hipLaunchKernelGGL(k_convert_state, dim3(c.wide_grid), dim3(BLOCK), 0, c.stream, st, PathState<float>{to_f32, c.slots},
                               w.queue[next].p, n_next);
            tm.end();
        }
    }
    if (dump) dump_slot(st, c.dump, "after shade", k, c.stream);
    if (k <= rp.max_depth && rp.integrator == 0) {  // integrators 1..3 trace no shadow rays
        tm.begin(TK_SHADOW);
        e = launch_trace(sc, true, c.counting, sc.trace_state.grid_for(n_bound), c.stream, io_shadow, q + Q_N_SHADOW, 0, q + Q_HEAD_SHADOW,
                         w.counters.p, (int)C_RAYS_SHADOW);
        if (e != hipSuccess) return e;
        tm.end();
        if (dump) dump_slot(st, c.dump, "after trace_shadow", k, c.stream);
    }
    return hipSuccess;
}

// the counters of a new call: zeros, and the bytes the traversal of `sc` reads per node and per primitive test
template <class R> TakeCounters fresh_counters(const SceneT<R> &sc) {
    TakeCounters c{};
    c.node_bytes = (int)node_bytes<R>(sc.trace.nodes);
    c.prim_bytes = PRIM_TEST_BYTES * (int)(sizeof(R) / 4);
    return c;
}
// the device counters of the call that has just finished -> tc (and raw, for the caller's own lines)
template <class R> int read_counters(const RenderWorkspace<R> &work, TakeCounters &tc, unsigned long long (&raw)[C_NUM_WORDS]) {
    HIP_TRY(hipMemcpy(raw, work.counters.p, sizeof raw, hipMemcpyDeviceToHost));
    tc.rays_closest = raw[C_RAYS_CLOSEST] + raw[C_RAYS_CLOSEST_TAIL];
    tc.rays_closest_f32 = raw[C_RAYS_CLOSEST_TAIL];
    tc.rays_shadow = raw[C_RAYS_SHADOW];
    tc.node_visits = raw[C_NODE_VISITS];
    tc.prim_tests = raw[C_PRIM_TESTS];
    tc.bounces = raw[C_BOUNCES];
    tc.leaf_visits = raw[C_LEAF_VISITS];
    tc.wave_node_steps = raw[C_WAVE_NODE_STEPS];
    tc.wave_leaf_steps = raw[C_WAVE_LEAF_STEPS];
    return TAKE_OK;
}

// Samples per batch of a render of npix pixels (-> spb, slots = spb * npix) with the workspace for them allocated.
// render = false (the feature pass): path records and queues only — the framebuffer, which holds a progressive
// sequence's sums, and the f32 records of a mixed scene stay as they are.
template <class R> int size_batches(const TakeScene *ts, RenderWorkspace<R> &work, const TakeRenderOpts &o, int64_t npix, int &spb, int64_t &slots, bool render) {
    // paths in flight per batch: up to 512 Mi (69 GB of f32 path state + 9 GB of queues) — bigger batches keep the
    // persistent trace grid full for more of each bounce (measured on the 1M-triangle scene, spp per batch 8 / 16 / 32 /
    // 64 / 128 / 256 = 53.2 / 57.7 / 60.3 / 61.9 | 64.5 / 64.9 / 65.5 Msamples/s), and a 288 GB device has the room;
    // capped at four fifths of what is free now (round 3: it was half — a mixed-precision render, 418 B per path, then
    // needed two batches for 256 spp at 1920x1080 and lost ~1 % to the second set of thin late rounds)
    int64_t target = (int64_t)512 << 20;
    const bool mixed_records = render && ts->precision == TAKE_PRECISION_MIXED;  // every slot has an f32 record beside its f64 one
    {
        size_t free_b = 0, total_b = 0;
        const int64_t per_path = (int64_t)PATH_REC * (int64_t)(sizeof(R) + (mixed_records ? sizeof(float) : 0)) + 4 * (int64_t)sizeof(int32_t);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const int64_t have = (int64_t)work.capacity * per_path;  // already allocated by an earlier render
            // (shards of a scene group that share a device size their batches concurrently: each takes its share)
            target = std::min<int64_t>(target, std::max<int64_t>((int64_t)1 << 20, ((int64_t)free_b / std::max(1, ts->mem_share) + have) / 5 * 4 / per_path));
        }
    }
    spb = o.samples_per_batch > 0 ? o.samples_per_batch : (int)std::max<int64_t>(1, target / npix);
    spb = std::min(spb, o.spp);
    while ((int64_t)spb * npix >= ((int64_t)1 << 31) - (1 << 26)) spb--;
    // The free-memory figure above is a snapshot: another process on the device (or another host thread) may take the
    // memory before the allocation lands.  A batch size the caller did not pin is then halved until it fits — the
    // image does not depend on it (a sample's random stream is a function of seed, pixel and sample index only).
    for (;;) {
        slots = (int64_t)spb * npix;
        const int rc = work.ensure(slots, render ? npix : 0, mixed_records);
        if (rc != TAKE_E_NOMEM || spb == 1 || o.samples_per_batch > 0) return rc;
        (void)hipGetLastError();
        spb = (spb + 1) / 2;
    }
}

// The kernels' view of a render's options, for records of precision R (a mixed-precision render makes both from here;
// s0 and spb are the batch's)
template <class R> RenderParams<R> make_params(const TakeRenderOpts &o, int W, int H, int n_rows, int first, int stride) {
    const int64_t npix = (int64_t)n_rows * W;
    RenderParams<R> rp{};
    rp.width = W, rp.height = H, rp.n_local_rows = n_rows, rp.npix = (int32_t)npix;
    rp.inv_npix = 1.0 / (double)npix, rp.inv_width = 1.0 / (double)W;
    rp.strip_first = first, rp.strip_stride = stride;
    rp.spp = o.spp, rp.max_depth = o.max_depth, rp.seed = o.seed, rp.integrator = o.integrator;
    rp.ray_eps = o.ray_epsilon > 0 ? R(o.ray_epsilon) : (sizeof(R) == 8 ? R(1e-7) : R(1e-4));
    return rp;
}

// Queue lengths read back asynchronously (PollRing: pinned word + event, polled — the launch loop never waits for the
// GPU): any value that has arrived bounds the grids of all later rounds (queues only shrink), and a zero ends the
// launching.  (Round 1 blocked on a stream sync every 4 rounds: with the ~370 launches of a small render that was a
// third of its 12 ms.)
struct QueuePoll {
    PollRing &ring;
    hipStream_t stream;
    int64_t issued = 0, done = 0;
    int post(const int32_t *d_length) {  // (skipped while the ring is full)
        if (issued - done >= PollRing::SIZE) return TAKE_OK;
        const int slot = issued % PollRing::SIZE;
        HIP_TRY(hipMemcpyAsync(ring.word + slot, d_length, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(ring.ev[slot], stream));
        issued++;
        return TAKE_OK;
    }
    // the lengths that have arrived: n_bound lowered to them, finished once one was zero
    int drain(int64_t &n_bound, bool &finished) {
        while (done < issued) {
            const int slot = done % PollRing::SIZE;
            hipError_t q = hipEventQuery(ring.ev[slot]);
            if (q == hipErrorNotReady) {
                (void)hipGetLastError();  // "not ready" is an answer, not an error: keep it out of the sticky state
                // stay at most 8 rounds ahead of the GPU: enough queued work that it never idles, close enough
                // that a batch whose paths have all ended stops being launched
                if (issued - done < 8) break;
                q = hipEventSynchronize(ring.ev[slot]);
            }
            HIP_TRY(q);
            const int32_t alive = ring.word[slot];
            done++;
            n_bound = std::min<int64_t>(n_bound, alive);
            if (alive == 0) finished = true;
        }
        return TAKE_OK;
    }
    // (outstanding read-backs of a batch complete with the stream; the ring indices just move on)
    void end_batch() { done = issued; }
};

// the event pairs of an instrumented render -> milliseconds and launch counts per kernel class
void sum_timings(const TakeScene *ts, TakeCounters &tc) {
    double acc[TK_NUM] = {0, 0, 0, 0, 0};
    for (auto &t : ts->timed) {
        float m = 0;
        if (hipEventElapsedTime(&m, t.second.first, t.second.second) == hipSuccess) acc[t.first] += m;
        if (t.first == TK_CLOSEST || t.first == TK_CLOSEST_TAIL) tc.launches_trace_closest++;
        if (t.first == TK_CLOSEST_TAIL) tc.launches_trace_closest_f32++;
        if (t.first == TK_SHADOW) tc.launches_trace_shadow++;
    }
    tc.ms_trace_closest = acc[TK_CLOSEST] + acc[TK_CLOSEST_TAIL];
    tc.ms_trace_closest_f32 = acc[TK_CLOSEST_TAIL];
    tc.ms_trace_shadow = acc[TK_SHADOW];
    tc.ms_shade = acc[TK_SHADE];
    tc.ms_other = acc[TK_OTHER];
}

// the strips the options name -> fr's first, stride, rows and pixels
template <class R> int pick_strips(Frame<R> &fr, const TakeRenderOpts &o) {
    StripSet s;
    if (const int rc = strip_set(fr.ts, o, s)) return rc;
    fr.first = s.first, fr.stride = s.stride, fr.n_rows = s.rows, fr.npix = s.npix;
    fr.width = fr.ts->width(), fr.height = fr.ts->height();
    return TAKE_OK;
}
// the same for a call over n texels that are no pixels of the camera (take_hip_render_rays*): one row of width n, so
// that slot_pixel / path_rng key texel i as pixel i
template <class R> void pick_texels(Frame<R> &fr, int64_t n) {
    fr.first = 0, fr.stride = 1;
    fr.width = (int)n, fr.height = 1, fr.n_rows = 1;
    fr.npix = n;
}
// The frame of a call over the pixels of those strips (a render; render = false: a feature pass), up to the call's own
// set-up: fresh counters, the batch size with the workspace for it, the kernels' parameters, the grids.  A strip set
// without pixels is TAKE_OK with fr.npix == 0: the caller has nothing to do.
template <class R> int begin_frame(Frame<R> &fr, const TakeRenderOpts &o, bool render) {
    TakeScene *ts = fr.ts;
    const int64_t npix = fr.npix;
    ts->counters = fresh_counters(fr.sc);
    if (render && ts->precision == TAKE_PRECISION_MIXED) ts->counters.prim_bytes = PRIM_TEST_BYTES;  // (most rounds read the f32 records)
    if (npix == 0) return TAKE_OK;
    if (npix >= ((int64_t)1 << 30)) return fail(TAKE_E_INVALID, "image too large");
    if (const int rc = size_batches(ts, fr.work, o, npix, fr.spb, fr.slots, render)) return rc;
    fr.st = PathState<R>{fr.work.records.p, fr.work.capacity};
    fr.rp = make_params<R>(o, fr.width, fr.height, fr.n_rows, fr.first, fr.stride);
    fr.wide_grid = (int)std::min<int64_t>((fr.slots + BLOCK - 1) / BLOCK, (int64_t)ts->num_cus * 8);
    fr.pix_grid = (int)std::min<int64_t>((npix + BLOCK - 1) / BLOCK, (int64_t)ts->num_cus * 8);
    return TAKE_OK;
}
// Every call, before its first launch: no timings of an earlier call, the device counters at zero, the begin event.
template <class R> int start_frame(Frame<R> &fr) {
    fr.ts->events.reset();
    fr.ts->timed.clear();
    HIP_TRY(hipMemsetAsync(fr.work.counters.p, 0, fr.work.counters.bytes(), fr.stream));
    fr.ev_begin = fr.ts->events.get(), fr.ev_end = fr.ts->events.get();
    HIP_TRY(hipEventRecord(fr.ev_begin, fr.stream));
    return TAKE_OK;
}
// Every call, after its last launch: the stream drained, then the device counters (-> fr.raw too), the call's samples
// and times -> ts->counters (fresh_counters' before the call)
template <class R> int end_frame(Frame<R> &fr, uint64_t samples) {
    HIP_TRY(hipEventRecord(fr.ev_end, fr.stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(fr.stream));
    if (fr.tm.err != hipSuccess) return fail(TAKE_E_DEVICE, std::string("kernel timing events: ") + hipGetErrorString(fr.tm.err));
    TakeCounters &tc = fr.ts->counters;
    if (const int rc = read_counters(fr.work, tc, fr.raw)) return rc;
    tc.samples = samples;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, fr.ev_begin, fr.ev_end));
    tc.ms_total = ms;
    sum_timings(fr.ts, tc);
    return TAKE_OK;
}

// Where the first rays of a call's batches come from, and how its samples are numbered: sample s of the call is sample
// first_sample + s of the random streams.
struct FirstRays {
    enum Kind {
        CAMERA,         // the camera's, of every pixel
        CAMERA_LISTED,  // the camera's, of the n_listed pixels in `list` (an adaptive pass after the first)
        CAMERA_EXPORT,  // the camera's, of every pixel, as records to be read: never left to the trace launch (the export)
        CALLER          // the caller's (take_hip_render_rays*): texel i of a one-row frame travels along ray i
    } kind = CAMERA;
    int32_t first_sample = 0;
    const int32_t *list = nullptr;  // device memory
    int32_t n_listed = 0;
    const TakeRayBatch *batch = nullptr;  // its rays in device memory
};
// The extend queue of a new batch, samples s .. s + nb - 1 of the call (-> its n paths), and its length in Q_N_EXT0:
// the identity where the closest-hit launch of round 0 makes the camera rays itself (camera_fused: the one place that
// asks, and fr.camera_in_trace is the answer launch_closest follows), else with the paths' initial records from the
// source's generator — the pinhole camera's or the lens's.  (The export runs no round: nothing reads the length.)
template <class R> int64_t start_batch(Frame<R> &fr, const FirstRays &src, int s, int nb) {
    const SceneT<R> &sc = fr.sc;
    const bool lens = sc.dev.cam.lens_radius > R(0);
    const int64_t n = (int64_t)nb * (src.kind == FirstRays::CAMERA_LISTED ? (int64_t)src.n_listed : fr.npix);
    int32_t *queue = fr.work.queue[0].p;
    const dim3 grid(fr.wide_grid), block(BLOCK);
    fr.rp.s0 = src.first_sample + s, fr.rp.spb = nb;
    fr.camera_in_trace = src.kind == FirstRays::CAMERA && camera_fused(sc.trace, fr.rp.integrator, fr.counting, lens);
    fr.tm.begin(TK_OTHER);
    if (fr.camera_in_trace) {
        hipLaunchKernelGGL(k_iota, grid, block, 0, fr.stream, queue, n);
    } else if (src.kind == FirstRays::CALLER) {
        const TakeRayBatch &b = *src.batch;
        hipLaunchKernelGGL((k_generate_rays<R>), grid, block, 0, fr.stream, (const RayRec<R> *)b.rays, fr.npix, 1.0 / (double)fr.npix,
                           b.ray_sets == 1 ? (int64_t)-1 : (int64_t)s, (int)(b.flags & TAKE_RAYS_NORMALIZE), fr.st, queue, n);
    } else if (src.kind == FirstRays::CAMERA_LISTED) {
        const dim3 list_grid((unsigned)std::min<int64_t>((n + BLOCK - 1) / BLOCK, (int64_t)fr.ts->num_cus * 8));
        const double inv_listed = 1.0 / (double)src.n_listed;
        if (lens) hipLaunchKernelGGL((ad::k_generate_list_lens<R>), list_grid, block, 0, fr.stream, sc.dev, fr.rp, fr.st, src.list, src.n_listed, inv_listed, queue, n);
        else hipLaunchKernelGGL((ad::k_generate_list<R>), list_grid, block, 0, fr.stream, sc.dev, fr.rp, fr.st, src.list, src.n_listed, inv_listed, queue, n);
    } else {
        if (lens) hipLaunchKernelGGL((k_generate_lens<R>), grid, block, 0, fr.stream, sc.dev, fr.rp, fr.st, queue, n);
        else hipLaunchKernelGGL((k_generate<R>), grid, block, 0, fr.stream, sc.dev, fr.rp, fr.st, queue, n);
    }
    if (src.kind != FirstRays::CAMERA_EXPORT) hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, fr.stream, fr.work.qwords.p, (int)Q_N_EXT0, (int32_t)n);
    fr.tm.end();
    return n;
}

// What a render refuses of its options before it looks at the strips (check_render_values: the part that needs no scene)
template <class R> int check_render_opts(const SceneT<R> &sc, const TakeRenderOpts &o) {
    if (const int rc = check_render_values(o)) return rc;
    if (o.integrator != 0 && sc.host.env.light >= 0)
        return fail(TAKE_E_INVALID, "integrators 1..3 are the reference's own: they do not know the environment-map extension");
    return TAKE_OK;
}
// What the batches of a render share beyond the frame (a render's own set-up after begin_frame: the material sort with
// its scratch, the dump slot, the f32 side of a mixed-precision render)
struct RenderLoop {
    // mixed precision (TAKE_PRECISION_MIXED): rounds k < exact_rounds on the f64 records and scene, the rest on f32
    // records of the same slots and the f32 scene
    bool mixed = false;
    int exact_rounds = 0;
    PathState<float> st32{nullptr, 0};
    RenderParams<float> rp32{};
};
template <class R> int prepare_loop(Frame<R> &fr, const TakeRenderOpts &o, RenderLoop &loop) {
    fr.sort_materials = fr.sc.host.n_material_tags > 1;
    if (const char *dump_env = std::getenv("TAKE_HIP_DUMP_SLOT")) fr.dump = std::atoll(dump_env);
    if (const char *coop_env = std::getenv("TAKE_HIP_SHADE_COOP")) fr.shade_coop = std::atoi(coop_env) != 0;  // read per call: a test flips it
    if (fr.sort_materials) {
        const size_t need = (size_t)N_SORT_KEYS * fr.wide_grid * (BLOCK / WAVE);
        if (fr.work.sort_hist.n != need) {
            HIP_TRY(fr.work.sort_hist.alloc(need));
            HIP_TRY(fr.work.sort_base.alloc(need));
        }
    }
    loop.mixed = sizeof(R) == 8 && fr.ts->precision == TAKE_PRECISION_MIXED;
    if (loop.mixed) {
        loop.exact_rounds = o.exact_bounces > 0 ? o.exact_bounces : TAKE_DEFAULT_EXACT_BOUNCES;
        if (o.integrator != 0) return fail(TAKE_E_INVALID, "mixed precision renders the reference's path_tracing (integrator 0) only");
        loop.st32 = PathState<float>{fr.work.records_f32.p, fr.slots};
        loop.rp32 = make_params<float>(o, fr.rp.width, fr.rp.height, fr.n_rows, fr.first, fr.stride);
    }
    return TAKE_OK;
}
// The rounds of one batch whose extend queue holds n paths (fr.rp.s0 / spb: the batch's): launched until the queue is
// known to be empty, never waiting for the GPU (QueuePoll)
template <class R> int run_rounds(Frame<R> &fr, RenderLoop &loop, int max_depth, int64_t n, QueuePoll &poll) {
    TakeScene *ts = fr.ts;
    loop.rp32.s0 = fr.rp.s0, loop.rp32.spb = fr.rp.spb;
    const int rounds = max_depth + 2;
    int64_t n_bound = n;  // upper bound of the extend-queue length (queues only shrink)
    bool finished = false;
    for (int k = 0; k < rounds && !finished; k++) {
        // mixed precision: the paths still alive after the last exact shade round continue on f32 records (and
        // the f32 scene) — converted by that round (k_shade, to_f32; k_convert_state without TK_SHADE_RECORD)
        if (loop.mixed && k >= loop.exact_rounds) HIP_TRY(launch_round(fr, ts->f, loop.st32, loop.rp32, k, n_bound, true, nullptr));
        else HIP_TRY(launch_round(fr, fr.sc, fr.st, fr.rp, k, n_bound, false, (loop.mixed && k == loop.exact_rounds - 1) ? loop.st32.r : nullptr));
        int rc = TAKE_OK;
        if (k + 1 < rounds) rc = poll.post(fr.work.qwords.p + (k & 1 ? Q_N_EXT0 : Q_N_EXT1));  // the length of the next round's queue
        if (!rc) rc = poll.drain(n_bound, finished);
        if (rc) return rc;
    }
    poll.end_batch();
    return TAKE_OK;
}

// The nb samples a batch has finished, from its path records (the f64 and f32 ones of a mixed-precision render) into
// the accumulator.  stats (the adaptive sampler's): also the counts and moments, of the source's listed pixels only
// (no list: of every pixel).
template <class R> void accumulate_batch(Frame<R> &fr, const RenderLoop &loop, const FirstRays &src, int nb, AdaptiveState *stats) {
    R *accum = fr.work.accum.p;
    const int32_t npix = (int32_t)fr.npix, n_listed = src.list ? src.n_listed : npix;
    const dim3 grid(stats ? (unsigned)std::min<int64_t>(((int64_t)n_listed + BLOCK - 1) / BLOCK, (int64_t)fr.ts->num_cus * 8) : (unsigned)fr.pix_grid), block(BLOCK);
    fr.tm.begin(TK_OTHER);
    // (loop.mixed is false for f32 records; the mixed kernels are compiled for f64 ones only)
    if (stats) {
        if constexpr (sizeof(R) == 8)
            if (loop.mixed) hipLaunchKernelGGL(ad::k_accumulate_stats_mixed, grid, block, 0, fr.stream, fr.st, loop.st32, accum, stats->count.p, stats->m1.p, stats->m2.p, src.list, n_listed, npix, nb);
        if (!loop.mixed) hipLaunchKernelGGL((ad::k_accumulate_stats<R>), grid, block, 0, fr.stream, fr.st, accum, stats->count.p, stats->m1.p, stats->m2.p, src.list, n_listed, npix, nb);
    } else {
        if constexpr (sizeof(R) == 8)
            if (loop.mixed) hipLaunchKernelGGL(k_accumulate_mixed, grid, block, 0, fr.stream, fr.st, loop.st32, accum, npix, nb);
        if (!loop.mixed) hipLaunchKernelGGL((k_accumulate<R>), grid, block, 0, fr.stream, fr.st, accum, npix, nb);
    }
    fr.tm.end();
}
// One batch of a path-traced call, samples s .. s + nb - 1 of it: the first rays, the rounds, the accumulate
template <class R>
int run_batch(Frame<R> &fr, RenderLoop &loop, const FirstRays &src, int s, int nb, int max_depth, QueuePoll &poll, AdaptiveState *stats = nullptr) {
    const int64_t n = start_batch(fr, src, s, nb);
    if (const int rc = run_rounds(fr, loop, max_depth, n, poll)) return rc;
    accumulate_batch(fr, loop, src, nb, stats);
    return TAKE_OK;
}

// A render of the camera's pixels (take_hip_render*, src.kind = CAMERA) or of the caller's rays (take_hip_render_rays*,
// CALLER; contract: include/take_hip.h, kernels: tk_rays.h) — then a frame of n texels in one row instead of the strips'
// pixels, so that the unchanged path_rng keys sample s of ray i as rng_key(seed, i, first_sample + s), and one row,
// which k_resolve does not flip.
// src.first_sample / keep_accum: progressive rendering — the samples of this call are numbered from first_sample (their
// random streams are those of a one-shot render's samples first_sample .. first_sample + spp - 1), keep_accum adds them
// to what `accum` holds instead of starting from zero, and the image is the mean over first_sample + spp samples (the
// camera's; the caller's rays only number their samples from first_sample: the mean is over spp) — written unless
// resolve is false (all but the last slice of take_hip_render_shutter*: the accumulator is the result).
// (What is a render's own between the frame's steps: its checks, the batch loop and resolve.)
template <class R> int render_impl(TakeScene *ts, SceneT<R> &sc, RenderWorkspace<R> &work, const TakeRenderOpts &o, const FirstRays &src, void *d_out,
                                   hipStream_t stream, bool keep_accum, bool resolve) {
    const bool camera = src.kind == FirstRays::CAMERA;
    if (!keep_accum) ts->acc_samples = 0;  // (a one-shot render overwrites the accumulator: a progressive sequence ends)
    if (const int rc = check_render_opts(sc, o)) return rc;
    Frame<R> fr{ts, sc, work, stream};
    int rc = TAKE_OK;
    if (camera) rc = pick_strips(fr, o);
    else pick_texels(fr, src.batch->n);
    if (!rc) rc = begin_frame(fr, o, true);
    const int64_t npix = fr.npix;
    if (rc || npix == 0) return rc;
    RenderLoop loop;
    if ((rc = prepare_loop(fr, o, loop))) return rc;
    if (!keep_accum) HIP_TRY(hipMemsetAsync(work.accum.p, 0, sizeof(R) * 3 * npix, stream));
    if ((rc = start_frame(fr))) return rc;
    HIP_TRY(ts->poll.create());
    QueuePoll poll{ts->poll, stream};

    for (int s = 0; s < o.spp; s += fr.spb)
        if ((rc = run_batch(fr, loop, src, s, std::min(fr.spb, o.spp - s), o.max_depth, poll))) return rc;
    fr.tm.begin(TK_OTHER);
    if (resolve) hipLaunchKernelGGL((k_resolve<R>), dim3(fr.pix_grid), dim3(BLOCK), 0, stream, work.accum.p, (R *)d_out, fr.rp.width, fr.n_rows,
                                    (camera ? src.first_sample : 0) + o.spp);
    fr.tm.end();
    if ((rc = end_frame(fr, (uint64_t)npix * (uint64_t)o.spp))) return rc;
    if (camera && std::getenv("TAKE_HIP_VERBOSE"))
        std::fprintf(stderr, "[take_hip] node-step ray slots: waiting-at-leaf %llu idle %llu running %llu; shadow rays the slot's previous occluder stops again: %llu of %llu\n",
                     fr.raw[C_WAIT_SLOTS], fr.raw[C_IDLE_SLOTS], fr.raw[C_NODE_VISITS], fr.raw[C_OCC_CACHE_HITS], fr.raw[C_RAYS_SHADOW]);
    return TAKE_OK;
}

// TakeAdaptiveOpts (null: all defaults) with the defaults filled in, for a render of o.spp > 0 samples at most
ad::Rule make_rule(const TakeRenderOpts &o, const TakeAdaptiveOpts *a) {
    ad::Rule r{o.spp, 16, 8, 0.05, 1e-3};
    if (a && a->min_spp > 0) r.min_spp = a->min_spp;
    if (a && a->step_spp > 0) r.step_spp = a->step_spp;
    if (a && a->threshold >= 0) r.threshold = a->threshold;
    if (a && a->floor > 0) r.floor = a->floor;
    r.min_spp = std::min(r.min_spp, o.spp);
    return r;
}

// Adaptive sampling (take_hip_render_adaptive*; contract: include/take_hip.h, kernels: tk_adaptive.h).  Pass 0 is a
// render's batches over min_spp samples of every pixel; every later pass is the same batches with the pixels still
// active as the source of their first rays (FirstRays::CAMERA_LISTED: k_generate_list).  Path records stay
// addressed by sample * npix + pixel, so the workspace is sized for max(min_spp, step_spp) samples of all pixels and
// a pass that does not fit is split into batches — which is what keeps slot_pixel / path_rng, and with them every shade
// instance, untouched.  After each pass: accumulate + moments, the test, the ordered compaction, and the length of the
// next list read back (one 4-byte copy and one synchronisation: the next pass's grid and reciprocal need it).
template <class R>
int adaptive_impl(TakeScene *ts, SceneT<R> &sc, RenderWorkspace<R> &work, const TakeRenderOpts &o, const TakeAdaptiveOpts *ao, void *d_out,
                  const TakeAdaptiveStats &stats, hipStream_t stream) {
    ts->acc_samples = 0;  // (the accumulator is overwritten: a progressive sequence ends)
    if (const int rc = check_render_opts(sc, o)) return rc;
    const ad::Rule rule = make_rule(o, ao);
    if (o.integrator != 0) return fail(TAKE_E_INVALID, "adaptive sampling renders the reference's path_tracing (integrator 0) only");
    Frame<R> fr{ts, sc, work, stream};
    int rc = pick_strips(fr, o);
    TakeRenderOpts sized = o;  // the batches hold the samples of one pass, not of the whole render
    sized.spp = std::min(o.spp, std::max(rule.min_spp, rule.step_spp));
    if (!rc) rc = begin_frame(fr, sized, true);
    const int64_t npix = fr.npix;
    if (rc || npix == 0) return rc;
    RenderLoop loop;
    if ((rc = prepare_loop(fr, o, loop))) return rc;
    if ((rc = work.ensure_adaptive(npix))) return rc;
    AdaptiveState &a = work.adaptive;
    HIP_TRY(hipMemsetAsync(work.accum.p, 0, sizeof(R) * 3 * npix, stream));
    HIP_TRY(hipMemsetAsync(a.count.p, 0, sizeof(int32_t) * npix, stream));
    HIP_TRY(hipMemsetAsync(a.m1.p, 0, sizeof(double) * npix, stream));
    HIP_TRY(hipMemsetAsync(a.m2.p, 0, sizeof(double) * npix, stream));
    if ((rc = start_frame(fr))) return rc;
    HIP_TRY(ts->poll.create());
    QueuePoll poll{ts->poll, stream};

    uint64_t samples = 0;
    const int32_t *list = nullptr;  // (pass 0: every pixel)
    int32_t n_active = (int32_t)npix;
    for (int pass = 0, n = 0; n_active > 0 && n < o.spp; pass++) {
        const int add = pass == 0 ? rule.min_spp : std::min(rule.step_spp, o.spp - n);
        const int list_grid = (int)std::min<int64_t>(((int64_t)n_active + BLOCK - 1) / BLOCK, (int64_t)ts->num_cus * 8);
        FirstRays src;
        if (pass > 0) src.kind = FirstRays::CAMERA_LISTED, src.list = list, src.n_listed = n_active;
        for (int done = 0; done < add; done += fr.spb)
            if ((rc = run_batch(fr, loop, src, n + done, std::min(fr.spb, add - done), o.max_depth, poll, &a))) return rc;
        n += add;
        samples += (uint64_t)n_active * (uint64_t)add;
        if (n >= o.spp) break;  // (every pixel still active has spp samples: it stops)
        // the test, and the pixels it keeps in ascending order -> the other list
        int32_t *next = a.list[pass & 1].p;
        fr.tm.begin(TK_OTHER);
        hipLaunchKernelGGL(ad::k_adaptive_select, dim3((unsigned)(((int64_t)n_active + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, rule, a.count.p, a.m1.p, a.m2.p, list,
                           n_active, a.mask.p);
        hipLaunchKernelGGL(ad::k_compact_scan, dim3(1), dim3(ad::SCAN_THREADS), 0, stream, a.mask.p, ad::groups_of(n_active), a.base.p, a.n_next.p);
        hipLaunchKernelGGL(ad::k_compact_scatter, dim3(list_grid), dim3(BLOCK), 0, stream, list, a.mask.p, a.base.p, n_active, next);
        fr.tm.end();
        int32_t kept = 0;
        HIP_TRY(hipMemcpyAsync(&kept, a.n_next.p, sizeof kept, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (kept < 0 || kept > n_active) return fail(TAKE_E_DEVICE, "adaptive sampling: the compacted list is longer than the list it came from");
        n_active = kept, list = next;
    }
    fr.tm.begin(TK_OTHER);
    hipLaunchKernelGGL((ad::k_resolve_adaptive<R>), dim3(fr.pix_grid), dim3(BLOCK), 0, stream, work.accum.p, a.count.p, a.m1.p, a.m2.p, (R *)d_out, stats.count, stats.m1,
                       stats.m2, fr.rp.width, fr.n_rows);
    fr.tm.end();
    return end_frame(fr, samples);
}

// The first-hit feature buffers of a scene (take_hip_render_features*; contract: include/take_hip.h): per batch the
// camera + closest-hit launch of a render's round 0, then k_features over the batch's records; sums of its own
// (work.features), so a progressive sequence — its accumulator and sample count — goes on afterwards.  The timer files
// k_features under the shade class: after the call ms_shade is its time.
template <class R>
int features_impl(TakeScene *ts, SceneT<R> &sc, RenderWorkspace<R> &work, const TakeRenderOpts &opts, const TakeFeatureBuffers &b, hipStream_t stream) {
    if (opts.spp <= 0) return fail(TAKE_E_INVALID, "spp must be positive");
    Frame<R> fr{ts, sc, work, stream};
    if (const int rc = pick_strips(fr, opts)) return rc;
    const FeatureOut<R> out{(R *)b.albedo, (R *)b.normal, (R *)b.depth, (R *)b.alpha, b.shape_id, b.material_id};
    const uint32_t want = out.want();
    if (want == 0) return fail(TAKE_E_INVALID, "no feature buffer was asked for: every pointer of TakeFeatureBuffers is NULL");
    TakeRenderOpts o = opts;
    o.max_depth = 0, o.integrator = 0, o.exact_bounces = 0;  // (ignored by this pass: the camera rays do not depend on them)
    int rc = begin_frame(fr, o, false);
    const int64_t npix = fr.npix;
    if (rc || npix == 0) return rc;
    if ((int64_t)work.features.n < FEATURE_WORDS * npix && work.features.alloc((size_t)FEATURE_WORDS * npix) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for the feature accumulators");
    HIP_TRY(hipMemsetAsync(work.features.p, 0, sizeof(R) * FEATURE_WORDS * npix, stream));
    if ((rc = start_frame(fr))) return rc;
    for (int s0 = 0; s0 < o.spp; s0 += fr.spb) {
        const int nb = std::min(fr.spb, o.spp - s0);
        const int64_t n = start_batch(fr, FirstRays{}, s0, nb);
        HIP_TRY(launch_closest(fr, sc, fr.st, fr.rp, 0, n, false));
        fr.tm.begin(TK_SHADE);
        hipLaunchKernelGGL((k_features<R>), dim3(fr.pix_grid), dim3(BLOCK), 0, stream, sc.dev, fr.st, work.features.p, out, fr.rp.width, fr.n_rows, nb, s0 == 0 ? 1 : 0, want);
        fr.tm.end();
    }
    fr.tm.begin(TK_OTHER);
    hipLaunchKernelGGL((k_features_resolve<R>), dim3(fr.pix_grid), dim3(BLOCK), 0, stream, work.features.p, out, fr.rp.width, fr.n_rows, o.spp);
    fr.tm.end();
    return end_frame(fr, (uint64_t)npix * (uint64_t)o.spp);
}

// The scene's own camera rays (take_hip_camera_rays*): per batch the first rays of a whole-image render as records
// (FirstRays::CAMERA_EXPORT: the pinhole camera's or the lens's generate pass), then k_export_rays over them.  Path
// records and queues only, as the feature pass: a progressive sequence goes on afterwards.  d_out: opts.spp sets of
// W * H records, sample-major.
template <class R> int camera_rays_impl(TakeScene *ts, SceneT<R> &sc, RenderWorkspace<R> &work, const TakeRenderOpts &opts, int32_t first_sample, void *d_out, hipStream_t stream) {
    if (opts.spp <= 0) return fail(TAKE_E_INVALID, "spp must be positive");
    Frame<R> fr{ts, sc, work, stream};
    TakeRenderOpts o{};  // (of the options only seed, spp and ray_epsilon are read: the whole image)
    o.spp = opts.spp, o.seed = opts.seed, o.ray_epsilon = opts.ray_epsilon, o.strip_first = 0, o.strip_stride = 1;
    if (const int rc = pick_strips(fr, o)) return rc;
    int rc = begin_frame(fr, o, false);
    const int64_t npix = fr.npix;
    if (rc || npix == 0) return rc;
    if ((rc = start_frame(fr))) return rc;
    FirstRays src;
    src.kind = FirstRays::CAMERA_EXPORT, src.first_sample = first_sample;
    for (int s0 = 0; s0 < o.spp; s0 += fr.spb) {
        const int64_t n = start_batch(fr, src, s0, std::min(fr.spb, o.spp - s0));
        fr.tm.begin(TK_OTHER);  // (a second interval of the class beside start_batch's: with timing on, one more event pair per batch)
        hipLaunchKernelGGL((k_export_rays<R>), dim3(fr.wide_grid), dim3(BLOCK), 0, stream, fr.st, (RayRec<R> *)d_out + (int64_t)s0 * npix, n, fr.rp.ray_eps);
        fr.tm.end();
    }
    return end_frame(fr, (uint64_t)npix * (uint64_t)o.spp);
}

// The motion pass of a scene (take_hip_render_motion*; contract: include/take_hip.h): one closest-hit launch over the
// whole image that makes the centre rays itself (CentreCameraIo: the work list is the identity, no queue is read),
// then k_motion over its records.  Path records and queue words only, as the feature pass: a progressive sequence goes
// on afterwards.  marked / marked_xforms: the camera and the placements' transforms the points are taken back to.
// geom: the marked geometry the handle holds (words null: none — the instance that follows no vertices).
// The timer files k_motion under the shade class.
template <class R>
int motion_impl(TakeScene *ts, SceneT<R> &sc, RenderWorkspace<R> &work, const TakeRenderOpts &opts, const TakeMotionBuffers &b, const CameraRec<R> &marked,
                const double *marked_xforms, const MarkedGeometry<R> &geom, hipStream_t stream) {
    const MotionOut<R> out{(R *)b.prev_xy, (R *)b.prev_depth, (R *)b.depth, b.shape_id};
    if (!out.prev_xy && !out.prev_depth && !out.depth && !out.shape_id)
        return fail(TAKE_E_INVALID, "no motion buffer was asked for: every pointer of TakeMotionBuffers is NULL");
    Frame<R> fr{ts, sc, work, stream};
    TakeRenderOpts o{};  // (of the options only ray_epsilon is read: one sample per pixel, the whole image)
    o.spp = 1, o.strip_first = 0, o.strip_stride = 1, o.ray_epsilon = opts.ray_epsilon;
    if (const int rc = pick_strips(fr, o)) return rc;
    int rc = begin_frame(fr, o, false);
    const int64_t npix = fr.npix;
    if (rc || npix == 0) return rc;
    if ((rc = start_frame(fr))) return rc;
    fr.rp.s0 = 0, fr.rp.spb = 1;
    int32_t *q = work.qwords.p;
    hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, stream, q, (int)Q_N_EXT0, (int32_t)npix);
    hipLaunchKernelGGL(k_prep, dim3(1), dim3(64), 0, stream, q, 1);
    fr.tm.begin(TK_CLOSEST);
    CentreCameraIo<R> io;
    static_cast<PathIo<R> &>(io) = PathIo<R>{sc.dev.prims, fr.st, work.queue[0].p, fr.rp.ray_eps};
    io.cam = sc.dev.cam, io.rp = fr.rp;
    HIP_TRY(launch_trace(sc, false, false, sc.trace_state.grid_for(npix), stream, io, q + Q_N_EXT0, 0, q + Q_HEAD_CLOSEST, work.counters.p, (int)C_RAYS_CLOSEST));
    fr.tm.end();
    fr.tm.begin(TK_SHADE);
    const double *xf = sc.dev.inst_trace ? marked_xforms : nullptr;
    if (geom.words) hipLaunchKernelGGL((k_motion<R, true>), dim3(fr.pix_grid), dim3(BLOCK), 0, stream, sc.dev, fr.st, marked, xf, geom, out, fr.rp.width, fr.n_rows);
    else hipLaunchKernelGGL((k_motion<R, false>), dim3(fr.pix_grid), dim3(BLOCK), 0, stream, sc.dev, fr.st, marked, xf, geom, out, fr.rp.width, fr.n_rows);
    fr.tm.end();
    return end_frame(fr, (uint64_t)npix);
}

template <class R>
int trace_impl(TakeScene *ts, SceneT<R> &sc, RenderWorkspace<R> &work, const void *d_rays, int64_t n, void *d_hits, int32_t *d_occ, bool any,
               bool count, hipStream_t stream) {
    if (n < 0 || n >= ((int64_t)1 << 31) - (1 << 26)) return fail(TAKE_E_INVALID, "ray count out of range");
    Frame<R> fr{ts, sc, work, stream};
    int32_t *q = work.qwords.p;
    HIP_TRY(hipMemsetAsync(q + Q_HEAD_CLOSEST, 0, sizeof(int32_t), stream));
    if (const int rc = start_frame(fr)) return rc;
    const HookIo<R> io{sc.dev.prims, (const RayAoS<R> *)d_rays, (HitAoS<R> *)d_hits, d_occ, sc.dev.inst_shade};
    HIP_TRY(launch_trace(sc, any, count, (unsigned)sc.trace_state.trace_grid, stream, io, nullptr, (int32_t)n, q + Q_HEAD_CLOSEST, work.counters.p, -1));
    TakeCounters &tc = ts->counters = fresh_counters(sc);
    if (const int rc = end_frame(fr, 0)) return rc;  // (the hooks count no rays on the device: n of the one kind)
    (any ? tc.rays_shadow : tc.rays_closest) = (uint64_t)n;
    (any ? tc.ms_trace_shadow : tc.ms_trace_closest) = tc.ms_total;
    (any ? tc.launches_trace_shadow : tc.launches_trace_closest) = 1;
    return TAKE_OK;
}

template <class R> int trace_host(TakeScene *ts, SceneT<R> &sc, RenderWorkspace<R> &work, const void *rays, int64_t n, void *hits, int32_t *occ, bool any) {
    if (n == 0) return TAKE_OK;
    // entry distances are ordered through their bit patterns (non-negative floats): a ray must start at tmin >= 0
    for (int64_t i = 0; i < n; i++) {
        const RayAoS<R> &q = ((const RayAoS<R> *)rays)[i];
        if (!(q.tmin >= R(0))) return fail(TAKE_E_INVALID, "ray " + std::to_string(i) + ": tmin must be >= 0");
    }
    DevBuf<RayAoS<R>> d_rays;
    DevBuf<HitAoS<R>> d_hits;
    DevBuf<int32_t> d_occ;
    HIP_TRY(d_rays.alloc(n));
    if (hipMemcpy(d_rays.p, rays, n * sizeof(RayAoS<R>), hipMemcpyHostToDevice) != hipSuccess)
        return fail(TAKE_E_DEVICE, "ray upload failed");
    if (any ? d_occ.alloc(n) != hipSuccess : d_hits.alloc(n) != hipSuccess) return fail(TAKE_E_NOMEM, "hit buffer allocation failed");
    const int rc = trace_impl(ts, sc, work, d_rays.p, n, d_hits.p, d_occ.p, any, false, nullptr);
    if (rc) return rc;
    hipError_t e = any ? hipMemcpy(occ, d_occ.p, n * sizeof(int32_t), hipMemcpyDeviceToHost)
                       : hipMemcpy(hits, d_hits.p, n * sizeof(HitAoS<R>), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(TAKE_E_DEVICE, "hit download failed");
    return TAKE_OK;
}

// take_hip_debug_env on one side of a scene (n <= 2^31 rows, checked by the caller: the grid size fits an unsigned)
template <class R> int debug_env_side(SceneT<R> &sc, int kind, const double *in, int64_t n, double *out) {
    if (sc.host.env.light < 0) return fail(TAKE_E_INVALID, "the scene has no environment map");
    if (n == 0) return TAKE_OK;
    DevBuf<double> d_in, d_out;
    if (d_in.alloc((size_t)n * ENV_IN_COLS[kind]) != hipSuccess || d_out.alloc((size_t)n * ENV_OUT_COLS[kind]) != hipSuccess)
        return fail(TAKE_E_NOMEM, "debug env allocation failed");
    HIP_TRY(hipMemcpy(d_in.p, in, d_in.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_out.p, 0, d_out.bytes()));
    hipLaunchKernelGGL((k_debug_env<R>), dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, nullptr, sc.dev, kind, d_in.p, n, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}
}  // namespace

namespace tk_host {

bool compressed_nodes_supported() { return TQ_GROUP <= 2; }

// The grid is resident blocks of the instance the render's closest-hit rounds run x CUs.  Blocks per CU: the
// occupancy of that instance, asked once per scene — a replica arrives with its source's figure.
template <class R> hipError_t alloc_trace_state(SceneT<R> &sc, int num_cus) {
    TraceState &t = sc.trace_state;
    hipError_t e = hipSuccess;
    int rays_per_block = 0;
    const bool found = with_trace_kernel<R, false, false, PathIo<R>>(sc.trace, [&](auto kernel, auto geom) {
        rays_per_block = geom.GROUPS, t.spill_levels = geom.SPILL;
        if (t.blocks_per_cu > 0) return;
        int per_cu = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, TQ_BLOCK, 0);
        per_cu = std::max(1, std::min(per_cu, 8));
        if (const char *env = std::getenv("TAKE_HIP_TRACE_BLOCKS")) per_cu = std::max(1, std::min(per_cu, std::atoi(env)));  // experiment: leave room for a concurrent kernel
        t.blocks_per_cu = per_cu;
    });
    if (e != hipSuccess) return e;
    if (!found) return hipErrorInvalidDeviceFunction;
    t.trace_grid = num_cus * t.blocks_per_cu;
    t.spill_stride = (int64_t)t.trace_grid * rays_per_block;
    return t.spill.alloc((size_t)t.spill_stride * t.spill_levels);
}
template hipError_t alloc_trace_state<float>(SceneT<float> &, int);
template hipError_t alloc_trace_state<double>(SceneT<double> &, int);

template <class R> hipError_t RenderWorkspace<R>::create() {
    hipError_t e = qwords.alloc(Q_NUM_WORDS + 2 * N_SORT_KEYS);
    if (e == hipSuccess) e = counters.alloc(C_NUM_WORDS);
    if (e == hipSuccess) e = hipMemset(qwords.p, 0, qwords.bytes());
    return e != hipSuccess ? e : hipMemset(counters.p, 0, counters.bytes());
}
// (the f32 records of a mixed-precision render stay: they are sized on their own, below)
template <class R> void RenderWorkspace<R>::release() {
    records.release(), queue[0].release(), queue[1].release(), shadow_queue.release();
    sorted_queue.release(), sort_keys.release();
    capacity = 0;
}
// (in this order: the allocation-failure tests count the allocations)
template <class R> int RenderWorkspace<R>::ensure(int64_t slots, int64_t npix, bool f32_records) {
    if (slots > capacity) {
        release();
        const bool ok = records.alloc((size_t)PATH_REC * slots) == hipSuccess && queue[0].alloc(slots) == hipSuccess &&
                        queue[1].alloc(slots) == hipSuccess && shadow_queue.alloc(slots) == hipSuccess &&
                        sorted_queue.alloc(slots) == hipSuccess && sort_keys.alloc(slots) == hipSuccess;
        if (!ok) {
            release();
            return fail(TAKE_E_NOMEM, "out of device memory for " + std::to_string(slots) + " path slots (" +
                                          std::to_string((size_t)slots * (PATH_REC * sizeof(R) + 17) >> 20) + " MiB)");
        }
        capacity = slots;
    }
    if ((int64_t)accum.n < 3 * npix) {
        if (accum.alloc(3 * npix) != hipSuccess || out.alloc(3 * npix) != hipSuccess) {
            accum.release(), out.release();
            return fail(TAKE_E_NOMEM, "out of device memory for the framebuffer");
        }
    }
    if (f32_records && (int64_t)records_f32.n < (int64_t)PATH_REC * slots && records_f32.alloc((size_t)PATH_REC * slots) != hipSuccess) {
        release();  // (a failed alloc has released records_f32 itself)
        return fail(TAKE_E_NOMEM, "out of device memory for the f32 path records of a mixed-precision render (" + std::to_string(slots) + " path slots)");
    }
    return TAKE_OK;
}
template <class R> int RenderWorkspace<R>::ensure_adaptive(int64_t npix) {
    AdaptiveState &a = adaptive;
    if ((int64_t)a.count.n >= npix) return TAKE_OK;
    const size_t n = (size_t)npix, groups = (size_t)ad::groups_of(npix);
    const bool ok = a.count.alloc(n) == hipSuccess && a.m1.alloc(n) == hipSuccess && a.m2.alloc(n) == hipSuccess && a.list[0].alloc(n) == hipSuccess &&
                    a.list[1].alloc(n) == hipSuccess && a.mask.alloc(groups) == hipSuccess && a.base.alloc(groups) == hipSuccess && a.n_next.alloc(1) == hipSuccess;
    if (ok) return TAKE_OK;
    a = AdaptiveState{};
    return fail(TAKE_E_NOMEM, "out of device memory for the adaptive sampler's per-pixel state");
}
template struct RenderWorkspace<float>;
template struct RenderWorkspace<double>;

int rows_of(int height, int first, int stride, int32_t *rows_out) {
    const int n_strips = (height + TILE_ROWS - 1) / TILE_ROWS;
    int n = 0;
    std::vector<int> ys;
    for (int s = first; s < n_strips; s += stride)
        for (int y = s * TILE_ROWS; y < std::min(height, (s + 1) * TILE_ROWS); y++) ys.push_back(y);
    n = (int)ys.size();
    if (rows_out)
        for (int j = 0; j < n; j++) rows_out[j] = height - 1 - ys[n - 1 - j];  // increasing image row
    return n;
}

int render_scene(TakeScene *ts, const TakeRenderOpts &o, void *d_out, hipStream_t stream, int64_t first_sample, bool keep_accum, bool resolve) {
    FirstRays camera;
    camera.first_sample = (int32_t)first_sample;
    return on_primary(ts, [&](auto &sc, auto &work) { return render_impl(ts, sc, work, o, camera, d_out, stream, keep_accum, resolve); });
}
int render_scene_to_out(TakeScene *ts, const TakeRenderOpts &o, int64_t npix, const void *&img) {
    return on_primary(ts, [&](auto &sc, auto &work) {
        int rc = work.ensure(0, npix, false);
        if (!rc) rc = render_impl(ts, sc, work, o, FirstRays{}, work.out.p, nullptr, false, true);
        img = work.out.p;
        return rc;
    });
}
int render_adaptive_scene(TakeScene *ts, const TakeRenderOpts &o, const TakeAdaptiveOpts *a, void *d_out, const TakeAdaptiveStats &d_stats, hipStream_t stream) {
    return on_primary(ts, [&](auto &sc, auto &work) { return adaptive_impl(ts, sc, work, o, a, d_out, d_stats, stream); });
}
int adaptive_min_spp(const TakeRenderOpts &o, const TakeAdaptiveOpts *a) { return make_rule(o, a).min_spp; }
int render_features_scene(TakeScene *ts, const TakeRenderOpts &o, const TakeFeatureBuffers &d_out, hipStream_t stream) {
    return on_primary(ts, [&](auto &sc, auto &work) { return features_impl(ts, sc, work, o, d_out, stream); });
}
int render_motion_scene(TakeScene *ts, const TakeRenderOpts &o, const TakeMotionBuffers &d_out, bool marked, hipStream_t stream) {
    if (marked && !ts->mark.set) return fail(TAKE_E_INVALID, "no marked frame: take_hip_scene_mark_frame has not been called on this scene");
    return on_primary(ts, [&](auto &sc, auto &work) {
        using R = std::remove_reference_t<decltype(*work.accum.p)>;
        const CameraRec<R> *cam = &sc.dev.cam;
        if constexpr (sizeof(R) == 8) { if (marked) cam = &ts->mark.cam_d; }
        else { if (marked) cam = &ts->mark.cam_f; }
        // (k_motion indexes the marked transforms with the hit's placement)
        if (marked && sc.inst_trace.n > 0 && ts->mark.xforms.n != 12 * sc.inst_trace.n)
            return fail(TAKE_E_INVALID, "unsupported: the marked frame does not have one transform per placement record (a scene built under TAKE_HIP_BRAID > 1)");
        // the marked geometry, when the handle holds it (take_hip_scene_track_vertices): one entry per record, and per
        // placement record the first entry of its prototype
        MarkedGeometry<R> geom{nullptr, nullptr};
        if (marked && ts->mark.has_geometry()) {
            if constexpr (sizeof(R) == 8) geom.words = ts->mark.geom_d.p;
            else geom.words = ts->mark.geom_f.p;
            const size_t held = sizeof(R) == 8 ? ts->mark.geom_d.n : ts->mark.geom_f.n;
            geom.inst_first = ts->mark.inst_first.p;
            if (!geom.words || held != (size_t)MARKED_STRIDE * sc.prims.n || ts->mark.inst_first.n != sc.inst_trace.n)
                return fail(TAKE_E_INVALID, "unsupported: the marked geometry does not have one entry per primitive record");
        }
        return motion_impl(ts, sc, work, o, d_out, *cam, marked ? ts->mark.xforms.p : nullptr, geom, stream);
    });
}
int check_render_values(const TakeRenderOpts &o) {
    if (o.spp <= 0) return fail(TAKE_E_INVALID, "spp must be positive");
    if (o.max_depth < -1) return fail(TAKE_E_INVALID, "max_depth must be >= -1");
    if (o.integrator < 0 || o.integrator > 3) return fail(TAKE_E_INVALID, "unknown integrator");
    return TAKE_OK;
}
int render_rays_scene(TakeScene *ts, const TakeRenderOpts &o, const TakeRayBatch &d_batch, void *d_out, hipStream_t stream) {
    FirstRays rays;
    rays.kind = FirstRays::CALLER, rays.first_sample = d_batch.first_sample, rays.batch = &d_batch;
    return on_primary(ts, [&](auto &sc, auto &work) { return render_impl(ts, sc, work, o, rays, d_out, stream, false, true); });
}
int camera_rays_scene(TakeScene *ts, const TakeRenderOpts &o, int32_t first_sample, void *d_rays_out, hipStream_t stream) {
    return on_primary(ts, [&](auto &sc, auto &work) { return camera_rays_impl(ts, sc, work, o, first_sample, d_rays_out, stream); });
}
int trace_rays_host(TakeScene *ts, const void *rays, int64_t n, void *hits, int32_t *occ, bool any) {
    return on_primary(ts, [&](auto &sc, auto &work) { return trace_host(ts, sc, work, rays, n, hits, occ, any); });
}
// take_hip_scene_focus_distance_at: the centre ray of the pixel from lookfrom — the pinhole ray, camera_dir_centre's
// operations on the host — through the closest-hit hook; the hit's t times -(w . d), its distance along the view axis
int focus_distance_scene(TakeScene *ts, int32_t column, int32_t row, double *distance_out) {
    return on_primary(ts, [&](auto &sc, auto &work) {
        using R = std::remove_reference_t<decltype(*work.accum.p)>;
        const CameraRec<R> &c = sc.dev.cam;
        const RenderParams<R> rp = make_params<R>(TakeRenderOpts{}, c.width, c.height, c.height, 0, 1);
        const Vec3<R> d = camera_dir_centre(c, rp, (int64_t)(c.height - 1 - row) * c.width + column);
        const RayAoS<R> ray{{c.lookfrom[0], c.lookfrom[1], c.lookfrom[2]}, R(0), {d.x, d.y, d.z}, Const<R>::inf()};
        HitAoS<R> hit{};
        if (const int rc = trace_host(ts, sc, work, &ray, 1, &hit, nullptr, false)) return rc;
        *distance_out = hit.shape_id >= 0 ? (double)(hit.t * -dot(Vec3<R>{c.w[0], c.w[1], c.w[2]}, d)) : 0.0;
        return (int)TAKE_OK;
    });
}
int trace_rays_device(TakeScene *ts, const void *d_rays, int64_t n, void *d_hits, bool count, hipStream_t stream) {
    return on_primary(ts, [&](auto &sc, auto &work) { return trace_impl(ts, sc, work, d_rays, n, d_hits, nullptr, false, count, stream); });
}
TakeCamera shutter_camera(const TakeCamera &marked, const TakeCamera &current, double t) {
    TakeCamera c = current;  // (width and height: the scene's)
    for (int a = 0; a < 3; a++) {
        c.lookfrom[a] = shutter_lerp(t, marked.lookfrom[a], current.lookfrom[a]);
        c.lookat[a] = shutter_lerp(t, marked.lookat[a], current.lookat[a]);
        c.up[a] = shutter_lerp(t, marked.up[a], current.up[a]);
    }
    c.vfov = shutter_lerp(t, marked.vfov, current.vfov);
    return c;
}
// On the default stream, as the re-pose that reads `posed` next; returns after the kernel has completed.
int shutter_pose_device(const double *d_marked, const double *d_current, const std::vector<double> &times, int64_t n, DevBuf<double> &posed, int64_t &first_bad,
                        std::vector<int> &moved) {
    first_bad = -1;
    moved.assign(times.size(), 0);
    const int64_t lanes = (int64_t)times.size() * n;
    if (lanes <= 0) return TAKE_OK;
    if (lanes >= ((int64_t)1 << 31) / 12) return fail(TAKE_E_INVALID, "unsupported: too many slices times placements for one launch");
    DevBuf<double> d_times;
    DevBuf<int> words;  // [0] the first offender, [1 ..] the slices' moved flags
    std::vector<int> words_h(1 + times.size(), 0);
    const int none = INT32_MAX;
    words_h[0] = none;
    if (posed.alloc(12 * (size_t)lanes) != hipSuccess || d_times.upload(times) != hipSuccess || words.upload(words_h) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for the placements' poses over the shutter");
    hipLaunchKernelGGL(k_shutter_pose, dim3((unsigned)((lanes + SHUTTER_BLOCK - 1) / SHUTTER_BLOCK)), dim3(SHUTTER_BLOCK), 0, nullptr, d_marked, d_current,
                       d_times.p, (int)times.size(), (int)n, posed.p, words.p, words.p + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(words_h.data(), words.p, words.bytes(), hipMemcpyDeviceToHost));
    if (words_h[0] != none) first_bad = words_h[0];
    std::copy(words_h.begin() + 1, words_h.end(), moved.begin());
    return TAKE_OK;
}
// The launch alone: the 16-byte path where the three addresses agree mod 16 (one element in front of it where they are
// 8 mod 16), the scalar loop for everything otherwise; a grid for the device, never for n.
void shutter_vertices_launch(const double *d_a, const double *d_b, int64_t n, double t, double *d_out, int *d_moved, int num_cus, hipStream_t stream) {
    if (n <= 0) return;
    const uintptr_t pa = (uintptr_t)d_a & 15, pb = (uintptr_t)d_b & 15, po = (uintptr_t)d_out & 15;
    const bool vec = pa == pb && pb == po && (pa == 0 || pa == 8);
    const int head = vec && pa == 8 ? 1 : 0;
    const int64_t pairs = vec ? (n - head) / 2 : 0;
    const int64_t lanes = std::max<int64_t>(pairs, n - 2 * pairs);
    const int64_t blocks = std::min<int64_t>((lanes + SHUTTER_BLOCK - 1) / SHUTTER_BLOCK, (int64_t)std::max(num_cus, 1) * SHUTTER_BLOCKS_PER_CU);
    hipLaunchKernelGGL(k_shutter_vertices, dim3((unsigned)blocks), dim3(SHUTTER_BLOCK), 0, stream, d_a, d_b, n, head, pairs, t, d_out, d_moved);
}

}  // namespace tk_host

extern "C" {

int take_hip_pack_exr_scanlines(const void *d_rgb, int32_t precision, int32_t width, int32_t height, uint16_t *d_out, void *stream) {
    if (!d_rgb || !d_out || width <= 0 || height <= 0) return fail(TAKE_E_INVALID, "bad argument");
    if (precision != TAKE_PRECISION_F32 && precision != TAKE_PRECISION_F64) return fail(TAKE_E_INVALID, "unknown precision");
    const int nd = check_device();
    if (nd < 0) return nd;
    const int64_t total = (int64_t)width * height * 3;
    const dim3 grid((unsigned)std::min<int64_t>((total + BLOCK - 1) / BLOCK, 8192));
    with_real(precision, [&](auto tag) {
        using R = decltype(tag);
        hipLaunchKernelGGL((k_pack_exr<R>), grid, dim3(BLOCK), 0, (hipStream_t)stream, (const R *)d_rgb, width, height, d_out);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return TAKE_OK;
}

int take_hip_debug_table(int32_t kind, int32_t precision, const double *in, int64_t n, int32_t in_cols,
                         const double *rnd, double *out, int32_t out_cols) {
    if (!in || !out || !rnd || n < 0) return fail(TAKE_E_INVALID, "null argument");
    int nd = check_device();
    if (nd < 0) return nd;
    if (n == 0) return TAKE_OK;
    DevBuf<double> d_in, d_rnd, d_out;
    DevBuf<ImageInfo> d_img;
    DevBuf<float> d_texf;
    DevBuf<double> d_texd;
    // the fixed 5x4 image the reference harness used for the material / texture tables (oracle/ref_harness.cpp)
    std::vector<float> tf(60);
    std::vector<double> td(60);
    for (int y = 0; y < 4; y++)
        for (int x = 0; x < 5; x++) {
            const double c[3] = {0.1 + 0.15 * x + 0.01 * y, 0.9 - 0.2 * y + 0.02 * x, 0.3 + 0.05 * ((x * 3 + y * 7) % 5)};
            for (int a = 0; a < 3; a++) td[3 * (y * 5 + x) + a] = c[a], tf[3 * (y * 5 + x) + a] = (float)c[a];
        }
    std::vector<ImageInfo> img{ImageInfo{5, 4, 0}};
    if (d_in.alloc((size_t)n * in_cols) != hipSuccess || d_rnd.alloc((size_t)n * TAB_RND) != hipSuccess ||
        d_out.alloc((size_t)n * out_cols) != hipSuccess || d_img.upload(img) != hipSuccess ||
        d_texf.upload(tf) != hipSuccess || d_texd.upload(td) != hipSuccess)
        return fail(TAKE_E_NOMEM, "debug table allocation failed");
    if (hipMemcpy(d_in.p, in, d_in.bytes(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_rnd.p, rnd, d_rnd.bytes(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_out.p, 0, d_out.bytes()) != hipSuccess)
        return fail(TAKE_E_DEVICE, "debug table upload failed");
    const dim3 g((unsigned)((n + BLOCK - 1) / BLOCK)), b(BLOCK);
    if (precision == TAKE_PRECISION_F64) {
        DeviceScene<double> sc{};
        sc.images = d_img.p, sc.texels = d_texd.p;
        hipLaunchKernelGGL((k_debug_table<double>), g, b, 0, nullptr, sc, kind, d_in.p, d_rnd.p, n, d_out.p);
    } else {
        DeviceScene<float> sc{};
        sc.images = d_img.p, sc.texels = d_texf.p;
        hipLaunchKernelGGL((k_debug_table<float>), g, b, 0, nullptr, sc, kind, d_in.p, d_rnd.p, n, d_out.p);
    }
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return fail(TAKE_E_DEVICE, "debug table kernel failed");
    if (hipMemcpy(out, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TAKE_E_DEVICE, "debug table download failed");
    return TAKE_OK;
}

int take_hip_debug_env(TakeScene *ts, int32_t side, int32_t kind, const double *in, int64_t n, double *out) {
    if (!ts || !in || !out || n < 0) return fail(TAKE_E_INVALID, "null argument");
    if (n > ((int64_t)1 << 31)) return fail(TAKE_E_INVALID, "more than 2^31 rows");
    if (kind != ENV_SAMPLE && kind != ENV_EVAL) return fail(TAKE_E_INVALID, "unknown kind");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    TAKE_ON_DEVICE(ts);
    return on_side(ts, side, [&](auto &sc) { return debug_env_side(sc, kind, in, n, out); });
}

}  // extern "C"

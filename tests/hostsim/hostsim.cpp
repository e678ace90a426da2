// hostsim.cpp — TEST INFRASTRUCTURE.  Serial host re-execution of the *device* code paths of take_amd/csrc:
// the same tk_host_scene.h (scene preparation + wide BVH), tk_traverse.h, tk_shade.h and tk_integrate.h that
// the HIP kernels call, driven by plain loops in the same round order as the kernels of tk_kernels.h.
//
// Purpose: debug the product's device logic on a machine without a GPU (the authoring container) by comparing
// it with the oracle at small sizes.  It is compiled only by tests/ (tests/hostsim/Makefile), is not part of
// take_amd/ and is never loaded by the product: libtake_hip.so has no CPU path.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "take_hip.h"
#include "tk_host_scene.h"
#include "tk_integrate.h"

using namespace tk;

namespace {
struct ArrayStack {
    int32_t child[128];
    float key[128];
    int max_level = 0;
    void push(int level, int32_t c, float k) {
        child[level] = c;
        key[level] = k;
        if (level + 1 > max_level) max_level = level + 1;
    }
    void pop(int level, int32_t &c, float &k) {
        c = child[level];
        k = key[level];
    }
};
std::string g_err;

template <class R> void dump_slot(const PathState<R> &st, int64_t slot, const char *tag, int k) {
    std::fprintf(stderr, "[slot %lld] k=%d %s R:", (long long)slot, k, tag);
    for (int c = 0; c < PATH_REC; c++)
        if (c != S_HIT && c != S_CTR && c != S_FLAGS) std::fprintf(stderr, " %.17g", (double)st.R_(c, slot));
    std::fprintf(stderr, " I:");
    for (int c : {(int)S_HIT, (int)S_CTR, (int)S_FLAGS}) std::fprintf(stderr, " %d", st.I_(c, slot));
    std::fprintf(stderr, "\n");
}

struct Stats {
    uint64_t closest = 0, shadow = 0, nodes = 0, prims = 0, max_stack = 0;
};
// Mixed precision, last exact round: what k_shade does in registers for a path that goes on (k_convert_state is the
// stand-alone form): ray, pending sample, throughput, radiance so far, stream counter and flags move to the f32
// record of the slot; the f64 record's radiance is cleared (it receives what this round's shadow ray adds) and
// S_CONV says that the f32 record counts.
void convert_to_f32(const PathState<double> &a, const PathState<float> &b, int64_t s) {
    constexpr int WORDS[] = {S_OX, S_OY, S_OZ, S_DX, S_DY, S_DZ, S_PDF, S_TX, S_TY, S_TZ, S_LX, S_LY, S_LZ, S_FX, S_FY, S_FZ};
    for (int w : WORDS) b.R_(w, s) = (float)a.R_(w, s);
    b.I_(S_CTR, s) = a.I_(S_CTR, s);
    b.I_(S_FLAGS, s) = a.I_(S_FLAGS, s);
    b.I_(S_OCC, s) = -1;
    a.R_(S_LX, s) = 0.0, a.R_(S_LY, s) = 0.0, a.R_(S_LZ, s) = 0.0;
    a.I_(S_CONV, s) = 1;
}

// One launch round k over the paths of `cur`: k_trace<closest>, k_shade (next / shadow requests), k_trace<shadow>.
// to_f32 (R = double only): the round is the last exact one of a mixed render — its continuing paths are converted
// after the shade and before the shadow rays, as the device does.
template <class R>
void run_round(const DeviceScene<R> &sc, const RenderParams<R> &rp, const PathState<R> &st, const std::vector<int32_t> &cur,
               std::vector<int32_t> &next, std::vector<int32_t> &shadow, int k, Stats &n, int64_t dump, int64_t slots,
               const PathState<float> *to_f32) {
    next.clear();
    shadow.clear();
    for (int32_t slot : cur) {  // k_trace<closest>
        RayT<R> ray = make_ray(st.R_(S_OX, slot), st.R_(S_OY, slot), st.R_(S_OZ, slot), st.R_(S_DX, slot),
                               st.R_(S_DY, slot), st.R_(S_DZ, slot), rp.ray_eps, Const<R>::inf());
        HitT<R> hit;
        ArrayStack stack;
        TravCount tc;
        traverse<R, false, true>(sc, ray, stack, hit, tc);
        n.nodes += tc.nodes, n.prims += tc.prims, n.closest++;
        n.max_stack = std::max<uint64_t>(n.max_stack, stack.max_level);
        st.I_(S_HIT, slot) = hit.prim;
        st.I_(S_INST, slot) = hit.inst;
        st.R_(S_HT, slot) = hit.t;
        st.R_(S_HU, slot) = hit.u;
        st.R_(S_HV, slot) = hit.v;
    }
    if (dump >= 0 && dump < slots) dump_slot(st, dump, "after trace_closest", k);
    for (int32_t slot : cur) {  // k_shade
        uint32_t req = rp.integrator ? shade_path_alt(sc, rp, st, (int64_t)slot, k) : shade_path(sc, rp, st, (int64_t)slot, k);
        if (req & REQ_EXTEND) next.push_back(slot);
        if (req & REQ_SHADOW) shadow.push_back(slot);
    }
    if constexpr (sizeof(R) == 8) {
        if (to_f32)
            for (int32_t slot : next) convert_to_f32(st, *to_f32, slot);
    }
    if (dump >= 0 && dump < slots) dump_slot(st, dump, "after shade", k);
    for (int32_t slot : shadow) {  // k_trace<shadow>
        RayT<R> ray = make_ray(st.R_(S_OX, slot), st.R_(S_OY, slot), st.R_(S_OZ, slot), st.R_(S_SX, slot),
                               st.R_(S_SY, slot), st.R_(S_SZ, slot), rp.ray_eps, st.R_(S_ST, slot));
        HitT<R> hit;
        ArrayStack stack;
        TravCount tc;
        traverse<R, true, true>(sc, ray, stack, hit, tc);
        n.nodes += tc.nodes, n.prims += tc.prims, n.shadow++;
        if (hit.prim < 0) {
            st.R_(S_LX, slot) = st.R_(S_LX, slot) + st.R_(S_CX, slot);
            st.R_(S_LY, slot) = st.R_(S_LY, slot) + st.R_(S_CY, slot);
            st.R_(S_LZ, slot) = st.R_(S_LZ, slot) + st.R_(S_CZ, slot);
        }
    }
    if (dump >= 0 && dump < slots) dump_slot(st, dump, "after trace_shadow", k);
}

template <class R> RenderParams<R> render_params(const HostScene<R> &hs, const TakeRenderOpts &o, int n_rows) {
    RenderParams<R> rp{};
    const int W = hs.cam.width, H = hs.cam.height;
    rp.width = W, rp.height = H, rp.n_local_rows = n_rows, rp.npix = (int32_t)((int64_t)n_rows * W);
    rp.inv_npix = 1.0 / (double)rp.npix, rp.inv_width = 1.0 / (double)W;
    rp.strip_first = o.strip_first, rp.strip_stride = o.strip_stride > 0 ? o.strip_stride : 1;
    rp.spp = o.spp, rp.max_depth = o.max_depth, rp.seed = o.seed, rp.integrator = o.integrator;
    rp.ray_eps = o.ray_epsilon > 0 ? R(o.ray_epsilon) : (sizeof(R) == 8 ? R(1e-7) : R(1e-4));
    return rp;
}

// MIXED: R = double, and rounds k >= exact_bounces (<= 0: TAKE_DEFAULT_EXACT_BOUNCES) run on f32 records of the same
// slots and the f32 scene (tk_render.hip: render_impl); the samples are accumulated as k_accumulate_mixed does.
template <class R, bool MIXED = false>
int render_t(const TakeSceneDesc &desc, const TakeRenderOpts &o, void *out_v, uint64_t *stats) {
    const int max_leaf = std::getenv("HOSTSIM_MAX_LEAF") ? std::atoi(std::getenv("HOSTSIM_MAX_LEAF")) : 0;
    HostScene<R> hs;
    g_err = prepare_scene<R>(desc, max_leaf, 1, hs);
    if (!g_err.empty()) return TAKE_E_INVALID;
    HostScene<float> hs32;
    if (MIXED) {
        if (o.integrator != 0) {
            g_err = "mixed precision renders the reference's path_tracing (integrator 0) only";
            return TAKE_E_INVALID;
        }
        g_err = prepare_scene<float>(desc, max_leaf, 1, hs32);
        if (!g_err.empty()) return TAKE_E_INVALID;
    }
    DeviceScene<R> sc = hs.view();
    DeviceScene<float> sc32 = MIXED ? hs32.view() : DeviceScene<float>{};
    const int exact_rounds = o.exact_bounces > 0 ? o.exact_bounces : TAKE_DEFAULT_EXACT_BOUNCES;
    const int W = hs.cam.width, H = hs.cam.height;
    const int stride = o.strip_stride > 0 ? o.strip_stride : 1;
    const int n_strips = (H + TILE_ROWS - 1) / TILE_ROWS;
    int n_rows = 0;
    for (int s = o.strip_first; s < n_strips; s += stride) n_rows += std::min(H, (s + 1) * TILE_ROWS) - s * TILE_ROWS;
    const int64_t npix = (int64_t)n_rows * W;
    RenderParams<R> rp = render_params(hs, o, n_rows);
    RenderParams<float> rp32{};
    if (MIXED) {  // the f32 rounds' parameters: the same but for the ray epsilon (1e-4 unless given)
        rp32 = render_params(hs32, o, n_rows);
        rp32.ray_eps = o.ray_epsilon > 0 ? (float)o.ray_epsilon : 1e-4f;
    }
    const int spb = o.samples_per_batch > 0 ? std::min(o.samples_per_batch, o.spp) : o.spp;
    const int64_t slots = (int64_t)spb * npix;
    std::vector<R> sr((size_t)PATH_REC * slots);
    PathState<R> st{sr.data(), slots};
    std::vector<float> sr32(MIXED ? (size_t)PATH_REC * slots : 0);
    PathState<float> st32{sr32.data(), slots};
    std::vector<R> accum(3 * npix, R(0));
    std::vector<int32_t> q[2], shadow;
    Stats n;
    const char *dump_env = std::getenv("TAKE_HIP_DUMP_SLOT");
    const int64_t dump = dump_env ? std::atoll(dump_env) : -1;
    for (int s0 = 0; s0 < o.spp; s0 += spb) {
        const int nb = std::min(spb, o.spp - s0);
        const int64_t nslot = (int64_t)nb * npix;
        rp.s0 = rp32.s0 = s0;
        rp.spb = rp32.spb = nb;
        q[0].clear();
        for (int64_t s = 0; s < nslot; s++) {
            generate_path(sc, rp, st, s);
            q[0].push_back((int32_t)s);
        }
        for (int k = 0; k < o.max_depth + 2; k++) {
            const int cur = k & 1, next = cur ^ 1;
            if (MIXED && k >= exact_rounds)
                run_round<float>(sc32, rp32, st32, q[cur], q[next], shadow, k, n, dump, slots, nullptr);
            else
                run_round<R>(sc, rp, st, q[cur], q[next], shadow, k, n, dump, slots,
                             MIXED && k == exact_rounds - 1 ? &st32 : nullptr);
            if (q[next].empty()) break;
        }
        for (int64_t p = 0; p < npix; p++)  // k_accumulate / k_accumulate_mixed
            for (int s = 0; s < nb; s++) {
                const int64_t slot = (int64_t)s * npix + p;
                for (int c = 0; c < 3; c++) {
                    if (MIXED) {
                        const bool conv = st.I_(S_CONV, slot) != 0;
                        accum[3 * p + c] = accum[3 * p + c] + (st.R_(S_LX + c, slot) + (conv ? (double)st32.R_(S_LX + c, slot) : 0.0));
                    } else {
                        accum[3 * p + c] = accum[3 * p + c] + st.R_(S_LX + c, slot);
                    }
                }
            }
    }
    R *out = (R *)out_v;  // k_resolve
    const R inv = R(1) / R(o.spp);
    for (int64_t p = 0; p < npix; p++) {
        const int lr = (int)(p / W), x = (int)(p % W);
        const int64_t oidx = 3 * ((int64_t)(n_rows - 1 - lr) * W + x);
        for (int c = 0; c < 3; c++) out[oidx + c] = accum[3 * p + c] * inv;
    }
    if (stats) {
        stats[0] = n.closest, stats[1] = n.shadow, stats[2] = n.nodes, stats[3] = n.prims, stats[4] = n.max_stack;
        stats[5] = (uint64_t)hs.stats.n_nodes, stats[6] = (uint64_t)hs.stats.depth;
    }
    return TAKE_OK;
}

template <class R> int trace_t(const TakeSceneDesc &desc, const void *rays_v, int64_t n, void *hits_v, int any) {
    HostScene<R> hs;
    g_err = prepare_scene<R>(desc, std::getenv("HOSTSIM_MAX_LEAF") ? std::atoi(std::getenv("HOSTSIM_MAX_LEAF")) : 0, 1, hs);
    if (!g_err.empty()) return TAKE_E_INVALID;
    DeviceScene<R> sc = hs.view();
    const R *rays = (const R *)rays_v;  // org3 tmin dir3 tmax
    R *hits = (R *)hits_v;              // shape t u v  (shape as R)
    for (int64_t i = 0; i < n; i++) {
        const R *q = rays + 8 * i;
        RayT<R> ray = make_ray(q[0], q[1], q[2], q[4], q[5], q[6], q[3], q[7]);
        HitT<R> hit;
        ArrayStack stack;
        TravCount tc;
        if (any)
            traverse<R, true, false>(sc, ray, stack, hit, tc);
        else
            traverse<R, false, false>(sc, ray, stack, hit, tc);
        hits[4 * i] = R(hit.shape);
        hits[4 * i + 1] = hit.prim >= 0 ? hit.t : R(0);
        hits[4 * i + 2] = hit.u;
        hits[4 * i + 3] = hit.v;
    }
    return TAKE_OK;
}
// The stack of hostsim_trace_stats: an ArrayStack that knows how deep the trace kernel's ONE stack is at the same point.
// traverse() nests a second stack for the prototype of a two-level scene; the kernel (tk_trace_quad.h) goes on above the
// entries of the top level and one return marker.  A nested stack therefore starts at the live entries of the one it
// was created under + 1 (the marker sits at level base - 1); g_deepest is the highest entry count reached since it was
// cleared, g_marker the highest level a return marker was put at (-1: none).
// g_drop >= 0 is a deliberate fault for the tests' non-vacuity guards: every entry the kernel would keep at level
// >= g_drop comes back as an empty child, i.e. is lost — what a spill area that loses its entries would do.
struct DepthStack : ArrayStack {
    static inline thread_local DepthStack *g_top = nullptr;
    static inline thread_local int g_deepest = 0, g_marker = -1, g_drop = -1;
    DepthStack *parent;
    int base, live = 0;
    DepthStack() : parent(g_top), base(g_top ? g_top->base + g_top->live + 1 : 0) {
        g_top = this;
        if (parent && base - 1 > g_marker) g_marker = base - 1;
        if (base > g_deepest) g_deepest = base;
    }
    ~DepthStack() { g_top = parent; }
    DepthStack(const DepthStack &) = delete;
    void push(int level, int32_t c, float k) {
        ArrayStack::push(level, c, k);
        live = level + 1;
        if (base + live > g_deepest) g_deepest = base + live;
    }
    void pop(int level, int32_t &c, float &k) {
        ArrayStack::pop(level, c, k);
        if (g_drop >= 0 && base + level >= g_drop) c = CHILD_EMPTY;
        live = level;
    }
};
// out[0] = deepest stack over the rays (entries, as the kernel counts them), out[1] = nodes, out[2] = depth of the tree,
// out[3..5] = interior nodes visited, primitives tested, leaves visited over all rays (TravCount), out[6] = rays whose
// own stack went beyond `lds_levels` entries, out[7] = highest level of a return marker + 1 (0: no placement entered).
// hits (may be null): n x 4 Real as hostsim_trace writes them.  drop_from < 0: no fault (see DepthStack).
template <class R>
int trace_stats_t(const TakeSceneDesc &desc, const void *rays_v, int64_t n, int any, int lds_levels, int drop_from, void *hits_v, uint64_t *out) {
    HostScene<R> hs;
    g_err = prepare_scene<R>(desc, std::getenv("HOSTSIM_MAX_LEAF") ? std::atoi(std::getenv("HOSTSIM_MAX_LEAF")) : 0, 1, hs);
    if (!g_err.empty()) return TAKE_E_INVALID;
    DeviceScene<R> sc = hs.view();
    const R *rays = (const R *)rays_v;  // org3 tmin dir3 tmax
    R *hits = (R *)hits_v;
    int deepest = 0;
    uint64_t n_deep = 0;
    DepthStack::g_marker = -1, DepthStack::g_drop = drop_from;
    TravCount tc;
    for (int64_t i = 0; i < n; i++) {
        const R *q = rays + 8 * i;
        RayT<R> ray = make_ray(q[0], q[1], q[2], q[4], q[5], q[6], q[3], q[7]);
        HitT<R> hit;
        DepthStack::g_deepest = 0;
        {
            DepthStack stack;
            if (any)
                traverse<R, true, true>(sc, ray, stack, hit, tc);
            else
                traverse<R, false, true>(sc, ray, stack, hit, tc);
        }
        deepest = std::max(deepest, DepthStack::g_deepest);
        n_deep += DepthStack::g_deepest > lds_levels;
        if (hits) hits[4 * i] = R(hit.shape), hits[4 * i + 1] = hit.prim >= 0 ? hit.t : R(0), hits[4 * i + 2] = hit.u, hits[4 * i + 3] = hit.v;
    }
    DepthStack::g_drop = -1;
    out[0] = (uint64_t)deepest, out[1] = (uint64_t)hs.stats.n_nodes, out[2] = (uint64_t)hs.stats.depth;
    out[3] = tc.nodes, out[4] = tc.prims, out[5] = tc.leaves, out[6] = n_deep, out[7] = (uint64_t)(DepthStack::g_marker + 1);
    return TAKE_OK;
}
// Compressed nodes of the f32 scene against the full-width ones they were made from, in exact (double) arithmetic.
// out[0] = child slots checked, out[1] = slots whose decoded box does NOT contain the true box widened by the
// builder's slack (must be 0), out[2] = child words that differ (must be 0), out[3] = 1e6 * surface-area inflation,
// out[4] = 1 if the scene uses compressed nodes, out[5] = node width (4 or 8), out[6] = 8-wide only: children whose
// centre lies on the wrong side of the node's centre on some axis for their slot (diagnostic, not an error)
template <int W>
static void check_qnodes_w(const HostScene<float> &hs, const std::vector<NodeW<float, W>> &nodes, const std::vector<QNodeW<W>> &qnodes, int64_t *out) {
    for (size_t n = 0; n < nodes.size(); n++)
        for (int i = 0; i < W; i++) {
            const NodeChild<float> &c = nodes[n].c[i];
            const QChild &q = qnodes[n].c[i];
            if (c.child != q.child) out[2]++;
            if (c.child == CHILD_EMPTY) continue;
            out[0]++;
            bool ok = true;
            for (int a = 0; a < 3; a++) {
                const double lo = (double)hs.grid_lo[a] + (double)(Q_BIAS + (q.q[a] & 0xffffu)) * (double)hs.grid_step[a];
                const double hi = (double)hs.grid_lo[a] + (double)(Q_BIAS + (q.q[a] >> 16)) * (double)hs.grid_step[a];
                const double slack = (double)Q_MAX * (double)hs.grid_step[a] * 0x1p-20;
                if (!(lo <= (double)c.bmin[a] - slack && hi >= (double)c.bmax[a] + slack)) ok = false;
                if ((q.q[a] & 0xffffu) > (q.q[a] >> 16) || (q.q[a] >> 16) > (uint32_t)Q_MAX) ok = false;
            }
            if (!ok) out[1]++;
        }
}
// take_hip_debug_tree's view (include/take_hip.h) of a scene the HOST prepared: the tree of prepare_scene<R>, in the node
// format upload_scene would send to the device, kept until the next call so that the caller can size its buffers
// from the info first.  The 8-wide tree exists compressed only.
template <class R> struct PreparedTree {
    HostScene<R> hs;
    TakeDebugTreeInfo info{};
    const void *nodes = nullptr;
    int prepare(const TakeSceneDesc &desc, int max_leaf, int32_t *depth) {
        hs = HostScene<R>{};
        g_err = prepare_scene<R>(desc, max_leaf, 2, hs);
        if (!g_err.empty()) return TAKE_E_INVALID;
        info = TakeDebugTreeInfo{};
        info.node_format = !hs.qnodes8.empty() ? 2 : (!hs.qnodes.empty() ? 1 : 0);
        info.node_width = hs.node_width;
        info.two_level = hs.inst_trace.empty() ? 0 : 1;
        info.root_child = hs.root_child;
        info.real_bytes = (int32_t)sizeof(R);
        info.node_bytes = (int32_t)(info.node_format == 2 ? sizeof(QNode8) : (info.node_format == 1 ? sizeof(QNode4) : sizeof(Node4<R>)));
        info.prim_bytes = (int32_t)sizeof(PrimRec<R>), info.inst_bytes = (int32_t)sizeof(InstTrace<R>);
        info.n_nodes = hs.stats.n_nodes, info.n_prims = (int64_t)hs.prims.size(), info.n_instances = (int64_t)hs.inst_trace.size();
        for (int a = 0; a < 3; a++) info.grid_lo[a] = hs.grid_lo[a], info.grid_step[a] = hs.grid_step[a];
        nodes = info.node_format == 2 ? (const void *)hs.qnodes8.data() : (info.node_format == 1 ? (const void *)hs.qnodes.data() : (const void *)hs.nodes.data());
        if (info.node_format == 0 && hs.node_width != 4) {
            g_err = "the 8-wide tree has no full-width form to traverse";
            return TAKE_E_INVALID;
        }
        *depth = hs.stats.depth;
        return TAKE_OK;
    }
    void copy(void *nodes_out, void *prims_out, void *inst_out) const {
        if (info.n_nodes) std::memcpy(nodes_out, nodes, (size_t)info.n_nodes * info.node_bytes);
        if (info.n_prims) std::memcpy(prims_out, hs.prims.data(), (size_t)info.n_prims * info.prim_bytes);
        if (info.n_instances) std::memcpy(inst_out, hs.inst_trace.data(), (size_t)info.n_instances * info.inst_bytes);
    }
};
PreparedTree<float> g_tree_f;
PreparedTree<double> g_tree_d;
// take_hip_debug_env's rows (tk_shade.h: debug_env_row) on the scene as prepare_scene leaves it
template <class R> int env_t(const TakeSceneDesc &desc, int kind, const double *in, int64_t n, double *out) {
    HostScene<R> hs;
    g_err = prepare_scene<R>(desc, 0, 1, hs);
    if (g_err.empty() && hs.env.light < 0) g_err = "the scene has no environment map";
    if (!g_err.empty()) return TAKE_E_INVALID;
    const DeviceScene<R> sc = hs.view();
    for (int64_t r = 0; r < n; r++) debug_env_row(sc, kind, in, r, out);
    return TAKE_OK;
}
}  // namespace

extern "C" {
const char *hostsim_last_error(void) { return g_err.c_str(); }
// out: rows*W*3 Real (float for f32, double for f64 and mixed); stats: 7 words (may be null)
int hostsim_render(const TakeSceneDesc *desc, int precision, const TakeRenderOpts *opts, void *out, uint64_t *stats) {
    if (precision == TAKE_PRECISION_MIXED) return render_t<double, true>(*desc, *opts, out, stats);
    return precision == TAKE_PRECISION_F64 ? render_t<double>(*desc, *opts, out, stats)
                                           : render_t<float>(*desc, *opts, out, stats);
}
// divmod_u31 (tk_integrate.h: the slot -> sample / pixel divisions of every shade round, by reciprocal) against the
// integer division, on divisors and dividends around every power of two, the extremes and `n_random` random pairs;
// returns the number of disagreements
int64_t hostsim_check_divmod(int64_t n_random, uint64_t seed) {
    int64_t bad = 0;
    auto check = [&](uint32_t n, uint32_t d) {
        if (d == 0 || n >= (1u << 31) || d >= (1u << 31)) return;
        uint32_t q, r;
        tk::divmod_u31(n, d, 1.0 / (double)d, q, r);
        bad += (q != n / d) || (r != n % d);
    };
    std::vector<uint32_t> edge;
    for (int b = 0; b < 31; b++)
        for (int64_t k = -2; k <= 2; k++) {
            const int64_t v = ((int64_t)1 << b) + k;
            if (v > 0 && v < ((int64_t)1 << 31)) edge.push_back((uint32_t)v);
        }
    edge.push_back((1u << 31) - 1), edge.push_back(1920 * 1080), edge.push_back(1920), edge.push_back(4096 * 4096), edge.push_back(3);
    for (uint32_t d : edge)
        for (uint32_t n : edge) {
            check(n, d);
            check((uint32_t)std::min<uint64_t>((uint64_t)n * d, (1ull << 31) - 1), d);      // exact multiples
            check((uint32_t)std::min<uint64_t>((uint64_t)n * d + d - 1, (1ull << 31) - 1), d);  // just below the next one
        }
    uint64_t z = seed;
    for (int64_t i = 0; i < n_random; i++) {
        z = tk::rng_mix(z + 0x9E3779B97F4A7C15ull);
        const uint32_t n = (uint32_t)(z >> 33), d = (uint32_t)(tk::rng_mix(z) >> (33 + (z & 31) % 30));
        check(n, d);
    }
    return bad;
}

int hostsim_check_qnodes(const TakeSceneDesc *desc, int64_t *out) {
    HostScene<float> hs;
    std::string err = prepare_scene<float>(*desc, 0, 2, hs);
    if (!err.empty()) {
        g_err = err;
        return -1;
    }
    out[0] = out[1] = out[2] = out[6] = 0;
    out[3] = (int64_t)(hs.q_inflation * 1e6);
    out[4] = hs.qnodes.empty() && hs.qnodes8.empty() ? 0 : 1;
    out[5] = hs.node_width;
    if (!hs.qnodes8.empty()) check_qnodes_w<8>(hs, hs.nodes8, hs.qnodes8, out);
    else if (!hs.qnodes.empty()) check_qnodes_w<4>(hs, hs.nodes, hs.qnodes, out);
    return 0;
}
// rays: n x 8 Real laid out as TakeRayF/TakeRayD; hits: n x 4 Real (shape id as Real, t, u, v)
int hostsim_trace(const TakeSceneDesc *desc, int precision, const void *rays, int64_t n, void *hits, int any) {
    return precision == TAKE_PRECISION_F64 ? trace_t<double>(*desc, rays, n, hits, any)
                                           : trace_t<float>(*desc, rays, n, hits, any);
}
// the same rays with the statistics of their traversal: out = 8 words (trace_stats_t); hits may be null; drop_from >= 0
// loses every stack entry at that level or above (the tests' stand-in for a broken spill area), < 0 changes nothing
int hostsim_trace_stats(const TakeSceneDesc *desc, int precision, const void *rays, int64_t n, int any, int lds_levels, int drop_from,
                        void *hits, uint64_t *out) {
    return precision == TAKE_PRECISION_F64 ? trace_stats_t<double>(*desc, rays, n, any, lds_levels, drop_from, hits, out)
                                           : trace_stats_t<float>(*desc, rays, n, any, lds_levels, drop_from, hits, out);
}
// The tree prepare_scene<R> builds for `desc` (TAKE_HIP_NODES as the environment has it), as take_hip_debug_tree shows a
// resident one: hostsim_tree_prepare fills the info and the depth (take_hip_scene_stats' figure) and keeps the scene,
// hostsim_tree_copy copies the kept scene's arrays into buffers sized from that info.
int hostsim_tree_prepare(const TakeSceneDesc *desc, int precision, int max_leaf, TakeDebugTreeInfo *info, int32_t *depth) {
    if (!desc || !info || !depth) return TAKE_E_INVALID;
    const int rc = precision == TAKE_PRECISION_F64 ? g_tree_d.prepare(*desc, max_leaf, depth) : g_tree_f.prepare(*desc, max_leaf, depth);
    if (rc == TAKE_OK) *info = precision == TAKE_PRECISION_F64 ? g_tree_d.info : g_tree_f.info;
    return rc;
}
int hostsim_tree_copy(int precision, void *nodes, void *prims, void *inst_trace) {
    if (!nodes || !prims || !inst_trace) return TAKE_E_INVALID;
    if (precision == TAKE_PRECISION_F64) g_tree_d.copy(nodes, prims, inst_trace);
    else g_tree_f.copy(nodes, prims, inst_trace);
    return TAKE_OK;
}
// the environment-map functions on rows of draws (kind 0) or directions (kind 1): columns as take_hip_debug_env's
int hostsim_env(const TakeSceneDesc *desc, int precision, int kind, const double *in, int64_t n, double *out) {
    if (!desc || !in || !out || (kind != 0 && kind != 1)) return TAKE_E_INVALID;
    return precision == TAKE_PRECISION_F64 ? env_t<double>(*desc, kind, in, n, out) : env_t<float>(*desc, kind, in, n, out);
}
}

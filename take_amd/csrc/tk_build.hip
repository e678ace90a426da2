// tk_build.hip — the host driver of the device LBVH builder: the records and trees of one side of a new scene made on
// the device from the caller's arrays (build_side_on_device, declared in tk_scene_handle.h; tk_create.hip's upload_scene
// calls it), and the three drivers that tk_scene_update.hip stages a change of a resident scene with: the top-level half
// of the build entered again for new transforms of the placements (repose_two_level_device), creation's tail entered
// again for new vertices (update_mesh_vertices_device), and both joined for the meshes of a two-level scene
// (update_two_level_meshes_device).  What they share with each other and with the fresh build is one step each, in the
// anonymous namespace: prototype_pass, top_level_resident, assemble_resident_nodes, placement_records,
// update_shape_records, commit_normals_and_lights.  The only unit that compiles the kernels of tk_build_gpu.h, and rocPRIM with them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"
#include "tk_build_gpu.h"

using namespace tk;
using namespace tk_host;

namespace tk_host {

int DeviceBuildInputs::upload(const TakeSceneDesc &d, const double *const *device_positions) {
    if (ready) return TAKE_OK;
    const size_t n = (size_t)d.n_shapes;
    pos_off.resize((size_t)d.n_meshes);
    int64_t nv = 0;
    for (int i = 0; i < d.n_meshes; i++) pos_off[i] = nv, nv += d.meshes[i].n_vertices;
    HIP_TRY(pos.alloc(3 * (size_t)std::max<int64_t>(nv, 1)));
    PinnedUploads pin;
    for (int i = 0; i < d.n_meshes; i++) {
        if (d.meshes[i].n_vertices <= 0) continue;
        const size_t bytes = sizeof(double) * 3 * (size_t)d.meshes[i].n_vertices;
        // a mesh decoded on the device (take_hip_mesh_from_ply): its positions never were on the host
        if (device_positions && device_positions[i])
            HIP_TRY(hipMemcpyAsync(pos.p + 3 * pos_off[i], device_positions[i], bytes, hipMemcpyDeviceToDevice, pin.stream));
        else
            HIP_TRY(pin.copy(pos.p + 3 * pos_off[i], d.meshes[i].positions, bytes));
    }
    auto up = [&](DevBuf<int32_t> &b, const int32_t *src) -> hipError_t {
        hipError_t e = b.alloc(n);
        return e != hipSuccess ? e : pin.copy(b.p, src, sizeof(int32_t) * n);
    };
    HIP_TRY(up(kind, d.shape_kind));
    HIP_TRY(up(ref, d.shape_ref));
    HIP_TRY(up(face, d.shape_face));
    HIP_TRY(up(area_light, d.shape_area_light));
    HIP_TRY(pin.finish());
    if (std::getenv("TAKE_HIP_VERBOSE"))
        std::fprintf(stderr, "[take_hip] scene_create: uploads pinned in place %.1f MB, pageable %.1f MB\n", pin.pinned_bytes / 1e6, pin.plain_bytes / 1e6);
    ready = true;
    return TAKE_OK;
}

}  // namespace tk_host

namespace {

// device memory in use (the whole device's, as hipMemGetInfo sees it), for the TAKE_HIP_VERBOSE lines; 0 if the runtime
// cannot say
double device_mb_in_use() {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
    return (double)(total_b - free_b) / 1e6;
}
// The high-water mark of a device build (TAKE_HIP_VERBOSE only): sampled where a phase holds the most — after the last
// allocation of the sort, the hierarchy, the collapse, the compression and the permute — each phase freeing what the
// next ones do not read.
struct BuildMemory {
    bool on = std::getenv("TAKE_HIP_VERBOSE") != nullptr;
    const char *side;
    double peak = 0;
    const char *peak_at = "";
    explicit BuildMemory(const char *side_) : side(side_) {}
    void sample(const char *phase) {
        if (!on) return;
        const double mb = device_mb_in_use();
        std::fprintf(stderr, "[take_hip] scene_create: %s device build, %-12s %8.1f MB of device memory in use\n", side, phase, mb);
        if (mb > peak) peak = mb, peak_at = phase;
    }
    void report() const {
        if (on) std::fprintf(stderr, "[take_hip] scene_create: %s device build, peak %.1f MB of device memory in use (%s)\n", side, peak, peak_at);
    }
};

// One LBVH on the device (tk_build_gpu.h): Morton codes -> rocPRIM sort -> k_leaves -> k_hierarchy -> k_refit ->
// k_collapse_count / scan / k_collapse per level.  The scene's only tree, the top-level tree of a two-level scene, or a prototype's.
struct DeviceTree {
    DevBuf<Node4<float>> nodes;  // breadth-first; child words local to the tree: node indices from 0, a leaf = a range of `order`
    DevBuf<uint32_t> order;      // Morton order -> entry of the span (a stable sort: coincident entries keep their order)
    int64_t n_nodes = 0;
    int depth = 0;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // bounds of the span's boxes: the tree's quantisation grid is laid over them
};
const int ORD_INIT[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};  // empty bounds (k_prim_boxes)
dim3 blocks_for(int64_t items) { return dim3((unsigned)((items + lbvh::BLK - 1) / lbvh::BLK)); }

// "Boxes of a span", in two steps (a prototype's records are made between them): the bounds (ord: six ordered ints)
// reset to empty; then the float boxes of n records into pb and their bounds into ord.  Whoever adds boxes of another
// kind (k_placement_pad) goes on growing the same bounds.
hipError_t reset_bounds(DevBuf<int> &ord) { return hipMemcpyAsync(ord.p, ORD_INIT, sizeof(ORD_INIT), hipMemcpyHostToDevice, nullptr); }
template <class R> void span_boxes(const PrimRec<R> *recs, int n, lbvh::Box *pb, DevBuf<int> &ord) {
    if (n > 0) hipLaunchKernelGGL(lbvh::k_prim_boxes<R>, blocks_for(n), dim3(lbvh::BLK), 0, nullptr, recs, n, pb, ord.p);
}

// The first offender a checking kernel met (atomicMin into cell: one word, allocated and set to `none`, which no offender is, by arm())
template <class T> struct FirstOffender {
    T none, first = none;
    DevBuf<T> cell;
    hipError_t arm() { return cell.upload({none}); }
    hipError_t read() { return hipMemcpy(&first, cell.p, sizeof(T), hipMemcpyDeviceToHost); }  // (waits for the kernel)
};
// A side takes a new tree, its arrays moved into sc already: what the host keeps of it (sc.host), what the kernels read (sc.dev)
template <class R> void install_tree(SceneT<R> &sc, int64_t n_nodes, int depth, int32_t root_child, const float *grid_lo, const float *grid_step) {
    sc.host.stats.n_nodes = n_nodes, sc.host.stats.depth = depth, sc.dev.n_nodes = (int32_t)n_nodes;
    sc.host.root_child = sc.dev.root_child = root_child;
    for (int a = 0; a < 3; a++) sc.host.grid_lo[a] = sc.dev.grid_lo[a] = grid_lo[a], sc.host.grid_step[a] = sc.dev.grid_step[a] = grid_step[a];
    sc.bind();
}
// Next to a device build's TAKE_OK (`why`: callers start it at Built): the tree was built — or why it is the host builder's to make
enum class BuildVerdict { Built, TooFewLeaves, TooDeep };
// what an entry with no host builder to turn to returns for a build that ended in rc, or in why; what: "tree", "top-level tree"
int unsupported(int rc, BuildVerdict why, const std::string &what) {
    return rc ? rc : fail(TAKE_E_INVALID, why == BuildVerdict::TooFewLeaves ? "unsupported: a " + what + " of fewer than two leaves"
                                                                           : "unsupported: the new " + what + " is too deep for the traversal stack");
}

// In: the n boxes of a span (pb: freed here, once the leaves exist) and their bounds (scene_ord: ordered ints, as
// k_prim_boxes leaves them).  Out: t.  TooDeep: long runs of equal Morton codes.
// The tree is made of float nodes whatever the scene's precision is (tk_build_gpu.h: only records and primitive boxes
// know it).
int build_tree_device(DevBuf<lbvh::Box> &pb, const DevBuf<int> &scene_ord, int n, int leaf_size, BuildMemory &mem, DeviceTree &t, BuildVerdict &why) {
    using namespace lbvh;
    const int n_leaves = (n + leaf_size - 1) / leaf_size;
    if (n_leaves < 2) return why = BuildVerdict::TooFewLeaves, TAKE_OK;
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    // (a release waits for the kernels launched before it: hipFree synchronises the device)
    DevBuf<Box> lbox, ibox;
    DevBuf<uint64_t> keys, keys_s, lkey;
    DevBuf<uint32_t> vals;
    DevBuf<int> parent_i, parent_l, flag, frontier[2];
    DevBuf<int2> child;
    DevBuf<char> temp;
    // Morton codes, sort
    HIP_TRY(keys.alloc(n));
    HIP_TRY(vals.alloc(n));
    HIP_TRY(keys_s.alloc(n));
    HIP_TRY(t.order.alloc(n));
    hipLaunchKernelGGL(k_morton, blocks_for(n), blk, 0, stream, pb.p, n, scene_ord.p, keys.p, vals.p);
    size_t temp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys.p, keys_s.p, vals.p, t.order.p, (size_t)n, 0, 63, stream));
    HIP_TRY(temp.alloc(temp_bytes));
    mem.sample("sort");
    HIP_TRY(rocprim::radix_sort_pairs(temp.p, temp_bytes, keys.p, keys_s.p, vals.p, t.order.p, (size_t)n, 0, 63, stream));
    keys.release(), vals.release(), temp.release();

    // leaves, hierarchy, refit
    HIP_TRY(lbox.alloc(n_leaves));
    HIP_TRY(lkey.alloc(n_leaves));
    hipLaunchKernelGGL(k_leaves, blocks_for(n_leaves), blk, 0, stream, pb.p, keys_s.p, t.order.p, n, leaf_size, n_leaves, lbox.p, lkey.p);
    pb.release(), keys_s.release();
    HIP_TRY(ibox.alloc(n_leaves));
    HIP_TRY(child.alloc(n_leaves));
    HIP_TRY(parent_i.alloc(n_leaves));
    HIP_TRY(parent_l.alloc(n_leaves));
    HIP_TRY(flag.alloc(n_leaves));
    mem.sample("hierarchy");
    HIP_TRY(hipMemsetAsync(flag.p, 0, flag.bytes(), stream));
    hipLaunchKernelGGL(k_hierarchy, blocks_for(n_leaves - 1), blk, 0, stream, lkey.p, n_leaves, child.p, parent_i.p, parent_l.p);
    hipLaunchKernelGGL(k_refit, blocks_for(n_leaves), blk, 0, stream, n_leaves, child.p, parent_i.p, parent_l.p, lbox.p, ibox.p, flag.p);
    lkey.release(), parent_i.release(), parent_l.release(), flag.release();

    // collapse to 4-wide nodes, breadth-first, level by level (at most one node per leaf; the count is known after).
    // The host reads each level's size (4 bytes) before it launches the next: the grids and the scans are sized to the
    // level, and the loop ends with the tree instead of running every level the stack allows.
    DevBuf<int> cnt, off, n_next;
    HIP_TRY(t.nodes.alloc(n_leaves));
    HIP_TRY(frontier[0].alloc(n_leaves));
    HIP_TRY(frontier[1].alloc(n_leaves));
    HIP_TRY(cnt.alloc(n_leaves));
    HIP_TRY(off.alloc(n_leaves));
    HIP_TRY(n_next.alloc(1));
    size_t scan_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, cnt.p, off.p, 0, (size_t)n_leaves, rocprim::plus<int>(), stream));
    HIP_TRY(temp.alloc(std::max<size_t>(scan_bytes, 1)));
    mem.sample("collapse");
    hipLaunchKernelGGL(k_fill_int, dim3(1), blk, 0, stream, frontier[0].p, 1, 0);  // level 0: one node, made from BVH2 node 0
    t.n_nodes = 0, t.depth = 0;
    int n_in = 1;
    for (int level = 0; n_in > 0; level++) {
        if (level == MAX_LEVELS) return why = BuildVerdict::TooDeep, TAKE_OK;
        size_t need = 0;
        HIP_TRY(rocprim::exclusive_scan(nullptr, need, cnt.p, off.p, 0, (size_t)n_in, rocprim::plus<int>(), stream));
        if (need > temp.bytes()) HIP_TRY(temp.alloc(need));
        hipLaunchKernelGGL(k_collapse_count, blocks_for(n_in), blk, 0, stream, frontier[level & 1].p, n_in, child.p, ibox.p, cnt.p);
        HIP_TRY(rocprim::exclusive_scan(temp.p, need, cnt.p, off.p, 0, (size_t)n_in, rocprim::plus<int>(), stream));
        hipLaunchKernelGGL(k_collapse, blocks_for(n_in), blk, 0, stream, frontier[level & 1].p, n_in, (int)t.n_nodes, off.p, frontier[(level + 1) & 1].p,
                           n_next.p, child.p, ibox.p, lbox.p, leaf_size, n, t.nodes.p);
        t.n_nodes += n_in, t.depth = level + 1;
        HIP_TRY(hipMemcpy(&n_in, n_next.p, sizeof(int), hipMemcpyDeviceToHost));
        if (n_in < 0 || t.n_nodes + n_in > n_leaves) return fail(TAKE_E_DEVICE, "the device collapse lost count of its nodes");
    }
    HIP_TRY(hipGetLastError());
    int ord_h[6];
    HIP_TRY(hipMemcpy(ord_h, scene_ord.p, sizeof(ord_h), hipMemcpyDeviceToHost));
    t.nodes.n = (size_t)t.n_nodes;  // the tail of the allocation is unused
    for (int a = 0; a < 3; a++) t.lo[a] = ord2f(ord_h[a]), t.hi[a] = ord2f(ord_h[3 + a]);
    return TAKE_OK;
}

// Compressed nodes of one tree on its own 15-bit grid (g: laid over the tree's bounds), into `out`; -> the mean
// surface-area inflation of its child boxes (quantise_nodes' figure, tk_bvh.h).  acc: two doubles of scratch.
int quantise_tree_device(const DeviceTree &t, QNode4 *out, DevBuf<double> &acc, QGrid &g, double &inflation) {
    using namespace lbvh;
    g = make_qgrid(t.lo, t.hi);
    HIP_TRY(hipMemsetAsync(acc.p, 0, acc.bytes(), nullptr));
    hipLaunchKernelGGL(k_quantise, blocks_for(t.n_nodes), dim3(BLK), 0, nullptr, t.nodes.p, (int)t.n_nodes, g, out, acc.p);
    double acc_h[2] = {0, 0};
    HIP_TRY(hipMemcpy(acc_h, acc.p, sizeof(acc_h), hipMemcpyDeviceToHost));
    inflation = acc_h[1] > 0 ? acc_h[0] / acc_h[1] : 1.0;
    return TAKE_OK;
}
// full-width nodes of one tree into `out`: the float ones as they are, or widened to double (exact: still conservative)
int wide_nodes_device(const DeviceTree &t, Node4<float> *out) {
    HIP_TRY(hipMemcpy(out, t.nodes.p, (size_t)t.n_nodes * sizeof(Node4<float>), hipMemcpyDeviceToDevice));
    return TAKE_OK;
}
int wide_nodes_device(const DeviceTree &t, Node4<double> *out) {
    hipLaunchKernelGGL(lbvh::k_widen_nodes, blocks_for(t.n_nodes), dim3(lbvh::BLK), 0, nullptr, t.nodes.p, (int)t.n_nodes, out);
    return TAKE_OK;
}
// the builder's default: 1 primitive per leaf — two Morton neighbours need not be close, and a leaf box around both costs
// more primitive tests than the extra node (1M soup, 16 spp: 1 / 2 / 4 per leaf = 55.2 / 38.3 / 30.0 Msamples/s)
int device_leaf_size(int max_leaf) { return std::max(1, std::min(max_leaf > 0 ? max_leaf : 1, (int)MAX_LEAF)); }

// Finished float trees -> the scene's node array: one tree (the scene's only one) or many (the top-level tree of a
// two-level scene, then the prototypes'); trees[i]'s nodes land at at[i], at[trees.size()] nodes in all.  Every tree is
// quantised on its own grid into sc.qnodes and the worst inflation decides for the whole scene, by the host path's
// rule (quantise_trees): above Q_MAX_INFLATION and not forced — or not wanted at all — sc.qnodes is given back and
// sc.nodes gets the full-width nodes (an f32 scene of one tree: the collapse's own buffer, no copy).  Child words stay
// local to each tree.  Out: the format, every tree's grid (when compressed_ok); in sc.host the inflation and trees[0]'s grid.
template <class R>
int assemble_nodes(SceneT<R> &sc, const std::vector<DeviceTree *> &trees, const std::vector<int64_t> &at, bool compressed_ok,
                   bool compressed_forced, BuildMemory &mem, bool &compressed, std::vector<QGrid> &grids) {
    HostScene<R> &h = sc.host;
    const size_t n_nodes = (size_t)at[trees.size()];
    compressed = false;
    grids.assign(trees.size(), QGrid{});
    if (compressed_ok) {
        DevBuf<double> acc;
        HIP_TRY(sc.qnodes.alloc(n_nodes));
        HIP_TRY(acc.alloc(2));
        mem.sample("compression");
        for (size_t i = 0; i < trees.size(); i++) {
            double infl = 1.0;
            const int rq = quantise_tree_device(*trees[i], sc.qnodes.p + at[i], acc, grids[i], infl);
            if (rq) return rq;
            h.q_inflation = i ? std::max(h.q_inflation, infl) : infl;
        }
        for (int a = 0; a < 3; a++) h.grid_lo[a] = grids[0].lo[a], h.grid_step[a] = grids[0].step[a];
        compressed = compressed_forced || h.q_inflation <= Q_MAX_INFLATION;
        if (!compressed) sc.qnodes.release();
    }
    if (compressed) return TAKE_OK;
    if constexpr (sizeof(R) == 4)
        if (trees.size() == 1) {
            sc.nodes = std::move(trees[0]->nodes);
            return TAKE_OK;
        }
    HIP_TRY(sc.nodes.alloc(n_nodes));
    mem.sample("wide nodes");
    for (size_t i = 0; i < trees.size(); i++) {
        const int rw = wide_nodes_device(*trees[i], sc.nodes.p + at[i]);
        if (rw) return rw;
    }
    return TAKE_OK;
}
// host-side statistics of a device-built scene, before its nodes are assembled; the root is node 0 of the first tree
template <class R> void init_stats(HostScene<R> &h, int64_t n_nodes, int64_t n_prims, int depth) {
    h.stats = WideBvhStats{};
    h.stats.n_nodes = n_nodes, h.stats.n_prims = n_prims, h.stats.depth = depth;
    h.root_child = 0;
    h.q_inflation = 1.0;
}

// BVH build on the device of a scene without placements.  In: sc.prims uploaded in SHAPE order.  Out: the records in
// leaf order, sc.nodes or sc.qnodes, host-side stats and grid.  A double scene refused compression gets its float nodes widened.
template <class R> int build_bvh_device(SceneT<R> &sc, int max_leaf, bool compressed_ok, bool compressed_forced, BuildVerdict &why) {
    using namespace lbvh;
    const int n = (int)sc.prims.n;
    const int leaf_size = device_leaf_size(max_leaf);
    if ((n + leaf_size - 1) / leaf_size < 2) return why = BuildVerdict::TooFewLeaves, TAKE_OK;
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    BuildMemory mem(sizeof(R) == 4 ? "f32" : "f64");
    DevBuf<Box> pb;
    DevBuf<int> scene_ord;
    DeviceTree t;
    HIP_TRY(pb.alloc(n));
    HIP_TRY(scene_ord.alloc(6));
    HIP_TRY(reset_bounds(scene_ord));
    span_boxes(sc.prims.p, n, pb.p, scene_ord);
    const int rt = build_tree_device(pb, scene_ord, n, leaf_size, mem, t, why);
    if (rt || why != BuildVerdict::Built) return rt;
    init_stats(sc.host, t.n_nodes, n, t.depth);
    bool compressed;
    std::vector<QGrid> grids;
    const int ra = assemble_nodes(sc, {&t}, {0, t.n_nodes}, compressed_ok, compressed_forced, mem, compressed, grids);
    if (ra) return ra;
    t.nodes.release();
    // records into leaf order (a stable sort: coincident primitives stay in shape order): shape-order and leaf-order
    // records coexist, next to the permutation and the finished nodes only
    DevBuf<PrimRec<R>> prims_sorted;
    HIP_TRY(prims_sorted.alloc(n));
    mem.sample("permute");
    hipLaunchKernelGGL((k_permute<PrimRec<R>>), blocks_for(n), blk, 0, stream, sc.prims.p, t.order.p, n, prims_sorted.p);
    HIP_TRY(hipStreamSynchronize(stream));
    sc.prims = std::move(prims_sorted);  // (frees the shape-order records)
    HIP_TRY(hipGetLastError());
    mem.report();
    return TAKE_OK;
}

// Primitive records of one side on the device (tk_build_gpu.h::k_make_prims<R>) from the shared inputs; the face indices
// are the validated concatenation the shading side keeps anyway (sc.face_idx: uploaded by the first side, copied on
// the device by the second).
template <class R> lbvh::MeshSrc mesh_src(const HostScene<R> &h, const DeviceBuildInputs &in, int mesh) {
    const MeshInfo &mi = h.meshes[mesh];
    return lbvh::MeshSrc{in.pos_off[mesh], mi.fbase, mi.material, h.materials[mi.material].tag, (mi.nbase >= 0 || mi.uvbase >= 0) ? 1 : 0};
}
template <class R> int make_prims_on_device(SceneT<R> &sc, const TakeSceneDesc &d, DeviceBuildInputs &in, const double *const *device_positions) {
    using namespace lbvh;
    const int n = (int)d.n_shapes;
    HostScene<R> &h = sc.host;
    const int ru = in.upload(d, device_positions);
    if (ru) return ru;
    std::vector<MeshSrc> ms(d.n_meshes);
    for (int i = 0; i < d.n_meshes; i++) ms[i] = mesh_src(h, in, i);
    std::vector<SphereSrc> ss(d.n_spheres);
    for (int i = 0; i < d.n_spheres; i++) {
        const TakeSphere &s = d.spheres[i];
        ss[i] = SphereSrc{{s.center[0], s.center[1], s.center[2]}, s.radius, s.material_id, h.materials[s.material_id].tag};
    }
    DevBuf<MeshSrc> d_ms;
    DevBuf<SphereSrc> d_ss;
    if (in.face_idx) {
        HIP_TRY(sc.face_idx.alloc(h.face_idx.size()));
        if (sc.face_idx.n) HIP_TRY(hipMemcpy(sc.face_idx.p, in.face_idx, sc.face_idx.bytes(), hipMemcpyDeviceToDevice));
    } else {
        HIP_TRY(sc.face_idx.upload(h.face_idx));
        in.face_idx = sc.face_idx.p;
    }
    HIP_TRY(d_ms.upload(ms));
    HIP_TRY(d_ss.upload(ss));
    HIP_TRY(sc.prims.alloc((size_t)n));
    if (n > 0)  // (a two-level scene may consist of placements only)
        hipLaunchKernelGGL(k_make_prims<R>, dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), 0, nullptr, in.kind.p, in.ref.p, in.face.p,
                           in.area_light.p, d_ms.p, in.pos.p, sc.face_idx.p, d_ss.p, n, sc.prims.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));  // (a failed kernel is reported here, not by a later call)
    return TAKE_OK;
}

// per placement the empty bounds (six ordered long longs) that k_placement_boxes* grow and k_placement_pad reads
std::vector<long long> empty_tight(int n_inst) {
    std::vector<long long> tight(6 * (size_t)n_inst);
    for (size_t i = 0; i < tight.size(); i++) tight[i] = i % 6 < 3 ? INT64_MAX : INT64_MIN;
    return tight;
}
// Step 3's finish of a built top-level tree: the shapes' records `src` into leaf order at the head of dst (empty: the head alone, allocated
// here).  TooDeep: the traversal stack holds both levels (proto_depth: the prototypes') and one return marker.
template <class R> int finish_top_level(DeviceTree &top, int proto_depth, int n_shapes, int n_top, const PrimRec<R> *src, DevBuf<PrimRec<R>> &dst, BuildVerdict &why) {
    using namespace lbvh;
    if (3 * (top.depth + proto_depth) + 2 > MAX_STACK_ENTRIES) return why = BuildVerdict::TooDeep, TAKE_OK;
    DevBuf<int> is_shape, rank;
    DevBuf<char> temp;
    HIP_TRY(is_shape.alloc(n_top));
    HIP_TRY(rank.alloc(n_top));
    if (!dst.p) HIP_TRY(dst.alloc(n_shapes));
    hipLaunchKernelGGL(k_flag_shapes, blocks_for(n_top), dim3(BLK), 0, nullptr, top.order.p, n_top, n_shapes, is_shape.p);
    size_t temp_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, temp_bytes, is_shape.p, rank.p, 0, (size_t)n_top, rocprim::plus<int>(), nullptr));
    HIP_TRY(temp.alloc(temp_bytes));
    HIP_TRY(rocprim::exclusive_scan(temp.p, temp_bytes, is_shape.p, rank.p, 0, (size_t)n_top, rocprim::plus<int>(), nullptr));
    hipLaunchKernelGGL(k_top_leaves, blocks_for(top.n_nodes), dim3(BLK), 0, nullptr, top.nodes.p, (int)top.n_nodes, top.order.p, rank.p, n_shapes);
    if (n_shapes > 0)  // (a scene of placements only: nothing to write, and dst may be empty)
        hipLaunchKernelGGL((k_permute_top<PrimRec<R>>), blocks_for(n_top), dim3(BLK), 0, nullptr, src, top.order.p, rank.p, n_top, n_shapes, dst.p);
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipGetLastError());
    top.order.release();
    return TAKE_OK;
}
// The prototype pass, of a fresh build and of an update alike.  In: recs, a prototype's nf records in FACE order (the
// caller's to free).  Out: t — boxes, tree, the float nodes cut to size (the collapse allocates a node per leaf and uses
// about a third; they wait for the assembly), `order` released — and the records in its leaf order at dst, their place
// in the scene's record array.  scene_ord: six ints of scratch.  Any verdict but Built: nothing else was made.
template <class R>
int prototype_pass(const PrimRec<R> *recs, int nf, int leaf_size, PrimRec<R> *dst, DevBuf<int> &scene_ord, BuildMemory &mem, DeviceTree &t, BuildVerdict &why) {
    using namespace lbvh;
    DevBuf<Box> pb;
    HIP_TRY(pb.alloc(nf));
    HIP_TRY(reset_bounds(scene_ord));
    span_boxes(recs, nf, pb.p, scene_ord);
    const int rt = build_tree_device(pb, scene_ord, nf, leaf_size, mem, t, why);
    if (rt || why != BuildVerdict::Built) return rt;
    hipLaunchKernelGGL((k_permute<PrimRec<R>>), blocks_for(nf), dim3(BLK), 0, nullptr, recs, t.order.p, nf, dst);
    DevBuf<Node4<float>> cut;
    HIP_TRY(cut.alloc((size_t)t.n_nodes));
    HIP_TRY(hipMemcpy(cut.p, t.nodes.p, cut.bytes(), hipMemcpyDeviceToDevice));
    t.nodes = std::move(cut);
    t.order.release();
    return TAKE_OK;
}

// BVH build on the device of a two-level scene (TakeInstance placements, TAKE_INSTANCES_TWO_LEVEL): the scene
// build_host_trees makes, with LBVH trees.  In: sc.prims = the shapes' records in shape order (possibly none),
// sc.face_idx, sc.host as prepare_scene(PREP_DEVICE_BUILD) leaves it (the placements' records and the PlacementPlan),
// `in` still holding the positions.  Out: sc.prims = the top-level tree's records in leaf order, then each prototype's;
// sc.qnodes or sc.nodes = the top-level tree's nodes, then each prototype's, child words global; the placements'
// root_child and grid; stats.  Any verdict but Built is for the whole scene: a tree of fewer than two leaves (a
// one-face prototype) or too deep a stack over both levels.
//   1. per distinct prototype k_make_proto_prims, then prototype_pass: its records go straight to their place behind
//      the shapes' records, its float nodes wait for step 4;
//   2. k_placement_boxes / k_placement_pad: the placements' boxes behind the shapes' boxes (host formula beyond 4e8
//      vertex transforms, placement_box);
//   3. the top-level tree over both, ONE entry per leaf whatever max_leaf is (a placement is a leaf of its own, and
//      the compacted record ranges of k_top_leaves are single records); finish_top_level;
//   4. every tree quantised on its own grid into the scene's node array — the worst inflation over all trees decides
//      for the whole scene between compressed and full-width nodes, as quantise_trees does — and k_rebase.
template <class R>
int build_two_level_device(SceneT<R> &sc, const TakeSceneDesc &d, const DeviceBuildInputs &in, int max_leaf, bool compressed_ok, bool compressed_forced, BuildVerdict &why) {
    using namespace lbvh;
    HostScene<R> &h = sc.host;
    const PlacementPlan &plan = h.placements;
    const int n_shapes = (int)d.n_shapes, n_inst = (int)d.n_instances, n_top = n_shapes + n_inst;
    const int n_protos = (int)plan.proto_mesh.size();
    const int leaf_size = device_leaf_size(max_leaf);
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    BuildMemory mem(sizeof(R) == 4 ? "f32" : "f64");
    if (n_top < 2) return why = BuildVerdict::TooFewLeaves, TAKE_OK;
    std::vector<int64_t> prim_base(n_protos + 1), node_at(n_protos + 2, 0);  // node_at: the top-level tree's nodes (0), each prototype's, the end
    prim_base[0] = n_shapes;
    for (int k = 0; k < n_protos; k++) {
        const int64_t nf = d.meshes[plan.proto_mesh[k]].n_faces;
        if ((nf + leaf_size - 1) / leaf_size < 2) return why = BuildVerdict::TooFewLeaves, TAKE_OK;
        prim_base[k + 1] = prim_base[k] + nf;
    }
    if (prim_base[n_protos] >= ((int64_t)1 << 28)) return fail(TAKE_E_INVALID, "too many primitive records for the 4-wide leaf encoding (2^28)");
    DevBuf<PrimRec<R>> prims;  // the scene's records
    HIP_TRY(prims.alloc((size_t)prim_base[n_protos]));
    DevBuf<int> scene_ord;
    HIP_TRY(scene_ord.alloc(6));

    // 1. the prototypes' trees
    std::vector<DeviceTree> protos(n_protos);
    int proto_depth = 0;
    for (int k = 0; k < n_protos; k++) {
        const int mesh = plan.proto_mesh[k], nf = (int)d.meshes[mesh].n_faces;
        DevBuf<PrimRec<R>> recs;
        HIP_TRY(recs.alloc(nf));
        hipLaunchKernelGGL(k_make_proto_prims<R>, blocks_for(nf), blk, 0, stream, mesh_src(h, in, mesh), mesh, in.pos.p, sc.face_idx.p, nf, recs.p);
        const int rt = prototype_pass(recs.p, nf, leaf_size, prims.p + prim_base[k], scene_ord, mem, protos[k], why);
        if (rt || why != BuildVerdict::Built) return rt;
        proto_depth = std::max(proto_depth, protos[k].depth);
    }
    mem.sample("prototypes");

    // 2. the placements' boxes, behind the shapes'
    DevBuf<Box> pb;
    HIP_TRY(pb.alloc(n_top));
    HIP_TRY(reset_bounds(scene_ord));
    span_boxes(sc.prims.p, n_shapes, pb.p, scene_ord);
    {
        std::vector<long long> tight_h = empty_tight(n_inst);
        std::vector<double> xf(12 * (size_t)n_inst);
        std::vector<std::vector<int32_t>> of_proto(n_protos);
        for (int i = 0; i < n_inst; i++) {
            std::memcpy(&xf[12 * (size_t)i], d.instances[i].xform, 12 * sizeof(double));
            of_proto[plan.inst_proto[i]].push_back(i);
        }
        // beyond 4e8 vertex transforms (placement_box's rule): the object box's corners under the transform, cut by the
        // image of its bounding sphere — the object box being the tree's float bounds, which contain the host's box
        std::vector<char> tight_on_device(n_protos);
        for (int k = 0; k < n_protos; k++) {
            const TakeMesh &m = d.meshes[plan.proto_mesh[k]];
            tight_on_device[k] = (double)m.n_vertices * (double)d.n_instances <= 4e8;
            if (tight_on_device[k]) continue;
            Bounds ob;
            ob.grow(protos[k].lo, protos[k].hi);
            for (int32_t i : of_proto[k]) {
                const Bounds w = placement_box(d, m, ob, Affine3{d.instances[i].xform});
                for (int a = 0; a < 3; a++) tight_h[6 * (size_t)i + a] = d2ord(w.lo[a]), tight_h[6 * (size_t)i + 3 + a] = d2ord(w.hi[a]);
            }
        }
        DevBuf<long long> tight;
        DevBuf<double> xforms;
        DevBuf<int32_t> ids;
        HIP_TRY(tight.upload(tight_h));
        HIP_TRY(xforms.upload(xf));
        for (int k = 0; k < n_protos; k++) {
            if (!tight_on_device[k]) continue;
            const int mesh = plan.proto_mesh[k];
            const int64_t nv = d.meshes[mesh].n_vertices;
            const int chunks = (int)((nv + PLACEMENT_CHUNK - 1) / PLACEMENT_CHUNK);
            HIP_TRY(ids.upload(of_proto[k]));  // (frees the previous prototype's list: waits for its kernel)
            hipLaunchKernelGGL(k_placement_boxes, dim3((unsigned)((int64_t)chunks * (int64_t)of_proto[k].size())), blk, 0, stream,
                               in.pos.p + 3 * in.pos_off[mesh], nv, chunks, ids.p, xforms.p, tight.p);
        }
        hipLaunchKernelGGL(k_placement_pad<R>, blocks_for(n_inst), blk, 0, stream, tight.p, n_inst, n_shapes, pb.p, scene_ord.p);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipGetLastError());
    }

    // 3. the top-level tree
    DeviceTree top;
    int rt = build_tree_device(pb, scene_ord, n_top, 1, mem, top, why);
    if (!rt && why == BuildVerdict::Built) rt = finish_top_level(top, proto_depth, n_shapes, n_top, sc.prims.p, prims, why);
    if (rt || why != BuildVerdict::Built) return rt;
    sc.prims = std::move(prims);  // (frees the shape-order records)

    // 4. assembly: the top-level tree's nodes, then each prototype's
    std::vector<DeviceTree *> trees{&top};
    for (DeviceTree &t : protos) trees.push_back(&t);
    for (int k = 0; k <= n_protos; k++) node_at[k + 1] = node_at[k] + trees[k]->n_nodes;
    const int64_t n_nodes = node_at[n_protos + 1];
    if (n_nodes >= ((int64_t)1 << 31)) return fail(TAKE_E_INVALID, "too many nodes");
    init_stats(h, n_nodes, n_shapes, top.depth + proto_depth);
    h.n_blas = n_protos, h.blas_nodes = n_nodes - top.n_nodes, h.blas_prims = prim_base[n_protos] - n_shapes;
    h.blas_depth = proto_depth;
    h.blas_prim_first.assign(prim_base.begin(), prim_base.begin() + n_protos), h.blas_prim_count.resize(n_protos);
    for (int k = 0; k < n_protos; k++) h.blas_prim_count[k] = prim_base[k + 1] - prim_base[k];
    h.blas_mesh = plan.proto_mesh, h.blas_node_first.assign(node_at.begin() + 1, node_at.begin() + 1 + n_protos);
    h.blas_node_count.resize(n_protos), h.blas_depths.resize(n_protos);
    for (int k = 0; k < n_protos; k++) h.blas_node_count[k] = protos[k].n_nodes, h.blas_depths[k] = protos[k].depth;
    bool use_q;
    std::vector<QGrid> grids;  // [1 + k]: prototype k's
    const int ra = assemble_nodes(sc, trees, node_at, compressed_ok, compressed_forced, mem, use_q, grids);
    if (ra) return ra;
    for (int k = 0; k < n_protos; k++) {
        const int nk = (int)protos[k].n_nodes;
        const int32_t node_base = (int32_t)node_at[1 + k];
        if (use_q) hipLaunchKernelGGL(k_rebase<QNode4>, blocks_for(nk), blk, 0, stream, sc.qnodes.p + node_base, nk, node_base, (int32_t)prim_base[k]);
        else hipLaunchKernelGGL(k_rebase<Node4<R>>, blocks_for(nk), blk, 0, stream, sc.nodes.p + node_base, nk, node_base, (int32_t)prim_base[k]);
    }
    // (a prototype's root is node 0 of its tree: it has at least two leaves)
    for (int i = 0; i < n_inst; i++) {
        const int k = plan.inst_proto[i];
        InstTrace<R> &it = h.inst_trace[i];
        it.root_child = (int32_t)node_at[1 + k];
        if (compressed_ok)
            for (int a = 0; a < 3; a++) it.grid_lo[a] = grids[1 + k].lo[a], it.grid_step[a] = grids[1 + k].step[a];
    }
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());
    mem.report();
    return TAKE_OK;
}


// The top level of a RESIDENT two-level scene made again, for the re-pose and for the update of a scene's meshes.  In: `head`, the n_shapes records of the
// shapes, in any order; `prims`, the record array whose spans h.blas_prim_first / _count hold the prototypes' records;
// the transforms (12 doubles per placement, device memory); proto_depth: the deepest prototype tree.  Out: `top`, its
// leaf words final (instance words, single records), and the shapes' records in its leaf order at the head of dst
// (empty: allocated here, the head alone).  Errors start with "unsupported" where no tree can be made.
//   2. tight world boxes from the prototypes' records (k_placement_boxes_resident), widened (k_widen_tight) and
//      padded (k_placement_pad) behind 3. the shapes' boxes from theirs;
//   4. the top-level tree, one entry per leaf, and its records.  Where the shapes come out of an OLD leaf order, not
//      the shape order a fresh build sorts, results do not depend on it.  Box tests are conservative, and a tie between
//      coincident primitives is decided by values — inside the top level by the position of the record, where every
//      group of coincident records holds its shape ids in ascending order (order_coincident; a stable sort of the shape
//      order) and keeps them so here: equal geometry is equal boxes is equal Morton codes, and the sort is stable.
template <class R>
int top_level_resident(const HostScene<R> &h, const PrimRec<R> *head, const PrimRec<R> *prims, int n_shapes, const double *d_xforms, int n_inst,
                       int proto_depth, BuildMemory &mem, DeviceTree &top, DevBuf<PrimRec<R>> &dst) {
    using namespace lbvh;
    const int n_protos = (int)h.blas_prim_first.size(), n_top = n_shapes + n_inst;
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    DevBuf<Box> pb;
    DevBuf<int> scene_ord;
    HIP_TRY(pb.alloc(n_top));
    HIP_TRY(scene_ord.alloc(6));
    HIP_TRY(reset_bounds(scene_ord));
    span_boxes(head, n_shapes, pb.p, scene_ord);
    {
        std::vector<int2> span_h((size_t)n_inst);
        std::vector<int64_t> block0_h((size_t)n_inst + 1, 0);
        const std::vector<long long> tight_h = empty_tight(n_inst);
        for (int i = 0; i < n_inst; i++) {
            const int k = h.placements.inst_proto[i];
            if (k < 0 || k >= n_protos) return fail(TAKE_E_INVALID, "the scene does not know the prototype of placement " + std::to_string(i));
            span_h[i] = make_int2((int)h.blas_prim_first[k], (int)h.blas_prim_count[k]);
            block0_h[i + 1] = block0_h[i] + (h.blas_prim_count[k] + REPOSE_CHUNK - 1) / REPOSE_CHUNK;
        }
        if (block0_h[n_inst] >= ((int64_t)1 << 31)) return fail(TAKE_E_INVALID, "unsupported: too many prototype records times placements for one launch");
        DevBuf<int2> span;
        DevBuf<int64_t> block0;
        DevBuf<long long> tight, maxabs;
        HIP_TRY(span.upload(span_h));
        HIP_TRY(block0.upload(block0_h));
        HIP_TRY(tight.upload(tight_h));
        HIP_TRY(maxabs.alloc(n_inst));
        HIP_TRY(hipMemsetAsync(maxabs.p, 0, maxabs.bytes(), stream));
        hipLaunchKernelGGL(k_placement_boxes_resident<R>, dim3((unsigned)block0_h[n_inst]), blk, 0, stream, prims, span.p, block0.p, n_inst, d_xforms,
                           tight.p, maxabs.p);
        hipLaunchKernelGGL(k_widen_tight<R>, blocks_for(n_inst), blk, 0, stream, tight.p, maxabs.p, d_xforms, n_inst);
        hipLaunchKernelGGL(k_placement_pad<R>, blocks_for(n_inst), blk, 0, stream, tight.p, n_inst, n_shapes, pb.p, scene_ord.p);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipGetLastError());
    }
    BuildVerdict why = BuildVerdict::Built;
    int rt = build_tree_device(pb, scene_ord, n_top, 1, mem, top, why);
    if (!rt && why == BuildVerdict::Built) rt = finish_top_level(top, proto_depth, n_shapes, n_top, head, dst, why);
    return rt || why != BuildVerdict::Built ? unsupported(rt, why, "top-level tree") : TAKE_OK;
}

// "This tree's nodes at dst, its grid out", once per node format of a resident scene: compressed on the tree's own grid
// (acc: quantise_tree_device's scratch, allocated by the first call; the inflation is not consulted — the scene keeps
// its format, and the box tests stay conservative), or full-width, which has no grid and leaves the caller's as it is.
int put_nodes(const DeviceTree &t, QNode4 *dst, DevBuf<double> &acc, float *grid_lo, float *grid_step) {
    QGrid g;
    double inflation = 1.0;
    if (!acc.p) HIP_TRY(acc.alloc(2));
    if (const int rq = quantise_tree_device(t, dst, acc, g, inflation)) return rq;
    for (int a = 0; a < 3; a++) grid_lo[a] = g.lo[a], grid_step[a] = g.step[a];
    return TAKE_OK;
}
template <class R> int put_nodes(const DeviceTree &t, Node4<R> *dst, DevBuf<double> &, float *, float *) { return wide_nodes_device(t, dst); }

// Node assembly for a RESIDENT two-level scene in the node format it keeps (NodeT; old, nodes: its array and the new
// one, out's): [new top level][prototype 0][prototype 1]...  Per prototype either its new tree (fresh[k]: put into
// place, rebased to its nodes and records, its float nodes freed) or null = untouched: the scene's nodes copied and
// rebased by their own node shift, primitive shift 0 — a run of untouched neighbours shares its shift: one copy, one
// launch.  Out: everything of `out` but the depth (full-width nodes: the grid stays the scene's, which the traversal
// does not read), and per prototype what its placements have to be told (target: k_retarget_placements).
template <class R, class NodeT>
int assemble_resident_nodes(const HostScene<R> &h, const DevBuf<NodeT> &old, const DeviceTree &top, const std::vector<DeviceTree *> &fresh, DevBuf<NodeT> &nodes,
                            ResidentNodes<R> &out, std::vector<lbvh::ProtoTarget> &target) {
    using namespace lbvh;
    const int n_protos = (int)fresh.size();
    const char *lost = "unsupported: the scene does not know where its prototypes are";
    if ((int)h.blas_node_first.size() != n_protos || (int)h.blas_node_count.size() != n_protos || (int)h.blas_prim_first.size() != n_protos) return fail(TAKE_E_INVALID, lost);
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    out.node_first.assign(n_protos, 0), out.node_count = h.blas_node_count;
    out.n_nodes = top.n_nodes;
    for (int k = 0; k < n_protos; k++) {
        if (fresh[k]) out.node_count[k] = fresh[k]->n_nodes;
        out.node_first[k] = out.n_nodes, out.n_nodes += out.node_count[k];
    }
    out.blas_nodes = out.n_nodes - top.n_nodes;
    if (out.n_nodes >= ((int64_t)1 << 31) || (uint64_t)out.n_nodes * sizeof(NodeT) >= (1ull << 32))
        return fail(TAKE_E_INVALID, "unsupported: too many nodes for the 32-bit record offsets of the trace kernels");
    target.assign(n_protos, ProtoTarget{});
    DevBuf<double> acc;
    for (int a = 0; a < 3; a++) out.grid_lo[a] = h.grid_lo[a], out.grid_step[a] = h.grid_step[a];
    HIP_TRY(nodes.alloc((size_t)out.n_nodes));
    if (const int rc = put_nodes(top, nodes.p, acc, out.grid_lo, out.grid_step)) return rc;
    for (int k = 0; k < n_protos;) {
        const int32_t first = (int32_t)out.node_first[k];
        if (fresh[k]) {
            const int nk = (int)fresh[k]->n_nodes;
            target[k].moved = 1, target[k].root = first, target[k].has_grid = std::is_same<NodeT, QNode4>::value;
            if (const int rc = put_nodes(*fresh[k], nodes.p + first, acc, target[k].grid_lo, target[k].grid_step)) return rc;
            hipLaunchKernelGGL(k_rebase<NodeT>, blocks_for(nk), blk, 0, stream, nodes.p + first, nk, first, (int32_t)h.blas_prim_first[k]);
            fresh[k]->nodes.release();
            k++;
            continue;
        }
        int e = k;
        int64_t run = 0;
        while (e < n_protos && !fresh[e]) run += h.blas_node_count[e], e++;
        const int64_t old_first = h.blas_node_first[k], shift = (int64_t)first - old_first;
        for (int j = k; j < e; j++) target[j].shift = (int32_t)shift;
        if (run > 0) {
            if (old_first < 0 || old_first + run > h.stats.n_nodes) return fail(TAKE_E_INVALID, lost);
            HIP_TRY(hipMemcpyAsync(nodes.p + first, old.p + old_first, (size_t)run * sizeof(NodeT), hipMemcpyDeviceToDevice, stream));
            if (shift) hipLaunchKernelGGL(k_rebase<NodeT>, blocks_for(run), blk, 0, stream, nodes.p + first, (int)run, (int32_t)shift, 0);
        }
        k = e;
    }
    return TAKE_OK;
}
// ... the node type chosen, once, by the format the scene traverses (Q8 scenes are refused before any of this)
template <class R> int assemble_resident_nodes(const SceneT<R> &sc, const DeviceTree &top, const std::vector<DeviceTree *> &fresh, ResidentNodes<R> &out, std::vector<lbvh::ProtoTarget> &target) {
    return sc.trace.nodes == NodeFormat::Q4 ? assemble_resident_nodes(sc.host, sc.qnodes, top, fresh, out.qnodes, out, target)
                                            : assemble_resident_nodes(sc.host, sc.nodes, top, fresh, out.nodes, out, target);
}
// What a stage's commit() does with them, last — it binds the scene's arrays: the scene takes the nodes and where the
// prototypes' are (the new top-level tree has at least two leaves: its root is node 0)
template <class R> void install_resident_nodes(SceneT<R> &sc, ResidentNodes<R> &t) {
    if (t.qnodes.p) sc.qnodes = std::move(t.qnodes);
    else sc.nodes = std::move(t.nodes);
    sc.host.blas_node_first = std::move(t.node_first), sc.host.blas_node_count = std::move(t.node_count), sc.host.blas_nodes = t.blas_nodes;
    install_tree(sc, t.n_nodes, t.depth, 0, t.grid_lo, t.grid_step);
}

// The placements' records under transforms they were not made from (d_xforms: 12 doubles each, device memory): trace
// and shade, allocated here, from the scene's and the transforms.  A transform that cannot be inverted is refused.
template <class R> int placement_records(const SceneT<R> &sc, const double *d_xforms, int n_inst, DevBuf<InstTrace<R>> &trace, DevBuf<InstShade<R>> &shade) {
    using namespace lbvh;
    FirstOffender<int> bad{INT32_MAX};
    HIP_TRY(trace.alloc((size_t)n_inst));
    HIP_TRY(shade.alloc((size_t)n_inst));
    HIP_TRY(bad.arm());
    hipLaunchKernelGGL(k_placement_records<R>, blocks_for(n_inst), dim3(BLK), 0, nullptr, d_xforms, n_inst, sc.inst_trace.p, sc.inst_shade.p, trace.p, shade.p, bad.cell.p);
    HIP_TRY(bad.read());
    HIP_TRY(hipGetLastError());
    if (bad.first != bad.none) return fail(TAKE_E_INVALID, "instance " + std::to_string(bad.first) + ": singular or non-finite transform");
    return TAKE_OK;
}

// The shapes' records — the first n_shapes of the scene's, in the leaf order of the tree that is being replaced — back in
// SHAPE order at dst, with new geometry where their mesh has new positions (k_update_prims: the order a fresh build
// starts from, and the one k_update_lights reads).  bad: armed by the caller, who may go on feeding it
// (k_update_proto_prims) before new_position_refusal reads it: mesh << 32 | vertex of the first coordinate that is not finite.
template <class R>
void update_shape_records(const SceneT<R> &sc, int n_shapes, const MeshUpdateInputs &in, const int32_t *d_shape_face, PrimRec<R> *dst, FirstOffender<unsigned long long> &bad) {
    using namespace lbvh;
    if (n_shapes > 0)
        hipLaunchKernelGGL(k_update_prims<R>, blocks_for(n_shapes), dim3(BLK), 0, nullptr, sc.prims.p, n_shapes, in.d_pos.p, sc.meshes.p, d_shape_face, sc.face_idx.p, dst, bad.cell.p);
}
int new_position_refusal(FirstOffender<unsigned long long> &bad) {
    HIP_TRY(bad.read());
    HIP_TRY(hipGetLastError());
    if (bad.first == bad.none) return TAKE_OK;
    return fail(TAKE_E_INVALID, "mesh " + std::to_string(bad.first >> 32) + ": vertex " + std::to_string(bad.first & 0xffffffffull) + ": a new position is not finite");
}
// What stage_normals_and_lights staged in `built`, moved into the scene (new_normals / new_lights: which of it was made)
template <class R> void commit_normals_and_lights(SceneT<R> &sc, SceneT<R> &built, bool new_normals, bool new_lights) {
    if (new_normals) sc.normals = std::move(built.normals);
    if (!new_lights) return;
    sc.lights = std::move(built.lights), sc.light_pmf = std::move(built.light_pmf), sc.light_cdf = std::move(built.light_cdf);
    sc.host.lights = std::move(built.host.lights), sc.host.light_pmf = std::move(built.host.light_pmf), sc.host.light_cdf = std::move(built.host.light_cdf);
}

}  // namespace

namespace tk_host {

template <class R>
int build_side_on_device(SceneT<R> &sc, const TakeSceneDesc &d, DeviceBuildInputs &in, const double *const *device_positions, int max_leaf,
                         bool compressed_ok, bool compressed_forced, bool last_side, PhaseClock &clock) {
    const bool two_level = d.n_instances > 0;
    BuildVerdict why = BuildVerdict::Built;
    int rc = make_prims_on_device(sc, d, in, device_positions);
    // (positions and shape arrays: not part of the build's peak — but a two-level build reads the prototypes' positions)
    if (last_side && !two_level) in.release();
    clock.lap("mesh arrays -> HBM, records");
    if (!rc) rc = two_level ? build_two_level_device(sc, d, in, max_leaf, compressed_ok, compressed_forced, why)
                            : build_bvh_device(sc, max_leaf, compressed_ok, compressed_forced, why);
    if (last_side) in.release();
    return rc || why == BuildVerdict::Built ? rc : 1;  // (the one bare 1: "use the host builder", whatever the verdict)
}
template int build_side_on_device<float>(SceneT<float> &, const TakeSceneDesc &, DeviceBuildInputs &, const double *const *, int, bool, bool, bool, PhaseClock &);
template int build_side_on_device<double>(SceneT<double> &, const TakeSceneDesc &, DeviceBuildInputs &, const double *const *, int, bool, bool, bool, PhaseClock &);

// The re-pose, by its steps: placement_records — a transform that cannot be inverted is reported before anything else
// is made; top_level_resident over the shapes' records (the head of the record array, in the leaf order of the tree
// that is being replaced) and the prototypes' resident records; assemble_resident_nodes with every prototype untouched —
// one run, moved by the difference of the two top-level trees' sizes — and k_shift_roots for the placements' roots.
template <class R> int repose_two_level_device(const SceneT<R> &sc, const double *d_xforms, int64_t n64, ReposeStage<R> &out) {
    using namespace lbvh;
    const HostScene<R> &h = sc.host;
    const int n_inst = (int)n64;
    const int n_shapes = (int)((int64_t)sc.prims.n - h.blas_prims);
    BuildMemory mem(sizeof(R) == 4 ? "f32 (placements re-posed)" : "f64 (placements re-posed)");
    if (const int rc = placement_records(sc, d_xforms, n_inst, out.inst_trace, out.inst_shade)) return rc;
    DeviceTree top;
    const int rt = top_level_resident(sc.host, sc.prims.p, sc.prims.p, n_shapes, d_xforms, n_inst, h.blas_depth, mem, top, out.head);
    if (rt) return rt;
    out.tree.depth = top.depth + h.blas_depth;
    std::vector<ProtoTarget> target;  // (not uploaded: every shift is delta)
    const int ra = assemble_resident_nodes(sc, top, std::vector<DeviceTree *>(h.blas_prim_first.size(), nullptr), out.tree, target);
    if (ra) return ra;
    const int64_t delta = out.tree.n_nodes - h.stats.n_nodes;
    if (delta) hipLaunchKernelGGL(k_shift_roots<R>, blocks_for(n_inst), dim3(BLK), 0, nullptr, out.inst_trace.p, n_inst, (int32_t)delta);
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipGetLastError());
    mem.report();
    return TAKE_OK;
}
template <class R> int ReposeStage<R>::commit(SceneT<R> &sc) {
    if (head.n) HIP_TRY(hipMemcpy(sc.prims.p, head.p, head.bytes(), hipMemcpyDeviceToDevice));
    sc.inst_trace = std::move(inst_trace), sc.inst_shade = std::move(inst_shade);
    install_resident_nodes(sc, tree);  // (the prototypes' nodes moved with the top-level tree's size)
    return TAKE_OK;
}
template struct ReposeStage<float>;
template struct ReposeStage<double>;
template int repose_two_level_device<float>(const SceneT<float> &, const double *, int64_t, ReposeStage<float> &);
template int repose_two_level_device<double>(const SceneT<double> &, const double *, int64_t, ReposeStage<double> &);

// ---- take_hip_scene_set_mesh_vertices
int MeshUpdateInputs::upload(const std::vector<int64_t> &mesh_vertices, const TakeMeshUpdate *updates, int32_t n_updates) {
    pos.assign(mesh_vertices.size(), nullptr), nrm.assign(mesh_vertices.size(), nullptr);
    PinnedUploads pin;
    for (int32_t i = 0; i < n_updates; i++) {
        const TakeMeshUpdate &u = updates[i];
        const size_t words = 3 * (size_t)std::max<int64_t>(mesh_vertices[u.mesh], 1);  // (an empty mesh: one word nobody reads)
        const double *src[2] = {u.positions, u.normals};
        const double **dst[2] = {&pos[u.mesh], &nrm[u.mesh]};
        for (int k = 0; k < 2; k++) {
            if (!src[k]) continue;
            if (u.flags & TAKE_MESH_DEVICE_ARRAYS) {
                *dst[k] = src[k];
                continue;
            }
            owned.emplace_back();
            HIP_TRY(owned.back().alloc(words));
            HIP_TRY(pin.copy(owned.back().p, src[k], sizeof(double) * 3 * (size_t)mesh_vertices[u.mesh]));
            *dst[k] = owned.back().p;
        }
    }
    HIP_TRY(pin.finish());
    HIP_TRY(d_pos.upload(pos));
    HIP_TRY(d_nrm.upload(nrm));
    return TAKE_OK;
}

// What an update of meshes changes beside records and trees, staged in b so that a commit only moves (new_normals /
// new_lights: which of it was made).  recs: the n_shapes records of the shapes in SHAPE order, new geometry in them.
//   new vertex normals as the scene keeps them: a copy of the scene's whole array with the named meshes' parts rewritten;
//   the light records of emissive faces, and the power tables from them: light_power_tables is a sequential sum in R
//   in light order — the records come back and the host sums, as it does for a new scene.
template <class R>
static int stage_normals_and_lights(const SceneT<R> &sc, const MeshUpdateInputs &in, const std::vector<int64_t> &mesh_vertices, const int32_t *d_shape_face,
                                    const PrimRec<R> *recs, int n_shapes, SceneT<R> &b, bool &new_normals, bool &new_lights) {
    using namespace lbvh;
    const int n_lights = (int)sc.lights.n;
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    for (size_t m = 0; m < in.nrm.size(); m++) {
        if (!in.nrm[m] || mesh_vertices[m] <= 0) continue;
        if (!new_normals) {
            HIP_TRY(b.normals.alloc(sc.normals.n));
            HIP_TRY(hipMemcpyAsync(b.normals.p, sc.normals.p, sc.normals.bytes(), hipMemcpyDeviceToDevice, stream));
            new_normals = true;
        }
        const int64_t words = 3 * mesh_vertices[m];
        hipLaunchKernelGGL(k_convert_normals<R>, blocks_for(words), blk, 0, stream, in.nrm[m], words, b.normals.p + 3 * (size_t)sc.host.meshes[m].nbase);
    }
    if (n_lights > 0) {
        HIP_TRY(b.lights.alloc((size_t)n_lights));
        HIP_TRY(hipMemcpyAsync(b.lights.p, sc.lights.p, sc.lights.bytes(), hipMemcpyDeviceToDevice, stream));
        hipLaunchKernelGGL(k_update_lights<R>, blocks_for(n_lights), blk, 0, stream, b.lights.p, n_lights, recs, n_shapes, in.d_pos.p, in.d_nrm.p, sc.meshes.p,
                           d_shape_face, sc.face_idx.p);
        b.host.lights.resize((size_t)n_lights);
        HIP_TRY(hipMemcpy(b.host.lights.data(), b.lights.p, b.lights.bytes(), hipMemcpyDeviceToHost));
        HIP_TRY(hipGetLastError());
        light_power_tables(b.host);
        HIP_TRY(b.light_pmf.upload(b.host.light_pmf));
        HIP_TRY(b.light_cdf.upload(b.host.light_cdf));
        new_lights = true;
    }
    return TAKE_OK;
}

// The update of a scene without placements, by its steps: update_shape_records — a coordinate that is not finite is
// reported before anything else is made; stage_normals_and_lights; creation's tail (build_bvh_device: boxes, tree, nodes
// in the format the inflation rule chooses, records into leaf order), and a trace state where the format changed.
template <class R>
int update_mesh_vertices_device(const SceneT<R> &sc, const MeshUpdateInputs &in, const std::vector<int64_t> &mesh_vertices, const int32_t *d_shape_face,
                                int max_leaf, bool compressed_ok, bool compressed_forced, int num_cus, MeshUpdateStage<R> &out) {
    const int n = (int)sc.prims.n;
    SceneT<R> &b = out.built;
    {
        FirstOffender<unsigned long long> bad{~0ull};
        HIP_TRY(b.prims.alloc((size_t)n));
        HIP_TRY(bad.arm());
        update_shape_records(sc, n, in, d_shape_face, b.prims.p, bad);
        if (const int rc = new_position_refusal(bad)) return rc;
    }
    const int rl = stage_normals_and_lights(sc, in, mesh_vertices, d_shape_face, b.prims.p, n, b, out.new_normals, out.new_lights);
    if (rl) return rl;
    BuildVerdict why = BuildVerdict::Built;
    const int rb = build_bvh_device(b, max_leaf, compressed_ok, compressed_forced, why);
    if (rb || why != BuildVerdict::Built) return unsupported(rb, why, "tree");
    b.trace = TraceKind{b.qnodes.p ? NodeFormat::Q4 : NodeFormat::WIDE, false};
    if ((uint64_t)b.host.stats.n_nodes * node_bytes<R>(b.trace.nodes) >= (1ull << 32))
        return fail(TAKE_E_INVALID, "unsupported: too many nodes for the 32-bit record offsets of the trace kernels");
    if (b.trace.nodes != sc.trace.nodes) {  // another trace kernel instance: its own grid and spill area
        const hipError_t e = alloc_trace_state(b, num_cus);
        if (e == hipErrorOutOfMemory) return fail(TAKE_E_NOMEM, "out of device memory for the trace state");
        HIP_TRY(e);
        out.new_trace_state = true;
    }
    return TAKE_OK;
}
template <class R> int MeshUpdateStage<R>::commit(SceneT<R> &sc) {
    commit_normals_and_lights(sc, built, new_normals, new_lights);
    sc.prims = std::move(built.prims);
    sc.qnodes = std::move(built.qnodes), sc.nodes = std::move(built.nodes);  // (the one the new format does not use is empty: the scene's is freed)
    sc.host.stats = built.host.stats, sc.host.q_inflation = built.host.q_inflation, sc.host.node_width = 4;  // (stats: n_prims and sah too)
    install_tree(sc, built.host.stats.n_nodes, built.host.stats.depth, built.host.root_child, built.host.grid_lo, built.host.grid_step);
    sc.trace = built.trace;
    sc.built_on_device = true;  // whoever built the tree that is gone
    if (new_trace_state) sc.trace_state = std::move(built.trace_state);
    return TAKE_OK;
}
template struct MeshUpdateStage<float>;
template struct MeshUpdateStage<double>;
template int update_mesh_vertices_device<float>(const SceneT<float> &, const MeshUpdateInputs &, const std::vector<int64_t> &, const int32_t *, int, bool, bool,
                                                int, MeshUpdateStage<float> &);
template int update_mesh_vertices_device<double>(const SceneT<double> &, const MeshUpdateInputs &, const std::vector<int64_t> &, const int32_t *, int, bool, bool,
                                                 int, MeshUpdateStage<double> &);

// ---- take_hip_scene_update_meshes on a two-level scene, by its steps:
//   1. the records: update_shape_records, and k_update_proto_prims for the moved prototypes', in face order, feeding the
//      same offender cell — a coordinate that is not finite, in either role, is reported before anything else is made;
//   2. stage_normals_and_lights;
//   3. per prototype prototype_pass, or its records copied to their place in the new record array;
//   4. top_level_resident under d_xforms: the shapes' boxes from their new records, the placements' from the
//      prototypes' records as they are now; the shapes' records into leaf order at the head of the new array;
//   5. assemble_resident_nodes;
//   6. the placements: their records as they are — transforms, materials, tags, shape bases — or, new_records,
//      placement_records under d_xforms; then k_retarget_placements to the roots, and the moved prototypes' grids, of
//      the new node array.
template <class R>
int update_two_level_meshes_device(const SceneT<R> &sc, const MeshUpdateInputs &in, const std::vector<int64_t> &mesh_vertices, const int32_t *d_shape_face,
                                   const double *d_xforms, int max_leaf, bool new_records, ProtoUpdateStage<R> &out) {
    using namespace lbvh;
    const HostScene<R> &h = sc.host;
    const int n_inst = (int)sc.inst_trace.n, n_protos = (int)h.blas_prim_first.size();
    const int n_shapes = (int)((int64_t)sc.prims.n - h.blas_prims);
    const int leaf_size = device_leaf_size(max_leaf);
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    BuildMemory mem(sizeof(R) == 4 ? "f32 (meshes updated)" : "f64 (meshes updated)");
    SceneT<R> &b = out.built;
    if ((int)h.blas_mesh.size() != n_protos || (int)h.blas_node_first.size() != n_protos || (int)h.blas_node_count.size() != n_protos ||
        (int)h.blas_depths.size() != n_protos || (int)h.placements.inst_proto.size() != n_inst || n_shapes < 0)
        return fail(TAKE_E_INVALID, "unsupported: the scene does not know where its prototypes are");
    std::vector<DeviceTree> trees(n_protos);
    std::vector<DeviceTree *> fresh(n_protos, nullptr);  // the moved prototypes' trees (step 3 builds them), null: untouched
    for (int k = 0; k < n_protos; k++) {
        const int32_t mesh = h.blas_mesh[k];
        if (mesh < 0 || (size_t)mesh >= in.pos.size() || (size_t)mesh >= h.meshes.size()) return fail(TAKE_E_INVALID, "unsupported: the scene does not know the mesh of prototype " + std::to_string(k));
        if (in.pos[mesh]) fresh[k] = &trees[k];
        if (fresh[k] && (h.blas_prim_count[k] + leaf_size - 1) / leaf_size < 2) return unsupported(TAKE_OK, BuildVerdict::TooFewLeaves, "prototype tree");
    }

    // 1.
    DevBuf<PrimRec<R>> shapes;              // shape order
    std::vector<DevBuf<PrimRec<R>>> faces(n_protos);  // face order, moved prototypes only
    {
        FirstOffender<unsigned long long> bad{~0ull};
        HIP_TRY(shapes.alloc((size_t)n_shapes));
        HIP_TRY(bad.arm());
        update_shape_records(sc, n_shapes, in, d_shape_face, shapes.p, bad);
        for (int k = 0; k < n_protos; k++) {
            if (!fresh[k]) continue;
            const int32_t mesh = h.blas_mesh[k];
            const MeshInfo &mi = h.meshes[mesh];
            const int nf = (int)h.blas_prim_count[k];
            const MeshSrc src{0, mi.fbase, mi.material, h.materials[mi.material].tag, (mi.nbase >= 0 || mi.uvbase >= 0) ? 1 : 0};
            HIP_TRY(faces[k].alloc((size_t)nf));
            hipLaunchKernelGGL(k_update_proto_prims<R>, blocks_for(nf), blk, 0, stream, src, mesh, in.pos[mesh], sc.face_idx.p, nf, faces[k].p, bad.cell.p);
        }
        if (const int rc = new_position_refusal(bad)) return rc;
    }

    // 2.
    const int rl = stage_normals_and_lights(sc, in, mesh_vertices, d_shape_face, shapes.p, n_shapes, b, out.new_normals, out.new_lights);
    if (rl) return rl;

    // 3.
    HIP_TRY(b.prims.alloc(sc.prims.n));
    DevBuf<int> scene_ord;
    HIP_TRY(scene_ord.alloc(6));
    out.depths = h.blas_depths;
    for (int k = 0; k < n_protos; k++) {
        const int nf = (int)h.blas_prim_count[k];
        PrimRec<R> *at = b.prims.p + h.blas_prim_first[k];
        if (!fresh[k]) {
            HIP_TRY(hipMemcpyAsync(at, sc.prims.p + h.blas_prim_first[k], (size_t)nf * sizeof(PrimRec<R>), hipMemcpyDeviceToDevice, stream));
            continue;
        }
        BuildVerdict why = BuildVerdict::Built;
        const int rt = prototype_pass(faces[k].p, nf, leaf_size, at, scene_ord, mem, trees[k], why);
        if (rt || why != BuildVerdict::Built) return unsupported(rt, why, "prototype tree");
        faces[k].release();
        out.depths[k] = trees[k].depth;
    }
    out.blas_depth = 0;
    for (int k = 0; k < n_protos; k++) out.blas_depth = std::max(out.blas_depth, out.depths[k]);
    mem.sample("prototypes");

    // 4.
    DeviceTree top;
    const int rt = top_level_resident(h, shapes.p, b.prims.p, n_shapes, d_xforms, n_inst, out.blas_depth, mem, top, b.prims);
    if (rt) return rt;
    shapes.release();
    out.tree.depth = top.depth + out.blas_depth;

    // 5.
    std::vector<ProtoTarget> target;
    const int ra = assemble_resident_nodes(sc, top, fresh, out.tree, target);
    if (ra) return ra;

    // 6.
    {
        DevBuf<int32_t> inst_proto;
        DevBuf<ProtoTarget> d_target;
        if (new_records) {
            if (const int rc = placement_records(sc, d_xforms, n_inst, b.inst_trace, b.inst_shade)) return rc;
        } else {
            HIP_TRY(b.inst_trace.alloc((size_t)n_inst));
            HIP_TRY(hipMemcpyAsync(b.inst_trace.p, sc.inst_trace.p, sc.inst_trace.bytes(), hipMemcpyDeviceToDevice, stream));
        }
        HIP_TRY(inst_proto.upload(h.placements.inst_proto));
        HIP_TRY(d_target.upload(target));
        hipLaunchKernelGGL(k_retarget_placements<R>, blocks_for(n_inst), blk, 0, stream, b.inst_trace.p, n_inst, inst_proto.p, d_target.p);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipGetLastError());
    }
    mem.report();
    return TAKE_OK;
}
template <class R> int ProtoUpdateStage<R>::commit(SceneT<R> &sc) {
    HostScene<R> &h = sc.host;
    commit_normals_and_lights(sc, built, new_normals, new_lights);
    sc.prims = std::move(built.prims);
    sc.inst_trace = std::move(built.inst_trace);
    if (built.inst_shade.p) sc.inst_shade = std::move(built.inst_shade);  // (new_records)
    h.blas_depths = std::move(depths), h.blas_depth = blas_depth;
    install_resident_nodes(sc, tree);
    return TAKE_OK;
}
template struct ProtoUpdateStage<float>;
template struct ProtoUpdateStage<double>;
template int update_two_level_meshes_device<float>(const SceneT<float> &, const MeshUpdateInputs &, const std::vector<int64_t> &, const int32_t *, const double *, int,
                                                   bool, ProtoUpdateStage<float> &);
template int update_two_level_meshes_device<double>(const SceneT<double> &, const MeshUpdateInputs &, const std::vector<int64_t> &, const int32_t *, const double *, int,
                                                    bool, ProtoUpdateStage<double> &);

// ---- take_hip_scene_track_vertices: the marked geometry of a side, before a mesh update replaces its records
template <class R> int copy_marked_geometry(const SceneT<R> &sc, DevBuf<R> &words, DevBuf<int32_t> &inst_first) {
    using namespace lbvh;
    const HostScene<R> &h = sc.host;
    const int64_t n = (int64_t)sc.prims.n, n_inst = (int64_t)sc.inst_trace.n;
    const int n_protos = n_inst > 0 ? (int)h.blas_prim_first.size() : 0;
    const int64_t n_shapes = n - (n_inst > 0 ? h.blas_prims : 0);
    hipStream_t stream = nullptr;
    if (n_inst > 0 && ((int)h.blas_prim_count.size() != n_protos || (int64_t)h.placements.inst_proto.size() != n_inst || n_shapes < 0))
        return fail(TAKE_E_INVALID, "unsupported: the scene does not know where its prototypes are");
    const char *nomem = "out of device memory for the marked frame's geometry";
    if (words.alloc((size_t)n * MARKED_STRIDE) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
    if (n_shapes > 0) hipLaunchKernelGGL(k_copy_marked<R>, blocks_for(n_shapes), dim3(BLK), 0, stream, sc.prims.p, (int)n_shapes, words.p);
    std::vector<int32_t> first((size_t)n_inst);
    for (int k = 0; k < n_protos; k++) {
        const int64_t at = h.blas_prim_first[k], nf = h.blas_prim_count[k];
        if (at < n_shapes || nf < 0 || at + nf > n) return fail(TAKE_E_INVALID, "unsupported: the scene does not know where its prototypes are");
        if (nf > 0) hipLaunchKernelGGL(k_copy_marked<R>, blocks_for(nf), dim3(BLK), 0, stream, sc.prims.p + at, (int)nf, words.p + MARKED_STRIDE * at);
    }
    for (int64_t i = 0; i < n_inst; i++) {
        const int32_t k = h.placements.inst_proto[(size_t)i];
        if (k < 0 || k >= n_protos) return fail(TAKE_E_INVALID, "unsupported: the scene does not know where its prototypes are");
        first[(size_t)i] = (int32_t)h.blas_prim_first[k];
    }
    if (n_inst > 0) {
        if (inst_first.alloc((size_t)n_inst) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
        HIP_TRY(hipMemcpy(inst_first.p, first.data(), inst_first.bytes(), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());
    return TAKE_OK;
}
template int copy_marked_geometry<float>(const SceneT<float> &, DevBuf<float> &, DevBuf<int32_t> &);
template int copy_marked_geometry<double>(const SceneT<double> &, DevBuf<double> &, DevBuf<int32_t> &);

}  // namespace tk_host

// tk_api.hip — implementation of the C ABI of include/take_hip.h: scene creation (host preparation, upload, the
// device build), scene groups, and the C entry points.  Tracing and rendering — everything that launches a kernel of
// tk_kernels.h — is tk_render.hip, reached through the functions of tk_scene_handle.h.  There is no CPU rendering
// path in this library: without a HIP device every entry point returns TAKE_E_NO_GPU.  The mesh entry points (PLY,
// serialized, OBJ, compute_normals) are tk_mesh.hip; the plumbing all units share is tk_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"
#include "tk_build_gpu.h"

using namespace tk;
using namespace tk_host;

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
// k_collapse.  The scene's only tree, the top-level tree of a two-level scene, or a prototype's.
struct DeviceTree {
    DevBuf<Node4<float>> nodes;  // breadth-first; child words local to the tree: node indices from 0, a leaf = a range of `order`
    DevBuf<uint32_t> order;      // Morton order -> entry of the span (a stable sort: coincident entries keep their order)
    int64_t n_nodes = 0;
    int depth = 0;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // bounds of the span's boxes: the tree's quantisation grid is laid over them
};
const int ORD_INIT[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};  // empty bounds (k_prim_boxes)
dim3 blocks_for(int64_t items) { return dim3((unsigned)((items + lbvh::BLK - 1) / lbvh::BLK)); }

// In: the n boxes of a span (pb: freed here, once the leaves exist) and their bounds (scene_ord: ordered ints, as
// k_prim_boxes leaves them).  Out: t.  Returns TAKE_OK, an error, or 1 = "use the host builder": fewer than two leaves,
// or a tree deeper than the traversal stack allows (long runs of equal Morton codes).
// The tree is made of float nodes whatever the scene's precision is (tk_build_gpu.h: only records and primitive boxes
// know it).
int build_tree_device(DevBuf<lbvh::Box> &pb, const DevBuf<int> &scene_ord, int n, int leaf_size, BuildMemory &mem, DeviceTree &t) {
    using namespace lbvh;
    const int n_leaves = (n + leaf_size - 1) / leaf_size;
    if (n_leaves < 2) return 1;
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    // (a release waits for the kernels launched before it: hipFree synchronises the device)
    DevBuf<Box> lbox, ibox;
    DevBuf<uint64_t> keys, keys_s, lkey;
    DevBuf<uint32_t> vals;
    DevBuf<int> parent_i, parent_l, flag, frontier[2], lvl;
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

    // collapse to 4-wide nodes, breadth-first, one launch per level (at most one node per leaf; the count is known after)
    HIP_TRY(t.nodes.alloc(n_leaves));
    HIP_TRY(frontier[0].alloc(n_leaves));
    HIP_TRY(frontier[1].alloc(n_leaves));
    HIP_TRY(lvl.alloc(MAX_LEVELS + 2));
    mem.sample("collapse");
    HIP_TRY(hipMemsetAsync(lvl.p, 0, lvl.bytes(), stream));
    hipLaunchKernelGGL(k_fill_int, dim3(1), blk, 0, stream, lvl.p, 1, 1);           // one node on level 0 ...
    hipLaunchKernelGGL(k_fill_int, dim3(1), blk, 0, stream, frontier[0].p, 1, 0);   // ... made from BVH2 node 0
    const int cgrid = std::max(1, std::min((n_leaves + BLK - 1) / BLK, 2048));
    for (int level = 0; level < MAX_LEVELS; level++)
        hipLaunchKernelGGL(k_collapse, dim3(cgrid), blk, 0, stream, level, frontier[level & 1].p, frontier[(level + 1) & 1].p,
                           lvl.p, child.p, ibox.p, lbox.p, leaf_size, n, t.nodes.p);
    int lvl_h[MAX_LEVELS + 2];
    int ord_h[6];
    HIP_TRY(hipMemcpyAsync(lvl_h, lvl.p, sizeof(lvl_h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(ord_h, scene_ord.p, sizeof(ord_h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (lvl_h[MAX_LEVELS] != 0) return 1;  // deeper than the traversal stack allows
    t.n_nodes = 0, t.depth = 0;
    for (int k = 0; k < MAX_LEVELS; k++)
        if (lvl_h[k] > 0) t.n_nodes += lvl_h[k], t.depth = k + 1;
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

// BVH build on the device of a scene without placements.  In: sc.prims uploaded in SHAPE order.  Out: the records in
// leaf order, sc.nodes or sc.qnodes, host-side stats and grid.  Returns TAKE_OK, an error, or 1 = "use the host
// builder" (build_tree_device).  A double scene that is refused compression gets its float nodes widened.
template <class R> int build_bvh_device(SceneT<R> &sc, int max_leaf, bool compressed_ok, bool compressed_forced) {
    using namespace lbvh;
    HostScene<R> &h = sc.host;
    const int n = (int)sc.prims.n;
    const int leaf_size = device_leaf_size(max_leaf);
    if ((n + leaf_size - 1) / leaf_size < 2) return 1;
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    BuildMemory mem(sizeof(R) == 4 ? "f32" : "f64");
    DevBuf<Box> pb;
    DevBuf<int> scene_ord;
    DevBuf<double> acc;
    DeviceTree t;
    HIP_TRY(pb.alloc(n));
    HIP_TRY(scene_ord.alloc(6));
    HIP_TRY(hipMemcpy(scene_ord.p, ORD_INIT, sizeof(ORD_INIT), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_prim_boxes<R>, blocks_for(n), blk, 0, stream, sc.prims.p, n, pb.p, scene_ord.p);
    const int rt = build_tree_device(pb, scene_ord, n, leaf_size, mem, t);
    if (rt) return rt;
    h.stats = WideBvhStats{};
    h.stats.n_nodes = t.n_nodes, h.stats.n_prims = n, h.stats.depth = t.depth;
    h.root_child = 0;

    // compressed nodes on the scene grid (same fall-back rule as the host path)
    h.q_inflation = 1.0;
    bool use_q = false;
    if (compressed_ok) {
        QGrid g;
        HIP_TRY(sc.qnodes.alloc((size_t)t.n_nodes));
        HIP_TRY(acc.alloc(2));
        mem.sample("compression");
        const int rq = quantise_tree_device(t, sc.qnodes.p, acc, g, h.q_inflation);
        if (rq) return rq;
        use_q = compressed_forced || h.q_inflation <= 1.10;
        for (int a = 0; a < 3; a++) h.grid_lo[a] = g.lo[a], h.grid_step[a] = g.step[a];
        if (!use_q) sc.qnodes.release();
    }
    if (!use_q) {  // full-width nodes
        if constexpr (sizeof(R) == 4) {
            sc.nodes = std::move(t.nodes);
        } else {
            HIP_TRY(sc.nodes.alloc((size_t)t.n_nodes));
            mem.sample("wide nodes");
            const int rw = wide_nodes_device(t, sc.nodes.p);
            if (rw) return rw;
        }
    }
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
// TAKE_INSTANCES_FLATTEN: the description with every placement expanded to a world-space mesh of its own — the geometry
// an instanced render is specified to equal (TakeInstance, include/take_hip.h).  Placement i becomes mesh n_meshes + i:
// positions M[:, :3] p + M[:, 3] and normals n^T L^-1 (not re-normalised: interpolation commutes with the linear map
// only then; the interpolated normal is normalised at the hit) in double, on `threads` host threads; the prototype's
// index and uv arrays are shared, not copied.  The shape arrays grow by the placements' faces in placement order, so
// shape ids are the two-level scene's (n_shapes + faces of the preceding placements + face).
struct FlattenedInstances {
    std::vector<TakeMesh> meshes;
    std::vector<std::vector<double>> arrays;
    std::vector<int32_t> kind, ref, face, area_light;
    int expand(TakeSceneDesc &d, int threads) {
        if (d.n_instances <= 0) return TAKE_OK;
        if (!d.instances) return fail(TAKE_E_INVALID, "n_instances > 0 but instances is null");
        int64_t extra = 0;
        for (int64_t i = 0; i < d.n_instances; i++) {
            const TakeInstance &in = d.instances[i];
            if (in.mesh_id < 0 || in.mesh_id >= d.n_meshes) return fail(TAKE_E_INVALID, "instance " + std::to_string(i) + ": bad mesh index");
            const TakeMesh &m = d.meshes[in.mesh_id];
            if (m.flags & TAKE_MESH_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, "instance " + std::to_string(i) + ": flattening reads the prototype on the host; it is a device-array mesh");
            if (m.n_vertices < 0 || m.n_faces < 0 || (m.n_faces > 0 && (!m.positions || !m.indices))) return fail(TAKE_E_INVALID, "instance " + std::to_string(i) + ": bad prototype mesh");
            if (in.material_id >= d.n_materials) return fail(TAKE_E_INVALID, "instance " + std::to_string(i) + ": bad material index");
            extra += m.n_faces;
        }
        if (d.n_shapes + extra >= ((int64_t)1 << 31) || (int64_t)d.n_meshes + d.n_instances >= ((int64_t)1 << 31))
            return fail(TAKE_E_INVALID, "flattened scene too large (" + std::to_string(d.n_shapes + extra) + " shapes)");
        meshes.assign(d.meshes, d.meshes + d.n_meshes);
        meshes.resize((size_t)d.n_meshes + (size_t)d.n_instances);
        arrays.resize(2 * (size_t)d.n_instances);
        std::string err;
        std::mutex mu;
        auto work = [&](int64_t lo, int64_t hi) {
            try {
            for (int64_t i = lo; i < hi; i++) {
                const TakeInstance &in = d.instances[i];
                const TakeMesh &m = d.meshes[in.mesh_id];
                const Affine3 x{in.xform};
                std::vector<double> &pos = arrays[2 * (size_t)i], &nrm = arrays[2 * (size_t)i + 1];
                pos.resize(3 * (size_t)m.n_vertices);
                for (int64_t v = 0; v < m.n_vertices; v++) {
                    const double px = m.positions[3 * v], py = m.positions[3 * v + 1], pz = m.positions[3 * v + 2];
                    for (int a = 0; a < 3; a++) pos[3 * v + a] = x.image(a, px, py, pz);
                }
                if (m.normals) {
                    double inv[9];
                    if (!x.inverse_linear(inv)) {
                        std::lock_guard<std::mutex> lock(mu);
                        err = "instance " + std::to_string(i) + ": singular transform";
                        return;
                    }
                    nrm.resize(3 * (size_t)m.n_vertices);
                    for (int64_t v = 0; v < m.n_vertices; v++) {
                        const double nx = m.normals[3 * v], ny = m.normals[3 * v + 1], nz = m.normals[3 * v + 2];
                        nrm[3 * v + 0] = nx * inv[0] + ny * inv[3] + nz * inv[6];  // (n^T L^-1)
                        nrm[3 * v + 1] = nx * inv[1] + ny * inv[4] + nz * inv[7];
                        nrm[3 * v + 2] = nx * inv[2] + ny * inv[5] + nz * inv[8];
                    }
                }
                TakeMesh &o = meshes[(size_t)d.n_meshes + (size_t)i];
                o = m;
                o.positions = pos.data();
                o.normals = m.normals ? nrm.data() : nullptr;
                o.material_id = in.material_id >= 0 ? in.material_id : m.material_id;
            }
            } catch (const std::exception &) {  // (an exception must not leave a worker thread)
                std::lock_guard<std::mutex> lock(mu);
                err = "out of host memory while flattening the instances";
            }
        };
        const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads, d.n_instances));
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; t++) pool.emplace_back(work, d.n_instances * t / nt, d.n_instances * (t + 1) / nt);
        for (auto &th : pool) th.join();
        if (!err.empty()) return fail(TAKE_E_INVALID, err);
        const size_t n0 = (size_t)d.n_shapes, n1 = n0 + (size_t)extra;
        kind.resize(n1), ref.resize(n1), face.resize(n1), area_light.resize(n1);
        if (n0) {
            std::memcpy(kind.data(), d.shape_kind, n0 * 4), std::memcpy(ref.data(), d.shape_ref, n0 * 4);
            std::memcpy(face.data(), d.shape_face, n0 * 4), std::memcpy(area_light.data(), d.shape_area_light, n0 * 4);
        }
        size_t at = n0;
        for (int64_t i = 0; i < d.n_instances; i++) {
            const int64_t nf = d.meshes[d.instances[i].mesh_id].n_faces;
            for (int64_t k = 0; k < nf; k++, at++) kind[at] = 1, ref[at] = (int32_t)(d.n_meshes + i), face[at] = (int32_t)k, area_light[at] = -1;
        }
        d.meshes = meshes.data(), d.n_meshes = (int32_t)meshes.size();
        d.shape_kind = kind.data(), d.shape_ref = ref.data(), d.shape_face = face.data(), d.shape_area_light = area_light.data();
        d.n_shapes = (int64_t)n1;
        d.n_instances = 0, d.instances = nullptr;
        return TAKE_OK;
    }
};

// Device-array meshes (TAKE_MESH_DEVICE_ARRAYS, take_hip_mesh_from_ply) in a scene description: the host side of the
// build — index validation, the face / normal / uv tables, the SAH builder — reads host copies, staged here.
struct StagedMeshes {
    bool any = false;
    std::vector<TakeMesh> meshes;            // what the build sees (d.meshes points here)
    std::vector<const double *> d_positions;  // per mesh: its device positions while they have not been staged
    std::vector<std::vector<double>> reals;
    std::vector<std::vector<int32_t>> ints;
    hipError_t real(const double *&p, size_t n) {
        if (!p || n == 0) return hipSuccess;
        reals.emplace_back(n);
        const hipError_t e = hipMemcpy(reals.back().data(), p, n * sizeof(double), hipMemcpyDeviceToHost);
        p = reals.back().data();
        return e;
    }
    // all_positions: the host builder will run (it reads every vertex).  Otherwise only the meshes an area light
    // sits on bring their positions to the host (the light records are made there); the device build copies the
    // others device-to-device.
    int stage(TakeSceneDesc &d, bool all_positions) {
        for (int i = 0; i < d.n_meshes; i++) any = any || (d.meshes && (d.meshes[i].flags & TAKE_MESH_DEVICE_ARRAYS));
        if (!any) return TAKE_OK;
        meshes.assign(d.meshes, d.meshes + d.n_meshes);
        d_positions.assign((size_t)d.n_meshes, nullptr);
        std::vector<char> emissive((size_t)d.n_meshes, 0);
        for (int i = 0; i < d.n_lights; i++) {
            const TakeLight &l = d.lights[i];
            if (l.kind != 1 || l.shape_id < 0 || l.shape_id >= d.n_shapes || d.shape_kind[l.shape_id] != 1) continue;
            const int32_t mi = d.shape_ref[l.shape_id];
            if (mi >= 0 && mi < d.n_meshes) emissive[mi] = 1;
        }
        for (int i = 0; i < d.n_meshes; i++) {
            TakeMesh &m = meshes[i];
            if (!(m.flags & TAKE_MESH_DEVICE_ARRAYS)) continue;
            if (m.n_vertices < 0 || m.n_faces < 0) return fail(TAKE_E_INVALID, "negative mesh size");
            if (all_positions || emissive[i]) HIP_TRY(real(m.positions, 3 * (size_t)m.n_vertices));
            else d_positions[i] = m.positions;
            HIP_TRY(real(m.normals, 3 * (size_t)m.n_vertices));
            HIP_TRY(real(m.uvs, 2 * (size_t)m.n_vertices));
            if (m.indices && m.n_faces > 0) {
                ints.emplace_back(3 * (size_t)m.n_faces);
                HIP_TRY(hipMemcpy(ints.back().data(), m.indices, ints.back().size() * sizeof(int32_t), hipMemcpyDeviceToHost));
                m.indices = ints.back().data();
            }
            m.flags &= ~TAKE_MESH_DEVICE_ARRAYS;
        }
        d.meshes = meshes.data();
        return TAKE_OK;
    }
    // the device build gave up (a tree too deep or of one leaf): the host builder needs every vertex after all
    int ensure_positions() {
        for (size_t i = 0; i < meshes.size(); i++) {
            if (!d_positions[i]) continue;
            HIP_TRY(real(meshes[i].positions, 3 * (size_t)meshes[i].n_vertices));
            d_positions[i] = nullptr;
        }
        return TAKE_OK;
    }
};

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
    int upload(const TakeSceneDesc &d, const double *const *device_positions) {
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
    void release() { pos.release(), kind.release(), ref.release(), face.release(), area_light.release(); }
};

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

// BVH build on the device of a two-level scene (TakeInstance placements, TAKE_INSTANCES_TWO_LEVEL): the scene
// build_host_trees makes, with LBVH trees.  In: sc.prims = the shapes' records in shape order (possibly none),
// sc.face_idx, sc.host as prepare_scene(PREP_DEVICE_BUILD) leaves it (the placements' records and the PlacementPlan),
// `in` still holding the positions.  Out: sc.prims = the top-level tree's records in leaf order, then each prototype's;
// sc.qnodes or sc.nodes = the top-level tree's nodes, then each prototype's, child words global; the placements'
// root_child and grid; stats.  Returns TAKE_OK, an error, or 1 = "use the host builder" — for the whole scene: a tree
// of fewer than two leaves (a one-face prototype) or too deep a stack over both levels.
//   1. per distinct prototype, one pass: k_make_proto_prims -> k_prim_boxes -> build_tree_device; its records go
//      straight to their place behind the shapes' records, its float nodes wait (cut to size) for step 4;
//   2. k_placement_boxes / k_placement_pad: the placements' boxes behind the shapes' boxes (host formula beyond 4e8
//      vertex transforms, placement_box);
//   3. the top-level tree over both, ONE entry per leaf whatever max_leaf is (a placement is a leaf of its own, and
//      the compacted record ranges of k_top_leaves are single records); k_top_leaves, k_permute_top;
//   4. every tree quantised on its own grid into the scene's node array — the worst inflation over all trees decides
//      for the whole scene between compressed and full-width nodes, as quantise_trees does — and k_rebase.
template <class R>
int build_two_level_device(SceneT<R> &sc, const TakeSceneDesc &d, const DeviceBuildInputs &in, int max_leaf, bool compressed_ok, bool compressed_forced) {
    using namespace lbvh;
    HostScene<R> &h = sc.host;
    const PlacementPlan &plan = h.placements;
    const int n_shapes = (int)d.n_shapes, n_inst = (int)d.n_instances, n_top = n_shapes + n_inst;
    const int n_protos = (int)plan.proto_mesh.size();
    const int leaf_size = device_leaf_size(max_leaf);
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    BuildMemory mem(sizeof(R) == 4 ? "f32" : "f64");
    if (n_top < 2) return 1;
    std::vector<int64_t> prim_base(n_protos + 1), node_base(n_protos + 1);
    prim_base[0] = n_shapes;
    for (int k = 0; k < n_protos; k++) {
        const int64_t nf = d.meshes[plan.proto_mesh[k]].n_faces;
        if ((nf + leaf_size - 1) / leaf_size < 2) return 1;
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
        DevBuf<Box> pb;
        HIP_TRY(recs.alloc(nf));
        HIP_TRY(pb.alloc(nf));
        HIP_TRY(hipMemcpyAsync(scene_ord.p, ORD_INIT, sizeof(ORD_INIT), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_make_proto_prims<R>, blocks_for(nf), blk, 0, stream, mesh_src(h, in, mesh), mesh, in.pos.p, sc.face_idx.p, nf, recs.p);
        hipLaunchKernelGGL(k_prim_boxes<R>, blocks_for(nf), blk, 0, stream, recs.p, nf, pb.p, scene_ord.p);
        DeviceTree &t = protos[k];
        const int rt = build_tree_device(pb, scene_ord, nf, leaf_size, mem, t);
        if (rt) return rt;
        hipLaunchKernelGGL((k_permute<PrimRec<R>>), blocks_for(nf), blk, 0, stream, recs.p, t.order.p, nf, prims.p + prim_base[k]);
        DevBuf<Node4<float>> cut;  // (the collapse allocates a node per leaf and uses about a third)
        HIP_TRY(cut.alloc((size_t)t.n_nodes));
        HIP_TRY(hipMemcpy(cut.p, t.nodes.p, cut.bytes(), hipMemcpyDeviceToDevice));
        t.nodes = std::move(cut);
        t.order.release();
        proto_depth = std::max(proto_depth, t.depth);
    }
    mem.sample("prototypes");

    // 2. the placements' boxes, behind the shapes'
    DevBuf<Box> pb;
    HIP_TRY(pb.alloc(n_top));
    HIP_TRY(hipMemcpy(scene_ord.p, ORD_INIT, sizeof(ORD_INIT), hipMemcpyHostToDevice));
    if (n_shapes > 0) hipLaunchKernelGGL(k_prim_boxes<R>, blocks_for(n_shapes), blk, 0, stream, sc.prims.p, n_shapes, pb.p, scene_ord.p);
    {
        std::vector<long long> tight_h(6 * (size_t)n_inst);
        std::vector<double> xf(12 * (size_t)n_inst);
        std::vector<std::vector<int32_t>> of_proto(n_protos);
        for (int i = 0; i < n_inst; i++) {
            for (int a = 0; a < 3; a++) tight_h[6 * (size_t)i + a] = INT64_MAX, tight_h[6 * (size_t)i + 3 + a] = INT64_MIN;
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
    const int rt = build_tree_device(pb, scene_ord, n_top, 1, mem, top);
    if (rt) return rt;
    const int depth = top.depth + proto_depth;
    if (3 * depth + 2 > MAX_STACK_ENTRIES) return 1;  // the traversal stack holds both levels and one return marker
    {
        DevBuf<int> is_shape, rank;
        DevBuf<char> temp;
        HIP_TRY(is_shape.alloc(n_top));
        HIP_TRY(rank.alloc(n_top));
        hipLaunchKernelGGL(k_flag_shapes, blocks_for(n_top), blk, 0, stream, top.order.p, n_top, n_shapes, is_shape.p);
        size_t temp_bytes = 0;
        HIP_TRY(rocprim::exclusive_scan(nullptr, temp_bytes, is_shape.p, rank.p, 0, (size_t)n_top, rocprim::plus<int>(), stream));
        HIP_TRY(temp.alloc(temp_bytes));
        HIP_TRY(rocprim::exclusive_scan(temp.p, temp_bytes, is_shape.p, rank.p, 0, (size_t)n_top, rocprim::plus<int>(), stream));
        hipLaunchKernelGGL(k_top_leaves, blocks_for(top.n_nodes), blk, 0, stream, top.nodes.p, (int)top.n_nodes, top.order.p, rank.p, n_shapes);
        hipLaunchKernelGGL((k_permute_top<PrimRec<R>>), blocks_for(n_top), blk, 0, stream, sc.prims.p, top.order.p, rank.p, n_top, n_shapes, prims.p);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipGetLastError());
    }
    top.order.release();
    sc.prims = std::move(prims);  // (frees the shape-order records)

    // 4. assembly: the top-level tree's nodes, then each prototype's
    node_base[0] = top.n_nodes;
    for (int k = 0; k < n_protos; k++) node_base[k + 1] = node_base[k] + protos[k].n_nodes;
    const int64_t n_nodes = node_base[n_protos];
    if (n_nodes >= ((int64_t)1 << 31)) return fail(TAKE_E_INVALID, "too many nodes");
    h.stats = WideBvhStats{};
    h.stats.n_nodes = n_nodes, h.stats.n_prims = n_shapes, h.stats.depth = depth;
    h.root_child = 0;
    h.n_blas = n_protos, h.blas_nodes = n_nodes - top.n_nodes, h.blas_prims = prim_base[n_protos] - n_shapes;
    h.q_inflation = 1.0;
    bool use_q = false;
    std::vector<QGrid> grids(n_protos);
    if (compressed_ok) {
        DevBuf<double> acc;
        HIP_TRY(sc.qnodes.alloc((size_t)n_nodes));
        HIP_TRY(acc.alloc(2));
        mem.sample("compression");
        QGrid g;
        int rq = quantise_tree_device(top, sc.qnodes.p, acc, g, h.q_inflation);
        for (int a = 0; a < 3; a++) h.grid_lo[a] = g.lo[a], h.grid_step[a] = g.step[a];
        for (int k = 0; k < n_protos && !rq; k++) {
            double infl = 1.0;
            rq = quantise_tree_device(protos[k], sc.qnodes.p + node_base[k], acc, grids[k], infl);
            h.q_inflation = std::max(h.q_inflation, infl);
        }
        if (rq) return rq;
        use_q = compressed_forced || h.q_inflation <= 1.10;
        if (!use_q) sc.qnodes.release();
    }
    if (!use_q) {
        HIP_TRY(sc.nodes.alloc((size_t)n_nodes));
        mem.sample("wide nodes");
        int rw = wide_nodes_device(top, sc.nodes.p);
        for (int k = 0; k < n_protos && !rw; k++) rw = wide_nodes_device(protos[k], sc.nodes.p + node_base[k]);
        if (rw) return rw;
    }
    for (int k = 0; k < n_protos; k++) {
        const int nk = (int)protos[k].n_nodes;
        if (use_q) hipLaunchKernelGGL(k_rebase<QNode4>, blocks_for(nk), blk, 0, stream, sc.qnodes.p + node_base[k], nk, (int32_t)node_base[k], (int32_t)prim_base[k]);
        else hipLaunchKernelGGL(k_rebase<Node4<R>>, blocks_for(nk), blk, 0, stream, sc.nodes.p + node_base[k], nk, (int32_t)node_base[k], (int32_t)prim_base[k]);
    }
    // (a prototype's root is node 0 of its tree: it has at least two leaves)
    for (int i = 0; i < n_inst; i++) {
        const int k = plan.inst_proto[i];
        InstTrace<R> &it = h.inst_trace[i];
        it.root_child = (int32_t)node_base[k];
        if (compressed_ok)
            for (int a = 0; a < 3; a++) it.grid_lo[a] = grids[k].lo[a], it.grid_step[a] = grids[k].step[a];
    }
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());
    mem.report();
    return TAKE_OK;
}

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

// One precision's side of a new scene: records, tree and shading tables prepared on the host and uploaded, or with
// device_builder the records and the tree made on the device — and, when the device tree would be too deep, on the
// host after all.  staged: the description's device-array meshes (StagedMeshes::stage).  inputs: what the device
// builder reads of the caller's arrays, shared by the sides of the scene; last_side: nothing needs them after this one.
template <class R>
int upload_scene(SceneT<R> &sc, int num_cus, const TakeSceneDesc &desc, const TakeBuildOpts &opts, int threads, bool device_builder,
                 StagedMeshes &staged, DeviceBuildInputs &inputs, bool last_side) {
    PhaseClock clock(sizeof(R) == 4 ? "f32" : "f64");
    int max_leaf = opts.max_leaf_size;
    if (max_leaf <= 0 && std::getenv("TAKE_HIP_MAX_LEAF")) max_leaf = std::atoi(std::getenv("TAKE_HIP_MAX_LEAF"));  // tuning knob
    const char *fmt_env = std::getenv("TAKE_HIP_NODES");
    const std::string fmt = fmt_env ? fmt_env : "";
    bool on_device = device_builder;
    std::string err = prepare_scene<R>(desc, max_leaf, threads, sc.host, on_device ? PREP_DEVICE_BUILD : PREP_HOST_BUILD, opts.burley_lobes != 0);
    if (!err.empty()) return fail(TAKE_E_INVALID, err);
    clock.lap(on_device ? "host validation + tables" : "host records + SAH build");
    HostScene<R> &h = sc.host;
    if (on_device) {
        const bool two_level = desc.n_instances > 0;
        const bool compressed_ok = compressed_nodes_supported() && fmt != "wide";
        int rc = make_prims_on_device(sc, desc, inputs, staged.any ? staged.d_positions.data() : nullptr);
        // (positions and shape arrays: not part of the build's peak — but a two-level build reads the prototypes' positions)
        if (last_side && !two_level) inputs.release();
        clock.lap("mesh arrays -> HBM, records");
        if (!rc) rc = two_level ? build_two_level_device(sc, desc, inputs, max_leaf, compressed_ok, fmt == "q16")
                                : build_bvh_device(sc, max_leaf, compressed_ok, fmt == "q16");
        if (last_side) inputs.release();
        if (rc == 1) {  // not buildable on the device (a tree too deep or of one leaf): do it on the host after all
            on_device = false;
            sc.prims.release(), sc.qnodes.release(), sc.nodes.release();
            const int rs = staged.ensure_positions();
            if (rs) return rs;
            err = prepare_scene<R>(desc, max_leaf, threads, sc.host, PREP_HOST_BUILD, opts.burley_lobes != 0);
            if (!err.empty()) return fail(TAKE_E_INVALID, err);
        } else if (rc != TAKE_OK) {
            return rc;
        }
    }
    if (!on_device) {
        HIP_TRY(sc.prims.upload(h.prims));
        clock.lap("primitive records -> HBM");
        const bool use_q = compressed_nodes_supported() && (!h.qnodes.empty() || !h.qnodes8.empty());
        if (!h.qnodes8.empty()) HIP_TRY(sc.qnodes8.upload(h.qnodes8));
        else if (use_q) HIP_TRY(sc.qnodes.upload(h.qnodes));
        else HIP_TRY(sc.nodes.upload(h.nodes));
    }
    sc.built_on_device = on_device;
    clock.lap(on_device ? "device LBVH build" : "nodes -> HBM");
    // (only the node format the kernels traverse is allocated)
    sc.trace = TraceKind{sc.qnodes8.p ? NodeFormat::Q8 : (sc.qnodes.p ? NodeFormat::Q4 : NodeFormat::WIDE), !h.inst_trace.empty()};
    // the trace kernels address nodes and primitive records with 32-bit byte offsets (full-rate integer math)
    {
        const uint64_t tree_bytes = (uint64_t)h.stats.n_nodes * node_bytes<R>(sc.trace.nodes);
        const uint64_t prim_bytes = (uint64_t)sc.prims.n * sizeof(PrimRec<R>);
        if (tree_bytes >= (1ull << 32) || prim_bytes >= (1ull << 32))
            return fail(TAKE_E_INVALID, "scene too large for the 32-bit record offsets of the trace kernels (" +
                                            std::to_string(sc.prims.n) + " primitives, " + std::to_string(h.stats.n_nodes) + " nodes)");
    }
    HIP_TRY(sc.meshes.upload(h.meshes));
    // (device build: already there, k_make_prims read it — also after a fall-back to the host builder)
    if (!sc.face_idx.p) HIP_TRY(sc.face_idx.upload(h.face_idx));
    HIP_TRY(sc.normals.upload(h.normals));
    HIP_TRY(sc.uvs.upload(h.uvs));
    HIP_TRY(sc.texels.upload(h.texels));
    HIP_TRY(sc.materials.upload(h.materials));
    HIP_TRY(sc.images.upload(h.images));
    HIP_TRY(sc.lights.upload(h.lights));
    HIP_TRY(sc.light_pmf.upload(h.light_pmf));
    HIP_TRY(sc.light_cdf.upload(h.light_cdf));
    HIP_TRY(sc.inst_trace.upload(h.inst_trace));
    HIP_TRY(sc.inst_shade.upload(h.inst_shade));
    HIP_TRY(sc.env_marginal.upload(h.env_marginal));
    HIP_TRY(sc.env_conditional.upload(h.env_conditional));
    HIP_TRY(sc.env_guide_m.upload(h.env_guide_m));
    HIP_TRY(sc.env_guide_c.upload(h.env_guide_c));
    sc.dev = h.view();  // (the counts, camera and small tables; the pointers are the device arrays')
    sc.bind();
    HIP_TRY(alloc_trace_state(sc, num_cus));  // queue words, counters, the persistent trace grid
    clock.lap("shading tables -> HBM, grid");
    // everything the kernels read is in HBM now; the host keeps the small tables (camera, material tags, tree
    // statistics) and drops the copies of the large arrays (1.1 GB at 10M triangles)
    h.nodes = {}, h.qnodes = {}, h.qnodes8 = {}, h.nodes8 = {}, h.prims = {}, h.shapes = {}, h.face_idx = {}, h.normals = {}, h.uvs = {}, h.texels = {};
    h.inst_trace = {}, h.inst_shade = {};
    return TAKE_OK;
}

}  // namespace

extern "C" {

const char *take_hip_last_error(void) { return g_error.c_str(); }
int take_hip_abi_version(void) { return TAKE_HIP_ABI_VERSION; }
int take_hip_device_count(void) { return check_device(); }

int take_hip_scene_create(const TakeSceneDesc *desc, const TakeBuildOpts *opts, TakeScene **out) {
    if (!desc || !out) return fail(TAKE_E_INVALID, "null argument");
    *out = nullptr;
    int nd = check_device();
    if (nd < 0) return nd;
    TakeBuildOpts o{};
    if (opts) o = *opts;
    if (o.precision != TAKE_PRECISION_F32 && o.precision != TAKE_PRECISION_F64 && o.precision != TAKE_PRECISION_MIXED)
        return fail(TAKE_E_INVALID, "unknown precision");
    if (o.builder < TAKE_BUILDER_AUTO || o.builder > TAKE_BUILDER_HOST_SAH) return fail(TAKE_E_INVALID, "unknown builder");
    if (o.instances != TAKE_INSTANCES_TWO_LEVEL && o.instances != TAKE_INSTANCES_FLATTEN) return fail(TAKE_E_INVALID, "unknown instance mode");
    // (a scene that fails is freed on return, with its device current: nothing here changes the current device)
    std::unique_ptr<TakeScene> ts(new (std::nothrow) TakeScene());
    if (!ts) return fail(TAKE_E_NOMEM, "out of host memory");
    ts->precision = o.precision;
    hipDeviceProp_t prop;
    if (hipGetDevice(&ts->device) != hipSuccess || hipGetDeviceProperties(&prop, ts->device) != hipSuccess)
        return fail(TAKE_E_DEVICE, "cannot query the HIP device");
    ts->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const int threads = std::max(1, o.bvh_threads > 0 ? o.bvh_threads : (int)std::thread::hardware_concurrency());
    int rc;
    try {
        // device-array meshes (take_hip_mesh_from_ply): the host side of the build — index validation, the face / normal /
        // uv tables, the SAH builder below TAKE_AUTO_DEVICE_BUILD_SHAPES shapes — reads host copies; the device build
        // takes the positions where they are
        StagedMeshes staged;
        FlattenedInstances flat;
        TakeSceneDesc local = *desc;
        if (o.instances == TAKE_INSTANCES_FLATTEN) {
            const int rf = flat.expand(local, threads);
            if (rf) return rf;
        }
        // builder of every side's tree: AUTO = host SAH (best trees) up to 4M primitives, device LBVH beyond: at 10M triangles
        // the host build is 6 s of setup per side against 0.2 s, for 2-6 % of traversal speed.  The device
        // builder needs enough primitives to make a tree.  A two-level scene counts its shapes, the faces of its distinct
        // prototypes and its placements; TAKE_HIP_BRAID > 1 and TAKE_HIP_NODES=q8 are the host builder's experiments
        // there (braid entries are subtrees of a host tree).  No minimum size per prototype: at a thousand prototypes of
        // 1k triangles, one build pass each, the device is still 1.5x faster than the host.
        int64_t n_build = local.n_shapes;
        bool device_can = true;
        if (local.n_instances > 0 && local.instances) {
            std::vector<char> seen((size_t)std::max(local.n_meshes, 0), 0);
            for (int64_t i = 0; i < local.n_instances; i++) {
                const int32_t mi = local.instances[i].mesh_id;
                if (mi < 0 || mi >= local.n_meshes || !local.meshes || seen[mi]) continue;  // (a bad index is prepare_scene's to report)
                seen[mi] = 1;
                n_build += std::max<int64_t>(local.meshes[mi].n_faces, 0);
            }
            n_build += local.n_instances;
            const char *braid = std::getenv("TAKE_HIP_BRAID"), *nodes = std::getenv("TAKE_HIP_NODES");
            device_can = !(braid && std::atoi(braid) > 1) && !(nodes && std::string(nodes) == "q8");
        }
        const bool device_builder = n_build >= 8 && device_can &&
                                    (o.builder == TAKE_BUILDER_DEVICE_LBVH || (o.builder == TAKE_BUILDER_AUTO && n_build >= TAKE_AUTO_DEVICE_BUILD_SHAPES));
        // every position comes to the host unless the device builder makes the trees
        rc = staged.stage(local, !device_builder);
        // the f64 side of F64 and MIXED scenes, the f32 side of F32 and MIXED ones; a mixed scene's two sides are two
        // independent trees (each from its own records' boxes) over one upload of the caller's arrays
        DeviceBuildInputs inputs;
        if (!rc && o.precision != TAKE_PRECISION_F32)
            rc = upload_scene(ts->d, ts->num_cus, local, o, threads, device_builder, staged, inputs, o.precision == TAKE_PRECISION_F64);
        if (!rc && o.precision != TAKE_PRECISION_F64) rc = upload_scene(ts->f, ts->num_cus, local, o, threads, device_builder, staged, inputs, true);
    } catch (const std::bad_alloc &) {
        rc = fail(TAKE_E_NOMEM, "out of host memory while preparing the scene");
    } catch (const std::exception &e) {
        rc = fail(TAKE_E_INVALID, e.what());
    }
    if (rc) return rc;
    *out = ts.release();
    return TAKE_OK;
}

int take_hip_scene_destroy(TakeScene *ts) {
    if (!ts) return TAKE_OK;
    DeviceGuard guard_(ts->device);
    delete ts;
    return TAKE_OK;
}

int take_hip_render_rows(const TakeScene *ts, int32_t strip_first, int32_t strip_stride, int32_t *rows_out) {
    if (!ts) return fail(TAKE_E_INVALID, "null scene");
    if (strip_stride <= 0 || strip_first < 0 || strip_first >= strip_stride)
        return fail(TAKE_E_INVALID, "strip_first must be in [0, strip_stride)");
    return rows_of(ts->height(), strip_first, strip_stride, rows_out);
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
    // (a workspace grown for a bigger batch keeps the accumulator: ensure_workspace only ever enlarges it, and the
    // strip set — hence the pixel count — is fixed for the sequence)
    const int rc = render_scene(ts, *opts, d_rgb_out, (hipStream_t)stream, first, !fresh);
    if (rc) {
        ts->acc_samples = 0;  // the accumulator may hold a partial batch: the sequence has to restart
        return rc;
    }
    ts->acc_samples = first + opts->spp;
    ts->acc_opts = *opts;
    return TAKE_OK;
}
int64_t take_hip_accumulated_samples(const TakeScene *ts) { return ts ? ts->acc_samples : 0; }

int take_hip_render(TakeScene *ts, const TakeRenderOpts *opts, void *rgb_out_host) {
    if (!ts || !opts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    const int W = ts->width();
    const int stride = opts->strip_stride > 0 ? opts->strip_stride : 1;
    if (opts->strip_first < 0 || opts->strip_first >= stride)
        return fail(TAKE_E_INVALID, "strip_first must be in [0, strip_stride)");
    const int rows = take_hip_render_rows(ts, opts->strip_first, stride, nullptr);
    if (rows < 0) return rows;
    const size_t bytes = (size_t)rows * W * 3 * (ts->f64() ? 8 : 4);
    if (bytes == 0) return TAKE_OK;
    // render into the scene's own output buffer, then copy out
    const void *img = nullptr;
    const int rc = render_scene_to_out(ts, *opts, (int64_t)rows * W, img);
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


// ------------------------------------------------------------------------------------------------ scene groups
}  // extern "C"

namespace {
// A replica of `src` on `device`: every device array is copied peer to peer (xGMI between the GPUs of a node), the
// small host tables by value — the scene is prepared and its tree built ONCE per group, whichever builder made it.
template <class T> int peer_copy(DevBuf<T> &dst, int dst_dev, const DevBuf<T> &src, int src_dev) {
    if (dst.alloc(src.n) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for a scene replica");
    if (src.n && hipMemcpyPeer(dst.p, dst_dev, src.p, src_dev, src.bytes()) != hipSuccess)
        return fail(TAKE_E_DEVICE, "hipMemcpyPeer of a scene array failed");
    return TAKE_OK;
}
template <class R> int replicate_t(const SceneT<R> &a, int a_dev, SceneT<R> &b, int b_dev, int b_cus) {
    int rc = TAKE_OK;
    SceneT<R>::for_each_array([&](auto &dst, const auto &src) { if (!rc) rc = peer_copy(dst, b_dev, src, a_dev); }, b, a);
    if (rc) return rc;
    b.host = a.host;  // (the camera, counts and small tables: upload_scene dropped the large vectors)
    b.dev = a.dev;    // the plain values; then the pointers of this device
    b.bind();
    // the persistent trace grid of THIS device: blocks per CU are a property of the kernels (the same code object on
    // every device), the CU count is the replica device's own
    b.built_on_device = a.built_on_device, b.trace = a.trace, b.blocks_per_cu = a.blocks_per_cu;
    const hipError_t e = alloc_trace_state(b, b_cus);
    if (e == hipErrorOutOfMemory) return fail(TAKE_E_NOMEM, "out of device memory for a scene replica");
    HIP_TRY(e);
    return TAKE_OK;
}
// -> a new scene handle on `device` (made current for the call), equal to `src`
int replicate_scene(const TakeScene *src, int device, TakeScene **out) {
    *out = nullptr;
    DeviceGuard guard(device);  // (declared before the replica: a failed one is freed with its device current)
    std::unique_ptr<TakeScene> ts(new (std::nothrow) TakeScene());
    if (!ts) return fail(TAKE_E_NOMEM, "out of host memory");
    ts->precision = src->precision, ts->device = device, ts->num_cus = src->num_cus, ts->instrumentation = 0;
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the replica's device current");
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ts->num_cus = cus;
    (void)hipGetLastError();
    // the sides take_hip_scene_create made, in its order
    int rc = TAKE_OK;
    if (src->precision != TAKE_PRECISION_F32) rc = replicate_t(src->d, src->device, ts->d, device, ts->num_cus);
    if (!rc && src->precision != TAKE_PRECISION_F64) rc = replicate_t(src->f, src->device, ts->f, device, ts->num_cus);
    if (rc) return rc;
    *out = ts.release();
    return TAKE_OK;
}
}  // namespace

struct TakeSceneGroup {
    std::vector<TakeScene *> scenes;        // one per shard, each on its device
    std::vector<DevBuf<char>> staging;      // on the first device: shard k's compact rows (k > 0), copied peer to peer
    std::vector<DevBuf<int32_t>> d_rows;    // on the first device: image row of each compact row of shard k
    std::vector<int> n_rows;
    DevBuf<char> d_full;                    // on the first device: the assembled image (take_hip_group_render)
    int width = 0, height = 0;
    bool f64 = false;
    ~TakeSceneGroup() {
        // the group's buffers are freed here, in the guard's scope: freed as members, they would go after the guard
        // (they exist only once the first shard does)
        if (!scenes.empty()) {
            DeviceGuard guard(scenes[0]->device);
            staging.clear(), d_rows.clear(), d_full = DevBuf<char>();
        }
        for (TakeScene *ts : scenes) take_hip_scene_destroy(ts);
    }
};

namespace {
constexpr int BLOCK = 256;  // threads per block of k_place_rows
// compact rows of one shard -> their rows of the full image
template <class R>
__global__ void __launch_bounds__(BLOCK) k_place_rows(const R *__restrict__ src, const int32_t *__restrict__ rows, int n_rows,
                                                      int row_words, R *dst) {
    const int64_t total = (int64_t)n_rows * row_words;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * BLOCK) {
        const int r = (int)(i / row_words), c = (int)(i % row_words);
        dst[(int64_t)rows[r] * row_words + c] = src[i];
    }
}

int group_render(TakeSceneGroup *g, const TakeRenderOpts &opts, void *d_out) {
    const int n = (int)g->scenes.size();
    const size_t esz = g->f64 ? 8 : 4;
    const int row_words = g->width * 3;
    // every shard renders its strips on its own device, from its own host thread
    std::vector<int> rc(n, TAKE_OK);
    std::vector<std::string> err(n);
    std::vector<std::thread> pool;
    for (int k = 0; k < n; k++)
        pool.emplace_back([&, k] {
            TakeScene *ts = g->scenes[k];
            TakeRenderOpts o = opts;
            o.strip_first = k, o.strip_stride = n;
            if (g->n_rows[k] == 0) return;
            DeviceGuard guard(ts->device);
            if (!guard.ok) {
                rc[k] = TAKE_E_DEVICE, err[k] = "cannot make the shard's device current";
                return;
            }
            const void *rows = nullptr;
            int r = render_scene_to_out(ts, o, (int64_t)g->n_rows[k] * g->width, rows);
            if (!r && k > 0) {  // the one exchange: this shard's rows to the first device
                const hipError_t e = hipMemcpyPeer(g->staging[k].p, g->scenes[0]->device, rows, ts->device, (size_t)g->n_rows[k] * row_words * esz);
                if (e != hipSuccess) r = TAKE_E_DEVICE, g_error = std::string("hipMemcpyPeer: ") + hipGetErrorString(e);
            }
            rc[k] = r;
            if (r) err[k] = g_error;  // g_error is thread-local: hand the message to the caller's thread
        });
    for (auto &t : pool) t.join();
    for (int k = 0; k < n; k++)
        if (rc[k]) return fail(rc[k], "shard " + std::to_string(k) + ": " + err[k]);
    // assemble on the first device
    DeviceGuard guard(g->scenes[0]->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the first device current");
    on_primary(g->scenes[0], [&](auto &sc0) {
        using R = std::remove_pointer_t<decltype(sc0.out.p)>;
        for (int k = 0; k < n; k++) {
            if (g->n_rows[k] == 0) continue;
            const R *src = k == 0 ? sc0.out.p : (const R *)g->staging[k].p;
            const int64_t total = (int64_t)g->n_rows[k] * row_words;
            const dim3 grid((unsigned)std::min<int64_t>((total + BLOCK - 1) / BLOCK, 4096));
            hipLaunchKernelGGL((k_place_rows<R>), grid, dim3(BLOCK), 0, nullptr, src, g->d_rows[k].p, g->n_rows[k], row_words, (R *)d_out);
        }
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return TAKE_OK;
}
}  // namespace

extern "C" {

int take_hip_group_create(const TakeSceneDesc *desc, const TakeBuildOpts *opts, int32_t n_gpus, const int32_t *devices,
                          TakeSceneGroup **out) {
    if (!desc || !out) return fail(TAKE_E_INVALID, "null argument");
    *out = nullptr;
    const int nd = check_device();
    if (nd < 0) return nd;
    if (n_gpus <= 0 || n_gpus > 64) return fail(TAKE_E_INVALID, "n_gpus must be in 1..64");
    for (int k = 0; k < n_gpus; k++) {
        const int dev = devices ? devices[k] : k;
        if (dev < 0 || dev >= nd) return fail(TAKE_E_INVALID, "device " + std::to_string(dev) + " of shard " + std::to_string(k) + " is not visible (" + std::to_string(nd) + " devices)");
    }
    std::unique_ptr<TakeSceneGroup> g(new (std::nothrow) TakeSceneGroup());
    if (!g) return fail(TAKE_E_NOMEM, "out of host memory");
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = TAKE_OK;
    for (int k = 0; k < n_gpus && !rc; k++) {
        const int dev = devices ? devices[k] : k;
        if (hipSetDevice(dev) != hipSuccess) {
            rc = fail(TAKE_E_DEVICE, "hipSetDevice failed");
            break;
        }
        TakeScene *ts = nullptr;
        // the first shard prepares and builds the scene; the others are peer-to-peer copies of its device arrays
        rc = k == 0 ? take_hip_scene_create(desc, opts, &ts) : replicate_scene(g->scenes[0], dev, &ts);
        if (!rc) g->scenes.push_back(ts);
    }
    if (!rc) {
        for (TakeScene *x : g->scenes) {  // shards that share a device share its free memory
            int share = 0;
            for (TakeScene *y : g->scenes) share += y->device == x->device;
            x->mem_share = share;
        }
        TakeScene *t0 = g->scenes[0];
        g->f64 = t0->f64(), g->width = t0->width(), g->height = t0->height();
        const size_t esz = g->f64 ? 8 : 4;
        g->staging.resize(n_gpus), g->d_rows.resize(n_gpus), g->n_rows.assign(n_gpus, 0);
        if (hipSetDevice(t0->device) != hipSuccess) rc = fail(TAKE_E_DEVICE, "hipSetDevice failed");
        for (int k = 0; k < n_gpus && !rc; k++) {
            std::vector<int32_t> rows((size_t)g->height);
            const int nr = rows_of(g->height, k, n_gpus, rows.data());
            rows.resize(nr);
            g->n_rows[k] = nr;
            if (nr == 0) continue;
            if (g->d_rows[k].upload(rows) != hipSuccess || (k > 0 && g->staging[k].alloc((size_t)nr * g->width * 3 * esz) != hipSuccess))
                rc = fail(TAKE_E_NOMEM, "out of device memory for the strip staging buffers");
            if (!rc && k > 0 && g->scenes[k]->device != t0->device) {
                // direct peer access if the fabric offers it (hipMemcpyPeer works either way)
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, t0->device, g->scenes[k]->device) == hipSuccess && can)
                    (void)hipDeviceEnablePeerAccess(g->scenes[k]->device, 0);
                (void)hipGetLastError();
            }
        }
    }
    (void)hipSetDevice(prev);
    if (rc) return rc;
    *out = g.release();
    return TAKE_OK;
}

int take_hip_group_destroy(TakeSceneGroup *g) {
    delete g;
    return TAKE_OK;
}
int take_hip_group_size(const TakeSceneGroup *g) { return g ? (int)g->scenes.size() : fail(TAKE_E_INVALID, "null group"); }

int take_hip_group_render_device(TakeSceneGroup *g, const TakeRenderOpts *opts, void *d_rgb_out) {
    if (!g || !opts || !d_rgb_out) return fail(TAKE_E_INVALID, "null argument");
    return group_render(g, *opts, d_rgb_out);
}

int take_hip_group_render(TakeSceneGroup *g, const TakeRenderOpts *opts, void *rgb_out_host) {
    if (!g || !opts || !rgb_out_host) return fail(TAKE_E_INVALID, "null argument");
    const size_t bytes = (size_t)g->width * g->height * 3 * (g->f64 ? 8 : 4);
    DeviceGuard guard(g->scenes[0]->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the first device current");
    if (!g->d_full.p && g->d_full.alloc(bytes) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the assembled image");
    const int rc = group_render(g, *opts, g->d_full.p);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(rgb_out_host, g->d_full.p, bytes, hipMemcpyDeviceToHost));
    return TAKE_OK;
}

int take_hip_group_get_counters(const TakeSceneGroup *g, int32_t k, TakeCounters *out) {
    if (!g || !out || k < 0 || k >= (int)g->scenes.size()) return fail(TAKE_E_INVALID, "bad argument");
    *out = g->scenes[k]->counters;
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
    const WideBvhStats s = on_primary(ts, [](const auto &sc) { return sc.host.stats; });
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
    if (f32_builder) *f32_builder = ts->precision == TAKE_PRECISION_F64 ? -1 : (ts->f.built_on_device ? TAKE_BUILDER_DEVICE_LBVH : TAKE_BUILDER_HOST_SAH);
    if (f64_builder) *f64_builder = ts->precision == TAKE_PRECISION_F32 ? -1 : (ts->d.built_on_device ? TAKE_BUILDER_DEVICE_LBVH : TAKE_BUILDER_HOST_SAH);
    return TAKE_OK;
}

}  // extern "C"

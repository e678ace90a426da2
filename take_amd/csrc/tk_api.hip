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

// BVH build on the device (tk_build_gpu.h).  In: sc.prims uploaded in SHAPE order.  Out: the records in
// leaf order, sc.nodes or sc.qnodes, host-side stats and grid.  Returns TAKE_OK, an error, or 1 = "use the host
// builder" (tree deeper than the traversal stack allows: long runs of equal Morton codes).
// The tree is made of float nodes whatever R is (tk_build_gpu.h: only records and primitive boxes know the
// precision); a double scene that is refused compression gets them widened, n_nodes of them.
template <class R> int build_bvh_device(SceneT<R> &sc, int max_leaf, bool compressed_ok, bool compressed_forced) {
    using namespace lbvh;
    HostScene<R> &h = sc.host;
    const int n = (int)sc.prims.n;
    // default 1 primitive per leaf: two Morton neighbours need not be close, and a leaf box around both costs more
    // primitive tests than the extra node (1M soup, 16 spp: 1 / 2 / 4 per leaf = 55.2 / 38.3 / 30.0 Msamples/s)
    const int leaf_size = std::max(1, std::min(max_leaf > 0 ? max_leaf : 1, MAX_LEAF));
    const int n_leaves = (n + leaf_size - 1) / leaf_size;
    if (n_leaves < 2) return 1;
    hipStream_t stream = nullptr;
    const dim3 blk(BLK);
    auto grid = [](int64_t items) { return dim3((unsigned)((items + BLK - 1) / BLK)); };
    BuildMemory mem(sizeof(R) == 4 ? "f32" : "f64");

    // (a release waits for the kernels launched before it: hipFree synchronises the device)
    DevBuf<Box> pb, lbox, ibox;
    DevBuf<uint64_t> keys, keys_s, lkey;
    DevBuf<uint32_t> vals, vals_s;
    DevBuf<int> scene_ord, parent_i, parent_l, flag, frontier[2], lvl;
    DevBuf<int2> child;
    DevBuf<char> temp;
    DevBuf<double> acc;
    DevBuf<Node4<float>> fnodes;
    // boxes, Morton codes, sort
    HIP_TRY(pb.alloc(n));
    HIP_TRY(keys.alloc(n));
    HIP_TRY(vals.alloc(n));
    HIP_TRY(keys_s.alloc(n));
    HIP_TRY(vals_s.alloc(n));
    HIP_TRY(scene_ord.alloc(6));
    const int ord_init[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
    HIP_TRY(hipMemcpy(scene_ord.p, ord_init, sizeof(ord_init), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_prim_boxes<R>, grid(n), blk, 0, stream, sc.prims.p, n, pb.p, scene_ord.p);
    hipLaunchKernelGGL(k_morton, grid(n), blk, 0, stream, pb.p, n, scene_ord.p, keys.p, vals.p);
    size_t temp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys.p, keys_s.p, vals.p, vals_s.p, (size_t)n, 0, 63, stream));
    HIP_TRY(temp.alloc(temp_bytes));
    mem.sample("sort");
    HIP_TRY(rocprim::radix_sort_pairs(temp.p, temp_bytes, keys.p, keys_s.p, vals.p, vals_s.p, (size_t)n, 0, 63, stream));
    keys.release(), vals.release(), temp.release();

    // leaves, hierarchy, refit
    HIP_TRY(lbox.alloc(n_leaves));
    HIP_TRY(lkey.alloc(n_leaves));
    hipLaunchKernelGGL(k_leaves, grid(n_leaves), blk, 0, stream, pb.p, keys_s.p, vals_s.p, n, leaf_size, n_leaves, lbox.p, lkey.p);
    pb.release(), keys_s.release();
    HIP_TRY(ibox.alloc(n_leaves));
    HIP_TRY(child.alloc(n_leaves));
    HIP_TRY(parent_i.alloc(n_leaves));
    HIP_TRY(parent_l.alloc(n_leaves));
    HIP_TRY(flag.alloc(n_leaves));
    mem.sample("hierarchy");
    HIP_TRY(hipMemsetAsync(flag.p, 0, flag.bytes(), stream));
    hipLaunchKernelGGL(k_hierarchy, grid(n_leaves - 1), blk, 0, stream, lkey.p, n_leaves, child.p, parent_i.p, parent_l.p);
    hipLaunchKernelGGL(k_refit, grid(n_leaves), blk, 0, stream, n_leaves, child.p, parent_i.p, parent_l.p, lbox.p, ibox.p, flag.p);
    lkey.release(), parent_i.release(), parent_l.release(), flag.release();

    // collapse to 4-wide nodes, breadth-first, one launch per level (at most one node per leaf; the count is known after)
    HIP_TRY(fnodes.alloc(n_leaves));
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
                           lvl.p, child.p, ibox.p, lbox.p, leaf_size, n, fnodes.p);
    int lvl_h[MAX_LEVELS + 2];
    int ord_h[6];
    HIP_TRY(hipMemcpyAsync(lvl_h, lvl.p, sizeof(lvl_h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(ord_h, scene_ord.p, sizeof(ord_h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (lvl_h[MAX_LEVELS] != 0) return 1;  // deeper than the traversal stack allows
    lbox.release(), ibox.release(), child.release(), frontier[0].release(), frontier[1].release();
    int64_t n_nodes = 0;
    int depth = 0;
    for (int k = 0; k < MAX_LEVELS; k++)
        if (lvl_h[k] > 0) n_nodes += lvl_h[k], depth = k + 1;
    h.stats = WideBvhStats{};
    h.stats.n_nodes = n_nodes, h.stats.n_prims = n, h.stats.depth = depth;
    h.root_child = 0;
    fnodes.n = (size_t)n_nodes;  // the tail of the allocation is unused

    // compressed nodes on the scene grid (same fall-back rule as the host path)
    h.q_inflation = 1.0;
    bool use_q = false;
    if (compressed_ok) {
        double lo[3], hi[3];
        for (int a = 0; a < 3; a++) lo[a] = ord2f(ord_h[a]), hi[a] = ord2f(ord_h[3 + a]);
        const QGrid g = make_qgrid(lo, hi);
        HIP_TRY(sc.qnodes.alloc((size_t)n_nodes));
        HIP_TRY(acc.alloc(2));
        mem.sample("compression");
        HIP_TRY(hipMemsetAsync(acc.p, 0, acc.bytes(), stream));
        hipLaunchKernelGGL(k_quantise, grid(n_nodes), blk, 0, stream, fnodes.p, (int)n_nodes, g, sc.qnodes.p, acc.p);
        double acc_h[2] = {0, 0};
        HIP_TRY(hipMemcpy(acc_h, acc.p, sizeof(acc_h), hipMemcpyDeviceToHost));
        h.q_inflation = acc_h[1] > 0 ? acc_h[0] / acc_h[1] : 1.0;
        use_q = compressed_forced || h.q_inflation <= 1.10;
        for (int a = 0; a < 3; a++) h.grid_lo[a] = g.lo[a], h.grid_step[a] = g.step[a];
        if (!use_q) sc.qnodes.release();
    }
    if (!use_q) {  // full-width nodes: the float ones as they are, or widened to double (exact: still conservative)
        if constexpr (sizeof(R) == 4) {
            sc.nodes = std::move(fnodes);
        } else {
            HIP_TRY(sc.nodes.alloc((size_t)n_nodes));
            mem.sample("wide nodes");
            hipLaunchKernelGGL(k_widen_nodes, grid(n_nodes), blk, 0, stream, fnodes.p, (int)n_nodes, sc.nodes.p);
        }
    }
    fnodes.release();
    // records into leaf order (a stable sort: coincident primitives stay in shape order): shape-order and leaf-order
    // records coexist, next to the permutation and the finished nodes only
    DevBuf<PrimRec<R>> prims_sorted;
    HIP_TRY(prims_sorted.alloc(n));
    mem.sample("permute");
    hipLaunchKernelGGL((k_permute<PrimRec<R>>), grid(n), blk, 0, stream, sc.prims.p, vals_s.p, n, prims_sorted.p);
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
    // the device build gave up (tree too deep): the host builder needs every vertex after all
    int ensure_positions() {
        for (size_t i = 0; i < meshes.size(); i++) {
            if (!d_positions[i]) continue;
            HIP_TRY(real(meshes[i].positions, 3 * (size_t)meshes[i].n_vertices));
            d_positions[i] = nullptr;
        }
        return TAKE_OK;
    }
};

// What k_make_prims reads of the caller's arrays, in device memory: the mesh positions as they are (double, one copy
// per mesh, no host staging) and the four shape arrays.  Uploaded once per scene: both sides of a mixed-precision
// scene make their records from these.
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
template <class R> int make_prims_on_device(SceneT<R> &sc, const TakeSceneDesc &d, DeviceBuildInputs &in, const double *const *device_positions) {
    using namespace lbvh;
    const int n = (int)d.n_shapes;
    HostScene<R> &h = sc.host;
    const int ru = in.upload(d, device_positions);
    if (ru) return ru;
    std::vector<MeshSrc> ms(d.n_meshes);
    for (int i = 0; i < d.n_meshes; i++) {
        const MeshInfo &mi = h.meshes[i];
        ms[i] = MeshSrc{in.pos_off[i], mi.fbase, mi.material, h.materials[mi.material].tag, (mi.nbase >= 0 || mi.uvbase >= 0) ? 1 : 0};
    }
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
    hipLaunchKernelGGL(k_make_prims<R>, dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), 0, nullptr, in.kind.p, in.ref.p, in.face.p,
                       in.area_light.p, d_ms.p, in.pos.p, sc.face_idx.p, d_ss.p, n, sc.prims.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));  // (a failed kernel is reported here, not by a later call)
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
        int rc = make_prims_on_device(sc, desc, inputs, staged.any ? staged.d_positions.data() : nullptr);
        if (last_side) inputs.release();  // (positions and shape arrays: not part of the build's peak)
        clock.lap("mesh arrays -> HBM, records");
        if (!rc) rc = build_bvh_device(sc, max_leaf, compressed_nodes_supported() && fmt != "wide", fmt == "q16");
        if (rc == 1) {  // not buildable on the device (tree too deep): do it on the host after all
            on_device = false;
            sc.prims.release();
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
        // builder of every side's tree: AUTO = host SAH (best trees) up to 4M shapes, device LBVH beyond: at 10M triangles
        // the host build is 6 s of setup per side against 0.2 s, for 2-6 % of traversal speed.  The device
        // builder needs enough primitives to make a tree and no instances.
        const bool device_builder = local.n_shapes >= 8 && local.n_instances == 0 &&
                                    (o.builder == TAKE_BUILDER_DEVICE_LBVH || (o.builder == TAKE_BUILDER_AUTO && local.n_shapes >= TAKE_AUTO_DEVICE_BUILD_SHAPES));
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

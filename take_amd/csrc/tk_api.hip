// tk_api.hip — implementation of the C ABI of include/take_hip.h: scene creation (host preparation, the choice of
// builder, upload), scene groups, and the C entry points.  Tracing and rendering — everything that launches a kernel of
// tk_kernels.h — is tk_render.hip; the device LBVH build — every kernel of tk_build_gpu.h — is tk_build.hip; both are
// reached through the functions of tk_scene_handle.h.  The one kernel launched here is the groups' row scatter.  There
// is no CPU rendering path in this library: without a HIP device every entry point returns TAKE_E_NO_GPU.  The mesh
// entry points (PLY, serialized, OBJ, compute_normals) are tk_mesh.hip; the plumbing all units share is tk_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
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

using namespace tk;
using namespace tk_host;

namespace {

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


// the leaf size request of a build: the caller's, else the environment's (a tuning knob), else 0 = the builder's default
int requested_max_leaf(const TakeBuildOpts &opts) {
    int max_leaf = opts.max_leaf_size;
    if (max_leaf <= 0 && std::getenv("TAKE_HIP_MAX_LEAF")) max_leaf = std::atoi(std::getenv("TAKE_HIP_MAX_LEAF"));
    return max_leaf;
}

// One precision's side of a new scene: records, tree and shading tables prepared on the host and uploaded, or with
// device_builder the records and the tree made on the device — and, when the device tree would be too deep, on the
// host after all.  staged: the description's device-array meshes (StagedMeshes::stage).  inputs: what the device
// builder reads of the caller's arrays, shared by the sides of the scene; last_side: nothing needs them after this one.
template <class R>
int upload_scene(SceneT<R> &sc, int num_cus, const TakeSceneDesc &desc, const TakeBuildOpts &opts, int threads, bool device_builder,
                 StagedMeshes &staged, DeviceBuildInputs &inputs, bool last_side) {
    PhaseClock clock(sizeof(R) == 4 ? "f32" : "f64");
    const int max_leaf = requested_max_leaf(opts);
    const std::string fmt = tree_knobs().nodes;
    bool on_device = device_builder;
    std::string err = prepare_scene<R>(desc, max_leaf, threads, sc.host, on_device ? PREP_DEVICE_BUILD : PREP_HOST_BUILD, opts.burley_lobes != 0);
    if (!err.empty()) return fail(TAKE_E_INVALID, err);
    clock.lap(on_device ? "host validation + tables" : "host records + SAH build");
    HostScene<R> &h = sc.host;
    if (on_device) {
        const bool compressed_ok = compressed_nodes_supported() && fmt != "wide";
        const int rc = build_side_on_device(sc, desc, inputs, staged.any ? staged.d_positions.data() : nullptr, max_leaf, compressed_ok,
                                            fmt == "q16", last_side, clock);
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
            const TreeKnobs knobs = tree_knobs();
            device_can = knobs.braid == 1 && knobs.nodes != "q8";
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
        // what take_hip_scene_set_mesh_vertices will need: the meshes' vertex counts, and for a scene without placements
        // the shape_face array in device memory — the device builder's upload, or one made here
        if (!rc) {
            ts->mesh_vertices.resize((size_t)desc->n_meshes);
            for (int i = 0; i < desc->n_meshes; i++) ts->mesh_vertices[i] = desc->meshes[i].n_vertices;
            ts->max_leaf = requested_max_leaf(o), ts->flattened = flat.meshes.size() > 0, ts->node_knob = tree_knobs().nodes;
            if (local.n_instances == 0 && !ts->flattened && local.n_shapes > 0) {
                if (inputs.face.p) {
                    ts->shape_face = std::move(inputs.face);
                } else if (ts->shape_face.alloc((size_t)local.n_shapes) != hipSuccess ||
                           hipMemcpy(ts->shape_face.p, local.shape_face, ts->shape_face.bytes(), hipMemcpyHostToDevice) != hipSuccess) {
                    rc = fail(TAKE_E_NOMEM, "out of device memory for the shape_face array");
                }
            }
        }
    } catch (const std::bad_alloc &) {
        rc = fail(TAKE_E_NOMEM, "out of host memory while preparing the scene");
    } catch (const std::exception &e) {
        rc = fail(TAKE_E_INVALID, e.what());
    }
    if (rc) return rc;
    ts->n_placements = o.instances == TAKE_INSTANCES_TWO_LEVEL ? desc->n_instances : 0;
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
    // (a workspace grown for a bigger batch keeps the accumulator: ensure_workspace only ever enlarges it, and the
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

// First-hit feature buffers (albedo, shading normal, depth, coverage, ids): tk_render.hip, features_impl.
int take_hip_render_features_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeFeatureBuffers *d_out, void *stream) {
    if (!ts || !opts || !d_out) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    return render_features_scene(ts, *opts, *d_out, (hipStream_t)stream);
}
int take_hip_render_features(TakeScene *ts, const TakeRenderOpts *opts, const TakeFeatureBuffers *host_out) {
    if (!ts || !opts || !host_out) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    const int stride = opts->strip_stride > 0 ? opts->strip_stride : 1;
    if (opts->strip_first < 0 || opts->strip_first >= stride) return fail(TAKE_E_INVALID, "strip_first must be in [0, strip_stride)");
    const int rows = take_hip_render_rows(ts, opts->strip_first, stride, nullptr);
    if (rows < 0) return rows;
    const size_t npix = (size_t)rows * ts->width(), real = ts->f64() ? 8 : 4;
    // the wanted planes in device memory, then copied out: (host pointer, bytes per pixel)
    const std::pair<void *, size_t> planes[6] = {{host_out->albedo, 3 * real}, {host_out->normal, 3 * real}, {host_out->depth, real},
                                                 {host_out->alpha, real},      {host_out->shape_id, 4},      {host_out->material_id, 4}};
    DevBuf<char> d_plane[6];
    void *d_ptr[6] = {};
    for (int k = 0; k < 6; k++) {
        if (!planes[k].first || npix == 0) continue;
        if (d_plane[k].alloc(npix * planes[k].second) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the feature buffers");
        d_ptr[k] = d_plane[k].p;
    }
    const TakeFeatureBuffers d_out{d_ptr[0], d_ptr[1], d_ptr[2], d_ptr[3], (int32_t *)d_ptr[4], (int32_t *)d_ptr[5]};
    TakeFeatureBuffers asked = npix == 0 ? *host_out : d_out;  // (an empty strip set: the checks run on what was asked for)
    const int rc = render_features_scene(ts, *opts, asked, nullptr);
    if (rc) return rc;
    for (int k = 0; k < 6; k++)
        if (d_ptr[k]) HIP_TRY(hipMemcpy(planes[k].first, d_ptr[k], d_plane[k].bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
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


// ------------------------------------------------------------------------------------------------ a resident scene changes
}  // extern "C"

namespace {
// what take_hip_scene_set_instance_transforms accepts, checked before anything is read or made
int check_repose(const TakeScene *ts, int64_t n) {
    if (ts->n_placements <= 0) return fail(TAKE_E_INVALID, "the scene has no placements (none were given, or TAKE_INSTANCES_FLATTEN expanded them)");
    if (n != ts->n_placements) return fail(TAKE_E_INVALID, "n = " + std::to_string(n) + ", but the scene has " + std::to_string(ts->n_placements) + " placements");
    const bool plain = on_primary(ts, [&](const auto &sc) {
        return sc.trace.two_level && sc.trace.nodes != NodeFormat::Q8 && (int64_t)sc.inst_trace.n == n && (int64_t)sc.host.placements.inst_proto.size() == n;
    });
    if (!plain) return fail(TAKE_E_INVALID, "unsupported: the scene was built under TAKE_HIP_BRAID > 1 or TAKE_HIP_NODES=q8");
    return TAKE_OK;
}
// New transforms (device memory, complete) for all placements of ts (check_repose passed): every side staged, then
// every side committed — a mixed scene gets both or neither.
int set_instance_transforms(TakeScene *ts, const double *d_xforms, int64_t n) {
    try {
        ReposeStage<double> sd;
        ReposeStage<float> sf;
        int rc = TAKE_OK;
        if (ts->precision != TAKE_PRECISION_F32) rc = repose_two_level_device(ts->d, d_xforms, n, sd);
        if (!rc && ts->precision != TAKE_PRECISION_F64) rc = repose_two_level_device(ts->f, d_xforms, n, sf);
        if (rc) return rc;
        if (ts->precision != TAKE_PRECISION_F32) rc = sd.commit(ts->d);
        if (!rc && ts->precision != TAKE_PRECISION_F64) rc = sf.commit(ts->f);
        ts->acc_samples = 0, ts->acc_restart_needed = true;
        return rc;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while re-posing the placements");
    }
}
}  // namespace

extern "C" {

int take_hip_scene_set_instance_transforms_device(TakeScene *ts, const double *d_xforms, int64_t n, void *stream) {
    if (!ts || !d_xforms) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    // (the build runs on the default stream, as scene_create's does: first whatever `stream` still has to write into d_xforms)
    const int rc = check_repose(ts, n);
    if (rc) return rc;
    if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return set_instance_transforms(ts, d_xforms, n);
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
    return set_instance_transforms(ts, d_xforms.p, n);
}
// New vertices for meshes of a resident scene (include/take_hip.h): the arguments that need no scene, the device, the
// arguments against the scene, what the path does not support; then every side staged and every side committed.
int take_hip_scene_set_mesh_vertices(TakeScene *ts, const TakeMeshUpdate *updates, int32_t n_updates) {
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
            const bool has_normals = on_primary(ts, [&](const auto &sc) { return (size_t)u.mesh < sc.host.meshes.size() && sc.host.meshes[u.mesh].nbase >= 0; });
            if (u.normals && !has_normals) return fail(TAKE_E_INVALID, who + "normals given for a mesh without vertex normals");
        }
        if (ts->n_placements > 0) return fail(TAKE_E_INVALID, "unsupported: a two-level scene (the prototypes' trees are not rebuilt)");
        if (ts->flattened) return fail(TAKE_E_INVALID, "unsupported: the scene was flattened from instances");
        const bool q8 = ts->node_knob == "q8" || on_primary(ts, [&](const auto &sc) { return sc.trace.nodes == NodeFormat::Q8; });
        if (q8) return fail(TAKE_E_INVALID, "unsupported: the scene was built under TAKE_HIP_NODES=q8");
        if (on_primary(ts, [&](const auto &sc) { return sc.trace.two_level; })) return fail(TAKE_E_INVALID, "unsupported: a two-level scene");
        if (!ts->shape_face.p) return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group, or has no shapes");
        if (on_primary(ts, [&](const auto &sc) { return sc.prims.n != ts->shape_face.n; }))
            return fail(TAKE_E_INVALID, "unsupported: the scene does not have one primitive record per shape");
        TAKE_ON_DEVICE(ts);
        MeshUpdateInputs in;
        int rc = in.upload(ts->mesh_vertices, updates, n_updates);
        if (rc) return rc;
        const bool compressed_ok = compressed_nodes_supported() && ts->node_knob != "wide", compressed_forced = ts->node_knob == "q16";
        MeshUpdateStage<double> sd;
        MeshUpdateStage<float> sf;
        if (ts->precision != TAKE_PRECISION_F32)
            rc = update_mesh_vertices_device(ts->d, in, ts->mesh_vertices, ts->shape_face.p, ts->max_leaf, compressed_ok, compressed_forced, ts->num_cus, sd);
        if (!rc && ts->precision != TAKE_PRECISION_F64)
            rc = update_mesh_vertices_device(ts->f, in, ts->mesh_vertices, ts->shape_face.p, ts->max_leaf, compressed_ok, compressed_forced, ts->num_cus, sf);
        if (rc) return rc;
        if (ts->precision != TAKE_PRECISION_F32) sd.commit(ts->d);
        if (ts->precision != TAKE_PRECISION_F64) sf.commit(ts->f);
        ts->acc_samples = 0, ts->acc_restart_needed = true;
        return TAKE_OK;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while updating the meshes");
    } catch (const std::exception &e) {
        return fail(TAKE_E_INVALID, std::string("updating the meshes failed: ") + e.what());
    }
}
int take_hip_scene_set_camera(TakeScene *ts, const TakeCamera *camera) {
    if (!ts || !camera) return fail(TAKE_E_INVALID, "null argument");
    if (camera->width != ts->width() || camera->height != ts->height())
        return fail(TAKE_E_INVALID, "the new camera is " + std::to_string(camera->width) + " x " + std::to_string(camera->height) + ", the scene " +
                                        std::to_string(ts->width()) + " x " + std::to_string(ts->height()) + ": the render buffers are sized at creation");
    if (ts->precision != TAKE_PRECISION_F32) make_camera<double>(*camera, ts->d.host.cam), ts->d.dev.cam = ts->d.host.cam;
    if (ts->precision != TAKE_PRECISION_F64) make_camera<float>(*camera, ts->f.host.cam), ts->f.dev.cam = ts->f.host.cam;
    ts->acc_samples = 0, ts->acc_restart_needed = true;
    return TAKE_OK;
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
    ts->n_placements = src->n_placements;
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

// ------------------------------------------------------------------------------------------------ test hook: the resident tree
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
bool has_side(const TakeScene *ts, int32_t side) {
    return side == TAKE_PRECISION_F32 ? ts->precision != TAKE_PRECISION_F64 : side == TAKE_PRECISION_F64 && ts->precision != TAKE_PRECISION_F32;
}
}  // namespace

extern "C" {

int take_hip_debug_tree_info(const TakeScene *ts, int32_t side, TakeDebugTreeInfo *info) {
    if (!ts || !info) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    *info = side == TAKE_PRECISION_F64 ? debug_tree_info(ts->d) : debug_tree_info(ts->f);
    return TAKE_OK;
}
int take_hip_debug_tree(const TakeScene *ts, int32_t side, void *nodes, void *prims, void *inst_trace) {
    if (!ts || !nodes || !prims) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    if (!has_side(ts, side)) return fail(TAKE_E_INVALID, "the scene has no such side");
    TAKE_ON_DEVICE(ts);
    HIP_TRY(hipDeviceSynchronize());
    return side == TAKE_PRECISION_F64 ? debug_tree_copy(ts->d, nodes, prims, inst_trace) : debug_tree_copy(ts->f, nodes, prims, inst_trace);
}

}  // extern "C"

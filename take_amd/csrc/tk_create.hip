// tk_create.hip — scene creation: the description flattened or staged where asked, the choice of builder, and per
// precision side the host preparation (tk_host_scene.h), the device or the host build, and the upload (upload_scene);
// take_hip_scene_destroy.  Launches no kernel: the device build is tk_build.hip, reached through tk_scene_handle.h.
#include <hip/hip_runtime.h>

#include <algorithm>
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
// builder reads of the caller's arrays, shared by the sides of the scene: nothing needs them after the last, the f32 or only one.
template <class R>
int upload_scene(SceneT<R> &sc, int num_cus, const TakeSceneDesc &desc, const TakeBuildOpts &opts, int threads, bool device_builder,
                 StagedMeshes &staged, DeviceBuildInputs &inputs) {
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
                                            fmt == "q16", sizeof(R) == 4 || opts.precision == TAKE_PRECISION_F64, clock);
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
    HIP_TRY(alloc_trace_state(sc, num_cus));  // the persistent trace grid
    clock.lap("shading tables -> HBM, grid");
    // everything the kernels read is in HBM now; the host keeps the small tables (camera, material tags, tree
    // statistics) and drops the copies of the large arrays (1.1 GB at 10M triangles)
    h.nodes = {}, h.qnodes = {}, h.qnodes8 = {}, h.nodes8 = {}, h.prims = {}, h.shapes = {}, h.face_idx = {}, h.normals = {}, h.uvs = {}, h.texels = {};
    h.inst_trace = {}, h.inst_shade = {};
    return TAKE_OK;
}

}  // namespace

extern "C" {

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
    ts->precision = o.precision, ts->burley_lobes = o.burley_lobes != 0;
    ts->look_distance = look_distance(desc->camera), ts->camera = desc->camera;
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
        // (a mixed scene's two sides are two independent trees, each from its own records' boxes, over one upload of the caller's arrays)
        DeviceBuildInputs inputs;
        if (!rc) rc = for_each_side(ts.get(), [&](auto &sc) { return upload_scene(sc, ts->num_cus, local, o, threads, device_builder, staged, inputs); });
        if (!rc) rc = on_primary(ts.get(), [](auto &, auto &work) -> int { HIP_TRY(work.create()); return TAKE_OK; });  // queue words, counters
        // what take_hip_scene_set_mesh_vertices / _update_meshes will need: the meshes' vertex counts, the shape_face
        // array in device memory — the device builder's upload, or one made here — and, of a two-level scene, the
        // placements' transforms in double
        if (!rc) {
            ts->mesh_vertices.resize((size_t)desc->n_meshes);
            for (int i = 0; i < desc->n_meshes; i++) ts->mesh_vertices[i] = desc->meshes[i].n_vertices;
            ts->max_leaf = requested_max_leaf(o), ts->flattened = flat.meshes.size() > 0, ts->node_knob = tree_knobs().nodes;
            if (!ts->flattened && local.n_shapes > 0) {
                if (inputs.face.p) {
                    ts->shape_face = std::move(inputs.face);
                } else if (ts->shape_face.alloc((size_t)local.n_shapes) != hipSuccess ||
                           hipMemcpy(ts->shape_face.p, local.shape_face, ts->shape_face.bytes(), hipMemcpyHostToDevice) != hipSuccess) {
                    rc = fail(TAKE_E_NOMEM, "out of device memory for the shape_face array");
                }
            }
            if (!rc && local.n_instances > 0) {
                std::vector<double> xf(12 * (size_t)local.n_instances);
                for (int64_t i = 0; i < local.n_instances; i++) std::memcpy(&xf[12 * (size_t)i], local.instances[i].xform, 12 * sizeof(double));
                if (ts->xforms.upload(xf) != hipSuccess) rc = fail(TAKE_E_NOMEM, "out of device memory for the placements' transforms");
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

}  // extern "C"

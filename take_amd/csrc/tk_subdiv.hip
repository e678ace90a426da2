// tk_subdiv.hip — Loop subdivision surfaces on the device (include/take_hip.h: take_hip_subdiv_*,
// take_hip_scene_subdivide_meshes), and the only unit that compiles the kernels of tk_subdiv.h.  A handle
// owns every buffer a refine touches, so a refine allocates nothing; take_hip_scene_subdivide_meshes refines into those
// buffers and hands them to take_hip_scene_update_meshes as device arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"
#include "tk_subdiv.h"

using namespace tk;
using namespace tk_host;

struct TakeSubdiv {
    int device = 0;
    int64_t cage_vertices = 0, n_vertices = 0, n_faces = 0;
    int32_t levels = 0;
    struct Level {  // the tables of one level in device memory
        int64_t n_vertices = 0, n_edges = 0;
        DevBuf<subdiv::Edge> edges;
        DevBuf<int32_t> nbr_start, nbr, bnd;
        subdiv::LevelView view() const { return {n_vertices, n_edges, edges.p, nbr_start.p, nbr.p, bnd.p}; }
    };
    std::vector<Level> level;
    DevBuf<int32_t> indices, face_start, faces;  // the refined mesh: its faces, every vertex's row of faces
    // what a refine writes: the staged cage of a host call (or a bound rig's pose), the levels between the cage and the
    // result (level l writes ping[l & 1]; the last one the caller's array), the face normals, the handle's own results
    DevBuf<double> cage, ping[2], face_n, out_p, out_n;
    size_t device_bytes() const {
        size_t b = indices.bytes() + face_start.bytes() + faces.bytes() + cage.bytes() + ping[0].bytes() + ping[1].bytes() + face_n.bytes() + out_p.bytes() + out_n.bytes();
        for (const Level &l : level) b += l.edges.bytes() + l.nbr_start.bytes() + l.nbr.bytes() + l.bnd.bytes();
        return b;
    }
};

namespace {

const char *NOMEM = "out of device memory for the subdivision tables";

template <class T> int upload(DevBuf<T> &dst, const std::vector<T> &src) {
    if (dst.alloc(src.size()) != hipSuccess) return fail(TAKE_E_NOMEM, NOMEM);
    if (!src.empty()) HIP_TRY(hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return TAKE_OK;
}

// what all three calls that take a description refuse of it, then the topology
int topology_of(const TakeSubdivDesc *d, bool keep_tables, subdiv::Topology &topo) {
    if (!d || !d->indices) return fail(TAKE_E_INVALID, "null argument");
    if (d->flags != 0) return fail(TAKE_E_INVALID, "unknown flag bits");
    std::string msg;
    if (subdiv::build_topology(d->n_vertices, d->n_faces, d->indices, d->uvs, d->levels, keep_tables, topo, msg) != subdiv::TOPOLOGY_OK) return fail(TAKE_E_INVALID, msg);
    return TAKE_OK;
}

int subdiv_create(const TakeSubdivDesc *d, TakeSubdiv **out) {
    subdiv::Topology topo;
    if (int rc = topology_of(d, true, topo)) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    TakeSubdiv *s = new TakeSubdiv();
    struct Drop {
        TakeSubdiv *s;
        ~Drop() { delete s; }
    } drop{s};
    HIP_TRY(hipGetDevice(&s->device));
    s->cage_vertices = d->n_vertices, s->n_vertices = topo.n_vertices, s->n_faces = topo.n_faces, s->levels = d->levels;
    s->level.resize((size_t)d->levels);
    size_t between[2] = {0, 0};
    for (int32_t l = 0; l < d->levels; l++) {
        const subdiv::Level &h = topo.levels[l];
        TakeSubdiv::Level &lv = s->level[l];
        lv.n_vertices = h.n_vertices, lv.n_edges = h.n_edges;
        if (int rc = upload(lv.edges, h.edges)) return rc;
        if (int rc = upload(lv.nbr_start, h.nbr_start)) return rc;
        if (int rc = upload(lv.nbr, h.nbr)) return rc;
        if (int rc = upload(lv.bnd, h.bnd)) return rc;
        if (l + 1 < d->levels) between[l & 1] = std::max(between[l & 1], 3 * (size_t)(h.n_vertices + h.n_edges));
    }
    if (int rc = upload(s->indices, topo.indices)) return rc;
    if (int rc = upload(s->face_start, topo.face_start)) return rc;
    if (int rc = upload(s->faces, topo.faces)) return rc;
    const size_t nv = (size_t)topo.n_vertices;
    if (s->cage.alloc(3 * (size_t)d->n_vertices) != hipSuccess || s->ping[0].alloc(between[0]) != hipSuccess || s->ping[1].alloc(between[1]) != hipSuccess ||
        s->face_n.alloc(3 * (size_t)topo.n_faces) != hipSuccess || s->out_p.alloc(3 * nv) != hipSuccess || s->out_n.alloc(3 * nv) != hipSuccess)
        return fail(TAKE_E_NOMEM, NOMEM);
    drop.s = nullptr;
    *out = s;
    return TAKE_OK;
}

// Every level, then the normals, on `stream`; the handle's device is current; d_cage is device memory.  out_n null: no
// normals are computed.  Allocates nothing, and the host waits once, at the end.  TAKE_HIP_VERBOSE=1: every launch between
// events, printed to stderr once all have completed.
int refine_on_stream(TakeSubdiv &s, const double *d_cage, double *out_p, double *out_n, hipStream_t stream) {
    const int L = s.levels;
    EventPool events;
    hipEvent_t ev[2 * subdiv::MAX_LEVELS + 3] = {};
    const int n_ev = 2 * L + 3;
    bool clocked = std::getenv("TAKE_HIP_VERBOSE") != nullptr;
    for (int i = 0; clocked && i < n_ev; i++) clocked = (ev[i] = events.get()) != nullptr;
    int mark = 0;
    auto tick = [&]() {
        if (clocked) (void)hipEventRecord(ev[mark++], stream);
    };
    const dim3 block(subdiv::BLOCK);
    const double *in = d_cage;
    tick();
    for (int l = 0; l < L; l++) {
        const subdiv::LevelView t = s.level[l].view();
        double *out = l == L - 1 ? out_p : s.ping[l & 1].p;
        hipLaunchKernelGGL(subdiv::k_subdiv_even, dim3((unsigned)subdiv::blocks_for(t.n_vertices)), block, 0, stream, t, in, out);
        tick();
        hipLaunchKernelGGL(subdiv::k_subdiv_odd, dim3((unsigned)subdiv::blocks_for(t.n_edges)), block, 0, stream, t, in, out);
        tick();
        in = out;
    }
    // TAKE_HIP_SUBDIV_NORMALS=recompute: the variant without the face-normal array (a measurement switch: same bits)
    const char *variant = std::getenv("TAKE_HIP_SUBDIV_NORMALS");
    const bool recompute = variant && std::string(variant) == "recompute";
    if (out_n && recompute) {
        tick();
        hipLaunchKernelGGL(subdiv::k_subdiv_vertex_normals_recomputed, dim3((unsigned)subdiv::blocks_for(s.n_vertices)), block, 0, stream, (const int32_t *)s.face_start.p,
                           (const int32_t *)s.faces.p, (const int32_t *)s.indices.p, (const double *)out_p, s.n_vertices, out_n);
        tick();
    } else if (out_n) {
        subdiv_launch_normals(s.indices.p, s.face_start.p, s.faces.p, out_p, s.n_faces, s.n_vertices, s.face_n.p, out_n, stream, clocked ? ev[mark] : nullptr);
        mark++;
        tick();
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    if (clocked) {
        float ms = 0;
        for (int l = 0; l < L; l++) {
            if (hipEventElapsedTime(&ms, ev[2 * l], ev[2 * l + 1]) == hipSuccess)
                std::fprintf(stderr, "[take_hip] subdiv_refine: level %d k_subdiv_even %lld vertices %9.4f ms\n", l + 1, (long long)s.level[l].n_vertices, ms);
            if (hipEventElapsedTime(&ms, ev[2 * l + 1], ev[2 * l + 2]) == hipSuccess)
                std::fprintf(stderr, "[take_hip] subdiv_refine: level %d k_subdiv_odd %lld edges %9.4f ms\n", l + 1, (long long)s.level[l].n_edges, ms);
        }
        if (out_n && recompute && hipEventElapsedTime(&ms, ev[2 * L + 1], ev[2 * L + 2]) == hipSuccess)
            std::fprintf(stderr, "[take_hip] subdiv_refine: normals k_subdiv_vertex_normals_recomputed %lld vertices %9.4f ms\n", (long long)s.n_vertices, ms);
        if (out_n && !recompute && hipEventElapsedTime(&ms, ev[2 * L], ev[2 * L + 1]) == hipSuccess)
            std::fprintf(stderr, "[take_hip] subdiv_refine: normals k_subdiv_face_normals %lld faces %9.4f ms\n", (long long)s.n_faces, ms);
        if (out_n && !recompute && hipEventElapsedTime(&ms, ev[2 * L + 1], ev[2 * L + 2]) == hipSuccess)
            std::fprintf(stderr, "[take_hip] subdiv_refine: normals k_subdiv_vertex_normals %lld vertices %9.4f ms\n", (long long)s.n_vertices, ms);
    }
    return TAKE_OK;
}

// a cage from host memory goes through the handle's staging buffer, on the stream the refine runs on
int refine_from(TakeSubdiv &s, const double *cage, bool on_device, double *out_p, double *out_n, hipStream_t stream) {
    if (!on_device) {
        HIP_TRY(hipMemcpyAsync(s.cage.p, cage, s.cage.bytes(), hipMemcpyHostToDevice, stream));
        cage = s.cage.p;
    }
    return refine_on_stream(s, cage, out_p, out_n, stream);
}

int subdivide_meshes(TakeScene *ts, const TakeSubdivBinding *bindings, int32_t n) {
    if (!ts || !bindings) return fail(TAKE_E_INVALID, "null argument");
    if (n <= 0) return fail(TAKE_E_INVALID, "n must be positive");
    std::vector<int32_t> meshes((size_t)n);
    std::vector<const TakeSubdiv *> handles((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const TakeSubdivBinding &b = bindings[i];
        const std::string who = "binding " + std::to_string(i) + ": ";
        if (b.mesh < 0) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        if (!b.subdiv) return fail(TAKE_E_INVALID, who + "null argument");
        if (b.flags & ~TAKE_SUBDIV_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, who + "unknown flag bits");
        if ((b.cage_positions != nullptr) == (b.rig != nullptr)) return fail(TAKE_E_INVALID, who + "exactly one of cage_positions and rig must be given");
        if (b.rig)
            if (int rc = rig_check_pose(b.rig, &b.pose, who)) return rc;
        meshes[i] = b.mesh, handles[i] = b.subdiv;
    }
    std::sort(meshes.begin(), meshes.end());
    std::sort(handles.begin(), handles.end());
    for (int32_t i = 1; i < n; i++) {
        if (meshes[i] == meshes[i - 1]) return fail(TAKE_E_INVALID, "mesh " + std::to_string(meshes[i]) + " appears more than once");
        if (handles[i] == handles[i - 1]) return fail(TAKE_E_INVALID, "a subdivision handle is bound more than once");
    }
    const int nd = check_device();
    if (nd < 0) return nd;
    std::vector<TakeMeshUpdate> updates((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const TakeSubdivBinding &b = bindings[i];
        const std::string who = "binding " + std::to_string(i) + ": ";
        if ((size_t)b.mesh >= ts->mesh_vertices.size()) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        if (b.subdiv->device != ts->device) return fail(TAKE_E_INVALID, who + "the subdivision handle lives on another device than the scene");
        if (b.rig) {
            int device = 0;
            int64_t nv = 0;
            rig_shape(b.rig, &device, &nv);
            if (device != ts->device) return fail(TAKE_E_INVALID, who + "the rig lives on another device than the scene");
            if (nv != b.subdiv->cage_vertices)
                return fail(TAKE_E_INVALID, who + "the rig has " + std::to_string(nv) + " vertices, the cage has " + std::to_string(b.subdiv->cage_vertices));
        }
        if (b.subdiv->n_vertices != ts->mesh_vertices[b.mesh])
            return fail(TAKE_E_INVALID, who + "the refined cage has " + std::to_string(b.subdiv->n_vertices) + " vertices, mesh " + std::to_string(b.mesh) + " has " +
                                            std::to_string(ts->mesh_vertices[b.mesh]));
        const bool normals = on_primary(ts, [&](const auto &sc, const auto &) { return (size_t)b.mesh < sc.host.meshes.size() && sc.host.meshes[b.mesh].nbase >= 0; });
        updates[i] = TakeMeshUpdate{b.mesh, TAKE_MESH_DEVICE_ARRAYS, b.subdiv->out_p.p, normals ? b.subdiv->out_n.p : nullptr};
    }
    // the poses and the refines, on the default stream as the update: handle-owned memory only, before anything of the
    // scene is staged
    for (int32_t i = 0; i < n; i++) {
        const TakeSubdivBinding &b = bindings[i];
        const double *p = nullptr, *nrm = nullptr;
        if (int rc = subdiv_refine_own(b.subdiv, b.cage_positions, (b.flags & TAKE_SUBDIV_DEVICE_ARRAYS) != 0, b.rig, &b.pose, updates[i].normals != nullptr, &p, &nrm)) return rc;
    }
    return take_hip_scene_update_meshes(ts, updates.data(), n);
}

}  // namespace

// what tk_displace.hip calls of this unit (tk_host.h)
void tk_host::subdiv_shape(const TakeSubdiv *subdiv, int *device, int64_t *cage_vertices, int64_t *n_vertices) {
    *device = subdiv->device, *cage_vertices = subdiv->cage_vertices, *n_vertices = subdiv->n_vertices;
}
int tk_host::subdiv_refine_own(TakeSubdiv *subdiv, const double *cage_positions, bool on_device, TakeRig *rig, const TakeRigPose *pose, bool normals,
                               const double **d_positions, const double **d_normals) {
    TakeSubdiv &s = *subdiv;
    if (rig)  // (posed into the handle's staged cage: positions alone — the normals are the refined surface's)
        if (int rc = take_hip_rig_pose_device(rig, pose, s.cage.p, nullptr, nullptr)) return rc;
    DeviceGuard guard(s.device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the subdivision handle's device current");
    if (int rc = refine_from(s, rig ? s.cage.p : cage_positions, rig || on_device, s.out_p.p, normals ? s.out_n.p : nullptr, nullptr)) return rc;
    *d_positions = s.out_p.p, *d_normals = normals ? s.out_n.p : nullptr;
    return TAKE_OK;
}
void tk_host::subdiv_launch_normals(const int32_t *indices, const int32_t *face_start, const int32_t *faces, const double *positions, int64_t n_faces, int64_t n_vertices,
                                    double *face_n, double *out_n, hipStream_t stream, hipEvent_t between) {
    const dim3 block(subdiv::BLOCK);
    hipLaunchKernelGGL(subdiv::k_subdiv_face_normals, dim3((unsigned)subdiv::blocks_for(n_faces)), block, 0, stream, indices, positions, n_faces, face_n);
    if (between) (void)hipEventRecord(between, stream);
    hipLaunchKernelGGL(subdiv::k_subdiv_vertex_normals, dim3((unsigned)subdiv::blocks_for(n_vertices)), block, 0, stream, face_start, faces, (const double *)face_n, n_vertices,
                       out_n);
}

extern "C" {

int take_hip_subdiv_counts(const TakeSubdivDesc *desc, int64_t *n_vertices_out, int64_t *n_faces_out) {
    try {
        subdiv::Topology topo;
        if (int rc = topology_of(desc, false, topo)) return rc;
        if (n_vertices_out) *n_vertices_out = topo.n_vertices;
        if (n_faces_out) *n_faces_out = topo.n_faces;
        return TAKE_OK;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory for the subdivision topology");
    }
}
int take_hip_subdiv_topology(const TakeSubdivDesc *desc, int32_t *indices_out, double *uvs_out) {
    try {
        if (!indices_out) return fail(TAKE_E_INVALID, "null argument");
        if (desc && uvs_out && !desc->uvs) return fail(TAKE_E_INVALID, "uvs wanted from a cage without uvs");
        subdiv::Topology topo;
        if (int rc = topology_of(desc, false, topo)) return rc;
        std::copy(topo.indices.begin(), topo.indices.end(), indices_out);
        if (uvs_out) std::copy(topo.uvs.begin(), topo.uvs.end(), uvs_out);
        return TAKE_OK;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory for the subdivision topology");
    }
}
int take_hip_subdiv_create(const TakeSubdivDesc *desc, TakeSubdiv **out) {
    if (!desc || !out) return fail(TAKE_E_INVALID, "null argument");
    try {
        return subdiv_create(desc, out);
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory for the subdivision tables");
    }
}
int take_hip_subdiv_destroy(TakeSubdiv *subdiv) {
    if (!subdiv) return fail(TAKE_E_INVALID, "null argument");
    DeviceGuard guard(subdiv->device);  // (the buffers are freed on the handle's device)
    delete subdiv;
    return TAKE_OK;
}
int take_hip_subdiv_info(const TakeSubdiv *subdiv, int64_t *cage_vertices, int64_t *n_vertices, int64_t *n_faces, int32_t *levels, int64_t *device_bytes) {
    if (!subdiv) return fail(TAKE_E_INVALID, "null argument");
    if (cage_vertices) *cage_vertices = subdiv->cage_vertices;
    if (n_vertices) *n_vertices = subdiv->n_vertices;
    if (n_faces) *n_faces = subdiv->n_faces;
    if (levels) *levels = subdiv->levels;
    if (device_bytes) *device_bytes = (int64_t)subdiv->device_bytes();
    return TAKE_OK;
}
int take_hip_subdiv_refine_device(TakeSubdiv *subdiv, const double *cage_positions, int32_t flags, double *d_positions_out, double *d_normals_out, void *stream) {
    if (!subdiv || !cage_positions || !d_positions_out) return fail(TAKE_E_INVALID, "null argument");
    if (flags & ~TAKE_SUBDIV_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, "unknown flag bits");
    const int nd = check_device();
    if (nd < 0) return nd;
    DeviceGuard guard(subdiv->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the subdivision handle's device current");
    return refine_from(*subdiv, cage_positions, (flags & TAKE_SUBDIV_DEVICE_ARRAYS) != 0, d_positions_out, d_normals_out, (hipStream_t)stream);
}
int take_hip_subdiv_refine(TakeSubdiv *subdiv, const double *cage_positions, double *positions_out, double *normals_out) {
    if (!subdiv || !cage_positions || !positions_out) return fail(TAKE_E_INVALID, "null argument");
    const int nd = check_device();
    if (nd < 0) return nd;
    DeviceGuard guard(subdiv->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the subdivision handle's device current");
    if (int rc = refine_from(*subdiv, cage_positions, false, subdiv->out_p.p, normals_out ? subdiv->out_n.p : nullptr, nullptr)) return rc;
    HIP_TRY(hipMemcpy(positions_out, subdiv->out_p.p, subdiv->out_p.bytes(), hipMemcpyDeviceToHost));
    if (normals_out) HIP_TRY(hipMemcpy(normals_out, subdiv->out_n.p, subdiv->out_n.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}
int take_hip_scene_subdivide_meshes(TakeScene *ts, const TakeSubdivBinding *bindings, int32_t n) {
    try {
        return subdivide_meshes(ts, bindings, n);
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while subdividing the meshes");
    }
}

}  // extern "C"

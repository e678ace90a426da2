// tk_displace.hip — displacement mapping on the device (include/take_hip.h: take_hip_displace_*,
// take_hip_scene_displace_meshes), and the only unit that compiles the kernel of tk_displace.h.  A handle
// owns every buffer a call touches, so a call allocates nothing; take_hip_scene_displace_meshes displaces into those
// buffers and hands them to take_hip_scene_update_meshes as device arrays.  The normals in front of and behind the
// displacement are tk_subdiv.hip's launches (tk_host.h: subdiv_launch_normals).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "take_hip.h"
#include "tk_displace.h"
#include "tk_scene_handle.h"

using namespace tk;
using namespace tk_host;

struct TakeDisplace {
    int device = 0;
    int64_t n_vertices = 0, n_faces = 0;
    int32_t width = 0, height = 0, real = TAKE_PRECISION_F32;
    DevBuf<char> texels;                         // the image, in the width it came in
    DevBuf<displace::Source> sources;            // every vertex's (a, b)
    DevBuf<int32_t> indices, face_start, faces;  // the mesh: its faces, every vertex's row of faces
    // what a call writes: the staged base positions of a host call, the direction normals (staged, or the handle's
    // own), the face normals of either normal pass, the handle's own results
    DevBuf<double> base_p, base_n, face_n, out_p, out_n;
    size_t device_bytes() const {
        return texels.bytes() + sources.bytes() + indices.bytes() + face_start.bytes() + faces.bytes() + base_p.bytes() + base_n.bytes() + face_n.bytes() + out_p.bytes() +
               out_n.bytes();
    }
};

namespace {

const char *NOMEM = "out of device memory for the displacement tables";
const char *WRONG_DEVICE = "cannot make the displacement handle's device current";

template <class T> int upload(DevBuf<T> &dst, const std::vector<T> &src) {
    if (dst.alloc(src.size()) != hipSuccess) return fail(TAKE_E_NOMEM, NOMEM);
    if (!src.empty()) HIP_TRY(hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return TAKE_OK;
}

int displace_create(const TakeDisplaceDesc *d, TakeDisplace **out) {
    std::string msg;
    const double lookup[4] = {d->uscale, d->vscale, d->uoffset, d->voffset};
    static_assert(TAKE_PRECISION_F32 == 0 && TAKE_PRECISION_F64 == 1, "tk_displace.h names the two texel widths 0 and 1");
    if (displace::check_inputs(d->n_vertices, d->n_faces, d->indices, d->uvs, d->width, d->height, d->texels, d->real, d->flags, TAKE_DISPLACE_DEVICE_ARRAYS, lookup, msg))
        return fail(TAKE_E_INVALID, msg);
    std::vector<displace::Source> sources;
    if (displace::build_sources(d->n_vertices, d->uvs, lookup, sources, msg)) return fail(TAKE_E_INVALID, msg);
    const int nd = check_device();
    if (nd < 0) return nd;
    std::vector<int32_t> face_start, faces;
    displace::build_rows(d->n_vertices, d->n_faces, d->indices, face_start, faces);
    TakeDisplace *s = new TakeDisplace();
    struct Drop {
        TakeDisplace *s;
        ~Drop() { delete s; }
    } drop{s};
    HIP_TRY(hipGetDevice(&s->device));
    s->n_vertices = d->n_vertices, s->n_faces = d->n_faces, s->width = d->width, s->height = d->height, s->real = d->real;
    const size_t texel_bytes = (size_t)d->width * (size_t)d->height * (d->real == TAKE_PRECISION_F64 ? sizeof(double) : sizeof(float));
    if (s->texels.alloc(texel_bytes) != hipSuccess) return fail(TAKE_E_NOMEM, NOMEM);
    HIP_TRY(hipMemcpy(s->texels.p, d->texels, texel_bytes, (d->flags & TAKE_DISPLACE_DEVICE_ARRAYS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (int rc = upload(s->sources, sources)) return rc;
    if (s->indices.alloc(3 * (size_t)d->n_faces) != hipSuccess) return fail(TAKE_E_NOMEM, NOMEM);
    HIP_TRY(hipMemcpy(s->indices.p, d->indices, s->indices.bytes(), hipMemcpyHostToDevice));
    if (int rc = upload(s->face_start, face_start)) return rc;
    if (int rc = upload(s->faces, faces)) return rc;
    const size_t nv = (size_t)d->n_vertices;
    if (s->base_p.alloc(3 * nv) != hipSuccess || s->base_n.alloc(3 * nv) != hipSuccess || s->face_n.alloc(3 * (size_t)d->n_faces) != hipSuccess ||
        s->out_p.alloc(3 * nv) != hipSuccess || s->out_n.alloc(3 * nv) != hipSuccess)
        return fail(TAKE_E_NOMEM, NOMEM);
    HIP_TRY(hipDeviceSynchronize());  // (a device-to-device copy of the texels need not have completed)
    drop.s = nullptr;
    *out = s;
    return TAKE_OK;
}

// The direction normals unless given, the displacement, the normals of the result unless out_n is null, on `stream`; the
// handle's device is current; d_p and d_n are device memory (d_n null: the handle's own normals of d_p).  Allocates
// nothing, and the host waits once, at the end.  TAKE_HIP_VERBOSE=1: every launch between events, printed to stderr once
// all have completed.
int displace_on_stream(TakeDisplace &s, const double *d_p, const double *d_n, double scale, double bias, double *out_p, double *out_n, hipStream_t stream) {
    EventPool events;
    hipEvent_t ev[6] = {};
    bool clocked = std::getenv("TAKE_HIP_VERBOSE") != nullptr;
    for (int i = 0; clocked && i < 6; i++) clocked = (ev[i] = events.get()) != nullptr;
    auto tick = [&](int i) {
        if (clocked) (void)hipEventRecord(ev[i], stream);
    };
    const bool own = d_n == nullptr;
    tick(0);
    if (own) {
        subdiv_launch_normals(s.indices.p, s.face_start.p, s.faces.p, d_p, s.n_faces, s.n_vertices, s.face_n.p, s.base_n.p, stream, clocked ? ev[1] : nullptr);
        d_n = s.base_n.p;
    }
    tick(2);
    const dim3 grid((unsigned)displace::blocks_for(s.n_vertices)), block(displace::BLOCK);
    if (s.real == TAKE_PRECISION_F64)
        hipLaunchKernelGGL(displace::k_displace<double>, grid, block, 0, stream, (const displace::Source *)s.sources.p, (const double *)s.texels.p, s.width, s.height, scale,
                           bias, d_p, d_n, s.n_vertices, out_p);
    else
        hipLaunchKernelGGL(displace::k_displace<float>, grid, block, 0, stream, (const displace::Source *)s.sources.p, (const float *)s.texels.p, s.width, s.height, scale,
                           bias, d_p, d_n, s.n_vertices, out_p);
    tick(3);
    if (out_n) subdiv_launch_normals(s.indices.p, s.face_start.p, s.faces.p, out_p, s.n_faces, s.n_vertices, s.face_n.p, out_n, stream, clocked ? ev[4] : nullptr);
    tick(5);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    if (clocked) {
        float ms = 0;
        auto say = [&](int from, const char *what, const char *kernel, long long n, const char *of) {
            if (hipEventElapsedTime(&ms, ev[from], ev[from + 1]) == hipSuccess)
                std::fprintf(stderr, "[take_hip] displace_apply: %s %s %lld %s %9.4f ms\n", what, kernel, n, of, ms);
        };
        if (own) say(0, "direction", "k_subdiv_face_normals", (long long)s.n_faces, "faces"), say(1, "direction", "k_subdiv_vertex_normals", (long long)s.n_vertices, "vertices");
        say(2, "positions", s.real == TAKE_PRECISION_F64 ? "k_displace<double>" : "k_displace<float>", (long long)s.n_vertices, "vertices");
        if (out_n) say(3, "normals", "k_subdiv_face_normals", (long long)s.n_faces, "faces"), say(4, "normals", "k_subdiv_vertex_normals", (long long)s.n_vertices, "vertices");
    }
    return TAKE_OK;
}

// base arrays from host memory go through the handle's staging buffers, on the stream the displacement runs on
int displace_from(TakeDisplace &s, const double *p, const double *n, bool on_device, double scale, double bias, double *out_p, double *out_n, hipStream_t stream) {
    if (!on_device) {
        HIP_TRY(hipMemcpyAsync(s.base_p.p, p, s.base_p.bytes(), hipMemcpyHostToDevice, stream));
        p = s.base_p.p;
        if (n) {
            HIP_TRY(hipMemcpyAsync(s.base_n.p, n, s.base_n.bytes(), hipMemcpyHostToDevice, stream));
            n = s.base_n.p;
        }
    }
    return displace_on_stream(s, p, n, scale, bias, out_p, out_n, stream);
}

int check_amplitude(double scale, double bias, const std::string &who) {
    if (!displace::finite(scale) || !displace::finite(bias)) return fail(TAKE_E_INVALID, who + "scale and bias must be finite");
    return TAKE_OK;
}

int displace_meshes(TakeScene *ts, const TakeDisplaceBinding *bindings, int32_t n) {
    if (!ts || !bindings) return fail(TAKE_E_INVALID, "null argument");
    if (n <= 0) return fail(TAKE_E_INVALID, "n must be positive");
    std::vector<int32_t> meshes((size_t)n);
    std::vector<const TakeDisplace *> handles((size_t)n);
    std::vector<const TakeSubdiv *> subdivs;
    for (int32_t i = 0; i < n; i++) {
        const TakeDisplaceBinding &b = bindings[i];
        const std::string who = "binding " + std::to_string(i) + ": ";
        if (b.mesh < 0) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        if (!b.displace) return fail(TAKE_E_INVALID, who + "null argument");
        if (b.flags & ~TAKE_DISPLACE_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, who + "unknown flag bits");
        if (int rc = check_amplitude(b.scale, b.bias, who)) return rc;
        if ((b.positions != nullptr) == (b.subdiv != nullptr)) return fail(TAKE_E_INVALID, who + "exactly one of positions and subdiv must be given");
        if (b.subdiv) {
            if (b.normals) return fail(TAKE_E_INVALID, who + "normals cannot be given with subdiv: the direction is the refined surface's");
            if ((b.cage_positions != nullptr) == (b.rig != nullptr)) return fail(TAKE_E_INVALID, who + "exactly one of cage_positions and rig must be given");
            if (b.rig)
                if (int rc = rig_check_pose(b.rig, &b.pose, who)) return rc;
            subdivs.push_back(b.subdiv);
        } else if (b.cage_positions || b.rig) {
            return fail(TAKE_E_INVALID, who + "cage_positions and rig go with subdiv");
        }
        meshes[i] = b.mesh, handles[i] = b.displace;
    }
    std::sort(meshes.begin(), meshes.end());
    std::sort(handles.begin(), handles.end());
    std::sort(subdivs.begin(), subdivs.end());
    for (int32_t i = 1; i < n; i++) {
        if (meshes[i] == meshes[i - 1]) return fail(TAKE_E_INVALID, "mesh " + std::to_string(meshes[i]) + " appears more than once");
        if (handles[i] == handles[i - 1]) return fail(TAKE_E_INVALID, "a displacement handle is bound more than once");
    }
    for (size_t i = 1; i < subdivs.size(); i++)
        if (subdivs[i] == subdivs[i - 1]) return fail(TAKE_E_INVALID, "a subdivision handle is bound more than once");
    const int nd = check_device();
    if (nd < 0) return nd;
    std::vector<TakeMeshUpdate> updates((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const TakeDisplaceBinding &b = bindings[i];
        const std::string who = "binding " + std::to_string(i) + ": ";
        if ((size_t)b.mesh >= ts->mesh_vertices.size()) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        if (b.displace->device != ts->device) return fail(TAKE_E_INVALID, who + "the displacement handle lives on another device than the scene");
        const int64_t mesh_nv = ts->mesh_vertices[b.mesh];
        if (b.subdiv) {
            int device = 0;
            int64_t cage_nv = 0, refined_nv = 0;
            subdiv_shape(b.subdiv, &device, &cage_nv, &refined_nv);
            if (device != ts->device) return fail(TAKE_E_INVALID, who + "the subdivision handle lives on another device than the scene");
            if (b.rig) {
                int64_t nv = 0;
                rig_shape(b.rig, &device, &nv);
                if (device != ts->device) return fail(TAKE_E_INVALID, who + "the rig lives on another device than the scene");
                if (nv != cage_nv) return fail(TAKE_E_INVALID, who + "the rig has " + std::to_string(nv) + " vertices, the cage has " + std::to_string(cage_nv));
            }
            if (refined_nv != b.displace->n_vertices || refined_nv != mesh_nv)
                return fail(TAKE_E_INVALID, who + "the refined cage has " + std::to_string(refined_nv) + " vertices, the displacement handle has " +
                                                std::to_string(b.displace->n_vertices) + ", mesh " + std::to_string(b.mesh) + " has " + std::to_string(mesh_nv));
        } else if (b.displace->n_vertices != mesh_nv) {
            return fail(TAKE_E_INVALID, who + "the displacement handle has " + std::to_string(b.displace->n_vertices) + " vertices, mesh " + std::to_string(b.mesh) + " has " +
                                            std::to_string(mesh_nv));
        }
        const bool normals = on_primary(ts, [&](const auto &sc, const auto &) { return (size_t)b.mesh < sc.host.meshes.size() && sc.host.meshes[b.mesh].nbase >= 0; });
        updates[i] = TakeMeshUpdate{b.mesh, TAKE_MESH_DEVICE_ARRAYS, b.displace->out_p.p, normals ? b.displace->out_n.p : nullptr};
    }
    // the poses, the refines and the displacements, on the default stream as the update: handle-owned memory only, before
    // anything of the scene is staged
    for (int32_t i = 0; i < n; i++) {
        const TakeDisplaceBinding &b = bindings[i];
        TakeDisplace &s = *b.displace;
        const double *p = b.positions, *nrm = b.normals;
        bool on_device = (b.flags & TAKE_DISPLACE_DEVICE_ARRAYS) != 0;
        if (b.subdiv) {
            if (int rc = subdiv_refine_own(b.subdiv, b.cage_positions, on_device, b.rig, &b.pose, true, &p, &nrm)) return rc;
            on_device = true;
        }
        TAKE_ON_DEVICE(ts);
        if (int rc = displace_from(s, p, nrm, on_device, b.scale, b.bias, s.out_p.p, updates[i].normals ? s.out_n.p : nullptr, nullptr)) return rc;
    }
    return take_hip_scene_update_meshes(ts, updates.data(), n);
}

}  // namespace

extern "C" {

int take_hip_displace_create(const TakeDisplaceDesc *desc, TakeDisplace **out) {
    if (!desc || !out) return fail(TAKE_E_INVALID, "null argument");
    try {
        return displace_create(desc, out);
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory for the displacement tables");
    }
}
int take_hip_displace_destroy(TakeDisplace *displace) {
    if (!displace) return fail(TAKE_E_INVALID, "null argument");
    DeviceGuard guard(displace->device);  // (the buffers are freed on the handle's device)
    delete displace;
    return TAKE_OK;
}
int take_hip_displace_info(const TakeDisplace *displace, int64_t *n_vertices, int64_t *n_faces, int32_t *width, int32_t *height, int64_t *device_bytes) {
    if (!displace) return fail(TAKE_E_INVALID, "null argument");
    if (n_vertices) *n_vertices = displace->n_vertices;
    if (n_faces) *n_faces = displace->n_faces;
    if (width) *width = displace->width;
    if (height) *height = displace->height;
    if (device_bytes) *device_bytes = (int64_t)displace->device_bytes();
    return TAKE_OK;
}
int take_hip_displace_apply_device(TakeDisplace *displace, const double *positions, const double *normals, int32_t flags, double scale, double bias, double *d_positions_out,
                                   double *d_normals_out, void *stream) {
    if (!displace || !positions || !d_positions_out) return fail(TAKE_E_INVALID, "null argument");
    if (flags & ~TAKE_DISPLACE_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, "unknown flag bits");
    if (int rc = check_amplitude(scale, bias, "")) return rc;
    // (k_displace and the normal kernels take their inputs and outputs as distinct arrays)
    if (d_positions_out == positions || d_positions_out == normals || d_positions_out == d_normals_out || (d_normals_out && (d_normals_out == positions || d_normals_out == normals)))
        return fail(TAKE_E_INVALID, "an output array is an input: displace into a second array");
    const int nd = check_device();
    if (nd < 0) return nd;
    DeviceGuard guard(displace->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, WRONG_DEVICE);
    return displace_from(*displace, positions, normals, (flags & TAKE_DISPLACE_DEVICE_ARRAYS) != 0, scale, bias, d_positions_out, d_normals_out, (hipStream_t)stream);
}
int take_hip_displace_apply(TakeDisplace *displace, const double *positions, const double *normals, double scale, double bias, double *positions_out, double *normals_out) {
    if (!displace || !positions || !positions_out) return fail(TAKE_E_INVALID, "null argument");
    if (int rc = check_amplitude(scale, bias, "")) return rc;
    const int nd = check_device();
    if (nd < 0) return nd;
    DeviceGuard guard(displace->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, WRONG_DEVICE);
    if (int rc = displace_from(*displace, positions, normals, false, scale, bias, displace->out_p.p, normals_out ? displace->out_n.p : nullptr, nullptr)) return rc;
    HIP_TRY(hipMemcpy(positions_out, displace->out_p.p, displace->out_p.bytes(), hipMemcpyDeviceToHost));
    if (normals_out) HIP_TRY(hipMemcpy(normals_out, displace->out_n.p, displace->out_n.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}
int take_hip_scene_displace_meshes(TakeScene *ts, const TakeDisplaceBinding *bindings, int32_t n) {
    try {
        return displace_meshes(ts, bindings, n);
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while displacing the meshes");
    }
}

}  // extern "C"

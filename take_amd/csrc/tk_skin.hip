// tk_skin.hip — rigs: skinning and morph targets on the device (include/take_hip.h: take_hip_rig_*,
// take_hip_scene_pose_meshes), and the only unit that compiles the kernels of tk_skin.h.  A rig owns
// every buffer a pose touches, so a pose allocates nothing; take_hip_scene_pose_meshes poses into those buffers and
// hands them to take_hip_scene_update_meshes as device arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"
#include "tk_skin.h"

using namespace tk;
using namespace tk_host;

struct TakeRig {
    int device = 0;
    int64_t n_vertices = 0;
    int32_t n_joints = 0, n_influences = 0, n_targets = 0;
    DevBuf<double> rest_p, rest_n, weights, inverse_bind, target_p, target_n;
    DevBuf<int32_t> joints;
    // what a pose writes: the staged pose of a host call (joint_xforms, then target_weights), the palette, the results
    DevBuf<double> pose_in, palette, posed_p, posed_n;
    bool has_normals() const { return rest_n.p != nullptr; }
    size_t device_bytes() const {
        return rest_p.bytes() + rest_n.bytes() + weights.bytes() + inverse_bind.bytes() + target_p.bytes() + target_n.bytes() + joints.bytes() + pose_in.bytes() +
               palette.bytes() + posed_p.bytes() + posed_n.bytes();
    }
    skin::RigView view() const { return {n_vertices, n_joints, n_influences, n_targets, rest_p.p, rest_n.p, joints.p, weights.p, target_p.p, target_n.p}; }
};

namespace {

// a rig array of `count` elements into `dst`: from host or from device memory; null: left empty
template <class T> int take_array(DevBuf<T> &dst, const T *src, size_t count, bool on_device) {
    if (!src) return TAKE_OK;
    if (dst.alloc(count) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the rig");
    HIP_TRY(hipMemcpy(dst.p, src, count * sizeof(T), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return TAKE_OK;
}
int first_not_finite(const char *name, const double *a, size_t count) {
    for (size_t i = 0; a && i < count; i++)
        if (!std::isfinite(a[i])) return fail(TAKE_E_INVALID, std::string(name) + "[" + std::to_string(i) + "] is not finite");
    return TAKE_OK;
}

int rig_create(const TakeRigDesc &d, TakeRig **out) {
    const int32_t K = d.n_influences;
    if (d.n_vertices <= 0) return fail(TAKE_E_INVALID, "n_vertices must be positive");
    if (d.n_joints < 0 || d.n_targets < 0) return fail(TAKE_E_INVALID, "n_joints and n_targets must not be negative");
    if (d.n_joints > 0 && (K < 1 || K > 8)) return fail(TAKE_E_INVALID, "n_influences must be 1..8 for a rig with joints");
    if (d.n_joints == 0 && K != 0) return fail(TAKE_E_INVALID, "n_influences must be 0 for a rig without joints");
    if (!d.positions) return fail(TAKE_E_INVALID, "positions is null");
    if (d.n_joints > 0 && (!d.joints || !d.weights)) return fail(TAKE_E_INVALID, "joints and weights are required for a rig with joints");
    if (d.n_targets > 0 && !d.target_positions) return fail(TAKE_E_INVALID, "target_positions is required for a rig with targets");
    if (d.n_targets > 0 && d.target_normals && !d.normals) return fail(TAKE_E_INVALID, "target_normals given for a rig without normals");
    if (d.flags & ~TAKE_RIG_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, "unknown flag bits");
    const int nd = check_device();
    if (nd < 0) return nd;
    const bool on_device = (d.flags & TAKE_RIG_DEVICE_ARRAYS) != 0;
    const size_t nv = (size_t)d.n_vertices, nj = (size_t)d.n_joints, nt = (size_t)d.n_targets;
    if (!on_device) {
        for (size_t i = 0; i < nv * (size_t)K; i++)
            if (d.joints[i] < 0 || d.joints[i] >= d.n_joints)
                return fail(TAKE_E_INVALID, "vertex " + std::to_string(i / (size_t)K) + ": joint index " + std::to_string(d.joints[i]) + " out of range");
        if (int rc = first_not_finite("positions", d.positions, 3 * nv)) return rc;
        if (int rc = first_not_finite("normals", d.normals, 3 * nv)) return rc;
        if (int rc = first_not_finite("weights", nj ? d.weights : nullptr, nv * (size_t)K)) return rc;
        if (int rc = first_not_finite("inverse_bind", nj ? d.inverse_bind : nullptr, 12 * nj)) return rc;
        if (int rc = first_not_finite("target_positions", nt ? d.target_positions : nullptr, 3 * nt * nv)) return rc;
        if (int rc = first_not_finite("target_normals", nt ? d.target_normals : nullptr, 3 * nt * nv)) return rc;
    }
    TakeRig *rig = new TakeRig();
    struct Drop {
        TakeRig *r;
        ~Drop() { delete r; }
    } drop{rig};
    HIP_TRY(hipGetDevice(&rig->device));
    rig->n_vertices = d.n_vertices, rig->n_joints = d.n_joints, rig->n_influences = K, rig->n_targets = d.n_targets;
    if (int rc = take_array(rig->rest_p, d.positions, 3 * nv, on_device)) return rc;
    if (int rc = take_array(rig->rest_n, d.normals, 3 * nv, on_device)) return rc;
    if (nj) {
        if (int rc = take_array(rig->joints, d.joints, nv * (size_t)K, on_device)) return rc;
        if (int rc = take_array(rig->weights, d.weights, nv * (size_t)K, on_device)) return rc;
        if (int rc = take_array(rig->inverse_bind, d.inverse_bind, 12 * nj, on_device)) return rc;
    }
    if (nt) {
        if (int rc = take_array(rig->target_p, d.target_positions, 3 * nt * nv, on_device)) return rc;
        if (int rc = take_array(rig->target_n, d.target_normals, 3 * nt * nv, on_device)) return rc;
    }
    if (rig->pose_in.alloc(12 * nj + nt) != hipSuccess || rig->palette.alloc(12 * nj) != hipSuccess || rig->posed_p.alloc(3 * nv) != hipSuccess ||
        (d.normals && rig->posed_n.alloc(3 * nv) != hipSuccess))
        return fail(TAKE_E_NOMEM, "out of device memory for the rig");
    if (on_device && nj) {
        DevBuf<unsigned long long> bad;
        if (bad.alloc(1) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the rig");
        HIP_TRY(hipMemset(bad.p, 0xff, sizeof(unsigned long long)));
        hipLaunchKernelGGL(skin::k_skin_check_joints, dim3((unsigned)skin::blocks_for(d.n_vertices)), dim3(skin::BLOCK), 0, nullptr, (const int32_t *)rig->joints.p, K,
                           d.n_joints, d.n_vertices, bad.p);
        HIP_TRY(hipGetLastError());
        unsigned long long first = 0;
        HIP_TRY(hipMemcpy(&first, bad.p, sizeof first, hipMemcpyDeviceToHost));
        if (first != ~0ull) return fail(TAKE_E_INVALID, "vertex " + std::to_string(first) + ": joint index out of range");
    }
    drop.r = nullptr;
    *out = rig;
    return TAKE_OK;
}

// what a pose call refuses without a device: the rig's counts are host memory of a handle that exists
int check_pose_args(const TakeRig *rig, const TakeRigPose *pose, const std::string &who) {
    if (!rig || !pose) return fail(TAKE_E_INVALID, who + "null argument");
    if (pose->flags & ~TAKE_RIG_POSE_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, who + "unknown flag bits");
    if (rig->n_joints > 0 && !pose->joint_xforms) return fail(TAKE_E_INVALID, who + "joint_xforms is required for a rig with joints");
    if (rig->n_targets > 0 && !pose->target_weights) return fail(TAKE_E_INVALID, who + "target_weights is required for a rig with targets");
    return TAKE_OK;
}

// The palette, then every vertex, on `stream`; the rig's device is current.  out_n null: no normals are computed.
// Allocates nothing.  TAKE_HIP_VERBOSE=1: both kernels between events, printed to stderr once they have completed.
int pose_on_stream(TakeRig &rig, const TakeRigPose &pose, double *out_p, double *out_n, hipStream_t stream) {
    const size_t nj = (size_t)rig.n_joints, nt = (size_t)rig.n_targets;
    const double *d_x = pose.joint_xforms, *d_w = pose.target_weights;
    if (!(pose.flags & TAKE_RIG_POSE_DEVICE_ARRAYS)) {
        if (nj) HIP_TRY(hipMemcpyAsync(rig.pose_in.p, pose.joint_xforms, 12 * nj * sizeof(double), hipMemcpyHostToDevice, stream));
        if (nt) HIP_TRY(hipMemcpyAsync(rig.pose_in.p + 12 * nj, pose.target_weights, nt * sizeof(double), hipMemcpyHostToDevice, stream));
        d_x = rig.pose_in.p, d_w = rig.pose_in.p + 12 * nj;
    }
    EventPool events;
    hipEvent_t ev[3] = {};
    if (std::getenv("TAKE_HIP_VERBOSE"))
        for (hipEvent_t &e : ev) e = events.get();
    const bool clocked = ev[0] && ev[1] && ev[2];
    if (clocked) (void)hipEventRecord(ev[0], stream);
    if (nj)
        hipLaunchKernelGGL(skin::k_skin_palette, dim3((unsigned)skin::blocks_for(rig.n_joints)), dim3(skin::BLOCK), 0, stream, d_x, (const double *)rig.inverse_bind.p,
                           rig.palette.p, (int64_t)rig.n_joints);
    if (clocked) (void)hipEventRecord(ev[1], stream);
    const dim3 grid((unsigned)skin::blocks_for(rig.n_vertices)), block(skin::BLOCK);
    const bool staged = nj > 0 && rig.n_joints <= skin::LDS_MAX_JOINTS;  // (the block's copy of the palette in LDS: DESIGN.md §4q)
    if (staged)
        hipLaunchKernelGGL(skin::k_skin_pose<true>, grid, block, 0, stream, rig.view(), (const double *)rig.palette.p, d_w, out_p, out_n);
    else
        hipLaunchKernelGGL(skin::k_skin_pose<false>, grid, block, 0, stream, rig.view(), (const double *)rig.palette.p, d_w, out_p, out_n);
    if (clocked) (void)hipEventRecord(ev[2], stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    float ms[2] = {0, 0};
    if (clocked && hipEventElapsedTime(&ms[0], ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&ms[1], ev[1], ev[2]) == hipSuccess) {
        std::fprintf(stderr, "[take_hip] rig_pose: k_skin_palette %d joints %8.3f ms\n", rig.n_joints, ms[0]);
        std::fprintf(stderr, "[take_hip] rig_pose: k_skin_pose%s %lld vertices K %d T %d %s %9.4f ms\n", staged ? "<lds>" : "<global>", (long long)rig.n_vertices,
                     rig.n_influences, rig.n_targets, out_n ? "normals" : "positions", ms[1]);
    }
    return TAKE_OK;
}

int pose_meshes(TakeScene *ts, const TakeRigBinding *bindings, int32_t n) {
    if (!ts || !bindings) return fail(TAKE_E_INVALID, "null argument");
    if (n <= 0) return fail(TAKE_E_INVALID, "n must be positive");
    std::vector<int32_t> meshes((size_t)n);
    std::vector<const TakeRig *> rigs((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const std::string who = "binding " + std::to_string(i) + ": ";
        if (bindings[i].mesh < 0) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        if (int rc = check_pose_args(bindings[i].rig, &bindings[i].pose, who)) return rc;
        meshes[i] = bindings[i].mesh, rigs[i] = bindings[i].rig;
    }
    std::sort(meshes.begin(), meshes.end());
    std::sort(rigs.begin(), rigs.end());
    for (int32_t i = 1; i < n; i++) {
        if (meshes[i] == meshes[i - 1]) return fail(TAKE_E_INVALID, "mesh " + std::to_string(meshes[i]) + " appears more than once");
        if (rigs[i] == rigs[i - 1]) return fail(TAKE_E_INVALID, "a rig is bound more than once");
    }
    const int nd = check_device();
    if (nd < 0) return nd;
    std::vector<TakeMeshUpdate> updates((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const TakeRigBinding &b = bindings[i];
        const std::string who = "binding " + std::to_string(i) + ": ";
        if ((size_t)b.mesh >= ts->mesh_vertices.size()) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        if (b.rig->device != ts->device) return fail(TAKE_E_INVALID, who + "the rig lives on another device than the scene");
        if (b.rig->n_vertices != ts->mesh_vertices[b.mesh])
            return fail(TAKE_E_INVALID, who + "the rig has " + std::to_string(b.rig->n_vertices) + " vertices, mesh " + std::to_string(b.mesh) + " has " +
                                            std::to_string(ts->mesh_vertices[b.mesh]));
        const bool mesh_normals = on_primary(ts, [&](const auto &sc, const auto &) { return (size_t)b.mesh < sc.host.meshes.size() && sc.host.meshes[b.mesh].nbase >= 0; });
        const bool normals = mesh_normals && b.rig->has_normals();
        updates[i] = TakeMeshUpdate{b.mesh, TAKE_MESH_DEVICE_ARRAYS, b.rig->posed_p.p, normals ? b.rig->posed_n.p : nullptr};
    }
    {  // the poses, on the default stream as the update: rig-owned memory only, before anything of the scene is staged
        TAKE_ON_DEVICE(ts);
        for (int32_t i = 0; i < n; i++) {
            TakeRig &rig = *bindings[i].rig;
            if (int rc = pose_on_stream(rig, bindings[i].pose, rig.posed_p.p, updates[i].normals ? rig.posed_n.p : nullptr, nullptr)) return rc;
        }
    }
    return take_hip_scene_update_meshes(ts, updates.data(), n);
}

}  // namespace

// what tk_subdiv.hip needs of a rig it is bound with (declared in tk_host.h)
namespace tk_host {
int rig_check_pose(const TakeRig *rig, const TakeRigPose *pose, const std::string &who) { return check_pose_args(rig, pose, who); }
void rig_shape(const TakeRig *rig, int *device, int64_t *n_vertices) { *device = rig->device, *n_vertices = rig->n_vertices; }
}  // namespace tk_host

extern "C" {

int take_hip_rig_create(const TakeRigDesc *desc, TakeRig **out) {
    if (!desc || !out) return fail(TAKE_E_INVALID, "null argument");
    try {
        return rig_create(*desc, out);
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory for the rig");
    }
}
int take_hip_rig_destroy(TakeRig *rig) {
    if (!rig) return fail(TAKE_E_INVALID, "null argument");
    DeviceGuard guard(rig->device);  // (the buffers are freed on the rig's device)
    delete rig;
    return TAKE_OK;
}
int take_hip_rig_info(const TakeRig *rig, int64_t *n_vertices, int32_t *n_joints, int32_t *n_influences, int32_t *n_targets, int32_t *has_normals, int64_t *device_bytes) {
    if (!rig) return fail(TAKE_E_INVALID, "null argument");
    if (n_vertices) *n_vertices = rig->n_vertices;
    if (n_joints) *n_joints = rig->n_joints;
    if (n_influences) *n_influences = rig->n_influences;
    if (n_targets) *n_targets = rig->n_targets;
    if (has_normals) *has_normals = rig->has_normals() ? 1 : 0;
    if (device_bytes) *device_bytes = (int64_t)rig->device_bytes();
    return TAKE_OK;
}
int take_hip_rig_pose_device(TakeRig *rig, const TakeRigPose *pose, double *d_positions_out, double *d_normals_out, void *stream) {
    if (int rc = check_pose_args(rig, pose, "")) return rc;
    if (!d_positions_out) return fail(TAKE_E_INVALID, "null argument");
    if (d_normals_out && !rig->has_normals()) return fail(TAKE_E_INVALID, "normals wanted from a rig without normals");
    const int nd = check_device();
    if (nd < 0) return nd;
    DeviceGuard guard(rig->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the rig's device current");
    return pose_on_stream(*rig, *pose, d_positions_out, d_normals_out, (hipStream_t)stream);
}
int take_hip_rig_pose(TakeRig *rig, const TakeRigPose *pose, double *positions_out, double *normals_out) {
    if (int rc = check_pose_args(rig, pose, "")) return rc;
    if (!positions_out) return fail(TAKE_E_INVALID, "null argument");
    if (normals_out && !rig->has_normals()) return fail(TAKE_E_INVALID, "normals wanted from a rig without normals");
    const int nd = check_device();
    if (nd < 0) return nd;
    DeviceGuard guard(rig->device);
    if (!guard.ok) return fail(TAKE_E_DEVICE, "cannot make the rig's device current");
    if (int rc = pose_on_stream(*rig, *pose, rig->posed_p.p, normals_out ? rig->posed_n.p : nullptr, nullptr)) return rc;
    HIP_TRY(hipMemcpy(positions_out, rig->posed_p.p, rig->posed_p.bytes(), hipMemcpyDeviceToHost));
    if (normals_out) HIP_TRY(hipMemcpy(normals_out, rig->posed_n.p, rig->posed_n.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}
int take_hip_scene_pose_meshes(TakeScene *ts, const TakeRigBinding *bindings, int32_t n) {
    try {
        return pose_meshes(ts, bindings, n);
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while posing the meshes");
    }
}

}  // extern "C"

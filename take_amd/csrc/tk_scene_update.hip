// tk_scene_update.hip — the C entry points of include/take_hip.h that change a scene which is already on the device: new
// transforms for its placements, new vertices for its meshes, camera and lens, the marked frame and vertex tracking, and
// the render over a shutter, which changes the scene slice by slice and puts it back.  Launches no kernel, as tk_api.hip
// (the entry points that render and trace): the drivers that stage a change are tk_build.hip's, the shutter's kernels
// and the render tk_render.hip's, reached through tk_scene_handle.h.  Arguments are looked at before a device is looked for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "take_hip.h"
#include "tk_scene_handle.h"

using namespace tk;
using namespace tk_host;

namespace {
// what take_hip_scene_set_instance_transforms accepts, checked before anything is read or made
int check_repose(const TakeScene *ts, int64_t n) {
    if (ts->n_placements <= 0) return fail(TAKE_E_INVALID, "the scene has no placements (none were given, or TAKE_INSTANCES_FLATTEN expanded them)");
    if (n != ts->n_placements) return fail(TAKE_E_INVALID, "n = " + std::to_string(n) + ", but the scene has " + std::to_string(ts->n_placements) + " placements");
    const bool plain = on_primary(ts, [&](const auto &sc, const auto &) {
        return sc.trace.two_level && sc.trace.nodes != NodeFormat::Q8 && (int64_t)sc.inst_trace.n == n && (int64_t)sc.host.placements.inst_proto.size() == n;
    });
    if (!plain) return fail(TAKE_E_INVALID, "unsupported: the scene was built under TAKE_HIP_BRAID > 1 or TAKE_HIP_NODES=q8");
    return TAKE_OK;
}
// New transforms for all placements of ts, from host or device memory (kind).  The scene gets a copy it can keep — the
// caller's memory stays the caller's — and a successful call keeps it: the scene's current transforms from then on
// (TakeScene::xforms).  The build runs on the default stream, as scene_create's does: first whatever `stream` still has
// to write into the caller's array.
int set_instance_transforms(TakeScene *ts, const double *src, int64_t n, hipMemcpyKind kind, void *stream) {
    if (!ts || !src) return fail(TAKE_E_INVALID, "null argument");
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    if (const int rc = check_repose(ts, n)) return rc;
    if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    DevBuf<double> xforms;
    if (xforms.alloc(12 * (size_t)n) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the transforms");
    HIP_TRY(hipMemcpy(xforms.p, src, xforms.bytes(), kind));
    try {
        const int rc = stage_then_commit<ReposeStage>(ts, [&](const auto &sc, auto &stage) { return repose_two_level_device(sc, xforms.p, n, stage); });
        if (!rc) ts->xforms = std::move(xforms);
        return rc;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while re-posing the placements");
    }
}
// a two-level scene holds its placements' current transforms itself (a replica of a scene group does not)
bool has_own_transforms(const TakeScene *ts) { return ts->xforms.p && (int64_t)ts->xforms.n == 12 * ts->n_placements; }

// ---- a list of meshes with new arrays — the updates ("update i: "), the motions of take_hip_render_shutter_meshes*
// ("motion i: ") — looked at in two steps with check_device between them.  item(i) -> what both steps read of entry i.
struct MeshItem {
    int32_t mesh, flags;
    const char *arrays;  // what is wrong with the arrays the entry has to bring, or null
    bool normals;        // it brings vertex normals
};
auto update_item(const TakeMeshUpdate *u) {
    return [u](int32_t i) { return MeshItem{u[i].mesh, u[i].flags, u[i].positions ? nullptr : "positions is null", u[i].normals != nullptr}; };
}
auto motion_item(const TakeMeshMotion *m) {
    return [m](int32_t i) {
        const char *arrays = !m[i].positions0 || !m[i].positions1 ? "positions0 or positions1 is null"
                                                                   : (!m[i].normals0 != !m[i].normals1 ? "normals0 and normals1 must be given together" : nullptr);
        return MeshItem{m[i].mesh, m[i].flags, arrays, m[i].normals0 != nullptr};
    };
}
// what needs no scene: an index >= 0, known flag bits, the required arrays, no mesh twice
template <class Item> int check_mesh_list(const char *what, int32_t n, Item item) {
    std::vector<int32_t> ids((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const MeshItem m = item(i);
        const std::string who = what + std::to_string(i) + ": ";
        if (m.mesh < 0) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        if (m.flags & ~TAKE_MESH_DEVICE_ARRAYS) return fail(TAKE_E_INVALID, who + "unknown flag bits");
        if (m.arrays) return fail(TAKE_E_INVALID, who + m.arrays);
        ids[i] = m.mesh;
    }
    std::sort(ids.begin(), ids.end());
    for (int32_t i = 1; i < n; i++)
        if (ids[i] == ids[i - 1]) return fail(TAKE_E_INVALID, "mesh " + std::to_string(ids[i]) + " appears more than once");
    return TAKE_OK;
}
// what needs the scene: an index the scene has, normals only for a mesh that has vertex normals
template <class Item> int check_mesh_list_in_scene(const TakeScene *ts, const char *what, int32_t n, Item item) {
    for (int32_t i = 0; i < n; i++) {
        const MeshItem m = item(i);
        const std::string who = what + std::to_string(i) + ": ";
        if ((size_t)m.mesh >= ts->mesh_vertices.size()) return fail(TAKE_E_INVALID, who + "mesh index out of range");
        const bool has = on_primary(ts, [&](const auto &sc, const auto &) { return (size_t)m.mesh < sc.host.meshes.size() && sc.host.meshes[m.mesh].nbase >= 0; });
        if (m.normals && !has) return fail(TAKE_E_INVALID, who + "normals given for a mesh without vertex normals");
    }
    return TAKE_OK;
}

// ---- new vertices for meshes of a resident scene (include/take_hip.h).  What the update does not support of a scene,
// in its words (take_hip_render_shutter_meshes* refuses the same); two_level_too: take_hip_scene_update_meshes — a scene
// with placements takes update_two_level_meshes_device, any other scene the one path both symbols share
int check_update_scene(const TakeScene *ts, bool two_level_too) {
    const bool two_level = ts->n_placements > 0;
    if (two_level && !two_level_too) return fail(TAKE_E_INVALID, "unsupported: a two-level scene (take_hip_scene_update_meshes moves the vertices of its meshes)");
    if (ts->flattened) return fail(TAKE_E_INVALID, "unsupported: the scene was flattened from instances");
    const bool q8 = ts->node_knob == "q8" || on_primary(ts, [&](const auto &sc, const auto &) { return sc.trace.nodes == NodeFormat::Q8; });
    if (q8) return fail(TAKE_E_INVALID, "unsupported: the scene was built under TAKE_HIP_NODES=q8");
    if (two_level) {
        if (const int rc = check_repose(ts, ts->n_placements)) return rc;  // (TAKE_HIP_BRAID > 1: "unsupported")
        if (!has_own_transforms(ts)) return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group");
        if (on_primary(ts, [&](const auto &sc, const auto &) { return (int64_t)sc.prims.n - sc.host.blas_prims != (int64_t)ts->shape_face.n; }))
            return fail(TAKE_E_INVALID, "unsupported: the scene does not have one primitive record per shape");
    } else {
        if (on_primary(ts, [&](const auto &sc, const auto &) { return sc.trace.two_level; })) return fail(TAKE_E_INVALID, "unsupported: a two-level scene");
        if (!ts->shape_face.p) return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group, or has no shapes");
        if (on_primary(ts, [&](const auto &sc, const auto &) { return sc.prims.n != ts->shape_face.n; }))
            return fail(TAKE_E_INVALID, "unsupported: the scene does not have one primitive record per shape");
    }
    return TAKE_OK;
}
// The core of an update (check_update_scene passed): every side staged from `in`, then every side committed.  A scene
// with placements gets its top level under d_xforms; new_records: they are not the transforms its placement records
// were made from (a slice of take_hip_render_shutter_meshes*), which are made again with it.  The mark, vertex tracking
// and the current transforms are the caller's business.
int commit_mesh_update(TakeScene *ts, const MeshUpdateInputs &in, const double *d_xforms, bool new_records) {
    if (ts->n_placements > 0)
        return stage_then_commit<ProtoUpdateStage>(ts, [&](const auto &sc, auto &stage) {
            return update_two_level_meshes_device(sc, in, ts->mesh_vertices, ts->shape_face.p, d_xforms, ts->max_leaf, new_records, stage);
        });
    const bool compressed_ok = compressed_nodes_supported() && ts->node_knob != "wide", compressed_forced = ts->node_knob == "q16";
    return stage_then_commit<MeshUpdateStage>(ts, [&](const auto &sc, auto &stage) {
        return update_mesh_vertices_device(sc, in, ts->mesh_vertices, ts->shape_face.p, ts->max_leaf, compressed_ok, compressed_forced, ts->num_cus, stage);
    });
}
// The public symbols: the arguments that need no scene, the device, the arguments against the scene, the scene, the core, the mark's bookkeeping
int update_meshes(TakeScene *ts, const TakeMeshUpdate *updates, int32_t n_updates, bool two_level_too) {
    if (!ts || !updates) return fail(TAKE_E_INVALID, "null argument");
    if (n_updates <= 0) return fail(TAKE_E_INVALID, "n_updates must be positive");
    try {
        if (const int rc = check_mesh_list("update ", n_updates, update_item(updates))) return rc;
        if (const int nd = check_device(); nd < 0) return nd;
        if (const int rc = check_mesh_list_in_scene(ts, "update ", n_updates, update_item(updates))) return rc;
        if (const int rc = check_update_scene(ts, two_level_too)) return rc;
        TAKE_ON_DEVICE(ts);
        MeshUpdateInputs in;
        int rc = in.upload(ts->mesh_vertices, updates, n_updates);
        if (rc) return rc;
        // take_hip_scene_track_vertices: the first update after a mark keeps the geometry words of the primary side's
        // records as they are now — staged with the update, and the handle's only when every side committed
        TakeScene::FrameMark kept;
        const bool keep = ts->track_flags && ts->mark.set && !ts->mark.updated && !ts->mark.has_geometry();
        if (keep) {
            rc = ts->f64() ? copy_marked_geometry(ts->d, kept.geom_d, kept.inst_first) : copy_marked_geometry(ts->f, kept.geom_f, kept.inst_first);
            if (rc) return rc;
        }
        rc = commit_mesh_update(ts, in, ts->xforms.p, false);
        if (rc) return rc;
        ts->mark.updated = true;
        if (keep) ts->mark.geom_f = std::move(kept.geom_f), ts->mark.geom_d = std::move(kept.geom_d), ts->mark.inst_first = std::move(kept.inst_first);
        return TAKE_OK;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while updating the meshes");
    } catch (const std::exception &e) {
        return fail(TAKE_E_INVALID, std::string("updating the meshes failed: ") + e.what());
    }
}

// every side's camera record from `cam`, lens members kept (make_camera leaves its two members alone; nothing else of the handle)
void pose_camera(TakeScene *ts, const TakeCamera &cam) {
    for_each_side(ts, [&](auto &sc) { return make_camera(cam, sc.host.cam), sc.dev.cam = sc.host.cam, TAKE_OK; });
}
// the lens of the handle (ts->lens, ts->lens_focus) -> every side's camera record, each value rounded to Real once;
// radius 0 is the pinhole camera, whose record holds zeros there
void apply_lens(TakeScene *ts) {
    const bool on = ts->lens.aperture_radius > 0;
    for_each_side(ts, [&](auto &sc) {
        using R = std::remove_reference_t<decltype(sc.host.cam.focus)>;
        sc.host.cam.lens_radius = on ? R(ts->lens.aperture_radius) : R(0), sc.host.cam.focus = on ? R(ts->lens_focus) : R(0);
        sc.dev.cam = sc.host.cam;
        return TAKE_OK;
    });
}
// > 0, and still finite where the scene has an f32 side
bool lens_focus_usable(const TakeScene *ts, double focus) {
    return focus > 0 && std::isfinite(focus) && (ts->precision == TAKE_PRECISION_F64 || ((float)focus > 0 && std::isfinite((float)focus)));
}

// ---- motion blur.  A render over a shutter between the marked and the current frame (include/take_hip.h; DESIGN.md
// §4l): the plan, the pose at a time (tk_shutter.h; launched by tk_render.hip's shutter_pose_device) and the loop over
// the slices, which re-poses through set_instance_transforms' own path and renders through take_hip_render_accumulate's.
// With deforming meshes (take_hip_render_shutter_meshes*) the same loop also lerps their vertices per
// slice (tk_shutter.h: k_shutter_vertices; tk_render.hip: shutter_vertices_launch) and takes them in through commit_mesh_update.
int check_shutter(const TakeShutter &s) {
    if (!std::isfinite(s.open) || !std::isfinite(s.close) || !(0.0 <= s.open && s.open <= s.close && s.close <= 1.0))
        return fail(TAKE_E_INVALID, "the shutter must have 0 <= open <= close <= 1");
    if (s.flags != 0) return fail(TAKE_E_INVALID, "unknown flag bits");
    return TAKE_OK;
}
// what the shutter needs of the scene: a mark, and — with placements — what the re-pose accepts and both sets of transforms
int check_shutter_scene(const TakeScene *ts) {
    if (!ts->mark.set) return fail(TAKE_E_INVALID, "no marked frame: take_hip_scene_mark_frame has not been called on this scene");
    if (ts->n_placements <= 0) return TAKE_OK;
    if (const int rc = check_repose(ts, ts->n_placements)) return rc;
    if (!has_own_transforms(ts) || (int64_t)ts->mark.xforms.n != 12 * ts->n_placements) return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group");
    return TAKE_OK;
}
// The poses at the times of the slices (check_shutter_scene passed), looked at before anything is rendered: the cameras
// on the host, then — with placements, and if wanted — their transforms on the device (posed, moved: shutter_pose_device's)
int shutter_poses(const TakeScene *ts, const std::vector<double> &time, bool transforms, std::vector<TakeCamera> &cams, DevBuf<double> &posed, std::vector<int> &moved) {
    for (size_t k = 0; k < time.size(); k++) {
        const TakeCamera c = shutter_camera(ts->mark.camera, ts->camera, time[k]);
        bool finite = std::isfinite(c.vfov), apart = false;
        for (int a = 0; a < 3; a++) finite = finite && std::isfinite(c.lookfrom[a]) && std::isfinite(c.lookat[a]) && std::isfinite(c.up[a]), apart = apart || c.lookfrom[a] != c.lookat[a];
        if (!finite || !apart) return fail(TAKE_E_INVALID, "slice " + std::to_string(k) + ": the interpolated camera is not finite, or its lookat coincides with its lookfrom");
        cams.push_back(c);
    }
    const int64_t n = ts->n_placements;
    int64_t first_bad = -1;
    if (!transforms || n <= 0) return TAKE_OK;
    if (const int rc = shutter_pose_device(ts->mark.xforms.p, ts->xforms.p, time, n, posed, first_bad, moved)) return rc;
    if (first_bad < 0) return TAKE_OK;
    return fail(TAKE_E_INVALID, "slice " + std::to_string(first_bad / n) + ": instance " + std::to_string(first_bad % n) + ": singular or non-finite transform");
}
// The deforming meshes of a render over the shutter, in device memory: per array of a motion its two ends (host arrays
// uploaded once, device arrays borrowed) and the buffer the slices' vertices are made in; the update's inputs over
// those buffers — the same for every slice — and over the current ends, which put the scene back.
struct SliceMeshes {
    struct Array {
        const double *a, *b;
        double *out;
        int64_t n;
    };
    std::vector<DevBuf<double>> owned;
    std::vector<Array> arrays;
    MeshUpdateInputs slice, current;
    DevBuf<int> moved;
    int make(const TakeScene *ts, const TakeMeshMotion *motions, int32_t n) {
        const char *nomem = "out of device memory for the meshes' vertices over the shutter";
        std::vector<TakeMeshUpdate> to_slice((size_t)n), to_current((size_t)n);
        auto resident = [&](const double *src, bool device, size_t words, const double *&dst) {
            if (device) return dst = src, (int)TAKE_OK;
            owned.emplace_back();
            if (owned.back().alloc(std::max<size_t>(words, 1)) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
            if (words) HIP_TRY(hipMemcpy(owned.back().p, src, words * sizeof(double), hipMemcpyHostToDevice));
            return dst = owned.back().p, (int)TAKE_OK;
        };
        for (int32_t i = 0; i < n; i++) {
            const TakeMeshMotion &m = motions[i];
            const size_t words = 3 * (size_t)ts->mesh_vertices[m.mesh];
            const bool device = (m.flags & TAKE_MESH_DEVICE_ARRAYS) != 0;
            const double *ends[2][2] = {{m.positions0, m.positions1}, {m.normals0, m.normals1}};
            const double *out[2] = {nullptr, nullptr}, *now[2] = {nullptr, nullptr};
            for (int k = 0; k < 2; k++) {
                if (!ends[k][0]) continue;
                Array arr{nullptr, nullptr, nullptr, (int64_t)words};
                if (const int rc = resident(ends[k][0], device, words, arr.a)) return rc;
                if (const int rc = resident(ends[k][1], device, words, arr.b)) return rc;
                owned.emplace_back();
                if (owned.back().alloc(std::max<size_t>(words, 1)) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
                arr.out = owned.back().p, out[k] = arr.out, now[k] = arr.b;
                arrays.push_back(arr);
            }
            to_slice[i] = TakeMeshUpdate{m.mesh, TAKE_MESH_DEVICE_ARRAYS, out[0], out[1]};
            to_current[i] = TakeMeshUpdate{m.mesh, TAKE_MESH_DEVICE_ARRAYS, now[0], now[1]};
        }
        if (moved.alloc(1) != hipSuccess) return fail(TAKE_E_NOMEM, nomem);
        if (const int rc = slice.upload(ts->mesh_vertices, to_slice.data(), n)) return rc;
        return current.upload(ts->mesh_vertices, to_current.data(), n);
    }
    // every array at time t -> its buffer (the default stream, as the update that reads them next); any: some vertex is
    // not the current one bit for bit
    int lerp(double t, int num_cus, bool &any) {
        HIP_TRY(hipMemsetAsync(moved.p, 0, sizeof(int), nullptr));
        for (const Array &x : arrays) shutter_vertices_launch(x.a, x.b, x.n, t, x.out, moved.p, num_cus, nullptr);
        HIP_TRY(hipGetLastError());
        int flag = 0;
        HIP_TRY(hipMemcpy(&flag, moved.p, sizeof(int), hipMemcpyDeviceToHost));
        any = flag != 0;
        return TAKE_OK;
    }
};
// What a render over the shutter refuses of its arguments before a device is looked for; out: where the image goes
int check_shutter_call(const TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n_motions, const void *out) {
    if (!ts || !opts || !out) return fail(TAKE_E_INVALID, "null argument");
    int32_t K = 0;
    if (int rc = take_hip_shutter_plan(opts->spp, shutter, &K, nullptr, nullptr)) return rc;
    if (n_motions < 0) return fail(TAKE_E_INVALID, "n must not be negative");
    if (n_motions > 0 && !motions) return fail(TAKE_E_INVALID, "null argument");
    try {
        return check_mesh_list("motion ", n_motions, motion_item(motions));
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while rendering over the shutter");
    }
}
// The one loop over the slices (check_shutter_call passed), into device memory; n_motions = 0: take_hip_render_shutter*
int render_over_shutter(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n_motions, void *d_rgb_out,
                        void *stream) {
    try {
        if (const int nd = check_device(); nd < 0) return nd;
        TAKE_ON_DEVICE(ts);
        if (const int rc = check_mesh_list_in_scene(ts, "motion ", n_motions, motion_item(motions))) return rc;
        if (const int rc = check_shutter_scene(ts)) return rc;
        if (const int rc = n_motions > 0 ? check_update_scene(ts, true) : (int)TAKE_OK) return rc;
        int32_t K = 0;
        take_hip_shutter_plan(opts->spp, shutter, &K, nullptr, nullptr);
        std::vector<int32_t> first((size_t)K + 1);
        std::vector<double> time((size_t)K);
        take_hip_shutter_plan(opts->spp, shutter, &K, first.data(), time.data());
        const int64_t n = ts->n_placements;
        std::vector<TakeCamera> cams;
        DevBuf<double> posed;
        std::vector<int> moved;
        if (const int rc = shutter_poses(ts, time, true, cams, posed, moved)) return rc;
        // the deforming meshes: both ends and the slices' buffers in device memory before the first slice (the default
        // stream reads them: first whatever `stream` still has to write into device arrays)
        SliceMeshes meshes;
        if (n_motions > 0) {
            if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
            if (const int rc = meshes.make(ts, motions, n_motions)) return rc;
        }
        // the slices; whatever happens from here on, the scene goes back to its current pose.  `at`: the transforms the
        // placements are under — a slice whose pose is the current transforms bit for bit is rendered under those, and
        // placements that did not move since the mark are never re-posed at all.  `deformed`: the meshes are not at
        // their current vertices — a slice whose vertices are the current ones bit for bit, in a scene that is at them,
        // runs no update, and one that runs it makes the placements' records and the top level for its pose with it
        const bool restart_needed = ts->acc_restart_needed;  // (a re-pose sets it; a one-shot render leaves it alone, and so does this call)
        const double *at = ts->xforms.p;
        bool deformed = false, updated = false;
        auto repose_to = [&](const double *x) {
            if (x == at) return (int)TAKE_OK;
            const int rc = stage_then_commit<ReposeStage>(ts, [&](const auto &sc, auto &stage) { return repose_two_level_device(sc, x, n, stage); });
            if (!rc) at = x;
            return rc;
        };
        auto update_to = [&](const MeshUpdateInputs &in, const double *x, bool now_deformed) {
            const int rc = commit_mesh_update(ts, in, x, x != at);
            if (!rc) at = x, deformed = now_deformed, updated = true;
            return rc;
        };
        int rc = TAKE_OK;
        for (int32_t k = 0; k < K && !rc; k++) {
            pose_camera(ts, cams[k]);
            const double *x = n > 0 && moved[k] ? posed.p + 12 * n * (int64_t)k : ts->xforms.p;
            bool any = false;
            if (n_motions > 0) rc = meshes.lerp(time[k], ts->num_cus, any);
            if (!rc && (any || deformed)) {
                rc = update_to(meshes.slice, x, any);
                if (rc) rc = fail(rc, "slice " + std::to_string(k) + ": " + g_error);
            } else if (!rc && n > 0) {
                rc = repose_to(x);
            }
            TakeRenderOpts o = *opts;
            o.spp = first[k + 1] - first[k];
            if (!rc) rc = render_scene(ts, o, d_rgb_out, (hipStream_t)stream, first[k], k > 0, k + 1 == K);
        }
        const std::string why = g_error;
        pose_camera(ts, ts->camera);
        const int back = updated ? update_to(meshes.current, ts->xforms.p, false) : (n > 0 ? repose_to(ts->xforms.p) : (int)TAKE_OK);
        ts->acc_samples = 0, ts->acc_restart_needed = restart_needed || back != TAKE_OK;
        if (rc) return fail(rc, why);
        if (back) return fail(back, "the render is complete, but putting the scene back at its current pose failed: " + g_error);
        return TAKE_OK;
    } catch (const std::bad_alloc &) {
        return fail(TAKE_E_NOMEM, "out of host memory while rendering over the shutter");
    }
}
int render_shutter_to_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n_motions, void *d_rgb_out,
                             void *stream) {
    const int rc = check_shutter_call(ts, opts, shutter, motions, n_motions, d_rgb_out);
    return rc ? rc : render_over_shutter(ts, opts, shutter, motions, n_motions, d_rgb_out, stream);
}
// the host entries: the image in device memory, then copied out
int render_shutter_to_host(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n_motions, void *rgb_out_host) {
    if (int rc = check_shutter_call(ts, opts, shutter, motions, n_motions, rgb_out_host)) return rc;
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    StripSet s;
    if (int rc = strip_set(ts, *opts, s)) return rc;
    const size_t bytes = (size_t)s.npix * 3 * (ts->f64() ? 8 : 4);
    if (bytes == 0) return TAKE_OK;
    DevBuf<char> img;
    if (img.alloc(bytes) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the image");
    if (int rc = render_over_shutter(ts, opts, shutter, motions, n_motions, img.p, nullptr)) return rc;
    HIP_TRY(hipMemcpy(rgb_out_host, img.p, bytes, hipMemcpyDeviceToHost));
    return TAKE_OK;
}
// The vertices of a mesh at a time of the shutter, without a scene (include/take_hip.h; tk_shutter.h: k_shutter_vertices)
int check_shutter_vertices(const void *a, const void *b, int64_t n, double t, const void *out) {
    if (!a || !b || !out) return fail(TAKE_E_INVALID, "null argument");
    if (n <= 0) return fail(TAKE_E_INVALID, "n must be positive");
    if (!(t >= 0.0 && t <= 1.0)) return fail(TAKE_E_INVALID, "t must be in [0, 1]");
    return TAKE_OK;
}
}  // namespace

extern "C" {
// ------------------------------------------------------------------------------------------------ transforms, vertices
int take_hip_scene_set_instance_transforms_device(TakeScene *ts, const double *d, int64_t n, void *stream) { return set_instance_transforms(ts, d, n, hipMemcpyDeviceToDevice, stream); }
int take_hip_scene_set_instance_transforms(TakeScene *ts, const double *xforms, int64_t n) { return set_instance_transforms(ts, xforms, n, hipMemcpyHostToDevice, nullptr); }
int take_hip_scene_set_mesh_vertices(TakeScene *ts, const TakeMeshUpdate *updates, int32_t n_updates) { return update_meshes(ts, updates, n_updates, false); }
int take_hip_scene_update_meshes(TakeScene *ts, const TakeMeshUpdate *updates, int32_t n_updates) { return update_meshes(ts, updates, n_updates, true); }
// ------------------------------------------------------------------------------------------------ camera and lens
int take_hip_scene_set_camera(TakeScene *ts, const TakeCamera *camera) {
    if (!ts || !camera) return fail(TAKE_E_INVALID, "null argument");
    if (camera->width != ts->width() || camera->height != ts->height())
        return fail(TAKE_E_INVALID, "the new camera is " + std::to_string(camera->width) + " x " + std::to_string(camera->height) + ", the scene " +
                                        std::to_string(ts->width()) + " x " + std::to_string(ts->height()) + ": the render buffers are sized at creation");
    // (the lens stays; an automatic focus follows the new lookat)
    const double look = look_distance(*camera);
    const bool refocus = ts->lens.aperture_radius > 0 && !(ts->lens.focus_distance > 0);
    if (refocus && !lens_focus_usable(ts, look)) return fail(TAKE_E_INVALID, "the scene's lens focuses on lookat, and the new camera's lookat is not in front of its lookfrom");
    pose_camera(ts, *camera);
    ts->look_distance = look, ts->camera = *camera;
    if (!(ts->lens.focus_distance > 0)) ts->lens_focus = look;
    apply_lens(ts);
    ts->acc_samples = 0, ts->acc_restart_needed = true;
    return TAKE_OK;
}

// The thin lens (include/take_hip.h; tk_lens.h): two members of every side's camera record, which the launches pass by
// value — no device memory changes, so no device is looked for.
int take_hip_scene_set_lens(TakeScene *ts, const TakeLens *lens) {
    if (!ts || !lens) return fail(TAKE_E_INVALID, "null argument");
    if (!(lens->aperture_radius >= 0) || !std::isfinite(lens->aperture_radius)) return fail(TAKE_E_INVALID, "the aperture radius must be finite and >= 0");
    if (!std::isfinite(lens->focus_distance)) return fail(TAKE_E_INVALID, "the focus distance must be finite");
    if (lens->flags != 0 || lens->reserved != 0) return fail(TAKE_E_INVALID, "flags and reserved must be 0");
    const double focus = lens->focus_distance > 0 ? lens->focus_distance : ts->look_distance;
    if (lens->aperture_radius > 0 && !lens_focus_usable(ts, focus))
        return fail(TAKE_E_INVALID, "the effective focus distance must be > 0 (and finite in the scene's precision): focus_distance <= 0 asks for |lookat - lookfrom|");
    ts->lens = *lens, ts->lens_focus = focus;
    apply_lens(ts);
    ts->acc_samples = 0, ts->acc_restart_needed = true;
    return TAKE_OK;
}
int take_hip_scene_get_lens(const TakeScene *ts, TakeLens *out) {
    if (!ts || !out) return fail(TAKE_E_INVALID, "null argument");
    *out = ts->lens;
    out->focus_distance = ts->lens_focus;
    return TAKE_OK;
}
int take_hip_scene_focus_distance_at(TakeScene *ts, int32_t column, int32_t row, double *distance_out) {
    if (!ts || !distance_out) return fail(TAKE_E_INVALID, "null argument");
    if (column < 0 || column >= ts->width() || row < 0 || row >= ts->height())
        return fail(TAKE_E_INVALID, "pixel (" + std::to_string(column) + ", " + std::to_string(row) + ") is outside the " + std::to_string(ts->width()) + " x " +
                                        std::to_string(ts->height()) + " image");
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    return focus_distance_scene(ts, column, row, distance_out);
}
// ------------------------------------------------------------------------------------------------ mark and track
// "The previous frame" of the temporal accumulation (include/take_hip.h): every side's camera and a copy of the
// placements' current transforms.  The copy is made first: a failed call leaves the earlier mark whole.
int take_hip_scene_mark_frame(TakeScene *ts) {
    if (!ts) return fail(TAKE_E_INVALID, "null argument");
    TAKE_ON_DEVICE(ts);
    DevBuf<double> copy;
    if (ts->n_placements > 0) {
        if (!has_own_transforms(ts)) return fail(TAKE_E_INVALID, "unsupported: the scene is a replica of a scene group");
        if (copy.alloc(ts->xforms.n) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the marked frame's transforms");
        HIP_TRY(hipMemcpy(copy.p, ts->xforms.p, copy.bytes(), hipMemcpyDeviceToDevice));
    }
    ts->mark.xforms = std::move(copy);
    ts->mark.drop_geometry(), ts->mark.updated = false;  // (the records are the marked ones again)
    ts->mark.cam_f = ts->f.dev.cam, ts->mark.cam_d = ts->d.dev.cam;  // (a side the scene does not have: never read)
    ts->mark.camera = ts->camera;
    ts->mark.set = true;
    return TAKE_OK;
}

// Following moved vertices in the motion pass (include/take_hip.h): a switch in the handle; what it holds is made by
// update_meshes and dropped by take_hip_scene_mark_frame.
int take_hip_scene_track_vertices(TakeScene *ts, int32_t flags) {
    if (!ts) return fail(TAKE_E_INVALID, "null argument");
    if (flags & ~TAKE_TRACK_VERTICES) return fail(TAKE_E_INVALID, "unknown flag bits");
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    if (!flags) ts->mark.drop_geometry();
    ts->track_flags = flags;
    return TAKE_OK;
}
int take_hip_scene_tracking_info(const TakeScene *ts, int32_t *flags, int64_t *marked_bytes) {
    if (!ts) return fail(TAKE_E_INVALID, "null argument");
    if (flags) *flags = ts->track_flags;
    if (marked_bytes) *marked_bytes = (int64_t)(ts->mark.geom_f.bytes() + ts->mark.geom_d.bytes() + ts->mark.inst_first.bytes());
    return TAKE_OK;
}
// ------------------------------------------------------------------------------------------------ the shutter
int take_hip_shutter_plan(int32_t spp, const TakeShutter *shutter, int32_t *slices_out, int32_t *first_sample, double *time) {
    if (!slices_out) return fail(TAKE_E_INVALID, "null argument");
    const TakeShutter s = shutter ? *shutter : TakeShutter{0.0, 1.0, 0, 0};
    if (int rc = check_shutter(s)) return rc;
    if (spp <= 0) return fail(TAKE_E_INVALID, "spp must be positive");
    const int32_t K = s.slices <= 0 ? std::min<int32_t>(spp, 16) : std::min(s.slices, spp);
    *slices_out = K;
    for (int32_t k = 0; first_sample && k <= K; k++) first_sample[k] = (int32_t)((int64_t)k * spp / K);
    for (int32_t k = 0; time && k < K; k++) time[k] = s.open + (s.close - s.open) * ((k + 0.5) / K);
    return TAKE_OK;
}
int take_hip_shutter_pose(TakeScene *ts, double t, TakeCamera *camera_out, double *xforms_out) {
    if (!ts || !camera_out) return fail(TAKE_E_INVALID, "null argument");
    if (!(t >= 0.0 && t <= 1.0)) return fail(TAKE_E_INVALID, "t must be in [0, 1]");
    if (const int nd = check_device(); nd < 0) return nd;
    TAKE_ON_DEVICE(ts);
    if (const int rc = check_shutter_scene(ts)) return rc;
    std::vector<TakeCamera> cams;
    DevBuf<double> posed;
    std::vector<int> moved;
    if (const int rc = shutter_poses(ts, {t}, xforms_out != nullptr, cams, posed, moved)) return rc;
    if (posed.p) HIP_TRY(hipMemcpy(xforms_out, posed.p, posed.bytes(), hipMemcpyDeviceToHost));
    *camera_out = cams[0];
    return TAKE_OK;
}
int take_hip_render_shutter_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, void *d_rgb_out, void *stream) {
    return render_shutter_to_device(ts, opts, shutter, nullptr, 0, d_rgb_out, stream);
}
int take_hip_render_shutter(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, void *rgb_out_host) {
    return render_shutter_to_host(ts, opts, shutter, nullptr, 0, rgb_out_host);
}
int take_hip_render_shutter_meshes_device(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n,
                                          void *d_rgb_out, void *stream) {
    return render_shutter_to_device(ts, opts, shutter, motions, n, d_rgb_out, stream);
}
int take_hip_render_shutter_meshes(TakeScene *ts, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n,
                                   void *rgb_out_host) {
    return render_shutter_to_host(ts, opts, shutter, motions, n, rgb_out_host);
}
int take_hip_shutter_vertices_device(const double *d_a, const double *d_b, int64_t n, double t, double *d_out, int32_t *moved_host, void *stream) {
    if (int rc = check_shutter_vertices(d_a, d_b, n, t, d_out)) return rc;
    if (const int nd = check_device(); nd < 0) return nd;
    int device = 0, num_cus = 0;
    HIP_TRY(hipGetDevice(&device));
    if (hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || num_cus <= 0) num_cus = 256;
    DevBuf<int> moved;
    if (moved.alloc(1) != hipSuccess) return fail(TAKE_E_NOMEM, "out of device memory for the vertices at a time of the shutter");
    HIP_TRY(hipMemsetAsync(moved.p, 0, sizeof(int), (hipStream_t)stream));
    shutter_vertices_launch(d_a, d_b, n, t, d_out, moved.p, num_cus, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, moved.p, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (moved_host) *moved_host = flag;
    return TAKE_OK;
}
int take_hip_shutter_vertices(const double *a, const double *b, int64_t n, double t, double *out, int32_t *moved) {
    if (int rc = check_shutter_vertices(a, b, n, t, out)) return rc;
    if (const int nd = check_device(); nd < 0) return nd;
    DevBuf<double> d_a, d_b, d_out;
    if (d_a.alloc((size_t)n) != hipSuccess || d_b.alloc((size_t)n) != hipSuccess || d_out.alloc((size_t)n) != hipSuccess)
        return fail(TAKE_E_NOMEM, "out of device memory for the vertices at a time of the shutter");
    HIP_TRY(hipMemcpy(d_a.p, a, d_a.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_b.p, b, d_b.bytes(), hipMemcpyHostToDevice));
    if (int rc = take_hip_shutter_vertices_device(d_a.p, d_b.p, n, t, d_out.p, moved, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost));
    return TAKE_OK;
}

}  // extern "C"

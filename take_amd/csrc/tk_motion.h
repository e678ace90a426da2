// tk_motion.h — the motion pass (take_hip_render_motion*): per pixel, where the surface point the pixel's centre ray
// hits was in the MARKED frame (take_hip_scene_mark_frame: the previous camera, the previous placements), as plane
// coordinates of that frame, with its distance from the marked camera; and the centre ray's own depth and shape id —
// the planes the temporal accumulation (tk_temporal.h) tests its history against.  Specification: DESIGN.md §4i.
//
//   CentreCameraIo   the camera ray through the pixel centre, made by the closest-hit launch that traces it (CameraIo
//                    with 0.5 in place of the two draws: no generate pass, no random stream)
//   k_motion         per pixel: the hit the launch left in the path record -> P -> through the placement's current
//                    inverse and its marked transform -> projected with the marked camera -> the caller's planes;
//                    TRACKED (the handle holds marked geometry: take_hip_scene_track_vertices): a triangle hit goes
//                    back through the words its record had at the mark instead (tk_motion_pixel.h: tracked_pixel)
//
// The pass is one closest-hit launch followed by k_motion.  Nothing here is reached by a render.
#pragma once

#include "tk_features.h"
#include "tk_motion_pixel.h"

namespace tk {

// camera_dir (tk_integrate.h) for the centre of the pixel of path slot `slot`: the same operations with rx = ry = 0.5
template <class R> TK_HD Vec3<R> camera_dir_centre(const CameraRec<R> &c, const RenderParams<R> &rp, int64_t slot) {
    int sl, lr, x;
    slot_pixel(rp, slot, sl, lr, x);
    const int y = local_row_to_y(rp, lr);
    return normalize(ld3(c.u) * ((R(x) + R(0.5)) / R(c.width) - R(0.5)) * c.viewport_width +
                     ld3(c.v) * ((R(y) + R(0.5)) / R(c.height) - R(0.5)) * c.viewport_height - ld3(c.w));
}
template <class R> struct CentreCameraIo : PathIo<R> {
    CameraRec<R> cam;
    RenderParams<R> rp;
    template <bool SHADOW> __device__ __forceinline__ void load(int32_t i, RayT<R> &ray, int32_t &tag) const {
        const int64_t slot = i;
        tag = i;
        const Vec3<R> d = camera_dir_centre(cam, rp, slot);
        const PathState<R> &st = this->st;
        st.R_(S_OX, slot) = cam.lookfrom[0], st.R_(S_OY, slot) = cam.lookfrom[1], st.R_(S_OZ, slot) = cam.lookfrom[2];
        st.R_(S_DX, slot) = d.x, st.R_(S_DY, slot) = d.y, st.R_(S_DZ, slot) = d.z;
        ray = make_ray(cam.lookfrom[0], cam.lookfrom[1], cam.lookfrom[2], d.x, d.y, d.z, this->eps, Const<R>::inf());
    }
};

template <class R> struct MotionOut {  // TakeMotionBuffers for records of precision R, in device memory
    R *prev_xy, *prev_depth, *depth;
    int32_t *shape_id;
};

// marked: the camera of the marked frame; marked_xforms: the placements' object -> world transforms of the marked
// frame, 12 doubles each (null in a scene without placements), each rounded to R once where it is used.
// TRACKED: geom is the marked geometry (its words never null); per pixel one more gather, of the 9 words of the hit
// record's entry (36 bytes in f32, 72 in f64), and no read of the placement's inverse for a triangle.
template <class R, bool TRACKED>
__global__ void __launch_bounds__(BLOCK)
k_motion(DeviceScene<R> sc, PathState<R> st, CameraRec<R> marked, const double *__restrict__ marked_xforms, MarkedGeometry<R> geom, MotionOut<R> out, int32_t width,
         int32_t n_local_rows) {
    const int32_t npix = width * n_local_rows;
    for (int32_t p = blockIdx.x * BLOCK + threadIdx.x; p < npix; p += gridDim.x * BLOCK) {
        const int64_t slot = p;
        const int32_t prim = st.I_(S_HIT, slot);
        const Vec3<R> rd{st.R_(S_DX, slot), st.R_(S_DY, slot), st.R_(S_DZ, slot)};
        R depth = R(0), prev_depth = R(0), px = R(-2), py = R(-2);
        int32_t shape = -1;
        if constexpr (TRACKED) {
            MotionHit<R> h{MOTION_MISS, Vec3<R>{R(0), R(0), R(0)}, rd, R(0), R(0), R(0), nullptr, nullptr, nullptr};
            if (prim >= 0) {
                const int32_t inst = sc.inst_shade ? st.I_(S_INST, slot) : -1;
                const int32_t id = sc.prims[prim].shape_id;  // the shape id, or the face of a prototype's record
                const bool in_placement = inst >= 0 && marked_xforms;
                h.ro = {st.R_(S_OX, slot), st.R_(S_OY, slot), st.R_(S_OZ, slot)};
                h.t = depth = st.R_(S_HT, slot);
                shape = inst >= 0 ? id + sc.inst_shade[inst].shape_base : id;
                if (in_placement) h.inv = sc.inst_trace[inst].inv, h.fwd = marked_xforms + 12 * (int64_t)inst;
                if ((sc.prims[prim].meta & 0xff) == PRIM_TRIANGLE) {
                    h.kind = MOTION_TRIANGLE, h.u = st.R_(S_HU, slot), h.v = st.R_(S_HV, slot);
                    h.words = geom.words + MARKED_STRIDE * ((int64_t)id + (inst >= 0 ? geom.inst_first[inst] : 0));
                } else {
                    h.kind = MOTION_POINT;
                }
            }
            tracked_pixel(marked, h, px, py, prev_depth);
            const int64_t o = feature_out_index(p, width, n_local_rows);
            if (out.prev_xy) out.prev_xy[2 * o] = px, out.prev_xy[2 * o + 1] = py;
            if (out.prev_depth) out.prev_depth[o] = prev_depth;
            if (out.depth) out.depth[o] = depth;
            if (out.shape_id) out.shape_id[o] = shape;
            continue;
        }
        Vec3<R> e = rd;  // a miss: a point at infinity
        if (prim >= 0) {
            const R t = st.R_(S_HT, slot);
            const Vec3<R> ro{st.R_(S_OX, slot), st.R_(S_OY, slot), st.R_(S_OZ, slot)};
            const int32_t inst = sc.inst_shade ? st.I_(S_INST, slot) : -1;
            Vec3<R> P = ro + rd * t;
            shape = sc.prims[prim].shape_id;
            if (inst >= 0) {
                shape += sc.inst_shade[inst].shape_base;
                if (marked_xforms) {
                    R fwd[12];
                    for (int k = 0; k < 12; k++) fwd[k] = (R)marked_xforms[12 * (int64_t)inst + k];
                    P = affine_point(fwd, affine_point(sc.inst_trace[inst].inv, P));
                }
            }
            depth = t;
            e = P - Vec3<R>{marked.lookfrom[0], marked.lookfrom[1], marked.lookfrom[2]};
        }
        const bool seen = project_marked(marked, e, px, py);
        if (!seen) px = R(-2), py = R(-2);
        else if (prim >= 0) prev_depth = tk_sqrt((e.x * e.x + e.y * e.y) + e.z * e.z);
        const int64_t o = feature_out_index(p, width, n_local_rows);
        if (out.prev_xy) out.prev_xy[2 * o] = px, out.prev_xy[2 * o + 1] = py;
        if (out.prev_depth) out.prev_depth[o] = prev_depth;
        if (out.depth) out.depth[o] = depth;
        if (out.shape_id) out.shape_id[o] = shape;
    }
}

}  // namespace tk

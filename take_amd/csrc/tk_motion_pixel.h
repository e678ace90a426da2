// tk_motion_pixel.h — the per-pixel arithmetic of the motion pass (tk_motion.h; specification: DESIGN.md §4i): the
// projection with the marked camera that every instance of k_motion ends in, and tracked_pixel — the whole pixel of the
// instances that follow moved vertices (take_hip_scene_track_vertices), which take a triangle hit back through the
// geometry words its record had in the marked frame.  TK_HD and written once, as tk_temporal.h's accumulate_pixel: the
// kernel runs it on the device, tests/motion_host runs the same text on the host, tests/motion_ref.py restates it in
// numpy.  Every + - * / is one operation in the order written (-ffp-contract=off).
#pragma once
#include <cstdint>

#include "tk_scene.h"

namespace tk {

// a 3 x 4 row-major affine map applied to a point, each row ((m0 * x + m1 * y) + m2 * z) + m3
template <class R> TK_HD Vec3<R> affine_point(const R *m, Vec3<R> p) {
    return {((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3], ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7], ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11]};
}
template <class R> TK_HD R dot3(const R *a, Vec3<R> e) { return (a[0] * e.x + a[1] * e.y) + a[2] * e.z; }

// e (P' - lookfrom', or a direction for a point at infinity) projected with the marked camera -> plane coordinates
// (column, row), a pixel's centre at +0.5; false: behind the camera (z <= 0, or not a number)
template <class R> TK_HD bool project_marked(const CameraRec<R> &m, Vec3<R> e, R &px, R &py) {
    const R z = -dot3(m.w, e);
    if (!(z > R(0))) return false;
    const R sx = (dot3(m.u, e) / z / m.viewport_width + R(0.5)) * R(m.width);
    const R sy = (dot3(m.v, e) / z / m.viewport_height + R(0.5)) * R(m.height);
    px = sx, py = R(m.height) - sy;
    return true;
}

// ---- the marked geometry (take_hip_scene_track_vertices): the geometry words PrimRec::a — v0, e1, e2 — every record
// had at the mark, one entry of MARKED_STRIDE Reals per record IDENTITY (the words first, the rest zero: an entry is
// whole 16-byte words, 48 bytes in f32 and 96 in f64).  A rebuild puts records into a new leaf order, identities stay:
// entry = the shape id for the shapes' records (the head of the record array), first entry of the placement's prototype
// + face (PrimRec::shape_id of a prototype's record) for a prototype's — as many entries as the scene has records.
constexpr int MARKED_STRIDE = 12;
template <class R> struct MarkedGeometry {
    const R *words;             // MARKED_STRIDE Reals per entry; null: the handle holds none
    const int32_t *inst_first;  // per placement: the first entry of its prototype (null in a scene without placements)
};

// What the centre ray of a pixel found, for tracked_pixel.  MISS: a point at infinity in direction rd.  POINT: the
// world-space point ro + rd * t, rigid in its placement (inv, fwd: the placement's current inverse in Real and its
// marked transform in double; both null outside a placement) — a sphere.  TRIANGLE: barycentrics u (along e1, as
// tri_test has them) and v (along e2) on the marked words of the hit record's identity; fwd as for POINT.
enum MotionKind : int32_t { MOTION_MISS = 0, MOTION_POINT = 1, MOTION_TRIANGLE = 2 };
template <class R> struct MotionHit {
    int32_t kind;
    Vec3<R> ro, rd;
    R t, u, v;
    const R *words;     // 9 Reals: v0', e1', e2'
    const R *inv;       // 12 Reals
    const double *fwd;  // 12 doubles, each rounded to Real once
};

// -> prev_xy (px, py; -2, -2 where the marked camera does not see the point) and prev_depth (0 for a miss or an unseen point)
template <class R> TK_HD void tracked_pixel(const CameraRec<R> &marked, const MotionHit<R> &h, R &px, R &py, R &prev_depth) {
    Vec3<R> e = h.rd;
    if (h.kind != MOTION_MISS) {
        Vec3<R> P;
        if (h.kind == MOTION_TRIANGLE) {
            const R *g = h.words;
            P = {(g[0] + g[3] * h.u) + g[6] * h.v, (g[1] + g[4] * h.u) + g[7] * h.v, (g[2] + g[5] * h.u) + g[8] * h.v};
        } else {
            P = h.ro + h.rd * h.t;
            if (h.fwd) P = affine_point(h.inv, P);
        }
        if (h.fwd) {
            R fwd[12];
            for (int k = 0; k < 12; k++) fwd[k] = (R)h.fwd[k];
            P = affine_point(fwd, P);
        }
        e = P - Vec3<R>{marked.lookfrom[0], marked.lookfrom[1], marked.lookfrom[2]};
    }
    px = R(-2), py = R(-2), prev_depth = R(0);
    const bool seen = project_marked(marked, e, px, py);
    if (!seen) px = R(-2), py = R(-2);
    else if (h.kind != MOTION_MISS) prev_depth = tk_sqrt((e.x * e.x + e.y * e.y) + e.z * e.z);
}

}  // namespace tk

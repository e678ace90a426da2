// tk_shutter.h — the pose of a scene at a time of the shutter (EXTENSION, parity unpinned; specification: DESIGN.md
// §4l): scene time 0 is the marked frame (take_hip_scene_mark_frame), 1 the current one, and everything in between is
// the entry-by-entry lerp of the two — the matrix motion transform of Embree and OptiX: a rotation moves along its
// chord, not its arc.  TK_HD and written once, as tk_lens.h: k_shutter_pose runs it on the device, tk_render.hip's
// shutter_camera calls the same text for the camera, tests/shutter_host runs it on the host, tests/shutter_ref.py restates it in numpy.  Every
// + - * is one operation of double in the order written (-ffp-contract=off).  k_shutter_vertices runs the same lerp over
// the vertex arrays of a deforming mesh (tests/shutter_deform_host, tests/shutter_deform_ref.py).
#pragma once
#include <cstdint>

#include "tk_common.h"

namespace tk {

// (1 - t) a + t b: `1 - t` rounded once, two products, one sum.  t = 0 gives a and t = 1 gives b (as values: a zero
// comes out as +0 unless both ends are -0).  Where the ends are equal the result is the current end, b, itself — the
// sum above is not: (1 - t) a + t a rounds three times — so what did not move between the mark and now stays where it
// is at every t, bit for bit.
TK_HD double shutter_lerp(double t, double a, double b) {
    const double s = 1.0 - t;
    return a == b ? b : s * a + t * b;
}

// The 12 doubles of a placement's object -> world transform at time t, between a (t = 0) and b (t = 1) -> out; false
// where the re-pose would refuse the result (k_placement_records' rule: an entry that is not finite, or a linear part
// with |det| <= 1e-300 — the determinant in its expression).  out is written either way.
TK_HD bool shutter_pose12(const double *a, const double *b, double t, double *out) {
    bool finite = true;
    for (int k = 0; k < 12; k++) out[k] = shutter_lerp(t, a[k], b[k]), finite = finite && __builtin_isfinite(out[k]);
    const double a00 = out[0], a01 = out[1], a02 = out[2], a10 = out[4], a11 = out[5], a12 = out[6], a20 = out[8], a21 = out[9], a22 = out[10];
    const double det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    return finite && __builtin_fabs(det) > 1e-300;
}

#if defined(__HIPCC__)
constexpr int SHUTTER_BLOCK = 256;
// One lane per (slice, placement), lane = slice * n + placement: the n placements of a scene, marked -> current, at
// the times of n_slices slices -> posed[12 * lane ..].  The smallest lane whose pose the re-pose would refuse is left
// in *bad (INT_MAX before): the first offending slice, and in it the first placement.  moved[slice] (0 before) becomes
// 1 where any entry of the slice's pose is not, bit for bit, the current transform's: a slice that stays 0 IS the
// current pose and needs no re-pose (placements that did not move since the mark: camera blur only).
__global__ void __launch_bounds__(SHUTTER_BLOCK) k_shutter_pose(const double *__restrict__ marked, const double *__restrict__ current,
                                                                const double *__restrict__ times, int n_slices, int n, double *__restrict__ posed, int *bad,
                                                                int *moved) {
    const int64_t lane = (int64_t)blockIdx.x * SHUTTER_BLOCK + threadIdx.x;
    if (lane >= (int64_t)n_slices * n) return;
    const int k = (int)(lane / n), i = (int)(lane % n);
    double a[12], b[12], m[12];
#pragma unroll
    for (int e = 0; e < 12; e++) a[e] = marked[12 * (int64_t)i + e], b[e] = current[12 * (int64_t)i + e];
    const bool ok = shutter_pose12(a, b, times[k], m);
    bool same = true;
#pragma unroll
    for (int e = 0; e < 12; e++) posed[12 * lane + e] = m[e], same = same && __double_as_longlong(m[e]) == __double_as_longlong(b[e]);
    if (!ok) atomicMin(bad, (int)lane);
    if (!same) atomicOr(&moved[k], 1);
}

// The vertices of a deforming mesh at scene time t (take_hip_render_shutter_meshes*): n doubles — the
// 3 n_vertices coordinates of its positions, or of its vertex normals —, a (the marked frame) -> b (the current one),
// out[e] = shutter_lerp(t, a[e], b[e]).  Nothing is looked at: a value that is not finite passes through, a lerped normal
// is not renormalised.  A streaming kernel: per lane and step 16 bytes in from each side and 16 out, over a grid sized
// to the device (SHUTTER_BLOCKS_PER_CU blocks per CU) that strides over the array.  `head` (0 or 1) elements come before
// the `pairs` 16-byte-aligned pairs — the launch finds both from the three addresses, pairs = 0 where they do not agree
// mod 16 — and n - head - 2 pairs after them; those take the scalar loop.  out may be a or b: every lane reads its
// elements before it writes them.  *moved (0 before) becomes 1 where any out[e] is not b[e] bit for bit: the flags are
// reduced inside the wave, and a wave adds at most one atomic.
constexpr int SHUTTER_BLOCKS_PER_CU = 8;
__global__ void __launch_bounds__(SHUTTER_BLOCK) k_shutter_vertices(const double *a, const double *b, int64_t n, int head, int64_t pairs, double t, double *out,
                                                                    int *moved) {
    const int64_t lane = (int64_t)blockIdx.x * SHUTTER_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * SHUTTER_BLOCK;
    const double2 *a2 = (const double2 *)(a + head), *b2 = (const double2 *)(b + head);
    double2 *out2 = (double2 *)(out + head);
    bool differs = false;
    for (int64_t i = lane; i < pairs; i += step) {
        const double2 x = a2[i], y = b2[i];
        double2 r;
        r.x = shutter_lerp(t, x.x, y.x), r.y = shutter_lerp(t, x.y, y.y);
        out2[i] = r;
        differs = differs || __double_as_longlong(r.x) != __double_as_longlong(y.x) || __double_as_longlong(r.y) != __double_as_longlong(y.y);
    }
    const int64_t tail = head + 2 * pairs, rest = head + (n - tail);
    for (int64_t i = lane; i < rest; i += step) {
        const int64_t e = i < head ? i : tail + (i - head);
        const double y = b[e], r = shutter_lerp(t, a[e], y);
        out[e] = r;
        differs = differs || __double_as_longlong(r) != __double_as_longlong(y);
    }
    if (__any(differs) && (threadIdx.x & 63) == 0) atomicOr(moved, 1);
}
#endif

}  // namespace tk

// tk_displace.h — displacement mapping of triangle meshes: what take_hip_displace_* and take_hip_scene_displace_meshes in
// front of the mesh update compute (include/take_hip.h; specification: DESIGN.md §4t).  Three parts:
//   1. the per-vertex body, TK_HD and written once: the kernel at the end of this file runs it on the device,
//      tests/displace_host runs it in the kernel's loop structure on the host;
//   2. what creation does on the host, once per handle: the check of a description, every vertex's row of faces, and
//      the lookup coordinates (a, b) of every vertex;
//   3. the kernel.  Launched from tk_displace.hip.
// The normals before and after the displacement are face_normal and vertex_normal of tk_subdiv.h, launched by
// tk_subdiv.hip (tk_host.h: subdiv_launch_normals); this file does not include that one, whose kernels one unit compiles.
//
// Arithmetic: everything is double (a float texel is widened on load, which is exact); every + - * / is one operation
// in the order written (-ffp-contract=off); fmod and floor are the only library calls.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "tk_common.h"

namespace tk {
namespace displace {

// Where vertex v looks the height up: a = modulo1(uscale * u + uoffset), b = modulo1(vscale * v + voffset), both in
// [0, 1).  16 bytes, aligned: one dwordx4 load per lane.
struct alignas(16) Source {
    double a, b;
};

// ---------------------------------------------------------------------------------------------- 1. the body
// modulo(a, 1) as the texture lookup has it (tk_shade.h: modulo1, restated here): for a in (-2^-54, 0) the sum r + 1
// rounds to exactly 1 and the result is the largest double below 1 instead, so it lies in [0, 1) for every finite a.
TK_HD double modulo1(double a) {
    double r = tk_fmod(a, 1.0);
    if (r < 0.0) {
        r = r + 1.0;
        r = (r < 1.0) ? r : Const<double>::BELOW_ONE;
    }
    return r;
}

// The cell of coordinate c in [0, 1) along an axis of n texels, sample i at c = i / n: its two texels i1, i2 (i2 wraps to
// 0 behind the last) and the fraction f in [0, 1) between them.  n * c < n for every c < 1 (n * (1 - 2^-53) rounds below
// n), so 0 <= i1 < n.
TK_HD void cell(double c, int32_t n, int32_t &i1, int32_t &i2, double &f) {
    const double x = (double)n * c;
    const double x1 = tk_floor(x);
    f = x - x1;
    i1 = (int32_t)x1;
    i2 = (i1 + 1 == n) ? 0 : i1 + 1;
}

// The height at (a, b): bilinear between the cell's four texels, with wrap.
template <class T> TK_HD double height_at(const T *texels, int32_t width, int32_t height, Source s) {
    int32_t x1, x2, y1, y2;
    double fx, fy;
    cell(s.a, width, x1, x2, fx);
    cell(s.b, height, y1, y2, fy);
    const double q11 = (double)texels[(int64_t)y1 * width + x1], q21 = (double)texels[(int64_t)y1 * width + x2];
    const double q12 = (double)texels[(int64_t)y2 * width + x1], q22 = (double)texels[(int64_t)y2 * width + x2];
    return (q11 * (1.0 - fx) + q21 * fx) * (1.0 - fy) + (q12 * (1.0 - fx) + q22 * fx) * fy;
}

// Vertex v: d = scale * h + bias, p' = p + d * n -> out[3 v ..].
template <class T>
TK_HD void displace_vertex(const Source *src, const T *texels, int32_t width, int32_t height, double scale, double bias, const double *p, const double *n, int64_t v,
                           double *out) {
    const double h = height_at(texels, width, height, src[v]);
    const double d = scale * h + bias;
    double q[3];
    for (int a = 0; a < 3; a++) q[a] = p[3 * v + a] + d * n[3 * v + a];
    for (int a = 0; a < 3; a++) out[3 * v + a] = q[a];
}

constexpr int BLOCK = 256;
constexpr int64_t MAX_BLOCKS = 1 << 16;  // a launch's grid: beyond BLOCK * MAX_BLOCKS vertices the blocks stride
inline int64_t blocks_for(int64_t n) {
    const int64_t b = (n + BLOCK - 1) / BLOCK;
    return b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

// ---------------------------------------------------------------------------------------------- 2. creation, on the host
enum { INPUT_OK = 0, INPUT_INVALID = 1, INPUT_UNSUPPORTED = 2 };
inline bool finite(double x) { return x - x == 0.0; }

// What creation refuses of a description before a device is looked for (real: 0 = float texels, 1 = double texels,
// TAKE_PRECISION_F32 / _F64) -> INPUT_OK, or a refusal with its message in `msg`.
inline int check_inputs(int64_t n_vertices, int64_t n_faces, const int32_t *indices, const double *uvs, int32_t width, int32_t height, const void *texels, int32_t real,
                        int32_t flags, int32_t known_flags, const double lookup[4], std::string &msg) {
    if (!indices || !texels) return msg = "null argument", INPUT_INVALID;
    if (!uvs) return msg = "uvs are required: a displacement looks its height up at every vertex's uv", INPUT_INVALID;
    if (flags & ~known_flags) return msg = "unknown flag bits", INPUT_INVALID;
    if (n_vertices <= 0 || n_faces <= 0) return msg = "n_vertices and n_faces must be positive", INPUT_INVALID;
    if (n_vertices > INT32_MAX || 3 * n_faces > INT32_MAX) return msg = "unsupported: a mesh beyond 32-bit indices", INPUT_UNSUPPORTED;
    if (width <= 0 || height <= 0) return msg = "width and height must be positive", INPUT_INVALID;
    if ((int64_t)width * height > INT32_MAX) return msg = "width * height must not pass INT32_MAX", INPUT_INVALID;
    if (real != 0 && real != 1) return msg = "unknown precision", INPUT_INVALID;
    for (int k = 0; k < 4; k++)
        if (!finite(lookup[k])) return msg = "uscale, vscale, uoffset and voffset must be finite", INPUT_INVALID;
    for (int64_t f = 0; f < n_faces; f++)
        for (int k = 0; k < 3; k++) {
            const int32_t i = indices[3 * f + k];
            if (i < 0 || i >= n_vertices) return msg = "face " + std::to_string(f) + ": vertex index " + std::to_string(i) + " out of range", INPUT_INVALID;
        }
    return INPUT_OK;
}

// Every vertex's lookup coordinates.  lookup: uscale, vscale, uoffset, voffset.  A vertex whose s or t is not finite is
// refused and named: the kernel never converts a NaN to an index.
inline int build_sources(int64_t n_vertices, const double *uvs, const double lookup[4], std::vector<Source> &out, std::string &msg) {
    out.resize((size_t)n_vertices);
    for (int64_t v = 0; v < n_vertices; v++) {
        const double s = lookup[0] * uvs[2 * v] + lookup[2];
        const double t = lookup[1] * uvs[2 * v + 1] + lookup[3];
        if (!finite(s) || !finite(t)) return msg = "vertex " + std::to_string(v) + ": its lookup coordinates are not finite", INPUT_INVALID;
        out[v] = Source{modulo1(s), modulo1(t)};
    }
    return INPUT_OK;
}

// Every vertex's row of incident faces, ascending (faces are walked in ascending order: so is every row), by a counting
// sort as subdiv::Topology's face_start / faces are made.  face_start: n_vertices + 1 rows; faces: 3 n_faces.
inline void build_rows(int64_t n_vertices, int64_t n_faces, const int32_t *indices, std::vector<int32_t> &face_start, std::vector<int32_t> &faces) {
    face_start.assign((size_t)n_vertices + 1, 0);
    for (int64_t i = 0; i < 3 * n_faces; i++) face_start[indices[i] + 1]++;
    for (int64_t v = 0; v < n_vertices; v++) face_start[v + 1] += face_start[v];
    faces.resize(3 * (size_t)n_faces);
    std::vector<int32_t> at(face_start.begin(), face_start.end() - 1);
    for (int64_t f = 0; f < n_faces; f++)
        for (int k = 0; k < 3; k++) faces[at[indices[3 * f + k]]++] = (int32_t)f;
}

// ---------------------------------------------------------------------------------------------- 3. the kernel
#if defined(__HIPCC__)
// (The byte figures in this comment are counted from the layout, not measured.)
// One lane per vertex, consecutive lanes consecutive vertices: a wave reads 1024 contiguous bytes of (a, b) pairs — one
// 16-byte load per lane —, 1536 + 1536 of positions and normals, and writes 1536; the four texels are the gather — 4 or 8
// bytes each, two pairs of neighbours in a row unless the cell wraps.  No atomics, no LDS: a vertex shared by several
// faces is one lane and moves once.  Two instances: float and double texels.
template <class T>
__global__ __launch_bounds__(BLOCK) void k_displace(const Source *__restrict__ src, const T *__restrict__ texels, int32_t width, int32_t height, double scale, double bias,
                                                    const double *__restrict__ p, const double *__restrict__ n, int64_t n_vertices, double *__restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < n_vertices; v += (int64_t)gridDim.x * BLOCK)
        displace_vertex(src, texels, width, height, scale, bias, p, n, v, out);
}
#endif  // __HIPCC__

}  // namespace displace
}  // namespace tk

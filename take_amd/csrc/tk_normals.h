// compute_normals on the device: Nelson Max angle-weighted vertex normals (src/compute_normals.cpp:12-47), what the
// reference's parse_scene puts into a mesh loaded without normals unless the shape sets faceNormals
// (src/parse/parse_scene.cpp:828-833, 856-861, 884-889).
//
// The reference is one serial loop: per face the unit face normal n (from corner 0), per corner the angle between the
// two sides at it, and normals[index[i]] += n * angle; then every sum is normalized.  The per-face and per-vertex
// arithmetic below is the reference's, operation for operation (src/vector.h: `v / s` multiplies by 1 / s, dot sums
// left to right, length = sqrt(dot)), and is TK_HD so that tests/normals_shim builds it for the host and checks it bit
// for bit against the reference's output.  The order of the sums is the reference's too — floating-point addition is
// not associative — so the device reduction is ordered, never atomic:
//   1. k_nrm_faces: one face per lane writes its three products n * angle, and one (vertex, corner) pair per corner;
//      a face whose normal has length 0 contributes nothing (the reference `break`s before its first add), its
//      corners get the key n_vertices, which sorts behind every vertex.
//   2. a stable rocPRIM radix sort of the pairs on the vertex (ceil(log2(n_vertices + 1)) key bits): within a vertex
//      the corners stay in increasing order = increasing face, then corner 0, 1, 2 = the reference's order.
//   3. k_nrm_bounds: each vertex's segment [begin, end) of the sorted pairs; segments longer than HEAVY are listed.
//   4. k_nrm_vertices: one lane per vertex sums its segment from +0.0 (8 contributions loaded ahead of the dependent
//      adds) and normalizes; k_nrm_heavy: one wave per listed vertex (the centre of a fan) stages 256 contributions
//      per step in LDS, the next step's loads in flight while the adds run, and every lane runs the one ordered
//      chain on broadcast reads.
// The angle goes through asin: the device's (ocml) is not glibc's and may differ in the last bit, so the host build
// reproduces the reference bit for bit and the device agrees within a few ulp (tests/test_gpu_normals.py).
#pragma once
#include <cstdint>

#include "tk_common.h"

namespace tk {
namespace nrm {

constexpr double C_PI = 3.14159265358979323846;  // c_PI (src/take.h:34)

struct V3 {
    double x, y, z;
};
TK_HD V3 add3(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
TK_HD V3 sub3(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
TK_HD V3 mul3(V3 a, double s) { return V3{a.x * s, a.y * s, a.z * s}; }
TK_HD double dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
TK_HD double length3(V3 a) { return sqrt(dot3(a, a)); }
TK_HD V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// Vector3 / Real (src/vector.h:194-197): one reciprocal, three multiplies
TK_HD V3 div3(V3 a, double s) {
    const double inv_s = 1.0 / s;
    return V3{a.x * inv_s, a.y * inv_s, a.z * inv_s};
}
// normalize (src/vector.h:250-256)
TK_HD V3 normalize3(V3 a) {
    const double l = length3(a);
    if (l <= 0) return V3{0, 0, 0};
    return div3(a, l);
}
// unit_angle (src/compute_normals.cpp:4-10).  The obtuse branch is the reference's as written: (pi - 2) * asin(...),
// not pi - 2 * asin(...) — kept, like the other upstream quirks the device reproduces.
TK_HD double unit_angle(V3 u, V3 v) {
    if (dot3(u, v) < 0) return (C_PI - 2) * asin(0.5 * length3(add3(v, u)));
    return 2 * asin(0.5 * length3(sub3(v, u)));
}

TK_HD V3 load3(const double *p, int64_t i) { return V3{p[3 * i + 0], p[3 * i + 1], p[3 * i + 2]}; }

// the three products n * angle of one face, corner 0, 1, 2 -> false: |n| == 0, the face adds nothing anywhere
TK_HD bool face_contributions(const double *pos, int32_t i0, int32_t i1, int32_t i2, V3 out[3]) {
    const V3 p[3] = {load3(pos, i0), load3(pos, i1), load3(pos, i2)};
    V3 n{0, 0, 0};
    for (int i = 0; i < 3; i++) {
        const V3 v0 = p[i], v1 = p[(i + 1) % 3], v2 = p[(i + 2) % 3];
        const V3 side1 = sub3(v1, v0), side2 = sub3(v2, v0);
        if (i == 0) {
            n = cross3(side1, side2);
            const double l = length3(n);
            if (l == 0) return false;
            n = div3(n, l);
        }
        out[i] = mul3(n, unit_angle(normalize3(side1), normalize3(side2)));
    }
    return true;
}

// the last loop of compute_normals: a zero sum stays (+0, +0, +0)
TK_HD V3 finish(V3 s) {
    const double l = length3(s);
    if (l != 0) return div3(s, l);
    return V3{0, 0, 0};
}

// any index outside [0, n_vertices)
TK_HD bool bad_face(const int32_t *idx, int64_t f, int64_t nv) {
    bool bad = false;
    for (int k = 0; k < 3; k++) bad = bad || idx[3 * f + k] < 0 || idx[3 * f + k] >= nv;
    return bad;
}

// The reference's loop as it stands, serially, on these functions (host build only: the CPU tests).  -> false: an
// index is out of range (nothing written).
inline bool compute_normals_serial(const double *pos, int64_t nv, const int32_t *idx, int64_t nf, double *out) {
    for (int64_t f = 0; f < nf; f++)
        if (bad_face(idx, f, nv)) return false;
    for (int64_t i = 0; i < 3 * nv; i++) out[i] = 0.0;
    for (int64_t f = 0; f < nf; f++) {
        V3 c[3];
        if (!face_contributions(pos, idx[3 * f], idx[3 * f + 1], idx[3 * f + 2], c)) continue;
        for (int i = 0; i < 3; i++) {
            double *s = out + 3 * (int64_t)idx[3 * f + i];
            s[0] = s[0] + c[i].x, s[1] = s[1] + c[i].y, s[2] = s[2] + c[i].z;
        }
    }
    for (int64_t v = 0; v < nv; v++) {
        const V3 r = finish(load3(out, v));
        out[3 * v + 0] = r.x, out[3 * v + 1] = r.y, out[3 * v + 2] = r.z;
    }
    return true;
}

#if defined(__HIPCC__)
constexpr int BLK = 256;
constexpr int LOOKAHEAD = 8;  // contributions a lane of k_nrm_vertices loads before it adds
constexpr int HEAVY = 64;     // longer segments: k_nrm_heavy
constexpr int HCHUNK = 4;     // contributions per lane per step of k_nrm_heavy (4 * 64 = 256 per step)

// one face per lane: keys[c] = the vertex of corner c (n_vertices: nothing to add), vals[c] = c, contrib[3c..3c+2] =
// n * angle.  status[0] |= 1: an index outside [0, n_vertices) (the face adds nothing, its positions are not read)
__global__ __launch_bounds__(BLK) void k_nrm_faces(const double *pos, const int32_t *idx, int64_t nf, int64_t nv,
                                                   double *contrib, uint32_t *keys, int32_t *vals, uint32_t *status) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const bool bad = bad_face(idx, f, nv);
    if (bad) atomicOr(status, 1u);
    V3 c[3];
    const bool ok = !bad && face_contributions(pos, idx[3 * f], idx[3 * f + 1], idx[3 * f + 2], c);
    for (int i = 0; i < 3; i++) {
        const int64_t k = 3 * f + i;
        keys[k] = ok ? (uint32_t)idx[k] : (uint32_t)nv;
        vals[k] = (int32_t)k;
        if (ok) contrib[3 * k + 0] = c[i].x, contrib[3 * k + 1] = c[i].y, contrib[3 * k + 2] = c[i].z;
    }
}

// per vertex, its run [begin, end) in the sorted keys (begin / end zeroed beforehand: a vertex no face adds to keeps
// the empty run); runs longer than HEAVY go on the list k_nrm_heavy works through (status[1] = its length)
__global__ __launch_bounds__(BLK) void k_nrm_bounds(const uint32_t *keys, int64_t n, uint32_t nv, int32_t *begin,
                                                    int32_t *end, int32_t *heavy, uint32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k >= nv) return;
    if (i == 0 || keys[i - 1] != k) {
        begin[k] = (int32_t)i;
        if (i + HEAVY < n && keys[i + HEAVY] == k) heavy[atomicAdd(status + 1, 1u)] = (int32_t)k;
    }
    if (i == n - 1 || keys[i + 1] != k) end[k] = (int32_t)(i + 1);
}

TK_D void store3(double *out, int64_t v, V3 r) { out[3 * v + 0] = r.x, out[3 * v + 1] = r.y, out[3 * v + 2] = r.z; }

// one vertex per lane, runs of at most HEAVY contributions: the sum from +0.0 in the sorted (= the reference's) order
__global__ __launch_bounds__(BLK) void k_nrm_vertices(const double *contrib, const int32_t *order, const int32_t *begin,
                                                      const int32_t *end, int64_t nv, double *out) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int32_t b = begin[v], e = end[v];
    if (e - b > HEAVY) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t j = b; j < e; j += LOOKAHEAD) {
        int32_t c[LOOKAHEAD];
        double x[LOOKAHEAD], y[LOOKAHEAD], z[LOOKAHEAD];
#pragma unroll
        for (int q = 0; q < LOOKAHEAD; q++) c[q] = j + q < e ? order[j + q] : -1;
#pragma unroll
        for (int q = 0; q < LOOKAHEAD; q++)
            if (c[q] >= 0) x[q] = contrib[3 * (int64_t)c[q]], y[q] = contrib[3 * (int64_t)c[q] + 1], z[q] = contrib[3 * (int64_t)c[q] + 2];
#pragma unroll
        for (int q = 0; q < LOOKAHEAD; q++)
            if (c[q] >= 0) sx = sx + x[q], sy = sy + y[q], sz = sz + z[q];
    }
    store3(out, v, finish(V3{sx, sy, sz}));
}

struct Chunk {
    double x[HCHUNK], y[HCHUNK], z[HCHUNK];
};
// contributions base + q * 64 + lane of the run (those before `e`); o: their corners
TK_D void load_order(const int32_t *order, int64_t base, int64_t e, int lane, int32_t o[HCHUNK]) {
#pragma unroll
    for (int q = 0; q < HCHUNK; q++) o[q] = base + q * 64 + lane < e ? order[base + q * 64 + lane] : -1;
}
TK_D void load_chunk(const double *contrib, const int32_t o[HCHUNK], Chunk &c) {
#pragma unroll
    for (int q = 0; q < HCHUNK; q++) {
        c.x[q] = c.y[q] = c.z[q] = 0.0;
        if (o[q] >= 0) c.x[q] = contrib[3 * (int64_t)o[q]], c.y[q] = contrib[3 * (int64_t)o[q] + 1], c.z[q] = contrib[3 * (int64_t)o[q] + 2];
    }
}

// one wave per listed vertex (wave-uniform loop): per step 256 contributions, lane l loading elements q * 64 + l and
// staging them in the wave's slice of LDS; the corners of step s + 2 and the contributions of step s + 1 are loaded
// before step s is added, element by element, every lane running the same chain on broadcast LDS reads
__global__ __launch_bounds__(BLK) void k_nrm_heavy(const double *contrib, const int32_t *order, const int32_t *begin,
                                                   const int32_t *end, const int32_t *heavy, const uint32_t *status,
                                                   double *out) {
    constexpr int64_t STEP = HCHUNK * 64;
    __shared__ double lds[BLK / 64][3][STEP];
    const int lane = (int)(threadIdx.x & 63);
    double *lx = lds[threadIdx.x >> 6][0], *ly = lds[threadIdx.x >> 6][1], *lz = lds[threadIdx.x >> 6][2];
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nh = (int64_t)status[1];
    for (int64_t h = wave; h < nh; h += n_waves) {
        const int32_t v = heavy[h];
        const int32_t b = begin[v], e = end[v];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int32_t o[HCHUNK];
        Chunk cur;
        load_order(order, b, e, lane, o);
        load_chunk(contrib, o, cur);
        load_order(order, b + STEP, e, lane, o);
        for (int64_t base = b; base < e; base += STEP) {
#pragma unroll
            for (int q = 0; q < HCHUNK; q++) lx[q * 64 + lane] = cur.x[q], ly[q * 64 + lane] = cur.y[q], lz[q * 64 + lane] = cur.z[q];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            load_chunk(contrib, o, cur);
            load_order(order, base + 2 * STEP, e, lane, o);
            const int32_t cnt = (int32_t)(e - base < STEP ? e - base : STEP);
#pragma unroll 8
            for (int32_t j = 0; j < cnt; j++) sx = sx + lx[j], sy = sy + ly[j], sz = sz + lz[j];
            __builtin_amdgcn_wave_barrier();  // (every lane's reads of this step before the next step's writes)
        }
        if (lane == 0) store3(out, v, finish(V3{sx, sy, sz}));
    }
}
#endif

}  // namespace nrm
}  // namespace tk

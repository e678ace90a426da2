// tk_subdiv.h — Loop subdivision of triangle meshes: what take_hip_subdiv_* and take_hip_scene_subdivide_meshes in front
// of the mesh update compute (include/take_hip.h; specification: DESIGN.md §4s).  Three parts:
//   1. the per-vertex bodies, TK_HD and written once: the kernels at the end of this file run them on the device,
//      tests/subdiv_host runs them in the kernels' loop structure on the host;
//   2. the topology build — edge numbering, refined faces, stencil tables, uvs —, host code that runs once per handle
//      (and for take_hip_subdiv_counts / _topology, which need no GPU);
//   3. the kernels.  Launched from tk_subdiv.hip.
//
// Arithmetic: everything is double; every + - * / is one operation in the order written (-ffp-contract=off); the weights
// are Warren's (no trigonometry); the square root of a normal's length is the only library call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "tk_common.h"

namespace tk {
namespace subdiv {

// One edge of a level's input mesh: its ends lo < hi, the corner opposite it in the lower-numbered face (c) and in the
// higher-numbered one (d; -1: a boundary edge).  16 bytes, aligned: one dwordx4 load per lane.
struct alignas(16) Edge {
    int32_t lo, hi, c, d;
};

// What the position kernels read of one level (device memory; on the host, the builder's vectors).
struct LevelView {
    int64_t n_vertices, n_edges;  // of the mesh that goes INTO the level; it leaves with n_vertices + n_edges
    const Edge *edges;            // n_edges, in ascending (lo, hi) order
    const int32_t *nbr_start;     // n_vertices + 1: the rows of nbr
    const int32_t *nbr;           // every vertex's neighbours, ascending
    const int32_t *bnd;           // n_vertices x 2: the two boundary neighbours b0 < b1, or (-1, -1) off the boundary
};

// ---------------------------------------------------------------------------------------------- 1. the bodies
// Even vertex v of a level: in (n_vertices x 3) -> out[3 v ..].
//   on the boundary            0.75 p[v] + 0.125 (p[b0] + p[b1])
//   no face uses it            copied
//   else, n neighbours         s = p[n0]; s = s + p[n1]; ...; (1 - n beta) p[v] + beta s, beta = 3/16 (n = 3), 3 / (8 n)
TK_HD void even_vertex(const LevelView &t, const double *in, int64_t v, double *out) {
    const int32_t b0 = t.bnd[2 * v], b1 = t.bnd[2 * v + 1];
    const int32_t first = t.nbr_start[v], n = t.nbr_start[v + 1] - first;
    double q[3];
    if (b0 >= 0) {
        for (int a = 0; a < 3; a++) q[a] = 0.75 * in[3 * v + a] + 0.125 * (in[3 * (int64_t)b0 + a] + in[3 * (int64_t)b1 + a]);
    } else if (n == 0) {
        for (int a = 0; a < 3; a++) q[a] = in[3 * v + a];
    } else {
        double s[3];
        for (int a = 0; a < 3; a++) s[a] = in[3 * (int64_t)t.nbr[first] + a];
        for (int32_t k = 1; k < n; k++) {
            const int64_t at = 3 * (int64_t)t.nbr[first + k];
            for (int a = 0; a < 3; a++) s[a] = s[a] + in[at + a];
        }
        const double beta = n == 3 ? 0.1875 : 3.0 / (8.0 * (double)n);
        const double keep = 1.0 - (double)n * beta;
        for (int a = 0; a < 3; a++) q[a] = keep * in[3 * v + a] + beta * s[a];
    }
    for (int a = 0; a < 3; a++) out[3 * v + a] = q[a];
}

// The odd vertex of edge e: in -> out[3 (n_vertices + e) ..].
//   interior   0.375 (p[lo] + p[hi]) + 0.125 (p[c] + p[d])
//   boundary   0.5 (p[lo] + p[hi])
TK_HD void odd_vertex(const LevelView &t, const double *in, int64_t e, double *out) {
    const Edge r = t.edges[e];
    const int64_t lo = 3 * (int64_t)r.lo, hi = 3 * (int64_t)r.hi, at = 3 * (t.n_vertices + e);
    double q[3];
    if (r.d >= 0) {
        const int64_t c = 3 * (int64_t)r.c, d = 3 * (int64_t)r.d;
        for (int a = 0; a < 3; a++) q[a] = 0.375 * (in[lo + a] + in[hi + a]) + 0.125 * (in[c + a] + in[d + a]);
    } else {
        for (int a = 0; a < 3; a++) q[a] = 0.5 * (in[lo + a] + in[hi + a]);
    }
    for (int a = 0; a < 3; a++) out[at + a] = q[a];
}

// N_f = cross(p1 - p0, p2 - p0) of face f, not normalised -> fn[3 f ..]
TK_HD void face_normal(const int32_t *indices, const double *p, int64_t f, double *fn) {
    const int64_t i0 = 3 * (int64_t)indices[3 * f], i1 = 3 * (int64_t)indices[3 * f + 1], i2 = 3 * (int64_t)indices[3 * f + 2];
    const double ux = p[i1] - p[i0], uy = p[i1 + 1] - p[i0 + 1], uz = p[i1 + 2] - p[i0 + 2];
    const double vx = p[i2] - p[i0], vy = p[i2 + 1] - p[i0 + 1], vz = p[i2 + 2] - p[i0 + 2];
    fn[3 * f] = uy * vz - uz * vy;
    fn[3 * f + 1] = uz * vx - ux * vz;
    fn[3 * f + 2] = ux * vy - uy * vx;
}

// The normal of vertex v: the sum of its faces' N_f in ascending face order, starting from the first; divided by its
// length when that is positive and finite (tk_skin.h, step 5), else as it is.  A vertex no face uses: (0, 0, 0).
TK_HD void vertex_normal(const int32_t *face_start, const int32_t *faces, const double *fn, int64_t v, double *out) {
    const int32_t first = face_start[v], n = face_start[v + 1] - first;
    double s[3] = {0, 0, 0};
    if (n > 0) {
        for (int a = 0; a < 3; a++) s[a] = fn[3 * (int64_t)faces[first] + a];
        for (int32_t k = 1; k < n; k++) {
            const int64_t at = 3 * (int64_t)faces[first + k];
            for (int a = 0; a < 3; a++) s[a] = s[a] + fn[at + a];
        }
        const double len = tk_sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
        if (len > 0 && len <= 1.7976931348623157e308)  // (finite: neither inf nor NaN)
            for (int a = 0; a < 3; a++) s[a] = s[a] / len;
    }
    for (int a = 0; a < 3; a++) out[3 * v + a] = s[a];
}

// The same normal without a face-normal array: every face's N_f is computed again by each of its three vertices.  The
// operations and their order are vertex_normal's over face_normal's, so the bits are the same.
TK_HD void vertex_normal_recomputed(const int32_t *face_start, const int32_t *faces, const int32_t *indices, const double *p, int64_t v, double *out) {
    const int32_t first = face_start[v], n = face_start[v + 1] - first;
    double s[3] = {0, 0, 0};
    if (n > 0) {
        face_normal(indices + 3 * (int64_t)faces[first], p, 0, s);
        for (int32_t k = 1; k < n; k++) {
            double fn[3];
            face_normal(indices + 3 * (int64_t)faces[first + k], p, 0, fn);
            for (int a = 0; a < 3; a++) s[a] = s[a] + fn[a];
        }
        const double len = tk_sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
        if (len > 0 && len <= 1.7976931348623157e308)
            for (int a = 0; a < 3; a++) s[a] = s[a] / len;
    }
    for (int a = 0; a < 3; a++) out[3 * v + a] = s[a];
}

constexpr int BLOCK = 256;
constexpr int64_t MAX_BLOCKS = 1 << 16;  // a launch's grid: beyond BLOCK * MAX_BLOCKS entries the blocks stride
inline int64_t blocks_for(int64_t n) {
    const int64_t b = (n + BLOCK - 1) / BLOCK;
    return b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b);
}
constexpr int MAX_LEVELS = 6;

// ---------------------------------------------------------------------------------------------- 2. the topology
// The tables of one level, as the builder leaves them in host memory.
struct Level {
    int64_t n_vertices = 0, n_faces = 0, n_edges = 0;  // of the mesh that goes into the level
    std::vector<Edge> edges;
    std::vector<int32_t> nbr_start, nbr, bnd;
    LevelView view() const { return {n_vertices, n_edges, edges.data(), nbr_start.data(), nbr.data(), bnd.data()}; }
};
struct Topology {
    std::vector<Level> levels;
    int64_t n_vertices = 0, n_faces = 0;     // of the refined mesh
    std::vector<int32_t> indices;            // its faces, n_faces x 3
    std::vector<double> uvs;                 // its uvs, n_vertices x 2 (empty: the cage had none)
    std::vector<int32_t> face_start, faces;  // per refined vertex: its incident faces, ascending (n_vertices + 1 rows)
};

enum { TOPOLOGY_OK = 0, TOPOLOGY_INVALID = 1, TOPOLOGY_UNSUPPORTED = 2 };

// A cage of n_vertices vertices and n_faces faces (indices: n_faces x 3; uvs: n_vertices x 2 or null) refined `levels`
// times -> out.  Numbering: the distinct unordered corner pairs (lo < hi) are the edges, 0 .. E-1 in ascending (lo, hi)
// order; even vertex v keeps index v, the odd vertex of edge e is V + e; face f = (a, b, c) becomes
// (a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca) at 4 f .. 4 f + 3.  An odd vertex's uv is 0.5 * (uv[lo] + uv[hi]).
// keep_tables false: counts, indices and uvs alone (take_hip_subdiv_counts / _topology).
// -> TOPOLOGY_OK, or a refusal with its message in `msg`.
inline int build_topology(int64_t n_vertices, int64_t n_faces, const int32_t *indices, const double *uvs, int32_t levels, bool keep_tables, Topology &out,
                          std::string &msg) {
    if (levels < 1 || levels > MAX_LEVELS) return msg = "levels must be 1.." + std::to_string(MAX_LEVELS), TOPOLOGY_INVALID;
    if (n_vertices <= 0 || n_faces <= 0) return msg = "n_vertices and n_faces must be positive", TOPOLOGY_INVALID;
    if (n_vertices > INT32_MAX || 3 * n_faces > INT32_MAX) return msg = "unsupported: a cage beyond 32-bit indices", TOPOLOGY_UNSUPPORTED;
    if (3 * (n_faces << (2 * levels)) > INT32_MAX)
        return msg = "unsupported: " + std::to_string(n_faces << (2 * levels)) + " refined faces are beyond 32-bit indices", TOPOLOGY_UNSUPPORTED;
    struct Half {  // one side of a face: its edge's key, the face, the opposite corner, where the face finds the edge
        uint64_t key;
        int32_t face, opposite, slot;
    };
    std::vector<int32_t> idx(indices, indices + 3 * n_faces), next;
    std::vector<double> uv, uv_next;
    if (uvs) uv.assign(uvs, uvs + 2 * n_vertices);
    std::vector<Half> halves;
    std::vector<int32_t> edge_of, below;
    int64_t V = n_vertices, F = n_faces;
    out = Topology();
    for (int32_t level = 0; level < levels; level++) {
        const std::string who = "level " + std::to_string(level) + ": ";
        halves.resize(3 * (size_t)F);
        for (int64_t f = 0; f < F; f++) {
            const int32_t *t = &idx[3 * f];
            for (int k = 0; k < 3; k++)
                if (t[k] < 0 || t[k] >= V)
                    return msg = who + "face " + std::to_string(f) + ": vertex index " + std::to_string(t[k]) + " out of range", TOPOLOGY_INVALID;
            if (t[0] == t[1] || t[1] == t[2] || t[2] == t[0])
                return msg = who + "face " + std::to_string(f) + " repeats vertex " + std::to_string(t[0] == t[1] || t[0] == t[2] ? t[0] : t[1]), TOPOLOGY_INVALID;
            for (int k = 0; k < 3; k++) {  // side k: corners k and k + 1, opposite corner k + 2
                const int32_t a = t[k], b = t[(k + 1) % 3];
                const uint64_t lo = (uint64_t)(a < b ? a : b), hi = (uint64_t)(a < b ? b : a);
                halves[3 * f + k] = Half{(lo << 32) | hi, (int32_t)f, t[(k + 2) % 3], (int32_t)(3 * f + k)};
            }
        }
        std::sort(halves.begin(), halves.end(), [](const Half &x, const Half &y) { return x.key != y.key ? x.key < y.key : x.face < y.face; });
        Level lv;
        lv.n_vertices = V, lv.n_faces = F;
        edge_of.resize(3 * (size_t)F);
        for (size_t i = 0; i < halves.size();) {
            size_t j = i + 1;
            while (j < halves.size() && halves[j].key == halves[i].key) j++;
            const int32_t lo = (int32_t)(halves[i].key >> 32), hi = (int32_t)(halves[i].key & 0xffffffffu);
            if (j - i > 2) return msg = who + "edge (" + std::to_string(lo) + ", " + std::to_string(hi) + ") has more than two faces", TOPOLOGY_INVALID;
            for (size_t k = i; k < j; k++) edge_of[halves[k].slot] = (int32_t)lv.edges.size();
            lv.edges.push_back(Edge{lo, hi, halves[i].opposite, j - i == 2 ? halves[i + 1].opposite : -1});
            i = j;
        }
        const int64_t E = lv.n_edges = (int64_t)lv.edges.size();
        if (V + E > INT32_MAX) return msg = "unsupported: " + std::to_string(V + E) + " refined vertices are beyond 32-bit indices", TOPOLOGY_UNSUPPORTED;
        // neighbours: vertex v's row is [the lo of every edge whose hi is v | the hi of every edge whose lo is v], each
        // part ascending because the edges are, the first part below v and the second above
        lv.nbr_start.assign((size_t)V + 1, 0);
        below.assign((size_t)V, 0);
        for (const Edge &e : lv.edges) lv.nbr_start[e.lo + 1]++, lv.nbr_start[e.hi + 1]++, below[e.hi]++;
        for (int64_t v = 0; v < V; v++) lv.nbr_start[v + 1] += lv.nbr_start[v];
        lv.nbr.resize(2 * (size_t)E);
        lv.bnd.assign(2 * (size_t)V, -1);
        std::vector<int32_t> at_lo(lv.nbr_start.begin(), lv.nbr_start.end() - 1), at_hi((size_t)V), on_boundary((size_t)V, 0);
        for (int64_t v = 0; v < V; v++) at_hi[v] = lv.nbr_start[v] + below[v];
        for (const Edge &e : lv.edges) {
            lv.nbr[at_lo[e.hi]++] = e.lo, lv.nbr[at_hi[e.lo]++] = e.hi;
            if (e.d < 0)
                for (int side = 0; side < 2; side++) {
                    const int32_t v = side ? e.hi : e.lo, other = side ? e.lo : e.hi;
                    if (on_boundary[v] < 2) lv.bnd[2 * v + on_boundary[v]] = other;
                    on_boundary[v]++;
                }
        }
        for (int64_t v = 0; v < V; v++)
            if (on_boundary[v] != 0 && on_boundary[v] != 2)
                return msg = who + "vertex " + std::to_string(v) + " is on " + std::to_string(on_boundary[v]) + " boundary edges, not two (a bow-tie)", TOPOLOGY_INVALID;
        // the refined faces and uvs
        next.resize(12 * (size_t)F);
        for (int64_t f = 0; f < F; f++) {
            const int32_t a = idx[3 * f], b = idx[3 * f + 1], c = idx[3 * f + 2];
            const int32_t ab = (int32_t)(V + edge_of[3 * f]), bc = (int32_t)(V + edge_of[3 * f + 1]), ca = (int32_t)(V + edge_of[3 * f + 2]);
            const int32_t four[12] = {a, ab, ca, ab, b, bc, ca, bc, c, ab, bc, ca};
            std::copy(four, four + 12, &next[12 * f]);
        }
        if (uvs) {
            uv_next.assign(uv.begin(), uv.end());
            uv_next.resize(2 * (size_t)(V + E));
            for (int64_t e = 0; e < E; e++)
                for (int a = 0; a < 2; a++) uv_next[2 * (V + e) + a] = 0.5 * (uv[2 * (size_t)lv.edges[e].lo + a] + uv[2 * (size_t)lv.edges[e].hi + a]);
            uv.swap(uv_next);
        }
        idx.swap(next);
        V += E, F *= 4;
        if (keep_tables) {
            out.levels.push_back(std::move(lv));
        } else {
            Level counts;
            counts.n_vertices = lv.n_vertices, counts.n_faces = lv.n_faces, counts.n_edges = lv.n_edges;
            out.levels.push_back(std::move(counts));
        }
    }
    out.n_vertices = V, out.n_faces = F;
    out.indices.swap(idx);
    out.uvs.swap(uv);
    if (keep_tables) {  // (faces are walked in ascending order: so is every vertex's row)
        out.face_start.assign((size_t)V + 1, 0);
        for (int32_t i : out.indices) out.face_start[i + 1]++;
        for (int64_t v = 0; v < V; v++) out.face_start[v + 1] += out.face_start[v];
        out.faces.resize(3 * (size_t)F);
        std::vector<int32_t> at(out.face_start.begin(), out.face_start.end() - 1);
        for (int64_t f = 0; f < F; f++)
            for (int k = 0; k < 3; k++) out.faces[at[out.indices[3 * f + k]]++] = (int32_t)f;
    }
    return TOPOLOGY_OK;
}

// ---------------------------------------------------------------------------------------------- 3. the kernels
#if defined(__HIPCC__)
// (The byte figures in these comments are counted from the layout, not measured.)
// One lane per even vertex, consecutive lanes consecutive vertices: a wave reads 1536 contiguous bytes of its own
// positions, 256 + 512 of the row starts and boundary pairs, and writes 1536; the neighbours' positions are the gather —
// 24-byte records by vertex index, about six per lane.  Even and odd vertices are separate launches, so every wave runs
// one rule's loop.
__global__ __launch_bounds__(BLOCK) void k_subdiv_even(LevelView t, const double *__restrict__ in, double *__restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < t.n_vertices; v += (int64_t)gridDim.x * BLOCK) even_vertex(t, in, v, out);
}
// One lane per edge: one 16-byte record (a wave: 1024 contiguous bytes), four 24-byte gathers — lo ascends along the
// wave, hi, c and d are near it in a mesh numbered with any locality —, 1536 contiguous bytes written.
__global__ __launch_bounds__(BLOCK) void k_subdiv_odd(LevelView t, const double *__restrict__ in, double *__restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < t.n_edges; e += (int64_t)gridDim.x * BLOCK) odd_vertex(t, in, e, out);
}
// one lane per refined face: 12 bytes of indices, three 24-byte gathers, 24 written
__global__ __launch_bounds__(BLOCK) void k_subdiv_face_normals(const int32_t *__restrict__ indices, const double *__restrict__ p, int64_t n_faces, double *__restrict__ fn) {
    for (int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * BLOCK) face_normal(indices, p, f, fn);
}
// one lane per refined vertex: its row of faces (about six), a 24-byte gather each, 24 written; no atomics — the order
// of the sum is the row's
__global__ __launch_bounds__(BLOCK) void k_subdiv_vertex_normals(const int32_t *__restrict__ face_start, const int32_t *__restrict__ faces, const double *__restrict__ fn,
                                                                 int64_t n_vertices, double *__restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < n_vertices; v += (int64_t)gridDim.x * BLOCK) vertex_normal(face_start, faces, fn, v, out);
}
// the variant without the face-normal array (TAKE_HIP_SUBDIV_NORMALS=recompute; DESIGN.md §4s has the timings of both):
// per face of the row 4 + 12 bytes of indices and three 24-byte gathers
__global__ __launch_bounds__(BLOCK) void k_subdiv_vertex_normals_recomputed(const int32_t *__restrict__ face_start, const int32_t *__restrict__ faces,
                                                                            const int32_t *__restrict__ indices, const double *__restrict__ p, int64_t n_vertices,
                                                                            double *__restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x; v < n_vertices; v += (int64_t)gridDim.x * BLOCK) vertex_normal_recomputed(face_start, faces, indices, p, v, out);
}
#endif  // __HIPCC__

}  // namespace subdiv
}  // namespace tk

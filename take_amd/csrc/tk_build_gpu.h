// tk_build_gpu.h — BVH construction on the device (f32 and f64 sides of a scene): the GPU counterpart of
// `construct_bvh` (src/bvh.cpp:8-45) for scenes where the host SAH build is the wait (10M triangles: ~6 s on 16 cores).
// The kernels; the host driver that launches them is tk_build.hip, the only unit that includes this header.
//
//   k_make_prims     primitive records, float or double, from the caller's mesh arrays
//   k_make_proto_prims  the same for a prototype mesh of a two-level scene: object space, shape_id = face
//   k_prim_boxes     primitive AABBs (of the geometry the intersection tests see: v0, v0+e1, v0+e2 — one ulp wider;
//                    double records: rounded outwards to float first) + scene bounds (wave reduce, ordered-int atomics)
//   k_morton         63-bit Morton code of the box centre (21 bits per axis: 30 bits leave whole clusters of a 10M-
//                    triangle scene in one cell); rocPRIM radix sort of (code, primitive) pairs
//   k_leaves         leaves = runs of `leaf_size` consecutive primitives in Morton order
//   k_hierarchy      Karras 2012: every internal node finds its key range and split in parallel
//   k_refit          bottom-up boxes, second arrival at a node computes it (agent-scope fences around the flag)
//   k_collapse       BVH2 -> 4-wide nodes, level by level (k_collapse_count, a scan, k_collapse), breadth-first
//                    numbering in the order of the parents (same layout and the same "open the child with the largest
//                    area" rule as the host collapse, tk_bvh.h); no atomic counter: the nodes are reproducible
//   k_quantise       64-byte compressed nodes on the 15-bit scene grid (same rounding rules as quantise_nodes)
//   k_widen_nodes    double scenes without compression: the float nodes as Node4<double>
//   k_permute        primitive and shading records into leaf order
// Two-level scenes (TakeInstance) add
//   k_placement_boxes   tight world box of every placement: its prototype's vertices under the transform, in double
//   k_placement_pad     the padded float box of a placement, behind the shapes' boxes of the top-level build
//   k_flag_shapes / k_top_leaves / k_permute_top   the top-level tree's leaves: a placement becomes an instance word,
//                    the shapes' records are compacted into leaf order
//   k_rebase         a prototype tree's child words (local node indices, local leaf ranges) -> the scene's arrays
// Re-posing the placements of a resident two-level scene (take_hip_scene_set_instance_transforms) adds
//   k_placement_records          the placements' InstTrace / InstShade records under new transforms
//   k_placement_boxes_resident   their tight world boxes from the prototypes' records in the scene, k_widen_tight
//   k_shift_roots                the placements' roots after the top-level tree changed its size
// Moving the vertices of meshes of a resident scene (take_hip_scene_set_mesh_vertices) adds
//   k_update_prims     the resident records back into shape order, updated meshes' triangles with new geometry words
//   k_convert_normals / k_update_lights   new vertex normals as R; the records of area lights on updated faces
// Moving the vertices of prototype meshes of a resident two-level scene (take_hip_scene_update_meshes) adds
//   k_update_proto_prims     a moved prototype's object-space records from its new positions, with the finiteness check
//   k_retarget_placements    the placements' roots (every prototype's nodes may move) and the moved prototypes' grids
// Following moved vertices in the motion pass (take_hip_scene_track_vertices) adds
//   k_copy_marked      the geometry words of the records an update is about to replace, by record identity
//
// The tree is an LBVH: built in milliseconds, but without the SAH its boxes overlap more, so traversal visits more
// nodes than with the host build (numbers in DESIGN.md).  Results do not depend on the tree (conservative box
// tests): the parity tests require bit-identical hit tables and images for both builders.
//
// Double scenes.  Only the records and the primitive boxes know the precision: every box of the pipeline is a float
// box (a conservative box test may be done in any precision), and a float box around double geometry is
// what k_prim_boxes<double> makes.  Everything after it is the f32 pipeline, float nodes included; the full-width
// fall-back of a double scene (Node4<double>) is those nodes widened to double by k_widen_nodes, which is exact.
#pragma once

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <cmath>
#include <limits>

#include "tk_bvh.h"
#include "tk_motion_pixel.h"
#include "tk_round.h"
#include "tk_scene.h"

namespace tk {
namespace lbvh {

constexpr int BLK = 256;
constexpr int MAX_LEVELS = (MAX_STACK_ENTRIES - 1) / 3;  // 4-wide levels the traversal stack can take

struct Box {
    float lo[3], hi[3];
};

// floats as integers with the same order (for atomicMin / atomicMax)
__host__ __device__ __forceinline__ int f2ord(float f) {
    int i;
    __builtin_memcpy(&i, &f, 4);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float ord2f(int i) {
    i = i >= 0 ? i : i ^ 0x7fffffff;
    float f;
    __builtin_memcpy(&f, &i, 4);
    return f;
}
__device__ __forceinline__ Box box_union(const Box &a, const Box &b) {
    Box r;
#pragma unroll
    for (int k = 0; k < 3; k++) r.lo[k] = fminf(a.lo[k], b.lo[k]), r.hi[k] = fmaxf(a.hi[k], b.hi[k]);
    return r;
}
__device__ __forceinline__ float half_area(const Box &b) {
    const float x = b.hi[0] - b.lo[0], y = b.hi[1] - b.lo[1], z = b.hi[2] - b.lo[2];
    return x * y + y * z + z * x;
}

// ---- primitive records straight from the caller's mesh arrays (parser -> device buffers).
// The same arithmetic as the host loop of tk_host_scene.h (triangle_record<R>, shape_record<R>: positions taken as R,
// e_k = v_k - v0 in R, no contraction), so the records — and with them every hit — are bit-identical to the host-built
// ones in float and in double.
struct MeshSrc {
    int64_t pos_off;   // first vertex of this mesh in the concatenated double positions (units: vertices)
    int32_t fbase;     // first face in face_idx (units: faces)
    int32_t material;
    int32_t tag;       // material tag
    int32_t has_attr;  // vertex normals and/or uvs exist
};
struct SphereSrc {
    double c[3], r;
    int32_t material, tag;
};
// The geometry words of a triangle record (a[9]: v0, e1, e2) from the mesh's double positions (its vertex 0 first) and
// the face's three vertex ids.  The one place this arithmetic lives on the device: a new scene's records
// (triangle_into) and the records of a resident scene whose vertices moved (k_update_prims) are made by it.
template <class R> __device__ __forceinline__ void triangle_geometry(R *a9, const double *__restrict__ mesh_positions, const int32_t *__restrict__ idx) {
    R v[3][3];
    for (int k = 0; k < 3; k++)
        for (int a = 0; a < 3; a++) v[k][a] = (R)mesh_positions[3 * (int64_t)idx[k] + a];
    for (int a = 0; a < 3; a++) a9[a] = v[0][a], a9[3 + a] = v[1][a] - v[0][a], a9[6 + a] = v[2][a] - v[0][a];
}
// triangle `face` of mesh `mesh_id` (m) into p: geometry, the mesh's material, its attribute index
template <class R>
__device__ __forceinline__ void triangle_into(PrimRec<R> &p, const MeshSrc &m, int32_t mesh_id, int32_t face, const double *__restrict__ positions,
                                              const int32_t *__restrict__ face_idx) {
    triangle_geometry(p.a, positions + 3 * m.pos_off, face_idx + 3 * ((int64_t)m.fbase + face));
    p.meta = PRIM_TRIANGLE | (m.tag << 8);
    p.material = m.material;
    p.mesh = mesh_id;
    if (m.has_attr) p.nidx = m.fbase + face, p.meta |= META_HAS_ATTR;
}
template <class R>
__global__ void __launch_bounds__(BLK)
k_make_prims(const int32_t *__restrict__ kind, const int32_t *__restrict__ ref, const int32_t *__restrict__ face,
             const int32_t *__restrict__ area_light, const MeshSrc *__restrict__ meshes, const double *__restrict__ positions,
             const int32_t *__restrict__ face_idx, const SphereSrc *__restrict__ spheres, int n, PrimRec<R> *out) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    PrimRec<R> p{};
    p.shape_id = i;
    p.area_light = area_light[i];
    p.nidx = -1;
    if (kind[i] == 0) {
        const SphereSrc s = spheres[ref[i]];
        p.a[0] = (R)s.c[0], p.a[1] = (R)s.c[1], p.a[2] = (R)s.c[2], p.a[3] = (R)s.r;
        p.meta = PRIM_SPHERE | (s.tag << 8);
        p.material = s.material;
        p.mesh = -(1 + ref[i]);
    } else {
        triangle_into(p, meshes[ref[i]], ref[i], face[i], positions, face_idx);
    }
    out[i] = p;
}
// The records of a prototype mesh (two-level scenes), in object space and in face order: what Prototype::build
// (tk_host_scene.h) makes with triangle_record — the shape id is the face (InstShade::shape_base is added at a hit),
// no area light.
template <class R>
__global__ void __launch_bounds__(BLK)
k_make_proto_prims(MeshSrc m, int32_t mesh_id, const double *__restrict__ positions, const int32_t *__restrict__ face_idx, int n_faces, PrimRec<R> *out) {
    const int f = blockIdx.x * BLK + threadIdx.x;
    if (f >= n_faces) return;
    PrimRec<R> p{};
    p.shape_id = f;
    p.area_light = -1;
    p.nidx = -1;
    triangle_into(p, m, mesh_id, f, positions, face_idx);
    out[f] = p;
}

// One coordinate interval [lo, hi] of a record's geometry -> a float interval that contains it.
// float records: the sums v0 + e_k and c -+ r round by at most half an ulp, so one float further out contains them.
// double records: the geometry the intersection tests see is the REAL triangle v0 + u e1 + v e2 (real sphere |x - c|
// = r) of the stored doubles; its extreme coordinates are the real numbers v0, v0 + e1, v0 + e2 (c -+ r), of which
// the double sums computed here are within half a DOUBLE ulp.  d2f_down / d2f_up (tk_round.h) give floats lo' <= the
// computed minimum and hi' >= the computed maximum, whatever the magnitude — far from the origin a rounding to nearest
// would land inside the triangle by up to half a float ulp, which is the case this exists for — and the one float
// further out that the f32 path also takes is 2^29 double ulps: more than the half ulp the real sums can lie beyond
// the computed ones.  (The caller's v1, v2 need not be looked at: e_k = fl(v_k - v0) makes v0 + e_k differ from v_k by
// a rounding, but only v0 + e_k is geometry to any test.)
__device__ __forceinline__ void widen(float lo, float hi, float &blo, float &bhi) { blo = f_below(lo), bhi = f_above(hi); }
__device__ __forceinline__ void widen(double lo, double hi, float &blo, float &bhi) { blo = f_below(d2f_down(lo)), bhi = f_above(d2f_up(hi)); }

// scene_ord[0..2] = min of lo (ordered ints), [3..5] = max of hi; initialised to INT_MAX / INT_MIN by the caller.
// With outward-rounded boxes the float scene bounds contain the double scene, so the grid make_qgrid lays over them
// and QRay's 2^-20-extent slack (tk_traverse.h) are what the host path gives an f64 scene: the same argument holds.
template <class R>
__global__ void __launch_bounds__(BLK) k_prim_boxes(const PrimRec<R> *__restrict__ prims, int n, Box *pb, int *scene_ord) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    Box b;
#pragma unroll
    for (int k = 0; k < 3; k++) b.lo[k] = __builtin_huge_valf(), b.hi[k] = -__builtin_huge_valf();
    if (i < n) {
        const PrimRec<R> p = prims[i];
        if ((p.meta & 0xff) == PRIM_TRIANGLE) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const R v0 = p.a[k], v1 = p.a[k] + p.a[3 + k], v2 = p.a[k] + p.a[6 + k];
                widen(tk_fmin(v0, tk_fmin(v1, v2)), tk_fmax(v0, tk_fmax(v1, v2)), b.lo[k], b.hi[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) widen(p.a[k] - p.a[3], p.a[k] + p.a[3], b.lo[k], b.hi[k]);
        }
        pb[i] = b;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float lo = b.lo[k], hi = b.hi[k];
        for (int off = 32; off > 0; off >>= 1) lo = fminf(lo, __shfl_xor(lo, off)), hi = fmaxf(hi, __shfl_xor(hi, off));
        if ((threadIdx.x & 63) == 0 && lo <= hi) {
            atomicMin(&scene_ord[k], f2ord(lo));
            atomicMax(&scene_ord[3 + k], f2ord(hi));
        }
    }
}

__device__ __forceinline__ uint64_t expand21(uint64_t v) {  // 21 bits -> every third bit
    v &= 0x1FFFFFull;
    v = (v | (v << 32)) & 0x001F00000000FFFFull;
    v = (v | (v << 16)) & 0x001F0000FF0000FFull;
    v = (v | (v << 8)) & 0x100F00F00F00F00Full;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}
__global__ void __launch_bounds__(BLK) k_morton(const Box *__restrict__ pb, int n, const int *__restrict__ scene_ord, uint64_t *keys, uint32_t *vals) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const Box b = pb[i];
    uint64_t q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = ord2f(scene_ord[k]), hi = ord2f(scene_ord[3 + k]);
        const float ext = hi - lo;
        const float t = ext > 0.0f ? (0.5f * (b.lo[k] + b.hi[k]) - lo) / ext : 0.0f;
        q[k] = (uint64_t)fminf(fmaxf(t * 2097152.0f, 0.0f), 2097151.0f);
    }
    keys[i] = (expand21(q[0]) << 2) | (expand21(q[1]) << 1) | expand21(q[2]);
    vals[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(BLK) k_leaves(const Box *__restrict__ pb, const uint64_t *__restrict__ keys_sorted, const uint32_t *__restrict__ vals_sorted,
                                                 int n, int leaf_size, int n_leaves, Box *lbox, uint64_t *lkey) {
    const int l = blockIdx.x * BLK + threadIdx.x;
    if (l >= n_leaves) return;
    const int first = l * leaf_size, cnt = min(leaf_size, n - first);
    Box b = pb[vals_sorted[first]];
    for (int k = 1; k < cnt; k++) b = box_union(b, pb[vals_sorted[first + k]]);
    lbox[l] = b;
    lkey[l] = keys_sorted[first];
}

// common-prefix length of leaf keys i and j (ties broken by the leaf index), -1 outside the array
__device__ __forceinline__ int prefix_len(const uint64_t *__restrict__ k, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t a = k[i], b = k[j];
    return a == b ? 64 + __clz((uint32_t)(i ^ j)) : __clzll((long long)(a ^ b));
}
// child reference: >= 0 internal node, < 0 leaf ~l.  parent_i[0] = -1 (root = internal node 0).
__global__ void __launch_bounds__(BLK) k_hierarchy(const uint64_t *__restrict__ lkey, int n_leaves, int2 *child, int *parent_i, int *parent_l) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n_leaves - 1) return;
    const int d = prefix_len(lkey, n_leaves, i, i + 1) - prefix_len(lkey, n_leaves, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = prefix_len(lkey, n_leaves, i, i - d);
    int lmax = 2;
    while (prefix_len(lkey, n_leaves, i, i + lmax * d) > dmin) lmax *= 2;
    int len = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (prefix_len(lkey, n_leaves, i, i + (len + t) * d) > dmin) len += t;
    const int j = i + len * d;
    const int dnode = prefix_len(lkey, n_leaves, i, j);
    int s = 0, t = len;
    do {
        t = (t + 1) >> 1;
        if (prefix_len(lkey, n_leaves, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + min(d, 0);
    const int lo = min(i, j), hi = max(i, j);
    const int left = lo == gamma ? ~gamma : gamma, right = hi == gamma + 1 ? ~(gamma + 1) : gamma + 1;
    child[i] = make_int2(left, right);
    if (left >= 0) parent_i[left] = i; else parent_l[~left] = i;
    if (right >= 0) parent_i[right] = i; else parent_l[~right] = i;
    if (i == 0) parent_i[0] = -1;
}

// flag[] zeroed by the caller.  A box written on one CU is read on another: release before the flag, acquire after
// it (a CU's vector L1 is not refreshed by other CUs' stores, MI355X_MICROARCH.md).
__global__ void __launch_bounds__(BLK) k_refit(int n_leaves, const int2 *__restrict__ child, const int *__restrict__ parent_i, const int *__restrict__ parent_l,
                                                const Box *lbox, Box *ibox, int *flag) {
    const int l = blockIdx.x * BLK + threadIdx.x;
    if (l >= n_leaves) return;
    int p = parent_l[l];
    while (p >= 0) {
        __threadfence();
        if (atomicAdd(&flag[p], 1) == 0) return;  // the sibling subtree is not done: its last thread will come by
        __threadfence();
        const int2 c = child[p];
        const Box a = c.x < 0 ? lbox[~c.x] : ibox[c.x], b = c.y < 0 ? lbox[~c.y] : ibox[c.y];
        ibox[p] = box_union(a, b);
        p = parent_i[p];
    }
}

// The up to four children a wide node gets from BVH2 node `node`: its two children, then the interior child with the
// largest surface area opened until there are four (or none is interior).  -> their number.
__device__ __forceinline__ int wide_children(int node, const int2 *__restrict__ child, const Box *__restrict__ ibox, int kids[4]) {
    const int2 c = child[node];
    int nk = 2;
    kids[0] = c.x, kids[1] = c.y, kids[2] = 0, kids[3] = 0;
    while (nk < 4) {  // open the interior child with the largest surface area
        int best = -1;
        float best_area = -1.0f;
        for (int i = 0; i < nk; i++)
            if (kids[i] >= 0) {
                const float a = half_area(ibox[kids[i]]);
                if (a > best_area) best_area = a, best = i;
            }
        if (best < 0) break;
        const int2 g = child[kids[best]];
        kids[best] = g.x;
        kids[nk++] = g.y;
    }
    return nk;
}
// One tree level of the collapse, in two launches around an exclusive scan.  The level's n_in wide nodes are made from
// the BVH2 nodes frontier_in[0 .. n_in); node index = first (the nodes on earlier levels) + position in the frontier.
// k_collapse_count: cnt[idx] = the interior children of node idx.  Their exclusive scan `off` numbers the next level's
// nodes in the order of their parents — no atomic counter, so the node array is a function of the records alone: two
// builds of the same input leave the same bytes (a scene whose vertices moved is compared with a fresh build byte for
// byte, tests/test_gpu_mesh_update.py).  k_collapse writes the nodes, the next frontier and its size.
__global__ void __launch_bounds__(BLK) k_collapse_count(const int *__restrict__ frontier_in, int n_in, const int2 *__restrict__ child,
                                                         const Box *__restrict__ ibox, int *cnt) {
    const int idx = blockIdx.x * BLK + threadIdx.x;
    if (idx >= n_in) return;
    int kids[4], n_int = 0;
    const int nk = wide_children(frontier_in[idx], child, ibox, kids);
    for (int i = 0; i < nk; i++) n_int += kids[i] >= 0;
    cnt[idx] = n_int;
}
__global__ void __launch_bounds__(BLK) k_collapse(const int *__restrict__ frontier_in, int n_in, int first, const int *__restrict__ off, int *frontier_out,
                                                   int *n_out, const int2 *__restrict__ child, const Box *__restrict__ ibox, const Box *__restrict__ lbox,
                                                   int leaf_size, int n_prims, Node4<float> *nodes) {
    const int idx = blockIdx.x * BLK + threadIdx.x;
    if (idx >= n_in) return;
    int kids[4];
    const int nk = wide_children(frontier_in[idx], child, ibox, kids);
    // slot order = visiting order of the (unranked) shadow-ray traversal: largest box first (tk_bvh.h)
    float ar[4];
    for (int i = 0; i < nk; i++) ar[i] = half_area(kids[i] >= 0 ? ibox[kids[i]] : lbox[~kids[i]]);
    for (int i = 1; i < nk; i++)
        for (int j = i; j > 0 && ar[j] > ar[j - 1]; j--) {
            const float ta = ar[j];
            ar[j] = ar[j - 1], ar[j - 1] = ta;
            const int tk = kids[j];
            kids[j] = kids[j - 1], kids[j - 1] = tk;
        }
    const int next_first = first + n_in;  // the next level's first node
    int next = off[idx];
    Node4<float> nd;
    for (int i = 0; i < 4; i++) {
        NodeChild<float> &o = nd.c[i];
        o.pad = 0;
        if (i < nk) {
            const int k = kids[i];
            const Box b = k >= 0 ? ibox[k] : lbox[~k];
            for (int a = 0; a < 3; a++) o.bmin[a] = b.lo[a], o.bmax[a] = b.hi[a];
            if (k >= 0) {
                frontier_out[next] = k;
                o.child = next_first + next;
                next++;
            } else {
                const int first_prim = (~k) * leaf_size;
                o.child = make_leaf(first_prim, min(leaf_size, n_prims - first_prim));
            }
        } else {
            for (int a = 0; a < 3; a++) o.bmin[a] = __builtin_huge_valf(), o.bmax[a] = -__builtin_huge_valf();
            o.child = CHILD_EMPTY;
        }
    }
    nodes[first + idx] = nd;
    if (idx == n_in - 1) *n_out = next;  // the size of the next level
}

// acc[0] += sum of min(decoded area / true area, 100) over child boxes, acc[1] += number of child boxes
__global__ void __launch_bounds__(BLK) k_quantise(const Node4<float> *__restrict__ nodes, int n, QGrid g, QNode4 *out, double *acc) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    double ratio = 0, slots = 0;
    if (i < n) {
        const Node4<float> nd = nodes[i];
        QNode4 q;
        for (int c = 0; c < 4; c++) {
            q.c[c].child = nd.c[c].child;
            q.c[c].q[0] = q.c[c].q[1] = q.c[c].q[2] = (uint32_t)Q_MAX;  // empty slot: inverted box (tk_bvh.h: quantise_nodes)
            if (nd.c[c].child == CHILD_EMPTY) continue;
            double et[3], eq[3];
            for (int a = 0; a < 3; a++) {
                long long ql, qh;
                qgrid_snap(g, a, (double)nd.c[c].bmin[a] - g.delta[a], (double)nd.c[c].bmax[a] + g.delta[a], ql, qh);
                q.c[c].q[a] = (uint32_t)ql | ((uint32_t)qh << 16);
                et[a] = (double)nd.c[c].bmax[a] - (double)nd.c[c].bmin[a];
                eq[a] = (double)(qh - ql) * (double)g.step[a];
            }
            const double at = et[0] * et[1] + et[1] * et[2] + et[2] * et[0], aq = eq[0] * eq[1] + eq[1] * eq[2] + eq[2] * eq[0];
            ratio += at > 0 ? fmin(aq / at, 100.0) : (aq > 0 ? 100.0 : 1.0);
            slots += 1;
        }
        out[i] = q;
    }
    for (int off = 32; off > 0; off >>= 1) ratio += __shfl_xor(ratio, off), slots += __shfl_xor(slots, off);
    if ((threadIdx.x & 63) == 0 && slots > 0) {
        atomicAdd(&acc[0], ratio);
        atomicAdd(&acc[1], slots);
    }
}

// Full-width nodes of a double scene (compression refused): the float planes as doubles — the same numbers, so the
// boxes contain what they contained; an empty slot's infinities stay infinities.
__global__ void __launch_bounds__(BLK) k_widen_nodes(const Node4<float> *__restrict__ in, int n, Node4<double> *out) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const Node4<float> a = in[i];
    Node4<double> b;
    for (int c = 0; c < 4; c++) {
        for (int k = 0; k < 3; k++) b.c[c].bmin[k] = (double)a.c[c].bmin[k], b.c[c].bmax[k] = (double)a.c[c].bmax[k];
        b.c[c].child = a.c[c].child, b.c[c].pad = 0;
    }
    out[i] = b;
}

template <class T>
__global__ void __launch_bounds__(BLK) k_permute(const T *__restrict__ in, const uint32_t *__restrict__ order, int n, T *out) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < n) out[i] = in[order[i]];
}
__global__ void k_fill_int(int *p, int n, int v) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < n) p[i] = v;
}


// ---- two-level scenes: placement boxes, the top-level tree's leaves, assembly
// doubles as 64-bit integers with the same order (atomicMin / atomicMax on long long)
__host__ __device__ __forceinline__ long long d2ord(double d) {
    long long i;
    __builtin_memcpy(&i, &d, 8);
    return i >= 0 ? i : i ^ 0x7fffffffffffffffll;
}
__host__ __device__ __forceinline__ double ord2d(long long i) {
    i = i >= 0 ? i : i ^ 0x7fffffffffffffffll;
    double d;
    __builtin_memcpy(&d, &i, 8);
    return d;
}
constexpr int PLACEMENT_CHUNK = 16 * BLK;  // vertices one block of k_placement_boxes transforms

// tight[6 i .. 6 i + 5] = ordered (min x y z, max x y z) of placement i's box, initialised to LLONG_MAX / LLONG_MIN by
// the caller.  One launch per prototype: block b transforms chunk b % chunks of the prototype's vertices (pos: its
// first vertex, n_vertices of them) under the transform of placement ids[b / chunks].  The image of a vertex is
// Affine3::image's expression (tk_host_scene.h), operand order included, and the build does not contract: min and max
// are exact and commute, so the box is the one placement_box computes on the host, to the sign of a zero.
__global__ void __launch_bounds__(BLK) k_placement_boxes(const double *__restrict__ pos, int64_t n_vertices, int chunks, const int32_t *__restrict__ ids,
                                                          const double *__restrict__ xforms, long long *tight) {
    __shared__ double part[BLK / 64][6];
    const int32_t pl = ids[blockIdx.x / (unsigned)chunks];
    const double *M = xforms + 12 * (int64_t)pl;
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = M[k];
    double lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) lo[a] = __builtin_huge_val(), hi[a] = -__builtin_huge_val();
    const int64_t v0 = (int64_t)(blockIdx.x % (unsigned)chunks) * PLACEMENT_CHUNK, v1 = min(n_vertices, v0 + PLACEMENT_CHUNK);
    for (int64_t v = v0 + threadIdx.x; v < v1; v += BLK) {
        const double px = pos[3 * v], py = pos[3 * v + 1], pz = pos[3 * v + 2];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double w = m[4 * a] * px + m[4 * a + 1] * py + m[4 * a + 2] * pz + m[4 * a + 3];
            lo[a] = fmin(lo[a], w), hi[a] = fmax(hi[a], w);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        for (int off = 32; off > 0; off >>= 1) lo[a] = fmin(lo[a], __shfl_xor(lo[a], off)), hi[a] = fmax(hi[a], __shfl_xor(hi[a], off));
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][a] = lo[a], part[threadIdx.x >> 6][3 + a] = hi[a];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        double l = part[0][a], h = part[0][3 + a];
        for (int w = 1; w < BLK / 64; w++) l = fmin(l, part[w][a]), h = fmax(h, part[w][3 + a]);
        if (l <= h) {
            atomicMin(&tight[6 * (int64_t)pl + a], d2ord(l));
            atomicMax(&tight[6 * (int64_t)pl + 3 + a], d2ord(h));
        }
    }
}

// The top-level box of placement i from its tight box: padded as make_placement pads (mag * 4e-6 for float scenes,
// mag * 1e-13 for double ones, in double), then rounded outwards to float; written behind the n_shapes shapes' boxes,
// and into the scene bounds as k_prim_boxes does.
template <class R>
__global__ void __launch_bounds__(BLK) k_placement_pad(const long long *__restrict__ tight, int n_instances, int n_shapes, Box *pb, int *scene_ord) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    Box b;
#pragma unroll
    for (int k = 0; k < 3; k++) b.lo[k] = __builtin_huge_valf(), b.hi[k] = -__builtin_huge_valf();
    if (i < n_instances) {
        double lo[3], hi[3], mag = 0;
        for (int a = 0; a < 3; a++) {
            lo[a] = ord2d(tight[6 * (int64_t)i + a]), hi[a] = ord2d(tight[6 * (int64_t)i + 3 + a]);
            mag = fmax(mag, fmax(fabs(lo[a]), fabs(hi[a])));
        }
        const double pad = mag * (sizeof(R) == 4 ? 4e-6 : 1e-13);
        for (int a = 0; a < 3; a++) b.lo[a] = d2f_down(lo[a] - pad), b.hi[a] = d2f_up(hi[a] + pad);
        pb[n_shapes + i] = b;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float lo = b.lo[k], hi = b.hi[k];
        for (int off = 32; off > 0; off >>= 1) lo = fminf(lo, __shfl_xor(lo, off)), hi = fmaxf(hi, __shfl_xor(hi, off));
        if ((threadIdx.x & 63) == 0 && lo <= hi) {
            atomicMin(&scene_ord[k], f2ord(lo));
            atomicMax(&scene_ord[3 + k], f2ord(hi));
        }
    }
}

// Top-level tree over n_shapes shapes and the placements behind them, one entry per leaf.  order[l] = the entry at
// position l of the Morton order; is_shape[l] = 1 if it is a shape.  Its exclusive prefix sum `rank` is where the
// shape's record goes: the records of the top-level tree are its shapes only, in leaf order.
__global__ void __launch_bounds__(BLK) k_flag_shapes(const uint32_t *__restrict__ order, int n, int n_shapes, int *is_shape) {
    const int l = blockIdx.x * BLK + threadIdx.x;
    if (l < n) is_shape[l] = order[l] < (uint32_t)n_shapes;
}
// leaf words of the collapse (position l in the Morton order, one entry) -> an instance word for a placement (what
// collapse_to_wide writes when it is given the build boxes, tk_bvh.h), the compacted record range for a shape
__global__ void __launch_bounds__(BLK) k_top_leaves(Node4<float> *nodes, int n, const uint32_t *__restrict__ order, const int *__restrict__ rank, int n_shapes) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < 4; c++) {
        const int32_t w = nodes[i].c[c].child;
        if (w >= 0 || w == CHILD_EMPTY) continue;
        const int l = leaf_first(w);
        const uint32_t e = order[l];
        nodes[i].c[c].child = e >= (uint32_t)n_shapes ? make_instance_word((int32_t)(e - (uint32_t)n_shapes)) : make_leaf(rank[l], 1);
    }
}
template <class T>
__global__ void __launch_bounds__(BLK) k_permute_top(const T *__restrict__ in, const uint32_t *__restrict__ order, const int *__restrict__ rank, int n, int n_shapes, T *out) {
    const int l = blockIdx.x * BLK + threadIdx.x;
    if (l < n && order[l] < (uint32_t)n_shapes) out[rank[l]] = in[order[l]];
}
// rebase_child (tk_host_scene.h) over the n nodes of a prototype's tree, in the format the scene traverses
template <class NodeT>
__global__ void __launch_bounds__(BLK) k_rebase(NodeT *nodes, int n, int32_t node_base, int32_t prim_base) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < 4; c++) {
        const int32_t w = nodes[i].c[c].child;
        if (w == CHILD_EMPTY) continue;
        nodes[i].c[c].child = w >= 0 ? w + node_base : make_leaf(leaf_first(w) + prim_base, leaf_count(w));
    }
}

// ---- re-posing the placements of a RESIDENT two-level scene (tk_build.hip: repose_two_level_device): new transforms,
// everything else read from what the scene keeps in device memory — no mesh positions, nothing of the caller's.

// The InstTrace / InstShade records of placement i under its new transform (xforms: 12 doubles per placement, as
// TakeInstance::xform): the expressions of Affine3::inverse_linear and placement_records (tk_host_scene.h), operand
// order included, and the build does not contract — the records are the bits a fresh scene_create computes on the
// host.  What a transform does not change comes from the old records: the prototype's root and grid, the material, its
// tag, the first shape id.  A transform inverse_linear refuses (|det| <= 1e-300, or a NaN that reaches the determinant),
// or with an entry that is not finite, writes nothing and leaves the smallest such index in *bad (INT_MAX before).
template <class R>
__global__ void __launch_bounds__(BLK) k_placement_records(const double *__restrict__ xforms, int n, const InstTrace<R> *__restrict__ old_trace,
                                                            const InstShade<R> *__restrict__ old_shade, InstTrace<R> *new_trace, InstShade<R> *new_shade, int *bad) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    double M[12];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = xforms[12 * (int64_t)i + k], finite = finite && __builtin_isfinite(M[k]);
    const double a00 = M[0], a01 = M[1], a02 = M[2], a10 = M[4], a11 = M[5], a12 = M[6], a20 = M[8], a21 = M[9], a22 = M[10];
    const double det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    if (!finite || !(fabs(det) > 1e-300)) {
        atomicMin(bad, i);
        return;
    }
    double inv[9];
    inv[0] = (a11 * a22 - a12 * a21) / det, inv[1] = (a02 * a21 - a01 * a22) / det, inv[2] = (a01 * a12 - a02 * a11) / det;
    inv[3] = (a12 * a20 - a10 * a22) / det, inv[4] = (a00 * a22 - a02 * a20) / det, inv[5] = (a02 * a10 - a00 * a12) / det;
    inv[6] = (a10 * a21 - a11 * a20) / det, inv[7] = (a01 * a20 - a00 * a21) / det, inv[8] = (a00 * a11 - a01 * a10) / det;
    InstTrace<R> it = old_trace[i];
    InstShade<R> is = old_shade[i];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) it.inv[4 * r + c] = (R)inv[3 * r + c], is.fwd[3 * r + c] = (R)M[4 * r + c];
        it.inv[4 * r + 3] = (R)(-(inv[3 * r] * M[3] + inv[3 * r + 1] * M[7] + inv[3 * r + 2] * M[11]));
    }
    new_trace[i] = it;
    new_shade[i] = is;
}

// Tight world boxes of the placements from the RESIDENT records of their prototypes.  span[i] = (first record, number
// of records) of placement i's prototype in `prims`; block0[i] = the first block of placement i, which gets one block
// per REPOSE_CHUNK records (block0[n] = the grid), found by bisection.  The vertices of a record are what k_prim_boxes
// reads, a[0..2], a[0..2] + a[3..5], a[0..2] + a[6..8], here summed and transformed in double (Affine3::image's
// expression, as k_placement_boxes); per-wave partials in LDS, then ordered 64-bit atomics into tight[6 i ..], and the
// prototype's largest |coordinate| (the order of non-negative doubles is the order of their bits) into maxabs[i].
// A streaming kernel: every record is read once per placement of its prototype, 36 (72) of its bytes.
constexpr int REPOSE_CHUNK = 16 * BLK;
template <class R>
__global__ void __launch_bounds__(BLK) k_placement_boxes_resident(const PrimRec<R> *__restrict__ prims, const int2 *__restrict__ span,
                                                                   const int64_t *__restrict__ block0, int n, const double *__restrict__ xforms,
                                                                   long long *tight, long long *maxabs) {
    __shared__ double part[BLK / 64][7];
    int lo_i = 0, hi_i = n;  // block0[lo_i] <= blockIdx.x < block0[hi_i]
    while (hi_i - lo_i > 1) {
        const int mid = (lo_i + hi_i) >> 1;
        if (block0[mid] <= (int64_t)blockIdx.x) lo_i = mid;
        else hi_i = mid;
    }
    const int pl = lo_i;
    const int2 sp = span[pl];
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = xforms[12 * (int64_t)pl + k];
    double lo[3], hi[3], big = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) lo[a] = __builtin_huge_val(), hi[a] = -__builtin_huge_val();
    const int r0 = (int)((int64_t)blockIdx.x - block0[pl]) * REPOSE_CHUNK, r1 = min(sp.y, r0 + REPOSE_CHUNK);
    for (int r = r0 + (int)threadIdx.x; r < r1; r += BLK) {
        const PrimRec<R> &p = prims[(int64_t)sp.x + r];
        double g[9];
#pragma unroll
        for (int k = 0; k < 9; k++) g[k] = (double)p.a[k];
#pragma unroll
        for (int v = 0; v < 3; v++) {
            const double px = v ? g[0] + g[3 * v] : g[0], py = v ? g[1] + g[3 * v + 1] : g[1], pz = v ? g[2] + g[3 * v + 2] : g[2];
            big = fmax(big, fmax(fabs(px), fmax(fabs(py), fabs(pz))));
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const double w = m[4 * a] * px + m[4 * a + 1] * py + m[4 * a + 2] * pz + m[4 * a + 3];
                lo[a] = fmin(lo[a], w), hi[a] = fmax(hi[a], w);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        for (int off = 32; off > 0; off >>= 1) lo[a] = fmin(lo[a], __shfl_xor(lo[a], off)), hi[a] = fmax(hi[a], __shfl_xor(hi[a], off));
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][a] = lo[a], part[threadIdx.x >> 6][3 + a] = hi[a];
    }
    for (int off = 32; off > 0; off >>= 1) big = fmax(big, __shfl_xor(big, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][6] = big;
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        double l = part[0][a], h = part[0][3 + a];
        for (int w = 1; w < BLK / 64; w++) l = fmin(l, part[w][a]), h = fmax(h, part[w][3 + a]);
        if (l <= h) {
            atomicMin(&tight[6 * (int64_t)pl + a], d2ord(l));
            atomicMax(&tight[6 * (int64_t)pl + 3 + a], d2ord(h));
        }
    } else if (threadIdx.x == 3) {
        double b = part[0][6];
        for (int w = 1; w < BLK / 64; w++) b = fmax(b, part[w][6]);
        atomicMax(&maxabs[pl], d2ord(b));
    }
}

// The tight boxes of k_placement_boxes_resident, widened until they contain the boxes a fresh scene_create computes
// from the caller's double positions (k_placement_boxes) — k_placement_pad then pads them as it pads those, from a
// magnitude that is no smaller.  The bound.  Let u be the unit roundoff of R (2^-24, 2^-53), p0 p1 p2 the caller's
// vertices of a face and m the prototype's largest |coordinate| over the vertices read here (maxabs).  The record
// holds v0 = fl(p0) and e1 = fl(fl(p1) - v0) (triangle_into), so per coordinate
//     |v0 - p0| <= u |p0|,    |(v0 + e1) - p1| <= |fl(p1) - p1| + |e1 - (fl(p1) - v0)| <= u |p1| + u |fl(p1) - v0|,
// with |fl(p1) - v0| <= 2 max(|p|) (1 + u) and max(|p|) <= m (1 + 4u): at most 3.1 u m; the double sum v0 + e1 read
// above adds at most 2^-53 |v0 + e1| (nothing for float records whose exponents differ by less than 29).  delta =
// 8 u m = m * 2^-21 (float) / m * 2^-50 (double) is twice that, which also pays for the roundings of the image of a
// vertex and of the subtraction below (a few 2^-53 of the box's magnitude).  A vertex moved by at most delta per
// coordinate moves coordinate a of its image by at most (|L[a][0]| + |L[a][1]| + |L[a][2]|) delta, L the transform's
// linear part: the box grows by that on both sides.
template <class R>
__global__ void __launch_bounds__(BLK) k_widen_tight(long long *tight, const long long *__restrict__ maxabs, const double *__restrict__ xforms, int n) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const double delta = ord2d(maxabs[i]) * (sizeof(R) == 4 ? 0x1p-21 : 0x1p-50);
    const double *M = xforms + 12 * (int64_t)i;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double w = (fabs(M[4 * a]) + fabs(M[4 * a + 1]) + fabs(M[4 * a + 2])) * delta;
        tight[6 * (int64_t)i + a] = d2ord(ord2d(tight[6 * (int64_t)i + a]) - w);
        tight[6 * (int64_t)i + 3 + a] = d2ord(ord2d(tight[6 * (int64_t)i + 3 + a]) + w);
    }
}
// The top-level tree changed its node count: the prototypes' nodes moved by `delta` nodes (k_rebase shifts their child
// words), and so did the roots the placements enter at.  (A leaf word — a one-leaf prototype of a host-built scene —
// names records, which stay where they are.)
template <class R> __global__ void __launch_bounds__(BLK) k_shift_roots(InstTrace<R> *trace, int n, int32_t delta) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < n && trace[i].root_child >= 0) trace[i].root_child += delta;
}


// ---- moving the vertices of meshes of a RESIDENT scene without placements (tk_build.hip: update_mesh_vertices_device):
// new positions (and vertex normals) of some meshes, everything else read from what the scene keeps in device memory.
// new_pos[m] / new_nrm[m]: mesh m's new double arrays in device memory (its vertex 0 first), null = this mesh keeps its
// own; shape_face: the description's shape_face, resident since creation (4 bytes per shape).

// One lane per resident record, in the leaf order of the tree that is being replaced; the record goes to stage[its
// shape id] — the shape order k_make_prims leaves for a fresh build (without placements the shape ids of the n records
// are a permutation of 0 .. n-1).  A triangle of an updated mesh gets new geometry words (triangle_geometry, from the
// resident face_idx at MeshInfo::fbase + face); every other word, and every other record, is copied.  A new coordinate
// that is not finite as R writes nothing new into the record and leaves the smallest mesh << 32 | vertex in *bad (all
// ones before).
template <class R>
__global__ void __launch_bounds__(BLK)
k_update_prims(const PrimRec<R> *__restrict__ recs, int n, const double *const *__restrict__ new_pos, const MeshInfo *__restrict__ meshes,
               const int32_t *__restrict__ shape_face, const int32_t *__restrict__ face_idx, PrimRec<R> *stage, unsigned long long *bad) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    PrimRec<R> p = recs[i];
    if ((uint32_t)p.shape_id >= (uint32_t)n) return;  // (never: the host checked that the scene has one record per shape)
    const double *pos = (p.meta & 0xff) == PRIM_TRIANGLE ? new_pos[p.mesh] : nullptr;
    if (pos) {
        const int32_t *idx = face_idx + 3 * ((int64_t)meshes[p.mesh].fbase + shape_face[p.shape_id]);
        bool finite = true;
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++)
                if (!__builtin_isfinite((R)pos[3 * (int64_t)idx[k] + a])) {
                    finite = false;
                    atomicMin(bad, ((unsigned long long)(uint32_t)p.mesh << 32) | (uint32_t)idx[k]);
                }
        if (finite) triangle_geometry(p.a, pos, idx);
    }
    stage[p.shape_id] = p;
}
// new vertex normals of one mesh as the scene keeps them: R(normal), what mesh_tables (tk_host_scene.h) stores
template <class R> __global__ void __launch_bounds__(BLK) k_convert_normals(const double *__restrict__ in, int64_t n, R *out) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < n) out[i] = (R)in[i];
}
// One lane per light record: an area light (kind 1) on a face of an updated mesh gets v[9] from the new positions and,
// when the mesh got new normals, n[9] from them — light_records' expressions, R(position) and R(normal) of the face's
// three vertices.  stage: the records in shape order (k_update_prims), which know the mesh of a shape.
template <class R>
__global__ void __launch_bounds__(BLK)
k_update_lights(LightRec<R> *lights, int n_lights, const PrimRec<R> *__restrict__ stage, int n_shapes, const double *const *__restrict__ new_pos,
                const double *const *__restrict__ new_nrm, const MeshInfo *__restrict__ meshes, const int32_t *__restrict__ shape_face,
                const int32_t *__restrict__ face_idx) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n_lights) return;
    LightRec<R> &l = lights[i];
    const int32_t shape = l.shape_id;
    if (l.kind != 1 || l.is_sphere || (uint32_t)shape >= (uint32_t)n_shapes) return;
    const int32_t mesh = stage[shape].mesh;
    const double *pos = new_pos[mesh], *nrm = new_nrm[mesh];
    if (!pos) return;
    const int32_t *idx = face_idx + 3 * ((int64_t)meshes[mesh].fbase + shape_face[shape]);
    for (int k = 0; k < 3; k++)
        for (int a = 0; a < 3; a++) {
            l.v[3 * k + a] = (R)pos[3 * (int64_t)idx[k] + a];
            if (nrm) l.n[3 * k + a] = (R)nrm[3 * (int64_t)idx[k] + a];
        }
}


// ---- moving the vertices of meshes of a RESIDENT two-level scene (tk_build.hip: update_two_level_meshes_device): the
// shapes' records are k_update_prims', the normals and lights as above; a prototype whose mesh moved gets new records
// and a new tree, and every prototype's nodes a new place behind the new top-level tree.

// k_make_proto_prims for a prototype whose vertices moved: one face per lane, the positions read from the update's own
// array (positions: the mesh's vertex 0 first, m.pos_off = 0), the indices from the resident face_idx.  A coordinate
// that is not finite as R leaves the smallest mesh << 32 | vertex in *bad (all ones before) and the lane writes nothing.
// Per record: 12 bytes of indices, up to 72 of gathered double vertices, 64 (f32) / 96 (f64) written.
template <class R>
__global__ void __launch_bounds__(BLK)
k_update_proto_prims(MeshSrc m, int32_t mesh_id, const double *__restrict__ positions, const int32_t *__restrict__ face_idx, int n_faces, PrimRec<R> *out,
                     unsigned long long *bad) {
    const int f = blockIdx.x * BLK + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t *idx = face_idx + 3 * ((int64_t)m.fbase + f);
    bool finite = true;
    for (int k = 0; k < 3; k++)
        for (int a = 0; a < 3; a++)
            if (!__builtin_isfinite((R)positions[3 * (int64_t)idx[k] + a])) {
                finite = false;
                atomicMin(bad, ((unsigned long long)(uint32_t)mesh_id << 32) | (uint32_t)idx[k]);
            }
    if (!finite) return;
    PrimRec<R> p{};
    p.shape_id = f;
    p.area_light = -1;
    p.nidx = -1;
    triangle_into(p, m, mesh_id, f, positions, face_idx);
    out[f] = p;
}
// Where the placements of prototype k enter after an update: the root of a moved prototype (node 0 of its new tree) and,
// in a scene of compressed nodes, its new grid; an untouched prototype's nodes moved by `shift` nodes, and its root with
// them — unless the root is a leaf word (a one-leaf prototype of a host-built scene), which names records: they stay.
struct ProtoTarget {
    int32_t shift, moved, root, has_grid;
    float grid_lo[3], grid_step[3];
};
template <class R>
__global__ void __launch_bounds__(BLK)
k_retarget_placements(InstTrace<R> *trace, int n, const int32_t *__restrict__ inst_proto, const ProtoTarget *__restrict__ protos) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const ProtoTarget t = protos[inst_proto[i]];
    if (t.moved) {
        trace[i].root_child = t.root;
        if (t.has_grid)
            for (int a = 0; a < 3; a++) trace[i].grid_lo[a] = t.grid_lo[a], trace[i].grid_step[a] = t.grid_step[a];
    } else if (trace[i].root_child >= 0) {
        trace[i].root_child += t.shift;
    }
}


// ---- the marked geometry (take_hip_scene_track_vertices; layout and look-up: tk_motion_pixel.h).  One lane per record
// of a run whose shape ids are a permutation of 0 .. n-1 — the shapes' records, or one prototype's, whose shape id is
// the face — in the leaf order of the tree an update is about to replace; the 9 geometry words go to entry[its shape
// id] as whole 16-byte words (3 in f32, 6 in f64: an entry is MARKED_STRIDE Reals, the last three zero), bit for bit.
// Per record: 64 (f32) / 96 (f64) bytes read, 48 / 96 written.
template <class R> __global__ void __launch_bounds__(BLK) k_copy_marked(const PrimRec<R> *__restrict__ recs, int n, R *__restrict__ entries) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const int32_t id = recs[i].shape_id;
    if ((uint32_t)id >= (uint32_t)n) return;  // (never: the host checked that the scene has one record per shape)
    constexpr int QUADS = (int)(MARKED_STRIDE * sizeof(R) / sizeof(uint4));
    static_assert(MARKED_STRIDE >= 9 && MARKED_STRIDE * sizeof(R) % sizeof(uint4) == 0, "an entry is whole 16-byte words");
    union {
        R r[MARKED_STRIDE];
        uint4 q[QUADS];
    } e;
    for (int k = 0; k < MARKED_STRIDE; k++) e.r[k] = k < 9 ? recs[i].a[k] : R(0);
    uint4 *dst = reinterpret_cast<uint4 *>(entries + MARKED_STRIDE * (int64_t)id);
    for (int k = 0; k < QUADS; k++) dst[k] = e.q[k];
}

}  // namespace lbvh
}  // namespace tk

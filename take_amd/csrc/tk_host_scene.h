// tk_host_scene.h — host-side preparation of a scene: validates a TakeSceneDesc, converts it to the
// R-typed arrays of tk_scene.h, builds the wide BVH.  The result is a set of plain host vectors; the C-ABI
// layer (tk_create.hip: upload_scene) uploads them to HBM.  Counterpart of the part of the reference's render() between
// parse_scene and the tile loop (src/render.cpp:37-50) plus build_bvh (src/scene.cpp:4-23).
// prepare_scene runs the steps: counts and camera, mesh_tables, material_table, image_table, validate_shape /
// shape_record per shape, light_records (env_light), light_power_tables, build_trees, records into leaf order;
// build_host_trees: Prototype::build and make_placement per instance, the top-level build, append_prototypes, quantise_trees.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "take_hip.h"
#include "tk_bvh.h"
#include "tk_envmap.h"
#include "tk_scene.h"
#include "tk_shading_update.h"

namespace tk {

// which meshes the device builder makes prototype trees of (plan_placements)
struct PlacementPlan {
    std::vector<int32_t> proto_mesh;  // per prototype: its mesh
    std::vector<int32_t> inst_proto;  // per placement: its prototype
};

template <class R> struct HostScene {
    std::vector<Node4<R>> nodes;
    std::vector<QNode4> qnodes;  // compressed copy of nodes (empty = not in use)
    std::vector<Node8<R>> nodes8; // the 8-wide tree at full width: the source of qnodes8 (checks only; never uploaded)
    std::vector<QNode8> qnodes8; // the 8-wide compressed tree (then nodes and qnodes are empty)
    int node_width = 4;          // 4 or 8
    float grid_lo[3] = {0, 0, 0}, grid_step[3] = {1, 1, 1};
    double q_inflation = 1.0;    // mean surface-area inflation of the compressed child boxes (1 = none)
    std::vector<PrimRec<R>> prims;
    int32_t root_child = CHILD_EMPTY;
    std::vector<ShapeInfo> shapes;
    std::vector<MeshInfo> meshes;
    std::vector<int32_t> face_idx;
    std::vector<R> normals, uvs, texels;
    std::vector<MaterialRec<R>> materials;
    std::vector<ImageInfo> images;
    std::vector<LightRec<R>> lights;
    std::vector<R> light_pmf, light_cdf;  // power-based light picking (integrator 3), see prepare_scene
    std::vector<InstTrace<R>> inst_trace;  // two-level scenes (TakeInstance): one record per placement
    std::vector<InstShade<R>> inst_shade;
    int64_t n_blas = 0, blas_nodes = 0, blas_prims = 0;  // stats: prototype trees and their total size
    // what re-posing the placements of the resident scene needs to know of its prototypes (tk_build.hip:
    // repose_two_level_device): per prototype its records in the scene's array, and the depth of the deepest tree
    std::vector<int64_t> blas_prim_first, blas_prim_count;
    int blas_depth = 0;
    // ... and what moving a prototype's vertices needs on top (update_two_level_meshes_device): per prototype its mesh,
    // its nodes in the scene's node array (none: a host-built tree of one leaf, entered through a leaf word) and its
    // depth.  Filled by both builders; every commit that moves nodes keeps them current.
    std::vector<int32_t> blas_mesh;
    std::vector<int64_t> blas_node_first, blas_node_count;
    std::vector<int> blas_depths;
    PlacementPlan placements;  // PREP_DEVICE_BUILD of a two-level scene: what the device builder is to build; inst_proto is kept by both builders
    EnvMap<R> env{-1, 0, 0, 1, 1, 0, 0, {R(0), R(0), R(0)}, nullptr, nullptr, nullptr, nullptr};  // pointers: view() / the uploader
    std::vector<R> env_marginal, env_conditional;
    std::vector<int32_t> env_guide_m, env_guide_c;
    R background[3];
    CameraRec<R> cam;
    WideBvhStats stats;
    int n_material_tags = 0;  // distinct material tags in use (1 => the material sort is skipped)
    uint32_t tag_mask = 0;    // bit t set: some material has tag t
    int single_tag = 0;       // the tag when n_material_tags == 1

    // pointers into the vectors above (a host "device scene" for tests/hostsim; tk_create.hip's upload_scene builds the real one)
    DeviceScene<R> view() const {
        DeviceScene<R> d{};
        d.nodes = nodes.data();
        d.qnodes = qnodes.empty() ? nullptr : qnodes.data();
        d.qnodes8 = qnodes8.empty() ? nullptr : qnodes8.data();
        for (int a = 0; a < 3; a++) d.grid_lo[a] = grid_lo[a], d.grid_step[a] = grid_step[a];
        d.prims = prims.data();
        d.root_child = root_child;
        d.n_nodes = (int32_t)stats.n_nodes;
        d.shapes = shapes.data();
        d.meshes = meshes.data();
        d.face_idx = face_idx.data();
        d.normals = normals.data();
        d.uvs = uvs.data();
        d.materials = materials.data();
        d.images = images.data();
        d.texels = texels.data();
        d.inst_trace = inst_trace.empty() ? nullptr : inst_trace.data();
        d.inst_shade = inst_shade.empty() ? nullptr : inst_shade.data();
        d.n_instances = (int32_t)inst_trace.size();
        d.lights = lights.data();
        d.light_pmf = light_pmf.data();
        d.light_cdf = light_cdf.data();
        d.env = env;
        d.env.marginal = env_marginal.data();
        d.env.conditional = env_conditional.data();
        d.env.guide_m = env_guide_m.data();
        d.env.guide_c = env_guide_c.data();
        d.n_lights = (int32_t)lights.size();
        d.n_shapes = (int32_t)shapes.size();
        for (int a = 0; a < 3; a++) d.background[a] = background[a];
        d.cam = cam;
        return d;
    }
};

// Exactly coincident primitives (identical geometry words: e.g. a duplicated face) tie in t AND in (u, v); the trace
// kernel then lets the larger primitive index win.  For that to mean the same thing in every tree, each group of
// coincident records inside [begin, end) gets its shape ids (with the shading side of the record) in ascending order of
// position — the geometry of the group's records is identical, so no box and no leaf changes.  The device builder needs
// no such pass: its Morton sort is stable, equal codes keep the shape order.
template <class R> inline void order_coincident(std::vector<PrimRec<R>> &prims, size_t begin, size_t end) {
    if (end - begin < 2) return;
    auto geom_hash = [](const PrimRec<R> &p) {
        uint64_t h = 0xcbf29ce484222325ull ^ (uint64_t)(p.meta & 0xff);
        const unsigned char *b = reinterpret_cast<const unsigned char *>(p.a);
        for (size_t i = 0; i < sizeof(p.a); i++) h = (h ^ b[i]) * 0x100000001b3ull;
        return h;
    };
    auto same_geom = [](const PrimRec<R> &x, const PrimRec<R> &y) {
        return (x.meta & 0xff) == (y.meta & 0xff) && std::memcmp(x.a, y.a, sizeof(x.a)) == 0;
    };
    std::vector<std::pair<uint64_t, uint32_t>> keys(end - begin);
    for (size_t i = begin; i < end; i++) keys[i - begin] = {geom_hash(prims[i]), (uint32_t)i};
    std::sort(keys.begin(), keys.end());
    std::vector<PrimRec<R>> group;
    for (size_t i = 0; i < keys.size();) {
        size_t j = i + 1;
        while (j < keys.size() && keys[j].first == keys[i].first) j++;
        if (j - i > 1) {
            // positions keys[i..j) ascend (sorted by (hash, index)); split the run into true geometry groups
            std::vector<char> done(j - i, 0);
            for (size_t a = i; a < j; a++) {
                if (done[a - i]) continue;
                std::vector<uint32_t> pos{keys[a].second};
                for (size_t b = a + 1; b < j; b++)
                    if (!done[b - i] && same_geom(prims[keys[a].second], prims[keys[b].second])) pos.push_back(keys[b].second), done[b - i] = 1;
                if (pos.size() > 1) {
                    group.clear();
                    for (uint32_t q : pos) group.push_back(prims[q]);
                    std::sort(group.begin(), group.end(), [](const PrimRec<R> &x, const PrimRec<R> &y) { return x.shape_id < y.shape_id; });
                    for (size_t q = 0; q < pos.size(); q++) prims[pos[q]] = group[q];
                }
            }
        }
        i = j;
    }
}

// Camera basis of src/render.cpp:37-44, in R arithmetic.
template <class R> inline void make_camera(const TakeCamera &c, CameraRec<R> &out) {
    const R vfov = R(c.vfov);
    const R theta = vfov / R(180) * Const<R>::PI;
    const R h = tk_tan(theta / R(2));
    out.viewport_height = R(2) * h;
    out.viewport_width = out.viewport_height / R(c.height) * R(c.width);
    Vec3<R> from{R(c.lookfrom[0]), R(c.lookfrom[1]), R(c.lookfrom[2])};
    Vec3<R> at{R(c.lookat[0]), R(c.lookat[1]), R(c.lookat[2])};
    Vec3<R> up{R(c.up[0]), R(c.up[1]), R(c.up[2])};
    Vec3<R> w = normalize(from - at);
    Vec3<R> u = normalize(cross(up, w));
    Vec3<R> v = cross(w, u);
    out.u[0] = u.x, out.u[1] = u.y, out.u[2] = u.z;
    out.v[0] = v.x, out.v[1] = v.y, out.v[2] = v.z;
    out.w[0] = w.x, out.w[1] = w.y, out.w[2] = w.z;
    out.lookfrom[0] = from.x, out.lookfrom[1] = from.y, out.lookfrom[2] = from.z;
    out.width = c.width, out.height = c.height;
}

// Run fn(begin, end) -> error string on `threads` contiguous chunks of [0, n); returns the error of the lowest chunk
// that failed ("" if none).  The per-shape loops below are independent per index.
template <class F> inline std::string for_chunks(int64_t n, int threads, F fn) {
    threads = (int)std::max<int64_t>(1, std::min<int64_t>(threads, n / 65536 + 1));
    if (threads == 1) return fn((int64_t)0, n);
    std::vector<std::string> err(threads);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) pool.emplace_back([&, t] { err[t] = fn(n * t / threads, n * (t + 1) / threads); });
    for (auto &th : pool) th.join();
    for (auto &e : err)
        if (!e.empty()) return e;
    return "";
}

// A placement transform (TakeInstance::xform: 3x4, row-major, object -> world), in double.  The expressions are the ones
// the flattening of tk_create.hip (FlattenedInstances) and SceneData.flattened() use, operand order included: the "instanced equals flattened"
// tests compare bits.
struct Affine3 {
    const double *m;
    // inverse of the linear part (row-major 3x3) by its determinant and cofactors; false for a singular transform
    bool inverse_linear(double inv[9]) const {
        const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
        const double det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
        if (!(std::fabs(det) > 1e-300)) return false;
        inv[0] = (a11 * a22 - a12 * a21) / det, inv[1] = (a02 * a21 - a01 * a22) / det, inv[2] = (a01 * a12 - a02 * a11) / det;
        inv[3] = (a12 * a20 - a10 * a22) / det, inv[4] = (a00 * a22 - a02 * a20) / det, inv[5] = (a02 * a10 - a00 * a12) / det;
        inv[6] = (a10 * a21 - a11 * a20) / det, inv[7] = (a01 * a20 - a00 * a21) / det, inv[8] = (a00 * a11 - a01 * a10) / det;
        return true;
    }
    // coordinate `a` of the image of the point (px, py, pz)
    double image(int a, double px, double py, double pz) const { return m[4 * a] * px + m[4 * a + 1] * py + m[4 * a + 2] * pz + m[4 * a + 3]; }
    // grow a box by the image of a point
    void grow(double px, double py, double pz, Bounds &b) const {
        for (int a = 0; a < 3; a++) {
            const double w = image(a, px, py, pz);
            b.lo[a] = std::min(b.lo[a], w), b.hi[a] = std::max(b.hi[a], w);
        }
    }
    // world box of an object-space box: the box of its eight corners' images
    Bounds box_image(const Bounds &o) const {
        Bounds b;
        for (int c8 = 0; c8 < 8; c8++) grow((c8 & 1) ? o.hi[0] : o.lo[0], (c8 & 2) ? o.hi[1] : o.lo[1], (c8 & 4) ? o.hi[2] : o.lo[2], b);
        return b;
    }
};

// a + b rounded downwards / upwards to a double: the residual of the rounded sum (TwoSum, exact without contraction —
// the build sets -ffp-contract=off) says on which side of it the real sum lies
inline double sum_down(double a, double b) {
    const double s = a + b, bb = s - a, err = (a - (s - bb)) + (b - bb);
    return err < 0 ? std::nextafter(s, -std::numeric_limits<double>::infinity()) : s;
}
inline double sum_up(double a, double b) {
    const double s = a + b, bb = s - a, err = (a - (s - bb)) + (b - bb);
    return err > 0 ? std::nextafter(s, std::numeric_limits<double>::infinity()) : s;
}

// The record of face f of mesh `mesh` (the vertices rounded to R, e_k = v_k - v_0 in R; the mesh's material; its
// attribute index) and its build box (of the record's geometry, in double).  Shape id and area light are the caller's.
// (tk_build_gpu.h::k_make_prims is the device twin of this arithmetic.)
template <class R> inline void triangle_record(const TakeSceneDesc &d, const HostScene<R> &hs, int32_t mesh, int64_t f, PrimRec<R> &p, BuildPrim &box) {
    const TakeMesh &m = d.meshes[mesh];
    const int32_t *idx = m.indices + 3 * f;
    Vec3<R> v[3];
    for (int k = 0; k < 3; k++)
        v[k] = {R(m.positions[3 * (int64_t)idx[k]]), R(m.positions[3 * (int64_t)idx[k] + 1]), R(m.positions[3 * (int64_t)idx[k] + 2])};
    const Vec3<R> e1 = v[1] - v[0], e2 = v[2] - v[0];
    p.a[0] = v[0].x, p.a[1] = v[0].y, p.a[2] = v[0].z;
    p.a[3] = e1.x, p.a[4] = e1.y, p.a[5] = e1.z;
    p.a[6] = e2.x, p.a[7] = e2.y, p.a[8] = e2.z;
    // the box of the geometry the intersection tests see — the real numbers v0, v0 + e1, v0 + e2 of the record, as
    // k_prim_boxes takes them (tk_build_gpu.h) —, not of the rounded vertices: e_k = fl(v_k - v0) puts v0 + e_k up to
    // half an ulp of e_k beyond v_k, which a full-width box made from v_k would leave outside
    for (int a = 0; a < 3; a++) {
        const double x0 = (double)p.a[a], e1 = (double)p.a[3 + a], e2 = (double)p.a[6 + a];
        box.bmin[a] = std::min(x0, std::min(sum_down(x0, e1), sum_down(x0, e2)));
        box.bmax[a] = std::max(x0, std::max(sum_up(x0, e1), sum_up(x0, e2)));
    }
    const MeshInfo &mi = hs.meshes[mesh];
    p.meta = PRIM_TRIANGLE | (hs.materials[m.material_id].tag << 8);
    p.material = m.material_id, p.nidx = -1, p.mesh = mesh;
    if (mi.nbase >= 0 || mi.uvbase >= 0) p.nidx = mi.fbase + (int32_t)f, p.meta |= META_HAS_ATTR;
}

// A child word of a prototype's tree (node index or leaf range local to that tree) -> the scene's arrays, where the
// tree's nodes start at node_base and its primitive records at prim_base
inline int32_t rebase_child(int32_t c, size_t node_base, size_t prim_base) {
    if (c == CHILD_EMPTY) return c;
    if (c >= 0) return c + (int32_t)node_base;
    return make_leaf(leaf_first(c) + (int32_t)prim_base, leaf_count(c));
}

// Two-level scenes (EXTENSION, TakeInstance): one tree per prototype mesh in object space ("BLAS"), their nodes and
// primitive records appended behind the top-level tree's; an instance enters the top-level build as one box per entry
// and leaves it as an instance word.
template <class R, int W> struct Prototype {
    std::vector<NodeW<R, W>> nodes;
    std::vector<PrimRec<R>> prims;
    Bounds box;  // object space
    int depth = 0;
    int mesh = -1;  // the mesh it was built from
    size_t node_base = 0, prim_base = 0;  // where nodes / prims start in the scene's arrays (append_prototypes)
    // "re-braiding" (Benthin et al. 2017): the entries a placement contributes to the top-level build — subtrees
    // of the prototype's tree (child word local to this tree + object-space box), the root opened largest box
    // first until `braid` entries exist.  Built and MEASURED in round 3 on configs[4] (1000 placements x 10k
    // triangles, boxes of 0.16 overlapping in a 1.7 box): 1 / 4 / 8 / 16 / 32 / 64 entries per placement = 45.0 /
    // 40.7 / 39.0 / 36.8 / 35.1 / 34.1 Msamples/s — every entry a ray enters costs a 96-byte record, a transform
    // and a return marker, and the entries of one placement overlap (their boxes are the corners' boxes of
    // rotated object boxes); that outweighs the shorter descents.  Default 1 (TAKE_HIP_BRAID overrides).
    struct Entry { int32_t word; Bounds box; };
    std::vector<Entry> entries;

    // records in leaf order, the tree, the object box, the entries
    void build(const TakeSceneDesc &d, const HostScene<R> &hs, int mesh_id, int leaf_size, int threads, int braid) {
        const int64_t nf = d.meshes[mesh_id].n_faces;
        mesh = mesh_id;
        std::vector<PrimRec<R>> recs(nf);
        std::vector<BuildPrim> bp(nf);
        for (int64_t f = 0; f < nf; f++) {
            recs[f] = PrimRec<R>{};
            triangle_record(d, hs, mesh_id, f, recs[f], bp[f]);
            recs[f].shape_id = (int32_t)f, recs[f].area_light = -1;  // local: the shape id of a hit is InstShade::shape_base + this
            box.grow(bp[f].bmin, bp[f].bmax);
            bp[f].id = (int32_t)f;
        }
        Bvh2Builder builder(bp, leaf_size, threads);
        const int root = builder.build();
        std::vector<int32_t> order;
        WideBvhStats st;
        const int32_t root_child = collapse_to_wide<R, W>(builder.nodes(), root, nodes, order, st);
        depth = st.depth;
        prims.resize(order.size());
        for (size_t k = 0; k < order.size(); k++) prims[k] = recs[bp[order[k]].id];
        order_coincident(prims, 0, prims.size());
        entries.assign(1, Entry{root_child, box});
        // open the entry with the largest box while at most `braid` entries result
        while ((int)entries.size() < braid) {
            int best = -1;
            double best_area = -1;
            for (size_t e = 0; e < entries.size(); e++) {
                if (entries[e].word < 0) continue;  // a leaf
                Bounds b;
                b.grow(entries[e].box.lo, entries[e].box.hi);
                if (b.half_area() > best_area) best_area = b.half_area(), best = (int)e;
            }
            if (best < 0) break;
            const NodeW<R, W> &nd = nodes[entries[best].word];
            int nkids = 0;
            for (int j = 0; j < W; j++) nkids += nd.c[j].child != CHILD_EMPTY;
            if ((int)entries.size() - 1 + nkids > braid) break;
            entries.erase(entries.begin() + best);
            for (int j = 0; j < W; j++) {
                if (nd.c[j].child == CHILD_EMPTY) continue;
                Entry e{nd.c[j].child, Bounds()};
                for (int a = 0; a < 3; a++) e.box.lo[a] = (double)nd.c[j].bmin[a], e.box.hi[a] = (double)nd.c[j].bmax[a];
                entries.push_back(e);
            }
        }
    }
};

// World box of a placement of mesh m (object box b) under x.  The TIGHT box: the prototype's vertices under the transform —
// the object box's eight corners under a rotation span up to sqrt(3) times the extent per axis (5x the volume for a
// round cloud), and every ray that enters a placement's box pays a descent from the prototype's root (round 2:
// instanced 42 vs flattened 66 Msamples/s on 1000 x 10k triangles).  Beyond 4e8 vertex transforms in total: the
// corners' box intersected with the box of the bounding sphere's image.
inline Bounds placement_box(const TakeSceneDesc &d, const TakeMesh &m, const Bounds &b, const Affine3 &x) {
    Bounds w;
    if ((double)m.n_vertices * (double)d.n_instances <= 4e8) {
        for (int64_t vtx = 0; vtx < m.n_vertices; vtx++) x.grow(m.positions[3 * vtx], m.positions[3 * vtx + 1], m.positions[3 * vtx + 2], w);
        return w;
    }
    w = x.box_image(b);
    // image of the object box's bounding sphere: centre M c, radius r * ||L||_F per axis row
    const double *M = x.m;
    double c[3], r2 = 0;
    for (int a = 0; a < 3; a++) c[a] = 0.5 * (b.lo[a] + b.hi[a]), r2 += 0.25 * (b.hi[a] - b.lo[a]) * (b.hi[a] - b.lo[a]);
    const double r = std::sqrt(r2);
    for (int a = 0; a < 3; a++) {
        const double wc = x.image(a, c[0], c[1], c[2]);
        const double wr = r * std::sqrt(M[4 * a] * M[4 * a] + M[4 * a + 1] * M[4 * a + 1] + M[4 * a + 2] * M[4 * a + 2]) * (1.0 + 1e-12);
        w.lo[a] = std::max(w.lo[a], wc - wr), w.hi[a] = std::min(w.hi[a], wc + wr);
    }
    return w;
}

// The trace and shade records of placement i: the inverse transform (in double) for the ray, the forward linear part,
// the resolved material.  shape_next: the first shape id of this placement's faces, advanced.  root_child and the grid
// are the builder's to fill in.
template <class R>
std::string placement_records(const TakeSceneDesc &d, int64_t i, const HostScene<R> &hs, int64_t &shape_next, InstTrace<R> &it, InstShade<R> &is) {
    const TakeInstance &in = d.instances[i];
    const TakeMesh &m = d.meshes[in.mesh_id];
    const double *M = in.xform;
    const Affine3 x{M};
    double inv[9];
    if (!x.inverse_linear(inv)) return "instance " + std::to_string(i) + ": singular transform";
    it = InstTrace<R>{};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) it.inv[4 * r + c] = R(inv[3 * r + c]);
        it.inv[4 * r + 3] = R(-(inv[3 * r] * M[3] + inv[3 * r + 1] * M[7] + inv[3 * r + 2] * M[11]));
    }
    is = InstShade<R>{};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) is.fwd[3 * r + c] = R(M[4 * r + c]);
    is.material = in.material_id >= 0 ? in.material_id : m.material_id;
    is.tag = hs.materials[is.material].tag;
    is.shape_base = (int32_t)shape_next;
    shape_next += m.n_faces;
    if (shape_next >= (int64_t)1 << 31) return "too many instanced faces for 32-bit shape ids";
    return "";
}
// what is checked about placement i of a description before anything reads it: "" or the error
inline std::string validate_instance(const TakeSceneDesc &d, int64_t i) {
    const TakeInstance &in = d.instances[i];
    if (in.mesh_id < 0 || in.mesh_id >= d.n_meshes) return "instance " + std::to_string(i) + ": bad mesh id";
    if (in.material_id < -1 || in.material_id >= d.n_materials) return "instance " + std::to_string(i) + ": bad material id";
    if (d.meshes[in.mesh_id].n_faces <= 0) return "instance " + std::to_string(i) + ": empty prototype mesh";
    return "";
}

// Placement i of a two-level scene, prototype b: one InstTrace / InstShade and one top-level box per ENTRY of the
// prototype ("virtual instances", placement-major: the tie rule on the instance id keeps ordering placements as the
// caller numbered them).  shape_next: the first shape id of this placement's faces, advanced.
template <class R, int W>
std::string make_placement(const TakeSceneDesc &d, int64_t i, const Prototype<R, W> &b, HostScene<R> &hs, int64_t &shape_next, std::vector<BuildPrim> &bp) {
    const TakeInstance &in = d.instances[i];
    const TakeMesh &m = d.meshes[in.mesh_id];
    const Affine3 x{in.xform};
    InstTrace<R> it;
    InstShade<R> is;
    const std::string perr = placement_records(d, i, hs, shape_next, it, is);
    if (!perr.empty()) return perr;
    // the placement's world box, padded for the rounding of the transformed ray (the specification is the flattened
    // geometry to fp rounding, see take_hip.h)
    const Bounds pb = placement_box(d, m, b.box, x);
    double mag = 0;
    for (int a = 0; a < 3; a++) mag = std::max(mag, std::max(std::fabs(pb.lo[a]), std::fabs(pb.hi[a])));
    const double pad = mag * (sizeof(R) == 4 ? 4e-6 : 1e-13);
    // one top-level entry per braid entry of the prototype: the entry's object box under the transform (its eight
    // corners), clipped to the placement's box, padded
    for (const auto &e : b.entries) {
        BuildPrim eb;
        const int64_t vid = (int64_t)hs.inst_trace.size();
        if (vid >= ((int64_t)1 << 28)) return "too many instance entries";
        eb.id = -(int32_t)(vid + 1);
        const Bounds w = x.box_image(e.box);
        for (int a = 0; a < 3; a++) {
            eb.bmin[a] = std::max(w.lo[a], pb.lo[a]) - pad, eb.bmax[a] = std::min(w.hi[a], pb.hi[a]) + pad;
            if (eb.bmin[a] > eb.bmax[a]) eb.bmin[a] = eb.bmax[a] = 0.5 * (eb.bmin[a] + eb.bmax[a]);  // (rounding of a flat entry)
        }
        bp.push_back(eb);
        InstTrace<R> ie = it;
        ie.root_child = e.word;  // local to the prototype's tree for now: made global by append_prototypes
        hs.inst_trace.push_back(ie);
        hs.inst_shade.push_back(is);
    }
    return "";
}

// The prototypes' trees behind the top-level tree's `nodes` (top_prims records): node indices and leaf ranges become
// global, in the nodes and in the placements' entry words (inst_proto: per virtual instance, its prototype).
template <class R, int W>
std::string append_prototypes(std::vector<Prototype<R, W>> &protos, const std::vector<int> &inst_proto, size_t top_prims,
                              std::vector<NodeW<R, W>> &nodes, HostScene<R> &hs) {
    const size_t top_nodes = nodes.size();
    size_t nb = top_nodes, pb = top_prims;
    int max_depth = 0;
    for (Prototype<R, W> &b : protos) {
        b.node_base = nb, b.prim_base = pb;
        nb += b.nodes.size(), pb += b.prims.size();
        max_depth = std::max(max_depth, b.depth);
    }
    if (pb >= ((size_t)1 << 28)) return "too many primitive records for the 4-wide leaf encoding (2^28)";
    nodes.reserve(nb);
    for (const Prototype<R, W> &b : protos)
        for (NodeW<R, W> nd : b.nodes) {
            for (int j = 0; j < W; j++) nd.c[j].child = rebase_child(nd.c[j].child, b.node_base, b.prim_base);
            nodes.push_back(nd);
        }
    for (size_t i = 0; i < inst_proto.size(); i++) {
        const Prototype<R, W> &b = protos[inst_proto[i]];
        hs.inst_trace[i].root_child = rebase_child(hs.inst_trace[i].root_child, b.node_base, b.prim_base);
    }
    hs.n_blas = (int64_t)protos.size(), hs.blas_nodes = (int64_t)(nb - top_nodes), hs.blas_prims = (int64_t)(pb - top_prims);
    hs.blas_depth = max_depth;
    hs.blas_prim_first.clear(), hs.blas_prim_count.clear();
    for (const Prototype<R, W> &b : protos) hs.blas_prim_first.push_back((int64_t)b.prim_base), hs.blas_prim_count.push_back((int64_t)b.prims.size());
    hs.blas_mesh.clear(), hs.blas_node_first.clear(), hs.blas_node_count.clear(), hs.blas_depths.clear();
    for (const Prototype<R, W> &b : protos) {
        hs.blas_mesh.push_back(b.mesh), hs.blas_depths.push_back(b.depth);
        hs.blas_node_first.push_back((int64_t)b.node_base), hs.blas_node_count.push_back((int64_t)b.nodes.size());
    }
    hs.placements.inst_proto.assign(inst_proto.begin(), inst_proto.end());  // (per top-level entry: per placement unless braided)
    hs.stats.n_nodes = (int64_t)nodes.size();
    hs.stats.depth += max_depth;  // the traversal stack holds both levels (+ one return marker)
    // primitive records: the top-level tree's in leaf order (prepare_scene fills them in), then each prototype's
    hs.prims.resize(top_prims + (size_t)hs.blas_prims);
    for (const Prototype<R, W> &b : protos) std::copy(b.prims.begin(), b.prims.end(), hs.prims.begin() + b.prim_base);
    return "";
}

// Both precisions traverse the 64-byte compressed nodes unless the 15-bit grid is too coarse for the geometry (child
// boxes growing by more than 10 % in area on average: a scene mixing scales by >1e4), or on request (TAKE_HIP_NODES=wide
// / =q16: A/B runs).  In f64 scenes only the box tests use them (conservative, so exactness is not at stake); hits are
// decided by the double-precision primitive tests.  Every tree of a two-level scene has its own grid (the top-level
// one is the scene's, a prototype's is in its InstTrace).  qnodes stays empty when the full-width nodes are to be used.
template <class R, int W>
void quantise_trees(const std::vector<NodeW<R, W>> &nodes, size_t top_nodes, const std::vector<Prototype<R, W>> &protos,
                    const std::vector<int> &inst_proto, const std::string &fmt, HostScene<R> &hs, std::vector<QNodeW<W>> &qnodes) {
    qnodes.clear();
    if (fmt == "wide" || nodes.empty()) return;
    std::vector<NodeW<R, W>> part(nodes.begin(), nodes.begin() + top_nodes);
    std::vector<QNodeW<W>> q;
    hs.q_inflation = top_nodes ? quantise_nodes<R, W>(part, q, hs.grid_lo, hs.grid_step) : 1.0;
    qnodes = q;
    std::vector<std::array<float, 6>> grids(protos.size());
    for (size_t k = 0; k < protos.size(); k++) {
        part.assign(nodes.begin() + protos[k].node_base, nodes.begin() + protos[k].node_base + protos[k].nodes.size());
        float glo[3], gst[3];
        const double infl = part.empty() ? 1.0 : quantise_nodes<R, W>(part, q, glo, gst);
        if (part.empty()) q.clear(), glo[0] = glo[1] = glo[2] = 0, gst[0] = gst[1] = gst[2] = 1;
        hs.q_inflation = std::max(hs.q_inflation, infl);
        qnodes.insert(qnodes.end(), q.begin(), q.end());
        grids[k] = {glo[0], glo[1], glo[2], gst[0], gst[1], gst[2]};
    }
    for (size_t i = 0; i < inst_proto.size(); i++)
        for (int a = 0; a < 3; a++)
            hs.inst_trace[i].grid_lo[a] = grids[inst_proto[i]][a], hs.inst_trace[i].grid_step[a] = grids[inst_proto[i]][3 + a];
    if (hs.q_inflation > Q_MAX_INFLATION && fmt != "q16") qnodes.clear();
}

// The host's share of a two-level scene the DEVICE builds (tk_build.hip: build_two_level_device): the placements validated, their InstTrace /
// InstShade records (small tables; root_child and grid are filled in after the build), and which meshes are prototypes
// — each distinct one once, in the order the placements first name them, as build_host_trees numbers them
// (PlacementPlan, above HostScene).
template <class R> std::string plan_placements(const TakeSceneDesc &d, HostScene<R> &hs, PlacementPlan &plan) {
    plan = PlacementPlan{};
    std::vector<int> proto_of_mesh(d.n_meshes, -1);
    int64_t shape_next = d.n_shapes;
    hs.inst_trace.assign((size_t)d.n_instances, InstTrace<R>{}), hs.inst_shade.assign((size_t)d.n_instances, InstShade<R>{});
    plan.inst_proto.resize((size_t)d.n_instances);
    for (int64_t i = 0; i < d.n_instances; i++) {
        std::string err = validate_instance(d, i);
        if (!err.empty()) return err;
        const int32_t mesh = d.instances[i].mesh_id;
        if (proto_of_mesh[mesh] < 0) proto_of_mesh[mesh] = (int)plan.proto_mesh.size(), plan.proto_mesh.push_back(mesh);
        plan.inst_proto[i] = proto_of_mesh[mesh];
        if (!(err = placement_records(d, i, hs, shape_next, hs.inst_trace[i], hs.inst_shade[i])).empty()) return err;
        hs.inst_trace[i].root_child = CHILD_EMPTY;
    }
    return "";
}

// The tree tuning knobs of the environment (experiments and tests; read when a scene is built), for everyone who
// asks: TAKE_HIP_NODES, the node format request — "" (compressed 4-wide unless the grid is too coarse), wide, q16
// (compressed whatever the grid), q8 (the 8-wide tree) — and TAKE_HIP_BRAID, the top-level entries per placement, 1..64.
struct TreeKnobs { std::string nodes; int braid; };
inline TreeKnobs tree_knobs() {
    const char *nodes = std::getenv("TAKE_HIP_NODES"), *braid = std::getenv("TAKE_HIP_BRAID");
    return TreeKnobs{nodes ? nodes : "", std::max(1, std::min(braid ? std::atoi(braid) : 1, 64))};
}

struct TreeOpts { int leaf_size, threads; std::string fmt; int braid; };  // fmt, braid: tree_knobs

// The host-side trees of a scene, W-wide: the top-level tree over `bp` (the shapes' boxes; one box per placement entry
// of a two-level scene is appended here), the prototype trees behind it, their compressed form.  Out: `nodes` (full
// width), `qnodes` (compressed; empty when the grid is too coarse or on request), hs.root_child / stats / grid /
// inst_* / the prototypes' records in hs.prims, `order` (leaf order of the top-level tree's primitives as indices into bp).
template <class R, int W>
std::string build_host_trees(const TakeSceneDesc &d, HostScene<R> &hs, std::vector<BuildPrim> &bp, const TreeOpts &o,
                             std::vector<int32_t> &order, std::vector<NodeW<R, W>> &nodes, std::vector<QNodeW<W>> &qnodes) {
    std::vector<Prototype<R, W>> protos;
    std::vector<int> proto_of_mesh(d.n_meshes, -1);
    std::vector<int> inst_proto;  // per virtual instance: its prototype
    int64_t shape_next = d.n_shapes;
    hs.inst_trace.clear(), hs.inst_shade.clear();
    for (int64_t i = 0; i < d.n_instances; i++) {
        const TakeInstance &in = d.instances[i];
        const std::string verr = validate_instance(d, i);
        if (!verr.empty()) return verr;
        if (proto_of_mesh[in.mesh_id] < 0) {
            proto_of_mesh[in.mesh_id] = (int)protos.size();
            protos.emplace_back();
            protos.back().build(d, hs, in.mesh_id, o.leaf_size, o.threads, o.braid);
        }
        const int k = proto_of_mesh[in.mesh_id];
        const std::string err = make_placement(d, i, protos[k], hs, shape_next, bp);
        if (!err.empty()) return err;
        inst_proto.resize(hs.inst_trace.size(), k);
    }
    Bvh2Builder builder(bp, o.leaf_size, o.threads);
    const int root = builder.build();
    hs.root_child = collapse_to_wide<R, W>(builder.nodes(), root, nodes, order, hs.stats, d.n_instances > 0 ? &bp : nullptr);
    const size_t top_nodes = nodes.size();
    const std::string err = append_prototypes(protos, inst_proto, order.size(), nodes, hs);
    if (!err.empty()) return err;
    quantise_trees(nodes, top_nodes, protos, inst_proto, o.fmt, hs, qnodes);
    return "";
}

// Trees of the width TAKE_HIP_NODES asks for.  The 4-wide compressed tree is the default.  =q8 selects the 8-wide one
// (128-byte nodes, octant-ordered slots; built and measured in round 3: a third fewer node visits per ray — 32.9 instead
// of 49.2 on the 1M soup — but eight 16-byte loads per lane and visit instead of four, and the vector L1 charges per load
// instruction and distinct line: closest hit +16 %, shadow rays +25 % slower); =wide / =q16 select
// full-width / forced-compressed 4-wide nodes (A/B runs), and a scene the 15-bit grid is too coarse for falls back to
// full-width 4-wide nodes.
template <class R>
std::string build_trees(const TakeSceneDesc &d, int max_leaf, int threads, HostScene<R> &hs, std::vector<BuildPrim> &bp, std::vector<int32_t> &order) {
    // default leaf size 2: on triangle soups the tighter leaf boxes save more primitive tests than the extra
    // interior nodes cost (1M soup: 48.5 node + 10.8 primitive tests per ray vs 42.6 + 42.6 with 4 per leaf)
    // one primitive per leaf: with one ray per lane a leaf's primitives are tested one after the other, so a second
    // one doubles the leaf step of the whole wave (measured 1 / 2 / 3 / 4 per leaf: 75.6 / 71.0 / 61.0 / 50.8 Msamples/s)
    const TreeKnobs knobs = tree_knobs();
    const TreeOpts o{max_leaf > 0 ? max_leaf : 1, threads, knobs.nodes, knobs.braid};
    hs.node_width = 4;
    if (o.fmt == "q8") {
        const std::string err = build_host_trees<R, 8>(d, hs, bp, o, order, hs.nodes8, hs.qnodes8);
        if (!err.empty()) return err;
        if (!hs.qnodes8.empty() || hs.nodes8.empty()) {
            hs.node_width = 8;
            hs.nodes.clear(), hs.qnodes.clear();
            return "";
        }
        // (grid too coarse: the full-width fall-back is 4-wide; the placements' boxes are appended again)
        bp.erase(std::remove_if(bp.begin(), bp.end(), [](const BuildPrim &b) { return b.id < 0; }), bp.end());
    }
    hs.qnodes8.clear(), hs.nodes8.clear();
    return build_host_trees<R, 4>(d, hs, bp, o, order, hs.nodes, hs.qnodes);
}

// meshes: concatenate face indices; normals / uvs only for meshes that carry them
template <class R> std::string mesh_tables(const TakeSceneDesc &d, int threads, HostScene<R> &hs) {
    hs.meshes.resize(d.n_meshes);
    int64_t nf = 0, nn = 0, nuv = 0;
    for (int i = 0; i < d.n_meshes; i++) {
        const TakeMesh &m = d.meshes[i];
        if (m.n_vertices < 0 || m.n_faces < 0 || (m.n_faces > 0 && (!m.positions || !m.indices)))
            return "mesh " + std::to_string(i) + ": missing arrays";
        if (m.material_id < 0 || m.material_id >= d.n_materials) return "mesh " + std::to_string(i) + ": bad material id";
        hs.meshes[i] = MeshInfo{(int32_t)nf, m.normals ? (int32_t)nn : -1, m.uvs ? (int32_t)nuv : -1, m.material_id};
        nf += m.n_faces;
        if (m.normals) nn += m.n_vertices;
        if (m.uvs) nuv += m.n_vertices;
    }
    if (nf >= (int64_t)1 << 30 || nn >= (int64_t)1 << 30 || nuv >= (int64_t)1 << 30) return "mesh arrays too large";
    hs.face_idx.resize(3 * (size_t)nf);
    hs.normals.resize(3 * (size_t)nn);
    hs.uvs.resize(2 * (size_t)nuv);
    for (int i = 0; i < d.n_meshes; i++) {
        const TakeMesh &m = d.meshes[i];
        const MeshInfo &mi = hs.meshes[i];
        const std::string err = for_chunks(3 * m.n_faces, threads, [&](int64_t k0, int64_t k1) -> std::string {
            for (int64_t k = k0; k < k1; k++) {
                const int32_t vi = m.indices[k];
                if (vi < 0 || vi >= m.n_vertices) return "mesh " + std::to_string(i) + ": vertex index out of range";
                hs.face_idx[3 * (size_t)mi.fbase + k] = vi;
            }
            return "";
        });
        if (!err.empty()) return err;
        if (m.normals)
            for (int64_t k = 0; k < 3 * m.n_vertices; k++) hs.normals[3 * (size_t)mi.nbase + k] = R(m.normals[k]);
        if (m.uvs)
            for (int64_t k = 0; k < 2 * m.n_vertices; k++) hs.uvs[2 * (size_t)mi.uvbase + k] = R(m.uvs[k]);
    }
    return "";
}

// The Burley lobes take square roots and logarithms of their parameters: a value outside the model's range (every
// parameter in [0, 1], an index of refraction > 0) would render NaN pixels — prepare_scene refuses it.
inline bool burley_params_in_range(int tag, const double *param) {
    auto unit = [&](int k) { return param[k] >= 0.0 && param[k] <= 1.0; };  // (false for NaN)
    bool ok = true;
    int eta_at = -1;
    switch (tag) {
        case TAKE_MAT_BURLEY_METAL: ok = unit(0) && unit(1); break;
        case TAKE_MAT_BURLEY_GLASS: ok = unit(0) && unit(1), eta_at = 2; break;
        case TAKE_MAT_BURLEY_CLEARCOAT:
        case TAKE_MAT_BURLEY_SHEEN: ok = unit(0); break;
        default:
            for (int k = 0; k < 11; k++) ok = ok && unit(k);
            eta_at = 11;
    }
    if (eta_at >= 0) ok = ok && param[eta_at] > 0.0 && std::isfinite(param[eta_at]);
    return ok;
}

// materials, and which material tags are in use
// (material i of a scene with n_images images -> its record, or the error: creation's table and
// take_hip_scene_set_materials check and convert a material with this one text)
template <class R> std::string material_record(const TakeMaterial &m, int i, int n_images, bool burley_lobes, MaterialRec<R> &o) {
    if (m.tag < 0 || m.tag >= TAKE_MAT_COUNT) return "material " + std::to_string(i) + ": unknown tag";
    const TakeTexture &t = m.reflectance;
    if (t.kind == 1 && (t.image_id < 0 || t.image_id >= n_images))
        return "material " + std::to_string(i) + ": bad texture image id";
    o.tag = m.tag;
    // TakeBuildOpts.burley_lobes: the reference's Disney alternatives (Lambert clones upstream) get the real lobes
    if (burley_lobes && m.tag >= TAKE_MAT_DISNEY_METAL && m.tag <= TAKE_MAT_DISNEY_BSDF) o.tag = m.tag + 5;
    o.tex_kind = t.kind, o.tex_image = t.image_id, o.pad = 0;
    for (int a = 0; a < 3; a++) o.color[a] = R(t.value[a]);
    o.uscale = R(t.uscale), o.vscale = R(t.vscale), o.uoffset = R(t.uoffset), o.voffset = R(t.voffset);
    o.p0 = R(m.param[0]), o.p1 = R(m.param[1]);
    for (int k = 0; k < TAKE_MATERIAL_PARAMS; k++) o.p[k] = R(m.param[k]);
    if (o.tag >= TAKE_MAT_BURLEY_METAL && o.tag <= TAKE_MAT_BURLEY_BSDF && !burley_params_in_range(o.tag, m.param))
        return "material " + std::to_string(i) + ": Burley parameter outside [0, 1] (or eta <= 0)";
    return "";
}
// which tags a material table uses, unused materials included: what decides whether a render sorts by material and
// which shade instances it launches
template <class R> void material_tags_in_use(const std::vector<MaterialRec<R>> &materials, int &n_material_tags, uint32_t &tag_mask, int &single_tag) {
    bool tag_used[TAKE_MAT_COUNT] = {false};
    for (const MaterialRec<R> &o : materials) tag_used[o.tag] = true;
    n_material_tags = 0, tag_mask = 0;
    for (int t = 0; t < TAKE_MAT_COUNT; t++)
        if (tag_used[t]) n_material_tags++, tag_mask |= 1u << t, single_tag = t;
}
template <class R> std::string material_table(const TakeSceneDesc &d, bool burley_lobes, HostScene<R> &hs) {
    hs.materials.resize(d.n_materials);
    for (int i = 0; i < d.n_materials; i++) {
        const std::string err = material_record(d.materials[i], i, d.n_images, burley_lobes, hs.materials[i]);
        if (!err.empty()) return err;
    }
    material_tags_in_use(hs.materials, hs.n_material_tags, hs.tag_mask, hs.single_tag);
    return "";
}

// texture images: one texel array, converted to R
template <class R> std::string image_table(const TakeSceneDesc &d, HostScene<R> &hs) {
    hs.images.resize(d.n_images);
    int64_t ntex = 0;
    for (int i = 0; i < d.n_images; i++) {
        if (d.images[i].width <= 0 || d.images[i].height <= 0 || !d.images[i].data) return "image: bad dimensions";
        hs.images[i] = ImageInfo{d.images[i].width, d.images[i].height, ntex};
        ntex += (int64_t)d.images[i].width * d.images[i].height;
    }
    hs.texels.resize(3 * (size_t)ntex);
    for (int i = 0; i < d.n_images; i++) {
        const int64_t n = (int64_t)d.images[i].width * d.images[i].height * 3;
        for (int64_t k = 0; k < n; k++) hs.texels[3 * (size_t)hs.images[i].offset + k] = R(d.images[i].data[k]);
    }
    return "";
}

// What is checked about shape i of a description: "" or the error.  (Both modes of prepare_scene report through this,
// and tk_build_gpu.h::k_make_prims relies on it.)  One place builds the message: the loop over 10M valid shapes stays lean.
inline std::string validate_shape(const TakeSceneDesc &d, int64_t i) {
    const char *what = nullptr;
    const int32_t al = d.shape_area_light[i], ref = d.shape_ref[i];
    if (al < -1 || al >= d.n_lights) what = "bad area_light id";
    else if (d.shape_kind[i] == 0) {
        if (ref < 0 || ref >= d.n_spheres) what = "bad sphere index";
        else if (d.spheres[ref].material_id < 0 || d.spheres[ref].material_id >= d.n_materials) return "sphere: bad material id";
    } else if (d.shape_kind[i] == 1) {
        if (ref < 0 || ref >= d.n_meshes) what = "bad mesh index";
        else if (d.shape_face[i] < 0 || d.shape_face[i] >= d.meshes[ref].n_faces) what = "bad face index";
    } else what = "unknown kind";
    return what ? "shape " + std::to_string(i) + ": " + what : std::string();
}

// Shape i (validated) -> its ShapeInfo, its primitive record, its build box
template <class R> inline void shape_record(const TakeSceneDesc &d, int64_t i, const HostScene<R> &hs, ShapeInfo &info, PrimRec<R> &p, BuildPrim &box) {
    p = PrimRec<R>{};
    const int32_t al = d.shape_area_light[i];
    if (d.shape_kind[i] == 0) {
        const int32_t si = d.shape_ref[i];
        const TakeSphere &s = d.spheres[si];
        for (int a = 0; a < 3; a++) p.a[a] = R(s.center[a]);
        p.a[3] = R(s.radius);
        for (int a = 0; a < 3; a++) {  // bounds of src/scene.cpp:8-10, from the R-typed values
            box.bmin[a] = (double)(p.a[a] - p.a[3]);
            box.bmax[a] = (double)(p.a[a] + p.a[3]);
            // an R-rounded centre -+ radius can round inwards: the real c -+ r, rounded outwards in double
            box.bmin[a] = std::min(box.bmin[a], sum_down((double)p.a[a], -(double)p.a[3]));
            box.bmax[a] = std::max(box.bmax[a], sum_up((double)p.a[a], (double)p.a[3]));
        }
        p.meta = PRIM_SPHERE | (hs.materials[s.material_id].tag << 8);
        p.material = s.material_id, p.nidx = -1, p.mesh = -(1 + si);
    } else {
        triangle_record(d, hs, d.shape_ref[i], (int64_t)d.shape_face[i], p, box);
    }
    p.shape_id = (int32_t)i, p.area_light = al, box.id = (int32_t)i;
    info = ShapeInfo{p.mesh, p.mesh < 0 ? 0 : d.shape_face[i], p.material, al};
}

// Sampling tables of an environment map (EnvMap, tk_scene.h), in double: per texel f = luminance * sin(theta of the
// row centre) with luminance = 0.2126 r + 0.7152 g + 0.0722 b (negatives count as 0); cond[y][x] = sum of the row's
// f left of x / row sum (x / width for an all-black row), marg[y] = sum of the row sums above y / total.  Both
// start at 0 and end at exactly 1.  (tests/env_ref.py restates this recipe independently, in numpy.)
inline bool env_tables(const double *rgb, int w, int h, std::vector<double> &marg, std::vector<double> &cond) {
    const double PI_D = 3.14159265358979323846;
    marg.assign((size_t)h + 1, 0.0);
    cond.assign((size_t)h * (w + 1), 0.0);
    std::vector<double> row_sum(h, 0.0);
    for (int y = 0; y < h; y++) {
        const double wy = std::sin(PI_D * (y + 0.5) / h);
        double *c = &cond[(size_t)y * (w + 1)];
        double run = 0;
        for (int x = 0; x < w; x++) {
            const double *t = rgb + 3 * ((size_t)y * w + x);
            c[x] = run;
            run += em::texel_weight(t[0], t[1], t[2], wy);
        }
        row_sum[y] = run;
        for (int x = 0; x <= w; x++) c[x] = em::cond_entry(c[x], run, x, w);
    }
    return em::marginal_cdf(row_sum.data(), h, marg.data());
}

// guide table over an R-typed CDF of n intervals (what the device searches): out[k] = interval of k / g, k = 0..g
// (the bisection: tk_envmap.h, which runs it per lane for take_hip_scene_set_envmap)
template <class R> inline void guide_table(const R *cdf, int n, int g, int32_t *out) {
    for (int k = 0; k <= g; k++) out[k] = em::guide_entry(cdf, n, g, k);
}
inline int pow2_at_least(int v, int cap) {
    int p = 1;
    while (p < v && p < cap) p <<= 1;
    return p;
}
// entries of the guide tables of a width x height map: one per ~quarter row / per column — the bisection that remains
// is 0-1 steps (round 3: with 256 / 64 entries it was 2-3 and ~5 dependent loads; shade kernel -4 % on the bench
// workload, same samples); TAKE_HIP_ENV_GUIDE="<m>,<c>", powers of two, overrides them
inline void env_guide_sizes(int width, int height, int &gm, int &gc) {
    gm = pow2_at_least(4 * height, ENV_GUIDE_M_MAX), gc = pow2_at_least(width, ENV_GUIDE_C_MAX);
    if (const char *e = std::getenv("TAKE_HIP_ENV_GUIDE")) {
        int a = 0, b = 0;
        if (std::sscanf(e, "%d,%d", &a, &b) == 2 && a > 0 && b > 0 && !(a & (a - 1)) && !(b & (b - 1)) && a <= (1 << 16) && b <= (1 << 16)) gm = a, gc = b;
    }
}

// Light i is an environment map (extension: shape_id = image index, intensity = scale): hs.env and its tables
template <class R> std::string env_light(const TakeSceneDesc &d, int i, HostScene<R> &hs) {
    const TakeLight &l = d.lights[i];
    if (hs.env.light >= 0) return "more than one environment-map light";
    if (l.shape_id < 0 || l.shape_id >= d.n_images) return "environment map: bad image index";
    const TakeImage3 &im = d.images[l.shape_id];
    std::vector<double> marg, cond;
    if (!env_tables(im.data, im.width, im.height, marg, cond)) return "environment map: no positive luminance";
    hs.env.light = i, hs.env.width = im.width, hs.env.height = im.height;
    hs.env.texel0 = hs.images[l.shape_id].offset;
    for (int a = 0; a < 3; a++) hs.env.scale[a] = R(l.intensity[a]);
    hs.env_marginal.assign(marg.begin(), marg.end());
    hs.env_conditional.assign(cond.begin(), cond.end());
    int gm, gc;
    env_guide_sizes(im.width, im.height, gm, gc);
    hs.env.n_guide_m = gm, hs.env.n_guide_c = gc;
    hs.env_guide_m.resize(gm + 1);
    guide_table(hs.env_marginal.data(), im.height, gm, hs.env_guide_m.data());
    hs.env_guide_c.resize((size_t)im.height * (gc + 1));
    for (int y = 0; y < im.height; y++)
        guide_table(hs.env_conditional.data() + (size_t)y * (im.width + 1), im.width, gc, hs.env_guide_c.data() + (size_t)y * (gc + 1));
    return "";
}

// light records (geometry read from the description, not from the primitive records: with the device builder there
// are none on the host)
template <class R> std::string light_records(const TakeSceneDesc &d, HostScene<R> &hs) {
    hs.env = EnvMap<R>{-1, 0, 0, 1, 1, 0, 0, {R(0), R(0), R(0)}, nullptr, nullptr, nullptr, nullptr};
    hs.env_marginal.clear(), hs.env_conditional.clear(), hs.env_guide_m.clear(), hs.env_guide_c.clear();
    hs.lights.resize(d.n_lights);
    for (int i = 0; i < d.n_lights; i++) {
        const TakeLight &l = d.lights[i];
        LightRec<R> &o = hs.lights[i];
        o = LightRec<R>{};
        o.kind = l.kind, o.shape_id = -1;
        for (int a = 0; a < 3; a++) o.intensity[a] = R(l.intensity[a]);
        if (l.kind == 0) continue;
        if (l.kind == 2) {
            const std::string err = env_light(d, i, hs);
            if (!err.empty()) return err;
            continue;
        }
        if (l.kind != 1) return "light " + std::to_string(i) + ": unknown kind";
        if (l.shape_id < 0 || l.shape_id >= d.n_shapes) return "light " + std::to_string(i) + ": bad shape id";
        o.shape_id = l.shape_id;
        if (d.shape_kind[l.shape_id] == 0) {
            o.is_sphere = 1;
            const TakeSphere &sp = d.spheres[d.shape_ref[l.shape_id]];
            for (int a = 0; a < 3; a++) o.v[a] = R(sp.center[a]);
            o.v[3] = R(sp.radius);
        } else {
            const TakeMesh &m = d.meshes[d.shape_ref[l.shape_id]];
            // the reference reads mesh.normals.at() when sampling a triangle light and throws on an emissive
            // mesh without vertex normals (src/shape.cpp:163-165): reject it up front
            if (!m.normals) return "light " + std::to_string(i) + ": emissive mesh has no vertex normals";
            const int32_t *idx = m.indices + 3 * (int64_t)d.shape_face[l.shape_id];
            for (int k = 0; k < 3; k++)
                for (int a = 0; a < 3; a++) {
                    o.v[3 * k + a] = R(m.positions[3 * (int64_t)idx[k] + a]);
                    o.n[3 * k + a] = R(m.normals[3 * (int64_t)idx[k] + a]);
                }
        }
    }
    return "";
}

// Power-based light picking (src/light.cpp:9-30).  The reference reads Scene::lights_power_pmf / _cdf but never
// fills them; filled here from its light_power(): luminance(intensity) * area * pi for an area light, 0 otherwise;
// pmf = power / total, cdf = running sum from 0 (n + 1 entries) — in R arithmetic, in light order (the recipe
// the golden `ptpow` tables were made with: the test harness applies it to the reference's own Scene).
// (the per-light expression and the serial pass: tk_shading_update.h, which runs the former per lane for
// take_hip_scene_set_light_intensities)
template <class R> void light_power_tables(HostScene<R> &hs) {
    hs.light_pmf.clear();  // (the powers first)
    for (const LightRec<R> &l : hs.lights) hs.light_pmf.push_back(su::light_power(l));
    su::light_tables_from_powers<R>(hs.light_pmf, hs.light_cdf);
}

// Who makes the primitive records and the tree.  PREP_HOST_BUILD: prepare_scene (records, host SAH tree).
// PREP_DEVICE_BUILD (TAKE_BUILDER_DEVICE_LBVH): the device — the records by tk_build_gpu.h::k_make_prims straight from
// the caller's mesh arrays (at 10M triangles the host loop that writes 640 MB of records was 470 of the 570 ms of
// scene_create), the tree from them in shape order; only validation and the small tables happen here.
enum PrepMode { PREP_HOST_BUILD = 0, PREP_DEVICE_BUILD = 1 };

// returns "" on success, else an error message (-> TAKE_E_INVALID)
template <class R>
std::string prepare_scene(const TakeSceneDesc &d, int max_leaf, int threads, HostScene<R> &hs, PrepMode mode = PREP_HOST_BUILD,
                          bool burley_lobes = false) {
    const bool host_build = mode == PREP_HOST_BUILD;
    if (d.camera.width <= 0 || d.camera.height <= 0) return "camera width/height must be positive";
    if (d.n_shapes < 0 || d.n_meshes < 0 || d.n_spheres < 0 || d.n_lights < 0 || d.n_materials < 0 || d.n_images < 0)
        return "negative count in scene description";
    if (d.n_shapes > 0 && (!d.shape_kind || !d.shape_ref || !d.shape_face || !d.shape_area_light)) return "shape arrays missing";
    if (d.n_shapes >= (int64_t)1 << 28) return "too many shapes for the 4-wide leaf encoding (2^28)";
    if (d.n_instances < 0 || (d.n_instances > 0 && !d.instances)) return "instance array missing";
    if (d.n_instances >= (int64_t)1 << 28) return "too many instances";
    std::string err;
    make_camera<R>(d.camera, hs.cam);
    for (int a = 0; a < 3; a++) hs.background[a] = R(d.background[a]);
    if (!(err = mesh_tables(d, threads, hs)).empty()) return err;
    if (!(err = material_table(d, burley_lobes, hs)).empty()) return err;
    if (!(err = image_table(d, hs)).empty()) return err;

    // shapes -> primitive records (shape order for now) + build boxes; the device builder makes its own
    const int64_t ns = d.n_shapes;
    hs.shapes.clear();
    if (host_build) hs.shapes.resize(ns);
    std::vector<PrimRec<R>> recs(host_build ? ns : 0);
    std::vector<BuildPrim> bp(host_build ? ns : 0);
    err = for_chunks(ns, threads, [&](int64_t i_begin, int64_t i_end) -> std::string {
        for (int64_t i = i_begin; i < i_end; i++) {
            std::string e = validate_shape(d, i);
            if (!e.empty()) return e;
            if (host_build) shape_record(d, i, hs, hs.shapes[i], recs[i], bp[i]);
        }
        return "";
    });
    if (!err.empty()) return err;
    if (!(err = light_records(d, hs)).empty()) return err;
    light_power_tables(hs);

    if (!host_build) {  // no tree, no records
        hs.nodes.clear(), hs.qnodes.clear(), hs.qnodes8.clear(), hs.nodes8.clear(), hs.prims.clear();
        if (!(err = plan_placements(d, hs, hs.placements)).empty()) return err;
        hs.node_width = 4, hs.root_child = CHILD_EMPTY;
        hs.n_blas = hs.blas_nodes = hs.blas_prims = 0;
        hs.stats = WideBvhStats{};
        hs.stats.n_prims = ns;
        return "";
    }
    std::vector<int32_t> order;
    if (!(err = build_trees(d, max_leaf, threads, hs, bp, order)).empty()) return err;
    // the top-level tree's records into its leaf order (order[k]: index into bp; two-level scenes: the prototypes' follow)
    if (hs.prims.size() < order.size()) hs.prims.resize(order.size());
    for_chunks((int64_t)order.size(), threads, [&](int64_t k_begin, int64_t k_end) -> std::string {
        for (int64_t k = k_begin; k < k_end; k++) hs.prims[k] = recs[bp[order[k]].id];
        return "";
    });
    order_coincident(hs.prims, 0, order.size());  // (device build: the stable Morton sort does it)
    if ((hs.node_width - 1) * hs.stats.depth + 2 > (hs.node_width == 8 ? MAX_STACK_ENTRIES_W8 : MAX_STACK_ENTRIES)) return "BVH too deep for the traversal stack";
    return "";
}

}  // namespace tk

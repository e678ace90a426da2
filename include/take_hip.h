/*
 * take_hip.h — C ABI of the MI355X path-tracing core (libtake_hip.so).
 *
 * This is the drop-in boundary for TaKe's hot path.  The reference has no FFI; the
 * seam is the C++ function `Image3 render(const std::vector<std::string>&)`
 * (reference src/render.h:5).  Everything between `build_bvh(scene)`
 * (src/render.cpp:49) and the end of the `parallel_for` tile loop
 * (src/render.cpp:59-82) is replaced by the calls below; the XML parser, the
 * `Scene` aggregate (src/scene.h:13-33) and `imwrite` (src/image.cpp:135) stay
 * on the host.  The flattening of a reference `Scene` into a `TakeSceneDesc` is
 * `take_amd/host/take_flatten.hpp`; INTEGRATION.md shows the 20-line patch to
 * src/render.cpp.
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every entry point
 * returns 0 on success or a negative TAKE_E_* code and records a message that
 * `take_hip_last_error()` returns (thread-local).  Host arrays in a
 * `TakeSceneDesc` are caller-owned and only read during `take_hip_scene_create`.
 * Handles are library-owned.  Calls are synchronous unless they take a stream.
 * One scene handle lives on one GPU (the current HIP device at create time); a
 * multi-GPU job is one process per GPU, each with its own handle (scene
 * replicated), rows sharded with `strip_first/strip_stride`.
 */
#ifndef TAKE_HIP_H
#define TAKE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAKE_HIP_ABI_VERSION 5 /* 2: TakeSceneDesc.instances, TakeRenderOpts.integrator (was reserved); 3: take_hip_render_accumulate; 4: TAKE_PRECISION_MIXED, TakeRenderOpts.exact_bounces; 5: TakeMesh.flags (was reserved), take_hip_mesh_from_ply / _from_serialized, TakeBuildOpts.instances (was reserved) */

/* error codes */
#define TAKE_OK 0
#define TAKE_E_INVALID (-1)   /* bad argument / malformed scene description   */
#define TAKE_E_DEVICE (-2)    /* HIP runtime error (message holds hipGetErrorString) */
#define TAKE_E_NO_GPU (-3)    /* no HIP device: the library never falls back to the CPU */
#define TAKE_E_NOMEM (-4)

/* Material tags: the alternative index of reference `Material`
 * (src/material.h:82-93), in declaration order. */
enum TakeMaterialTag {
    TAKE_MAT_DIFFUSE = 0,
    TAKE_MAT_MIRROR = 1,
    TAKE_MAT_PLASTIC = 2,
    TAKE_MAT_PHONG = 3,
    TAKE_MAT_BLINN_PHONG = 4,
    TAKE_MAT_BLINN_PHONG_MICROFACET = 5,
    TAKE_MAT_DISNEY_DIFFUSE = 6,
    TAKE_MAT_DISNEY_METAL = 7,
    TAKE_MAT_DISNEY_GLASS = 8,
    TAKE_MAT_DISNEY_CLEARCOAT = 9,
    TAKE_MAT_DISNEY_SHEEN = 10,
    TAKE_MAT_DISNEY_BSDF = 11,
    /* EXTENSION (not reference behaviour): the lobes the reference's README promises where its
     * src/materials/disney_{metal,glass,clearcoat,sheen,bsdf}.inl hold Lambert clones — Burley's
     * model in the five-lobe form of UCSD CSE 272 homework 1; specification: DESIGN.md §4d and
     * oracle/take_burley.hpp.  Tag = the reference alternative's tag + 5; a scene made from reference
     * materials gets them through TakeBuildOpts.burley_lobes. */
    TAKE_MAT_BURLEY_METAL = 12,
    TAKE_MAT_BURLEY_GLASS = 13,
    TAKE_MAT_BURLEY_CLEARCOAT = 14,
    TAKE_MAT_BURLEY_SHEEN = 15,
    TAKE_MAT_BURLEY_BSDF = 16,
    TAKE_MAT_COUNT = 17
};

/* reference `Texture = variant<ConstTexture, ImageTexture>` (src/texture.h:16-27) */
typedef struct TakeTexture {
    int32_t kind;      /* 0 = ConstTexture, 1 = ImageTexture */
    int32_t image_id;  /* index into TakeSceneDesc.images (ImageTexture::texture_id) */
    double value[3];   /* ConstTexture::value */
    double uscale, vscale, uoffset, voffset;
} TakeTexture;

/* One alternative of reference `Material`.  `param[]` = the alternative's scalar members in
 * declaration order (src/material.h:7-80), after `reflectance`:
 *   MIRROR, PLASTIC:                 eta
 *   PHONG, BLINN_PHONG, _MICROFACET: exponent
 *   DISNEY_DIFFUSE:                  roughness, subsurface
 *   DISNEY_METAL / BURLEY_METAL:     roughness, anisotropic
 *   DISNEY_GLASS / BURLEY_GLASS:     roughness, anisotropic, eta
 *   DISNEY_CLEARCOAT / BURLEY_CLEARCOAT: clearcoat_gloss
 *   DISNEY_SHEEN / BURLEY_SHEEN:     sheen_tint
 *   DISNEY_BSDF / BURLEY_BSDF:       specular_transmission, metallic, subsurface, specular, roughness,
 *                                    specular_tint, anisotropic, sheen, sheen_tint, clearcoat,
 *                                    clearcoat_gloss, eta
 * Tags 7..11 ignore their parameters, as the reference does (Lambert clones; CLEARCOAT evaluates
 * to zero); tags 12..16 use them.                                                              */
#define TAKE_MATERIAL_PARAMS 12
typedef struct TakeMaterial {
    int32_t tag;
    int32_t reserved;
    TakeTexture reflectance;
    double param[TAKE_MATERIAL_PARAMS];
} TakeMaterial;

/* reference `Image3` (src/image.h:13-39): texel (x,y) at data[(y*width+x)*3 + c] */
typedef struct TakeImage3 {
    int32_t width, height;
    const double *data;
} TakeImage3;

/* reference `TriangleMesh` (src/shape.h:13-18) */
typedef struct TakeMesh {
    int64_t n_vertices;
    int64_t n_faces;
    const double *positions; /* n_vertices * 3 */
    const int32_t *indices;  /* n_faces * 3 */
    const double *normals;   /* n_vertices * 3, or NULL (mesh.normals.empty()) */
    const double *uvs;       /* n_vertices * 2, or NULL (mesh.uvs.empty())     */
    int32_t material_id;
    int32_t flags;           /* 0, or TAKE_MESH_DEVICE_ARRAYS: the four arrays live in device memory (a mesh that
                                take_hip_mesh_from_ply / _serialized / _obj decoded there) */
} TakeMesh;
#define TAKE_MESH_DEVICE_ARRAYS 1

/* reference `Sphere` (src/shape.h:20-23) */
typedef struct TakeSphere {
    double center[3];
    double radius;
    int32_t material_id;
    int32_t reserved;
} TakeSphere;

/* reference `Light = variant<PointLight, DiffuseAreaLight>` (src/light.h:9-19) */
typedef struct TakeLight {
    int32_t kind;      /* 0 = PointLight (counts toward N, contributes nothing:
                          src/integrator/path_tracing.h:33), 1 = DiffuseAreaLight,
                          2 = environment map (EXTENSION, not in the reference: equirectangular
                          image, y up, row 0 = zenith; importance-sampled by luminance*sin(theta),
                          seen by rays that leave the scene instead of `background`; at most one) */
    int32_t shape_id;  /* kind 1: DiffuseAreaLight::shape_id (index into the shape arrays);
                          kind 2: index into `images`; `intensity` then scales the image   */
    double intensity[3];
    double position[3];
} TakeLight;

/* EXTENSION (BASELINE configs[4]: "10M-triangle instanced scene"; the reference has no instancing):
 * one placement of a prototype mesh.  The mesh is NOT copied: the instance is a leaf of the top-level BVH that holds
 * a transform, and a ray entering it is moved into the mesh's object space (two-level traversal).  The result is
 * specified as that of the same geometry flattened to world space (xform applied to the vertices), to fp rounding.
 * Instanced triangles are not emitters.  Their shape ids follow the ordinary shapes: n_shapes + (sum of the face
 * counts of the preceding instances) + face.                                                               */
typedef struct TakeInstance {
    int32_t mesh_id;      /* index into TakeSceneDesc.meshes: the prototype (it need not appear in the shape arrays) */
    int32_t material_id;  /* material of this placement; -1: the mesh's own */
    double xform[12];     /* object -> world, 3x4 row-major affine: world = M[:, :3] * p + M[:, 3]; invertible */
} TakeInstance;

/* reference `Camera` (src/camera.h:5-11) */
typedef struct TakeCamera {
    int32_t width, height;
    double lookfrom[3], lookat[3], up[3];
    double vfov;
} TakeCamera;

/* Flattened reference `Scene` (src/scene.h:13-33).  The shape arrays are
 * `scene.shapes` in order (index = BVH primitive id = DiffuseAreaLight::shape_id),
 * as SoA:  kind 0 = Sphere (ref = index into spheres), 1 = Triangle (ref = mesh id,
 * face = face id).  area_light = ShapeBase::area_light_id (-1 if none).           */
typedef struct TakeSceneDesc {
    TakeCamera camera;
    double background[3];
    int32_t n_meshes;
    int32_t n_spheres;
    const TakeMesh *meshes;
    const TakeSphere *spheres;
    int64_t n_shapes;
    const int32_t *shape_kind;
    const int32_t *shape_ref;
    const int32_t *shape_face;
    const int32_t *shape_area_light;
    int32_t n_lights;
    int32_t n_materials;
    const TakeLight *lights;
    const TakeMaterial *materials;
    int32_t n_images;
    int32_t reserved;
    const TakeImage3 *images;
    int64_t n_instances;            /* extension, see TakeInstance; 0 = none */
    const TakeInstance *instances;
} TakeSceneDesc;

#define TAKE_PRECISION_F32 0
#define TAKE_PRECISION_F64 1
/* Mixed precision: the scene is resident in both arithmetics; a render computes the first `exact_bounces` rounds of
 * every path — camera ray and the next bounces: the ones whose hit / miss decisions carry the most radiance — in
 * double on the f64 scene, converts the surviving paths' records to float and finishes them on the f32 scene.  Images
 * are double.  Why: the f32 path differs from the reference's arithmetic by whole samples wherever a discrete decision
 * flips (~1.7 % of the paths on the 1M-triangle soup: per-pixel RMSE 1.8e-3 at 256 spp, outside the north-star's
 * 1e-3), and a flip costs what the path still carries, which falls off geometrically with the bounce. */
#define TAKE_PRECISION_MIXED 2
#define TAKE_DEFAULT_EXACT_BOUNCES 3

/* scene_create options */
typedef struct TakeBuildOpts {
    int32_t precision;     /* TAKE_PRECISION_F32 (production) or _F64 (parity mode) */
    int32_t bvh_threads;   /* host threads for the BVH build; <=0: hardware_concurrency */
    int32_t max_leaf_size; /* primitives per leaf, 1..4; <=0: default (1) */
    int32_t builder;       /* TAKE_BUILDER_AUTO (0): host SAH below TAKE_AUTO_DEVICE_BUILD_SHAPES primitives, device
                              LBVH from there on (the threshold is the same for every precision, and every side of a
                              scene — both trees of a mixed one — gets that builder; a two-level scene counts its
                              shapes + the faces of its distinct prototypes + its placements);
                              TAKE_BUILDER_DEVICE_LBVH: primitive records, Morton-order tree and its compression are
                              made on the GPU straight from the caller's mesh arrays (10M triangles: 0.2 s);
                              TAKE_BUILDER_HOST_SAH: binned SAH on the host (10M triangles: 6 s; traversal 2-6 %
                              faster).  Results do not depend on the builder (conservative box tests).  Two-level
                              scenes (TakeInstance) are built by either: the device makes every prototype's tree,
                              the placements' boxes and the top-level tree.                     */
    int32_t burley_lobes;  /* 0: materials as given (tags 7..11 behave as the reference's stubs do);
                              1: tags 7..11 are taken as 12..16 — the scene's Disney materials get real lobes */
    int32_t instances;     /* what scene_create does with TakeSceneDesc.instances:
                              TAKE_INSTANCES_TWO_LEVEL (0): prototypes stay single, placements are leaves of a top-level
                              BVH (1000 x 10k triangles: 26 MB);
                              TAKE_INSTANCES_FLATTEN: every placement is expanded to world-space triangles before the
                              build — the geometry the instanced render is specified to equal, 1.1 GB for the same
                              scene, traversed a third faster (one tree resolves the overlap of the placements that
                              a two-level tree must descend into one by one).  Shape ids are the same either way. */
} TakeBuildOpts;
#define TAKE_INSTANCES_TWO_LEVEL 0
#define TAKE_INSTANCES_FLATTEN 1
#define TAKE_BUILDER_AUTO 0
#define TAKE_BUILDER_DEVICE_LBVH 1
#define TAKE_BUILDER_HOST_SAH 2
#define TAKE_AUTO_DEVICE_BUILD_SHAPES 4000000

/* render options: `scene.options` (src/scene.h:8-11) + what the reference
 * hard-codes in src/render.cpp. */
typedef struct TakeRenderOpts {
    int32_t spp;           /* RenderOptions::spp                                      */
    int32_t max_depth;     /* RenderOptions::max_depth; loop is i <= max_depth         */
    uint64_t seed;         /* global seed of the counter RNG (replaces the unseedable
                              std::random_device at src/render.cpp:60)                 */
    double ray_epsilon;    /* ray tmin / shadow-ray shortening (c_EPSILON's role at
                              src/render.cpp:75, path_tracing.h:53,79); <=0: default
                              (1e-7 in f64 as the reference, 1e-4 in f32 — the
                              reference's own commented alternative, src/take.h:31)    */
    int32_t strip_first;   /* multi-GPU: this rank renders the 4-row strips s with     */
    int32_t strip_stride;  /*   s % strip_stride == strip_first (1-GPU: 0 and 1)       */
    int32_t samples_per_batch; /* samples per pixel in flight at once; <=0: auto       */
    int32_t integrator;    /* which of the reference's integrators (src/integrator/path_tracing.h):
                              0 path_tracing (:5, multi-sample MIS — what render() calls; the default),
                              1 path_tracing_raw (:114), 2 path_tracing_one_sample_MIS (:161),
                              3 path_tracing_one_sample_MIS_power (:274, lights picked by power:
                              src/light.cpp:9-30).  1..3 are defined upstream but called by nothing there;
                              they do not know the environment-map extension (TAKE_E_INVALID with one) */
    int32_t exact_bounces; /* TAKE_PRECISION_MIXED scenes: rounds computed in double before the paths continue in
                              float (<= 0: TAKE_DEFAULT_EXACT_BOUNCES); ignored by f32 / f64 scenes             */
    int32_t reserved;
} TakeRenderOpts;
#define TAKE_INTEGRATOR_PATH_MIS 0
#define TAKE_INTEGRATOR_RAW 1
#define TAKE_INTEGRATOR_ONE_SAMPLE_MIS 2
#define TAKE_INTEGRATOR_ONE_SAMPLE_MIS_POWER 3

typedef struct TakeScene TakeScene; /* opaque */

/* ray / hit records of the trace hooks (test + traversal-only benchmark surface;
 * counterpart of scene_intersect / scene_occluded, src/scene.cpp:25-64).
 * Real-typed views: f32 scenes take/return the float fields, f64 scenes the doubles.
 * Contract of every trace hook: tmin >= 0 (the traversal orders entry distances through their bit patterns, which
 * needs non-negative values).  The host entry points (take_hip_trace_closest / _any) refuse a ray with tmin < 0 or
 * NaN with TAKE_E_INVALID; the *_device entry points, which cannot look at device-resident rays, start such a ray —
 * and one with tmin = -0.0 — at tmin = 0.
 * Directions need not have unit length (t is in units of |dir|), components of +0.0 / -0.0 and below 1e-30 are fine,
 * tmin and tmax are inclusive, and every ray of a call may have its own.
 * Range of "the closest hit does not depend on the tree" (it equals an exhaustive search over the primitives, up to
 * the tie rule of DESIGN.md par. 6): F64 and MIXED scenes, ray origins up to 1e6 scene extents away; F32 scenes, up to
 * about 100 scene extents.  Farther out the f32 primitive tests (the sphere quadratic first, the triangle test from
 * ~1e6) return distances whose cancellation error exceeds the margins of the box tests, so a computed hit can lie
 * outside its own primitive's box and whether it is found depends on the tree.  Rays of 4000 aimed from s extents
 * away that differ from the exhaustive search, f32 (DESIGN.md par. 3 has the command):
 *     s        cbox   mats   soup1k   spherelight   meshlight      (soup1k and meshlight hold no sphere)
 *     <= 100      0      0        0             0           0
 *     300         0      1        0             0           0
 *     1000        4     29        0            35           0
 *     3000      567   1341        0           845           0
 *     1e6      1993   2908      195          2233           3      (f64: 0 in every cell) */
typedef struct TakeRayF {
    float org[3], tmin, dir[3], tmax;
} TakeRayF;
typedef struct TakeRayD {
    double org[3], tmin, dir[3], tmax;
} TakeRayD;
typedef struct TakeHitF {
    int32_t shape_id; /* -1 = miss */
    float t, u, v;
} TakeHitF;
typedef struct TakeHitD {
    int32_t shape_id;
    int32_t reserved;
    double t, u, v;
} TakeHitD;

/* work counters of the most recent take_hip_render / trace call on the scene */
typedef struct TakeCounters {
    uint64_t samples;        /* camera paths                                      */
    uint64_t rays_closest;   /* scene_intersect calls                             */
    uint64_t rays_shadow;    /* scene_occluded calls                              */
    uint64_t node_visits;    /* wide-BVH interior nodes fetched (counting mode)   */
    uint64_t prim_tests;     /* ray/triangle + ray/sphere tests (counting mode)   */
    uint64_t bounces;        /* shade-kernel path iterations                      */
    double ms_trace_closest; /* summed HIP-event time of the closest-hit kernel   */
    double ms_trace_shadow;
    double ms_shade;
    double ms_other;
    double ms_total;         /* whole render, first kernel to last                */
    uint64_t launches_trace_closest;
    uint64_t launches_trace_shadow;
    uint64_t node_bytes;     /* bytes of one interior-node fetch in this layout   */
    uint64_t prim_bytes;     /* bytes of one primitive record                     */
    uint64_t leaf_visits;    /* leaves fetched (counting mode)                    */
    uint64_t wave_node_steps;/* wave-level node-phase iterations (counting mode): node_visits / (16 * this) is
                                the fraction of the 16 ray slots of a wave doing useful work in a node step */
    uint64_t wave_leaf_steps;/* wave-level leaf-phase iterations (counting mode)  */
    /* mixed-precision renders: the share of rays_closest / ms_trace_closest / launches_trace_closest that belongs to the
     * f32 rounds (the f32 instance of the closest-hit kernel); zero for f32 and f64 scenes */
    uint64_t rays_closest_f32;
    double ms_trace_closest_f32;
    uint64_t launches_trace_closest_f32;
} TakeCounters;

const char *take_hip_last_error(void);
int take_hip_abi_version(void);
/* number of visible HIP devices, or TAKE_E_NO_GPU */
int take_hip_device_count(void);

/* Replaces build_bvh(scene) (src/scene.cpp:4-23, src/bvh.cpp:8-45) + upload. */
int take_hip_scene_create(const TakeSceneDesc *desc, const TakeBuildOpts *opts, TakeScene **out);
int take_hip_scene_destroy(TakeScene *scene);

/* ---- a resident scene changes (new symbols of ABI version 5; no struct changed).  All of these calls: a failed call
 * leaves the scene exactly as it was (same hits, same image); a successful one ends a progressive sequence
 * (take_hip_accumulated_samples = 0) and the next take_hip_render_accumulate must be called with restart != 0
 * (TAKE_E_INVALID otherwise); F32, F64 and MIXED scenes — a mixed scene changes on both sides or on neither.  Scene
 * groups (take_hip_group_*) are out of scope: a group's replicas cannot be changed, create a new group.
 *
 * New object -> world transforms for ALL placements of a two-level scene, in the order of TakeSceneDesc.instances
 * (n must equal the scene's n_instances; 12 doubles each, as TakeInstance::xform).  Prototypes, materials and
 * shape ids stay as they are.  Afterwards the scene traces and renders exactly as a scene newly created from
 * the same description with these transforms would: hits and images bit for bit.  Only the top level is made again,
 * on the device, from what the scene keeps there: the placements' records and boxes (the prototypes' records under the
 * new transforms), an LBVH over the shapes and the placements, the node array with the prototypes' trees copied
 * behind the new top-level tree.  No mesh, texture or light table is read or uploaded; the prototypes' trees are not
 * touched; the scene keeps its node format.  Who built the scene does not matter (a host-SAH scene has an LBVH top
 * level from its first update on).
 * TAKE_E_INVALID: a NULL argument, a wrong n, a scene without placements (none given, or expanded by
 * TAKE_INSTANCES_FLATTEN), a singular (|det| <= 1e-300) or non-finite transform — the message names the first such
 * placement.  TAKE_E_INVALID with a message that starts with "unsupported": a scene built under TAKE_HIP_BRAID > 1 or
 * TAKE_HIP_NODES=q8, or a new top-level tree of fewer than two leaves or too deep for the traversal stack. */
int take_hip_scene_set_instance_transforms(TakeScene *scene, const double *xforms, int64_t n);
/* the same with the transforms in device memory (e.g. a torch tensor): waits for `stream` (hipStream_t, NULL = default
 * stream), whose work may still be writing them, builds on the default stream as scene_create does, returns after it
 * has completed */
int take_hip_scene_set_instance_transforms_device(TakeScene *scene, const double *d_xforms, int64_t n, void *stream);
/* New camera; width and height must equal the scene's (the render buffers are sized from them), TAKE_E_INVALID
 * otherwise.  Any scene, with or without placements. */
int take_hip_scene_set_camera(TakeScene *scene, const TakeCamera *camera);
/* New vertex positions — and, optionally, vertex normals — for meshes of a scene WITHOUT placements: the vertices
 * move, the topology stays.  Vertex and face counts are the scene's own (the handle remembers the counts of the
 * description it was created from); uvs, indices, materials, spheres and every mesh not named stay as they are.
 * Afterwards the scene is, byte for byte, the scene that take_hip_scene_create with TAKE_BUILDER_DEVICE_LBVH and the
 * same max_leaf_size makes from the description with the new arrays: records, nodes, grid, light records and power
 * tables, hits and images.  Nothing of the description is read or uploaded again: the primitive records of the named
 * meshes get new geometry from the scene's resident face indices, the tree is rebuilt on the device by the LBVH
 * pipeline (no refit: no quality to decay) — compressed or full-width nodes are chosen afresh by the inflation rule —,
 * new normals are converted in place, and area lights on faces of the named meshes get new records and power tables.
 * take_hip_scene_build_info reports TAKE_BUILDER_DEVICE_LBVH for every side afterwards, whoever built the scene;
 * take_hip_scene_stats reports the new tree.
 * TAKE_E_INVALID — arguments that need no scene are looked at before the device is, the others right after it: a NULL
 * scene or `updates`, n_updates <= 0, a mesh index out of range or named twice, positions == NULL, unknown flag bits,
 * normals for a mesh without vertex normals; a new position that is not finite (the message names mesh and vertex).
 * The finiteness check is the update's own — take_hip_scene_create has none — and covers what the records are made of:
 * the coordinates of every vertex a face refers to, as the scene's arithmetic takes them (1e300 is not finite for an
 * f32 or mixed scene).  A vertex no face refers to, and the normals, are taken as they are, as scene_create takes them.
 * TAKE_E_INVALID with a message that starts with "unsupported": a two-level scene (n_instances > 0: this symbol keeps
 * refusing it; take_hip_scene_update_meshes below takes every scene), a scene flattened from instances, a TAKE_HIP_NODES=q8 scene, a new tree of fewer than two leaves or too
 * deep for the traversal stack. */
typedef struct TakeMeshUpdate {
    int32_t mesh;             /* index into the TakeSceneDesc.meshes the scene was created from */
    int32_t flags;            /* 0, or TAKE_MESH_DEVICE_ARRAYS: the two pointers are device memory */
    const double *positions;  /* n_vertices x 3 of that mesh, complete; required */
    const double *normals;    /* n_vertices x 3, or NULL = keep; only for a mesh that has vertex normals */
} TakeMeshUpdate;
int take_hip_scene_set_mesh_vertices(TakeScene *scene, const TakeMeshUpdate *updates, int32_t n_updates);
/* The same for EVERY scene, two-level ones included (a new symbol of ABI version 5; TakeMeshUpdate is reused).
 * A scene without placements: this call IS take_hip_scene_set_mesh_vertices — same path, same bytes, same refusals,
 * a scene flattened from instances among them.
 * A two-level scene (n_instances > 0): every record made from a named mesh gets the new geometry, wherever it lives.
 *  - The mesh is the prototype of at least one placement: its object-space records are made again (shape_id = face,
 *    no area light), its tree is rebuilt on the device by the LBVH pipeline with the scene's leaf size request and put
 *    into the scene's node format on its own grid.  Prototypes not named keep their records and trees bit for bit,
 *    whoever built them.
 *  - Faces of the mesh are among the shape arrays (a mesh may be both): their records in the head of the record array
 *    are rewritten, and area lights on them get new records and power tables.
 *  - New vertex normals are converted in place of the old ones, for either role.
 *  - The top level is rebuilt under the scene's CURRENT transforms, by the path take_hip_scene_set_instance_transforms
 *    takes: the shapes' boxes from their records, the placements' from the prototypes' records after the update.
 *    Placement records keep their transforms, materials, tags and shape bases; placements of a moved prototype get its
 *    new root and grid, and every placement's root follows its prototype's new position in the node array.
 * Afterwards the scene traces and renders exactly as a scene newly created with TAKE_BUILDER_DEVICE_LBVH and the same
 * max_leaf_size from the description with the new arrays and the current transforms: hit tables, occlusion and images
 * bit for bit.  The top-level tree need not be byte-identical (its placement boxes come from records, not from the
 * caller's doubles, as after a re-pose); the moved prototypes' records are.  The scene KEEPS its node format — the
 * float nodes of untouched prototypes no longer exist, so the inflation rule cannot be run again for the whole scene;
 * results do not depend on it.  take_hip_scene_build_info keeps reporting what it reported (untouched trees may still
 * be the host's); take_hip_scene_stats reports the new node count and depth.  take_hip_scene_set_instance_transforms
 * and further updates work on the new layout.
 * TAKE_E_INVALID: as take_hip_scene_set_mesh_vertices, those that need no scene before the device is looked at; the
 * finiteness check covers the records made in either role.  TAKE_E_INVALID with a message that starts with
 * "unsupported": a scene built under TAKE_HIP_BRAID > 1 or TAKE_HIP_NODES=q8, a rebuilt prototype tree of fewer than
 * two leaves, a depth (new top level + deepest prototype + return marker) beyond the traversal stack, node counts
 * beyond the 32-bit record offsets. */
int take_hip_scene_update_meshes(TakeScene *scene, const TakeMeshUpdate *updates, int32_t n_updates);
/* Skinning and morph targets on the device (EXTENSION; new symbols of ABI version 5; no struct changed; specification:
 * DESIGN.md §4q).  A rig is the producer in front of take_hip_scene_update_meshes: it keeps a mesh's rest pose, joint
 * influences and morph targets in device memory, and a pose — one 3x4 matrix per joint, one weight per target — makes
 * the posed positions and normals there.  The handle is scene-free, bound to the device current at its creation, and
 * not thread-safe (it owns the buffers a pose is written into).
 * Arithmetic, in double, every operation in the order written:
 *   palette   J_j = X_j · B_j (3x4 affine; X = joint_xforms, B = inverse_bind; B NULL: J_j = X_j)
 *   morph     p = rest + sum_t w_t dp_t, t in order; n likewise with target_normals
 *   blend     M = sum_k weight_k J_{joint_k}, k in order, no influence skipped; weights are taken AS THEY ARE: they are
 *             neither checked for summing to 1 nor renormalised, and padding is a zero weight on any joint in range
 *   position  p' = M (p, 1)
 *   normal    n' = cof(M3x3) n, negated when det(M3x3) < 0 — the inverse transpose up to a positive factor, right under
 *             non-uniform scale and mirroring —, then divided by its length when that is positive and finite
 *   a rig without joints (n_joints == 0) only morphs: p' = p, n' = n / |n|. */
typedef struct TakeRig TakeRig;
#define TAKE_RIG_DEVICE_ARRAYS 1
#define TAKE_RIG_POSE_DEVICE_ARRAYS 1
typedef struct TakeRigDesc {
    int64_t n_vertices;             /* > 0 */
    const double *positions;        /* n_vertices x 3, rest pose; required */
    const double *normals;          /* n_vertices x 3, or NULL: the rig poses no normals */
    int32_t n_joints;               /* >= 0; 0 = a morph-only rig */
    int32_t n_influences;           /* K: 1..8 when n_joints > 0, else 0 */
    const int32_t *joints;          /* n_vertices x K, each in [0, n_joints) */
    const double *weights;          /* n_vertices x K; taken as they are, never renormalised */
    const double *inverse_bind;     /* n_joints x 12 (3x4 row-major, as set_instance_transforms takes them), NULL = identity */
    int32_t n_targets;              /* T >= 0 */
    const double *target_positions; /* T x n_vertices x 3 deltas, target-major; required when T > 0 */
    const double *target_normals;   /* T x n_vertices x 3 deltas, or NULL; only for a rig with normals */
    int32_t flags;                  /* 0, or TAKE_RIG_DEVICE_ARRAYS: every array above is device memory */
} TakeRigDesc;
typedef struct TakeRigPose {
    const double *joint_xforms;     /* n_joints x 12: joint -> world; required when n_joints > 0 */
    const double *target_weights;   /* T doubles; required when T > 0 */
    int32_t flags;                  /* 0, or TAKE_RIG_POSE_DEVICE_ARRAYS: both arrays are device memory */
} TakeRigPose;
typedef struct TakeRigBinding {
    int32_t mesh;                   /* index into the TakeSceneDesc.meshes the scene was created from */
    int32_t reserved;
    TakeRig *rig;
    TakeRigPose pose;
} TakeRigBinding;
/* The rig copies its arrays to the device and allocates everything a pose needs (posed positions, posed normals, the
 * palette, the staged pose): no later call allocates for the pose.
 * TAKE_E_INVALID before a device is looked for: a NULL argument, n_vertices <= 0, negative counts, K outside 1..8 with
 * joints or not 0 without, a missing required array, target_normals without normals, unknown flag bits.  With the
 * device: host arrays with a joint index out of range or a value that is not finite (the message names array and index);
 * device arrays with a joint index out of range (a kernel finds the smallest such vertex; values are not looked at).
 * TAKE_E_NOMEM: the device has no room for the rig. */
int take_hip_rig_create(const TakeRigDesc *desc, TakeRig **out);
int take_hip_rig_destroy(TakeRig *rig);
/* what the rig holds; device_bytes: everything it has allocated, which no pose changes.  Any output may be NULL. */
int take_hip_rig_info(const TakeRig *rig, int64_t *n_vertices, int32_t *n_joints, int32_t *n_influences, int32_t *n_targets, int32_t *has_normals,
                      int64_t *device_bytes);
/* The rig under `pose` into device memory: n_vertices x 3 doubles each; d_normals_out NULL = not wanted (given for a
 * rig without normals: TAKE_E_INVALID).  Runs on `stream` (hipStream_t, NULL = the default stream), after whatever that
 * stream still has to write into device pose arrays, and returns after it has completed. */
int take_hip_rig_pose_device(TakeRig *rig, const TakeRigPose *pose, double *d_positions_out, double *d_normals_out, void *stream);
/* the same into host arrays (the rig's own buffers, then a download); normals_out NULL = not wanted */
int take_hip_rig_pose(TakeRig *rig, const TakeRigPose *pose, double *positions_out, double *normals_out);
/* Pose and update in one step: every binding's rig is posed into the rig's own buffers, then the scene takes exactly the
 * path of take_hip_scene_update_meshes with TAKE_MESH_DEVICE_ARRAYS over them.  Afterwards the scene is, byte for byte,
 * the scene after take_hip_rig_pose to the host followed by take_hip_scene_update_meshes with those host arrays — with
 * everything that call carries: both kinds of scene, every precision, the finiteness refusal (which is what catches a
 * joint matrix that is not finite), frame marks and vertex tracking, the end of a progressive sequence, and a failed
 * call leaving the scene as it was (the pose kernels write rig-owned memory only, before anything is staged).
 * Normals are passed on only when both the rig and the mesh have them: a mesh with normals keeps them under a rig
 * without, and a rig with normals computes none for a mesh without.
 * TAKE_E_INVALID before a device is looked for: a NULL argument (a binding's rig, a required pose array), n <= 0, a
 * negative mesh index, unknown pose flag bits, a mesh named twice, a rig bound twice.  Right after it, against the
 * scene: a mesh index out of range, a rig on another device, a rig whose n_vertices is not the mesh's (the message
 * names the binding, the mesh and both counts).  Then every refusal of take_hip_scene_update_meshes, in its words. */
int take_hip_scene_pose_meshes(TakeScene *scene, const TakeRigBinding *bindings, int32_t n);
/* Loop subdivision surfaces on the device (EXTENSION; new symbols of ABI version 5; no struct changed; specification:
 * DESIGN.md §4s).  A TakeSubdiv is the stage between "pose" and "update": made once from a cage's TOPOLOGY — its faces,
 * optional per-vertex uvs, a level count —, it keeps the refined topology and the per-level stencil tables in device
 * memory; every frame cage POSITIONS go in and refined positions and vertex normals come out there.  The handle is
 * scene-free, bound to the device current at its creation, and not thread-safe (it owns the buffers a refine writes).
 * One level, in double, every operation in the order written:
 *   edges      the distinct unordered corner pairs (lo < hi), numbered in ascending (lo, hi) order
 *   vertices   even vertex v keeps index v; the odd vertex of edge e is V + e
 *   faces      (a, b, c) becomes (a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca) at 4 f .. 4 f + 3
 *   uvs        even: kept; odd: 0.5 * (uv[lo] + uv[hi]) — made once at creation, no refine touches them
 *   even       interior, neighbours n0 < n1 < ... (n of them): s = p[n0]; s = s + p[n1]; ...;
 *              (1.0 - n * beta) * p[v] + beta * s with beta = 3/16 for n = 3, else 3.0 / (8.0 * n)   (Warren's weights)
 *              on the boundary, boundary neighbours b0 < b1: 0.75 * p[v] + 0.125 * (p[b0] + p[b1]);  no face: copied
 *   odd        interior: 0.375 * (p[lo] + p[hi]) + 0.125 * (p[c] + p[d]), c the opposite corner in the lower-numbered
 *              face, d in the higher;  boundary: 0.5 * (p[lo] + p[hi])
 * After the last level: N_f = cross(p1 - p0, p2 - p0); a vertex's normal is the sum of N_f over its faces in ascending
 * face order, divided by its length when that is positive and finite. */
typedef struct TakeSubdiv TakeSubdiv;
#define TAKE_SUBDIV_DEVICE_ARRAYS 1 /* cage_positions is device memory */
typedef struct TakeSubdivDesc {
    int64_t n_vertices, n_faces; /* of the cage; > 0 */
    const int32_t *indices;      /* n_faces x 3; host memory */
    const double *uvs;           /* n_vertices x 2, or NULL; host memory */
    int32_t levels;              /* 1..6 */
    int32_t flags;               /* 0 */
} TakeSubdivDesc;
typedef struct TakeSubdivBinding {
    int32_t mesh;                 /* index into the TakeSceneDesc.meshes the scene was created from */
    int32_t flags;                /* 0, or TAKE_SUBDIV_DEVICE_ARRAYS */
    TakeSubdiv *subdiv;
    const double *cage_positions; /* cage vertices x 3, or NULL when `rig` is given */
    TakeRig *rig;                 /* NULL, or the cage comes from this rig under `pose` */
    TakeRigPose pose;
} TakeSubdivBinding;
/* These two need no GPU (as take_hip_ply_layout, take_hip_shutter_plan): the refined counts, and the refined faces
 * (n_faces_out x 3) and uvs (n_vertices_out x 2; NULL = not wanted; wanted from a cage without uvs: TAKE_E_INVALID) —
 * what a caller builds the TakeSceneDesc mesh from, with positions from one refine.
 * TAKE_E_INVALID, the message naming the level and the face, edge or vertex: a NULL argument, counts <= 0, levels
 * outside 1..6, unknown flag bits, an index out of range, a face with a repeated index, an edge with more than two
 * faces, a boundary vertex with other than two boundary edges (a bow-tie).  TAKE_E_INVALID with a message that starts
 * with "unsupported": refined counts at which 3 * n_faces or n_vertices passes INT32_MAX.  Inconsistent orientation
 * across an edge is accepted: no weight reads orientation. */
int take_hip_subdiv_counts(const TakeSubdivDesc *desc, int64_t *n_vertices_out, int64_t *n_faces_out);
int take_hip_subdiv_topology(const TakeSubdivDesc *desc, int32_t *indices_out, double *uvs_out);
/* The same refusals, before a device is looked for; then the tables are built on the host, uploaded, and everything a
 * refine needs is allocated: the staged cage, the level buffers, the face normals, the handle's own outputs.  No later
 * call allocates for the refine.  TAKE_E_NOMEM: the device has no room. */
int take_hip_subdiv_create(const TakeSubdivDesc *desc, TakeSubdiv **out);
int take_hip_subdiv_destroy(TakeSubdiv *subdiv);
/* what the handle holds; device_bytes: everything it has allocated, which no refine changes.  Any output may be NULL. */
int take_hip_subdiv_info(const TakeSubdiv *subdiv, int64_t *cage_vertices, int64_t *n_vertices, int64_t *n_faces, int32_t *levels, int64_t *device_bytes);
/* The cage refined into device memory: n_vertices x 3 doubles each; d_normals_out NULL = not wanted.  cage_positions is
 * host memory, or device memory under TAKE_SUBDIV_DEVICE_ARRAYS.  Runs on `stream` (hipStream_t, NULL = the default
 * stream), after whatever that stream still has to write into a device cage, and returns after it has completed.  A
 * position that is not finite is refined as it is: the mesh update's own finiteness check catches it. */
int take_hip_subdiv_refine_device(TakeSubdiv *subdiv, const double *cage_positions, int32_t flags, double *d_positions_out, double *d_normals_out, void *stream);
/* the same from a host cage into host arrays (the handle's own buffers, then a download); normals_out NULL = not wanted */
int take_hip_subdiv_refine(TakeSubdiv *subdiv, const double *cage_positions, double *positions_out, double *normals_out);
/* Refine and update in one step: every binding's cage — host or device positions, or a rig that is posed first (its
 * n_vertices must equal the cage's) — is refined into the handle's own buffers, then the scene takes exactly the path of
 * take_hip_scene_update_meshes with TAKE_MESH_DEVICE_ARRAYS over them, with everything that call carries: both kinds of
 * scene, every precision, the finiteness refusal, frame marks and vertex tracking, the end of a progressive sequence, and
 * a failed call leaving the scene as it was (the kernels write handle-owned memory only, before anything is staged).
 * Normals are passed on only when the mesh has vertex normals.
 * TAKE_E_INVALID before a device is looked for: a NULL argument, n <= 0, a negative mesh index, unknown flag bits,
 * neither or both of cage_positions and rig, what take_hip_rig_pose refuses of a bound rig's pose, a mesh named twice, a
 * handle bound twice.  Right after it, against the scene: a mesh index out of range, a handle or rig on another device,
 * a rig whose n_vertices is not the cage's, a refined vertex count that is not the mesh's (the message names the binding
 * and both counts).  Then every refusal of take_hip_scene_update_meshes, in its words. */
int take_hip_scene_subdivide_meshes(TakeScene *scene, const TakeSubdivBinding *bindings, int32_t n);
/* Displacement mapping on the device (EXTENSION; new symbols of ABI version 5; no struct changed; specification:
 * DESIGN.md §4t).  A TakeDisplace is the stage between "refine" and "update": made once from a mesh's TOPOLOGY — its
 * faces and per-vertex uvs — and a one-channel height image, it keeps the image, every vertex's lookup coordinates and
 * every vertex's row of faces in device memory; every frame base POSITIONS (and the unit normals to move along) go in and
 * displaced positions and their vertex normals come out there.  Displacement is per vertex: a vertex shared by several
 * faces moves once, so no mesh cracks.  The handle is scene-free, bound to the device current at its creation, and not
 * thread-safe (it owns the buffers a call writes).
 * In double, every operation in the order written:
 *   sources    once, at creation: s = uscale * u + uoffset, t = vscale * v + voffset, a = modulo1(s), b = modulo1(t), with
 *              the modulo of the texture lookup: in [0, 1) for every finite argument
 *   height     bilinear with wrap, sample i at a = i / width: x = width * a; x1 = floor(x); fx = x - x1;
 *              x2 = (x1 + 1 == width) ? 0 : x1 + 1; the same for y from b and height;
 *              h = (q11 * (1.0 - fx) + q21 * fx) * (1.0 - fy) + (q12 * (1.0 - fx) + q22 * fx) * fy with q11 = texel(y1, x1),
 *              q21 = texel(y1, x2), q12 = texel(y2, x1), q22 = texel(y2, x2); a float texel is widened, which is exact.
 *              (NOT the seam arithmetic of the colour textures, which extrapolates in the wrap cell.)
 *   position   d = scale * h + bias; p' = p + d * n
 *   direction  n as given, or — left out — the vertex normals of the base positions, by the rule of the last line
 *   normals    of the displaced positions: N_f = cross(p1 - p0, p2 - p0); a vertex's normal is the sum of N_f over its
 *              faces in ascending face order, divided by its length when that is positive and finite. */
typedef struct TakeDisplace TakeDisplace;
#define TAKE_DISPLACE_DEVICE_ARRAYS 1 /* texels (a description), positions and normals (a call, a binding) are device memory */
typedef struct TakeDisplaceDesc {
    int64_t n_vertices, n_faces; /* of the mesh; > 0 */
    const int32_t *indices;      /* n_faces x 3; host memory */
    const double *uvs;           /* n_vertices x 2; host memory; required */
    int32_t width, height;       /* of the height image; > 0, width * height <= INT32_MAX */
    const void *texels;          /* height * width values, row-major, ONE channel */
    int32_t real;                /* TAKE_PRECISION_F32: float texels, TAKE_PRECISION_F64: double texels */
    int32_t flags;               /* 0, or TAKE_DISPLACE_DEVICE_ARRAYS: texels is device memory */
    double uscale, vscale, uoffset, voffset; /* the lookup, as TakeTexture's */
} TakeDisplaceDesc;
typedef struct TakeDisplaceBinding {
    int32_t mesh;                 /* index into the TakeSceneDesc.meshes the scene was created from */
    int32_t flags;                /* 0, or TAKE_DISPLACE_DEVICE_ARRAYS: positions and normals, or cage_positions */
    TakeDisplace *displace;
    double scale, bias;
    const double *positions;      /* the base surface as arrays: n_vertices x 3, or NULL when `subdiv` is given */
    const double *normals;        /* n_vertices x 3 unit normals, or NULL = the handle's own; NULL with `subdiv` */
    TakeSubdiv *subdiv;           /* NULL, or the base surface is this handle's refined cage, moved along its normals */
    const double *cage_positions; /* with `subdiv`: cage vertices x 3, or NULL when `rig` is given */
    TakeRig *rig;                 /* with `subdiv`: NULL, or the cage comes from this rig under `pose` */
    TakeRigPose pose;
} TakeDisplaceBinding;
/* The image is copied to the device in the width it came in, the rows of faces and the lookup coordinates are built on
 * the host and uploaded, and everything a call needs is allocated: the staged base arrays, the face normals, the
 * handle's own outputs.  No later call allocates for the displacement.
 * TAKE_E_INVALID before a device is looked for, the message naming the face or vertex: a NULL argument, uvs == NULL,
 * counts <= 0, an index out of range, width or height <= 0 or width * height beyond INT32_MAX, `real` neither F32 nor
 * F64, unknown flag bits, a lookup parameter that is not finite, a vertex whose s or t is not finite.  TAKE_E_INVALID
 * with a message that starts with "unsupported": counts at which 3 * n_faces or n_vertices passes INT32_MAX.
 * TAKE_E_NOMEM: the device has no room. */
int take_hip_displace_create(const TakeDisplaceDesc *desc, TakeDisplace **out);
int take_hip_displace_destroy(TakeDisplace *displace);
/* what the handle holds; device_bytes: everything it has allocated, which no call changes.  Any output may be NULL. */
int take_hip_displace_info(const TakeDisplace *displace, int64_t *n_vertices, int64_t *n_faces, int32_t *width, int32_t *height, int64_t *device_bytes);
/* The base surface displaced into device memory: n_vertices x 3 doubles each; d_normals_out NULL = not wanted.  positions
 * and normals are host memory, or device memory under TAKE_DISPLACE_DEVICE_ARRAYS; normals NULL: the direction is the
 * handle's own vertex normals of `positions`.  Runs on `stream` (hipStream_t, NULL = the default stream), after whatever
 * that stream still has to write into device arrays, and returns after it has completed.  TAKE_E_INVALID before a device
 * is looked for: a NULL argument, unknown flag bits, a scale or bias that is not finite, an output that IS an input
 * (d_positions_out or d_normals_out equal to positions or normals: the kernels read and write through pointers they
 * take as distinct, so the outputs must not overlap the inputs or each other at all; displace into a second array).  A
 * base position that is not finite is displaced as it is: the mesh update's own finiteness check catches it. */
int take_hip_displace_apply_device(TakeDisplace *displace, const double *positions, const double *normals /* NULL = own */, int32_t flags, double scale, double bias,
                                   double *d_positions_out, double *d_normals_out /* NULL = not wanted */, void *stream);
/* the same from host arrays into host arrays (the handle's own buffers, then a download); normals_out NULL = not wanted */
int take_hip_displace_apply(TakeDisplace *displace, const double *positions, const double *normals, double scale, double bias, double *positions_out, double *normals_out);
/* Displace and update in one step.  Every binding names its base surface in exactly one of two ways: `positions` with
 * optional `normals` — host arrays, or device arrays under TAKE_DISPLACE_DEVICE_ARRAYS —, or `subdiv` with exactly one of
 * cage_positions and rig: the cage is then refined into the subdivision handle's own buffers, with normals, exactly as
 * take_hip_scene_subdivide_meshes refines it.  The surface is displaced into the displacement handle's own buffers, then
 * the scene takes exactly the path of take_hip_scene_update_meshes with TAKE_MESH_DEVICE_ARRAYS over them, with
 * everything that call carries: both kinds of scene, every precision, the finiteness refusal, frame marks and vertex
 * tracking, the end of a progressive sequence, and a failed call leaving the scene as it was (the kernels write
 * handle-owned memory only, before anything is staged).  Normals are passed on only when the mesh has vertex normals.
 * TAKE_E_INVALID before a device is looked for: a NULL argument, n <= 0, a negative mesh index, unknown flag bits, a scale
 * or bias that is not finite, neither or both of positions and subdiv, normals given with subdiv, neither or both of
 * cage_positions and rig under subdiv (either of them without it), what take_hip_rig_pose refuses of a bound rig's pose, a
 * mesh named twice, a displacement or subdivision handle bound twice.  Right after it, against the scene: a mesh index
 * out of range, a handle or rig on another device, a rig whose n_vertices is not the cage's, a refined count, a
 * displacement count and a mesh count that disagree (the message names the binding and the counts).  Then every refusal
 * of take_hip_scene_update_meshes, in its words.  The vertex counts are all that is compared: that the handle was made
 * from the FACES of that mesh is the caller's responsibility (a scene keeps its meshes' vertex counts, not their
 * topology) — a handle made from other faces over as many vertices gives the normals of that other mesh. */
int take_hip_scene_displace_meshes(TakeScene *scene, const TakeDisplaceBinding *bindings, int32_t n);
/* A new environment map (EXTENSION; new symbols of ABI version 5; no struct changed; specification: DESIGN.md §4o).
 * The call replaces the image images[k] of the description the scene was created from, k being the shape_id of its
 * environment-map light (TakeLight kind 2), and — with scale3 — that light's intensity; scale3 == NULL keeps it.
 * Afterwards the scene is, byte for byte, the scene take_hip_scene_create makes from that description with the image
 * (and the intensity) replaced, on every resident side:
 *  - the image's texels in the texel array — a material that uses image k as a texture sees the new image too;
 *  - the image table: later images keep their order and get shifted offsets.  With unchanged dimensions the texels are
 *    overwritten in place and nothing moves; otherwise the texel array is laid out again as [images before | new image |
 *    images after] by device-to-device copies;
 *  - the EnvMap record, the marginal and the conditional CDFs, both guide tables with their sizes (creation's rule,
 *    TAKE_HIP_ENV_GUIDE included) and the light record's intensity.
 * Renders, take_hip_debug_env outputs and trace results are those of the fresh scene, bit for bit.  A float image is
 * taken as its values widened to double: the fresh scene in question holds those doubles.  The tables are made on the
 * device (take_amd/csrc/tk_envmap.h), once in double, and rounded per side; each side's guide tables are searched on
 * that side's own rounded CDF.  The contract of "a resident scene changes" above holds: a failed call leaves the scene
 * exactly as it was (everything is built aside and swapped in at the end), a successful one ends a progressive sequence;
 * F32, F64 and MIXED scenes, a mixed scene on both sides or on neither; not for scene groups.
 * TAKE_E_INVALID, before a device is looked for: a NULL scene, image or data ("null argument"), width or height <= 0,
 * an unknown `real`, unknown flag bits, a scale that is not finite.  After a device was found: a scene without an
 * environment-map light ("no environment map": adding a light is out of scope), a map whose total weight is not > 0
 * ("environment map: no positive luminance", creation's own message; found on the device).  TAKE_E_NOMEM leaves the
 * scene untouched. */
typedef struct TakeEnvImage {
    int32_t width, height;
    const void *data;      /* height * width * 3, row 0 = zenith, as TakeImage3 */
    int32_t real;          /* TAKE_PRECISION_F32: float texels, TAKE_PRECISION_F64: double texels */
    int32_t flags;         /* 0, or TAKE_MESH_DEVICE_ARRAYS: data is device memory */
} TakeEnvImage;
int take_hip_scene_set_envmap(TakeScene *scene, const TakeEnvImage *image, const double *scale3 /* NULL = keep */);
/* the same after waiting for `stream` (hipStream_t, NULL = default stream), whose work may still be writing the texels
 * (e.g. a torch tensor): builds on the default stream, returns after it has completed */
int take_hip_scene_set_envmap_device(TakeScene *scene, const TakeEnvImage *image, const double *scale3, void *stream);
/* New materials and new light intensities (EXTENSION; new symbols of ABI version 5; no struct changed; specification:
 * DESIGN.md §4p).
 * take_hip_scene_set_materials replaces materials [first, first + count) of the table the scene was created with.
 * Afterwards every resident side holds, byte for byte, what take_hip_scene_create makes from the original description
 * with those materials replaced, under the same TakeBuildOpts (burley_lobes remaps a new material as it remapped the
 * old ones): the material table, the tag byte of every primitive record's meta, the tag of every placement record of a
 * two-level scene, and the host's record of which tags are in use — whether a render sorts by material and which shade
 * instances it launches; unused materials count, as at creation.  The table keeps its size, and which shape, mesh or
 * placement uses which material does not change.  Each new material passes creation's checks with creation's messages,
 * the material numbered by its place in the table.  The tag bytes are rewritten in place by a kernel (one lane per
 * record) only when some material of the range changes its effective tag; a change of colours, textures and
 * parameters writes the table alone.  Later updates (take_hip_scene_set_mesh_vertices, take_hip_scene_update_meshes,
 * take_hip_scene_set_instance_transforms) build on the new tags.
 * take_hip_scene_set_light_intensities replaces the intensity of lights [first, first + count) by rgb[3 k ..],
 * k = 0 .. count - 1 (host memory); kinds and geometry do not change.  Afterwards every resident side holds creation's
 * bytes for the light records, the power table and its running sum (a point light's power stays 0; a total power of 0
 * leaves creation's NaN tables) and, when the range holds the environment-map light, for the map's scale, as
 * take_hip_scene_set_envmap's scale3 sets it.  Only the 3 * count doubles are uploaded: the records are rewritten and
 * the range's powers computed on the device, the serial sum over all lights runs on the host.
 * The _device variant reads d_rgb from device memory after waiting for `stream` (hipStream_t, NULL = default stream),
 * whose work may still be writing the values; it runs on the default stream and returns after it has completed.  It
 * cannot look at the values before they are used: an intensity that is not finite is NOT refused there.
 * The contract of "a resident scene changes" above holds: everything that can fail happens aside, for every side of a
 * MIXED scene, before anything resident changes — a failed call leaves the scene exactly as it was; a successful one
 * ends a progressive sequence.  The marked frame and vertex tracking are left alone (no geometry moved); whether a
 * temporal history made under the old materials or lights is still worth keeping is the caller's decision.  F32, F64
 * and MIXED scenes; flattened, two-level, q8 and host- or device-built scenes alike; not for scene groups.
 * TAKE_E_INVALID before a device is looked for: a NULL scene or array ("null argument"), count <= 0, first < 0 or
 * first + count beyond INT32_MAX, and — host variant — an intensity that is not finite.  After a device was found: a
 * range that ends beyond the scene's table (the handle is not read earlier), an unknown tag, a bad texture image id
 * against the scene's image count, a Burley parameter outside its range.  TAKE_E_NOMEM leaves the scene untouched. */
int take_hip_scene_set_materials(TakeScene *scene, const TakeMaterial *materials, int32_t first, int32_t count);
int take_hip_scene_set_light_intensities(TakeScene *scene, const double *rgb /* 3 * count, host */, int32_t first, int32_t count);
int take_hip_scene_set_light_intensities_device(TakeScene *scene, const double *d_rgb, int32_t first, int32_t count, void *stream);

/* ---- thin-lens camera (EXTENSION; new symbols of ABI version 5; no struct changed): depth of field.  A scene is
 * created with a pinhole camera; take_hip_scene_set_lens gives it a circular aperture of radius aperture_radius (world
 * units) around lookfrom, in the plane spanned by the camera's u and v, focused on the plane perpendicular to the view
 * axis at focus_distance along it.  Every camera ray of a sample then starts at a point of the lens — a concentric
 * (Shirley-Chiu) map of two draws taken from the sample's own key at the counters 0xFFFFFFFE and 0xFFFFFFFF, which no
 * path reaches — and passes through the point of the plane of focus that the sample's pinhole ray passes through: the
 * two jitter draws, the stream counter after them and everything the shade rounds draw are the pinhole render's.
 * What follows the camera ray — take_hip_render*, _render_accumulate, _render_adaptive*, _render_features* (its
 * "exactly the render's camera rays" now are lens rays: depth is the t along the LENS ray, the first-hit guides are
 * means over the blur circle), the denoisers — takes the lens ray from the path record.  The motion pass, the marked
 * frame and the temporal calls are unchanged: their centre rays start at lookfrom, so with a lens the motion vectors,
 * depth and ids are those of the lens CENTRE.  The trace hooks trace the caller's rays as before.
 * set_lens follows the contract of "a resident scene changes" above (a failed call leaves the scene as it was; a
 * successful one ends a progressive sequence; F32, F64 and MIXED scenes, on both sides — the camera rays of a mixed
 * scene are made on its f64 side; not for scene groups).  aperture_radius == 0 returns the scene to the pinhole camera:
 * the kernels it launches and the bits it produces are those of a scene that never had a lens.  focus_distance <= 0
 * asks for |lookat - lookfrom| of the scene's current camera; the effective distance is computed in double and rounded
 * to the side's Real once.  take_hip_scene_set_camera keeps the lens, and an automatic focus follows the new lookat.
 * TAKE_E_INVALID, before a device is looked for: a NULL argument ("null argument"), a radius that is negative or not
 * finite, a focus distance that is not finite, non-zero flags or reserved; then, with a radius > 0, an effective focus
 * distance that is not > 0.
 * get_lens: the request as it was given (zeros before any), with focus_distance replaced by the effective distance.
 * focus_distance_at: what to focus on the surface seen in pixel (column, row; row 0 = the top): the pixel's centre ray
 * from lookfrom — the pinhole ray — is traced through the closest-hit hook (on the f64 side of a MIXED scene) and
 * *distance_out = t * -(w . d), the hit's distance along the view axis, which goes straight into
 * TakeLens::focus_distance; a miss gives 0 and TAKE_OK.  TAKE_E_INVALID: a NULL argument, a pixel outside the image. */
typedef struct TakeLens {
    double aperture_radius;  /* world units; 0 = pinhole */
    double focus_distance;   /* along the view axis; <= 0: |lookat - lookfrom| of the scene's current camera */
    int32_t flags, reserved; /* 0 */
} TakeLens;
int take_hip_scene_set_lens(TakeScene *scene, const TakeLens *lens);
int take_hip_scene_get_lens(const TakeScene *scene, TakeLens *out);
int take_hip_scene_focus_distance_at(TakeScene *scene, int32_t column, int32_t row /* 0 = top */, double *distance_out);

/* ---- motion blur (EXTENSION, parity unpinned; new symbols of ABI version 5; no struct changed; DESIGN.md par. 4l): a
 * render whose exposure lasts from `open` to `close` of the interval between the marked frame (scene time 0:
 * take_hip_scene_mark_frame) and the current one (scene time 1).  Time is sampled per SLICE of samples, not per ray:
 *  - The plan (take_hip_shutter_plan; needs no scene and no device).  K = slices, capped at spp; slices <= 0 asks for
 *    min(spp, 16), an interface default, not a tuned value.  Slice k holds the samples [floor(k spp / K),
 *    floor((k + 1) spp / K)) of every pixel (64-bit integer arithmetic; first_sample gets the K + 1 bounds): contiguous,
 *    covering [0, spp), none empty.  Its time is t_k = open + (close - open) * ((k + 0.5) / K) in double, each operation
 *    one rounding in that order.  The shutter is a box: every sample weighs the same.
 *  - The pose at t (take_hip_shutter_pose).  Every lerp is (1 - t) * a + t * b in double — `1 - t` rounded once, two
 *    products, one sum, no contraction — so t = 0 gives a and t = 1 gives b (as values: a zero comes out as +0 unless
 *    both ends are -0); where a == b the result is b itself (the sum's three roundings would not give it back), so what
 *    did not move between the mark and now stays where it is at every t, bit for bit.  Camera: lookfrom, lookat, up and vfov of the marked and the current TakeCamera, component by
 *    component; width and height are the scene's; the result goes through the arithmetic take_hip_scene_set_camera puts
 *    a camera through.  Placements: the 12 doubles of each object -> world transform, entry by entry, marked -> current:
 *    the matrix motion transform of Embree and OptiX.  A rotation moves along its CHORD, not its arc (a half turn passes
 *    through a singular matrix at t = 0.5): callers with fast rotations mark more often.  The lens (take_hip_scene_set_lens:
 *    radius and effective focus distance) is the current frame's at every t.  Vertices that moved since the mark
 *    (take_hip_scene_set_mesh_vertices / _update_meshes) are at their current positions throughout THESE calls, whether
 *    or not take_hip_scene_track_vertices is on: the scene keeps no second set of vertices.  A caller that has both sets
 *    passes them to take_hip_render_shutter_meshes* below, which lerps them per slice.
 *    xforms_out: 12 * n_instances doubles in host memory, or NULL = not wanted (ignored for a scene without placements).
 *  - The render.  For k = 0 .. K-1 the scene is posed at t_k on the device — the camera records; the placements by the
 *    path take_hip_scene_set_instance_transforms takes, the top level alone rebuilt — and slice k's samples are rendered
 *    on top of the accumulator take_hip_render_accumulate keeps; their numbers continue those of a one-shot render.  One
 *    resolve over spp.  The image is the mean over the samples s = 0 .. spp-1 of "sample s of take_hip_render of the
 *    scene posed at the time of s's slice": with no motion between mark and now it is take_hip_render's image bit for
 *    bit, and with one slice it is the image of a scene newly created (TAKE_BUILDER_DEVICE_LBVH) at the pose of t_0.
 *    Strips, samples_per_batch and the other options as take_hip_render takes them; F32, F64 and MIXED scenes (a mixed
 *    scene is posed on both sides); one- and two-level scenes — a scene without placements gets camera blur, with no
 *    rebuild at all.  The call ends a progressive sequence exactly as take_hip_render does.  Not for scene groups.  The
 *    adaptive, feature, motion and temporal calls are unchanged: they render the current frame.
 *  - Afterwards, on success or failure, the scene is at its current pose again and traces and renders exactly as before
 *    the call (hit tables, occlusion, images bit for bit); the mark, the current transforms and the current camera are
 *    untouched.  As after any re-pose, a host-built top level may have become an LBVH one (take_hip_scene_stats).
 * TAKE_E_INVALID, before a device is looked for: a NULL argument ("null argument"; `shutter` may be NULL = {0, 1, 0, 0}),
 * open / close not finite or outside 0 <= open <= close <= 1 (shutter_pose: t outside [0, 1]), non-zero flags, spp <= 0.
 * Then: no marked frame (the motion pass's message); what take_hip_scene_set_instance_transforms refuses of the scene
 * ("unsupported": TAKE_HIP_BRAID > 1, TAKE_HIP_NODES=q8); a pose that is singular (|det| <= 1e-300) or not finite, or a
 * camera whose lookat coincides with its lookfrom, at ANY slice time — found for all K slices before the first sample is
 * rendered; the message names the first such slice (and placement).  A refusal that can only appear in the loop (a
 * top-level tree too deep at some slice) restores the current pose before it returns. */
typedef struct TakeShutter {
    double open, close;  /* scene time: 0 = the marked frame, 1 = the current frame; 0 <= open <= close <= 1 */
    int32_t slices;      /* K >= 1; <= 0: the default, min(spp, 16) */
    int32_t flags;       /* 0 */
} TakeShutter;
int take_hip_shutter_plan(int32_t spp, const TakeShutter *shutter /* NULL = {0, 1, 0, 0} */,
                          int32_t *slices_out, int32_t *first_sample /* K + 1, may be NULL */, double *time /* K, may be NULL */);
int take_hip_shutter_pose(TakeScene *scene, double t, TakeCamera *camera_out, double *xforms_out /* 12 * n_instances, host; NULL = not wanted */);
int take_hip_render_shutter_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeShutter *shutter, void *d_rgb_out, void *stream);
int take_hip_render_shutter(TakeScene *scene, const TakeRenderOpts *opts, const TakeShutter *shutter, void *rgb_out_host);
/* Motion blur for deforming meshes (EXTENSION, parity unpinned; new symbols of ABI version 5; no struct changed;
 * DESIGN.md par. 4r): take_hip_render_shutter* with one addition — for every slice k, before its samples are rendered,
 * the named meshes are at the lerp of their two vertex arrays at t_k.
 *  - The arithmetic.  Every coordinate of a position, and every component of a vertex normal, is the shutter's lerp
 *    above ((1 - t) * a + t * b in double, `1 - t` rounded once, no contraction; b itself where a == b), so t = 0 gives
 *    the marked array, t = 1 the current one, and a vertex that did not move stays where it is bit for bit at every t.
 *    A vertex moves along its CHORD.  Normals are lerped component by component and NOT renormalised: the shading
 *    normal is normalised at every hit after the barycentric blend, into which the shorter lerped normals enter with a
 *    slightly smaller weight.  Values that are not finite pass through; refusing them is the update's business.
 *  - take_hip_shutter_vertices* needs no scene: the lerp of n doubles (3 * n_vertices) at one t, on the device — what
 *    take_hip_shutter_pose is for placements.  *moved (NULL = not wanted) becomes 1 where any out[e] differs bit for bit
 *    from b[e], else 0.  The _device variant reads and writes device memory on `stream` (hipStream_t, NULL = the default
 *    stream) and returns after it has completed; d_out may be d_a or d_b.
 *  - The render.  PRECONDITION: the scene's meshes are at positions1 / normals1 — the caller has updated them
 *    (take_hip_scene_update_meshes, take_hip_scene_pose_meshes); the call cannot check this and relies on it only where
 *    it skips work.  Per named mesh one buffer for positions (and one for normals) is allocated, and host arrays are
 *    uploaded, once, before the first slice.  Per slice the vertices are made in those buffers and the scene takes
 *    take_hip_scene_update_meshes' staged path over them — in a two-level scene under THAT SLICE's posed transforms, the
 *    placements' records and the one top-level rebuild serving both — so area lights on moved faces get their records
 *    and power tables as in an update.  A slice whose vertices are the current ones bit for bit, in a scene that is at
 *    them, runs no update: with n = 0, or positions0 == positions1 in value, the call IS take_hip_render_shutter — same
 *    launches, same image.  These updates are internal: the mark, vertex tracking (take_hip_scene_tracking_info, the
 *    marked geometry) and `updated since the mark` are left as they were.
 *  - Afterwards, on success or failure: if any slice updated the meshes they are updated once more with positions1 /
 *    normals1 under the current transforms, camera and placements are restored as by take_hip_render_shutter, and the
 *    scene traces and renders exactly as after take_hip_scene_update_meshes with the ...1 arrays — for a scene that was
 *    at them already, hit tables, occlusion and images are bit for bit those before the call.  As after any update,
 *    take_hip_scene_build_info and take_hip_scene_stats may report the device builder's tree.  A progressive sequence
 *    ends as take_hip_render_shutter ends it.  F32, F64 and MIXED scenes (both sides), one- and two-level; strips,
 *    samples_per_batch and a lens as take_hip_render_shutter.  Not for scene groups.
 * Still open: interpolating the POSE of a rig instead of its vertices (arcs for joints), a time per ray, scene groups.
 * TAKE_E_INVALID, before a device is looked for: everything take_hip_render_shutter* refuses there; n < 0; motions
 * NULL with n > 0; positions0 or positions1 NULL; one of normals0 / normals1 without the other; unknown flag bits; a
 * negative mesh index; a mesh named twice.  shutter_vertices: a NULL a, b or out, n <= 0, t outside [0, 1].  Against
 * the scene: a mesh index out of range; normals for a mesh without vertex normals; no marked frame; every
 * "unsupported" case of take_hip_scene_update_meshes, in its words.  In the loop: the update's own refusals (a vertex
 * that is not finite, a tree too deep), prefixed with "slice k: "; the scene is restored before the call returns.
 * TAKE_E_NOMEM: no room for the buffers, before anything changed. */
typedef struct TakeMeshMotion {
    int32_t mesh;              /* index into the TakeSceneDesc.meshes the scene was created from */
    int32_t flags;             /* 0, or TAKE_MESH_DEVICE_ARRAYS: all four pointers are device memory */
    const double *positions0;  /* n_vertices x 3 at the marked frame (scene time 0); required */
    const double *positions1;  /* n_vertices x 3 at the current frame (scene time 1); required */
    const double *normals0;    /* both or neither; only for a mesh that has vertex normals */
    const double *normals1;
} TakeMeshMotion;
int take_hip_shutter_vertices(const double *a, const double *b, int64_t n, double t, double *out, int32_t *moved /* NULL ok */);
int take_hip_shutter_vertices_device(const double *d_a, const double *d_b, int64_t n, double t, double *d_out, int32_t *moved_host, void *stream);
int take_hip_render_shutter_meshes(TakeScene *scene, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n,
                                   void *rgb_out_host);
int take_hip_render_shutter_meshes_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeShutter *shutter, const TakeMeshMotion *motions, int32_t n,
                                          void *d_rgb_out, void *stream);

/* Replaces the parallel_for tile loop of render() (src/render.cpp:59-82) and all it
 * calls.  rgb_out: this rank's rows only, compacted in increasing image-row order
 * (n_rows(strip_first, strip_stride) * width * 3 Real), already flipped as
 * `img(x, height-y-1)` (src/render.cpp:78) and divided by spp.  f32 scenes write
 * float, f64 scenes write double.  `take_hip_render_rows` returns how many rows. */
int take_hip_render(TakeScene *scene, const TakeRenderOpts *opts, void *rgb_out_host);
/* Same, output left in device memory (d_rgb_out = device pointer), enqueued on
 * `stream` (hipStream_t, NULL = default stream); returns after enqueue + sync. */
int take_hip_render_device(TakeScene *scene, const TakeRenderOpts *opts, void *d_rgb_out,
                           void *stream);
/* Progressive / interactive rendering: the per-pixel accumulate of the tile loop
 * (src/render.cpp:68-78) kept resident in HBM between calls.  Renders opts->spp MORE samples per pixel on top of
 * what the scene has accumulated since the last call with restart != 0 (or since a one-shot take_hip_render*, which
 * ends a sequence), and writes the mean over ALL samples so far to d_rgb_out (device memory, same layout as
 * take_hip_render_device).  The samples continue the one-shot render's numbering — same random streams, same order of
 * the additions — so after calls with a, b, c.. samples the image equals take_hip_render(spp = a + b + c ..) BIT FOR
 * BIT.  seed, max_depth, integrator, ray_epsilon, the strip set and — on mixed scenes — the effective exact_bounces
 * must stay the same within a sequence (TAKE_E_INVALID otherwise).  take_hip_accumulated_samples: samples per pixel in the accumulator. */
int take_hip_render_accumulate(TakeScene *scene, const TakeRenderOpts *opts, int32_t restart, void *d_rgb_out,
                               void *stream);
int64_t take_hip_accumulated_samples(const TakeScene *scene);
/* Egress on the device: the conversion half of the reference's imwrite("image.exr") (src/image.cpp:155-176 ->
 * tinyexr SaveEXR(components 3, fp16)).  d_rgb: height * width * 3 Real in device memory (row 0 = top, as
 * take_hip_render_device leaves it; precision says float or double) -> d_out: uint16 [height][3][width], per
 * scanline the channels B, G, R as half bit patterns rounded as that writer rounds (half-up on the first dropped
 * bit) — the bytes of an EXR scanline block before its ZIP pre-filter; the host deflates and frames them
 * (take_amd/exr.py: write_exr_scanlines).  Enqueued on `stream`, returns after it has completed. */
int take_hip_pack_exr_scanlines(const void *d_rgb, int32_t precision, int32_t width, int32_t height, uint16_t *d_out,
                                void *stream);
/* Render the whole image (strip_first / strip_stride are ignored) and hand back those scanlines in host memory
 * (height * 3 * width uint16): the float framebuffer never leaves the device. */
int take_hip_render_exr_scanlines(TakeScene *scene, const TakeRenderOpts *opts, uint16_t *out_host);

/* ---- first-hit feature buffers: the auxiliary images a denoiser or compositor asks a path tracer for — albedo,
 * shading normal, depth, coverage and the ids of the camera ray's hit — made on the device from the resident scene
 * (one closest-hit launch + one streaming kernel per batch: no sort, no shade round, no shadow rays).
 * Samples: the camera rays are exactly the ones take_hip_render traces for the same seed, spp, strip set and
 * ray_epsilon (pixel key, sample index, the two jitter draws — y before x —, tmin).  samples_per_batch is honoured;
 * max_depth, integrator and exact_bounces are ignored.
 * Per sample that hits: albedo = the reflectance texture of the hit's material at the hit's uv (the placement's material
 * where it overrides the prototype's; an emitter is a surface like any other; the Disney / Burley tags use their
 * reflectance); normal = the shading normal in world space (through the transposed inverse on placements), facing
 * as the reference's Intersection leaves it; depth = the hit's t; alpha = 1.  A sample that misses adds 0 to all
 * four, with or without an environment map.
 * Per pixel: the sum over the samples IN SAMPLE ORDER divided by spp — alpha-premultiplied; the normal is not
 * re-normalised.  shape_id / material_id: those of SAMPLE 0's hit, -1 / -1 where it misses; shape ids as the trace
 * hooks number them (placements: n_shapes + faces of the preceding placements + face).
 * Layout: this rank's rows, compacted, row 0 = the top of the image (as take_hip_render_device); the albedo and
 * normal planes can go straight into take_hip_pack_exr_scanlines.  f32 scenes write float, f64 and MIXED scenes
 * double (a MIXED scene uses its f64 side: the planes are the F64 scene's bit for bit).
 * The planes are bit-identical for any samples_per_batch and any strip sharding.
 * The call has per-pixel sums of its own: a progressive sequence (take_hip_render_accumulate,
 * take_hip_accumulated_samples) goes on after it as if it had not happened.  take_hip_get_counters afterwards:
 * samples, rays_closest and the timing fields as after a render; ms_shade is the time of the feature kernel.
 * TAKE_E_INVALID: a NULL scene, opts or buffers ("null argument", before a device is looked for), spp <= 0, a bad
 * strip pair, all six pointers NULL; a failed call leaves the scene as it was.  Not for scene groups. */
typedef struct TakeFeatureBuffers { /* every pointer may be NULL = not wanted */
    void *albedo;         /* n_rows * width * 3 Real */
    void *normal;         /* n_rows * width * 3 Real */
    void *depth;          /* n_rows * width Real     */
    void *alpha;          /* n_rows * width Real     */
    int32_t *shape_id;    /* n_rows * width          */
    int32_t *material_id; /* n_rows * width          */
} TakeFeatureBuffers;
/* d_out: pointers to device memory; enqueued on `stream`, returns after it has completed */
int take_hip_render_features_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeFeatureBuffers *d_out,
                                    void *stream);
/* host_out: pointers to host memory */
int take_hip_render_features(TakeScene *scene, const TakeRenderOpts *opts, const TakeFeatureBuffers *host_out);

/* ---- image-space denoiser (new symbols of ABI version 5; no struct changed): the edge-avoiding A-trous wavelet filter
 * of Dammertz et al. 2010 on the device, guided by the first-hit feature buffers.  EXTENSION without an upstream
 * counterpart — parity unpinned with respect to the reference; specified against its own f64 restatement
 * (tests/denoise_ref.py; DESIGN.md par. 4f has the arithmetic operation by operation).
 * Planes as take_hip_render_device and take_hip_render_features_device leave them: rgb height * width * 3 Real, row 0 =
 * top; guides (each optional): albedo and normal height * width * 3, depth height * width; Real = float or double by
 * `precision`; out height * width * 3 Real, and may be rgb itself (no other aliasing).
 * With an albedo (and without TAKE_DENOISE_KEEP_ALBEDO) the image is demodulated first — divided per channel by
 * max(albedo, albedo_floor) — and multiplied back at the end, so that texture detail is not filtered, only illumination.
 * Then `iterations` levels i = 0.., each a 5 x 5 B3-spline kernel (3/8, 1/4, 1/16) with holes of 2^i pixels, taps
 * outside the image skipped, every tap weighted by exp(-(|dc|^2 * 4^i / sigma_color^2 + |dn|^2 / sigma_normal^2 +
 * (dD / max(|D(p)|, |D(q)|))^2 / sigma_depth^2)): the colour sigma halves every level, the depth distance is relative
 * and symmetric (two misses, both at depth 0, are at distance 0).  exp is the library's exp / expf.  Deterministic:
 * the same planes give the same bits.  Non-finite inputs are taken as they are: a NaN or an infinity spreads through
 * every pixel whose footprint holds it.
 * The defaults are starting values: they have not been tuned on any image beyond the one condition the tests hold them
 * to (a 4-spp Cornell box gets closer to its 1024-spp render). */
#define TAKE_DENOISE_KEEP_ALBEDO 1 /* do not demodulate: filter rgb as it is even when an albedo is given */
typedef struct TakeDenoiseOpts {
    int32_t iterations;            /* 1..8; <= 0: 5 */
    int32_t flags;                 /* 0 or TAKE_DENOISE_KEEP_ALBEDO */
    double sigma_color;            /* <= 0: 1.0  */
    double sigma_normal;           /* <= 0: 0.3  */
    double sigma_depth;            /* <= 0: 0.05 */
    double albedo_floor;           /* <= 0: 1e-3 */
} TakeDenoiseOpts;
/* Needs no scene (as take_hip_pack_exr_scanlines does not): also for the output of take_hip_render_accumulate or of a
 * scene group.  d_rgb, d_out and the guides' pointers are device memory of the current device; d_guides: NULL = no
 * guides, otherwise its albedo / normal / depth are read (each may be NULL) and the rest ignored; opts: NULL =
 * defaults.  The two working images are allocated per call.  Enqueued on `stream`, returns after it has completed.
 * TAKE_E_INVALID, checked before a device is looked for: a NULL d_rgb / d_out ("null argument"), width or height <= 0,
 * an unknown precision (MIXED is a scene's, not a plane's: its planes are F64), iterations > 8, an unknown flag bit, a
 * sigma or floor that is not finite. */
int take_hip_denoise_device(const void *d_rgb, const TakeFeatureBuffers *d_guides, int32_t precision, int32_t width,
                            int32_t height, const TakeDenoiseOpts *opts, void *d_out, void *stream);
/* the same with host pointers (upload, the same kernels, download) */
int take_hip_denoise(const void *rgb, const TakeFeatureBuffers *guides, int32_t precision, int32_t width, int32_t height,
                     const TakeDenoiseOpts *opts, void *out);
/* Render the whole image (strip_first / strip_stride are ignored, as in take_hip_render_exr_scanlines), make albedo,
 * normal and depth with the same options, filter — all on the device, the planes and working images kept in the
 * handle.  Specified as, and bit for bit equal to, take_hip_render_device + take_hip_render_features_device +
 * take_hip_denoise_device made by hand: a progressive sequence ends as take_hip_render_device ends it, the counters are
 * the feature pass's.  f32 scenes write float, f64 and MIXED scenes double.  Not for scene groups.
 * TAKE_E_INVALID: a NULL scene, render options or output ("null argument"), and what take_hip_denoise_device refuses
 * of the denoise options, before a device is looked for; then what the render refuses. */
int take_hip_render_denoised_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeDenoiseOpts *denoise,
                                    void *d_out, void *stream);
int take_hip_render_denoised(TakeScene *scene, const TakeRenderOpts *opts, const TakeDenoiseOpts *denoise,
                             void *rgb_out_host);

/* ---- adaptive sampling (new symbols of ABI version 5; no struct changed): a pixel stops receiving samples once the
 * relative standard error of its mean is at or below a threshold.  EXTENSION without an upstream counterpart — parity
 * unpinned with respect to the reference: the sample values are the pinned render's, only the stopping rule is this
 * library's own (restated in tests/adaptive_ref.py; DESIGN.md par. 4g).
 * opts->spp is the MAXIMUM per pixel.  Pass 0 gives every pixel the samples 0 .. min_spp - 1; pass i >= 1 gives every
 * pixel still active the next min(step_spp, spp - n) samples; the active set only shrinks, so all active pixels have
 * the same number n of samples.  Per pixel, in sample order and in double whatever the scene's precision:
 *   L_s = ((double)r + (double)g) + (double)b of sample s — the values the image sums take (on MIXED scenes the
 *   per-channel doubles f64 record + converted f32 record) —, m1 += L_s, m2 += L_s * L_s.
 * After a pass, for a pixel with n samples (each + - * / sqrt one IEEE operation in this order):
 *   mean = m1 / n;  v = m2 / n - mean * mean;  v = v > 0 ? v : 0;  err = sqrt(v / (n - 1)) / (fabs(mean) + floor)
 * and the pixel stops iff (n >= 2 && err <= threshold) or n == spp.  A NaN err never satisfies <=: such a pixel runs
 * to spp.  A stopped pixel never restarts.  rgb = the render's own sums * (1 / count), flipped as take_hip_render_device.
 * Consequences: a pixel with count c equals take_hip_render(spp = c) there BIT FOR BIT; image, counts and moments do
 * not depend on samples_per_batch, on the strip set (pixel lists are local to the rank's rows) or on the run.  Like
 * every threshold rule the image is a biased estimate (pixels whose first samples happen to agree stop early): min_spp
 * is the guard.
 * MIXED, two-level and device-built scenes work; only the default integrator (0); not for scene groups.  Afterwards as
 * after take_hip_render_device: a progressive sequence has ended (take_hip_accumulated_samples() == 0), and
 * TakeCounters.samples is the sum of the counts.
 * TAKE_E_INVALID, checked before a device is looked for: a NULL scene, opts or rgb ("null argument"), a threshold or
 * floor that is not finite, an unknown flag bit; then integrators 1..3 and whatever a render refuses. */
typedef struct TakeAdaptiveOpts {
    int32_t min_spp;    /* samples every pixel gets before the first test; <= 0: 16; clamped to opts->spp */
    int32_t step_spp;   /* samples added per later pass to every pixel still active; <= 0: 8 */
    double threshold;   /* relative standard error of the mean at which a pixel stops; < 0: 0.05;
                           0 is a value (only pixels with zero sample variance stop) */
    double floor;       /* added to |mean| in the denominator; <= 0: 1e-3 */
    int32_t flags, reserved; /* 0 */
} TakeAdaptiveOpts;
typedef struct TakeAdaptiveStats { /* every pointer may be NULL; n_rows * width planes, row 0 = top, as rgb */
    int32_t *count;     /* samples the pixel received */
    double *m1, *m2;    /* sum of L_s and of L_s * L_s over those samples, always double */
} TakeAdaptiveStats;
/* d_rgb_out and the planes of d_stats: device memory; enqueued on `stream`, returns after it has completed */
int take_hip_render_adaptive_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeAdaptiveOpts *adaptive /* NULL = defaults */,
                                    void *d_rgb_out, const TakeAdaptiveStats *d_stats /* NULL ok */, void *stream);
/* the same with host pointers */
int take_hip_render_adaptive(TakeScene *scene, const TakeRenderOpts *opts, const TakeAdaptiveOpts *adaptive, void *rgb_out_host,
                             const TakeAdaptiveStats *host_stats);

/* ---- variance-guided denoiser (new symbols of ABI version 5; no struct changed): the spatial half of SVGF (Schied et
 * al. 2017) — the A-trous filter above, but the colour term of a tap is scaled by the pixel's own estimated standard
 * deviation, taken from the moment planes the adaptive sampler leaves (TakeAdaptiveStats), and that variance is
 * filtered along with the colour, so that later levels stop blurring once the estimate is clean.  (The temporal half:
 * take_hip_temporal_accumulate* below.)  No trained weights; deterministic.  EXTENSION without an upstream counterpart — parity unpinned with respect to the
 * reference; specified against its own f64 restatement (tests/denoise_var_ref.py; DESIGN.md par. 4h has the arithmetic
 * operation by operation).
 * Planes as take_hip_denoise_device takes them, and the three of TakeAdaptiveStats as take_hip_render_adaptive_device
 * leaves them: count int32, m1 and m2 double (always), height * width, row 0 = top; the moments are of L_s = (r + g) + b
 * of the raw radiance.  Real = float or double by `precision`; every + - * / is one operation of Real in the order
 * written, constants are computed in double and rounded once, exp is the library's, TINY the smallest normal Real.
 * Options: TakeDenoiseOpts, but sigma_color <= 0 means 4.0 in these calls — it is a multiple of the pixel's standard
 * deviation, not a radiance; the other defaults as above.
 *   Initial variance of the pixel mean, in double with the operations of the adaptive rule:
 *     n = (double)count;  mean = m1 / n;  v = m2 / n - mean * mean;  v = v > 0 ? v : 0;
 *     s2 = count >= 2 ? v / (n - 1) : mean * mean   (one sample: 100 % relative error; count <= 0: 0 / 0 = NaN, taken
 *     as it is);  V0 = (Real)s2.
 *   Demodulate (with an albedo and without TAKE_DENOISE_KEEP_ALBEDO): A = max(albedo, floor) per channel, C0 = rgb / A,
 *     Am = ((A.r + A.g) + A.b) * (Real)(1.0 / 3.0), V0 = V0 / (Am * Am); otherwise C0 = rgb.
 *   Level i = 0 .. iterations - 1, s = 2^i, at every pixel p:
 *     gv = sum of k3 * V_i(q) / sum of k3 over the 3 x 3 taps at unit spacing (dy outer, dx inner, taps outside the
 *       image skipped), k3 = g[|dx|] * g[|dy|], g = {1/2, 1/4};
 *     inv_c = 1 / (sigma_color^2 * gv + TINY)   (no 4^i: the variance falls by itself as the filter averages);
 *     the 5 x 5 taps q = p + s * (dx, dy) as above, k = h[|dx|] * h[|dy|], l(X) = (X.r + X.g) + X.b:
 *       dl = l(C_i(p)) - l(C_i(q));  x = (dl * dl) * inv_c (+inf gives weight 0), plus the normal and depth terms as
 *       above;  w = k * exp(-x);  num += w * C_i(q);  nv += (w * w) * V_i(q);  den += w;
 *     C_{i+1}(p) = num / den;  V_{i+1}(p) = nv / (den * den).
 *   Remodulate: out = C_n * A (or C_n); variance_out (optional, height * width Real) = V_n * (Am * Am) (or V_n): the
 *     filter's own estimate of the variance of l(out).
 * out may be rgb itself; no other aliasing.  The defaults are starting values, held to one condition by the tests (an
 * 8-spp Cornell box gets closer to its 1024-spp render).
 * Needs no scene; the working images are allocated per call; enqueued on `stream`, returns after it has completed.
 * TAKE_E_INVALID, checked before a device is looked for: a NULL d_rgb / d_out / d_stats or any of d_stats' three
 * pointers NULL ("null argument"), and everything take_hip_denoise_device refuses. */
int take_hip_denoise_variance_device(const void *d_rgb, const TakeFeatureBuffers *d_guides, const TakeAdaptiveStats *d_stats,
                                     int32_t precision, int32_t width, int32_t height, const TakeDenoiseOpts *opts,
                                     void *d_out, void *d_variance_out /* NULL ok */, void *stream);
/* the same with host pointers (upload, the same kernels, download) */
int take_hip_denoise_variance(const void *rgb, const TakeFeatureBuffers *guides, const TakeAdaptiveStats *stats,
                              int32_t precision, int32_t width, int32_t height, const TakeDenoiseOpts *opts, void *out,
                              void *variance_out /* NULL ok */);
/* Render the whole image adaptively (strip_first / strip_stride are ignored, as in take_hip_render_denoised_device),
 * make albedo, normal and depth, filter with the sampler's own moments — all on the device, the planes and working
 * images kept in the handle.  Specified as, and bit for bit equal to, three calls made by hand:
 * take_hip_render_adaptive_device; take_hip_render_features_device with the same options but spp = the effective
 * min_spp (after the defaults and the clamp to opts->spp: the samples every pixel has, so the guide pass does not grow
 * with the maximum); take_hip_denoise_variance_device in place.  d_stats: optional OUTPUTS (every pointer may be NULL,
 * as in take_hip_render_adaptive_device), d_variance_out optional.  Afterwards a progressive sequence has ended; the
 * counters are the feature pass's.  f32 scenes use float planes, f64 and MIXED scenes double.  Not for scene groups.
 * TAKE_E_INVALID: a NULL scene, render options or output ("null argument"), what take_hip_render_adaptive_device
 * refuses of the adaptive options, what take_hip_denoise_device refuses of the denoise options, in that order and
 * before a device is looked for; then what the adaptive render refuses. */
int take_hip_render_adaptive_denoised_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeAdaptiveOpts *adaptive,
                                             const TakeDenoiseOpts *denoise, void *d_out,
                                             const TakeAdaptiveStats *d_stats /* NULL ok: optional outputs */,
                                             void *d_variance_out /* NULL ok */, void *stream);
/* the same with host pointers */
int take_hip_render_adaptive_denoised(TakeScene *scene, const TakeRenderOpts *opts, const TakeAdaptiveOpts *adaptive,
                                      const TakeDenoiseOpts *denoise, void *rgb_out_host,
                                      const TakeAdaptiveStats *host_stats /* NULL ok */, void *variance_out_host /* NULL ok */);

/* ---- temporal reprojection and accumulation (new symbols of ABI version 5; no struct changed): the temporal half of
 * SVGF (Schied et al. 2017) — a frame of an animation starts from the samples of the frames before it, fetched through
 * per-pixel motion vectors that only the scene can make (it alone knows the previous camera and placements), tested
 * tap by tap and blended sample count by sample count.  EXTENSION without an upstream counterpart — parity unpinned
 * with respect to the reference; specified against its own restatement (tests/temporal_ref.py; DESIGN.md par. 4i has the
 * arithmetic operation by operation).  No trained weights; deterministic.
 *
 * take_hip_scene_mark_frame: stores "the previous frame" in the handle — the current camera of every resident side and,
 * in a two-level scene, a device copy of the placements' current object -> world transforms (12 doubles each, as
 * take_hip_scene_set_instance_transforms takes them).  A later mark replaces the earlier one;
 * take_hip_scene_set_camera, _set_instance_transforms, _set_mesh_vertices and _update_meshes leave it alone (the
 * placement count cannot change under them).  The vertices of the marked frame are not stored, and a vertex that moves
 * after the mark is not followed, unless tracking is on (take_hip_scene_track_vertices, below).  TAKE_E_INVALID: a NULL
 * scene ("null argument", before a device is looked for).  Not for scene groups. */
int take_hip_scene_mark_frame(TakeScene *scene);

/* take_hip_scene_track_vertices: lets the motion pass follow vertices that moved since the mark (a deforming mesh).
 * flags: 0 = off, the default — every call is what it is without these two symbols, bit for bit, and no update call
 * costs a byte or a launch more — or TAKE_TRACK_VERTICES.  With tracking on and a mark set, the FIRST successful
 * take_hip_scene_set_mesh_vertices / _update_meshes after that mark keeps the geometry words of every triangle record
 * as they were (copy on write: a mark with no update after it costs nothing; 9 Real per record of the side the motion
 * pass runs on, held as 12 — 48 bytes per record in f32, 96 in f64 — keyed by shape id, and by prototype and face for a
 * prototype's records, which survive the rebuild's new leaf order).  Further updates before the next mark leave the
 * copy alone: the marked frame stays the frame at the mark.  take_hip_scene_mark_frame drops it, and so does turning
 * tracking off; tracking turned on after an update holds nothing until the next mark.  The copy is staged with the
 * update: a failed update leaves it as it was, and an update that cannot allocate it fails as a whole with TAKE_E_NOMEM
 * ("out of device memory for the marked frame's geometry").  Spheres do not move; topology does not change.
 * TAKE_E_INVALID: a NULL scene ("null argument"), any other bit ("unknown flag bits") — both before a device is looked
 * for.  Not for scene groups.
 * take_hip_scene_tracking_info: the flags, and the device bytes of marked geometry the handle holds (0: none — the
 * motion pass is then the one that follows no vertices).  Either out may be NULL. */
#define TAKE_TRACK_VERTICES 1
int take_hip_scene_track_vertices(TakeScene *scene, int32_t flags);
int take_hip_scene_tracking_info(const TakeScene *scene, int32_t *flags, int64_t *marked_bytes);

/* The motion pass: ONE ray per pixel through the pixel's centre (the camera ray of a render with 0.5 in place of the
 * two jitter draws), made by the closest-hit launch that traces it, then one streaming kernel.  Of the options only
 * ray_epsilon is read; the pass always covers the whole image (as take_hip_render_denoised_device); a MIXED scene uses
 * its f64 side (as the feature pass).  Per pixel, in the side's Real, every + - * / sqrt one operation in this order,
 * dot products (a.x * b.x + a.y * b.y) + a.z * b.z, a 3 x 4 map applied row by row as ((m0 * x + m1 * y) + m2 * z) + m3:
 *   a hit at t:  P = o + d * t;  in placement i:  P' = M_i(marked) * (inv_i(current) * P) with the marked transform's
 *     doubles rounded to Real, otherwise P' = P (a vertex that moved since the mark is not followed: the surface counts
 *     as rigid in its mesh; the validity tests of the accumulation reject what no longer matches — unless tracking is
 *     on and the handle holds marked geometry: then a TRIANGLE hit with barycentrics u, v and the marked words v0', e1',
 *     e2' of its record has Q' = (v0' + e1' * u) + e2' * v per component, P' = M_i(marked) * Q' in placement i — no
 *     inverse — and P' = Q' otherwise; sphere hits and misses are as without tracking);  e = P' - lookfrom';
 *   a miss:  e = d (a point at infinity), depth = prev_depth = 0, shape_id = -1 — a static camera keeps its background
 *     history, a rotating one moves it;
 *   with the MARKED camera (u', v', w', lookfrom', viewport'):  z = -(w' . e);  z <= 0: prev_xy = (-2, -2), prev_depth =
 *     0;  otherwise sx = ((u' . e) / z / viewport_width' + 0.5) * width,  sy = ((v' . e) / z / viewport_height' + 0.5) *
 *     height,  prev_xy = (sx, height - sy),  prev_depth = |e| = sqrt(e . e) for a hit.
 * A render, a progressive sequence and the feature planes afterwards are what they were before; the counters are the
 * pass's own (samples = pixels).
 * TAKE_E_INVALID: a NULL scene, opts or buffers ("null argument"), all four pointers NULL — both before a device is
 * looked for —, no marked frame (the message says so); a failed call leaves the scene as it was.  Not for scene groups. */
typedef struct TakeMotionBuffers { /* every pointer may be NULL = not wanted; planes height * width, row 0 = top */
    void *prev_xy;      /* 2 Real: where this pixel's surface point was in the marked frame, in plane coordinates
                           (column, row), a pixel's centre at +0.5; (-2, -2) = nowhere */
    void *prev_depth;   /* Real: the distance of that point from the marked camera's lookfrom (0 for a miss) */
    void *depth;        /* Real: t of this frame's centre ray (0 for a miss) */
    int32_t *shape_id;  /* the centre ray's hit, numbered as the trace hooks number it; -1 = miss */
} TakeMotionBuffers;
/* d_out: pointers to device memory; enqueued on `stream`, returns after it has completed */
int take_hip_render_motion_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeMotionBuffers *d_out, void *stream);
/* host_out: pointers to host memory */
int take_hip_render_motion(TakeScene *scene, const TakeRenderOpts *opts, const TakeMotionBuffers *host_out);

/* Accumulate: needs no scene (as take_hip_denoise_device).  Real = float or double by `precision`; the footprint, the
 * weights, the depth test and the colour are Real, the moments and the history length double (with (double)w and
 * (double)W); every + - * / is one operation in the order written; depth_tol is rounded to Real once.
 * Per pixel p, with (px, py) = prev_xy(p):  fx = px - 0.5, x0 = floor(fx), tx = fx - x0, the same for y;  the taps q =
 * (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) in this order with weights w = (1 - tx) * (1 - ty), tx * (1 - ty),
 * (1 - tx) * ty, tx * ty.  A tap counts only if its weight is > 0, it is inside the image, count_h(q) > 0, where both
 * frames have ids shape_id_h(q) == shape_id_cur(p), and where the history has a depth plane and prev_depth is given
 * |depth_h(q) - prev_depth(p)| <= depth_tol * prev_depth(p).  W = the sum of the weights that count (every sum below
 * runs over the taps that count, in tap order).  W == 0 (a prev_xy that is not a number among the cases), or no
 * history: the output is the current frame bit for bit.  Otherwise, with c = count_cur(p) and n_h(q) = count_h(q):
 *   rgb_h = sum(w * rgb_h(q)) / W;  a_h = sum(w * (m1_h(q) / n_h(q))) / W;  b_h = sum(w * (m2_h(q) / n_h(q))) / W;
 *   n_r = sum(w * n_h(q)) / W;  n_h = min((int32)floor(n_r + 0.5), max_history);  n = n_h + c;
 *   rgb = (rgb_h * n_h + rgb_cur * c) / n;  m1 = a_h * n_h + m1_cur;  m2 = b_h * n_h + m2_cur;  count = n;
 * the output's depth and shape_id (where given, and the current frame has them) are the current frame's.
 * The output is TakeAdaptiveStats-shaped: it goes into take_hip_denoise_variance* unchanged, where it reads as an
 * adaptive render with larger counts, and it is the next frame's history; clamping n_h makes the blend exponential
 * once a pixel carries max_history samples.  d_out must not alias d_hist (the taps gather); it may alias d_cur.
 * TAKE_E_INVALID, checked before a device is looked for: a NULL d_cur / d_out / d_prev_xy or any of the two frames'
 * rgb / count / m1 / m2 ("null argument"), an unknown precision, width or height <= 0, a flag bit, a depth_tol that is
 * not finite, a history that is given but lacks one of rgb / count / m1 / m2. */
typedef struct TakeTemporalFrame {   /* one frame's planes, height * width, row 0 = top */
    void *rgb;                       /* 3 Real: the mean over `count` samples */
    int32_t *count; double *m1, *m2; /* as TakeAdaptiveStats */
    void *depth; int32_t *shape_id;  /* the centre-ray planes of the motion pass; each may be NULL = that test is off */
} TakeTemporalFrame;
typedef struct TakeTemporalOpts {
    int32_t max_history; /* samples of history a pixel may carry; <= 0: 64 */
    int32_t flags;       /* 0 */
    double depth_tol;    /* relative; <= 0: 0.05 */
} TakeTemporalOpts;
/* the frames' planes, d_prev_xy and d_prev_depth: device memory; opts: NULL = defaults; enqueued on `stream`, returns
 * after it has completed */
int take_hip_temporal_accumulate_device(const TakeTemporalFrame *d_cur, const TakeTemporalFrame *d_hist /* NULL = none */,
                                        const void *d_prev_xy, const void *d_prev_depth /* NULL ok */, int32_t precision, int32_t width,
                                        int32_t height, const TakeTemporalOpts *opts, const TakeTemporalFrame *d_out, void *stream);
/* the same with host pointers (upload, the same kernel, download) */
int take_hip_temporal_accumulate(const TakeTemporalFrame *cur, const TakeTemporalFrame *hist /* NULL = none */, const void *prev_xy,
                                 const void *prev_depth /* NULL ok */, int32_t precision, int32_t width, int32_t height,
                                 const TakeTemporalOpts *opts, const TakeTemporalFrame *out);

/* One frame of an animation: render the whole image adaptively, accumulate it onto the handle's history through the
 * motion pass, filter the accumulated image with the accumulated statistics — all on the device, the history kept in
 * the handle (two frames that alternate).  Specified as, and bit for bit equal to, the calls made by hand:
 *   1. take_hip_render_adaptive_device;
 *   2. restart == 0 and the handle has a history: take_hip_render_motion_device (all four planes), then
 *      take_hip_temporal_accumulate_device of the frame (with the motion pass's depth and shape_id) against the history;
 *      otherwise the frame is its own accumulation, its depth and shape_id the motion pass's (which then needs no mark:
 *      by hand, take_hip_scene_mark_frame first);
 *   3. the result becomes the handle's history;
 *   4. take_hip_render_features_device at the effective min_spp (as take_hip_render_adaptive_denoised_device), then
 *      take_hip_denoise_variance_device of the accumulated image with the accumulated count / m1 / m2 into d_out;
 *   5. take_hip_scene_mark_frame.
 * The caller changes opts->seed from frame to frame: a frame with the same seed is the same samples again, and pooling
 * them adds nothing.  The first frame, and one with restart != 0, equals take_hip_render_adaptive_denoised_device.
 * A call that fails before step 3 leaves the history and the mark as they were.  f32 scenes write float, f64 and MIXED
 * scenes double.  Not for scene groups.
 * TAKE_E_INVALID: a NULL scene, render options or output ("null argument"), what take_hip_render_adaptive_device refuses
 * of the adaptive options, what take_hip_temporal_accumulate_device refuses of the temporal options, what
 * take_hip_denoise_device refuses of the denoise options, in that order and before a device is looked for; then what
 * the adaptive render refuses. */
int take_hip_render_temporal_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeAdaptiveOpts *adaptive,
                                    const TakeTemporalOpts *temporal, const TakeDenoiseOpts *denoise, int32_t restart, void *d_out,
                                    void *stream);
/* the same with host pointers */
int take_hip_render_temporal(TakeScene *scene, const TakeRenderOpts *opts, const TakeAdaptiveOpts *adaptive,
                             const TakeTemporalOpts *temporal, const TakeDenoiseOpts *denoise, int32_t restart, void *rgb_out_host);

/* ---- display transform (new symbols of ABI version 5; no struct changed): the last stage of the image-space chain —
 * a luminance histogram made on the device, an auto-exposure derived from it (with temporal adaptation, so that the
 * frames of a sequence share an exposure that follows the scene smoothly), and one fused pass exposure -> tone operator
 * -> sRGB transfer -> 8-bit RGBA.  EXTENSION without an upstream counterpart — parity unpinned with respect to the
 * reference; specified against its own restatement (tests/display_ref.py; DESIGN.md par. 4j has the arithmetic
 * operation by operation).  Scene-free and deterministic: the same planes give the same bits.
 * Planes as take_hip_render_device leaves them: rgb height * width * 3 Real, row 0 = top; Real = float or double by
 * `precision`.
 *
 * The histogram.  Per pixel Y = ((0.2126 r) + (0.7152 g)) + (0.0722 b) in Real (Rec.709), rounded to float (nearest
 * even).  NaN or an infinity — a double beyond float's range included — counts in slot [385]; Y <= 0 in slot [384];
 * every other pixel in bin clamp((float_bits(Y) >> 20) - 8 * (127 - 24), 0, 383): the 8 exponent bits and the top 3
 * mantissa bits, 8 bins per octave over [2^-24, 2^24), what lies outside in the end bins.  No logarithm is taken: the
 * counts are exact, and the 386 slots sum to width * height. */
#define TAKE_LUMINANCE_BINS 384
#define TAKE_LUMINANCE_SLOTS 386 /* the bins, then [384] non-positive, [385] non-finite */
/* d_rgb: device memory of the current device; hist_out_host: TAKE_LUMINANCE_SLOTS counts in HOST memory (both calls).
 * The block histograms and their sum are allocated per call.  Enqueued on `stream`, returns after it has completed.
 * TAKE_E_INVALID, checked before a device is looked for: a NULL pointer ("null argument"), width or height <= 0, an
 * unknown precision (MIXED is a scene's, not a plane's: its planes are F64). */
int take_hip_luminance_histogram_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, int64_t *hist_out_host,
                                        void *stream);
/* the same with a host pointer (upload, the same kernels) */
int take_hip_luminance_histogram(const void *rgb, int32_t precision, int32_t width, int32_t height, int64_t *hist_out);

/* The auto-exposure of a histogram: the factor that takes the log-average luminance of the pixels between two
 * percentiles to `key`.  Host only, in double, needs no device.  In this order:
 *   1. N = the sum of the 384 bins (the two extra slots are left out); N == 0: target = 1, on to step 7;
 *   2. a = low_fraction * N, z = high_fraction * N; the bins in ascending order, c0 the count before bin b, c1 after it;
 *   3. the bin's weight w_b = max(0, min(c1, z) - max(c0, a)): the part of it between the percentiles;
 *   4. its representative log2 luminance l_b = e + log2(1 + (m + 0.5) / 8), e = b / 8 - 24, m = b % 8;
 *   5. mean = sum(w_b l_b) / sum(w_b); if sum(w_b) <= 0, with w_b = the bin's count instead;
 *   6. target = key / exp2(mean);
 *   7. with prev_exposure > 0: E = exp2(log2(prev) + rate * (log2(target) - log2(prev))) — a step of `rate` in log2,
 *      rate 1 jumps to the target; without: E = target;
 *   8. E clamped to [min_exposure, max_exposure].
 * TAKE_E_INVALID: a NULL hist or exposure_out ("null argument"), a negative count in any of the 386 slots, an option
 * that is not finite, low_fraction >= high_fraction, high_fraction > 1, rate > 1, min_exposure > max_exposure (each
 * after the defaults are filled in).  opts: NULL = defaults. */
typedef struct TakeExposureOpts { /* every field: <= 0 (low_fraction: < 0) = its default */
    double key;                   /* <= 0: 0.18 */
    double low_fraction;          /* < 0: 0.05 */
    double high_fraction;         /* <= 0: 0.95 */
    double min_exposure;          /* <= 0: 2^-16 */
    double max_exposure;          /* <= 0: 2^16 */
    double prev_exposure;         /* <= 0: none (no adaptation) */
    double rate;                  /* <= 0: 1.0 (jump to the target); in (0, 1]: the step in log2 */
} TakeExposureOpts;
int take_hip_auto_exposure(const int64_t *hist, const TakeExposureOpts *opts, double *exposure_out);

/* The fused pass.  Per channel c, in Real, every operation in the order written:
 *   1. x = c * E;   2. if (!(x > 0)) x = 0 (NaN and negatives become 0);   3. x = min(x, 65504);
 *   4. the operator: LINEAR y = x; REINHARD y = x * (1 + x / white^2) / (1 + x); ACES (Narkowicz's rational fit)
 *      y = (x * (2.51 x + 0.03)) / (x * (2.43 x + 0.59) + 0.14);
 *   5. y = min(y, 1);
 *   6. the transfer: SRGB y <= 0.0031308 ? 12.92 y : 1.055 pow(y, 1 / 2.4) - 0.055 (the library's pow / powf); LINEAR none;
 *   7. RGBA: code = (int)(y * 255 + 0.5), the bytes R, G, B, 255 per pixel; REAL: the three y.
 * E (and 1 / white^2) are computed in double and rounded to Real once. */
#define TAKE_TONEMAP_LINEAR 0
#define TAKE_TONEMAP_REINHARD 1
#define TAKE_TONEMAP_ACES 2
#define TAKE_TRANSFER_SRGB 0
#define TAKE_TRANSFER_LINEAR 1
#define TAKE_DISPLAY_RGBA 0 /* uint8 x 4 per pixel */
#define TAKE_DISPLAY_REAL 1 /* 3 Reals per pixel; out may be rgb */
typedef struct TakeTonemapOpts {
    double exposure;            /* > 0: used as given; <= 0: auto (the histogram + take_hip_auto_exposure with `auto_opts`) */
    double white;               /* REINHARD; <= 0: 4.0 */
    int32_t op;                 /* TAKE_TONEMAP_* */
    int32_t transfer;           /* TAKE_TRANSFER_* */
    int32_t format;             /* TAKE_DISPLAY_* */
    int32_t reserved;           /* 0 */
    TakeExposureOpts auto_opts; /* read (and checked) whether or not the exposure is automatic */
} TakeTonemapOpts;
/* d_rgb, d_out: device memory of the current device; d_out: height * width * 4 bytes (RGBA, 4-byte aligned) or height *
 * width * 3 Real (REAL; may be d_rgb itself, no other aliasing).  opts: NULL = ACES, sRGB, RGBA, automatic exposure with
 * the default options.  exposure_used (may be NULL; HOST memory in both calls): the E that was applied.  With an
 * automatic exposure the call is take_hip_luminance_histogram_device + take_hip_auto_exposure + the pass with that E,
 * made by hand.  Enqueued on `stream`, returns after it has completed.
 * TAKE_E_INVALID, checked before a device is looked for: a NULL d_rgb / d_out ("null argument"), width or height <= 0,
 * an unknown precision, an unknown op / transfer / format, reserved != 0, an exposure or white that is not finite, what
 * take_hip_auto_exposure refuses of auto_opts, RGBA output that overlaps the input or is not 4-byte aligned. */
int take_hip_tonemap_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts,
                            void *d_out, double *exposure_used, void *stream);
/* the same with host pointers (upload, the same kernels, download) */
int take_hip_tonemap(const void *rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts, void *out,
                     double *exposure_used);

/* ---- bloom for the display transform, on an image workspace the caller keeps (new symbols of ABI version 5; no struct
 * changed): glare around what exceeds the display range — a bright pass, a pyramid of 13-tap downsamples, bilinear
 * upsamples summed back, the layer added between the exposure and the tone operator.  EXTENSION, parity unpinned with
 * respect to the reference; specified against its own restatement (tests/bloom_ref.py; DESIGN.md par. 4m has the
 * arithmetic and every order of additions).  Scene-free; every output pixel is written by one thread from fixed inputs,
 * no atomics: the same planes give the same bits.  Planes as above.  In Real, every operation in the order written:
 *   1. per channel x = c * E; if (!(x > 0)) x = 0; x = min(x, 65504) — E the exposure the tone-mapping uses, so that
 *      threshold and knee are in exposed units: 1.0 is what the display clips;
 *   2. the bright pass (soft knee): Y = the Rec.709 luminance of x; with t = threshold, k = knee: s = Y - (t - k);
 *      s = min(max(s, 0), 2 k); s = k > 0 ? (s s) / (4 k) : 0; m = max(s, Y - t); w = m > 0 ? m / Y : 0; b = x w;
 *   3. level 0 has ceil(W / 2) x ceil(H / 2) pixels, every further level the ceil-halving of the one before; Lmax = the
 *      number of levels until both axes are 1 (at least 1), at most TAKE_BLOOM_MAX_LEVELS; L = levels > 0 ?
 *      min(levels, Lmax) : Lmax;
 *   4. downsample (the 13-tap filter of Jimenez, "Next Generation Post Processing in Call of Duty", discrete): a
 *      destination pixel reads the 6 x 6 source pixels at rows 2 y - 2 .. 2 y + 3 and columns 2 x - 2 .. 2 x + 3,
 *      clamped to the source; nine 2 x 2 means B on the even grid, four C on the odd grid;
 *      0.125 sum(C) + 0.125 B[1][1] + 0.0625 (the four edge B) + 0.03125 (the four corner B); D_0 of b, D_k of D_k-1;
 *   5. upsample: bilinear x 2, weights 9/16, 3/16, 3/16, 1/16 of the near and far source pixels per axis (even x: near
 *      x / 2, far x / 2 - 1; odd x: near (x - 1) / 2, far near + 1; far clamped); U_L-1 = D_L-1, U_k = D_k + up(U_k+1);
 *   6. layer = gain * up(U_0) at full resolution, gain = (Real)(intensity / L); x' = x + layer; then steps 3 to 7 of the
 *      fused pass above on x'. */
#define TAKE_BLOOM_MAX_LEVELS 8
typedef struct TakeBloomOpts { /* a field < 0 (levels: <= 0) = its default */
    double threshold;          /* < 0: 1.0 */
    double knee;               /* < 0: 0.5; at most the threshold */
    double intensity;          /* < 0: 0.25; 0 is allowed: no bloom */
    int32_t levels;            /* <= 0: all (Lmax) */
    int32_t reserved;          /* 0 */
} TakeBloomOpts;
/* The workspace of the scene-free image-space calls: it owns the histogram's block rows and the bloom pyramid (one
 * device allocation), grows on demand and never shrinks, so that a sequence of frames allocates nothing after its first.
 * Bound to the device that was current when it was created: a call with it on another device is TAKE_E_INVALID.  NOT
 * thread-safe: one call at a time per workspace.  destroy(NULL) is a no-op. */
typedef struct TakeImageWorkspace TakeImageWorkspace;
int take_hip_image_workspace_create(TakeImageWorkspace **out);
void take_hip_image_workspace_destroy(TakeImageWorkspace *ws);
/* The full-resolution layer of step 6, height * width * 3 Real, for an explicit exposure.  d_rgb, d_layer_out: device
 * memory of the current device; d_layer_out may be d_rgb itself.  opts: NULL = the defaults.  ws: NULL = the pyramid is
 * allocated per call and freed on return.  Enqueued on `stream`, returns after it has completed.
 * TAKE_E_INVALID, checked before a device is looked for: a NULL d_rgb / d_layer_out ("null argument"), width or height
 * <= 0, an unknown precision, an exposure that is not > 0 (NaN included), an option that is not finite, knee >
 * threshold, reserved != 0, levels > TAKE_BLOOM_MAX_LEVELS (each after the defaults are filled in), a layer output that
 * partly overlaps the input. */
int take_hip_bloom_layer_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, double exposure,
                                const TakeBloomOpts *opts, void *d_layer_out, TakeImageWorkspace *ws, void *stream);
/* the same with host pointers (upload, the same kernels, download; a temporary workspace) */
int take_hip_bloom_layer(const void *rgb, int32_t precision, int32_t width, int32_t height, double exposure, const TakeBloomOpts *opts,
                         void *layer_out);
/* take_hip_tonemap_device with the composite of step 6: the same options, formats, in-place rule for REAL and overlap
 * rule for RGBA; the automatic exposure is that of the input image's histogram, exactly as there (made in the
 * workspace's rows).  bloom: NULL = the defaults.  ws: NULL = allocate per call and free on return.
 * TAKE_E_INVALID, checked before a device is looked for: everything take_hip_tonemap_device refuses, and of `bloom`
 * what take_hip_bloom_layer_device refuses. */
int take_hip_tonemap_bloom_device(const void *d_rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts,
                                  const TakeBloomOpts *bloom, void *d_out, double *exposure_used, TakeImageWorkspace *ws, void *stream);
/* the same with host pointers (upload, the same kernels, download; a temporary workspace) */
int take_hip_tonemap_bloom(const void *rgb, int32_t precision, int32_t width, int32_t height, const TakeTonemapOpts *opts,
                           const TakeBloomOpts *bloom, void *out, double *exposure_used);

/* rows this rank owns / their image-row indices (rows_out may be NULL) */
int take_hip_render_rows(const TakeScene *scene, int32_t strip_first, int32_t strip_stride,
                         int32_t *rows_out);

/* Kernel-level hooks: n rays in host memory -> n hits in host memory. */
int take_hip_trace_closest(TakeScene *scene, const void *rays, int64_t n, void *hits);
int take_hip_trace_any(TakeScene *scene, const void *rays, int64_t n, int32_t *occluded);
/* Device-resident variants for the traversal-only benchmark: rays/hits are device
 * pointers; `count_mode` != 0 runs the instrumented kernel that fills node_visits /
 * prim_tests (never timed). */
int take_hip_trace_closest_device(TakeScene *scene, const void *d_rays, int64_t n, void *d_hits,
                                  int32_t count_mode, void *stream);

/* ---- path tracing of caller-supplied rays, and the scene's own camera rays (EXTENSION, parity unpinned; new symbols
 * of ABI version 5; no struct changed; DESIGN.md par. 4n).  The trace hooks above take rays from the caller and stop
 * at the first hit; take_hip_render_rays* carries radiance along them: light probes and lightmap texels, a panoramic,
 * orthographic or fisheye camera, a batch of rays in a torch tensor, a reprojected or foveated sample pattern.
 *  - take_hip_render_rays*: n rays = n output texels.  rgb_out: n * 3 Real in ray order (float for F32 scenes, double
 *    for F64 and MIXED ones); texel i is the mean over the opts->spp samples of "the integrator's radiance along that
 *    sample's ray", summed in sample order and then multiplied by 1 / spp, as a render's pixel is.  ray_sets == 1: ray
 *    i serves all spp samples of texel i; ray_sets == spp: sample s of texel i travels along rays[s * n + i].
 *    The random stream of sample s of ray i is the stream a render gives sample first_sample + s of pixel index i
 *    — rng_key(seed, i, first_sample + s) — and the path starts it at counter 2 (CAMERA_DRAWS): counters 0 and 1 are
 *    left to the caller's own jitter.  The stream does not depend on n, ray_sets or samples_per_batch: a ray traced in
 *    a call of its own at the same index i gives the same bits, and spp = 1 calls with first_sample = 0, 1, ... are
 *    the samples of one spp call.
 *    Of a ray record org and dir are used.  tmin and tmax are IGNORED: the first segment starts at the effective
 *    ray_epsilon and is unbounded, as a camera ray's is (the render loop keeps one tmin for all rays of a launch).
 *    Directions must have unit length: the shade rounds take cosines against them.  The host entry refuses a ray with
 *    a non-finite component of org or dir, and — without TAKE_RAYS_NORMALIZE — one with | |dir|^2 - 1 | > 1e-3 (with
 *    the flag: one whose direction has zero or overflowing length); the message names the first such ray.  The device
 *    entry cannot look: it takes the rays as they are, a direction that is not of unit length scales the cosines of
 *    its first vertex (a biased texel, no fault), and a non-finite one gives a texel that is not finite.  With
 *    TAKE_RAYS_NORMALIZE every direction goes through the camera ray's own normalize on the device before use.
 *    All four integrators, max_depth, samples_per_batch and ray_epsilon as take_hip_render takes them, environment
 *    maps too (and the refusal of one for integrators 1..3); strip_first / strip_stride are ignored, and so is the
 *    lens: the rays are the caller's.  F32, F64 and MIXED scenes (a mixed scene makes its records on the f64 side and
 *    hands over as a render does), one- and two-level scenes; not for scene groups.  The call uses the render
 *    workspace, the accumulator included: it ends a progressive sequence as take_hip_render does.
 *    take_hip_get_counters afterwards: samples = n * spp, the rest as after a render.  n == 0 is TAKE_OK and writes
 *    nothing.  The device entry: d_rays and d_rgb_out are device memory, d_rays 16-byte aligned; enqueued on `stream`,
 *    returns after enqueue + sync.
 *    TAKE_E_INVALID, before a device is looked for: a NULL argument ("null argument"; rays and the output may be NULL
 *    when n == 0), spp <= 0, max_depth < -1 or an unknown integrator, n < 0 or n >= 2^30, ray_sets other than 1 or
 *    spp, first_sample < 0 or first_sample + spp beyond int32, unknown flag bits, a non-zero reserved, a device ray
 *    pointer that is not 16-byte aligned; the host entry's look at the rays; then what take_hip_render refuses of the
 *    scene.  A failed call leaves the scene rendering as before.
 *  - take_hip_camera_rays*: the inverse — opts->spp * W * H ray records in that layout (ray_sets == spp, n = W * H),
 *    TakeRayF for F32 scenes and TakeRayD for F64 and MIXED ones (the f64 camera).  Ray index i = y * W + x with
 *    y = 0 the BOTTOM image row: the render loop's pixel index, so that the keys above line up.  Set s holds exactly
 *    the rays a whole-image take_hip_render with the same seed traces for sample first_sample + s: org = lookfrom for
 *    the pinhole camera, the lens ray with a lens (take_hip_scene_set_lens); tmin = the effective ray epsilon and
 *    tmax = +inf, so that the buffer can go straight into the trace hooks — or back into take_hip_render_rays*, whose
 *    image for (these rays, ray_sets = spp, the same seed and first_sample) is take_hip_render's bit for bit, row y of
 *    it being image row H - 1 - y.  Of the options only seed, spp and ray_epsilon are read; strips are ignored.  The
 *    call uses path records only: a progressive sequence goes on after it, as after the feature pass.  Not for scene
 *    groups.  TAKE_E_INVALID, before a device is looked for: a NULL argument, spp <= 0, first_sample < 0 or
 *    first_sample + spp beyond int32, a device pointer that is not 16-byte aligned. */
#define TAKE_RAYS_NORMALIZE 1 /* normalise every direction on the device before use */
typedef struct TakeRayBatch {
    const void *rays;     /* TakeRayF (F32 scenes) or TakeRayD (F64, MIXED): ray_sets * n records */
    int64_t n;            /* rays = output texels */
    int32_t ray_sets;     /* 1: ray i serves all spp samples; == spp: sample s of ray i is rays[s * n + i] */
    int32_t first_sample; /* samples are numbered first_sample .. first_sample + spp - 1 (>= 0) */
    int32_t flags;        /* 0 or TAKE_RAYS_NORMALIZE */
    int32_t reserved;     /* 0 */
} TakeRayBatch;
int take_hip_render_rays_device(TakeScene *scene, const TakeRenderOpts *opts, const TakeRayBatch *batch /* rays: device */, void *d_rgb_out, void *stream);
int take_hip_render_rays(TakeScene *scene, const TakeRenderOpts *opts, const TakeRayBatch *batch /* rays: host */, void *rgb_out_host);
int take_hip_camera_rays_device(TakeScene *scene, const TakeRenderOpts *opts, int32_t first_sample, void *d_rays_out, void *stream);
int take_hip_camera_rays(TakeScene *scene, const TakeRenderOpts *opts, int32_t first_sample, void *rays_out_host);

/* ---- several GPUs from ONE process (the C++ host of the reference is a single process: main.cpp -> render()).
 * Replaces the thread pool of src/parallel.cpp:183-237 for the drop-in: the scene is built once per device
 * (replicated), device k of n renders the 4-row strips s with s % n == k on its own host thread, and the strips are
 * gathered on the first device with hipMemcpyPeerAsync (xGMI between the GPUs of a node) — the only exchange.  The
 * image is identical for every n (pixel keys do not depend on the sharding).  `devices` lists the HIP devices to use
 * (NULL: 0 .. n_gpus-1); a device may appear more than once (logical shards of one GPU: how the sharding is tested
 * on a one-GPU box).  (A multi-process job — one process per GPU, RCCL gather — uses plain scene handles with
 * strip_first / strip_stride instead: take_amd/dist.py, bench.py.)                                               */
typedef struct TakeSceneGroup TakeSceneGroup; /* opaque */
int take_hip_group_create(const TakeSceneDesc *desc, const TakeBuildOpts *opts, int32_t n_gpus, const int32_t *devices,
                          TakeSceneGroup **out);
int take_hip_group_destroy(TakeSceneGroup *group);
/* Whole image (height * width * 3 Real, row 0 = top) into host memory / into memory of the group's first device.
 * opts->strip_first / strip_stride are ignored (the group shards by itself). */
int take_hip_group_render(TakeSceneGroup *group, const TakeRenderOpts *opts, void *rgb_out_host);
int take_hip_group_render_device(TakeSceneGroup *group, const TakeRenderOpts *opts, void *d_rgb_out);
int take_hip_group_size(const TakeSceneGroup *group);
/* counters of shard k's last render (ms_total etc. per device: load balance) */
int take_hip_group_get_counters(const TakeSceneGroup *group, int32_t k, TakeCounters *out);

int take_hip_get_counters(const TakeScene *scene, TakeCounters *out);
/* enable per-kernel HIP-event timing + counting mode for subsequent renders
 * (bit 0 = event timing, bit 1 = visit counters; both off by default) */
int take_hip_set_instrumentation(TakeScene *scene, int32_t flags);

/* Test hook: run the device shading functions on the rows of one of the reference's golden tables
 * (tests/golden/tables, column layouts of oracle/ref_harness.cpp).  kind: 0 material (27 -> 14 columns),
 * 1 light (30 -> 9), 2 texture (6 -> 3), 3 to_world (6 -> 3), 4 hemisphere_cos (1 -> 4).  `rnd` holds 8 doubles
 * per row: the first random_real() draws of the mt19937 stream the reference used for that row. */
int take_hip_debug_table(int32_t kind, int32_t precision, const double *in, int64_t n, int32_t in_cols,
                         const double *rnd, double *out, int32_t out_cols);

/* Test hook: the environment-map functions of the shade kernel on the rows of `in`, against the tables and guide
 * tables resident in `scene` (what its renders read).  side: TAKE_PRECISION_F32 / _F64 — which resident side (a MIXED
 * scene has both).  kind 0: in = (u1, u2) per row, the two uniform draws of one light sample -> out = 8 columns:
 * dir[3], radiance[3], pdf (solid angle), y * width + x of the texel the CDF searches found.  kind 1: in = dir[3] per
 * row -> out = 5 columns: radiance[3], pdf, y * width + x of the texel the direction falls into.  f32 sides round the
 * inputs to float.  TAKE_E_INVALID: a side the scene does not have, a scene without a map, NULL arguments. */
int take_hip_debug_env(TakeScene *scene, int32_t side, int32_t kind, const double *in, int64_t n, double *out);

/* Test hook (new symbols of ABI version 5; no struct changed): the acceleration structure of one resident side of a
 * scene, copied from device memory as the trace kernels read it — whoever built it, and after every
 * take_hip_scene_set_instance_transforms.  side: TAKE_PRECISION_F32 / _F64 (a MIXED scene has both).
 * take_hip_debug_tree_info says what there is; take_hip_debug_tree copies n_nodes * node_bytes bytes of nodes,
 * n_prims * prim_bytes bytes of primitive records (leaf order; in a two-level scene the shapes' first, then each
 * prototype's) and n_instances * inst_bytes bytes of placement records into host buffers the caller sized from the
 * info (inst_trace may be NULL for a scene without placements).  The layouts are those of take_amd/csrc/tk_scene.h:
 * node_format 0 = full-width 4-wide nodes of the side's Real (four slots of bmin[3], bmax[3], child word, pad),
 * 1 = 64-byte compressed 4-wide nodes, 2 = 128-byte compressed 8-wide nodes (slots of q[3] = lo | hi << 16, child word);
 * the records are PrimRec<Real> and InstTrace<Real>.  grid_lo / grid_step: the grid of the top-level tree's compressed
 * nodes (a prototype's own grid is in its placements' records).
 * TAKE_E_INVALID: NULL arguments ("null argument", before a device is looked for), a side the scene does not have. */
typedef struct TakeDebugTreeInfo {
    int32_t node_format; /* 0 full width, 1 compressed 4-wide, 2 compressed 8-wide */
    int32_t node_width;  /* slots per node: 4 or 8 */
    int32_t two_level;   /* 1: the scene has placements (instance words, prototype trees behind the top-level tree) */
    int32_t root_child;  /* child word of the root */
    int32_t real_bytes;  /* 4 or 8: the side's Real */
    int32_t node_bytes, prim_bytes, inst_bytes; /* element sizes */
    int64_t n_nodes, n_prims, n_instances;
    float grid_lo[3], grid_step[3];
} TakeDebugTreeInfo;
int take_hip_debug_tree_info(const TakeScene *scene, int32_t side, TakeDebugTreeInfo *info);
int take_hip_debug_tree(const TakeScene *scene, int32_t side, void *nodes, void *prims, void *inst_trace);

/* Test hook (new symbols of ABI version 5; no struct changed): the environment map of one resident side of a scene as
 * the shade kernels read it — the EnvMap record (take_amd/csrc/tk_scene.h), its tables, its texels and the scene's
 * whole image table, copied from device memory — after creation and after every take_hip_scene_set_envmap.
 * take_hip_debug_env_tables_info says what there is; take_hip_debug_env_tables copies height + 1 Reals of marginal,
 * height * (width + 1) of conditional, n_guide_m + 1 int32 of guide_m, height * (n_guide_c + 1) of guide_c,
 * 3 * width * height Reals of texels and n_images records of {int32 width, height; int64 offset} into host buffers the
 * caller sized from the info.
 * TAKE_E_INVALID: NULL arguments ("null argument", before a device is looked for), a side the scene does not have, a
 * scene without an environment map ("no environment map"). */
typedef struct TakeDebugEnvTablesInfo {
    int32_t width, height;
    int32_t n_guide_m, n_guide_c;
    int32_t real_bytes;  /* 4 or 8: the side's Real */
    int32_t n_images;
    int64_t texel0;      /* first texel of the map in the side's texel array */
    double scale[3];     /* EnvMap::scale and the light record's intensity, widened */
    double intensity[3];
} TakeDebugEnvTablesInfo;
int take_hip_debug_env_tables_info(const TakeScene *scene, int32_t side, TakeDebugEnvTablesInfo *info);
int take_hip_debug_env_tables(const TakeScene *scene, int32_t side, void *marginal, void *conditional, int32_t *guide_m, int32_t *guide_c, void *texels,
                              void *images);

/* Test hook (new symbols of ABI version 5; no struct changed): the shading tables of one resident side of a scene as
 * the kernels read them, copied from device memory — after creation and after every take_hip_scene_set_materials /
 * _set_light_intensities: n_materials MaterialRec, n_lights LightRec, n_pmf Reals of light_pmf, n_cdf of light_cdf and
 * n_instances InstShade (two-level scenes; take_amd/csrc/tk_scene.h has the layouts), into host buffers the caller
 * sized from the info — every pointer non-NULL, also where the count is 0.  The info also says what the HOST holds of
 * the material tags: tag_mask, n_material_tags, single_tag.  (Primitive records: take_hip_debug_tree.)
 * TAKE_E_INVALID: NULL arguments ("null argument", before a device is looked for), a side the scene does not have. */
typedef struct TakeDebugShadingTablesInfo {
    int32_t n_materials, n_lights;
    int64_t n_instances;
    int32_t real_bytes;  /* 4 or 8: the side's Real */
    int32_t material_bytes, light_bytes, inst_shade_bytes; /* element sizes */
    int32_t n_pmf, n_cdf;
    uint32_t tag_mask;
    int32_t n_material_tags, single_tag, reserved;
} TakeDebugShadingTablesInfo;
int take_hip_debug_shading_tables_info(const TakeScene *scene, int32_t side, TakeDebugShadingTablesInfo *info);
int take_hip_debug_shading_tables(const TakeScene *scene, int32_t side, void *materials, void *lights, void *light_pmf, void *light_cdf, void *inst_shade);

/* ---- PLY -> device mesh arrays ------------------------------------------------------------
 * Replaces src/parse/parse_ply.cpp:9-123 (`TriangleMesh parse_ply(filename, to_world)`) for binary_little_endian
 * files: the host reads only the text header, the binary body goes to HBM as it lies in the file and kernels do what
 * the reference's host loops do — widen x/y/z, nx/ny/nz, u/v to double, xform_point(to_world) on positions
 * (src/transform.cpp:79-87), xform_normal(inverse(to_world)) on normals (src/transform.cpp:95-100), narrow the face
 * list to int triples.  The arrays are bit-identical to the reference's `TriangleMesh` members.
 * `to_world` / `inv_to_world`: the reference's Matrix4x4, row-major (m[4*i+j] = M(i,j)); NULL = identity.  The caller
 * passes the inverse it already has (`inverse(to_world)`, src/matrix.h:81) — only meshes with normals read it.
 * On success `*out` describes a mesh whose arrays are DEVICE memory owned by the library (flags =
 * TAKE_MESH_DEVICE_ARRAYS): put it into a TakeSceneDesc like any other mesh, and give it back with
 * take_hip_mesh_release once every scene_create that uses it has returned.
 * Not decodable here (TAKE_E_INVALID, message starts with "unsupported"): ascii / big-endian files, list properties in
 * the vertex element or ahead of the mesh data — the caller keeps its host parser for those.  Faces that are not
 * triangles or index past the vertex array are TAKE_E_INVALID (the reference reads three indices per face
 * unconditionally, parse_ply.cpp:85-120). */
typedef struct TakePlyLayout {
    int64_t n_vertices, n_faces;
    int64_t vertex_offset, face_offset; /* bytes from the start of the file */
    int32_t vertex_stride, face_stride; /* bytes per row (faces: with three indices) */
    int32_t has_normals, has_uvs;
    int32_t position_is_f64, index_bytes;
    int32_t header_bytes, reserved;
} TakePlyLayout;
/* header only; needs no GPU */
int take_hip_ply_layout(const void *file_bytes, size_t n_bytes, TakePlyLayout *out);
int take_hip_mesh_from_ply(const void *file_bytes, size_t n_bytes, const double *to_world, const double *inv_to_world,
                           int32_t material_id, TakeMesh *out);
/* the same on a file (memory-mapped, so the body is read once, by the copy to the device) */
int take_hip_mesh_from_ply_file(const char *path, const double *to_world, const double *inv_to_world,
                                int32_t material_id, TakeMesh *out);
/* Mitsuba's serialized mesh format — replaces `TriangleMesh parse_serialized(filename, shape_index, to_world)`
 * (src/parse/parse_serialized.cpp:174-256).  The zlib stream is inflated on the host (a serial job) in ONE pass into one
 * buffer — the reference pulls it through ZStream::read three scalars per vertex — and the blocks (positions, normals,
 * uvs, [colours: skipped], index triples; float or double by EDoublePrecision) are decoded on the device by the kernels
 * of the PLY path, with the same transforms.  Versions 3 and 4, any sub-mesh (`shape_index`, offset table at the end of
 * the file: skip_to_idx, :117-133).  Arrays bit-identical to the reference's. */
int take_hip_mesh_from_serialized(const void *file_bytes, size_t n_bytes, int32_t shape_index, const double *to_world,
                                  const double *inv_to_world, int32_t material_id, TakeMesh *out);
int take_hip_mesh_from_serialized_file(const char *path, int32_t shape_index, const double *to_world,
                                       const double *inv_to_world, int32_t material_id, TakeMesh *out);
/* Wavefront OBJ -> device mesh arrays: the reference's parse_obj (src/parse/parse_obj.cpp:118-203), to_world applied as
 * parse_obj's get_vertex_id applies it (xform_point; normals through xform_normal(inv_to_world)).  The whole file is
 * decoded on the device; the arrays are bit-identical to the reference's TriangleMesh.  Scope: `v x y z [w]` (w
 * divides), `vt s t` (stored as (s, 1 - t)), `vn x y z` (normalized), `f` with 3 or 4 corners `v`, `v/vt`, `v//vn`,
 * `v/vt/vn` (a quad is (v0, v1, v2), (v0, v2, v3)); every other line is ignored.  Vertices are deduplicated on the raw
 * index triple in order of first use; a negative index is relative to its pool at the face's line (vt: pool + vt - 1,
 * as the reference resolves it).  uvs / normals are NULL when no vertex has a vt / vn.
 * TAKE_E_INVALID: a face with more than 4 corners (the reference's n-gon error) or fewer than 3, a vertex index 0, an
 * index outside its pool at its line.  TAKE_E_INVALID with a message that starts with "unsupported": a token the
 * reference's std::stoi would throw on, a number missing or outside [+-]?(d+(.d*)?|.d+)([eE][+-]?d+)?, a number out of
 * the range of a double, or only some vertices with a vt (vn) — the caller keeps its host parser for those. */
int take_hip_mesh_from_obj(const void *file_bytes, size_t n_bytes, const double *to_world, const double *inv_to_world,
                           int32_t material_id, TakeMesh *out);
int take_hip_mesh_from_obj_file(const char *path, const double *to_world, const double *inv_to_world, int32_t material_id,
                                TakeMesh *out);
/* compute_normals (src/compute_normals.cpp:12-47): Nelson Max angle-weighted vertex normals, what parse_scene
 * puts into a mesh loaded without normals unless the shape sets faceNormals. Device-array mesh
 * (TAKE_MESH_DEVICE_ARRAYS) whose normals are NULL: on success mesh->normals is a library-owned device array
 * (freed by take_hip_mesh_release). A mesh that already has normals, or host arrays: TAKE_E_INVALID.
 * The sums run in the reference's order (a stable sort, no atomics): the result is deterministic, and differs from
 * the reference's only where the device asin differs from the C library's in the last bit.  An index outside
 * [0, n_vertices), or more than INT32_MAX corners: TAKE_E_INVALID. */
int take_hip_mesh_compute_normals(TakeMesh *mesh);
/* the same on host arrays (upload, the same kernels, download): normals_out = n_vertices * 3 doubles */
int take_hip_compute_normals(const double *positions, int64_t n_vertices, const int32_t *indices, int64_t n_faces,
                             double *normals_out);
/* copy a device-array mesh to host arrays the caller sized from n_vertices / n_faces (NULL = skip that array) */
int take_hip_mesh_download(const TakeMesh *mesh, double *positions, int32_t *indices, double *normals, double *uvs);
int take_hip_mesh_release(TakeMesh *mesh);

/* BVH introspection (tests / DESIGN figures): node count, primitive count, depth */
int take_hip_scene_stats(const TakeScene *scene, int64_t *n_nodes, int64_t *n_prims,
                         int32_t *depth, int64_t *device_bytes);
/* Who built the scene's trees, per side: TAKE_BUILDER_DEVICE_LBVH, TAKE_BUILDER_HOST_SAH (asked for, chosen by AUTO,
 * or the fall-back of a device build: fewer than 8 primitives, a Morton-order tree deeper than the traversal stack —
 * both levels of a two-level scene counted —, a prototype of a single leaf, or a two-level scene under TAKE_HIP_BRAID > 1
 * or TAKE_HIP_NODES=q8), or -1 for a side the scene does not have (f32_builder of an F64 scene, f64_builder of an F32 one; a MIXED
 * scene has both).  Either pointer may be NULL. */
int take_hip_scene_build_info(const TakeScene *scene, int32_t *f32_builder, int32_t *f64_builder);

#ifdef __cplusplus
}
#endif
#endif /* TAKE_HIP_H */

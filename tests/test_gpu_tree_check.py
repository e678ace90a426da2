"""The structural validator (tests/tree_check.py) on the trees the DEVICE builder leaves in device memory, read back
through take_hip_debug_tree (capi.Scene.debug_tree) — nodes, records and placement records as the trace kernels read
them.  No rays, no renders: every child box against the exact extents of the primitives below it, every node reached
once, every record in one leaf, the placements' boxes against the images of their prototypes' records, and the
records themselves against the host builder's (tests/hostsim), byte for byte.  Each case first asserts who built the
scene: a silent fall-back to the host builder fails where a device tree is expected.
The diagnostics (smallest margin between a box and its contents, surface-area inflation) are printed, not judged;
tests/test_tree_check_cpu.py holds the controls that prove the validator bites."""
import os

import numpy as np
import pytest

import tree_check as T
from helpers import golden_scene, hostsim_debug_tree, random_linear, sheared_placements
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import SceneData

pytestmark = pytest.mark.gpu
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
NAMES = {F32: "f32", F64: "f64", MIXED: "mixed"}
OFFSET = np.array([1000.3, -2000.7, 500.1])  # tests/test_gpu_device_build_f64.py::test_far_from_the_origin's


def sides_of(precision):
    return {F32: [F32], F64: [F64], MIXED: [F64, F32]}[precision]


def built_by(precision, builder):
    return {"f32": -1 if precision == F64 else builder, "f64": -1 if precision == F32 else builder}


def create(sd, precision, fmt, leaf, builder=DEV):
    """a scene built under TAKE_HIP_NODES=fmt ("" = unset: compressed unless the grid is too coarse); the variable is put back"""
    old = os.environ.get("TAKE_HIP_NODES")
    try:
        os.environ.pop("TAKE_HIP_NODES", None)
        if fmt:
            os.environ["TAKE_HIP_NODES"] = fmt
        return capi.Scene(sd, precision=precision, builder=builder, max_leaf_size=leaf)
    finally:
        os.environ.pop("TAKE_HIP_NODES", None)
        if old is not None:
            os.environ["TAKE_HIP_NODES"] = old


def validate(sc, sd, precision, leaf, tag, xforms=None, want_format=None):
    """every resident side of `sc`: all error counts 0, the depth the scene reports, the host builder's records"""
    if xforms is None and sd.instance_mesh:
        xforms = np.array(sd.instance_xform)
    # (leaf sizes: the top-level tree of a two-level scene has one entry per leaf whatever the request)
    for side in sides_of(precision):
        tree = sc.debug_tree(side)
        if want_format is not None:
            assert tree["node_format"] == want_format, tree["node_format"]
        primary = side == sides_of(precision)[0]  # take_hip_scene_stats reports the primary side
        r = T.check_tree(tree, max(1, leaf), n_shapes=sd.n_shapes, xforms=xforms, expected_depth=sc.stats()["depth"] if primary else None)
        d = r["diag"]
        print(f"\n[tree] {tag} {NAMES[precision]}/{'f64' if side == F64 else 'f32'} leaf {leaf} format {tree['node_format']}: "
              f"{tree['n_nodes']} nodes, {tree['n_prims']} records, depth {d['depth']}, min margin lo {d['min_margin_lo']:.3g} "
              f"hi {d['min_margin_hi']:.3g} {d['margin_unit']}, inflation {d['inflation']:.6f}"
              + (f", placement margin {d['min_placement_margin_rel']:.3g} of the magnitude" if "min_placement_margin_rel" in d else ""))
        assert T.total_errors(r) == 0, (r["errors"], r["where"])
        host = hostsim_debug_tree(sd, 1 if side == F64 else 0, leaf)
        assert T.record_mismatches(tree, host, sd.n_shapes) == 0
    return tree


def triangles(n, seed=3):
    sd = SceneData(width=16, height=16, lookfrom=(0.0, 0.0, 3.9), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=39.0,
                   background=(0.1, 0.1, 0.1), spp=1, max_depth=2)
    sd.add_mesh(*scenes.soup_triangles(n, seed, 0.9, 0.05), sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7)))
    return sd


# ------------------------------------------------------------------ 1. primitive counts around the wave and block edges
COUNTS = [8, 9, 63, 64, 65, 255, 256, 257, 1000, 4097]
LEAVES = [1, 2, 4]
PRECISIONS = [F32, F64, MIXED]
FORMATS = ["", "wide"]
# every (n, leaf) pair once — 30 cases instead of 180 —, the side and the node format rotated so that every pair of
# values of any two axes occurs (checked below); n is no multiple of the leaf size for 15 of the 20 cases with leaves
# of 2 and 4 (a short last leaf), the even counts keep their full leaves
COUNT_CASES = [(n, leaf, PRECISIONS[(ni + li) % 3], FORMATS[(3 * ni + li) % 2])
               for ni, n in enumerate(COUNTS) for li, leaf in enumerate(LEAVES)]


def test_the_count_cases_cover_every_pair_of_values():
    axes = [COUNTS, LEAVES, PRECISIONS, FORMATS]
    for a in range(4):
        for b in range(a + 1, 4):
            seen = {(c[a], c[b]) for c in COUNT_CASES}
            assert len(seen) == len(axes[a]) * len(axes[b]), (a, b)


@pytest.mark.parametrize("n,leaf,precision,fmt", COUNT_CASES)
def test_primitive_counts(n, leaf, precision, fmt):
    sd = triangles(n)
    sc = create(sd, precision, fmt, leaf)
    try:
        assert sc.build_info() == built_by(precision, DEV), sc.build_info()
        validate(sc, sd, precision, leaf, f"{n} triangles", want_format=0 if fmt == "wide" else None)
    finally:
        sc.close()


# ------------------------------------------------------------------ 2. many CUs, many collapse blocks
@pytest.mark.parametrize("precision", [F32, F64])
def test_soup_100k(precision):
    """k_refit's fence between CUs and k_collapse's slot allocation across blocks: 100 000 leaves, 391 blocks"""
    sd = scenes.soup_scene(100_000, 32, 32, 1)
    sc = create(sd, precision, "", 1)
    try:
        assert sc.build_info() == built_by(precision, DEV)
        validate(sc, sd, precision, 1, "soup100k")
    finally:
        sc.close()


# ------------------------------------------------------------------ 3. degenerate extents
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("precision", [F32, F64])
def test_all_triangles_in_one_plane(precision, fmt):
    """z = 0 everywhere: the ext == 0 branch of k_morton, the flat-axis branch of make_qgrid"""
    sd = triangles(1000)
    sd.meshes[0].positions[:, 2] = 0.0
    sc = create(sd, precision, fmt, 2)
    try:
        assert sc.build_info() == built_by(precision, DEV)
        validate(sc, sd, precision, 2, "flat z = 0")
    finally:
        sc.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_coincident_triangles(precision):
    """5000 identical triangles — one Morton code, prefix_len's tie-break on the index — next to a small soup: the
    tree of whichever builder build_info reports"""
    sd = scenes.soup_scene(64, 16, 16, spp=1)
    tri = np.array([[0.1, 0.1, 0.0], [0.3, 0.1, 0.0], [0.2, 0.3, 0.0]])
    sd.add_mesh(np.tile(tri, (5000, 1)), np.arange(15000, dtype=np.int32).reshape(-1, 3), 0)
    sc = create(sd, precision, "", 1)
    try:
        who = sc.build_info()["f64" if precision == F64 else "f32"]
        assert who in (DEV, HOST)
        validate(sc, sd, precision, 1, f"5000 coincident triangles (built by {'the device' if who == DEV else 'the host'})")
    finally:
        sc.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["mats", "spherelight"])
def test_spheres_among_triangles(name, precision, fmt):
    sd = golden_scene(name)
    assert len(sd.spheres) > 0 and sd.n_shapes >= 8
    sc = create(sd, precision, fmt, 2)
    try:
        assert sc.build_info() == built_by(precision, DEV)
        validate(sc, sd, precision, 2, name)
    finally:
        sc.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_f64_geometry_far_from_the_origin(fmt):
    """the d2f_down / d2f_up case: |x| ~ 2000, where floats are 1.2e-4 apart, an extent-1e-3 soup whose vertices are no
    floats (the generator of tests/test_gpu_device_build_f64.py::test_far_from_the_origin) — every box plane is rounded"""
    from test_gpu_device_build_f64 import far_scene

    sd, pos = far_scene(1e-3, 2_000, 0.5)
    assert (pos.astype(np.float32).astype(np.float64) != pos).all()
    sc = create(sd, F64, fmt, 1)
    try:
        assert sc.build_info() == built_by(F64, DEV)
        validate(sc, sd, F64, 1, "far from the origin")
    finally:
        sc.close()


# ------------------------------------------------------------------ 4. two-level scenes
def two_prototypes():
    """about 12 placements of 300-face prototypes, two distinct ones, next to the box of instanced_scene"""
    sd = scenes.instanced_scene(6, 300, 16, 16, 1)
    rng = np.random.default_rng(5)
    second = sd.add_prototype(*scenes.soup_triangles(300, 77, 0.1, 0.03), 0)
    for lin in random_linear(rng, 6):
        sd.add_instance(second, np.concatenate([0.5 * lin, rng.uniform(-0.7, 0.7, (3, 1))], axis=1))
    return sd


def far_placements():
    from test_gpu_device_build_instanced import everything_scene

    return everything_scene(OFFSET, res=16)


TWO_LEVEL = {"two_prototypes": two_prototypes, "sheared": sheared_placements, "far": far_placements}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(TWO_LEVEL))
def test_two_level_scenes(name, precision, fmt):
    """k_make_proto_prims, k_placement_boxes, k_placement_pad, k_top_leaves, k_permute_top, k_rebase"""
    sd = TWO_LEVEL[name]()
    sc = create(sd, precision, fmt, 2)
    try:
        assert sc.build_info() == built_by(precision, DEV)
        validate(sc, sd, precision, 2, name)
    finally:
        sc.close()


def new_transforms(sd, seed):
    rng = np.random.default_rng(seed)
    n = len(sd.instance_mesh)
    return np.stack([np.concatenate([0.6 * lin, rng.uniform(-0.9, 0.9, (3, 1))], axis=1) for lin in random_linear(rng, n, shear=0.8)])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("builder", [DEV, HOST])
def test_re_posed_placements(builder, precision, fmt):
    """take_hip_scene_set_instance_transforms with fresh sheared transforms, validated against THOSE transforms:
    k_placement_boxes_resident, k_widen_tight, k_shift_roots.  A scene the host SAH built gets an LBVH top level on its
    first update; its prototypes' trees stay the host's."""
    sd = two_prototypes()
    sc = create(sd, precision, fmt, 2, builder)
    try:
        assert sc.build_info() == built_by(precision, builder)
        for seed in (1, 2):
            x = new_transforms(sd, seed)
            sc.set_instance_transforms(x)
            validate(sc, sd, precision, 2, f"re-posed ({'device' if builder == DEV else 'host'}-built)", xforms=x)
    finally:
        sc.close()

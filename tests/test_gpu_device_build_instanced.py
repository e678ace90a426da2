"""Two-level (instanced) scenes built on the device (TAKE_BUILDER_DEVICE_LBVH: k_make_proto_prims, k_placement_boxes,
k_placement_pad, the top-level tree with instance words, k_rebase — take_amd/csrc/tk_build_gpu.h, tk_build.hip) against
the host SAH build of the same scene and against the flattened geometry.  The trees differ and the RESULTS must not:
box tests are conservative and ties are broken on values, so every DEV-against-HOST comparison is np.array_equal; the
comparisons with the flattened scene use the bars of tests/test_instancing.py."""
import copy
import os
import time

import numpy as np
import pytest

from helpers import random_linear, random_rays, rays_to_abi, rmse, sheared_placements
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import SceneData
from test_instancing import sheared_with_normals, small

pytestmark = pytest.mark.gpu
DEV, HOST, AUTO = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH, D.TAKE_BUILDER_AUTO
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
ALL_EXACT = 60  # more exact bounces than a depth-50 path has rounds
OFFSET = np.array([1000.3, -2000.7, 500.1])  # tests/test_gpu_device_build_f64.py::test_far_from_the_origin's


def built_by(precision, builder):
    return {"f32": -1 if precision == F64 else builder, "f64": -1 if precision == F32 else builder}


def abi(rays8, precision):
    if precision == F32:
        rays8 = rays8.astype(np.float32).astype(np.float64)
    return rays_to_abi(rays8, 0 if precision == F32 else 1)


def same_hits(a, b, rays):
    ha, hb = a.trace_closest(rays), b.trace_closest(rays)
    for f in ("shape_id", "t", "u", "v"):
        assert np.array_equal(ha[f], hb[f]), f
    assert np.array_equal(a.trace_any(rays), b.trace_any(rays))
    return hb


def render(sc, exact_bounces=0, **kw):
    sc.exact_bounces = exact_bounces
    return sc.render(**kw)


def scene_with_node_format(fmt, sd, **kw):
    """a scene built under TAKE_HIP_NODES=fmt (read once, when the scene is built); the variable is put back"""
    old = os.environ.get("TAKE_HIP_NODES")
    try:
        os.environ["TAKE_HIP_NODES"] = fmt
        return capi.Scene(sd, **kw)
    finally:
        if old is None:
            os.environ.pop("TAKE_HIP_NODES", None)
        else:
            os.environ["TAKE_HIP_NODES"] = old


def pair(sd, precision, want=DEV, **kw):
    """(host-built, device-built) scenes; the device one must be built by `want` on every side it has"""
    a = capi.Scene(sd, precision=precision, builder=HOST, **kw)
    b = capi.Scene(sd, precision=precision, builder=DEV, **kw)
    assert a.build_info() == built_by(precision, HOST), a.build_info()
    assert b.build_info() == built_by(precision, want), b.build_info()
    return a, b


def same_scene(sd, precision, rays8, want=DEV, spp=4, max_depth=6, min_hits=0.02):
    """DEV against HOST_SAH: hit tables, occlusion, images (mixed: default and all-exact bounces), primitive count"""
    a, b = pair(sd, precision, want)
    try:
        assert a.stats()["n_prims"] == b.stats()["n_prims"]
        if precision != MIXED:
            hits = same_hits(a, b, abi(rays8, precision))
            assert (hits["shape_id"] >= 0).mean() > min_hits
        for eb in ((0, ALL_EXACT) if precision == MIXED else (0,)):
            ia, ib = render(a, eb, spp=spp, max_depth=max_depth, seed=5), render(b, eb, spp=spp, max_depth=max_depth, seed=5)
            assert np.array_equal(ia, ib), eb
            assert np.isfinite(ia).all() and ia.mean() > 0
    finally:
        a.close(), b.close()


def bent_grid(n=3):
    """an n x n grid of quads (2 n^2 faces) in the plane y = 0 with bent vertex normals and uvs"""
    g = np.linspace(-0.5, 0.5, n + 1)
    x, z = np.meshgrid(g, g, indexing="ij")
    pos = np.stack([x.ravel(), 0.05 * np.sin(7 * x.ravel() + 3 * z.ravel()), z.ravel()], -1)
    nrm = np.stack([0.3 * np.cos(5 * x.ravel()), np.ones(x.size), 0.2 * np.sin(4 * z.ravel())], -1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    uv = np.stack([x.ravel() + 0.5, z.ravel() + 0.5], -1)
    idx = []
    for i in range(n):
        for j in range(n):
            v = i * (n + 1) + j
            idx += [[v, v + n + 2, v + 1], [v, v + n + 1, v + n + 2]]
    return pos, np.array(idx, np.int32), nrm, uv


def sheared_grid():
    """sheared_with_normals() with a prototype of 18 faces instead of 2 (that scene has 6 primitives: below the device
    builder's minimum of 8): vertex normals and uvs on the prototype, scale + shear, one placement with its own material"""
    sd = SceneData(width=40, height=40, lookfrom=(0.0, 1.2, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0,
                   background=(0.2, 0.3, 0.4), spp=4, max_depth=4)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7))
    gold = sd.add_material(D.MAT_BLINN_PHONG_MICROFACET, (0.8, 0.7, 0.3), (30.0,))
    pos, idx, nrm, uv = bent_grid()
    proto = sd.add_prototype(pos, idx, grey, normals=nrm, uvs=uv)
    sd.add_instance(proto, [[1.5, 0.3, 0.0, -0.4], [0.0, 1.0, 0.2, 0.0], [0.1, 0.0, 0.8, 0.2]])
    sd.add_instance(proto, [[0.6, 0.0, 0.0, 0.6], [0.2, 0.7, 0.0, 0.3], [0.0, 0.0, 1.1, -0.3]], gold)
    lp, li, ln, lu = scenes._quad((0, 1.5, 0), (0.4, 0, 0), (0, 0, 0.4), (0, -1, 0))
    sd.add_mesh(lp, li, grey, normals=ln, uvs=lu, emission=(12.0, 12.0, 12.0))
    return sd


def everything_scene(offset=(0.0, 0.0, 0.0), res=64):
    """ordinary meshes, spheres, an area light and placements in one scene: three prototypes — one of them ALSO an
    ordinary mesh of the shape arrays —, material overrides and -1, and one prototype placed twice under the SAME
    transform (every ray into it ties in (t, u, v) between two placements: the larger instance id wins, in every tree)"""
    off = np.asarray(offset, np.float64)
    sd = SceneData(width=res, height=res, lookfrom=tuple(off + (0.0, 0.0, 3.9)), lookat=tuple(off), up=(0.0, 1.0, 0.0),
                   vfov=39.0, background=(0.05, 0.06, 0.08), spp=4, max_depth=6)
    white = sd.add_material(D.MAT_DIFFUSE, (0.73, 0.73, 0.73))
    red = sd.add_material(D.MAT_DIFFUSE, (0.65, 0.05, 0.05))
    blue = sd.add_material(D.MAT_PLASTIC, (0.2, 0.3, 0.8), (1.5,))
    gold = sd.add_material(D.MAT_BLINN_PHONG_MICROFACET, (0.8, 0.7, 0.3), (50.0,))
    fp, fi, fn, fu = scenes._quad(tuple(off + (0, -1, 0)), (1.2, 0, 0), (0, 0, -1.2), (0, 1, 0))
    sd.add_mesh(fp, fi, white, normals=fn, uvs=fu)
    lp, li, ln, lu = scenes._quad(tuple(off + (0, 1.4, 0)), (0.4, 0, 0), (0, 0, 0.4), (0, -1, 0))
    sd.add_mesh(lp, li, white, normals=ln, uvs=lu, emission=(15.0, 15.0, 15.0))
    sd.add_sphere(tuple(off + (-0.7, -0.7, 0.3)), 0.3, blue)
    sd.add_sphere(tuple(off + (0.75, -0.75, -0.2)), 0.25, gold)
    rng = np.random.default_rng(31)
    cloud, cidx = scenes.soup_triangles(400, 77, 0.12, 0.03)
    both = sd.add_mesh(cloud + off + (0.0, -0.6, 0.5), cidx, red)  # an ordinary mesh of 400 shapes ... and a prototype
    protos = [sd.add_prototype(cloud, cidx, white),
              sd.add_prototype(*bent_grid(4)[:2], gold, normals=bent_grid(4)[2], uvs=bent_grid(4)[3]),
              both]
    lin = random_linear(rng, 30)
    for k in range(30):
        p = protos[k % 3]
        scale = 1.0 if p != protos[1] else 0.35
        t = rng.uniform(-0.8, 0.8, 3) + (off if p != both else rng.uniform(-0.2, 0.2, 3))
        x = np.concatenate([scale * (lin[k] if k % 2 else np.eye(3) * rng.uniform(0.5, 1.5)), t[:, None]], axis=1)
        sd.add_instance(p, x, (-1, blue, gold)[k % 3] if k % 5 else -1)
    twice = np.concatenate([2.0 * lin[3], (off + (0.1, 0.2, 0.9))[:, None]], axis=1)
    sd.add_instance(protos[0], twice, red)
    sd.add_instance(protos[0], twice, blue)
    return sd


def scene_rays(n, seed, offset=(0.0, 0.0, 0.0), tmin=1e-4):
    r = random_rays(n, seed, tmin=tmin)
    r[:, 0:3] += np.asarray(offset)
    return r


# ------------------------------------------------------------------ 1. honoured
def test_the_device_builder_is_honoured_on_two_level_scenes():
    sd = small(20, 100, 16)
    assert sd.n_shapes + 100 + 20 >= 8
    for precision in (F32, F64, MIXED):
        for builder, want in ((DEV, DEV), (HOST, HOST), (AUTO, HOST)):  # (AUTO: far below its threshold)
            sc = capi.Scene(sd, precision=precision, builder=builder)
            try:
                assert sc.build_info() == built_by(precision, want), (precision, builder, sc.build_info())
            finally:
                sc.close()


# ------------------------------------------------------------------ 2. the same scene as the host build's
@pytest.mark.parametrize("precision", [F32, F64, MIXED])
@pytest.mark.parametrize("name", ["small", "sheared_with_normals", "sheared_grid", "everything"])
def test_results_do_not_depend_on_the_builder(name, precision):
    sd = {"small": lambda: small(60, 300, 64), "sheared_with_normals": sheared_with_normals, "sheared_grid": sheared_grid,
          "everything": everything_scene}[name]()
    # sheared_with_normals() is 2 + 2 + 2 primitives: the documented minimum of the device builder is 8
    want = HOST if name == "sheared_with_normals" else DEV
    same_scene(sd, precision, scene_rays(8192, 3, tmin=1e-7 if precision == F64 else 1e-4), want)


@pytest.mark.parametrize("precision", [F32, F64])
def test_coincident_placements_tie_on_the_instance_id(precision):
    """the prototype placed twice under one transform: the second placement (the larger instance id) is every hit"""
    sd = everything_scene()
    n = len(sd.instance_mesh)
    faces = sd.meshes[sd.instance_mesh[n - 1]].indices.shape[0]
    total = sd.n_shapes + sum(sd.meshes[m].indices.shape[0] for m in sd.instance_mesh)
    first_of_last, first_of_prev = total - faces, total - 2 * faces
    b = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        assert b.build_info() == built_by(precision, DEV)
        ids = b.trace_closest(abi(scene_rays(20000, 9), precision))["shape_id"]
        assert (ids >= first_of_last).sum() > 20 and not ((ids >= first_of_prev) & (ids < first_of_last)).any()
    finally:
        b.close()


@pytest.mark.parametrize("precision", [F32, F64, MIXED])
def test_placements_far_from_the_origin(precision):
    sd = everything_scene(OFFSET)
    same_scene(sd, precision, scene_rays(8192, 4, OFFSET, tmin=1e-7 if precision == F64 else 1e-3), min_hits=0.01)


@pytest.mark.parametrize("precision", [F32, F64, MIXED])
def test_full_width_nodes(precision):
    """TAKE_HIP_NODES=wide: every tree's float nodes as they are, or widened to double, child words rebased"""
    if os.environ.get("TAKE_HIP_NODES"):
        pytest.skip("experiment knobs select the node format")
    sd = everything_scene()
    a = capi.Scene(sd, precision=precision, builder=HOST)
    b = scene_with_node_format("wide", sd, precision=precision, builder=DEV)
    try:
        assert b.build_info() == built_by(precision, DEV)
        if precision != MIXED:
            same_hits(a, b, abi(scene_rays(8192, 6), precision))
        assert np.array_equal(a.render(spp=4, max_depth=6, seed=2), b.render(spp=4, max_depth=6, seed=2))
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 3. still the specified geometry
@pytest.mark.parametrize("precision", [F64, F32])
def test_device_built_instanced_equals_flattened(precision):
    """the bars of tests/test_instancing.py: shape ids agree on > 0.995 of the rays, f64 t at rounding level, f32 image
    RMSE < 3e-3"""
    f64 = precision == F64
    for sd in (scenes.instanced_scene(60, 500, 96, 96, spp=4, max_depth=50), everything_scene(res=96)):
        a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd.flattened(), precision=precision, builder=HOST)
        try:
            assert a.build_info() == built_by(precision, DEV)
            rays = abi(random_rays(50000, 4, tmin=1e-7 if f64 else 1e-4), precision)
            ha, hb = a.trace_closest(rays), b.trace_closest(rays)
            same = ha["shape_id"] == hb["shape_id"]
            print(f"\n{'f64' if f64 else 'f32'}: shape ids agree on {same.mean():.6f} of the rays")
            assert same.mean() > 0.995, same.mean()
            hit = same & (ha["shape_id"] >= 0)
            dt = np.abs(ha["t"][hit].astype(np.float64) - hb["t"][hit]) / np.maximum(1.0, hb["t"][hit])
            print(f"  max relative difference of t {dt.max():.3e}")
            assert dt.max() < (1e-13 if f64 else 1e-5), dt.max()
            assert np.array_equal(a.trace_any(rays).astype(bool), ha["shape_id"] >= 0)
            ia, ib = a.render(spp=4, max_depth=50, seed=5), b.render(spp=4, max_depth=50, seed=5)
            d = np.abs(ia.astype(np.float64) - ib).max(axis=2)
            print(f"  image RMSE {rmse(ia, ib):.3e}")
            if f64:
                assert np.median(d) < 1e-12 and (d < 1e-9).mean() > 0.99, (d < 1e-9).mean()
            else:
                assert rmse(ia, ib) < 3e-3, rmse(ia, ib)
        finally:
            a.close(), b.close()


# ------------------------------------------------------------------ 4. placement boxes, through hits
@pytest.mark.parametrize("precision", [F32, F64])
def test_sheared_placements_same_hits_as_the_host_build(precision):
    """both instances of k_placement_pad (mag * 4e-6 for float scenes, mag * 1e-13 for double ones) on boxes that are
    not the corners' boxes: 60 000 rays, hit tables bit-identical to the host build's"""
    same_scene(sheared_placements(), precision, random_rays(60000, 17, tmin=1e-7 if precision == F64 else 1e-4), spp=1, max_depth=2,
               min_hits=0.5)


def test_placement_boxes_contain_the_placed_geometry():
    """a placement box that lost part of its geometry loses hits the flattened scene has.  In double: a ray would have
    to pass within 1e-16 of an edge for the two spaces to disagree about it (in float the two spaces do disagree
    about rays through an edge, boxes or not: the float boxes are held to the host build's hits, above)."""
    sd = sheared_placements()
    a, b = capi.Scene(sd, precision=F64, builder=DEV), capi.Scene(sd.flattened(), precision=F64, builder=HOST)
    try:
        assert a.build_info() == built_by(F64, DEV)
        rays = abi(random_rays(60000, 17, tmin=1e-7), F64)
        ha, hb = a.trace_closest(rays), b.trace_closest(rays)
        hit = hb["shape_id"] >= 0
        assert hit.sum() > 10000
        assert (ha["shape_id"][hit] >= 0).all()
        # at that distance, to the rounding level tests/test_instancing.py allows an f64 t (1e-13, relative above t = 1)
        assert (ha["t"][hit] <= hb["t"][hit] + 1e-13 * np.maximum(1.0, hb["t"][hit])).all()
        assert np.array_equal(a.trace_any(rays).astype(bool)[hit], hit[hit])
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 5. a prototype decoded on the device
def mesh_to_ply(m):
    """a scene.Mesh's positions and faces as a double-precision binary PLY (values exact)"""
    vert = np.zeros(len(m.positions), [("x", "<f8"), ("y", "<f8"), ("z", "<f8")])
    vert["x"], vert["y"], vert["z"] = m.positions[:, 0], m.positions[:, 1], m.positions[:, 2]
    face = np.zeros(len(m.indices), [("n", "u1"), ("i", "<u4", 3)])
    face["n"], face["i"] = 3, m.indices
    hdr = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {len(vert)}", "property double x", "property double y",
                     "property double z", f"element face {len(face)}", "property list uchar uint vertex_indices", "end_header"]) + "\n"
    return hdr.encode() + vert.tobytes() + face.tobytes()


def test_device_decoded_prototype_in_a_mixed_scene():
    """file -> device arrays -> prototype records, placement boxes and trees of BOTH sides on the device: the positions
    never visit the host (tests/test_gpu_device_build_f64.py::test_device_decoded_soup_in_a_mixed_scene)"""
    sd = scenes.instanced_scene(40, 5000, 96, 64, spp=4)
    proto = sd.instance_mesh[0]
    dm = capi.DeviceMesh(mesh_to_ply(sd.meshes[proto]), material_id=sd.meshes[proto].material_id)
    sd_host, sd_dev = copy.copy(sd), copy.copy(sd)
    sd_host.meshes, sd_dev.meshes = list(sd.meshes), list(sd.meshes)
    sd_host.meshes[proto] = dm.download()
    sd_dev.meshes[proto] = dm
    assert np.array_equal(sd_host.meshes[proto].positions, sd.meshes[proto].positions)
    a = capi.Scene(sd_host, precision=MIXED, builder=HOST)
    b = capi.Scene(sd_dev, precision=MIXED, builder=DEV)
    try:
        assert b.build_info() == {"f32": DEV, "f64": DEV}
        for eb in (0, ALL_EXACT):
            ia, ib = render(a, eb, spp=4, max_depth=50, seed=3), render(b, eb, spp=4, max_depth=50, seed=3)
            assert np.array_equal(ia, ib) and ia.mean() > 0.01
    finally:
        a.close(), b.close(), dm.close()


def uploaded_mb(capfd):
    """MB the last scene_create copied host -> device for the device builder (its TAKE_HIP_VERBOSE line: mesh positions
    and shape arrays; positions that are on the device already are copied device to device and do not count)"""
    import re

    lines = re.findall(r"uploads pinned in place ([0-9.]+) MB, pageable ([0-9.]+) MB", capfd.readouterr().err)
    assert len(lines) == 1, lines  # once per scene: both sides of a mixed scene read one upload
    return float(lines[0][0]) + float(lines[0][1])


def test_device_decoded_prototype_positions_stay_on_the_device(capfd, monkeypatch):
    """a 200k-triangle prototype is 14.4 MB of positions.  From host arrays the device build uploads them; decoded on
    the device they are neither staged to the host nor uploaded again — a staged copy would come back up through the
    same host -> device copy and show in the figure."""
    sd = scenes.instanced_scene(16, 200_000, 48, 32, spp=1)
    proto = sd.instance_mesh[0]
    pos_mb = sd.meshes[proto].positions.nbytes / 1e6
    dm = capi.DeviceMesh(mesh_to_ply(sd.meshes[proto]), material_id=sd.meshes[proto].material_id)
    sd_dev = copy.copy(sd)
    sd_dev.meshes = list(sd.meshes)
    sd_dev.meshes[proto] = dm
    monkeypatch.setenv("TAKE_HIP_VERBOSE", "1")
    capfd.readouterr()
    a = capi.Scene(sd, precision=MIXED, builder=DEV)
    up_host = uploaded_mb(capfd)
    b = capi.Scene(sd_dev, precision=MIXED, builder=DEV)
    up_dev = uploaded_mb(capfd)
    try:
        print(f"\nprototype positions {pos_mb:.1f} MB; uploaded: host arrays {up_host:.1f} MB, device-decoded {up_dev:.1f} MB")
        assert a.build_info() == b.build_info() == {"f32": DEV, "f64": DEV}
        assert up_host >= pos_mb - 0.1 and up_dev < 0.5
        assert np.array_equal(a.render(spp=1, max_depth=6, seed=3), b.render(spp=1, max_depth=6, seed=3))
    finally:
        a.close(), b.close(), dm.close()


# ------------------------------------------------------------------ 6. fall-backs
@pytest.mark.parametrize("precision", [F32, MIXED])
def test_braided_scenes_stay_with_the_host_builder(precision, monkeypatch):
    """TAKE_HIP_BRAID > 1: a placement's entries are subtrees of a host tree"""
    sd = small(30, 300, 48)
    want = capi.Scene(sd, precision=precision, builder=HOST)
    monkeypatch.setenv("TAKE_HIP_BRAID", "4")
    a, b = pair(sd, precision, HOST)
    try:
        ia = a.render(spp=4, max_depth=6, seed=1)
        assert np.array_equal(ia, b.render(spp=4, max_depth=6, seed=1))
        if precision == F32:  # (the braided scene against the plain one: same hits, tests/test_instancing.py)
            rays = abi(random_rays(8192, 2), F32)
            assert np.array_equal(b.trace_closest(rays)["shape_id"], want.trace_closest(rays)["shape_id"])
    finally:
        a.close(), b.close(), want.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_prototype_of_coincident_triangles(precision):
    """5000 identical triangles (one Morton code) as a prototype: device trees or the fall-back to the host builder, the
    results equal the host build's (tests/test_gpu_device_build_f64.py::test_coincident_primitives_f64)"""
    sd = small(10, 100, 48)
    tri = np.array([[0.1, 0.1, 0.0], [0.3, 0.1, 0.0], [0.2, 0.3, 0.0]])
    p = sd.add_prototype(np.tile(tri, (5000, 1)), np.arange(15000, dtype=np.int32).reshape(-1, 3), 0)
    sd.add_instance(p, [[1, 0, 0, 0.2], [0, 1, 0, -0.3], [0, 0, 1, 0.5]])
    sd.add_instance(p, [[0, -2, 0, -0.4], [2, 0, 0, 0.1], [0, 0, 2, 0.2]], 1)
    a = capi.Scene(sd, precision=precision, builder=HOST)
    b = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        side = "f32" if precision == F32 else "f64"
        print(f"\na prototype of 5000 coincident triangles, {side}: built by {'the device' if b.build_info()[side] == DEV else 'the host (fall-back)'}")
        same_hits(a, b, abi(random_rays(30000, 9, tmin=1e-7 if precision == F64 else 1e-4), precision))
        assert np.array_equal(a.render(spp=2, max_depth=6, seed=1), b.render(spp=2, max_depth=6, seed=1))
    finally:
        a.close(), b.close()


def seven_primitive_scene(one_face=False):
    """2 shapes (a quad) + a prototype of 2 faces (or, one_face: of 1) + 3 placements"""
    sd = SceneData(width=16, height=16, lookfrom=(0.0, 0.0, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0,
                   background=(0.2, 0.3, 0.4), spp=1, max_depth=3)
    m = sd.add_material(D.MAT_DIFFUSE, (0.5, 0.5, 0.5))
    pos, idx, nrm, uv = scenes._quad((0, 0, -0.5), (1, 0, 0), (0, 1, 0), (0, 0, 1))
    sd.add_mesh(pos, idx, m, normals=nrm, uvs=uv)
    qp, qi, _, _ = scenes._quad((0, 0, 0), (0.3, 0, 0), (0, 0.3, 0), (0, 0, 1))
    p = sd.add_prototype(qp, qi[:1] if one_face else qi, m)
    n = 8 if one_face else 3
    for k in range(n):
        sd.add_instance(p, [[1, 0, 0, -0.5 + k / n], [0, 1, 0, 0.2 * (k % 3) - 0.2], [0, 0, 1, 0.1 * k]])
    return sd


@pytest.mark.parametrize("precision", [F32, F64, MIXED])
def test_tiny_scenes_and_one_face_prototypes_are_built_by_the_host(precision):
    """fewer than 8 primitives in all: the documented minimum.  A prototype of one face makes a tree of one leaf: the
    whole scene takes the host route (tk_build.hip: build_two_level_device)"""
    for sd in (seven_primitive_scene(), seven_primitive_scene(one_face=True)):
        a, b = pair(sd, precision, HOST)
        try:
            ia = a.render(spp=2, max_depth=3, seed=1)
            assert np.array_equal(ia, b.render(spp=2, max_depth=3, seed=1)) and ia.std() > 0
        finally:
            a.close(), b.close()


# ------------------------------------------------------------------ 7. size
def two_big_prototypes(tris, placements, res):
    sd = scenes.instanced_scene(placements, tris, res, res, spp=1)
    second = sd.add_prototype(*scenes.soup_triangles(tris, 999, 0.09, 0.01), 0)
    for i in range(1, placements, 2):
        sd.instance_mesh[i] = second
    return sd


@pytest.mark.parametrize("precision", [F32, MIXED])
def test_two_500k_triangle_prototypes_same_image_and_build_time(precision):
    sd = two_big_prototypes(500_000, 64, 96)
    t0 = time.time()
    a = capi.Scene(sd, precision=precision, builder=HOST)
    t_host = time.time() - t0
    t0 = time.time()
    b = capi.Scene(sd, precision=precision, builder=DEV)
    t_dev = time.time() - t0
    try:
        assert b.build_info() == built_by(precision, DEV)
        sa, sb = a.stats(), b.stats()
        print(f"\n2 x 500k triangles x 64 placements, {'f32' if precision == F32 else 'mixed'}: scene_create host SAH {t_host:.2f} s "
              f"({sa['n_nodes']} nodes, depth {sa['depth']}), device LBVH {t_dev:.2f} s ({sb['n_nodes']} nodes, depth {sb['depth']})")
        assert sa["n_prims"] == sb["n_prims"]
        assert np.array_equal(a.render(spp=1, max_depth=50, seed=4), b.render(spp=1, max_depth=50, seed=4))
    finally:
        a.close(), b.close()


def test_beyond_the_tight_box_limit():
    """210k prototype vertices x 2000 placements = 4.2e8 vertex transforms, past placement_box's limit of 4e8: the
    placements' boxes are the host's formula (corners' box cut by the bounding sphere's) around the device tree's bounds"""
    sd = scenes.instanced_scene(2000, 70_000, 96, 54, spp=1)
    assert len(sd.meshes[sd.instance_mesh[0]].positions) * len(sd.instance_mesh) > 4e8
    a, b = pair(sd, F32)
    try:
        same_hits(a, b, abi(random_rays(20000, 5), F32))
        assert np.array_equal(a.render(spp=1, max_depth=50, seed=2), b.render(spp=1, max_depth=50, seed=2))
    finally:
        a.close(), b.close()


def test_1000_placements_of_10k_triangles():
    """BASELINE configs[4]'s shape at a reduced frame"""
    sd = scenes.instanced_scene(1000, 10_000, 160, 90, spp=2)
    a, b = pair(sd, F32)
    try:
        ia = a.render(spp=2, max_depth=50, seed=1)
        # (a dark image: 1000 clouds of 10k triangles fill the closed box)
        assert np.array_equal(ia, b.render(spp=2, max_depth=50, seed=1)) and np.isfinite(ia).all() and ia.std() > 0
    finally:
        a.close(), b.close()

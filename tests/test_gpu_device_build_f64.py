"""Double-precision and mixed-precision scenes built on the device (TAKE_BUILDER_DEVICE_LBVH: k_make_prims<double>,
k_prim_boxes<double> with outward-rounded float boxes, take_amd/csrc/tk_build_gpu.h) against the host SAH build and the
oracle's exhaustive search.  As for f32 scenes (tests/test_gpu_device_build.py) the tree differs and the RESULTS must
not: every comparison here is np.array_equal."""
import copy
import os
import time

import numpy as np
import pytest

import oracle
from helpers import GOLDEN_SCENES, golden_scene, random_rays, rays_to_abi
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import SceneData

pytestmark = pytest.mark.gpu
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
F64, MIXED = D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
ALL_EXACT = 60  # more exact bounces than a depth-50 path has rounds


def same_hits(a, b, rays):
    ha, hb = a.trace_closest(rays), b.trace_closest(rays)
    for f in ("shape_id", "t", "u", "v"):
        assert np.array_equal(ha[f], hb[f]), f
    assert np.array_equal(a.trace_any(rays), b.trace_any(rays))
    return hb


def same_as_exhaustive_search(sd, hits, occ, rays8):
    osc = oracle.OracleScene(sd, precision=1)
    want = osc.isect_brute(rays8)
    osc.close()
    assert np.array_equal(hits["shape_id"], want[:, 0].astype(np.int32))
    hit = want[:, 0] >= 0
    assert hit.sum() > len(hit) // 20
    for k, col in (("t", 1), ("u", 2), ("v", 3)):
        assert np.array_equal(hits[k][hit], want[hit, col]), k
    assert np.array_equal(occ.astype(bool), hit)


def pair(sd, precision, **kw):
    """(host-built, device-built) scenes; the device one must really be device-built on every side it has"""
    a = capi.Scene(sd, precision=precision, builder=HOST, **kw)
    b = capi.Scene(sd, precision=precision, builder=DEV, **kw)
    want = {"f32": DEV if precision == MIXED else -1, "f64": DEV}
    assert b.build_info() == want, b.build_info()
    return a, b


def scene_with_node_format(fmt, sd, **kw):
    """a scene built under TAKE_HIP_NODES=fmt (read once, when the scene is built); the variable is put back"""
    old = os.environ.get("TAKE_HIP_NODES")
    try:
        if fmt is None:
            os.environ.pop("TAKE_HIP_NODES", None)
        else:
            os.environ["TAKE_HIP_NODES"] = fmt
        return capi.Scene(sd, **kw)
    finally:
        if old is None:
            os.environ.pop("TAKE_HIP_NODES", None)
        else:
            os.environ["TAKE_HIP_NODES"] = old


def render(sc, exact_bounces=0, **kw):
    sc.exact_bounces = exact_bounces
    return sc.render(**kw)


def seven_shape_scene():
    sd = SceneData(width=16, height=16, lookfrom=(0.0, 0.0, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0,
                   background=(0.2, 0.3, 0.4), spp=1, max_depth=3)
    m = sd.add_material(D.MAT_DIFFUSE, (0.5, 0.5, 0.5))
    for z in (0.0, -0.5, -1.0):
        pos, idx, nrm, uv = scenes._quad((0, 0, z), (1, 0, 0), (0, 1, 0), (0, 0, 1))
        sd.add_mesh(pos, idx, m, normals=nrm, uvs=uv)
    sd.add_mesh(np.array([[0.0, 0.0, 0.5], [0.5, 0.0, 0.5], [0.0, 0.5, 0.5]]), np.array([[0, 1, 2]], np.int32), m)
    assert sd.n_shapes == 7
    return sd


def test_double_sides_are_built_on_the_device_when_asked():
    sd = scenes.soup_scene(100_000, 64, 64, spp=1)
    for precision, builder, want in ((F64, DEV, {"f32": -1, "f64": DEV}), (MIXED, DEV, {"f32": DEV, "f64": DEV}),
                                     (F64, HOST, {"f32": -1, "f64": HOST}), (MIXED, HOST, {"f32": HOST, "f64": HOST}),
                                     (D.TAKE_PRECISION_F32, DEV, {"f32": DEV, "f64": -1}),
                                     (MIXED, D.TAKE_BUILDER_AUTO, {"f32": HOST, "f64": HOST})):  # (below AUTO's threshold)
        sc = capi.Scene(sd, precision=precision, builder=builder)
        try:
            assert sc.build_info() == want, (precision, builder, sc.build_info())
        finally:
            sc.close()
    tiny = seven_shape_scene()  # fewer than 8 shapes: the documented minimum of the device builder
    for precision, want in ((F64, {"f32": -1, "f64": HOST}), (MIXED, {"f32": HOST, "f64": HOST})):
        sc = capi.Scene(tiny, precision=precision, builder=DEV)
        try:
            assert sc.build_info() == want
        finally:
            sc.close()


@pytest.mark.parametrize("name", GOLDEN_SCENES + ["soup100k"])
def test_f64_hit_tables_do_not_depend_on_the_builder(name):
    sd = scenes.soup_scene(100_000, 64, 64, spp=1) if name == "soup100k" else golden_scene(name)
    assert sd.n_shapes >= 8
    rays8 = random_rays(60_000, 5, tmin=1e-7)
    rays = rays_to_abi(rays8, 1)
    a, b = pair(sd, F64)
    try:
        hits = same_hits(a, b, rays)
        occ = b.trace_any(rays)
        st = b.stats()
        assert st["n_prims"] == sd.n_shapes and st["depth"] >= 1
    finally:
        a.close(), b.close()
    if name == "soup1k":
        same_as_exhaustive_search(sd, hits, occ, rays8)


def envmap_soup():
    return scenes.soup_scene(1000, 64, 64, spp=2, envmap=(128, 64))


@pytest.mark.parametrize("precision", [F64, MIXED])
@pytest.mark.parametrize("name", ["cbox", "mats", "meshlight", "spherelight", "envmap_soup"])
def test_images_do_not_depend_on_the_builder(name, precision):
    sd = envmap_soup() if name == "envmap_soup" else golden_scene(name)
    a, b = pair(sd, precision)
    try:
        for eb in ((0,) if precision == F64 else (0, 1, ALL_EXACT)):
            ia, ib = render(a, eb, spp=4, max_depth=50, seed=3), render(b, eb, spp=4, max_depth=50, seed=3)
            assert np.array_equal(ia, ib), eb
            assert np.isfinite(ia).all() and ia.mean() > 0
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("precision", [F64, MIXED])
@pytest.mark.parametrize("leaf", [1, 2, 3, 4])
def test_leaf_sizes(leaf, precision):
    sd = scenes.soup_scene(100_000, 128, 128, spp=1)
    a = capi.Scene(sd, precision=precision, builder=HOST)
    b = capi.Scene(sd, precision=precision, builder=DEV, max_leaf_size=leaf)
    try:
        assert b.build_info()["f64"] == DEV
        same_hits(a, b, rays_to_abi(random_rays(50_000, 11, tmin=1e-7), 1))
        assert np.array_equal(a.render(spp=2, max_depth=50, seed=1), b.render(spp=2, max_depth=50, seed=1))
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("precision", [F64, MIXED])
def test_full_width_double_nodes_from_the_device(precision):
    """TAKE_HIP_NODES=wide: the f64 kernels traverse Node4<double>, the device tree's float nodes widened"""
    if os.environ.get("TAKE_HIP_NODES"):
        pytest.skip("experiment knobs select the node format")
    sd = scenes.soup_scene(50_000, 128, 128, spp=1)
    a = capi.Scene(sd, precision=precision, builder=HOST)
    b = scene_with_node_format("wide", sd, precision=precision, builder=DEV)
    try:
        assert b.build_info()["f64"] == DEV
        b.set_instrumentation(timing=False, counting=True)
        ib = b.render(spp=1, max_depth=50, seed=2)
        if precision == F64:
            assert b.counters()["node_bytes"] == 4 * 64  # sizeof(Node4<double>): four 16-byte-aligned children of 6 doubles + a word
        b.set_instrumentation(False, False)
        assert np.array_equal(a.render(spp=1, max_depth=50, seed=2), ib)
        same_hits(a, b, rays_to_abi(random_rays(50_000, 13, tmin=1e-7), 1))
    finally:
        a.close(), b.close()


OFFSET = np.array([1000.3, -2000.7, 500.1])


def far_scene(extent, n, jitter):
    """a soup of the given extent around OFFSET, camera and all: vertices made in double, none of them a float"""
    rng = np.random.default_rng(77)
    c = rng.uniform(-0.45 + jitter, 0.45 - jitter, (n, 1, 3)) if jitter < 0.45 else np.zeros((n, 1, 3))
    pos = (OFFSET + extent * (c + rng.uniform(-jitter, jitter, (n, 3, 3)))).reshape(-1, 3)
    sd = SceneData(width=96, height=96, lookfrom=tuple(OFFSET + extent * np.array([0.0, 0.0, 2.0])), lookat=tuple(OFFSET),
                   up=(0.0, 1.0, 0.0), vfov=35.0, background=(0.5, 0.6, 0.7), spp=2, max_depth=50)
    sd.add_mesh(pos, np.arange(3 * n, dtype=np.int32).reshape(n, 3), sd.add_material(D.MAT_DIFFUSE, (0.7, 0.6, 0.5)))
    return sd, pos


def far_rays(extent, n, seed):
    r = random_rays(n, seed, tmin=1e-7)
    r[:, 0:3] = OFFSET + 0.5 * extent * r[:, 0:3]  # origins inside and around the soup, a share from outside (z = 1.95 extents)
    r[:, 7] *= extent
    return r


# extent 1e-3: the triangles span the soup.  The triangle test culls |det| < 1e-7 (the reference's epsilon), and det is
# of the order of the edges' product: 4e-5 triangles — the extent-1 soup scaled down — are never hit by anything.
@pytest.mark.parametrize("extent,n,jitter", [(1.0, 20_000, 0.02), (1e-3, 2_000, 0.5)])
def test_far_from_the_origin(extent, n, jitter):
    """where float boxes around double geometry are coarsest: at |x| ~ 2000 floats are 1.2e-4 apart — 12 % of the
    whole extent-1e-3 soup — and no vertex is a float, so every box plane is a rounded one.  A box that lost part of
    a triangle would lose hits against the host build and exhaustive search.  (It does not tell outward rounding from
    rounding to nearest followed by the one-float widening, which contains the geometry too; the rounding itself is
    held to its specification by tests/test_build_info_cpu.py.)"""
    sd, pos = far_scene(extent, n, jitter)
    assert (pos.astype(np.float32).astype(np.float64) != pos).all()  # no coordinate survives a rounding to float
    rays8 = far_rays(extent, 60_000, 21)
    rays = rays_to_abi(rays8, 1)
    a, b = pair(sd, F64)
    try:
        hits = same_hits(a, b, rays)
        occ = b.trace_any(rays)
        ia, ib = a.render(spp=2, max_depth=50, seed=5), b.render(spp=2, max_depth=50, seed=5)
        assert np.array_equal(ia, ib) and np.isfinite(ia).all() and ia.std() > 0
    finally:
        a.close(), b.close()
    same_as_exhaustive_search(sd, hits, occ, rays8)


def test_coincident_primitives_f64():
    """5000 identical triangles (one Morton code): device tree or fall-back, the results equal the host build's"""
    sd = scenes.soup_scene(64, 64, 64, spp=1)
    tri = np.array([[0.1, 0.1, 0.0], [0.3, 0.1, 0.0], [0.2, 0.3, 0.0]])
    sd.add_mesh(np.tile(tri, (5000, 1)), np.arange(15000, dtype=np.int32).reshape(-1, 3), 0)
    a = capi.Scene(sd, precision=F64, builder=HOST)
    b = capi.Scene(sd, precision=F64, builder=DEV)
    try:
        print(f"\n5000 coincident triangles, f64: built by {'the device' if b.build_info()['f64'] == DEV else 'the host (fall-back)'}")
        same_hits(a, b, rays_to_abi(random_rays(50_000, 9, tmin=1e-7), 1))
        assert np.array_equal(a.render(spp=1, max_depth=10, seed=1), b.render(spp=1, max_depth=10, seed=1))
    finally:
        a.close(), b.close()


def test_exact_ties_resolve_the_same_way_in_every_f64_tree():
    """the two coplanar, overlapping quads of test_gpu_device_build.py: every ray into the overlap has an exact tie in t"""
    sd = SceneData(width=96, height=96, lookfrom=(0.3, 0.4, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=45.0,
                   background=(0.1, 0.1, 0.1), spp=4, max_depth=6)
    red = sd.add_material(D.MAT_DIFFUSE, (0.8, 0.1, 0.1))
    blue = sd.add_material(D.MAT_DIFFUSE, (0.1, 0.1, 0.8))
    grey = sd.add_material(D.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    for c, m in (((-0.3, 0.0, 0.0), red), ((0.3, 0.1, 0.0), blue)):
        pos, idx, nrm, uv = scenes._quad(c, (0.7, 0, 0), (0, 0.7, 0), (0, 0, 1))
        sd.add_mesh(pos, idx, m, normals=nrm, uvs=uv)
    rng = np.random.default_rng(5)
    for k in range(64):
        x, z = (k % 8) * 0.25 - 1.0, (k // 8) * 0.25 - 1.0
        lo, hi = np.array([x, -1.0, z]), np.array([x + 0.25, -1.0 + rng.uniform(0.1, 0.5), z + 0.25])
        corners = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], lo[2]],
                            [lo[0], lo[1], hi[2]], [hi[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]])
        faces = np.array([[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 4, 5], [0, 5, 1], [3, 2, 6], [3, 6, 7],
                          [0, 3, 7], [0, 7, 4], [1, 5, 6], [1, 6, 2]], np.int32)
        sd.add_mesh(corners, faces, grey)
    pos, idx, nrm, uv = scenes._quad((0, 1.5, 0), (0.5, 0, 0), (0, 0, 0.5), (0, -1, 0))
    sd.add_mesh(pos, idx, grey, normals=nrm, uvs=uv, emission=(10.0, 10.0, 10.0))
    imgs = []
    for builder, fmt in ((HOST, None), (DEV, None), (HOST, "wide"), (DEV, "wide")):
        sc = scene_with_node_format(fmt, sd, precision=F64, builder=builder)
        assert sc.build_info()["f64"] == builder
        imgs.append(sc.render(spp=4, max_depth=6, seed=8))
        sc.close()
    for im in imgs[1:]:
        assert np.array_equal(imgs[0], im)
    assert np.isfinite(imgs[0]).all() and imgs[0][40:56, 44:52].mean() > 0


def mesh_to_ply(m):
    """a scene.Mesh as a double-precision binary PLY (values exact), normals / uvs if it has them"""
    cols = [("x", m.positions[:, 0]), ("y", m.positions[:, 1]), ("z", m.positions[:, 2])]
    if m.normals is not None:
        cols += [("nx", m.normals[:, 0]), ("ny", m.normals[:, 1]), ("nz", m.normals[:, 2])]
    if m.uvs is not None:
        cols += [("u", m.uvs[:, 0]), ("v", m.uvs[:, 1])]
    vert = np.zeros(len(m.positions), [(k, "<f8") for k, _ in cols])
    for k, c in cols:
        vert[k] = c
    face = np.zeros(len(m.indices), [("n", "u1"), ("i", "<u4", 3)])
    face["n"], face["i"] = 3, m.indices
    hdr = "\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {len(vert)}"] + [f"property double {k}" for k, _ in cols] +
                    [f"element face {len(face)}", "property list uchar uint vertex_indices", "end_header"]) + "\n"
    return hdr.encode() + vert.tobytes() + face.tobytes()


@pytest.mark.parametrize("normals", [None, "scene"])
def test_device_decoded_soup_in_a_mixed_scene(normals):
    """file -> device arrays -> records and trees of BOTH sides on the device: the positions never visit the host"""
    sd = scenes.soup_scene(20_000, 96, 64, spp=4)
    soup = max(range(len(sd.meshes)), key=lambda i: sd.meshes[i].indices.shape[0])
    dm = capi.DeviceMesh(mesh_to_ply(sd.meshes[soup]), material_id=sd.meshes[soup].material_id, normals=normals)
    sd_host, sd_dev = copy.copy(sd), copy.copy(sd)
    sd_host.meshes, sd_dev.meshes = list(sd.meshes), list(sd.meshes)
    sd_host.meshes[soup] = dm.download()  # (with the device-computed normals, if any)
    sd_dev.meshes[soup] = dm
    assert np.array_equal(sd_host.meshes[soup].positions, sd.meshes[soup].positions)
    assert (sd_host.meshes[soup].normals is not None) == (normals == "scene")
    a = capi.Scene(sd_host, precision=MIXED, builder=HOST)
    b = capi.Scene(sd_dev, precision=MIXED, builder=DEV)
    try:
        assert b.build_info() == {"f32": DEV, "f64": DEV}
        for eb in (0, ALL_EXACT):
            ia, ib = render(a, eb, spp=4, max_depth=50, seed=3), render(b, eb, spp=4, max_depth=50, seed=3)
            assert np.array_equal(ia, ib) and ia.mean() > 0.01
    finally:
        a.close(), b.close(), dm.close()


@pytest.mark.parametrize("precision", [F64, MIXED])
def test_device_decoded_meshes_with_an_area_light(precision):
    """every mesh of the meshlight scene decoded on the device; the emissive one is staged for the light records while
    the others stay on the device"""
    sd = golden_scene("meshlight")
    dms = [capi.DeviceMesh(mesh_to_ply(m), material_id=m.material_id) for m in sd.meshes]
    sd_host, sd_dev = copy.copy(sd), copy.copy(sd)
    sd_host.meshes = [dm.download() for dm in dms]
    sd_dev.meshes = list(dms)
    a = capi.Scene(sd_host, precision=precision, builder=HOST)
    b = capi.Scene(sd_dev, precision=precision, builder=DEV)
    try:
        assert b.build_info()["f64"] == DEV
        ia, ib = a.render(spp=4, max_depth=50, seed=2), b.render(spp=4, max_depth=50, seed=2)
        assert np.array_equal(ia, ib) and ia.mean() > 0.01
    finally:
        a.close(), b.close()
        for dm in dms:
            dm.close()


@pytest.mark.parametrize("precision", [F64, MIXED])
def test_1m_triangles_same_results_and_build_time(precision):
    sd = scenes.soup_scene(1_000_000, 1920, 1080, spp=1)
    t0 = time.time()
    a = capi.Scene(sd, precision=precision, builder=HOST)
    t_host = time.time() - t0
    t0 = time.time()
    b = capi.Scene(sd, precision=precision, builder=DEV)
    t_dev = time.time() - t0
    try:
        assert b.build_info()["f64"] == DEV and (precision == F64 or b.build_info()["f32"] == DEV)
        sa, sb = a.stats(), b.stats()
        print(f"\n1M triangles, {'f64' if precision == F64 else 'mixed'}: scene_create host SAH {t_host:.2f} s ({sa['n_nodes']} nodes, "
              f"depth {sa['depth']}), device LBVH {t_dev:.2f} s ({sb['n_nodes']} nodes, depth {sb['depth']})")
        assert sb["n_prims"] == sa["n_prims"]
        same_hits(a, b, rays_to_abi(random_rays(200_000, 3, tmin=1e-7), 1))
        assert np.array_equal(a.render(spp=1, max_depth=50, seed=4), b.render(spp=1, max_depth=50, seed=4))
        for sc, nm in ((a, "host SAH"), (b, "device LBVH")):
            sc.set_instrumentation(timing=True, counting=True)
            sc.render(spp=1, max_depth=50, seed=4)
            c = sc.counters()
            sc.set_instrumentation(False, False)
            rays_n = c["rays_closest"] + c["rays_shadow"]
            print(f"  {nm}: {c['node_visits'] / rays_n:.1f} nodes/ray, {c['prim_tests'] / rays_n:.1f} prims/ray")
    finally:
        a.close(), b.close()


def test_f64_device_built_scene_group():
    sd = golden_scene("cbox")
    one = capi.Scene(sd, precision=F64, builder=DEV)
    assert one.build_info() == {"f32": -1, "f64": DEV}
    want = one.render(spp=4, max_depth=50, seed=6)
    one.close()
    g = capi.SceneGroup(sd, [0, 0], precision=F64, builder=DEV)
    try:
        assert g.size() == 2
        assert np.array_equal(g.render(spp=4, max_depth=50, seed=6), want)
    finally:
        g.close()

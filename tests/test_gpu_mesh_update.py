"""Moving the vertices of a resident scene: take_hip_scene_set_mesh_vertices (k_update_prims, k_convert_normals,
k_update_lights, then creation's own tail — take_amd/csrc/tk_build_gpu.h, tk_build.hip: update_mesh_vertices_device).
The yardstick is always a FRESH capi.Scene of the same description with the new arrays, built by the device LBVH
builder with the same max_leaf_size: the resident tree (debug_tree: nodes, records, grid, info of every side), hit
tables, occlusion and images, all np.array_equal."""
import copy
import dataclasses
import time

import numpy as np
import pytest

from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import Light, SceneData
from test_gpu_device_build_instanced import ALL_EXACT, OFFSET, abi, bent_grid, built_by, render, same_hits, scene_rays, scene_with_node_format
from test_gpu_repose import same_everything, tmin_of
from test_instancing import small

pytestmark = pytest.mark.gpu
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]
GRID, SOUP = 0, 1  # the meshes of base_scene


def base_scene(offset=(0.0, 0.0, 0.0), res=48):
    """mesh 0: a bent grid of 1458 triangles with vertex normals and uvs; mesh 1: a soup of 700 triangles with neither;
    three spheres; a point light.  2161 records: no multiple of 64 or of the build's block size of 256"""
    off = np.asarray(offset, np.float64)
    sd = SceneData(width=res, height=res, lookfrom=tuple(off + (0.0, 1.0, 3.9)), lookat=tuple(off), up=(0.0, 1.0, 0.0), vfov=39.0,
                   background=(0.2, 0.3, 0.4), spp=4, max_depth=6)
    white = sd.add_material(D.MAT_DIFFUSE, (0.73, 0.73, 0.73))
    red = sd.add_material(D.MAT_DIFFUSE, (0.65, 0.05, 0.05))
    blue = sd.add_material(D.MAT_PLASTIC, (0.2, 0.3, 0.8), (1.5,))
    gold = sd.add_material(D.MAT_BLINN_PHONG_MICROFACET, (0.8, 0.7, 0.3), (50.0,))
    pos, idx, nrm, uv = bent_grid(27)
    sd.add_mesh(2.0 * pos + off + (0.0, -0.6, 0.0), idx, gold, normals=nrm, uvs=uv)
    cloud, cidx = scenes.soup_triangles(700, 77, 0.6, 0.08)
    sd.add_mesh(cloud + off + (0.0, 0.2, 0.0), cidx, red)
    sd.add_sphere(tuple(off + (-0.7, -0.2, 0.3)), 0.3, blue)
    sd.add_sphere(tuple(off + (0.75, -0.25, -0.2)), 0.25, white)
    sd.add_sphere(tuple(off + (0.0, 0.9, -0.4)), 0.2, gold)
    sd.lights.append(Light(0, -1, (12.0, 12.0, 12.0), tuple(off + (0.3, 2.0, 1.5))))
    assert sd.n_shapes == 2161 and sd.n_shapes % 64 and sd.n_shapes % 256
    return sd


def with_arrays(sd, updates):
    """the description with other positions / normals of some meshes: {mesh: positions} or {mesh: (positions, normals)},
    normals None = the mesh's own"""
    out = copy.copy(sd)
    out.meshes = list(sd.meshes)
    for m, arrays in updates.items():
        pos, nrm = arrays if isinstance(arrays, tuple) else (arrays, None)
        old = sd.meshes[m]
        out.meshes[m] = dataclasses.replace(old, positions=np.ascontiguousarray(pos, np.float64), normals=old.normals if nrm is None else np.ascontiguousarray(nrm, np.float64))
    return out


def smooth(pos):
    return pos + 0.12 * np.sin(3.0 * pos[:, [1, 2, 0]] + 0.5)


def crumpled(pos):
    c = pos.mean(axis=0)
    return c + 0.1 * (pos - c)


def sides_of(precision):
    return {F32: (F32,), F64: (F64,), MIXED: (F32, F64)}[precision]


def same_trees(a, b, precision):
    """the resident tree of every side, byte for byte: nodes, records, grid, info"""
    for side in sides_of(precision):
        ta, tb = a.debug_tree(side), b.debug_tree(side)
        assert set(ta) == set(tb)
        for k in ta:
            assert np.array_equal(ta[k], tb[k]), (side, k)
        assert ta["n_prims"] > 0 and ta["n_nodes"] > 0


def same_scene(a, b, precision, rays8, **kw):
    same_trees(a, b, precision)
    same_everything(a, b, precision, rays8, **kw)
    sa, sb = a.stats(), b.stats()
    assert (sa["n_nodes"], sa["n_prims"], sa["depth"]) == (sb["n_nodes"], sb["n_prims"], sb["depth"])


def snapshot(sc, precision, rays):
    out = [render(sc, eb, spp=2, max_depth=6, seed=1) for eb in ((0, ALL_EXACT) if precision == MIXED else (0,))]
    if precision != MIXED:
        h = sc.trace_closest(rays)
        out += [h[f] for f in ("shape_id", "t", "u", "v")] + [sc.trace_any(rays)]
    for side in sides_of(precision):
        t = sc.debug_tree(side)
        out += [np.asarray(t[k]) for k in sorted(t)]
    return out


def unchanged(sc, precision, rays, before):
    return all(np.array_equal(p, q) for p, q in zip(before, snapshot(sc, precision, rays)))


# ------------------------------------------------------------------ 1. equals a fresh scene
@pytest.mark.parametrize("builder", [DEV, HOST])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_updated_scene_equals_a_fresh_scene(precision, builder):
    """a smooth deformation of the grid, then the grid crumpled into a tenth of its extent: the node count changes.  A
    is built by the device in one run and by the host SAH in the other; afterwards the device has built every side."""
    sd = base_scene()
    rays = scene_rays(8192, 3, tmin=tmin_of(precision))
    a = capi.Scene(sd, precision=precision, builder=builder)
    try:
        assert a.build_info() == built_by(precision, builder)
        n_nodes = [a.stats()["n_nodes"]]
        for deform in (smooth, crumpled):
            pos = deform(sd.meshes[GRID].positions)
            a.set_mesh_vertices({GRID: pos})
            assert a.build_info() == built_by(precision, DEV)
            n_nodes.append(a.stats()["n_nodes"])
            b = capi.Scene(with_arrays(sd, {GRID: pos}), precision=precision, builder=DEV)
            try:
                same_scene(a, b, precision, rays)
            finally:
                b.close()
        print(f"\nnodes: created {n_nodes[0]}, smooth {n_nodes[1]}, crumpled {n_nodes[2]}")
        assert n_nodes[1] != n_nodes[2], n_nodes
    finally:
        a.close()


# ------------------------------------------------------------------ 2. round trip and repetition
@pytest.mark.parametrize("precision", PRECISIONS)
def test_round_trip_and_repetition(precision):
    sd = base_scene()
    rays = scene_rays(8192, 3, tmin=tmin_of(precision))
    pos = smooth(sd.meshes[SOUP].positions)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        i0 = a.render(spp=4, max_depth=6, seed=5)
        a.set_mesh_vertices({SOUP: pos})
        once = snapshot(a, precision, abi(rays, precision))
        assert not np.array_equal(i0, render(a, 0, spp=4, max_depth=6, seed=5))
        a.set_mesh_vertices({SOUP: pos})  # the same again: the same bytes
        assert unchanged(a, precision, abi(rays, precision), once)
        a.set_mesh_vertices({SOUP: sd.meshes[SOUP].positions})
        same_scene(a, b, precision, rays)
        assert np.array_equal(i0, render(a, 0, spp=4, max_depth=6, seed=5))  # (same_scene left a at all-exact bounces)
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 3. both meshes in one call; device pointers
@pytest.mark.parametrize("precision", PRECISIONS)
def test_both_meshes_and_device_pointers(precision):
    import torch

    sd = base_scene()
    rays = scene_rays(8192, 4, tmin=tmin_of(precision))
    new = {GRID: (smooth(sd.meshes[GRID].positions), sd.meshes[GRID].normals[::-1].copy()), SOUP: crumpled(sd.meshes[SOUP].positions)}
    a, c = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(with_arrays(sd, new), precision=precision, builder=DEV)
    try:
        a.set_mesh_vertices(new)
        same_scene(a, b, precision, rays)
        on_device = {GRID: tuple(torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in new[GRID]), SOUP: torch.from_numpy(new[SOUP]).to("cuda")}
        c.set_mesh_vertices(on_device)
        same_scene(c, b, precision, rays)
        # host arrays for one mesh and device arrays for the other, in one call
        c.set_mesh_vertices({GRID: sd.meshes[GRID].positions, SOUP: torch.from_numpy(sd.meshes[SOUP].positions).to("cuda")})
        c.set_mesh_vertices({SOUP: on_device[SOUP], GRID: new[GRID]})
        same_scene(c, b, precision, rays)
    finally:
        a.close(), b.close(), c.close()


# ------------------------------------------------------------------ 4. normals
@pytest.mark.parametrize("precision", PRECISIONS)
def test_normals_are_replaced_or_kept(precision):
    sd = base_scene()
    rays = scene_rays(8192, 5, tmin=tmin_of(precision))
    pos = smooth(sd.meshes[GRID].positions)
    nrm = sd.meshes[GRID].normals * [-1.0, 1.0, 1.0] + [0.0, 0.0, 0.4]
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        a.set_mesh_vertices({GRID: (pos, None)})  # the old normals stay
        kept = a.render(spp=4, max_depth=6, seed=5)
        b = capi.Scene(with_arrays(sd, {GRID: pos}), precision=precision, builder=DEV)
        try:
            same_scene(a, b, precision, rays)
        finally:
            b.close()
        a.set_mesh_vertices({GRID: (pos, nrm)})
        assert not np.array_equal(kept, render(a, 0, spp=4, max_depth=6, seed=5))
        b = capi.Scene(with_arrays(sd, {GRID: (pos, nrm)}), precision=precision, builder=DEV)
        try:
            same_scene(a, b, precision, rays)
        finally:
            b.close()
    finally:
        a.close()


# ------------------------------------------------------------------ 5. an emissive mesh
def emissive_scene():
    """a box of walls lit only by 20 of the 72 faces of a bent grid under the ceiling (mesh 5), and a soup"""
    sd = SceneData(width=40, height=40, lookfrom=(0.0, 0.0, 3.9), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=39.0,
                   background=(0.0, 0.0, 0.0), spp=4, max_depth=5)
    white = sd.add_material(D.MAT_DIFFUSE, (0.73, 0.73, 0.73))
    red = sd.add_material(D.MAT_DIFFUSE, (0.65, 0.05, 0.05))
    for c, ux, uy, n in (((0, 0, -1), (1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, -1, 0), (1, 0, 0), (0, 0, -1), (0, 1, 0)),
                         ((0, 1, 0), (1, 0, 0), (0, 0, 1), (0, -1, 0)), ((-1, 0, 0), (0, 0, -1), (0, 1, 0), (1, 0, 0)),
                         ((1, 0, 0), (0, 0, 1), (0, 1, 0), (-1, 0, 0))):
        p, i, nn, uv = scenes._quad(c, ux, uy, n)
        sd.add_mesh(p, i, red if c[0] else white, normals=nn, uvs=uv)
    pos, idx, nrm, uv = bent_grid(6)
    first = sd.n_shapes
    lamp = sd.add_mesh(0.6 * pos + (0.0, 0.8, 0.0), idx, white, normals=-nrm, uvs=uv)
    for f in range(7, 67, 3):  # 20 faces, the rest of the mesh does not emit
        sd.shape_area_light[first + f] = len(sd.lights)
        sd.lights.append(Light(1, first + f, (40.0, 35.0, 25.0)))
    sd.add_sphere((0.5, -0.6, 0.2), 0.2, white, emission=(3.0, 3.0, 6.0))  # a light the update leaves alone
    cloud, cidx = scenes.soup_triangles(150, 5, 0.5, 0.1)
    sd.add_mesh(cloud + (0.0, -0.3, 0.0), cidx, white)
    assert lamp == 5
    return sd, lamp


@pytest.mark.parametrize("precision", PRECISIONS)
def test_emissive_mesh_light_records_and_power_tables(precision):
    sd, lamp = emissive_scene()
    old = sd.meshes[lamp].positions
    centre = old.mean(axis=0)
    new = {"deformed": (smooth(old) - (0.0, 0.15, 0.0), None), "scaled by 2": (centre + 2.0 * (old - centre) - (0.0, 0.1, 0.0), None),
           "new normals": (old, -bent_grid(6)[2][::-1].copy())}
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        # (integrator 3 picks lights by the power tables; a mixed scene renders integrator 0 only: its two sides are
        # the f32 and f64 scenes' code)
        integrators = (0,) if precision == MIXED else (0, 3)
        power_before = a.render(spp=4, max_depth=5, seed=2, integrator=integrators[-1])
        for name, arrays in new.items():
            a.set_mesh_vertices({lamp: arrays})
            b = capi.Scene(with_arrays(sd, {lamp: arrays}), precision=precision, builder=DEV)
            try:
                same_trees(a, b, precision)
                for integrator in integrators:
                    for eb in ((0, ALL_EXACT) if precision == MIXED else (0,)):
                        ia = render(a, eb, spp=4, max_depth=5, seed=2, integrator=integrator)
                        assert np.array_equal(ia, render(b, eb, spp=4, max_depth=5, seed=2, integrator=integrator)), (name, integrator, eb)
                        assert np.isfinite(ia).all() and ia.mean() > 0
                if name == "scaled by 2":  # four times the lamp's power against the sphere light's: other picks
                    assert not np.array_equal(power_before, render(a, 0, spp=4, max_depth=5, seed=2, integrator=integrators[-1]))
            finally:
                b.close()
    finally:
        a.close()


# ------------------------------------------------------------------ 6. the tie rule
@pytest.mark.parametrize("precision", [F32, F64])
def test_faces_made_coincident_tie_on_the_larger_shape_id(precision):
    """a mesh of two separate triangles with different vertex normals, in front of the camera; the update puts the
    second exactly onto the first: every hit there carries the larger shape id"""
    sd = base_scene()
    tri = np.array([[-0.4, 0.1, 1.6], [0.4, 0.1, 1.6], [0.0, 0.7, 1.6]])
    pos = np.concatenate([tri, tri + (0.0, 0.0, -0.3)])
    nrm = np.concatenate([np.tile([0.0, 0.0, 1.0], (3, 1)), np.tile([0.6, 0.0, 0.8], (3, 1))])
    first = sd.n_shapes
    pair = sd.add_mesh(pos, np.array([[0, 1, 2], [3, 4, 5]], np.int32), 0, normals=nrm)
    onto = np.concatenate([tri, tri])
    rays = abi(scene_rays(20000, 9), precision)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(with_arrays(sd, {pair: onto}), precision=precision, builder=DEV)
    try:
        assert (a.trace_closest(rays)["shape_id"] == first).sum() > 20
        a.set_mesh_vertices({pair: onto})
        same_trees(a, b, precision)
        ids = same_hits(a, b, rays)["shape_id"]
        assert (ids == first + 1).sum() > 20 and not (ids == first).any()
        assert np.array_equal(a.render(spp=4, max_depth=6, seed=5), b.render(spp=4, max_depth=6, seed=5))
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 7. far from the origin
@pytest.mark.parametrize("precision", [F64, MIXED])
def test_far_from_the_origin(precision):
    """(1000.3, -2000.7, 500.1): the outward-rounded float boxes around double records, through the update path"""
    sd = base_scene(OFFSET)
    new = {GRID: smooth(sd.meshes[GRID].positions - OFFSET) + OFFSET, SOUP: crumpled(sd.meshes[SOUP].positions)}
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(with_arrays(sd, new), precision=precision, builder=DEV)
    try:
        a.set_mesh_vertices(new)
        same_scene(a, b, precision, scene_rays(8192, 4, OFFSET, tmin=1e-7 if precision == F64 else 1e-3))
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 8. full-width nodes
@pytest.mark.parametrize("precision", PRECISIONS)
def test_wide_scenes_stay_wide_and_mixed_scales_become_wide(precision, monkeypatch):
    monkeypatch.delenv("TAKE_HIP_NODES", raising=False)  # the test chooses the node format itself
    sd = base_scene()
    rays = scene_rays(8192, 6, tmin=tmin_of(precision))
    pos = smooth(sd.meshes[GRID].positions)
    a = scene_with_node_format("wide", sd, precision=precision, builder=DEV)
    b = scene_with_node_format("wide", with_arrays(sd, {GRID: pos}), precision=precision, builder=DEV)
    try:
        a.set_mesh_vertices({GRID: pos})
        assert all(a.debug_tree(side)["node_format"] == 0 for side in sides_of(precision))
        same_scene(a, b, precision, rays)
    finally:
        a.close(), b.close()
    # the soup shrunk to 1e-5 of its size: a 15-bit grid over the scene is far too coarse for a third of the leaves
    c = sd.meshes[SOUP].positions.mean(axis=0)
    tiny = c + 1e-5 * (sd.meshes[SOUP].positions - c)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(with_arrays(sd, {SOUP: tiny}), precision=precision, builder=DEV)
    o = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        assert all(a.debug_tree(side)["node_format"] == 1 for side in sides_of(precision))
        assert all(b.debug_tree(side)["node_format"] == 0 for side in sides_of(precision))  # the fresh create's decision
        a.set_mesh_vertices({SOUP: tiny})
        same_scene(a, b, precision, rays)
        a.set_mesh_vertices({SOUP: sd.meshes[SOUP].positions})  # ... and back to compressed nodes
        assert all(a.debug_tree(side)["node_format"] == 1 for side in sides_of(precision))
        same_scene(a, o, precision, rays)
    finally:
        a.close(), b.close(), o.close()


# ------------------------------------------------------------------ 9. refusals leave the scene unchanged
def refused(sc, updates, starts=None, raw=None):
    """raw: (mesh, flags, positions, normals) tuples straight into the C call — what the dict of capi cannot express"""
    with pytest.raises(capi.TakeError) as e:
        if raw is None:
            sc.set_mesh_vertices(updates)
        else:
            recs = (D.TakeMeshUpdate * max(len(raw), 1))()
            for k, (mesh, flags, pos, nrm) in enumerate(raw):
                recs[k].mesh, recs[k].flags = mesh, flags
                recs[k].positions, recs[k].normals = (None if pos is None else pos.ctypes.data), (None if nrm is None else nrm.ctypes.data)
            capi._check(capi.lib().take_hip_scene_set_mesh_vertices(sc.h, recs if updates is None else None, len(raw)))
    assert e.value.code == D.TAKE_E_INVALID
    msg = str(e.value).split(": ", 1)[1]
    assert msg
    if starts:
        assert msg.startswith(starts), msg
    return msg


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_scene_unchanged(precision, monkeypatch):
    sd = base_scene()
    rays = abi(scene_rays(4096, 8, tmin=tmin_of(precision)), precision)
    grid, soup = sd.meshes[GRID].positions, sd.meshes[SOUP].positions
    good = smooth(grid)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        before = snapshot(a, precision, rays)
        refused(a, {})  # n_updates = 0
        refused(a, "null", raw=[(0, 0, good, None)])  # updates = NULL
        assert "out of range" in refused(a, {2: good})
        assert "out of range" in refused(a, {-1: good})
        assert "more than once" in refused(a, None, raw=[(GRID, 0, good, None), (SOUP, 0, soup, None), (GRID, 0, grid, None)])
        assert "positions" in refused(a, None, raw=[(SOUP, 0, None, None)])
        assert "without vertex normals" in refused(a, {SOUP: (soup, soup)})
        assert "flag" in refused(a, None, raw=[(GRID, 6, good, None)])
        assert unchanged(a, precision, rays, before)
        nan = good.copy()
        face = sd.meshes[GRID].indices[100]
        nan[face[1], 2] = np.nan
        nan[sd.meshes[GRID].indices[900][0], 0] = np.inf
        bad_vertex = min(int(face[1]), int(sd.meshes[GRID].indices[900][0]))
        msg = refused(a, {SOUP: smooth(soup), GRID: nan})
        assert f"mesh {GRID}" in msg and f"vertex {bad_vertex}" in msg, msg
        assert unchanged(a, precision, rays, before)
        a.set_mesh_vertices({GRID: good})  # ... and the scene still takes an update
        assert not unchanged(a, precision, rays, before)
    finally:
        a.close()
    # what the path does not support
    two_level = small(20, 100, 16)
    few = SceneData(width=16, height=16, lookfrom=(0.0, 0.0, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0, background=(0.3, 0.3, 0.3))
    few.add_mesh(*scenes._quad((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))[:2], few.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7)))
    monkeypatch.setenv("TAKE_HIP_NODES", "q8")
    q8 = capi.Scene(sd, precision=precision, builder=HOST)
    monkeypatch.delenv("TAKE_HIP_NODES")
    cases = [(capi.Scene(two_level, precision=precision, builder=DEV), two_level.meshes[0].positions),
             (capi.Scene(two_level, precision=precision, flatten_instances=True), two_level.meshes[0].positions),
             (q8, good),
             (capi.Scene(few, precision=precision, builder=HOST, max_leaf_size=4), 0.5 * few.meshes[0].positions)]  # one leaf
    for k, (sc, pos) in enumerate(cases):  # images, hits and debug_tree, as above
        try:
            before = snapshot(sc, precision, rays)
            refused(sc, {0: pos}, starts="unsupported")
            assert unchanged(sc, precision, rays, before), k
        finally:
            sc.close()


# ------------------------------------------------------------------ 10. progressive rendering
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_update_ends_a_progressive_sequence(precision):
    import torch

    sd = base_scene()
    pos = smooth(sd.meshes[GRID].positions)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(with_arrays(sd, {GRID: pos}), precision=precision, builder=DEV)
    try:
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4, restart=True) == 2
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4) == 4
        a.set_mesh_vertices({GRID: pos})
        assert capi.lib().take_hip_accumulated_samples(a.h) == 0
        with pytest.raises(capi.TakeError) as e:
            a.render_accumulate(buf.data_ptr(), 3, 6, seed=4)
        assert e.value.code == D.TAKE_E_INVALID and "restart" in str(e.value)
        assert a.render_accumulate(buf.data_ptr(), 3, 6, seed=4, restart=True) == 3
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), b.render(spp=3, max_depth=6, seed=4))
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 11. one timing
@pytest.mark.parametrize("precision", [F32, MIXED])
def test_updating_a_million_triangles_is_faster_than_creating_them(precision):
    """median of three updates against median of three fresh device-built creates from host arrays, in a warm process.
    A create does every step of an update and validation, the tables and the upload of all arrays on top: only the
    inequality is asserted."""
    sd = scenes.soup_scene(1_000_000, 64, 64, 1)
    soup = len(sd.meshes) - 1
    old = sd.meshes[soup].positions
    moved = [np.ascontiguousarray(old + 0.01 * np.sin(40.0 * old[:, [2, 0, 1]] + k)) for k in range(3)]
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        t_update, t_create = [], []
        for pos in moved:
            t0 = time.perf_counter()
            a.set_mesh_vertices({soup: pos})
            t_update.append(time.perf_counter() - t0)
        fresh = with_arrays(sd, {soup: moved[-1]})
        image = None
        for _ in range(3):
            t0 = time.perf_counter()
            b = capi.Scene(fresh, precision=precision, builder=DEV)
            t_create.append(time.perf_counter() - t0)
            try:
                if image is None:
                    assert b.stats()["n_nodes"] == a.stats()["n_nodes"]
                    image = b.render(spp=1, max_depth=4, seed=4)
            finally:
                b.close()
        assert np.array_equal(image, a.render(spp=1, max_depth=4, seed=4))
        update, create = float(np.median(t_update)), float(np.median(t_create))
        print(f"\n1M-triangle soup, {'f32' if precision == F32 else 'mixed'}: set_mesh_vertices {1e3 * update:.1f} ms "
              f"(of {[round(1e3 * t, 1) for t in t_update]}), fresh device-built scene_create {1e3 * create:.1f} ms "
              f"(of {[round(1e3 * t, 1) for t in t_create]}): {create / update:.2f}x")
        assert update < create, (t_update, t_create)
    finally:
        a.close()

"""Moving the vertices of meshes of a resident TWO-LEVEL scene: take_hip_scene_update_meshes (k_update_proto_prims, the
prototype's tree rebuilt, the top level rebuilt under the scene's current transforms, k_retarget_placements —
take_amd/csrc/tk_build_gpu.h, tk_build.hip: update_two_level_meshes_device).  The yardstick is always a FRESH capi.Scene
built by the device LBVH builder from the description with the new arrays and the scene's current transforms: hit
tables, occlusion and images bit for bit, the moved prototypes' records byte for byte, and the structural validator
(tests/tree_check.py) clean on every resident side."""
import time

import numpy as np
import pytest

import tree_check as T
from take_amd import capi
from take_amd import cdefs as D
from test_gpu_device_build_instanced import (OFFSET, abi, bent_grid, built_by, everything_scene, render, same_hits, scene_rays,
                                             scene_with_node_format, two_big_prototypes)
from test_gpu_mesh_update import base_scene, same_trees, sides_of, smooth, snapshot, unchanged, with_arrays
from test_gpu_repose import drawn, original, posed, same_everything, tmin_of
from test_instancing import small

pytestmark = pytest.mark.gpu
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]
FLOOR, LAMP, BOTH, SOUP, GRID4, GRID = 0, 1, 2, 3, 4, 5  # the meshes of scene()


def scene(offset=(0.0, 0.0, 0.0)):
    """everything_scene() and a prototype of bent_grid(27) — 1458 faces with normals and uvs: no multiple of 64 or 256,
    the last block and the last wave of a launch over its faces are partial — placed twice, FIRST: it is prototype 0,
    and every other prototype's nodes lie behind its tree's"""
    sd = everything_scene(offset)
    pos, idx, nrm, uv = bent_grid(27)
    grid = sd.add_prototype(pos, idx, 3, normals=nrm, uvs=uv)
    assert grid == GRID and idx.shape[0] == 1458 and sd.meshes[BOTH].indices.shape[0] == 400 and BOTH in sd.instance_mesh
    off = np.asarray(offset, np.float64)
    for k, (t, s) in enumerate((((-0.5, 0.5, 0.2), 0.8), ((0.45, -0.2, 0.6), 0.6))):
        c, sn = np.cos(0.7 + k), np.sin(0.7 + k)
        lin = s * np.array([[c, -sn, 0.0], [sn, c, 0.2], [0.1, 0.0, 1.0]])
        sd.instance_mesh.insert(k, grid), sd.instance_material.insert(k, -1 if k else 2)
        sd.instance_xform.insert(k, np.concatenate([lin, (off + t)[:, None]], axis=1))
    assert proto_meshes(sd) == [GRID, SOUP, GRID4, BOTH]
    return sd


def proto_meshes(sd):
    """the prototypes in the library's order: first use by the placements"""
    return list(dict.fromkeys(sd.instance_mesh))


def proto_spans(sd):
    """{mesh: (first record, records)} of the prototypes' records behind the shapes'"""
    out, at = {}, sd.n_shapes
    for m in proto_meshes(sd):
        out[m] = (at, sd.meshes[m].indices.shape[0])
        at += out[m][1]
    return out


def proto_node_counts(tree):
    """nodes per prototype tree, in node order, from the placements' roots"""
    roots = np.unique(tree["inst_trace"]["root_child"])
    assert (roots >= 0).all()
    return np.diff(np.append(roots, tree["n_nodes"]))


def half_shrunk(pos, factor=0.1):
    """the vertices with x < 0 shrunk about their centroid: the prototype's bounds stay, the Morton codes do not"""
    out = pos.copy()
    sel = pos[:, 0] < 0
    c = pos[sel].mean(axis=0)
    out[sel] = c + factor * (pos[sel] - c)
    return out


def equals_fresh(a, sd, arrays, x, precision, rays, moved, device_built, b=None, **kw):
    """a against a fresh device-built scene of sd with `arrays` and transforms x: same_everything, n_prims, the
    prototypes' records (all of them when the device built a; the moved ones' spans otherwise), check_tree on a"""
    own = b is None
    if own:
        b = capi.Scene(posed(with_arrays(sd, arrays), x), precision=precision, builder=DEV, **kw)
    try:
        same_everything(a, b, precision, rays)
        assert a.stats()["n_prims"] == b.stats()["n_prims"]
        spans = proto_spans(sd)
        for side in sides_of(precision):
            ta, tb = a.debug_tree(side), b.debug_tree(side)
            assert ta["n_prims"] == tb["n_prims"] == sd.n_shapes + sum(c for _, c in spans.values())
            if device_built:
                assert np.array_equal(ta["prims"][sd.n_shapes:], tb["prims"][sd.n_shapes:]), side
            for m in moved:
                first, count = spans[m]
                assert np.array_equal(ta["prims"][first:first + count], tb["prims"][first:first + count]), (side, m)
            primary = side == (F32 if precision == F32 else F64)  # take_hip_scene_stats reports the primary side
            r = T.check_tree(ta, n_shapes=sd.n_shapes, xforms=np.asarray(x, np.float64), expected_depth=a.stats()["depth"] if primary else None)
            assert T.total_errors(r) == 0, (side, r["errors"], r["where"])
    finally:
        if own:
            b.close()


# ------------------------------------------------------------------ 1. prototype 0 moves; the others' nodes shift
@pytest.mark.parametrize("builder", [DEV, HOST])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_prototype_0_deformed_equals_a_fresh_scene(precision, builder):
    """a smooth deformation of prototype 0, then half of it shrunk to a tenth: its tree's node count changes, so the
    nodes of every later prototype and the roots of their placements really shift.  A is built by the device in one run
    and by the host SAH in the other: build_info keeps saying so (the untouched trees are still the host's)."""
    sd = scene()
    x = original(sd)
    rays = scene_rays(8192, 3, tmin=tmin_of(precision))
    a = capi.Scene(sd, precision=precision, builder=builder)
    try:
        assert a.build_info() == built_by(precision, builder)
        counts = []
        for deform in (smooth, half_shrunk):
            pos = deform(sd.meshes[GRID].positions)
            a.update_meshes({GRID: pos})
            assert a.build_info() == built_by(precision, builder)
            tree = a.debug_tree()
            counts.append(int(proto_node_counts(tree)[0]))
            assert a.stats()["n_nodes"] == tree["n_nodes"]
            equals_fresh(a, sd, {GRID: pos}, x, precision, rays, [GRID], builder == DEV)
        print(f"\nnodes of prototype 0: smooth {counts[0]}, half shrunk {counts[1]}")
        assert counts[0] != counts[1], counts
    finally:
        a.close()


# ------------------------------------------------------------------ 2. several prototypes in one call; device pointers; normals
@pytest.mark.parametrize("precision", PRECISIONS)
def test_several_prototypes_device_pointers_and_normals(precision):
    import torch

    sd = scene()
    x = original(sd)
    rays = scene_rays(8192, 4, tmin=tmin_of(precision))
    grid, soup = sd.meshes[GRID], sd.meshes[SOUP]
    nrm = grid.normals * [-1.0, 1.0, 1.0] + [0.0, 0.0, 0.4]
    new = {GRID: (smooth(grid.positions), nrm), SOUP: half_shrunk(soup.positions, 0.5)}
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        a.update_meshes({GRID: (new[GRID][0], None)})  # normals None: the old ones stay
        kept = render(a, 0, spp=4, max_depth=6, seed=5)
        equals_fresh(a, sd, {GRID: new[GRID][0]}, x, precision, rays, [GRID], True)
        on_device = tuple(torch.from_numpy(np.ascontiguousarray(v)).to("cuda") for v in new[GRID])
        a.update_meshes({SOUP: new[SOUP], GRID: on_device})  # host arrays for one mesh, device arrays for the other
        equals_fresh(a, sd, new, x, precision, rays, [GRID, SOUP], True)
        assert not np.array_equal(kept, render(a, 0, spp=4, max_depth=6, seed=5))
        before = snapshot(a, precision, abi(rays, precision))
        with pytest.raises(capi.TakeError) as e:
            a.update_meshes({SOUP: (soup.positions, soup.positions)})
        assert e.value.code == D.TAKE_E_INVALID and "without vertex normals" in str(e.value)
        assert unchanged(a, precision, abi(rays, precision), before)
    finally:
        a.close()


# ------------------------------------------------------------------ 3. both roles, an ordinary mesh, the emissive quad
@pytest.mark.parametrize("precision", PRECISIONS)
def test_both_roles_an_ordinary_mesh_and_the_light(precision):
    """`both` is a mesh of the shape arrays AND a prototype: both kinds of records change.  The floor is ordinary only.
    The lamp carries the area lights: their records and the power tables (integrator 3 picks by them) are a fresh scene's."""
    sd = scene()
    x = original(sd)
    rays = scene_rays(8192, 5, tmin=tmin_of(precision))
    lamp = sd.meshes[LAMP].positions
    centre = lamp.mean(axis=0)
    new = {BOTH: smooth(sd.meshes[BOTH].positions), FLOOR: sd.meshes[FLOOR].positions + (0.0, 0.1, 0.0)}
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        i0 = render(a, 0, spp=4, max_depth=6, seed=5)
        a.update_meshes(new)
        assert not np.array_equal(i0, render(a, 0, spp=4, max_depth=6, seed=5))
        equals_fresh(a, sd, new, x, precision, rays, [BOTH], True)
        new[LAMP] = centre + 2.0 * (lamp - centre) - (0.0, 0.1, 0.0)
        a.update_meshes({LAMP: new[LAMP]})
        b = capi.Scene(posed(with_arrays(sd, new), x), precision=precision, builder=DEV)
        try:
            equals_fresh(a, sd, new, x, precision, rays, [], True, b=b)
            if precision != MIXED:  # (a mixed scene renders integrator 0 only)
                ia = a.render(spp=4, max_depth=6, seed=2, integrator=3)
                assert np.array_equal(ia, b.render(spp=4, max_depth=6, seed=2, integrator=3))
                assert np.isfinite(ia).all() and ia.mean() > 0
        finally:
            b.close()
    finally:
        a.close()


# ------------------------------------------------------------------ 4. order with the re-pose
@pytest.mark.parametrize("builder", [DEV, HOST])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_with_the_re_pose(precision, builder):
    """re-pose, then update: the top level must be rebuilt under the NEW transforms (host and device entry of the
    re-pose once each); update, then re-pose: the re-pose must find the prototypes where the update put them"""
    import torch

    sd = scene()
    rays = scene_rays(8192, 6, tmin=tmin_of(precision))
    arrays = {}
    a = capi.Scene(sd, precision=precision, builder=builder)
    try:
        for k, (mesh, deform) in enumerate(((GRID, half_shrunk), (SOUP, smooth))):
            x = drawn(sd, 20 + k, 0.7)
            a.set_instance_transforms(torch.from_numpy(x).to("cuda") if k else x)
            arrays[mesh] = deform(sd.meshes[mesh].positions)
            a.update_meshes({mesh: arrays[mesh]})
            equals_fresh(a, sd, arrays, x, precision, rays, list(arrays), builder == DEV)
        y = drawn(sd, 31, 0.4)
        a.set_instance_transforms(y)
        equals_fresh(a, sd, arrays, y, precision, rays, list(arrays), builder == DEV)
        arrays[GRID] = smooth(sd.meshes[GRID].positions)  # ... and a further update on that layout
        a.update_meshes({GRID: arrays[GRID]})
        equals_fresh(a, sd, arrays, y, precision, rays, list(arrays), builder == DEV)
    finally:
        a.close()


# ------------------------------------------------------------------ 5. round trip and repetition
@pytest.mark.parametrize("precision", PRECISIONS)
def test_round_trip_and_repetition(precision):
    sd = scene()
    rays = abi(scene_rays(8192, 3, tmin=tmin_of(precision)), precision)
    pos = smooth(sd.meshes[GRID].positions)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        h0 = a.trace_closest(rays) if precision != MIXED else None
        i0 = render(a, 0, spp=4, max_depth=6, seed=5)
        a.update_meshes({GRID: pos, BOTH: smooth(sd.meshes[BOTH].positions)})
        once = snapshot(a, precision, rays)
        assert not np.array_equal(i0, render(a, 0, spp=4, max_depth=6, seed=5))
        a.update_meshes({GRID: pos})  # the same again: nothing changes
        assert unchanged(a, precision, rays, once)
        a.update_meshes({GRID: sd.meshes[GRID].positions, BOTH: sd.meshes[BOTH].positions})
        assert np.array_equal(i0, render(a, 0, spp=4, max_depth=6, seed=5))
        if h0 is not None:
            h2 = a.trace_closest(rays)
            for f in ("shape_id", "t", "u", "v"):
                assert np.array_equal(h0[f], h2[f]), f
    finally:
        a.close()


# ------------------------------------------------------------------ 6. the scene keeps its node format
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_scene_keeps_its_node_format(precision, monkeypatch):
    monkeypatch.delenv("TAKE_HIP_NODES", raising=False)  # the test chooses the node format itself
    sd = scene()
    x = original(sd)
    rays = scene_rays(8192, 6, tmin=tmin_of(precision))
    pos = smooth(sd.meshes[GRID].positions)
    a = scene_with_node_format("wide", sd, precision=precision, builder=DEV)
    try:
        a.update_meshes({GRID: pos})
        assert all(a.debug_tree(side)["node_format"] == 0 for side in sides_of(precision))  # (mixed: the widened double nodes too)
        equals_fresh(a, sd, {GRID: pos}, x, precision, rays, [GRID], True)
    finally:
        a.close()
    # half of the prototype shrunk to 1e-5 about a point: a 15-bit grid over its bounds is far too coarse for those leaves
    tiny = half_shrunk(sd.meshes[GRID].positions, 1e-5)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(posed(with_arrays(sd, {GRID: tiny}), x), precision=precision, builder=DEV)
    try:
        assert all(a.debug_tree(side)["node_format"] == 1 for side in sides_of(precision))
        assert all(b.debug_tree(side)["node_format"] == 0 for side in sides_of(precision))  # the fresh create's decision
        a.update_meshes({GRID: tiny})
        assert all(a.debug_tree(side)["node_format"] == 1 for side in sides_of(precision))  # ... is not the update's
        equals_fresh(a, sd, {GRID: tiny}, x, precision, rays, [GRID], True, b=b)
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 7. the tie rule; far from the origin
@pytest.mark.parametrize("precision", [F32, F64])
def test_coincident_placements_still_tie_on_the_larger_instance_id(precision):
    sd = scene()
    n = len(sd.instance_mesh)
    assert sd.instance_mesh[n - 1] == sd.instance_mesh[n - 2] == SOUP and np.array_equal(sd.instance_xform[n - 1], sd.instance_xform[n - 2])
    faces = sd.meshes[SOUP].indices.shape[0]
    total = sd.n_shapes + sum(sd.meshes[m].indices.shape[0] for m in sd.instance_mesh)
    first_of_last, first_of_prev = total - faces, total - 2 * faces
    pos = smooth(sd.meshes[SOUP].positions)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(with_arrays(sd, {SOUP: pos}), precision=precision, builder=DEV)
    try:
        a.update_meshes({SOUP: pos})
        ids = same_hits(a, b, abi(scene_rays(20000, 9), precision))["shape_id"]
        assert (ids >= first_of_last).sum() > 20 and not ((ids >= first_of_prev) & (ids < first_of_last)).any()
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_prototype_moved_far_from_the_origin(precision):
    """the prototype's vertices go to OFFSET in object space, its placements' translations take them back: the records
    and the prototype's boxes are far from the origin, the hits still a fresh scene's"""
    sd = scene()
    pos = sd.meshes[GRID].positions + OFFSET
    x = original(sd)
    for i, m in enumerate(sd.instance_mesh):
        if m == GRID:
            x[i, :, 3] -= x[i, :, :3] @ OFFSET
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        a.set_instance_transforms(x)
        a.update_meshes({GRID: pos})
        equals_fresh(a, sd, {GRID: pos}, x, precision, scene_rays(8192, 4, tmin=1e-7 if precision == F64 else 1e-3), [GRID], True)
    finally:
        a.close()


# ------------------------------------------------------------------ 8. refusals leave the scene unchanged
def refused(sc, updates, starts=None, raw=None):
    """raw: (mesh, flags, positions, normals) tuples straight into the C call — what the dict of capi cannot express"""
    with pytest.raises(capi.TakeError) as e:
        if raw is None:
            sc.update_meshes(updates)
        else:
            recs = (D.TakeMeshUpdate * max(len(raw), 1))()
            for k, (mesh, flags, pos, nrm) in enumerate(raw):
                recs[k].mesh, recs[k].flags = mesh, flags
                recs[k].positions, recs[k].normals = (None if pos is None else pos.ctypes.data), (None if nrm is None else nrm.ctypes.data)
            capi._check(capi.lib().take_hip_scene_update_meshes(sc.h, recs, len(raw)))
    assert e.value.code == D.TAKE_E_INVALID
    msg = str(e.value).split(": ", 1)[1]
    assert msg
    if starts:
        assert msg.startswith(starts), msg
    return msg


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_scene_unchanged(precision, monkeypatch):
    monkeypatch.delenv("TAKE_HIP_NODES", raising=False)
    monkeypatch.delenv("TAKE_HIP_BRAID", raising=False)
    sd = scene()
    rays = abi(scene_rays(4096, 8, tmin=tmin_of(precision)), precision)
    grid, soup = sd.meshes[GRID].positions, sd.meshes[SOUP].positions
    good = smooth(grid)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        before = snapshot(a, precision, rays)
        nan = good.copy()
        face = sd.meshes[GRID].indices[100]
        nan[face[1], 2] = np.nan
        nan[sd.meshes[GRID].indices[900][0], 0] = np.inf
        bad_vertex = min(int(face[1]), int(sd.meshes[GRID].indices[900][0]))
        msg = refused(a, {SOUP: smooth(soup), GRID: nan})  # in a prototype
        assert f"mesh {GRID}" in msg and f"vertex {bad_vertex}" in msg, msg
        assert unchanged(a, precision, rays, before)
        both = sd.meshes[BOTH].positions.copy()
        both[sd.meshes[BOTH].indices[7][2], 1] = np.inf  # in a mesh of both roles
        msg = refused(a, {BOTH: both})
        assert f"mesh {BOTH}" in msg and f"vertex {int(sd.meshes[BOTH].indices[7][2])}" in msg, msg
        assert "more than once" in refused(a, None, raw=[(GRID, 0, good, None), (SOUP, 0, soup, None), (GRID, 0, grid, None)])
        assert "out of range" in refused(a, {len(sd.meshes): good})
        assert unchanged(a, precision, rays, before)
        a.update_meshes({GRID: good})  # ... and the scene still takes an update
        assert not unchanged(a, precision, rays, before)
    finally:
        a.close()
    # what the path does not support
    two_level = small(20, 300, 16)
    monkeypatch.setenv("TAKE_HIP_BRAID", "4")
    braided = capi.Scene(two_level, precision=precision, builder=HOST)
    monkeypatch.delenv("TAKE_HIP_BRAID")
    monkeypatch.setenv("TAKE_HIP_NODES", "q8")
    q8 = capi.Scene(two_level, precision=precision, builder=HOST)
    monkeypatch.delenv("TAKE_HIP_NODES")
    one_face = small(20, 100, 16)
    tri = one_face.add_prototype(np.array([[-0.2, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.3, 0.0]]), np.array([[0, 1, 2]], np.int32), 0)
    one_face.add_instance(tri, np.concatenate([np.eye(3), [[0.0], [0.0], [1.0]]], axis=1))
    cases = [(braided, 0, two_level.meshes[0].positions), (q8, 0, two_level.meshes[0].positions),
             (capi.Scene(one_face, precision=precision, builder=HOST), tri, 0.5 * one_face.meshes[tri].positions)]
    for k, (sc, mesh, pos) in enumerate(cases):
        try:
            before = snapshot(sc, precision, rays)
            refused(sc, {mesh: pos}, starts="unsupported")
            assert unchanged(sc, precision, rays, before), k
            if k == 2:  # the one-leaf prototype survives an update of another prototype untouched
                proto = one_face.instance_mesh[0]
                moved = smooth(one_face.meshes[proto].positions)
                sc.update_meshes({proto: moved})
                # (the fresh scene falls back to the host builder, as this one did: results, not record orders, are compared)
                equals_fresh(sc, one_face, {proto: moved}, original(one_face), precision, scene_rays(4096, 8, tmin=tmin_of(precision)), [], False)
        finally:
            sc.close()


# ------------------------------------------------------------------ 9. a scene without placements; the old symbol
@pytest.mark.parametrize("precision", PRECISIONS)
def test_without_placements_it_is_set_mesh_vertices(precision):
    sd = base_scene()
    new = {0: (smooth(sd.meshes[0].positions), sd.meshes[0].normals[::-1].copy()), 1: half_shrunk(sd.meshes[1].positions)}
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    try:
        a.update_meshes(new)
        b.set_mesh_vertices(new)
        same_trees(a, b, precision)
        assert a.build_info() == b.build_info() and a.stats() == b.stats()
    finally:
        a.close(), b.close()
    flat = capi.Scene(small(20, 100, 16), precision=precision, flatten_instances=True)
    two = capi.Scene(small(20, 100, 16), precision=precision, builder=DEV)
    try:
        refused(flat, {0: small(20, 100, 16).meshes[0].positions}, starts="unsupported")
        with pytest.raises(capi.TakeError) as e:
            two.set_mesh_vertices({0: small(20, 100, 16).meshes[0].positions})  # the old symbol keeps refusing
        assert e.value.code == D.TAKE_E_INVALID and str(e.value).split(": ", 1)[1].startswith("unsupported")
    finally:
        flat.close(), two.close()


# ------------------------------------------------------------------ 10. progressive rendering
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_update_ends_a_progressive_sequence(precision):
    import torch

    sd = scene()
    pos = smooth(sd.meshes[GRID].positions)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(with_arrays(sd, {GRID: pos}), precision=precision, builder=DEV)
    try:
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4, restart=True) == 2
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4) == 4
        a.update_meshes({GRID: pos})
        assert capi.lib().take_hip_accumulated_samples(a.h) == 0
        with pytest.raises(capi.TakeError) as e:
            a.render_accumulate(buf.data_ptr(), 3, 6, seed=4)
        assert e.value.code == D.TAKE_E_INVALID and "restart" in str(e.value)
        assert a.render_accumulate(buf.data_ptr(), 3, 6, seed=4, restart=True) == 3
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), b.render(spp=3, max_depth=6, seed=4))
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 11. size and time
@pytest.mark.parametrize("precision", [F32, MIXED])
def test_updating_one_of_two_500k_triangle_prototypes_is_faster_than_creating_the_scene(precision):
    """median of three updates of ONE prototype against median of three fresh device-built creates of the same
    description, in a warm process.  An update does a strict subset of a create's work — one prototype pass instead of
    two, no validation, no tables, one mesh uploaded: only the inequality is asserted."""
    sd = two_big_prototypes(500_000, 64, 96)
    mesh = sd.instance_mesh[1]
    old = sd.meshes[mesh].positions
    moved = [np.ascontiguousarray(old + 0.004 * np.sin(60.0 * old[:, [2, 0, 1]] + k)) for k in range(3)]
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        t_update, t_create = [], []
        for pos in moved:
            t0 = time.perf_counter()
            a.update_meshes({mesh: pos})
            t_update.append(time.perf_counter() - t0)
        fresh = with_arrays(sd, {mesh: moved[-1]})
        image = None
        for _ in range(3):
            t0 = time.perf_counter()
            b = capi.Scene(fresh, precision=precision, builder=DEV)
            t_create.append(time.perf_counter() - t0)
            try:
                if image is None:
                    image = b.render(spp=1, max_depth=4, seed=4)
            finally:
                b.close()
        assert np.array_equal(image, a.render(spp=1, max_depth=4, seed=4))
        update, create = float(np.median(t_update)), float(np.median(t_create))
        print(f"\n2 x 500k triangles x 64 placements, {'f32' if precision == F32 else 'mixed'}: update_meshes of one prototype {1e3 * update:.1f} ms "
              f"(of {[round(1e3 * t, 1) for t in t_update]}), fresh device-built scene_create {1e3 * create:.1f} ms "
              f"(of {[round(1e3 * t, 1) for t in t_create]}): {create / update:.2f}x")
        assert update < create, (t_update, t_create)
    finally:
        a.close()

"""Loop subdivision on the device: take_hip_subdiv_refine*, take_hip_scene_subdivide_meshes (k_subdiv_even, k_subdiv_odd,
k_subdiv_face_normals, k_subdiv_vertex_normals — take_amd/csrc/tk_subdiv.h, tk_subdiv.hip).  Two
yardsticks: the host build of the same bodies (tests/subdiv_host, itself held to tests/subdiv_ref.py by
tests/test_subdiv_cpu.py) for the refined arrays, bit for bit; and for the scene-bound call the scene after refine() to
the host + update_meshes(host arrays), and a FRESH device-built scene from the refined arrays: debug_tree records,
stats, hit tables and render bytes."""
import functools
import types

import numpy as np
import pytest
import torch

import subdiv_ref
from take_amd import capi
from take_amd import cdefs as D
from take_amd.scene import Light, SceneData
from test_gpu_device_build_instanced import abi, scene_rays
from test_gpu_mesh_update import same_scene, snapshot, unchanged, with_arrays
from test_gpu_repose import same_everything, tmin_of
from test_gpu_skin import strip_pose, strip_rig
from test_subdiv_cpu import differing, host_refine

pytestmark = pytest.mark.gpu
DEV = D.TAKE_BUILDER_DEVICE_LBVH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]
CAGE, OTHER = 0, 1  # the meshes of cage_scene


@functools.lru_cache(maxsize=None)
def reference():
    """[(name, levels, cage positions, indices, uvs, host positions, host normals, host indices, host uvs)]: computed
    once, shared, never written"""
    out = []
    for name, pos, idx, uv, levels in subdiv_ref.cases():
        for L in levels:
            p, n, i, u = host_refine(pos, idx, L, uvs=uv)  # (the launches' own grids: what the device runs)
            p.setflags(write=False), n.setflags(write=False)
            out.append((name, L, pos, idx, uv, p, n, i, u))
    return out


def wobbled(pos, seed):
    """another cage over the same topology"""
    return pos + 0.07 * np.sin(4.0 * pos[:, [1, 2, 0]] + seed)


# ------------------------------------------------------------------ 1. the refined arrays
@pytest.mark.parametrize("source", ["host", "device", "other-stream"])
def test_refine_equals_the_host_build_bit_for_bit(source):
    """over the CPU case list, every level: the cage from host memory / from a device tensor / from a device tensor
    written on another stream just before the call"""
    side = torch.cuda.Stream()
    assert len(reference()) == sum(len(c[4]) for c in subdiv_ref.cases()) >= 23
    for name, L, pos, idx, uv, want_p, want_n, want_idx, want_uv in reference():
        nv = want_p.shape[0]
        with capi.Subdiv(idx, pos.shape[0], L, uvs=uv) as sub:
            info = sub.info()
            assert (info["cage_vertices"], info["n_vertices"], info["n_faces"], info["levels"]) == (pos.shape[0], nv, want_idx.shape[0], L), name
            got_idx, got_uv = sub.topology()
            assert np.array_equal(got_idx, want_idx) and (got_uv is None) == (uv is None), name
            if uv is not None:
                assert differing(got_uv, want_uv) == 0, name
            out_p = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device="cuda")  # (a guard row behind each output)
            out_n = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device="cuda")
            if source == "host":
                got_p, got_n = sub.refine(pos)
                sub.refine_device(out_p, out_n, pos)
            else:
                stream = side if source == "other-stream" else torch.cuda.current_stream()
                with torch.cuda.stream(stream):
                    if source == "other-stream":  # (work in front of the write: a call that does not wait reads zeros)
                        busy = torch.ones((1024, 1024), device="cuda")
                        for _ in range(8):
                            busy = busy @ busy * 1e-3
                    cage = torch.zeros(pos.shape, dtype=torch.float64, device="cuda").copy_(torch.from_numpy(pos), non_blocking=True)
                    got_p, got_n = sub.refine(cage)
                    sub.refine_device(out_p, out_n, cage, stream=stream.cuda_stream if source == "other-stream" else None)
            torch.cuda.synchronize()
            assert differing(got_p, want_p) == 0, f"{name} L{L}: positions"
            assert differing(got_n, want_n) == 0, f"{name} L{L}: normals"
            assert differing(out_p[:nv].cpu().numpy(), want_p) == 0 and (out_p[nv] == -7.0).all(), f"{name} L{L}: positions, device"
            assert differing(out_n[:nv].cpu().numpy(), want_n) == 0 and (out_n[nv] == -7.0).all(), f"{name} L{L}: normals, device"


def test_normals_can_be_left_out_and_the_buffers_are_reused_not_grown():
    name, L, pos, idx, uv, want_p, want_n, _, _ = next(r for r in reference() if r[:2] == ("strip33", 3))
    nv = want_p.shape[0]
    with capi.Subdiv(idx, pos.shape[0], L) as sub:
        created = sub.info()["device_bytes"]
        assert created > 8 * 3 * nv * 2
        out_p = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device="cuda")
        sub.refine_device(out_p, None, pos)
        assert differing(out_p[:nv].cpu().numpy(), want_p) == 0 and (out_p[nv] == -7.0).all()
        assert differing(sub.refine(pos, normals=False), want_p) == 0
        other = wobbled(pos, 1.0)
        p, n, _, _ = host_refine(other, idx, L)
        got_p, got_n = sub.refine(other)
        assert differing(got_p, p) == 0 and differing(got_n, n) == 0 and differing(got_p, want_p) > 0
        assert sub.info()["device_bytes"] == created


# ------------------------------------------------------------------ 2. scenes
CAGES = {"octahedron": (3, lambda: subdiv_ref.octahedron()), "strip23": (2, lambda: subdiv_ref.strip(23))}


def cage_of(kind):
    """-> (levels, cage positions, cage indices): the octahedron shrunk into the view"""
    L, make = CAGES[kind]
    pos, idx = make()
    if kind == "octahedron":
        pos = 0.55 * pos * np.array([1.0, 0.8, 1.3])
    return L, pos, idx


def cage_scene(kind, normals=True, two_level=False):
    """mesh 0: the cage of `kind` refined (positions and normals by the host build); mesh 1: a strip of 65 vertices
    without vertex normals that nothing touches; a sphere beside them; a point light.  two_level: mesh 0 is a prototype
    placed three times instead."""
    L, pos, idx = cage_of(kind)
    p, n, i, _ = host_refine(pos, idx, L)
    sd = SceneData(width=16, height=16, lookfrom=(0.0, 0.2, 3.6), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0, background=(0.2, 0.3, 0.4), spp=4,
                   max_depth=6)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7))
    gold = sd.add_material(D.MAT_BLINN_PHONG_MICROFACET, (0.8, 0.7, 0.3), (30.0,))
    if two_level:
        assert sd.add_prototype(p, i, gold, normals=n if normals else None) == CAGE
    else:
        sd.add_mesh(p, i, gold, normals=n if normals else None)
    pos2, idx2 = subdiv_ref.strip(65, -0.9)
    sd.add_mesh(pos2, idx2, grey)
    if two_level:
        for k, (t, s) in enumerate((((0.0, 0.0, 0.0), 1.0), ((0.3, 0.6, -0.5), 0.7), ((-0.4, 0.9, 0.4), 0.5))):
            c, sn = np.cos(0.4 * k), np.sin(0.4 * k)
            sd.add_instance(CAGE, np.concatenate([s * np.array([[c, -sn, 0.0], [sn, c, 0.1], [0.0, 0.0, 1.0]]), np.array(t)[:, None]], axis=1), -1 if k else grey)
    sd.add_sphere((0.0, 0.75, 0.0), 0.25, grey)
    sd.lights.append(Light(0, -1, (12.0, 12.0, 12.0), (0.3, 2.0, 1.5)))
    return sd, L, pos, idx


def refined_arrays(sub, cage, mesh):
    """what update_meshes takes for the mesh: refined positions, and normals when the mesh has them"""
    p, n = sub.refine(cage)
    return (p, n) if mesh.normals is not None else p


@pytest.mark.parametrize("two_level", [False, True], ids=["one-level", "two-level"])
@pytest.mark.parametrize("kind", list(CAGES))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_subdivide_meshes_equals_refine_then_update_equals_a_fresh_scene(precision, kind, two_level):
    sd, L, pos, idx = cage_scene(kind, two_level=two_level)
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    sub = capi.Subdiv(idx, pos.shape[0], L)
    try:
        assert sub.n_vertices == sd.meshes[CAGE].positions.shape[0]
        for seed, device in ((1.0, False), (2.0, True)):
            cage = wobbled(pos, seed)
            a.subdivide_meshes([(CAGE, sub, torch.from_numpy(cage).cuda() if device else cage)])
            arrays = refined_arrays(sub, cage, sd.meshes[CAGE])
            assert isinstance(arrays, tuple) and np.abs(arrays[0] - sd.meshes[CAGE].positions).max() > 0.02
            b.update_meshes({CAGE: arrays})
            same_scene(a, b, precision, rays)
            c = capi.Scene(with_arrays(sd, {CAGE: arrays}), precision=precision, builder=DEV)
            try:
                (same_everything if two_level else same_scene)(a, c, precision, rays)
                assert a.stats()["n_prims"] == c.stats()["n_prims"]
            finally:
                c.close()
    finally:
        a.close(), b.close(), sub.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_mesh_without_vertex_normals_gets_positions_alone(precision):
    sd, L, pos, idx = cage_scene("strip23", normals=False)
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    sub = capi.Subdiv(idx, pos.shape[0], L)
    try:
        cage = wobbled(pos, 3.0)
        a.subdivide_meshes([(CAGE, sub, cage)])
        arrays = refined_arrays(sub, cage, sd.meshes[CAGE])
        assert not isinstance(arrays, tuple)
        b.update_meshes({CAGE: arrays})
        same_scene(a, b, precision, rays)
    finally:
        a.close(), b.close(), sub.close()


# ------------------------------------------------------------------ 3. a rig in front
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_bound_rig_equals_pose_then_refine_then_update(precision):
    sd, L, pos, idx = cage_scene("strip23")
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    sub = capi.Subdiv(idx, pos.shape[0], L)
    rig = strip_rig(types.SimpleNamespace(positions=pos, normals=None), normals=False)
    try:
        X, tw = strip_pose(4)
        a.subdivide_meshes([(CAGE, sub, (rig, X, tw))])
        posed = rig.pose(X, tw)
        assert np.abs(posed - pos).max() > 0.05
        want_p, want_n, _, _ = host_refine(posed, idx, L)
        got_p, got_n = sub.refine(posed)
        assert differing(got_p, want_p) == 0 and differing(got_n, want_n) == 0
        b.update_meshes({CAGE: (got_p, got_n)})
        same_scene(a, b, precision, rays)
        # the same with the pose in device memory
        a.subdivide_meshes([(CAGE, sub, (rig, torch.from_numpy(X).cuda(), torch.from_numpy(tw).cuda()))])
        same_scene(a, b, precision, rays)
    finally:
        a.close(), b.close(), sub.close(), rig.close()


# ------------------------------------------------------------------ 4. tracking
@pytest.mark.parametrize("two_level", [False, True], ids=["one-level", "two-level"])
def test_tracked_motion_planes_equal_those_after_update_meshes(two_level):
    sd, L, pos, idx = cage_scene("strip23", two_level=two_level)
    a, b = capi.Scene(sd, precision=F32), capi.Scene(sd, precision=F32)
    sub = capi.Subdiv(idx, pos.shape[0], L)
    try:
        cage = wobbled(pos, 5.0)
        for sc in (a, b):
            sc.track_vertices()
            sc.mark_frame()
        a.subdivide_meshes([(CAGE, sub, cage)])
        b.update_meshes({CAGE: refined_arrays(sub, cage, sd.meshes[CAGE])})
        assert a.tracking_info() == b.tracking_info() and a.tracking_info()["marked_bytes"] > 0
        pa, pb = a.render_motion(), b.render_motion()
        assert set(pa) == set(pb) and all(np.array_equal(pa[k], pb[k]) for k in pa)
        plain = capi.Scene(sd, precision=F32)  # (without tracking the motion pass does not see the cage move)
        try:
            plain.mark_frame()
            plain.subdivide_meshes([(CAGE, sub, cage)])
            untracked = plain.render_motion()
            assert np.array_equal(untracked["shape_id"], pa["shape_id"]) and np.abs(untracked["prev_xy"] - pa["prev_xy"]).max() > 0.02
        finally:
            plain.close()
    finally:
        a.close(), b.close(), sub.close()


# ------------------------------------------------------------------ 5. failures
def refused(sc, bindings, code=D.TAKE_E_INVALID):
    with pytest.raises(capi.TakeError) as e:
        sc.subdivide_meshes(bindings)
    assert e.value.code == code, str(e.value)
    return str(e.value).split(": ", 1)[1]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_scene_unchanged(precision):
    sd, L, pos, idx = cage_scene("strip23")
    rays = abi(scene_rays(1024, 8, tmin=tmin_of(precision)), precision)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    sub, other, wrong = capi.Subdiv(idx, pos.shape[0], L), capi.Subdiv(subdiv_ref.strip(33)[1], 33, 1), capi.Subdiv(idx, pos.shape[0], L - 1)
    rig = strip_rig(types.SimpleNamespace(positions=pos, normals=None), normals=False)
    short = strip_rig(types.SimpleNamespace(positions=pos[:21], normals=None), normals=False)
    try:
        X, tw = strip_pose(8)
        cage = wobbled(pos, 6.0)
        cage33 = subdiv_ref.strip(33)[0]
        before = snapshot(a, precision, rays)
        assert "n must be positive" in refused(a, [])
        assert "binding 1: mesh index out of range" in refused(a, [(CAGE, sub, cage), (2, other, cage33)])
        assert "binding 0: mesh index out of range" in refused(a, [(-1, sub, cage)])
        msg = refused(a, [(CAGE, wrong, cage)])
        assert "binding 0" in msg and f"{wrong.n_vertices} vertices" in msg and f"mesh {CAGE} has {sub.n_vertices}" in msg, msg
        assert "mesh 0 appears more than once" in refused(a, [(CAGE, sub, cage), (CAGE, other, cage33)])
        assert "bound more than once" in refused(a, [(CAGE, sub, cage), (OTHER, sub, cage)])
        assert "exactly one of cage_positions and rig" in refused(a, [(CAGE, sub, None)])
        assert "joint_xforms is required" in refused(a, [(CAGE, sub, (rig, None, tw))])
        msg = refused(a, [(CAGE, sub, (short, X, tw))])
        assert "binding 0" in msg and "the rig has 21 vertices, the cage has 23" in msg, msg
        bad = cage.copy()
        bad[11, 1] = np.inf  # a cage position that is not finite: the update's own finiteness check names mesh and vertex
        msg = refused(a, [(CAGE, sub, bad)])
        assert f"mesh {CAGE}" in msg and "vertex" in msg and "finite" in msg, msg
        assert unchanged(a, precision, rays, before)
        a.subdivide_meshes([(CAGE, sub, cage)])  # ... and the scene still takes a cage
        assert not unchanged(a, precision, rays, before)
    finally:
        a.close(), sub.close(), other.close(), wrong.close(), rig.close(), short.close()


@pytest.mark.parametrize("precision", [F32, MIXED])
def test_every_allocation_failing_in_turn_leaves_the_scene_as_it_was(precision, monkeypatch):
    sd, L, pos, idx = cage_scene("strip23")
    rays = abi(scene_rays(1024, 8, tmin=tmin_of(precision)), precision)
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    sub = capi.Subdiv(idx, pos.shape[0], L)
    try:
        cage = wobbled(pos, 7.0)
        before = snapshot(a, precision, rays)
        bytes_before = sub.info()["device_bytes"]
        failed = 0
        for nth in range(1, 400):
            monkeypatch.setenv("TAKE_HIP_FAIL_ALLOC", str(nth))
            try:
                a.subdivide_meshes([(CAGE, sub, cage)])
                break
            except capi.TakeError as e:
                assert e.code in (D.TAKE_E_NOMEM, D.TAKE_E_DEVICE), str(e)
                failed += 1
            finally:
                monkeypatch.delenv("TAKE_HIP_FAIL_ALLOC")
            assert unchanged(a, precision, rays, before), nth
        else:
            pytest.fail("the call never ran out of allocations to fail")
        print(f"\n{failed} allocations of the call failed in turn")
        assert failed >= 4 and sub.info()["device_bytes"] == bytes_before
        b.update_meshes({CAGE: refined_arrays(sub, cage, sd.meshes[CAGE])})
        same_scene(a, b, precision, rays if precision == MIXED else scene_rays(1024, 8, tmin=tmin_of(precision)))
    finally:
        a.close(), b.close(), sub.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_subdivision_ends_a_progressive_sequence_and_a_refused_one_does_not(precision):
    sd, L, pos, idx = cage_scene("strip23")
    a = capi.Scene(sd, precision=precision, builder=DEV)
    sub = capi.Subdiv(idx, pos.shape[0], L)
    try:
        cage = wobbled(pos, 9.0)
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4, restart=True) == 2
        bad = cage.copy()
        bad[0, 1] = np.nan
        refused(a, [(CAGE, sub, bad)])
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4) == 4, "a refused call leaves the sequence running"
        a.subdivide_meshes([(CAGE, sub, cage)])
        assert capi.lib().take_hip_accumulated_samples(a.h) == 0
        with pytest.raises(capi.TakeError) as e:
            a.render_accumulate(buf.data_ptr(), 3, 6, seed=4)
        assert e.value.code == D.TAKE_E_INVALID and "restart" in str(e.value)
        assert a.render_accumulate(buf.data_ptr(), 3, 6, seed=4, restart=True) == 3
        torch.cuda.synchronize()
        b = capi.Scene(with_arrays(sd, {CAGE: refined_arrays(sub, cage, sd.meshes[CAGE])}), precision=precision, builder=DEV)
        try:
            assert np.array_equal(buf.cpu().numpy(), b.render(spp=3, max_depth=6, seed=4))
        finally:
            b.close()
    finally:
        a.close(), sub.close()


# ------------------------------------------------------------------ 6. the command line's -subdivide
def test_subdivide_scene_refines_what_it_can_and_names_what_it_cannot():
    """take_amd.render.subdivide_scene (python -m take_amd.render scene -subdivide L): the refined description renders as
    the one made from the host build's arrays; a mesh the scheme refuses is named and left as loaded"""
    from take_amd.render import subdivide_scene, with_refined_meshes

    L, pos, idx = cage_of("octahedron")
    sd = SceneData(width=16, height=16, lookfrom=(0.0, 0.2, 3.6), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0, background=(0.2, 0.3, 0.4), spp=4,
                   max_depth=6)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7))
    sd.add_mesh(pos, idx, grey, normals=pos / np.linalg.norm(pos, axis=1, keepdims=True))
    bow = np.array([[-1.0, -1.0, 0.0], [-0.5, -1.0, 0.0], [-0.7, -0.6, 0.0], [-1.0, -0.2, 0.0], [-0.5, -0.2, 0.0]])
    sd.add_mesh(bow, np.array([[0, 1, 2], [2, 4, 3]], np.int32), grey, normals=np.tile([0.0, 0.0, 1.0], (5, 1)), emission=(4.0, 4.0, 4.0))  # a bow-tie: refused
    sd.add_sphere((0.0, 0.75, 0.0), 0.25, grey)
    said = []
    got = subdivide_scene(sd, 2, log=said.append)
    assert len(said) == 1 and "mesh 1 is left as loaded" in said[0] and "bow-tie" in said[0]
    p, n, i, _ = host_refine(pos, idx, 2)
    want = with_refined_meshes(sd, {0: (p, i, n, None)}, 2)
    assert np.array_equal(got.meshes[0].indices, i) and differing(got.meshes[0].positions, p) == 0 and differing(got.meshes[0].normals, n) == 0
    assert got.meshes[1] is sd.meshes[1] and got.n_shapes == 8 * 16 + 2 + 1
    a, b = capi.Scene(got, precision=F32), capi.Scene(want, precision=F32)
    try:
        ia, ib = a.render(spp=4, max_depth=6, seed=2), b.render(spp=4, max_depth=6, seed=2)
        assert np.array_equal(ia, ib) and np.isfinite(ia).all() and ia.mean() > 0
        assert a.stats()["n_prims"] == 8 * 16 + 2 + 1
    finally:
        a.close(), b.close()


def test_the_recomputing_normal_pass_gives_the_same_bits(monkeypatch):
    """TAKE_HIP_SUBDIV_NORMALS=recompute (the variant without the face-normal array; DESIGN.md §4s has its timing)"""
    monkeypatch.setenv("TAKE_HIP_SUBDIV_NORMALS", "recompute")
    for name, L, pos, idx, uv, want_p, want_n, _, _ in reference():
        with capi.Subdiv(idx, pos.shape[0], L) as sub:
            got_p, got_n = sub.refine(pos)
            assert differing(got_p, want_p) == 0 and differing(got_n, want_n) == 0, f"{name} L{L}"

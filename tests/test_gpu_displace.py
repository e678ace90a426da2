"""Displacement mapping on the device: take_hip_displace_apply*, take_hip_scene_displace_meshes (k_displace —
take_amd/csrc/tk_displace.h, tk_displace.hip — between tk_subdiv.hip's two normal launches).  Two
yardsticks: the host build of the same bodies (tests/displace_host, itself held to tests/displace_ref.py by
tests/test_displace_cpu.py) for the displaced arrays, bit for bit; and for the scene-bound call the scene after apply()
to the host + update_meshes(host arrays), and a FRESH device-built scene from the displaced arrays: debug_tree records,
stats, hit tables and render bytes."""
import functools
import types

import numpy as np
import pytest
import torch

import displace_ref
import subdiv_ref
from take_amd import capi
from take_amd import cdefs as D
from take_amd.scene import SceneData
from test_displace_cpu import differing, host_apply, host_case
from test_gpu_device_build_instanced import abi, scene_rays
from test_gpu_mesh_update import same_scene, snapshot, unchanged, with_arrays
from test_gpu_repose import same_everything, tmin_of
from test_gpu_skin import strip_pose, strip_rig
from test_gpu_subdiv import CAGE, OTHER, cage_of, cage_scene, wobbled
from test_subdiv_cpu import host_refine

pytestmark = pytest.mark.gpu
DEV = D.TAKE_BUILDER_DEVICE_LBVH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]
SCALE, BIAS = 0.08, -0.01  # (small against the scene: the displaced meshes stay in view)


@functools.lru_cache(maxsize=None)
def reference():
    """[(case, host positions, host direction, host normals)] over the CPU case list: computed once, shared, never
    written (the launches' own grids: what the device runs)"""
    out = []
    for c in displace_ref.cases():
        got = host_case(c)
        for k in ("positions", "direction", "normals"):
            got[k].setflags(write=False)
        out.append((c, got["positions"], got["direction"], got["normals"]))
    return out


def same_bits(got, want, nan):
    """bit for bit; where the image has a NaN texel the payload of a NaN is the arithmetic unit's to choose"""
    if not nan:
        return differing(got, want) == 0
    return np.array_equal(np.isnan(got), np.isnan(want)) and differing(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0)) == 0


# ------------------------------------------------------------------ 1. the displaced arrays
@pytest.mark.parametrize("source", ["host", "device", "other-stream"])
def test_apply_equals_the_host_build_bit_for_bit(source):
    """over the CPU case list: the base arrays from host memory / from device tensors / from device tensors written on
    another stream just before the call; the image from host memory and from a device tensor in turn"""
    side = torch.cuda.Stream()
    assert len(reference()) == 52
    for k, (c, want_p, want_d, want_n) in enumerate(reference()):
        nv = want_p.shape[0]
        image = torch.from_numpy(np.array(c["image"])).cuda() if k % 2 else c["image"]
        with capi.Displace(c["indices"], nv, c["uvs"], image, c["uvxf"]) as dis:
            info = dis.info()
            assert (info["n_vertices"], info["n_faces"], info["width"], info["height"]) == (nv, c["indices"].shape[0]) + c["image"].shape[::-1], c["name"]
            out_p = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device="cuda")  # (a guard row behind each output)
            out_n = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device="cuda")
            if source == "host":
                got_p, got_n = dis.apply(c["positions"], c["normals"], c["scale"], c["bias"])
                dis.apply_device(out_p, out_n, c["positions"], c["normals"], c["scale"], c["bias"])
            else:
                stream = side if source == "other-stream" else torch.cuda.current_stream()
                with torch.cuda.stream(stream):
                    if source == "other-stream":  # (work in front of the write: a call that does not wait reads zeros)
                        busy = torch.ones((1024, 1024), device="cuda")
                        for _ in range(8):
                            busy = busy @ busy * 1e-3
                    base_p = torch.zeros((nv, 3), dtype=torch.float64, device="cuda").copy_(torch.from_numpy(np.array(c["positions"])), non_blocking=True)
                    base_n = None
                    if c["normals"] is not None:
                        base_n = torch.zeros((nv, 3), dtype=torch.float64, device="cuda").copy_(torch.from_numpy(np.array(c["normals"])), non_blocking=True)
                    got_p, got_n = dis.apply(base_p, base_n, c["scale"], c["bias"])
                    dis.apply_device(out_p, out_n, base_p, base_n, c["scale"], c["bias"], stream=stream.cuda_stream if source == "other-stream" else None)
            torch.cuda.synchronize()
            assert same_bits(got_p, want_p, c["nan"]), f"{c['name']}: positions"
            assert same_bits(got_n, want_n, c["nan"]), f"{c['name']}: normals"
            assert same_bits(out_p[:nv].cpu().numpy(), want_p, c["nan"]) and (out_p[nv] == -7.0).all(), f"{c['name']}: positions, device"
            assert same_bits(out_n[:nv].cpu().numpy(), want_n, c["nan"]) and (out_n[nv] == -7.0).all(), f"{c['name']}: normals, device"


def test_normals_can_be_left_out_either_way_and_the_buffers_are_reused_not_grown():
    c, want_p, want_d, want_n = next(r for r in reference() if r[0]["name"] == "strip23-L2/16x16-float32")
    nv = want_p.shape[0]
    mesh = next(m for m in displace_ref.meshes() if m[0] == c["mesh"])
    with capi.Displace(c["indices"], nv, c["uvs"], c["image"], c["uvxf"]) as dis:
        created = dis.info()["device_bytes"]
        assert created > 8 * 3 * nv * 4 + c["image"].nbytes
        out_p = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device="cuda")
        dis.apply_device(out_p, None, c["positions"], c["normals"], c["scale"], c["bias"])  # normals out left out
        assert differing(out_p[:nv].cpu().numpy(), want_p) == 0 and (out_p[nv] == -7.0).all()
        assert differing(dis.apply(c["positions"], c["normals"], c["scale"], c["bias"], out_normals=False), want_p) == 0
        # normals in left out against the same normals given: the handle's own are the refined surface's
        own = dis.apply(c["positions"], None, c["scale"], c["bias"])
        given = dis.apply(c["positions"], mesh[2], c["scale"], c["bias"])
        assert differing(own[0], given[0]) == 0 and differing(own[1], given[1]) == 0
        # another scale and bias over another base: the same buffers
        other = wobbled(np.array(c["positions"]), 1.0)
        want = host_apply(other, None, c["indices"], c["uvs"], c["image"], c["uvxf"], -0.4, 0.07)
        got_p, got_n = dis.apply(other, None, -0.4, 0.07)
        assert differing(got_p, want["positions"]) == 0 and differing(got_n, want["normals"]) == 0 and differing(got_p, want_p) > 0
        assert dis.info()["device_bytes"] == created
        in_place = torch.from_numpy(other).cuda()  # displacing into the base array itself is refused, and nothing is written
        with pytest.raises(capi.TakeError, match="an output array is an input"):
            dis.apply_device(in_place, None, in_place, None, -0.4, 0.07)
        assert differing(in_place.cpu().numpy(), other) == 0


# ------------------------------------------------------------------ 2. scenes
IMAGE = displace_ref.image(16, 16, np.float32)


def surface_of(kind):
    """the refined cage of test_gpu_subdiv's scene with uvs -> (levels, cage positions, cage indices, cage uvs, refined
    indices, refined uvs)"""
    L, pos, idx = cage_of(kind)
    cage_uv = displace_ref.mesh_uvs(pos.shape[0])
    i, _, uv = subdiv_ref.topology(idx, pos.shape[0], L, cage_uv)
    return L, pos, idx, cage_uv, i, uv


def displaced_arrays(dis, base, mesh, scale=SCALE, bias=BIAS):
    """what update_meshes takes for the mesh: displaced positions, and normals when the mesh has them"""
    p, n = dis.apply(base[0], base[1], scale, bias)
    return (p, n) if mesh.normals is not None else p


@pytest.mark.parametrize("two_level", [False, True], ids=["one-level", "two-level"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_displace_meshes_equals_apply_then_update_equals_a_fresh_scene(precision, two_level):
    """mesh 0 displaced beside an untouched mesh and a sphere: host base arrays with given normals, then device tensors
    with the handle's own normals"""
    kind = "octahedron" if two_level else "strip23"
    sd, L, pos, idx = cage_scene(kind, two_level=two_level)
    _, _, _, _, i, uv = surface_of(kind)
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    dis = capi.Displace(i, sd.meshes[CAGE].positions.shape[0], uv, IMAGE)
    try:
        for seed, device in ((1.0, False), (2.0, True)):
            p, n, _, _ = host_refine(wobbled(pos, seed), idx, L)
            base = (p, None if device else n)
            a.displace_meshes([(CAGE, dis, tuple(None if x is None else torch.from_numpy(x).cuda() for x in base) if device else base, SCALE, BIAS)])
            arrays = displaced_arrays(dis, base, sd.meshes[CAGE])
            assert isinstance(arrays, tuple) and np.abs(arrays[0] - p).max() > 0.02
            b.update_meshes({CAGE: arrays})
            same_scene(a, b, precision, rays)
            c = capi.Scene(with_arrays(sd, {CAGE: arrays}), precision=precision, builder=DEV)
            try:
                (same_everything if two_level else same_scene)(a, c, precision, rays)
                assert a.stats()["n_prims"] == c.stats()["n_prims"]
            finally:
                c.close()
    finally:
        a.close(), b.close(), dis.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_subdivision_binding_equals_refine_then_apply_then_update(precision):
    """the cage as positions (host, then device), then as a rig's pose"""
    sd, L, pos, idx = cage_scene("strip23")
    _, _, _, cage_uv, i, uv = surface_of("strip23")
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    sub = capi.Subdiv(idx, pos.shape[0], L, uvs=cage_uv)
    dis = capi.Displace.of_subdiv(sub, IMAGE)
    rig = strip_rig(types.SimpleNamespace(positions=pos, normals=None), normals=False)
    try:
        assert dis.n_vertices == sub.n_vertices == sd.meshes[CAGE].positions.shape[0]
        for seed, device in ((3.0, False), (4.0, True)):
            cage = wobbled(pos, seed)
            a.displace_meshes([(CAGE, dis, (sub, torch.from_numpy(cage).cuda() if device else cage), SCALE, BIAS)])
            p, n = sub.refine(cage)
            want = host_apply(p, n, i, uv, IMAGE, scale=SCALE, bias=BIAS)
            got_p, got_n = dis.apply(p, n, SCALE, BIAS)
            assert differing(got_p, want["positions"]) == 0 and differing(got_n, want["normals"]) == 0
            b.update_meshes({CAGE: (got_p, got_n)})
            same_scene(a, b, precision, rays)
        X, tw = strip_pose(4)
        a.displace_meshes([(CAGE, dis, (sub, (rig, X, tw)), SCALE, BIAS)])
        p, n = sub.refine(rig.pose(X, tw))
        b.update_meshes({CAGE: dis.apply(p, n, SCALE, BIAS)})
        same_scene(a, b, precision, rays)
        a.displace_meshes([(CAGE, dis, (sub, (rig, torch.from_numpy(X).cuda(), torch.from_numpy(tw).cuda())), SCALE, BIAS)])  # the pose in device memory
        same_scene(a, b, precision, rays)
    finally:
        a.close(), b.close(), sub.close(), dis.close(), rig.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_mesh_without_vertex_normals_gets_positions_alone(precision):
    sd, L, pos, idx = cage_scene("strip23", normals=False)
    _, _, _, _, i, uv = surface_of("strip23")
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    dis = capi.Displace(i, sd.meshes[CAGE].positions.shape[0], uv, IMAGE)
    try:
        p, n, _, _ = host_refine(wobbled(pos, 3.0), idx, L)
        a.displace_meshes([(CAGE, dis, (p, n), SCALE, BIAS)])
        arrays = displaced_arrays(dis, (p, n), sd.meshes[CAGE])
        assert not isinstance(arrays, tuple)
        b.update_meshes({CAGE: arrays})
        same_scene(a, b, precision, rays)
    finally:
        a.close(), b.close(), dis.close()


# ------------------------------------------------------------------ 3. tracking
@pytest.mark.parametrize("two_level", [False, True], ids=["one-level", "two-level"])
def test_tracked_motion_planes_equal_those_after_update_meshes(two_level):
    sd, L, pos, idx = cage_scene("strip23", two_level=two_level)
    _, _, _, _, i, uv = surface_of("strip23")
    a, b = capi.Scene(sd, precision=F32), capi.Scene(sd, precision=F32)
    dis = capi.Displace(i, sd.meshes[CAGE].positions.shape[0], uv, IMAGE)
    try:
        base = host_refine(wobbled(pos, 5.0), idx, L)[:2]
        for sc in (a, b):
            sc.track_vertices()
            sc.mark_frame()
        a.displace_meshes([(CAGE, dis, base, SCALE, BIAS)])
        b.update_meshes({CAGE: displaced_arrays(dis, base, sd.meshes[CAGE])})
        assert a.tracking_info() == b.tracking_info() and a.tracking_info()["marked_bytes"] > 0
        pa, pb = a.render_motion(), b.render_motion()
        assert set(pa) == set(pb) and all(np.array_equal(pa[k], pb[k]) for k in pa)
    finally:
        a.close(), b.close(), dis.close()


# ------------------------------------------------------------------ 4. failures
def refused(sc, bindings, code=D.TAKE_E_INVALID):
    with pytest.raises(capi.TakeError) as e:
        sc.displace_meshes(bindings)
    assert e.value.code == code, str(e.value)
    return str(e.value).split(": ", 1)[1]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_scene_unchanged(precision):
    sd, L, pos, idx = cage_scene("strip23")
    _, _, _, cage_uv, i, uv = surface_of("strip23")
    rays = abi(scene_rays(1024, 8, tmin=tmin_of(precision)), precision)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    nv = sd.meshes[CAGE].positions.shape[0]
    sub, coarse = capi.Subdiv(idx, pos.shape[0], L, uvs=cage_uv), capi.Subdiv(idx, pos.shape[0], L - 1, uvs=cage_uv)
    dis, second, small = capi.Displace(i, nv, uv, IMAGE), capi.Displace(i, nv, uv, IMAGE), capi.Displace.of_subdiv(coarse, IMAGE)
    pos65, idx65 = subdiv_ref.strip(65, -0.9)
    other = capi.Displace(idx65, 65, displace_ref.mesh_uvs(65), IMAGE)
    rig = strip_rig(types.SimpleNamespace(positions=pos, normals=None), normals=False)
    short = strip_rig(types.SimpleNamespace(positions=pos[:21], normals=None), normals=False)
    try:
        X, tw = strip_pose(8)
        cage = wobbled(pos, 6.0)
        p, n, _, _ = host_refine(cage, idx, L)
        before = snapshot(a, precision, rays)
        assert "n must be positive" in refused(a, [])
        assert "binding 1: mesh index out of range" in refused(a, [(CAGE, dis, (p, n)), (2, other, pos65)])
        assert "binding 0: mesh index out of range" in refused(a, [(-1, dis, p)])
        msg = refused(a, [(CAGE, small, small_base(coarse, cage))])
        assert "binding 0" in msg and f"the displacement handle has {small.n_vertices} vertices" in msg and f"mesh {CAGE} has {nv}" in msg, msg
        msg = refused(a, [(CAGE, dis, (coarse, cage))])
        assert "binding 0" in msg and f"the refined cage has {coarse.n_vertices} vertices" in msg and f"the displacement handle has {nv}" in msg and f"mesh {CAGE} has {nv}" in msg, msg
        msg = refused(a, [(CAGE, small, (sub, cage))])
        assert f"the refined cage has {nv} vertices" in msg and f"the displacement handle has {small.n_vertices}" in msg, msg
        assert "mesh 0 appears more than once" in refused(a, [(CAGE, dis, p), (CAGE, second, p)])
        assert "a displacement handle is bound more than once" in refused(a, [(CAGE, dis, p), (OTHER, dis, p)])
        assert "a subdivision handle is bound more than once" in refused(a, [(CAGE, dis, (sub, cage)), (OTHER, other, (sub, cage))])
        assert "exactly one of positions and subdiv" in refused(a, [(CAGE, dis, None)])
        assert "exactly one of cage_positions and rig" in refused(a, [(CAGE, dis, (sub, None))])
        assert "scale and bias must be finite" in refused(a, [(CAGE, dis, p, np.nan, 0.0)])
        assert "scale and bias must be finite" in refused(a, [(CAGE, dis, p, 1.0, -np.inf)])
        assert "joint_xforms is required" in refused(a, [(CAGE, dis, (sub, (rig, None, tw)))])
        msg = refused(a, [(CAGE, dis, (sub, (short, X, tw)))])
        assert "binding 0" in msg and "the rig has 21 vertices, the cage has 23" in msg, msg
        bad = p.copy()
        bad[11, 1] = np.inf  # a base position that is not finite: the update's own finiteness check names mesh and vertex
        msg = refused(a, [(CAGE, dis, (bad, n))])
        assert f"mesh {CAGE}" in msg and "vertex" in msg and "finite" in msg, msg
        assert unchanged(a, precision, rays, before)
        a.displace_meshes([(CAGE, dis, (p, n), SCALE, BIAS)])  # ... and the scene still takes a displacement
        assert not unchanged(a, precision, rays, before)
    finally:
        for h in (a, sub, coarse, dis, second, small, other, rig, short):
            h.close()


def small_base(sub, cage):
    return sub.refine(cage)


def test_every_allocation_failing_in_turn_leaves_the_scene_as_it_was(monkeypatch):
    precision = F32
    sd, L, pos, idx = cage_scene("strip23")
    _, _, _, cage_uv, i, uv = surface_of("strip23")
    rays = abi(scene_rays(1024, 8, tmin=tmin_of(precision)), precision)
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    sub = capi.Subdiv(idx, pos.shape[0], L, uvs=cage_uv)
    dis = capi.Displace.of_subdiv(sub, IMAGE)
    try:
        cage = wobbled(pos, 7.0)
        before = snapshot(a, precision, rays)
        bytes_before = (sub.info()["device_bytes"], dis.info()["device_bytes"])
        failed = 0
        for nth in range(1, 400):
            monkeypatch.setenv("TAKE_HIP_FAIL_ALLOC", str(nth))
            try:
                a.displace_meshes([(CAGE, dis, (sub, cage), SCALE, BIAS)])
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
        assert failed >= 4 and (sub.info()["device_bytes"], dis.info()["device_bytes"]) == bytes_before
        p, n = sub.refine(cage)
        b.update_meshes({CAGE: dis.apply(p, n, SCALE, BIAS)})
        same_scene(a, b, precision, scene_rays(1024, 8, tmin=tmin_of(precision)))
    finally:
        a.close(), b.close(), sub.close(), dis.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_displacement_ends_a_progressive_sequence_and_a_refused_one_does_not(precision):
    sd, L, pos, idx = cage_scene("strip23")
    _, _, _, _, i, uv = surface_of("strip23")
    a = capi.Scene(sd, precision=precision, builder=DEV)
    dis = capi.Displace(i, sd.meshes[CAGE].positions.shape[0], uv, IMAGE)
    try:
        p, n, _, _ = host_refine(wobbled(pos, 9.0), idx, L)
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4, restart=True) == 2
        bad = p.copy()
        bad[0, 1] = np.nan
        refused(a, [(CAGE, dis, (bad, n), SCALE, BIAS)])
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4) == 4, "a refused call leaves the sequence running"
        a.displace_meshes([(CAGE, dis, (p, n), SCALE, BIAS)])
        assert capi.lib().take_hip_accumulated_samples(a.h) == 0
        with pytest.raises(capi.TakeError) as e:
            a.render_accumulate(buf.data_ptr(), 3, 6, seed=4)
        assert e.value.code == D.TAKE_E_INVALID and "restart" in str(e.value)
        assert a.render_accumulate(buf.data_ptr(), 3, 6, seed=4, restart=True) == 3
        torch.cuda.synchronize()
        b = capi.Scene(with_arrays(sd, {CAGE: displaced_arrays(dis, (p, n), sd.meshes[CAGE])}), precision=precision, builder=DEV)
        try:
            assert np.array_equal(buf.cpu().numpy(), b.render(spp=3, max_depth=6, seed=4))
        finally:
            b.close()
    finally:
        a.close(), dis.close()


# ------------------------------------------------------------------ 5. the command line's -displace
def test_displace_scene_displaces_what_it_can_and_names_what_it_cannot():
    """take_amd.render.displace_scene (python -m take_amd.render scene -displace FILE,SCALE[,BIAS]): a mesh with uvs and
    normals moves along its own normals and gets new ones; one with uvs alone moves along the handle's own normals and
    gets none; a mesh without uvs is named and left as loaded"""
    from take_amd.render import displace_scene

    L, pos, idx, cage_uv, i, uv = surface_of("octahedron")
    p, n, _, _ = host_refine(pos, idx, L)
    sd = SceneData(width=16, height=16, lookfrom=(0.0, 0.2, 3.6), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0, background=(0.2, 0.3, 0.4), spp=4,
                   max_depth=6)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7))
    sd.add_mesh(p, i, grey, normals=n, uvs=uv)
    pos2, idx2 = subdiv_ref.strip(65, -0.9)
    sd.add_mesh(pos2, idx2, grey, uvs=displace_ref.mesh_uvs(65))
    sd.add_mesh(pos2 + np.array([0.0, 0.0, -0.5]), idx2, grey)  # no uvs: left as loaded
    sd.add_sphere((0.0, 0.75, 0.0), 0.25, grey)
    said = []
    got = displace_scene(sd, IMAGE, SCALE, BIAS, log=said.append)
    assert len(said) == 1 and "mesh 2 is left as loaded" in said[0] and "no uvs" in said[0]
    first = host_apply(p, n, i, uv, IMAGE, scale=SCALE, bias=BIAS)
    second = host_apply(pos2, None, idx2, displace_ref.mesh_uvs(65), IMAGE, scale=SCALE, bias=BIAS)
    assert differing(got.meshes[0].positions, first["positions"]) == 0 and differing(got.meshes[0].normals, first["normals"]) == 0
    assert differing(got.meshes[1].positions, second["positions"]) == 0 and got.meshes[1].normals is None
    assert got.meshes[2] is sd.meshes[2] and np.array_equal(got.meshes[0].indices, i) and sd.meshes[0].positions is not got.meshes[0].positions
    assert differing(sd.meshes[0].positions, p) == 0  # (the description that went in is as it was)
    a, b = capi.Scene(got, precision=F32), capi.Scene(with_arrays(sd, {0: (first["positions"], first["normals"]), 1: second["positions"]}), precision=F32)
    try:
        ia, ib = a.render(spp=4, max_depth=6, seed=2), b.render(spp=4, max_depth=6, seed=2)
        assert np.array_equal(ia, ib) and np.isfinite(ia).all() and ia.mean() > 0
    finally:
        a.close(), b.close()

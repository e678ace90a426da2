"""Rigs on the device: take_hip_rig_pose*, take_hip_scene_pose_meshes (k_skin_palette, k_skin_pose, k_skin_check_joints —
take_amd/csrc/tk_skin.h, tk_skin.hip).  Two yardsticks: the host build of the same bodies
(tests/skin_host, itself held to tests/skin_ref.py by tests/test_skin_cpu.py) for the posed arrays, bit for bit; and
for the scene-bound call the scene after rig.pose() + update_meshes(host arrays), and a FRESH device-built scene from
the posed arrays: debug_tree records, stats, hit tables and render bytes."""
import functools

import numpy as np
import pytest
import torch

from take_amd import capi
from take_amd import cdefs as D
from take_amd.scene import Light, SceneData
from test_gpu_device_build_instanced import abi, scene_rays
from test_gpu_mesh_update import same_scene, snapshot, unchanged, with_arrays
from test_gpu_repose import same_everything, tmin_of
from test_skin_cpu import all_cases, differing, host, host_pose

pytestmark = pytest.mark.gpu
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]
RIG_KEYS = ("positions", "normals", "joints", "weights", "inverse_bind", "target_positions", "target_normals")


@functools.lru_cache(maxsize=None)
def reference():
    """[(name, case, host positions, host normals)]: computed once, shared, never written"""
    out = []
    for name, grid, case in all_cases():
        p, n = host_pose(case)  # (the launch's own grid: what the device runs)
        p.setflags(write=False)
        out.append((name, case, p, n))
    return out


def rig_of(case, device=False):
    args = {k: case.get(k) for k in RIG_KEYS}
    if device:
        args = {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in args.items()}
    nj = None if case.get("joints") is None else case["joint_xforms"].shape[0]
    return capi.Rig(n_joints=nj, **args)


# ------------------------------------------------------------------ 1. the posed arrays
@pytest.mark.parametrize("source", ["host", "device", "other-stream"])
def test_pose_equals_the_host_build_bit_for_bit(source):
    """over the CPU case list: rig arrays from host memory / from device tensors; pose arrays from host memory / device
    tensors / device tensors written on another stream just before the call"""
    side = torch.cuda.Stream()
    for name, case, want_p, want_n in reference():
        nv = case["positions"].shape[0]
        with rig_of(case, device=(source == "device")) as rig:
            info = rig.info()
            assert (info["n_vertices"], info["has_normals"]) == (nv, want_n is not None), name
            X, tw = case.get("joint_xforms"), case.get("target_weights")
            out_p = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device="cuda")  # (a guard row behind each output)
            out_n = torch.full((nv + 1, 3), -7.0, dtype=torch.float64, device="cuda") if want_n is not None else None
            if source == "host":
                got = rig.pose(X, tw)
                rig.pose_device(out_p, out_n, X, tw)
            else:
                stream = side if source == "other-stream" else torch.cuda.current_stream()
                with torch.cuda.stream(stream):
                    if source == "other-stream":  # (work in front of the writes: a call that does not wait reads zeros)
                        busy = torch.ones((1024, 1024), device="cuda")
                        for _ in range(8):
                            busy = busy @ busy * 1e-3
                    dX = None if X is None else torch.zeros(X.shape, dtype=torch.float64, device="cuda").copy_(torch.from_numpy(X), non_blocking=True)
                    dw = None if tw is None else torch.zeros(tw.shape, dtype=torch.float64, device="cuda").copy_(torch.from_numpy(tw), non_blocking=True)
                    got = rig.pose(dX, dw)
                    rig.pose_device(out_p, out_n, dX, dw, stream=stream.cuda_stream if source == "other-stream" else None)
            torch.cuda.synchronize()
            got_p, got_n = got if want_n is not None else (got, None)
            assert differing(got_p, want_p) == 0, f"{name}: positions"
            assert differing(out_p[:nv].cpu().numpy(), want_p) == 0 and (out_p[nv] == -7.0).all(), f"{name}: positions, device"
            if want_n is not None:
                assert differing(got_n, want_n) == 0, f"{name}: normals"
                assert differing(out_n[:nv].cpu().numpy(), want_n) == 0 and (out_n[nv] == -7.0).all(), f"{name}: normals, device"


def test_a_rig_with_normals_poses_positions_alone_when_no_normals_are_wanted():
    name, case, want_p, want_n = next(r for r in reference() if r[0] == "mirror")
    nv = case["positions"].shape[0]
    with rig_of(case) as rig:
        out_p = torch.zeros((nv, 3), dtype=torch.float64, device="cuda")
        rig.pose_device(out_p, None, case["joint_xforms"], case["target_weights"])
        assert differing(out_p.cpu().numpy(), want_p) == 0


def test_device_rig_reports_the_smallest_bad_vertex():
    case = dict(next(r for r in reference() if r[0] == "grid2")[1])
    joints = case["joints"].copy()
    joints[900, 1], joints[411, 3], joints[1300, 0] = 7, -1, 99  # (7 joints: 0..6)
    case["joints"] = joints
    assert host().skin_host_check_joints(joints.ctypes.data, 4, 7, 1301, 0) == 411
    with pytest.raises(capi.TakeError) as e:
        rig_of(case, device=True)
    assert e.value.code == D.TAKE_E_INVALID and "vertex 411:" in str(e.value) and "out of range" in str(e.value)
    with pytest.raises(capi.TakeError) as e:  # the host variant names the index too
        rig_of(case)
    assert e.value.code == D.TAKE_E_INVALID and "vertex 411:" in str(e.value) and "-1" in str(e.value)
    bad = dict(case, joints=next(r for r in reference() if r[0] == "grid2")[1]["joints"])
    bad["weights"] = bad["weights"].copy()
    bad["weights"][5, 0] = np.nan
    with pytest.raises(capi.TakeError) as e:
        rig_of(bad)
    assert e.value.code == D.TAKE_E_INVALID and "weights[20] is not finite" in str(e.value)


# ------------------------------------------------------------------ 2. scenes
STRIP, OTHER = 0, 1  # the meshes of strip_scene


def strip(nv, y0, normals):
    """a bent strip of triangles over nv vertices in two rows: nv - 2 faces (one vertex: one degenerate face)"""
    i = np.arange(nv)
    x = -1.0 + 2.0 * (i // 2) / max((nv - 1) // 2, 1)
    pos = np.stack([x, y0 + 0.4 * (i % 2), 0.3 * np.sin(2.0 * x)], axis=1)
    idx = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(nv - 2)] or [[0, 0, 0]], np.int32)
    nrm = None
    if normals:
        nrm = np.stack([-0.6 * np.cos(2.0 * x), np.zeros(nv), np.ones(nv)], axis=1)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return pos, idx, nrm


def strip_scene(nv, normals=True, two_level=False):
    """mesh 0: the strip of nv vertices; mesh 1: a strip of 65 vertices without vertex normals; a sphere beside them; a
    point light.  two_level: mesh 0 is a prototype placed three times instead.  nv = 1: mesh 0 alone."""
    sd = SceneData(width=16, height=16, lookfrom=(0.0, 0.2, 3.6), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0, background=(0.2, 0.3, 0.4), spp=4,
                   max_depth=6)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7))
    gold = sd.add_material(D.MAT_BLINN_PHONG_MICROFACET, (0.8, 0.7, 0.3), (30.0,))
    pos, idx, nrm = strip(nv, -0.2, normals)
    if two_level:
        assert sd.add_prototype(pos, idx, gold, normals=nrm) == STRIP
    else:
        sd.add_mesh(pos, idx, gold, normals=nrm)
    if nv > 1:
        pos2, idx2, _ = strip(65, -0.9, False)
        sd.add_mesh(pos2, idx2, grey)
    if two_level:
        for k, (t, s) in enumerate((((0.0, 0.0, 0.0), 1.0), ((0.3, 0.6, -0.5), 0.7), ((-0.4, 0.9, 0.4), 0.5))):
            c, sn = np.cos(0.4 * k), np.sin(0.4 * k)
            sd.add_instance(STRIP, np.concatenate([s * np.array([[c, -sn, 0.0], [sn, c, 0.1], [0.0, 0.0, 1.0]]), np.array(t)[:, None]], axis=1), -1 if k else grey)
    if nv > 1:  # (one vertex: one degenerate face and nothing else — a tree of a single leaf)
        sd.add_sphere((0.0, 0.75, 0.0), 0.25, grey)
    sd.lights.append(Light(0, -1, (12.0, 12.0, 12.0), (0.3, 2.0, 1.5)))
    return sd


def strip_rig(mesh, normals=True, targets=1):
    """three joints along x, K = 4 (the fourth influence is padding), inverse bind matrices, `targets` morph targets"""
    pos = mesh.positions
    nv = pos.shape[0]
    centres = np.array([-1.0, 0.0, 1.0])
    w = np.maximum(1.0 - np.abs(pos[:, :1] - centres[None, :]), 0.0) + 0.05
    w = np.concatenate([w / w.sum(axis=1, keepdims=True), np.zeros((nv, 1))], axis=1)
    joints = np.tile(np.array([0, 1, 2, 1], np.int32), (nv, 1))
    bind = np.tile(np.eye(3, 4), (3, 1, 1))
    bind[:, 0, 3] = -centres
    tp = np.stack([0.1 * np.sin(5.0 * pos + t) for t in range(targets)]) if targets else None
    tn = np.stack([0.05 * np.cos(3.0 * pos + t) for t in range(targets)]) if targets and normals else None
    nrm = mesh.normals if normals else None
    if normals and nrm is None:
        nrm = np.tile([0.0, 0.0, 1.0], (nv, 1))
    return capi.Rig(pos, normals=nrm, joints=joints, weights=w, inverse_bind=bind, target_positions=tp, target_normals=tn)


def strip_pose(seed, targets=1, identity=False):
    """joint -> world matrices for strip_rig: a rotation about z by a few tenths, a non-uniform scale, back to the joint"""
    rng = np.random.default_rng(seed)
    X = np.tile(np.eye(3, 4), (3, 1, 1))
    X[:, 0, 3] = [-1.0, 0.0, 1.0]
    if not identity:
        for j in range(3):
            a = rng.uniform(-0.5, 0.5)
            X[j, :, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) * rng.uniform(0.8, 1.2, 3)[None, :]
            X[j, :, 3] += rng.uniform(-0.1, 0.1, 3)
    tw = None if not targets else (np.zeros(targets) if identity else rng.uniform(0.2, 1.0, targets))
    return X, tw


def posed_arrays(rig, X, tw, mesh):
    """what update_meshes takes for the mesh: positions, and normals when both the rig and the mesh have them"""
    got = rig.pose(X, tw)
    p, n = got if rig.has_normals else (got, None)
    return (p, n) if (n is not None and mesh.normals is not None) else p


@pytest.mark.parametrize("nv", [63, 64, 65, 257])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pose_meshes_equals_pose_then_update_equals_a_fresh_scene(precision, nv):
    sd = strip_scene(nv)
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    rig = strip_rig(sd.meshes[STRIP])
    try:
        for seed, identity in ((1, False), (2, True)):
            X, tw = strip_pose(seed, identity=identity)
            a.pose_meshes([(STRIP, rig, X, tw)])
            arrays = posed_arrays(rig, X, tw, sd.meshes[STRIP])
            assert isinstance(arrays, tuple)
            if identity:
                # an identity pose: X · B = I up to the rounding of (x - c) + c, weights that sum to 1 up to theirs — a dozen
                # roundings of 2^-53 on coordinates below 2 (bit equality is for binary-fraction weights: the CPU file)
                assert np.abs(arrays[0] - sd.meshes[STRIP].positions).max() <= 16 * 2.0**-52
            else:
                assert np.abs(arrays[0] - sd.meshes[STRIP].positions).max() > 0.05
            b.update_meshes({STRIP: arrays})
            same_scene(a, b, precision, rays)
            c = capi.Scene(with_arrays(sd, {STRIP: arrays}), precision=precision, builder=DEV)
            try:
                same_scene(a, c, precision, rays)
            finally:
                c.close()
    finally:
        a.close(), b.close(), rig.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_meshes_in_one_call_and_normals_only_where_both_have_them(precision):
    """mesh 0 has vertex normals, mesh 1 has none; rigs with and without normals on either: a mesh with normals under a
    rig without keeps its own, a rig with normals computes none for a mesh without"""
    sd = strip_scene(257)
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    for rig_normals in ((True, True), (False, False)):
        a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
        rigs = [strip_rig(sd.meshes[m], normals=rig_normals[m], targets=2 - m) for m in (STRIP, OTHER)]
        try:
            poses = [strip_pose(3 + m, targets=2 - m) for m in (STRIP, OTHER)]
            # device tensors for one binding, host arrays for the other
            a.pose_meshes([(OTHER, rigs[OTHER], poses[OTHER][0], poses[OTHER][1]),
                           (STRIP, rigs[STRIP], torch.from_numpy(poses[STRIP][0]).cuda(), torch.from_numpy(poses[STRIP][1]).cuda())])
            arrays = {m: posed_arrays(rigs[m], *poses[m], sd.meshes[m]) for m in (STRIP, OTHER)}
            assert isinstance(arrays[STRIP], tuple) == rig_normals[STRIP] and not isinstance(arrays[OTHER], tuple)
            b.update_meshes(arrays)
            same_scene(a, b, precision, rays)
            c = capi.Scene(with_arrays(sd, arrays), precision=precision, builder=DEV)
            try:
                same_scene(a, c, precision, rays)
            finally:
                c.close()
        finally:
            a.close(), b.close()
            for r in rigs:
                r.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_level_scene_whose_prototype_is_posed(precision):
    """as take_hip_scene_update_meshes specifies it for a two-level scene: against the update from host arrays everything,
    trees included; against a fresh scene hit tables and images"""
    sd = strip_scene(65, two_level=True)
    rays = scene_rays(2048, 3, tmin=tmin_of(precision))
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    rig = strip_rig(sd.meshes[STRIP])
    try:
        X, tw = strip_pose(5)
        a.pose_meshes([(STRIP, rig, X, tw)])
        arrays = posed_arrays(rig, X, tw, sd.meshes[STRIP])
        b.update_meshes({STRIP: arrays})
        same_scene(a, b, precision, rays)
        c = capi.Scene(with_arrays(sd, {STRIP: arrays}), precision=precision, builder=DEV)
        try:
            same_everything(a, c, precision, rays)
            assert a.stats()["n_prims"] == c.stats()["n_prims"]
        finally:
            c.close()
    finally:
        a.close(), b.close(), rig.close()


# ------------------------------------------------------------------ 3. tracking
@pytest.mark.parametrize("two_level", [False, True])
def test_tracked_motion_planes_equal_those_after_update_meshes(two_level):
    sd = strip_scene(65, two_level=two_level)
    a, b = capi.Scene(sd, precision=F32), capi.Scene(sd, precision=F32)
    rig = strip_rig(sd.meshes[STRIP])
    try:
        X, tw = strip_pose(6)
        for sc in (a, b):
            sc.track_vertices()
            sc.mark_frame()
        a.pose_meshes([(STRIP, rig, X, tw)])
        b.update_meshes({STRIP: posed_arrays(rig, X, tw, sd.meshes[STRIP])})
        assert a.tracking_info() == b.tracking_info() and a.tracking_info()["marked_bytes"] > 0
        pa, pb = a.render_motion(), b.render_motion()
        assert set(pa) == set(pb) and all(np.array_equal(pa[k], pb[k]) for k in pa)
        plain = capi.Scene(sd, precision=F32)  # (without tracking the motion pass does not see the pose)
        try:
            plain.mark_frame()
            plain.pose_meshes([(STRIP, rig, X, tw)])
            untracked = plain.render_motion()
            assert np.array_equal(untracked["shape_id"], pa["shape_id"]) and np.abs(untracked["prev_xy"] - pa["prev_xy"]).max() > 0.05
        finally:
            plain.close()
    finally:
        a.close(), b.close(), rig.close()


# ------------------------------------------------------------------ 4. failures
def refused(sc, bindings, code=D.TAKE_E_INVALID):
    with pytest.raises(capi.TakeError) as e:
        sc.pose_meshes(bindings)
    assert e.value.code == code, str(e.value)
    return str(e.value).split(": ", 1)[1]


@pytest.mark.parametrize("precision", [F32, MIXED])
def test_every_allocation_failing_in_turn_leaves_the_scene_as_it_was(precision, monkeypatch):
    sd = strip_scene(65)
    rays = abi(scene_rays(1024, 8, tmin=tmin_of(precision)), precision)
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    rig = strip_rig(sd.meshes[STRIP])
    try:
        X, tw = strip_pose(7)
        before = snapshot(a, precision, rays)
        bytes_before = rig.info()["device_bytes"]
        failed = 0
        for nth in range(1, 400):
            monkeypatch.setenv("TAKE_HIP_FAIL_ALLOC", str(nth))
            try:
                a.pose_meshes([(STRIP, rig, X, tw)])
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
        assert failed >= 4 and rig.info()["device_bytes"] == bytes_before
        b.update_meshes({STRIP: posed_arrays(rig, X, tw, sd.meshes[STRIP])})
        same_scene(a, b, precision, rays if precision == MIXED else scene_rays(1024, 8, tmin=tmin_of(precision)))
    finally:
        a.close(), b.close(), rig.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_scene_unchanged(precision):
    sd = strip_scene(65)
    rays = abi(scene_rays(1024, 8, tmin=tmin_of(precision)), precision)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    rig, other, wrong = strip_rig(sd.meshes[STRIP]), strip_rig(sd.meshes[OTHER]), strip_rig(strip_scene(63).meshes[STRIP])
    try:
        X, tw = strip_pose(8)
        before = snapshot(a, precision, rays)
        assert "n must be positive" in refused(a, [])
        assert "binding 1: mesh index out of range" in refused(a, [(STRIP, rig, X, tw), (2, other, X, tw)])
        assert "binding 0: mesh index out of range" in refused(a, [(-1, rig, X, tw)])
        msg = refused(a, [(STRIP, wrong, X, tw)])
        assert "binding 0" in msg and "63 vertices" in msg and f"mesh {STRIP} has 65" in msg, msg
        assert "mesh 0 appears more than once" in refused(a, [(STRIP, rig, X, tw), (STRIP, other, X, tw)])
        assert "a rig is bound more than once" in refused(a, [(STRIP, rig, X, tw), (OTHER, rig, X, tw)])
        assert "joint_xforms is required" in refused(a, [(STRIP, rig, None, tw)])
        assert "target_weights is required" in refused(a, [(STRIP, rig, X, None)])
        bad = X.copy()
        bad[1, 0, 3] = np.inf  # a joint matrix that is not finite: the update's own finiteness check names mesh and vertex
        msg = refused(a, [(OTHER, other, X, tw), (STRIP, rig, bad, tw)])
        assert f"mesh {STRIP}" in msg and "vertex" in msg and "finite" in msg, msg
        assert unchanged(a, precision, rays, before)
        a.pose_meshes([(STRIP, rig, X, tw)])  # ... and the scene still takes a pose
        assert not unchanged(a, precision, rays, before)
    finally:
        a.close(), rig.close(), other.close(), wrong.close()
    # one vertex: a scene of fewer than two leaves, which update_meshes does not support — in its words
    one = strip_scene(1)
    sc = capi.Scene(one, precision=precision, builder=HOST, max_leaf_size=4)
    single = capi.Rig(one.meshes[STRIP].positions, joints=np.zeros((1, 1), np.int32), weights=np.ones((1, 1)))
    try:
        before = snapshot(sc, precision, rays)
        Y = np.eye(3, 4)[None].copy()
        Y[0, 0, 3] = 0.25
        assert differing(single.pose(Y), one.meshes[STRIP].positions + [0.25, 0.0, 0.0]) == 0
        assert refused(sc, [(STRIP, single, Y, None)]).startswith("unsupported")
        assert unchanged(sc, precision, rays, before)
    finally:
        sc.close(), single.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_pose_ends_a_progressive_sequence_and_a_refused_one_does_not(precision):
    sd = strip_scene(65)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    rig = strip_rig(sd.meshes[STRIP])
    try:
        X, tw = strip_pose(9)
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4, restart=True) == 2
        bad = X.copy()
        bad[0, 1, 1] = np.nan
        refused(a, [(STRIP, rig, bad, tw)])
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4) == 4, "a refused pose leaves the sequence running"
        a.pose_meshes([(STRIP, rig, X, tw)])
        assert capi.lib().take_hip_accumulated_samples(a.h) == 0
        with pytest.raises(capi.TakeError) as e:
            a.render_accumulate(buf.data_ptr(), 3, 6, seed=4)
        assert e.value.code == D.TAKE_E_INVALID and "restart" in str(e.value)
        assert a.render_accumulate(buf.data_ptr(), 3, 6, seed=4, restart=True) == 3
        torch.cuda.synchronize()
        b = capi.Scene(with_arrays(sd, {STRIP: posed_arrays(rig, X, tw, sd.meshes[STRIP])}), precision=precision, builder=DEV)
        try:
            assert np.array_equal(buf.cpu().numpy(), b.render(spp=3, max_depth=6, seed=4))
        finally:
            b.close()
    finally:
        a.close(), rig.close()


def test_the_rigs_buffers_are_reused_not_grown():
    sd = strip_scene(257)
    a = capi.Scene(sd, precision=F32, builder=DEV)
    rig = strip_rig(sd.meshes[STRIP], targets=2)
    try:
        created = rig.info()
        nv = 257
        # rest (p, n), K = 4 joints and weights, 3 bind matrices, 2 targets (p, n), the staged pose, the palette, posed (p, n)
        want = 8 * (2 * 3 * nv + 4 * nv + 12 * 3 + 2 * 2 * 3 * nv + (12 * 3 + 2) + 12 * 3 + 2 * 3 * nv) + 4 * 4 * nv
        assert created == {"n_vertices": nv, "n_joints": 3, "n_influences": 4, "n_targets": 2, "has_normals": True, "device_bytes": want}
        sizes = []
        for seed in (1, 2, 3):
            a.pose_meshes([(STRIP, rig, *strip_pose(seed, targets=2))])
            sizes.append(rig.info()["device_bytes"])
        assert sizes == [want] * 3
    finally:
        a.close(), rig.close()

"""CPU side of rigs — skinning and morph targets on the device (take_hip_rig_*, take_hip_scene_pose_meshes,
include/take_hip.h):

1. The kernels' bodies (take_amd/csrc/tk_skin.h) without a GPU: tests/skin_host builds them for the host and runs them in
   the launches' loop structure; they equal tests/skin_ref.py — a numpy restatement written from the specification —
   bit for bit over the shared case list, and have the properties that need no tolerance.
2. The cofactor rule is the right rule: posed normals stay perpendicular to posed edges under non-uniform scale and
   mirroring, within a bound derived from the arithmetic.
3. The API: symbols, struct layouts, every refusal that needs no device, TAKE_E_NO_GPU for valid arguments.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import skin_ref
from take_amd import capi
from take_amd import cdefs as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ["take_hip_rig_create", "take_hip_rig_destroy", "take_hip_rig_info", "take_hip_rig_pose_device", "take_hip_rig_pose", "take_hip_scene_pose_meshes"]

_HOST = None


def host():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "skin_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libskin_host.so"))
        L.skin_host_pose.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 9 + [C.c_int] + [C.c_void_p] * 2
        L.skin_host_check_joints.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int]
        L.skin_host_check_joints.restype = C.c_int64
        _HOST = L
    return _HOST


def host_pose(case, grid=0):
    """tk_skin.h's bodies on the host over a case of skin_ref.make_case -> (positions, normals or None)"""
    keep = []

    def ptr(name, dtype=np.float64):
        a = case.get(name)
        if a is None:
            return None
        keep.append(np.ascontiguousarray(a, dtype))
        return keep[-1].ctypes.data

    nv = case["positions"].shape[0]
    nj = 0 if case.get("joints") is None else case["joint_xforms"].shape[0]
    K = 0 if nj == 0 else case["joints"].shape[1]
    T = 0 if case.get("target_positions") is None else case["target_positions"].shape[0]
    out_p = np.zeros((nv, 3))
    out_n = np.zeros((nv, 3)) if case.get("normals") is not None else None
    rc = host().skin_host_pose(nv, nj, K, T, ptr("positions"), ptr("normals"), ptr("joints", np.int32), ptr("weights"), ptr("inverse_bind"), ptr("target_positions"),
                               ptr("target_normals"), ptr("joint_xforms"), ptr("target_weights"), grid, out_p.ctypes.data, None if out_n is None else out_n.ctypes.data)
    assert rc == 0, f"a write outside the output arrays ({rc})"
    return out_p, out_n


def differing(a, b):
    """how many doubles of a and b differ in any bit"""
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))


def ref_pose(case):
    return skin_ref.pose(**case)


def all_cases():
    return skin_ref.cases(host().skin_host_lds_max_joints())


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_host_build_equals_the_restatement_bit_for_bit():
    cases = all_cases()
    assert len(cases) >= 40
    sizes, ks, ts = set(), set(), set()
    for name, grid, case in cases:
        got_p, got_n = host_pose(case, grid)
        want_p, want_n = ref_pose(case)
        assert differing(got_p, want_p) == 0, f"{name}: positions"
        assert (got_n is None) == (want_n is None), name
        if want_n is not None:
            assert differing(got_n, want_n) == 0, f"{name}: normals"
        sizes.add(case["positions"].shape[0])
        ks.add(0 if case.get("joints") is None else case["joints"].shape[1])
        ts.add(0 if case.get("target_positions") is None else case["target_positions"].shape[0])
    assert sizes >= set(skin_ref.SIZES) and ks >= {0, 1, 4, 8} and ts >= {0, 1, 3}


def test_the_hard_inputs_are_what_they_claim():
    """the mirrored joint has det < 0 somewhere, the zero normals stay zero, the unnormalised weights do not sum to 1"""
    by_name = {name: case for name, _, case in all_cases()}
    m = by_name["mirror"]
    J = skin_ref.palette(m["joint_xforms"], m.get("inverse_bind"))
    assert np.linalg.det(J[0][:, :3]) < 0 and (m["joints"][:, 0] == 0).any()
    z = by_name["zero_normal"]
    _, n = host_pose(z)
    assert not z["normals"][::3].any() and not n[::3].any() and np.allclose(np.linalg.norm(n[1::3], axis=1), 1.0)
    u = by_name["unnormalised"]
    assert np.abs(u["weights"].sum(axis=1) - 1.0).max() > 0.1
    s = by_name["scale"]
    sv = np.linalg.svd(s["joint_xforms"][:, :, :3], compute_uv=False)
    assert (sv[:, 0] / sv[:, 2]).max() > 2


def test_identity_joints_with_binary_fraction_weights_return_the_rest_pose():
    rng = np.random.default_rng(5)
    nv = 257
    pos = rng.uniform(-3, 3, (nv, 3))
    nrm = np.zeros((nv, 3))
    nrm[np.arange(nv), np.arange(nv) % 3] = 1.0
    eye = np.tile(np.eye(3, 4), (4, 1, 1))
    case = {"positions": pos, "normals": nrm, "joints": rng.integers(0, 4, (nv, 4)).astype(np.int32), "weights": np.tile([0.5, 0.25, 0.25, 0.0], (nv, 1)),
            "joint_xforms": eye}
    p, n = host_pose(case)
    assert differing(p, pos) == 0 and differing(n, nrm) == 0
    case["inverse_bind"] = eye
    p, n = host_pose(case)
    assert differing(p, pos) == 0 and differing(n, nrm) == 0


def test_one_influence_of_weight_one_applies_the_palette_matrix():
    rng = np.random.default_rng(6)
    nv, nj = 65, 3
    case = skin_ref.make_case(nv, nj, 1, 0, normals=False, seed=6)
    case["weights"] = np.ones((nv, 1))
    p, _ = host_pose(case)
    J = skin_ref.palette(case["joint_xforms"], case["inverse_bind"])
    M = J[case["joints"][:, 0]]
    q = case["positions"]
    want = np.stack([((M[:, r, 0] * q[:, 0] + M[:, r, 1] * q[:, 1]) + M[:, r, 2] * q[:, 2]) + M[:, r, 3] for r in range(3)], axis=1)
    assert differing(p, want) == 0


def test_morph_only_rig_with_zero_weights_returns_the_rest_pose():
    case = skin_ref.make_case(257, 0, 0, 3, normals=False, seed=7)
    case["target_weights"] = np.zeros(3)
    p, _ = host_pose(case)
    assert differing(p, case["positions"]) == 0


def test_control_swapping_two_influences_changes_bits():
    """the comparison is not blind: the sum over influences is ordered, and the other order shows"""
    case = skin_ref.make_case(257, 6, 4, 0, seed=8)
    case["weights"] = np.tile([0.37, 0.29, 0.21, 0.13], (257, 1))
    swapped = dict(case)
    order = [2, 1, 0, 3]
    swapped["joints"], swapped["weights"] = case["joints"][:, order].copy(), case["weights"][:, order].copy()
    p, n = host_pose(case)
    q, m = host_pose(swapped)
    assert differing(p, q) > 0, "swapping influences 0 and 2 changed no bit of the positions"
    want_p, want_n = ref_pose(swapped)
    assert differing(q, want_p) == 0 and differing(m, want_n) == 0
    assert differing(p, want_p) > 0


@pytest.mark.parametrize("kind", ["scale", "mirror"])
def test_posed_normals_stay_perpendicular_to_posed_edges(kind):
    """A flat patch under ONE joint that is scaled non-uniformly / mirrored: the posed normal against the two posed edge
    vectors.  Inputs are O(1); the chain from the inputs to dot(n', e) is a few dozen roundings of relative size 2^-53
    each, hence |dot(n', e)| <= 256 * 2^-52 * |e|."""
    rng = np.random.default_rng(9)
    scale = (0.4, 1.0, 2.5) if kind == "scale" else (-1.0, 0.7, 1.3)
    X = skin_ref.affine(rng, scale)[None]
    if kind == "mirror":
        assert np.linalg.det(X[0][:, :3]) < 0
    worst = 0.0
    for trial in range(64):
        a, e1, e2 = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        e1, e2 = e1 * (rng.uniform(0.5, 1.5) / np.linalg.norm(e1)), e2 * (rng.uniform(0.5, 1.5) / np.linalg.norm(e2))  # (edges of magnitude O(1))
        nrm = np.cross(e1, e2)
        nrm /= np.linalg.norm(nrm)
        case = {"positions": np.stack([a, a + e1, a + e2]), "normals": np.tile(nrm, (3, 1)), "joints": np.zeros((3, 1), np.int32), "weights": np.ones((3, 1)),
                "joint_xforms": X}
        p, n = host_pose(case)
        assert abs(np.linalg.norm(n[0]) - 1.0) < 1e-15
        for e in (p[1] - p[0], p[2] - p[0]):
            d = abs(float(np.dot(n[0], e)))
            worst = max(worst, d / np.linalg.norm(e))
            assert d <= 256 * 2.0**-52 * np.linalg.norm(e), f"{kind}, trial {trial}: |dot| {d:.3e}"
        # the normal keeps its side: for a mirrored joint the determinant's sign is what keeps it
        if kind == "mirror":
            assert np.dot(n[0], np.cross(p[1] - p[0], p[2] - p[0])) < 0  # (a mirrored patch: its winding turned, the normal did not)
    print(f"{kind}: the largest |dot(n', e)| / |e| over 128 edges is {worst * 2.0**52:.2f} * 2^-52 (bound 256 * 2^-52)")


def test_joint_check_reports_the_smallest_bad_vertex():
    rng = np.random.default_rng(10)
    joints = rng.integers(0, 4, (1301, 4)).astype(np.int32)
    assert host().skin_host_check_joints(joints.ctypes.data, 4, 4, 1301, 0) == -1
    joints[900, 1], joints[411, 3], joints[1300, 0] = 4, -1, 7
    for grid in (0, 1, 2, 3):
        assert host().skin_host_check_joints(joints.ctypes.data, 4, 4, 1301, grid) == 411


# ------------------------------------------------------------------------------------------------ the API
@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_symbols_exist(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    assert callable(capi.Rig.pose) and callable(capi.Rig.pose_device) and callable(capi.Rig.info) and callable(capi.Scene.pose_meshes)
    assert lib.take_hip_abi_version() == 5


def test_struct_layouts_match_the_header():
    fields = {"TakeRigDesc": D.TakeRigDesc, "TakeRigPose": D.TakeRigPose, "TakeRigBinding": D.TakeRigBinding}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){"]
    for n, cls in fields.items():
        prog.append(f'printf("{n} %zu\\n", sizeof({n}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{n}.{fname} %zu\\n", offsetof({n}, {fname}));')
    prog.append('printf("flags %d %d\\n", TAKE_RIG_DEVICE_ARRAYS, TAKE_RIG_POSE_DEVICE_ARRAYS);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write("\n".join(prog))
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    assert lines[-1] == ["flags", str(D.TAKE_RIG_DEVICE_ARRAYS), str(D.TAKE_RIG_POSE_DEVICE_ARRAYS)]
    want = dict(lines[:-1])
    for n, cls in fields.items():
        assert C.sizeof(cls) == int(want[n]), n
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == int(want[f"{n}.{fname}"]), f"{n}.{fname}"


def rig_desc(**over):
    """a valid 4-vertex, 2-joint, K = 2, one-target description over host arrays (kept alive on the struct)"""
    nv = 4
    a = {"positions": np.zeros((nv, 3)), "normals": np.tile([0.0, 0.0, 1.0], (nv, 1)), "joints": np.zeros((nv, 2), np.int32), "weights": np.full((nv, 2), 0.5),
         "inverse_bind": np.tile(np.eye(3, 4), (2, 1, 1)), "target_positions": np.zeros((1, nv, 3)), "target_normals": np.zeros((1, nv, 3))}
    d = D.TakeRigDesc()
    d.n_vertices, d.n_joints, d.n_influences, d.n_targets, d.flags = nv, 2, 2, 1, 0
    for k, v in a.items():
        setattr(d, k, v.ctypes.data)
    d._keep = a
    for k, v in over.items():
        setattr(d, k, v)
    return d


CREATE_REFUSALS = [
    ({"n_vertices": 0}, b"n_vertices must be positive"),
    ({"n_vertices": -3}, b"n_vertices must be positive"),
    ({"n_joints": -1}, b"must not be negative"),
    ({"n_targets": -1}, b"must not be negative"),
    ({"n_influences": 0}, b"n_influences must be 1..8"),
    ({"n_influences": 9}, b"n_influences must be 1..8"),
    ({"n_joints": 0}, b"n_influences must be 0"),
    ({"positions": None}, b"positions is null"),
    ({"joints": None}, b"joints and weights are required"),
    ({"weights": None}, b"joints and weights are required"),
    ({"target_positions": None}, b"target_positions is required"),
    ({"normals": None}, b"target_normals given for a rig without normals"),
    ({"flags": 2}, b"unknown flag bits"),
    ({"flags": D.TAKE_RIG_DEVICE_ARRAYS | 4}, b"unknown flag bits"),
]


@pytest.mark.parametrize("over,message", CREATE_REFUSALS)
def test_rig_create_refusals_before_a_device_is_looked_for(lib, over, message):
    out = C.c_void_p()
    d = rig_desc(**over)
    assert lib.take_hip_rig_create(C.byref(d), C.byref(out)) == D.TAKE_E_INVALID
    assert message in lib.take_hip_last_error(), lib.take_hip_last_error()
    assert not out.value


def test_null_arguments_are_refused_before_a_device_is_looked_for(lib):
    out = C.c_void_p()
    d = rig_desc()
    pose = D.TakeRigPose()
    buf = np.zeros((4, 3))
    fake = C.c_void_p(buf.ctypes.data)  # (never dereferenced: the other argument is refused first)
    for rc in (lib.take_hip_rig_create(None, C.byref(out)), lib.take_hip_rig_create(C.byref(d), None), lib.take_hip_rig_destroy(None),
               lib.take_hip_rig_info(None, None, None, None, None, None, None), lib.take_hip_rig_pose(None, C.byref(pose), buf.ctypes.data, None),
               lib.take_hip_rig_pose_device(None, C.byref(pose), buf.ctypes.data, None, None), lib.take_hip_scene_pose_meshes(None, None, 1),
               lib.take_hip_scene_pose_meshes(fake, None, 1)):
        assert rc == D.TAKE_E_INVALID
        assert b"null argument" in lib.take_hip_last_error()
    b = (D.TakeRigBinding * 2)()
    assert lib.take_hip_scene_pose_meshes(fake, b, 0) == D.TAKE_E_INVALID and b"n must be positive" in lib.take_hip_last_error()
    b[0].mesh = -1
    assert lib.take_hip_scene_pose_meshes(fake, b, 1) == D.TAKE_E_INVALID and b"binding 0: mesh index out of range" in lib.take_hip_last_error()
    b[0].mesh = 0
    assert lib.take_hip_scene_pose_meshes(fake, b, 1) == D.TAKE_E_INVALID and b"binding 0: null argument" in lib.take_hip_last_error()  # (no rig)


def test_valid_arguments_without_a_gpu_are_no_gpu(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the no-GPU contract is checked in the CPU container")
    out = C.c_void_p()
    d = rig_desc()
    assert lib.take_hip_rig_create(C.byref(d), C.byref(out)) == D.TAKE_E_NO_GPU
    assert b"no CPU path" in lib.take_hip_last_error() and not out.value
    d = rig_desc(n_joints=0, n_influences=0, n_targets=0)  # a rest pose alone is a valid (if idle) rig
    assert lib.take_hip_rig_create(C.byref(d), C.byref(out)) == D.TAKE_E_NO_GPU
    with pytest.raises(capi.TakeError) as e:
        capi.Rig(np.zeros((4, 3)), joints=np.zeros((4, 1), np.int32), weights=np.ones((4, 1)))
    assert e.value.code == D.TAKE_E_NO_GPU


def test_python_wrapper_refuses_mismatched_shapes():
    with pytest.raises(ValueError, match="normals must have shape"):
        capi.Rig(np.zeros((4, 3)), normals=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="joints and weights go together"):
        capi.Rig(np.zeros((4, 3)), joints=np.zeros((4, 1), np.int32))
    with pytest.raises(ValueError, match="weights must have shape"):
        capi.Rig(np.zeros((4, 3)), joints=np.zeros((4, 2), np.int32), weights=np.ones((4, 1)))
    with pytest.raises(ValueError, match="target_normals without target_positions"):
        capi.Rig(np.zeros((4, 3)), target_normals=np.zeros((1, 4, 3)))

"""CPU side of Loop subdivision on the device (take_hip_subdiv_*, take_hip_scene_subdivide_meshes, include/take_hip.h;
DESIGN.md §4s):

1. The kernels' bodies and the topology build (take_amd/csrc/tk_subdiv.h) without a GPU: tests/subdiv_host builds them
   for the host and runs them in the launches' loop structure; they equal tests/subdiv_ref.py — a numpy restatement
   written from the specification — bit for bit over the shared cages, at every level and every grid.
2. The real library without a GPU: counts and topology, every refusal that needs no device, the ABI version.
3. Properties that do not lean on the restatement: Euler characteristic, the bounding box, the octahedron's symmetry,
   unit normals, the sanitizer build.
"""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import subdiv_ref
from take_amd import capi
from take_amd import cdefs as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ["take_hip_subdiv_counts", "take_hip_subdiv_topology", "take_hip_subdiv_create", "take_hip_subdiv_destroy", "take_hip_subdiv_info",
           "take_hip_subdiv_refine_device", "take_hip_subdiv_refine", "take_hip_scene_subdivide_meshes"]

_HOST = None


def host():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "subdiv_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libsubdiv_host.so"))
        L.subdiv_host_message.restype = C.c_char_p
        L.subdiv_host_counts.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.subdiv_host_refine.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        _HOST = L
    return _HOST


def host_refine(positions, indices, levels, uvs=None, grid=0, normals=True):
    """tk_subdiv.h on the host -> (positions, normals or None, indices, uvs or None)"""
    pos, idx = np.ascontiguousarray(positions, np.float64), np.ascontiguousarray(indices, np.int32)
    uv = None if uvs is None else np.ascontiguousarray(uvs, np.float64)
    nv, nf = C.c_int64(), C.c_int64()
    rc = host().subdiv_host_counts(pos.shape[0], idx.shape[0], idx.ctypes.data, levels, C.byref(nv), C.byref(nf))
    assert rc == 0, host().subdiv_host_message()
    out_p, out_n = np.zeros((nv.value, 3)), (np.zeros((nv.value, 3)) if normals else None)
    out_idx, out_uv = np.zeros((nf.value, 3), np.int32), (None if uv is None else np.zeros((nv.value, 2)))
    rc = host().subdiv_host_refine(pos.shape[0], idx.shape[0], idx.ctypes.data, None if uv is None else uv.ctypes.data, levels, pos.ctypes.data, grid, out_idx.ctypes.data,
                                   None if out_uv is None else out_uv.ctypes.data, out_p.ctypes.data, None if out_n is None else out_n.ctypes.data)
    assert rc == 0, f"a write outside the output arrays, or a refusal ({rc}: {host().subdiv_host_message()})"
    return out_p, out_n, out_idx, out_uv


def differing(a, b):
    """how many doubles of a and b differ in any bit"""
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))


@functools.lru_cache(maxsize=None)
def restated():
    """{(name, levels): (positions, normals, indices, uvs)} by the restatement: computed once, shared, never written"""
    out = {}
    for name, pos, idx, uv, levels in subdiv_ref.cases():
        for L in levels:
            p, n, i = subdiv_ref.refine(pos, idx, L)
            _, _, u = subdiv_ref.topology(idx, pos.shape[0], L, uv)
            for a in (p, n, i):
                a.setflags(write=False)
            out[(name, L)] = (p, n, i, u)
    return out


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_the_cases_have_the_counts_the_specification_lists():
    seen = {}
    for (name, L), (p, _, idx, _) in restated().items():
        seen.setdefault(name, {})[L] = p.shape[0]
        assert idx.max() == p.shape[0] - 1 or name == "strip9-unused-vertex"
    for name, counts in subdiv_ref.COUNTS.items():
        for L, nv in seen[name].items():
            assert nv == counts[L - 1], (name, L)
    assert set(seen["octahedron"]) == {1, 2, 3, 4} and set(seen["closed-fan200"]) == {2}


def test_host_build_equals_the_restatement_bit_for_bit():
    for name, pos, idx, uv, levels in subdiv_ref.cases():
        for L in levels:
            want_p, want_n, want_idx, want_uv = restated()[(name, L)]
            for grid in (0, 1, 2, 3):
                got_p, got_n, got_idx, got_uv = host_refine(pos, idx, L, uvs=uv, grid=grid)
                assert np.array_equal(got_idx, want_idx), f"{name} L{L}: indices"
                assert differing(got_p, want_p) == 0, f"{name} L{L} grid {grid}: positions"
                assert differing(got_n, want_n) == 0, f"{name} L{L} grid {grid}: normals"
                if uv is not None:
                    assert differing(got_uv, want_uv) == 0, f"{name} L{L}: uvs"
                    assert differing(got_uv[:uv.shape[0]], uv) == 0


def test_the_unused_vertex_is_copied_and_has_a_zero_normal():
    name, pos, idx, _, _ = next(c for c in subdiv_ref.cases() if c[0] == "strip9-unused-vertex")
    p, n, _, _ = host_refine(pos, idx, 2)
    assert differing(p[9], pos[9]) == 0 and not n[9].any()
    assert np.abs(p[:9] - pos[:9]).max() > 1e-3  # (the others moved)


def test_inconsistent_orientation_changes_no_position():
    """no weight reads orientation: the strip with one face flipped refines to the same positions; its normals differ"""
    by = {c[0]: c for c in subdiv_ref.cases()}
    _, pos, idx, _, _ = by["strip23"]
    _, _, flipped, _, _ = by["strip23-flipped-face"]
    p, n, _, _ = host_refine(pos, idx, 2)
    q, m, _, _ = host_refine(pos, flipped, 2)
    assert differing(p, q) == 0 and differing(n, m) > 0


def test_control_another_neighbour_order_changes_bits():
    """the comparison is not blind: the sum over neighbours is ordered, and a relabelled cage shows it"""
    pos, idx = subdiv_ref.octahedron()
    pos = pos * np.array([1.0, 0.8, 1.3]) + np.array([0.1, 0.37, 0.013])
    perm = np.array([3, 5, 0, 4, 1, 2])
    inv = np.argsort(perm)
    p, _, _, _ = host_refine(pos, idx, 1, normals=False)
    q, _, _, _ = host_refine(pos[perm], inv[idx].astype(np.int32), 1, normals=False)
    assert np.abs(p[:6] - q[inv]).max() < 1e-15 and differing(p[:6], q[inv]) > 0


# ------------------------------------------------------------------------------------------------ properties
def euler(indices, n_vertices):
    lo, hi, c, d, _ = subdiv_ref.edges(indices, n_vertices)
    return n_vertices - len(lo) + len(indices), int((d < 0).sum())


@pytest.mark.parametrize("name", ["octahedron", "tetrahedron", "strip23", "open-fan7", "closed-fan200"])
def test_euler_characteristic_is_kept_and_a_closed_cage_stays_closed(name):
    _, pos, idx, _, levels = next(c for c in subdiv_ref.cases() if c[0] == name)
    chi0, open0 = euler(idx, pos.shape[0])
    assert chi0 == (2 if name in ("octahedron", "tetrahedron") else 1)
    for L in levels:
        p, _, i, _ = host_refine(pos, idx, L, normals=False)
        chi, boundary = euler(i, p.shape[0])
        assert chi == chi0, (name, L)
        assert (boundary == 0) == (open0 == 0) and boundary == open0 * 2**L


def test_refined_positions_stay_in_the_cages_bounding_box():
    """every weight is non-negative and a vertex's weights sum to 1: a refined position is a convex combination, up to
    rounding — 4 ulp of the largest coordinate"""
    for name, pos, idx, _, levels in subdiv_ref.cases():
        slack = 4 * np.spacing(np.abs(pos).max())
        for L in levels:
            p, _, _, _ = host_refine(pos, idx, L, normals=False)
            assert (p >= pos.min(axis=0) - slack).all() and (p <= pos.max(axis=0) + slack).all(), (name, L)


def test_octahedron_keeps_its_48_fold_symmetry():
    pos, idx = subdiv_ref.octahedron()
    for L in (1, 2, 3):
        p, _, _, _ = host_refine(pos, idx, L, normals=False)
        for perm in itertools.permutations(range(3)):
            for signs in itertools.product((1.0, -1.0), repeat=3):
                q = p[:, perm] * np.array(signs)
                d = np.abs(q[:, None, :] - p[None, :, :]).max(axis=2)  # every image of a vertex is a vertex, and each is hit once
                assert d.min(axis=1).max() <= 1e-14, (L, perm, signs)
                assert len(set(d.argmin(axis=1))) == p.shape[0], (L, perm, signs)


def test_normals_have_unit_length_or_are_exactly_zero():
    for (name, L), (p, n, _, _) in restated().items():
        got = host_refine(*next((c[1], c[2]) for c in subdiv_ref.cases() if c[0] == name), L)[1]
        length = np.sqrt((got * got).sum(axis=1))
        zero = ~got.any(axis=1)
        assert (np.abs(length[~zero] - 1.0) <= 2 * np.spacing(1.0)).all(), (name, L)
        assert zero.sum() == (1 if name == "strip9-unused-vertex" else 0)


def test_octahedron_normals_point_outwards():
    pos, idx = subdiv_ref.octahedron()
    p, n, _, _ = host_refine(pos, idx, 3)
    assert ((p * n).sum(axis=1) > 0.9 * np.linalg.norm(p, axis=1)).all()


def test_sanitizer_build_runs_clean():
    r = subprocess.run(["make", "-C", os.path.join(HERE, "subdiv_host"), "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and ", 0 mismatches" in r.stdout, r.stdout[-3000:]


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_symbols_exist_and_the_abi_version_stays(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    assert callable(capi.Subdiv.refine) and callable(capi.Subdiv.refine_device) and callable(capi.Subdiv.info) and callable(capi.Subdiv.topology)
    assert callable(capi.Scene.subdivide_meshes)
    assert lib.take_hip_abi_version() == 5


def test_struct_layouts_match_the_header():
    import tempfile

    fields = {"TakeSubdivDesc": D.TakeSubdivDesc, "TakeSubdivBinding": D.TakeSubdivBinding}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){"]
    for n, cls in fields.items():
        prog.append(f'printf("{n} %zu\\n", sizeof({n}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{n}.{fname} %zu\\n", offsetof({n}, {fname}));')
    prog.append('printf("flags %d\\n", TAKE_SUBDIV_DEVICE_ARRAYS);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write("\n".join(prog))
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    assert lines[-1] == ["flags", str(D.TAKE_SUBDIV_DEVICE_ARRAYS)]
    want = dict(lines[:-1])
    for n, cls in fields.items():
        assert C.sizeof(cls) == int(want[n]), n
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == int(want[f"{n}.{fname}"]), f"{n}.{fname}"


def test_counts_and_topology_equal_the_restatement(lib):
    for name, pos, idx, uv, levels in subdiv_ref.cases():
        for L in levels:
            _, _, want_idx, want_uv = restated()[(name, L)]
            want_nv = restated()[(name, L)][0].shape[0]
            assert capi.subdiv_counts(idx, pos.shape[0], L) == (want_nv, want_idx.shape[0]), (name, L)
            got_idx, got_uv = capi.subdiv_topology(idx, pos.shape[0], L, uvs=uv)
            assert np.array_equal(got_idx, want_idx), (name, L)
            assert (got_uv is None) == (uv is None)
            if uv is not None:
                assert differing(got_uv, want_uv) == 0


def desc(idx, n_vertices, levels, flags=0):
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    d = D.TakeSubdivDesc()
    d.n_vertices, d.n_faces, d.indices, d.levels, d.flags = n_vertices, idx.shape[0], idx.ctypes.data, levels, flags
    d._keep = idx
    return d


STRIP9 = subdiv_ref.strip(9)[1]
CREATE_REFUSALS = [
    ("index-range", desc([[0, 1, 2], [2, 1, 5]], 5, 1), b"level 0: face 1: vertex index 5 out of range"),
    ("index-negative", desc([[0, -1, 2]], 5, 1), b"level 0: face 0: vertex index -1 out of range"),
    ("repeated", desc([[0, 1, 2], [3, 1, 3]], 5, 1), b"level 0: face 1 repeats vertex 3"),
    ("three-faces", desc([[0, 1, 2], [1, 0, 3], [0, 1, 4]], 5, 1), b"level 0: edge (0, 1) has more than two faces"),
    ("bow-tie", desc([[0, 1, 2], [2, 3, 4]], 5, 1), b"level 0: vertex 2 is on 4 boundary edges"),
    ("levels-0", desc(STRIP9, 9, 0), b"levels must be 1..6"),
    ("levels-7", desc(STRIP9, 9, 7), b"levels must be 1..6"),
    ("flags", desc(STRIP9, 9, 1, flags=1), b"unknown flag bits"),
    ("no-vertices", desc(STRIP9, 0, 1), b"must be positive"),
]


@pytest.mark.parametrize("name,d,message", CREATE_REFUSALS, ids=[r[0] for r in CREATE_REFUSALS])
def test_refusals_of_a_description_before_a_device_is_looked_for(lib, name, d, message):
    nv, nf, out = C.c_int64(), C.c_int64(), C.c_void_p()
    idx_out = np.zeros((64, 3), np.int32)  # (never written: refused first)
    for rc in (lib.take_hip_subdiv_counts(C.byref(d), C.byref(nv), C.byref(nf)), lib.take_hip_subdiv_topology(C.byref(d), idx_out.ctypes.data, None),
               lib.take_hip_subdiv_create(C.byref(d), C.byref(out))):
        assert rc == D.TAKE_E_INVALID
        assert message in lib.take_hip_last_error(), lib.take_hip_last_error()
    assert not out.value


def test_counts_beyond_32_bit_indices_are_unsupported(lib):
    _, idx = subdiv_ref.strip(180_002)  # 180000 faces: 3 * 4^6 * 180000 > INT32_MAX
    d = desc(idx, 180_002, 6)
    nv, nf, out = C.c_int64(), C.c_int64(), C.c_void_p()
    for rc in (lib.take_hip_subdiv_counts(C.byref(d), C.byref(nv), C.byref(nf)), lib.take_hip_subdiv_create(C.byref(d), C.byref(out))):
        assert rc == D.TAKE_E_INVALID and lib.take_hip_last_error().startswith(b"unsupported"), lib.take_hip_last_error()
    d = desc(idx, 180_002, 1)
    assert lib.take_hip_subdiv_counts(C.byref(d), C.byref(nv), C.byref(nf)) == 0 and nf.value == 720_000


def test_null_arguments_and_bindings_are_refused_before_a_device_is_looked_for(lib):
    out = C.c_void_p()
    d = desc(STRIP9, 9, 1)
    buf = np.zeros((64, 3))
    fake = C.c_void_p(buf.ctypes.data)  # (never dereferenced: refused first)
    no_indices = desc(STRIP9, 9, 1)
    no_indices.indices = None
    for rc in (lib.take_hip_subdiv_create(None, C.byref(out)), lib.take_hip_subdiv_create(C.byref(d), None), lib.take_hip_subdiv_create(C.byref(no_indices), C.byref(out)),
               lib.take_hip_subdiv_counts(None, None, None), lib.take_hip_subdiv_topology(C.byref(d), None, None), lib.take_hip_subdiv_destroy(None),
               lib.take_hip_subdiv_info(None, None, None, None, None, None), lib.take_hip_subdiv_refine(None, buf.ctypes.data, buf.ctypes.data, None),
               lib.take_hip_subdiv_refine_device(None, buf.ctypes.data, 0, buf.ctypes.data, None, None), lib.take_hip_scene_subdivide_meshes(None, None, 1),
               lib.take_hip_scene_subdivide_meshes(fake, None, 1)):
        assert rc == D.TAKE_E_INVALID
        assert b"null argument" in lib.take_hip_last_error()
    uv_out = np.zeros((64, 2))
    assert lib.take_hip_subdiv_topology(C.byref(d), buf.ctypes.data, uv_out.ctypes.data) == D.TAKE_E_INVALID and b"uvs wanted from a cage without uvs" in lib.take_hip_last_error()
    b = (D.TakeSubdivBinding * 2)()

    def refused(n, message):
        assert lib.take_hip_scene_subdivide_meshes(fake, b, n) == D.TAKE_E_INVALID
        assert message in lib.take_hip_last_error(), lib.take_hip_last_error()

    refused(0, b"n must be positive")
    b[0].mesh = -1
    refused(1, b"binding 0: mesh index out of range")
    b[0].mesh = 0
    refused(1, b"binding 0: null argument")  # (no handle)
    b[0].subdiv = fake
    refused(1, b"binding 0: exactly one of cage_positions and rig")  # neither
    b[0].cage_positions, b[0].rig = buf.ctypes.data, fake
    refused(1, b"binding 0: exactly one of cage_positions and rig")  # both
    b[0].rig, b[0].flags = None, 2
    refused(1, b"binding 0: unknown flag bits")
    b[0].flags = 0
    b[1].mesh, b[1].subdiv, b[1].cage_positions = 0, buf.ctypes.data + 8, buf.ctypes.data
    refused(2, b"mesh 0 appears more than once")
    b[1].mesh, b[1].subdiv = 1, fake
    refused(2, b"a subdivision handle is bound more than once")


def test_valid_arguments_without_a_gpu_are_no_gpu(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the no-GPU contract is checked in the CPU container")
    out = C.c_void_p()
    d = desc(STRIP9, 9, 2)
    assert lib.take_hip_subdiv_create(C.byref(d), C.byref(out)) == D.TAKE_E_NO_GPU
    assert b"no CPU path" in lib.take_hip_last_error() and not out.value
    with pytest.raises(capi.TakeError) as e:
        capi.Subdiv(STRIP9, 9, 2)
    assert e.value.code == D.TAKE_E_NO_GPU


def test_python_wrapper_refuses_mismatched_shapes():
    with pytest.raises(ValueError, match="indices must have shape"):
        capi.subdiv_counts(np.zeros((4, 2), np.int32), 9, 1)
    with pytest.raises(ValueError, match="uvs must have shape"):
        capi.subdiv_topology(STRIP9, 9, 1, uvs=np.zeros((8, 2)))


# ------------------------------------------------------------------------------------------------ the CLI's description
def test_a_description_with_refined_meshes_keeps_its_shapes_and_lights_in_order():
    """-subdivide: face f becomes the faces 4^L f .. 4^L (f + 1) - 1, each a shape in the old shape's place; an area light
    on a face becomes one light per new face; spheres, other meshes and other lights keep their order"""
    from take_amd.render import with_refined_meshes
    from take_amd.scene import Light, SceneData

    sd = SceneData(width=8, height=8)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7))
    pos, idx = subdiv_ref.strip(5)
    sd.lights.append(Light(0, -1, (1.0, 1.0, 1.0), (0.0, 2.0, 0.0)))
    sd.add_sphere((0.0, 1.0, 0.0), 0.25, grey, emission=(2.0, 2.0, 2.0))
    sd.add_mesh(pos, idx, grey, normals=np.tile([0.0, 0.0, 1.0], (5, 1)), emission=(3.0, 3.0, 3.0))  # the mesh that is refined
    sd.add_mesh(pos + 2.0, idx, grey)  # one that is left
    L = 2
    p, n, i, _ = host_refine(pos, idx, L)
    out = with_refined_meshes(sd, {0: (p, i, n, None)}, L)
    k = 4**L
    assert out.n_shapes == 1 + 3 * k + 3 and len(out.lights) == 1 + 1 + 3 * k
    assert list(out.shape_kind) == [0] + [1] * (3 * k + 3) and list(out.shape_ref) == [0] + [0] * (3 * k) + [1] * 3
    assert list(out.shape_face) == [0] + list(range(3 * k)) + [0, 1, 2]
    assert list(out.shape_area_light) == [1] + list(range(2, 2 + 3 * k)) + [-1] * 3
    assert [(light.kind, light.shape_id) for light in out.lights] == [(0, -1), (1, 0)] + [(1, 1 + f) for f in range(3 * k)]
    assert all(light.intensity == (3.0, 3.0, 3.0) for light in out.lights[2:])
    assert np.array_equal(out.meshes[0].indices, i) and differing(out.meshes[0].normals, n) == 0 and out.meshes[1] is sd.meshes[1]
    assert sd.n_shapes == 7 and len(sd.lights) == 5  # (the description that went in is as it was)
    # every new face lies on the old face it came from: the children of face f are the faces 4^L f ..
    _, _, i1, _ = host_refine(pos, idx, 1)
    assert set(i1[4:8].ravel()) & set(idx[1]) == set(idx[1])

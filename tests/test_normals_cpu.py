"""compute_normals, CPU side (take_hip_compute_normals / take_hip_mesh_compute_normals): the host build of the device
header take_amd/csrc/tk_normals.h (tests/normals_shim) and the numpy restatement (tests/normals_ref.py) against the
normals the reference's OWN compute_normals gave the committed meshes (tests/golden/normals, written by
tools/gen_normals_golden.py through oracle/_ref/ref_harness), bit for bit; the two against each other on generated
meshes; the reference's rules one by one; the library's exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import normals_ref
from helpers import GOLD, HERE
from take_amd import capi
from take_amd import cdefs as D

NRM = os.path.join(GOLD, "normals")
CASES = sorted(f[:-len("_mesh.f64")] for f in os.listdir(NRM) if f.endswith("_mesh.f64"))

_SHIM = None


def shim():
    global _SHIM
    if _SHIM is None:
        d = os.path.join(HERE, "normals_shim")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libnormals_shim.so"))
        L.normals_shim_compute.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        L.normals_shim_face.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _SHIM = L
    return _SHIM


def shim_normals(positions, indices):
    pos = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    out = np.full(pos.shape, np.nan)
    if shim().normals_shim_compute(pos.ctypes.data, pos.shape[0], idx.ctypes.data, idx.shape[0], out.ctypes.data) != 0:
        raise IndexError("vertex index out of range")
    return out


def shim_face(positions, face):
    pos = np.ascontiguousarray(positions, np.float64)
    f = np.ascontiguousarray(face, np.int32)
    out = np.full((3, 3), np.nan)
    return shim().normals_shim_face(pos.ctypes.data, f.ctypes.data, out.ctypes.data) == 1, out


def load_case(name):
    """-> (positions, indices, the reference's normals)"""
    a = np.fromfile(os.path.join(NRM, name + "_mesh.f64"), "<f8")
    nv, nf = int(a[0]), int(a[1])
    o = 2
    pos = a[o:o + 3 * nv].reshape(nv, 3)
    o += 3 * nv
    idx = a[o:o + 3 * nf].reshape(nf, 3).astype(np.int32)
    o += 3 * nf
    nrm = a[o:o + 3 * nv].reshape(nv, 3)
    assert o + 3 * nv == a.size
    return pos, idx, nrm


def assert_bits(got, want):
    """equal as bit patterns: -0.0 is not +0.0"""
    assert got.shape == want.shape
    g, w = got.view(np.uint64), want.view(np.uint64)
    bad = np.nonzero(g != w)
    assert bad[0].size == 0, f"{bad[0].size} components differ, first at {bad[0][0]}: {got[bad][0]!r} != {want[bad][0]!r}"


def soup(nf, nv, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (nv, 3)), rng.integers(0, nv, (nf, 3)).astype(np.int32)


def jittered_grid(nx, ny, seed):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx, dtype=float), np.arange(ny, dtype=float))
    p = np.stack([x + rng.uniform(-0.4, 0.4, x.shape), 0.3 * y + rng.uniform(-0.1, 0.1, y.shape),
                  rng.uniform(-0.3, 0.3, x.shape)], axis=-1).reshape(-1, 3)
    a = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)])
    return p, f.astype(np.int32)


def fan(n, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    rim = np.stack([np.cos(t), np.sin(t), rng.uniform(-0.5, 0.5, n)], 1)
    p = np.concatenate([[[0.0, 0.0, 0.3]], rim])
    i = np.arange(n)
    return p, np.stack([np.zeros(n, int), 1 + i, 1 + (i + 1) % n], 1).astype(np.int32)


def test_fixture_set_covers_the_issue_cases():
    assert {"closed", "obtuse", "planar", "degenerate", "unreferenced", "cancelling", "fan"} <= set(CASES)


def test_fixtures_exercise_what_they_are_named_for():
    # obtuse: corners where unit_angle takes the dot < 0 branch; closed: none
    for name, want in (("obtuse", True), ("closed", False)):
        p, f, _ = load_case(name)
        q = p[f]
        obt = [normals_ref.dot(normals_ref.normalize(q[:, (i + 1) % 3] - q[:, i]), normals_ref.normalize(q[:, (i + 2) % 3] - q[:, i])) < 0
               for i in range(3)]
        assert np.any(obt) == want, name
    # planar: face normals with signed-zero components of both signs
    p, f, _ = load_case("planar")
    n = normals_ref.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert np.all(p[:, 2] == 0) and np.any(np.signbit(n[:, :2])) and np.any(~np.signbit(n[:, :2]))
    # degenerate: zero-area faces; unreferenced: an unused vertex; cancelling: a sum of exactly zero; fan: valence 2000
    p, f, r = load_case("degenerate")
    assert sum(not shim_face(p, face)[0] for face in f) == 3
    p, f, r = load_case("unreferenced")
    assert 3 not in f and np.array_equal(r[3], np.zeros(3)) and not np.any(np.signbit(r[3]))
    p, f, r = load_case("cancelling")
    assert np.array_equal(r[0], np.zeros(3)) and not np.any(np.signbit(r[0]))
    p, f, r = load_case("fan")
    assert np.count_nonzero(f == 0) == 2000


@pytest.mark.parametrize("name", CASES)
def test_host_build_of_the_kernels_matches_the_reference_bit_for_bit(name):
    p, f, want = load_case(name)
    assert_bits(shim_normals(p, f), want)


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_matches_the_reference_bit_for_bit(name):
    p, f, want = load_case(name)
    assert_bits(normals_ref.compute_normals(p, f), want)


@pytest.mark.parametrize("kind", ["soup", "grid", "fan"])
def test_restatement_and_host_build_agree_on_100k_faces(kind):
    if kind == "soup":
        p, f = soup(100_000, 30_000, 5)
        f[:50] = f[:50, [0, 0, 1]]  # (repeated indices)
        p[f[50:60, 1]] = p[f[50:60, 0]]  # (coincident positions)
    elif kind == "grid":
        p, f = jittered_grid(317, 160, 6)
    else:
        p, f = fan(100_000, 7)
    assert f.shape[0] >= 98_000
    assert_bits(shim_normals(p, f), normals_ref.compute_normals(p, f))


def test_zero_length_face_adds_nothing():
    """the reference `break`s before the first add of a face whose normal has length 0: it changes no sum"""
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [5, 5, 5]], float)
    ok, _ = shim_face(p, [0, 1, 3])  # collinear
    assert not ok
    ok, _ = shim_face(p, [4, 4, 2])  # a repeated index
    assert not ok
    ok, c = shim_face(p, [0, 1, 2])
    assert ok and np.allclose(c[:, 2], [np.pi / 2, np.pi / 4, np.pi / 4])
    got = shim_normals(p, [[0, 1, 2], [0, 1, 3]])
    assert_bits(got, shim_normals(p, [[0, 1, 2]]))


def test_unreferenced_and_cancelled_vertices_get_positive_zeros():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [7, 7, 7]], float)
    got = shim_normals(p, [[0, 1, 2], [0, 2, 1]])
    assert_bits(got, np.zeros((4, 3)))


def test_obtuse_corner_takes_the_references_formula():
    """unit_angle's dot < 0 branch is (pi - 2) * asin(|u + v| / 2), as the reference wrote it"""
    p = np.array([[0, 0, 0], [1, 0, 0], [-1, 0.5, 0]], float)
    ok, c = shim_face(p, [0, 1, 2])
    u, v = np.array([1.0, 0, 0]), np.array([-1, 0.5, 0]) / np.hypot(1, 0.5)
    assert ok and c[0, 2] == pytest.approx((np.pi - 2) * np.arcsin(0.5 * np.linalg.norm(u + v)), rel=1e-15)
    assert c[0, 2] != pytest.approx(np.pi - 2 * np.arcsin(0.5 * np.linalg.norm(u + v)))


@pytest.mark.parametrize("bad", [-1, 4, 2**31 - 1])
def test_out_of_range_index_is_refused(bad):
    p = np.zeros((4, 3))
    with pytest.raises(IndexError):
        shim_normals(p, [[0, 1, 2], [1, bad, 3]])
    with pytest.raises(IndexError):
        normals_ref.compute_normals(p, [[0, 1, 2], [1, bad, 3]])


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "take_hip.h")).read()
    for sym in ("take_hip_mesh_compute_normals", "take_hip_compute_normals"):
        assert sym + "(" in hdr and sym in capi.EXPORTS
        assert hasattr(capi.lib(), sym)


def test_device_mesh_normals_keyword_is_checked():
    with pytest.raises(ValueError):
        capi.DeviceMesh(b"ply\n", normals="smooth")


def test_generator_reproduces_the_fixtures(tmp_path):
    """the committed fixtures are what tools/gen_normals_golden.py makes through the compiled reference"""
    from oracle.gen_golden import HARNESS

    if not os.path.exists(HARNESS):
        pytest.skip("oracle/_ref/ref_harness is built only where the reference sources are")
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "tools", "gen_normals_golden.py"), "--out", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    for name in CASES:
        assert (tmp_path / (name + "_mesh.f64")).read_bytes() == open(os.path.join(NRM, name + "_mesh.f64"), "rb").read(), name


def test_counts_beyond_the_kernels_are_refused_before_any_device_work():
    """checked on the host before the device is touched: runs without a GPU"""
    L = capi.lib()
    assert L.take_hip_compute_normals(None, 3, None, 2**31 // 3 + 1, None) == D.TAKE_E_INVALID
    assert "INT32_MAX corners" in L.take_hip_last_error().decode()
    assert L.take_hip_compute_normals(None, 2**31, None, 1, None) == D.TAKE_E_INVALID
    assert L.take_hip_compute_normals(None, -1, None, 1, None) == D.TAKE_E_INVALID


def test_mesh_entry_point_refuses_host_arrays_and_meshes_with_normals():
    pos = np.zeros((3, 3))
    idx = np.array([[0, 1, 2]], np.int32)
    m = D.TakeMesh()
    m.n_vertices, m.n_faces = 3, 1
    m.positions = pos.ctypes.data_as(C.POINTER(C.c_double))
    m.indices = idx.ctypes.data_as(C.POINTER(C.c_int32))
    L = capi.lib()
    assert L.take_hip_mesh_compute_normals(C.byref(m)) == D.TAKE_E_INVALID  # host arrays
    assert "not a device-array mesh" in L.take_hip_last_error().decode()
    m.flags = D.TAKE_MESH_DEVICE_ARRAYS
    m.normals = pos.ctypes.data_as(C.POINTER(C.c_double))
    assert L.take_hip_mesh_compute_normals(C.byref(m)) == D.TAKE_E_INVALID  # normals already
    assert "has normals already" in L.take_hip_last_error().decode()
    assert L.take_hip_mesh_compute_normals(None) == D.TAKE_E_INVALID

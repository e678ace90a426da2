"""compute_normals on the GPU (take_hip_compute_normals / take_hip_mesh_compute_normals, tk_normals.h).

The reduction is ordered (a stable sort, no atomics), so the only difference from the reference is the device asin
(ocml) against the C library's, which differ in the last bit for some arguments.  A per-component ulp bound cannot
hold: a component that is the small difference of large contributions moves by about one ulp of the row — thousands of
its own ulps — and a component the reference gets as exactly zero by symmetry can come out as +-1e-17.  The bound is
therefore per component in ulps of the row's largest component times the vertex's condition number (scaled_ulp), and
rows the reference leaves at zero must be (+0, +0, +0) bit for bit.  Measured on an MI355X: 2.0 over the fixtures
(tests/golden/normals, the reference's own output; 88-100 % of their rows bit-identical), 2.98 on the 1M-face grid +
soup and 3.0 on the 1M-face fan against the host build of the same kernels (tests/normals_shim); the bound is 4, the
ceiling (twice the measured value would be 6).  Two runs give the same bits; a device mesh's normals are the
host-array entry point's, bit for bit; the emissive tetrahedron of the `meshlight` golden scene, decoded on the device
with normals="scene", renders at the f64 parity bar of tests/test_gpu_parity.py — a scene the library refused before
compute_normals existed (an emissive mesh needs vertex normals)."""
import copy
import os

import numpy as np
import pytest

import normals_ref
import oracle
from helpers import GOLD, golden_scene, rmse
from take_amd import capi
from take_amd import cdefs as D
from test_normals_cpu import CASES, fan, jittered_grid, load_case, shim_normals, soup

pytestmark = pytest.mark.gpu

MEASURED_ULP = 3
ULP_BOUND = min(4, 2 * MEASURED_ULP)
TETRA = os.path.join(GOLD, "scenes", "tetra_light.ply")


def scaled_ulp(got, want, positions, indices):
    """per component |got - want| in units in the last place of the largest component of the reference's row, divided
    by the vertex's condition number (normals_ref.condition, at least 1).  A normal is a unit vector: a component that
    is the small difference of large contributions carries their rounding (an asin one ulp apart moves it by about one
    ulp of the row, which can be thousands of its own ulps, or flip the sign of a component that is zero to within
    that), and where the contributions nearly cancel (a sliver next to its neighbour, a random soup) the whole row moves
    by their sum over the size of the result.  Rows the reference leaves at zero — no contribution, or sums that cancel
    exactly — must be (+0, +0, +0) bit for bit."""
    assert got.shape == want.shape
    zero = ~np.any(want != 0, axis=1)
    assert np.array_equal(got[zero].view(np.uint64), want[zero].view(np.uint64)), "zero rows differ"
    kappa = np.nan_to_num(normals_ref.condition(positions, indices), nan=1.0, posinf=1.0)
    scale = np.spacing(np.abs(want).max(axis=1, initial=0)) * np.maximum(kappa, 1.0)
    return np.abs(got - want) / scale[:, None]


def assert_close(got, want, what, positions, indices):
    d = scaled_ulp(got, want, positions, indices)
    assert d.max(initial=0) <= ULP_BOUND, f"{what}: {d.max()} ulp at {np.unravel_index(d.argmax(), d.shape)}"
    return float(d.max(initial=0))


@pytest.mark.parametrize("name", CASES)
def test_fixtures_within_the_ulp_bound_of_the_reference(name):
    p, f, want = load_case(name)
    assert_close(capi.compute_normals(p, f), want, name, p, f)


@pytest.fixture(scope="module")
def million():
    g = jittered_grid(801, 401, 21)  # 640k faces
    s = soup(360_000, 120_000, 22)
    p = np.concatenate([g[0], s[0]])
    f = np.concatenate([g[1], s[1] + len(g[0])]).astype(np.int32)
    return p, f


def test_million_face_mesh_against_the_host_build(million):
    p, f = million
    assert f.shape[0] >= 1_000_000
    got = capi.compute_normals(p, f)
    assert_close(got, shim_normals(p, f), "1M mesh", p, f)
    assert np.array_equal(capi.compute_normals(p, f).view(np.uint64), got.view(np.uint64)), "two runs differ"


def test_million_face_fan_against_the_host_build():
    p, f = fan(1_000_000, 23)
    assert np.count_nonzero(f == 0) == 1_000_000
    got = capi.compute_normals(p, f)
    assert_close(got, shim_normals(p, f), "1M fan", p, f)
    assert np.array_equal(capi.compute_normals(p, f).view(np.uint64), got.view(np.uint64)), "two runs differ"


def test_fans_at_the_wave_path_threshold():
    """centre valences around the split between one lane and one wave per vertex (64) and its 256-element steps"""
    for n in (63, 64, 65, 255, 256, 257, 513, 1000):
        p, f = fan(n, n)
        assert_close(capi.compute_normals(p, f), shim_normals(p, f), f"fan {n}", p, f)


def test_edge_sizes():
    assert capi.compute_normals(np.zeros((0, 3)), np.zeros((0, 3), np.int32)).shape == (0, 3)
    got = capi.compute_normals(np.ones((5, 3)), np.zeros((0, 3), np.int32))
    assert np.array_equal(got.view(np.uint64), np.zeros((5, 3)).view(np.uint64))


@pytest.mark.parametrize("bad", [-1, 4, 2**31 - 1])
def test_out_of_range_index_is_invalid(bad):
    p, f = np.random.default_rng(1).uniform(size=(4, 3)), np.array([[0, 1, 2], [1, bad, 3]], np.int32)
    with pytest.raises(capi.TakeError) as e:
        capi.compute_normals(p, f)
    assert e.value.code == D.TAKE_E_INVALID and "outside the vertex array" in str(e.value)


def write_ply(path, p, f, normals=None):
    from oracle.gen_golden import write_ply as w

    w(str(path), p, f, normals)
    return str(path)


def test_device_mesh_normals_equal_the_host_entry_point(tmp_path):
    p, f = jittered_grid(300, 200, 24)
    m = capi.DeviceMesh(write_ply(tmp_path / "grid.ply", p, f))
    try:
        assert not m.c.normals
        host = m.download()
        m.compute_normals()
        got = m.download()
        assert np.array_equal(got.positions, host.positions) and np.array_equal(got.indices, host.indices)
        want = capi.compute_normals(host.positions, host.indices)
        assert np.array_equal(got.normals.view(np.uint64), want.view(np.uint64))
        with pytest.raises(capi.TakeError) as e:  # normals already there
            m.compute_normals()
        assert e.value.code == D.TAKE_E_INVALID
    finally:
        m.close()
    s = capi.DeviceMesh(write_ply(tmp_path / "grid.ply", p, f), normals="scene")
    try:
        assert np.array_equal(s.download().normals.view(np.uint64), want.view(np.uint64))
    finally:
        s.close()


def test_scene_rule_keeps_a_files_own_normals(tmp_path):
    p, f = jittered_grid(20, 10, 25)
    n = np.tile([0.0, 0.6, 0.8], (len(p), 1))
    path = write_ply(tmp_path / "with_normals.ply", p, f, n)
    a, b = capi.DeviceMesh(path), capi.DeviceMesh(path, normals="scene")
    try:
        na, nb = a.download().normals, b.download().normals
        assert na is not None and np.array_equal(na.view(np.uint64), nb.view(np.uint64))
    finally:
        a.close(), b.close()


def test_host_arrays_mesh_is_invalid():
    p, f = np.random.default_rng(2).uniform(size=(3, 3)), np.array([[0, 1, 2]], np.int32)
    m = D.TakeMesh()
    m.n_vertices, m.n_faces = 3, 1
    import ctypes as C

    m.positions = p.ctypes.data_as(C.POINTER(C.c_double))
    m.indices = f.ctypes.data_as(C.POINTER(C.c_int32))
    assert capi.lib().take_hip_mesh_compute_normals(C.byref(m)) == D.TAKE_E_INVALID
    assert not m.normals


def meshlight_with_device_tetra(normals):
    sd = golden_scene("meshlight")
    dm = capi.DeviceMesh(TETRA, normals=normals)
    pos = dm.download().positions
    k = [i for i, m in enumerate(sd.meshes) if m.positions.shape == pos.shape and np.array_equal(m.positions, pos)]
    assert len(k) == 1
    dm.material_id = sd.meshes[k[0]].material_id
    dm.c.material_id = dm.material_id
    sd_dev = copy.copy(sd)
    sd_dev.meshes = list(sd.meshes)
    sd_dev.meshes[k[0]] = dm
    return sd, sd_dev, k[0], dm


def test_emissive_device_mesh_without_normals_is_refused():
    """what the "scene" rule is for: the reference's parse_scene would have computed them"""
    sd, sd_dev, k, dm = meshlight_with_device_tetra(None)
    try:
        assert sd.meshes[k].normals is not None and not dm.c.normals
        with pytest.raises(capi.TakeError, match="emissive mesh has no vertex normals"):
            capi.Scene(sd_dev, precision=D.TAKE_PRECISION_F64)
    finally:
        dm.close()


def test_meshlight_with_device_computed_normals_renders_at_the_parity_bar():
    sd, sd_dev, k, dm = meshlight_with_device_tetra("scene")
    try:
        nrm = dm.download().normals
        exact = np.array_equal(nrm.view(np.uint64), sd.meshes[k].normals.view(np.uint64))
        assert_close(nrm, sd.meshes[k].normals, "tetra_light", sd.meshes[k].positions, sd.meshes[k].indices)
        osc = oracle.OracleScene(sd, precision=1)
        want = osc.render(4, 5, rng_mode=oracle.RNG_COUNTER, seed=11)
        osc.close()
        sc = capi.Scene(sd_dev, precision=D.TAKE_PRECISION_F64)
        try:
            got = sc.render(spp=4, max_depth=5, seed=11)
        finally:
            sc.close()
        assert rmse(got, want) < 1e-9, rmse(got, want)
        if exact:
            ref = capi.Scene(sd, precision=D.TAKE_PRECISION_F64)
            try:
                assert np.array_equal(ref.render(spp=4, max_depth=5, seed=11), got)
            finally:
                ref.close()
    finally:
        dm.close()

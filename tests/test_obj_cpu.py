"""OBJ ingestion, CPU side (take_hip_mesh_from_obj): the numpy restatement of the reference's parse_obj (tests/obj_ref.py)
against the arrays the reference's OWN parser made of the committed files (tests/golden/obj, written by
tools/gen_obj_golden.py through oracle/_ref/ref_harness), the generator's reproducibility, and the library's exports."""
import ctypes as C
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import obj_ref
from helpers import GOLD
from take_amd import capi
from take_amd import cdefs as D
from test_ply_cpu import assert_same_mesh

OBJ = os.path.join(GOLD, "obj")
CASES = sorted(f[:-4] for f in os.listdir(OBJ) if f.endswith(".obj"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_case(name):
    """-> (file bytes, to_world, the reference's inverse(to_world), the reference's TriangleMesh arrays)"""
    data = open(os.path.join(OBJ, name + ".obj"), "rb").read()
    xf = np.fromfile(os.path.join(OBJ, name + "_xform.f64"), "<f8").reshape(4, 4)
    a = np.fromfile(os.path.join(OBJ, name + "_mesh.f64"), "<f8")
    nv, nf, has_n, has_uv = (int(x) for x in a[:4])
    inv = a[4:20].reshape(4, 4)
    o = 20
    ref = {"positions": a[o:o + 3 * nv].reshape(nv, 3)}
    o += 3 * nv
    ref["indices"] = a[o:o + 3 * nf].reshape(nf, 3).astype(np.int32)
    o += 3 * nf
    ref["normals"] = a[o:o + 3 * nv].reshape(nv, 3) if has_n else None
    o += 3 * nv * has_n
    ref["uvs"] = a[o:o + 2 * nv].reshape(nv, 2) if has_uv else None
    o += 2 * nv * has_uv
    assert o == a.size
    return data, xf, inv, ref


def test_fixture_set_covers_the_issue_cases():
    assert {"tri_full_identity", "quad_vn_affine", "negative_interleaved", "homogeneous_projective", "whitespace_formats",
            "negative_vt_vn", "vt_only", "zero_vn", "slash_forms"} <= set(CASES)


def test_format_fixture_needs_the_host_fixup_path():
    """17-digit numbers: outside Clinger's exact case, so the device hands them to the host's strtod"""
    data = load_case("whitespace_formats")[0]
    assert b"\r\n" in data and b"\t" in data and not data.endswith(b"\n")
    assert b"0.30000000000000004" in data and b"+2E+2" in data and b"-0.0" in data


@pytest.mark.parametrize("name", CASES)
def test_obj_ref_matches_reference(name):
    data, xf, inv, ref = load_case(name)
    assert_same_mesh(obj_ref.parse_obj(data, xf, inv), ref)


def test_negative_zero_survives():
    """`vt -0.0 ...`: the reference's uv keeps the sign of zero (num_get -> strtod), and so must the decode"""
    _, _, _, ref = load_case("whitespace_formats")
    assert np.signbit(ref["uvs"][0, 0]) and ref["uvs"][0, 0] == 0


@pytest.mark.parametrize("text,code", [
    (b"v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nv 2 2 2\nf 1 2 3 4 5\n", obj_ref.NGON),
    (b"v 0 0 0\nv 1 0 0\nf 1 0 2\n", obj_ref.V0),
    (b"v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n", obj_ref.RANGE),
    (b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 1 2\n", obj_ref.RANGE),
    (b"v 0 0 0\nv 1 0 0\nf 1 2\n", obj_ref.FEW),
    (b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3 # c\n", obj_ref.UNSUPPORTED),
    (b"v 0 0 0\nv 1 0 nan\nv 0 1 0\nf 1 2 3\n", obj_ref.UNSUPPORTED),
    (b"v 0 0 0\nv 1 0 1e999\nv 0 1 0\nf 1 2 3\n", obj_ref.UNSUPPORTED),
    (b"v 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n", obj_ref.UNSUPPORTED),
])
def test_obj_ref_errors(text, code):
    with pytest.raises(obj_ref.ObjError) as e:
        obj_ref.parse_obj(text)
    assert e.value.code == code


def test_obj_ref_partial_vt_is_unsupported():
    with pytest.raises(obj_ref.ObjError) as e:
        obj_ref.parse_obj(b"v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2 3\n")
    assert e.value.unsupported


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "ref_harness")), reason="oracle/_ref/ref_harness not built")
def test_generator_regenerates_the_fixtures_byte_identically(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_obj_golden.py"), "--out", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    assert sorted(os.listdir(tmp_path)) == sorted(os.listdir(OBJ))
    match, mismatch, errors = filecmp.cmpfiles(OBJ, str(tmp_path), sorted(os.listdir(OBJ)), shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_obj_symbols_are_exported():
    lib = capi.lib()
    for name in ("take_hip_mesh_from_obj", "take_hip_mesh_from_obj_file"):
        assert name in capi.EXPORTS
        assert hasattr(lib, name), name


def test_decode_without_gpu_is_an_error_not_a_host_parse():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the no-GPU contract is checked in the CPU container")
    data = load_case("tri_full_identity")[0]
    m = D.TakeMesh()
    rc = capi.lib().take_hip_mesh_from_obj(data, len(data), None, None, 0, C.byref(m))
    assert rc == D.TAKE_E_NO_GPU and not m.positions


def test_device_mesh_rejects_an_unknown_format():
    with pytest.raises(ValueError):
        capi.DeviceMesh(b"v 0 0 0\n", format="stl")

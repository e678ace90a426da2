"""OBJ ingestion, CPU side (take_hip_mesh_from_obj): the numpy restatement of the reference's parse_obj (tests/obj_ref.py)
against the arrays the reference's OWN parser made of the committed files (tests/golden/obj, written by
tools/gen_obj_golden.py through oracle/_ref/ref_harness), the generator's reproducibility, the library's exports, and the
device's per-token and per-line functions built for the host (tests/obj_host) against float() and the restatement on the
tokens and lines tests/obj_numbers.py spells around the edges of the device's number window."""
import ctypes as C
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import obj_numbers
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
            "negative_vt_vn", "vt_only", "zero_vn", "slash_forms", "number_grammar"} <= set(CASES)


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


# ---- the device's per-token and per-line text, built for the host (tests/obj_host) ----------------------------------
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(ROOT, "tests", "obj_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        _HOST = C.CDLL(os.path.join(d, "libobj_host.so"))
        for f in (_HOST.obj_host_parse_real, _HOST.obj_host_stoi_prefix, _HOST.obj_host_parse_corner):
            f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p], None
        _HOST.obj_host_classify.argtypes, _HOST.obj_host_classify.restype = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p], None
        _HOST.obj_host_line_types.argtypes, _HOST.obj_host_line_types.restype = [C.c_void_p], None
    return _HOST


def packed(items):
    """-> (the items back to back, their n + 1 offsets)"""
    off = np.zeros(len(items) + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in items])
    return np.frombuffer(b"".join(items) + b"\0", np.uint8), off  # (+ one byte: an empty buffer has no address)


def host_parse_real(tokens):
    """-> (codes, values); a value the host build did not write holds the pattern 7.0"""
    buf, off = packed(tokens)
    code, val = np.full(len(tokens), 99, np.int32), np.full(len(tokens), 7.0)
    host_lib().obj_host_parse_real(buf.ctypes.data, off.ctypes.data, len(tokens), code.ctypes.data, val.ctypes.data)
    return code, val


@pytest.fixture(scope="module")
def number_tokens():
    return obj_numbers.number_tokens(30_000)


def test_number_generator_is_deterministic_and_covers_its_list(number_tokens):
    assert number_tokens == obj_numbers.number_tokens(30_000) and len(set(number_tokens)) > 25_000
    text = b" ".join(number_tokens)
    for piece in (b"e+00", b"E-00", b" .", b". ", b" +.", b" -0", b" 00000"):
        assert piece in text, piece
    for t in obj_numbers.NEGATIVE_ZEROS + obj_numbers.POSITIVE_ZEROS:
        assert t in obj_numbers.CURATED and float(t) == 0 and bool(np.signbit(float(t))) == (t in obj_numbers.NEGATIVE_ZEROS)


def test_host_build_numbers_match_float_and_the_restatement(number_tokens):
    """parse_real as the device runs it: outside the grammar exactly where the restatement says so, and every value it
    converts itself is float()'s correctly rounded one, bit for bit (the sign of a zero included)"""
    tokens = number_tokens + obj_numbers.CURATED + obj_numbers.REFUSED
    code, val = host_parse_real(tokens)
    assert set(code.tolist()) <= {-1, 0, 1}
    grammar = np.array([obj_ref.NUMBER.fullmatch(t) is not None for t in tokens])
    wrong = [tokens[i] for i in np.nonzero((code == -1) == grammar)[0]]
    assert not wrong, wrong[:10]
    dev = np.nonzero(code == 0)[0]
    want = np.array([float(tokens[i]) for i in dev])
    diff = [(tokens[i], val[i], w) for i, w in zip(dev, want) if val[i:i + 1].view(np.uint64)[0] != np.float64(w).view(np.uint64)]
    assert not diff, diff[:10]
    assert all(obj_ref.real(tokens[i]) is not None for i in dev)
    assert np.all(val[code != 0].view(np.uint64) == np.float64(7.0).view(np.uint64))  # (nothing written on the other paths)
    # the refusal list: refused by the restatement; never converted on the device (the grammar ones -1, the range ones
    # left to the host's strtod, which reports them)
    at = {t: i for i, t in enumerate(tokens)}
    for t in obj_numbers.REFUSED:
        assert obj_ref.real(t) is None and code[at[t]] != 0, t
    for t in obj_numbers.REFUSED_RANGE:
        assert code[at[t]] == 1, t
    for t in obj_numbers.CURATED:
        assert obj_ref.real(t) is not None and code[at[t]] >= 0, t
    # both paths stay populated: of the accepted tokens at least a quarter each way
    ok = np.array([obj_ref.real(t) is not None for t in tokens])
    n_dev, n_host = int(np.sum(ok & (code == 0))), int(np.sum(ok & (code == 1)))
    assert n_dev + n_host == int(ok.sum())
    assert 4 * n_dev >= ok.sum() and 4 * n_host >= ok.sum(), (n_dev, n_host)


def test_host_build_window_edges_take_the_path_the_header_documents():
    """tk_obj.h: at most 15 significant digits and an effective exponent in [-22, 22] are the device's; trailing and
    leading zeros are not significant digits"""
    device = [b"999999999999999e22", b"123456789012345e-22", b"1e22", b"10e21", b"1200e20", b"12e22", b".12e24", b"1.5e-21",
              b"15e-22", b"100000000000000e1", b"100000000000001e1", b"1000000000000000", b"123456789012345000000000", b"0.000000123456789012345",
              b"0e999999999999", b"-0E-999999999999", b"000000000000000000001"]
    host = [b"1e23", b"10e22", b"100000000000000000000000", b"1200e21", b"12e23", b".12e25", b"1.5e-22", b"15e-23", b"15e-24",
            b"9007199254740993", b"1000000000000001", b"1000000000000001e1", b"1.7976931348623157e308", b"2.2250738585072014e-308"]
    code, _ = host_parse_real(device + host)
    assert code.tolist() == [0] * len(device) + [1] * len(host)


def test_host_build_corners_match_split_face():
    tokens = obj_numbers.corner_tokens(3_000)
    assert {b"1/2/3/4", b"/2", b"1//", b"12abc", b"abc", b"-0", b"2147483647", b"2147483648", b"-2147483648", b"-2147483649"} <= set(tokens)
    buf, off = packed(tokens)
    ok, key = np.full(len(tokens), 9, np.int32), np.full((len(tokens), 3), 9, np.int32)
    host_lib().obj_host_parse_corner(buf.ctypes.data, off.ctypes.data, len(tokens), ok.ctypes.data, key.ctypes.data)
    want = [obj_ref.split_face(t) for t in tokens]
    assert 0.2 < np.mean([w is None for w in want]) < 0.8
    for t, o, k, w in zip(tokens, ok.tolist(), key.tolist(), want):
        assert (o, k if o else None) == (int(w is not None), w), (t, o, k, w)
    # std::stoi alone, on the pieces
    pieces = sorted({p for t in tokens for p in t.split(b"/") if p})
    buf, off = packed(pieces)
    ok, val = np.full(len(pieces), 9, np.int32), np.full(len(pieces), 9, np.int32)
    host_lib().obj_host_stoi_prefix(buf.ctypes.data, off.ctypes.data, len(pieces), ok.ctypes.data, val.ctypes.data)
    for p, o, v in zip(pieces, ok.tolist(), val.tolist()):
        w = obj_ref.stoi(p)
        assert (o, v if o else None) == (int(w is not None), w), (p, o, v, w)


def test_host_build_line_types_match_the_restatement():
    rng = np.random.default_rng(5)
    blanks = [b" ", b"\t", b"\v", b"\f", b"\r", b"  ", b" \t", b"\r \f"]
    keywords = [b"v", b"vt", b"vn", b"f", b"vp", b"vtx", b"vnn", b"vv", b"ff", b"fv", b"V", b"F", b"VT", b"#", b"#v", b"#f", b"v#", b"f#",
                b"o", b"g", b"s", b"l", b"usemtl", b"mtllib", b"v\xa0", b"\x1fv", b"f\x00", b"vt.", b"t", b"n"]
    args = [b"1", b"-2/3", b"0.5", b"#", b"x", b"1//2", b"f", b"v", b"\xa0", b"1\x1f2"]

    def pick(xs):
        return xs[int(rng.integers(len(xs)))]

    lines = [b"", b" ", b"\r", b"\t\v\f\r ", b"#", b"  # f 1 2 3", b"\t#v 1 2 3", b"f", b"f ", b" f\r", b"v", b"vt\r", b"vn\t"]
    for kw in keywords:
        for n in range(7):
            for _ in range(3):
                ln = (pick(blanks) if rng.random() < 0.5 else b"") + kw
                for _ in range(n):
                    ln += pick(blanks) + pick(args)
                lines.append(ln + (pick(blanks) if rng.random() < 0.5 else b""))
    assert not any(b"\n" in ln for ln in lines)
    names = np.zeros(7, np.uint8)
    host_lib().obj_host_line_types(names.ctypes.data)
    assert len(set(names.tolist())) == 7
    name_of = dict(zip(names.tolist(), (None, "v", "vt", "vn", "f3", "f4", "fbad")))
    buf, off = packed(lines)
    got = np.full(len(lines), 99, np.uint8)
    host_lib().obj_host_classify(buf.ctypes.data, off.ctypes.data, len(lines), got.ctypes.data)
    want = [obj_ref.line_kind(ln)[0] for ln in lines]
    assert set(want) == set(name_of.values())
    for ln, g, w in zip(lines, got.tolist(), want):
        assert name_of[g] == w, (ln, g, w)

"""CPU side of displacement mapping on the device (take_hip_displace_*, take_hip_scene_displace_meshes,
include/take_hip.h):

1. The kernel's body and what creation builds (take_amd/csrc/tk_displace.h) without a GPU: tests/displace_host builds
   them for the host and runs them — between tk_subdiv.h's two normal bodies — in the launches' loop structure; they
   equal tests/displace_ref.py — a numpy restatement written from the specification — bit for bit over the shared
   cases, under every grid.
2. Properties that do not lean on the restatement: every height within its cell's texels, scale 0 moves by the bias
   alone, fractions and indices inside the image, unit normals, the sanitizer build.
3. The real library without a GPU: every refusal that needs no device, the exported symbols, the ABI version.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import displace_ref
from take_amd import capi
from take_amd import cdefs as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ["take_hip_displace_create", "take_hip_displace_destroy", "take_hip_displace_info", "take_hip_displace_apply_device", "take_hip_displace_apply",
           "take_hip_scene_displace_meshes"]

_HOST = None


def host():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "displace_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libdisplace_host.so"))
        L.displace_host_message.restype = C.c_char_p
        L.displace_host_apply.argtypes = ([C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 5)
        _HOST = L
    return _HOST


def host_apply(positions, normals, indices, uvs, image, uvxf=(1.0, 1.0, 0.0, 0.0), scale=1.0, bias=0.0, grid=0, out_normals=True):
    """tk_displace.h on the host -> {"positions", "direction", "normals" (or None), "cells" (nv, 4: x1, x2, y1, y2),
    "fractions" (nv, 3: fx, fy, h)}"""
    pos, idx = np.ascontiguousarray(positions, np.float64), np.ascontiguousarray(indices, np.int32)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float64)
    uv, img = np.ascontiguousarray(uvs, np.float64), np.ascontiguousarray(image)
    assert img.dtype in (np.float32, np.float64) and img.ndim == 2
    lookup = np.array(uvxf, np.float64)
    nv = pos.shape[0]
    out = {"positions": np.zeros((nv, 3)), "direction": np.zeros((nv, 3)), "normals": np.zeros((nv, 3)) if out_normals else None,
           "cells": np.zeros((nv, 4), np.int32), "fractions": np.zeros((nv, 3))}
    rc = host().displace_host_apply(nv, idx.shape[0], idx.ctypes.data, uv.ctypes.data, img.shape[1], img.shape[0], img.ctypes.data, int(img.dtype == np.float64),
                                    lookup.ctypes.data, pos.ctypes.data, None if nrm is None else nrm.ctypes.data, scale, bias, grid, out["positions"].ctypes.data,
                                    out["direction"].ctypes.data, None if out["normals"] is None else out["normals"].ctypes.data, out["cells"].ctypes.data,
                                    out["fractions"].ctypes.data)
    assert rc == 0, f"a write outside the output arrays, or a refusal ({rc}: {host().displace_host_message()})"
    return out


def host_case(case, grid=0, **over):
    c = dict(case, **over)
    return host_apply(c["positions"], c["normals"], c["indices"], c["uvs"], c["image"], c["uvxf"], c["scale"], c["bias"], grid)


def differing(a, b):
    """how many doubles of a and b differ in any bit"""
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))


@functools.lru_cache(maxsize=None)
def restated():
    """{case name: (positions, direction, normals)} by the restatement: computed once, shared, never written"""
    out = {}
    for c in displace_ref.cases():
        arrays = displace_ref.displace(c["positions"], c["normals"], c["indices"], c["uvs"], c["image"], c["uvxf"], c["scale"], c["bias"])
        for a in arrays:
            a.setflags(write=False)
        out[c["name"]] = arrays
    return out


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_the_case_list_reaches_what_the_specification_lists():
    cases = displace_ref.cases()
    assert len(cases) == 4 * 13 and len({c["name"] for c in cases}) == len(cases)
    assert {c["image"].shape[::-1] for c in cases} == set(displace_ref.SHAPES)
    assert {c["image"].dtype for c in cases} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert sum(bool(np.isnan(c["image"]).any()) for c in cases) == 4
    assert any(c["scale"] == 0 and c["bias"] != 0 for c in cases) and any(c["scale"] < 0 for c in cases)
    assert any(c["normals"] is None for c in cases) and any(c["normals"] is not None for c in cases)
    for name, p, n, i, uv in displace_ref.meshes():
        assert (uv[0] == 0).all() and (uv[1] == 1).all() and uv[2, 0] == -1e-20, name
        assert uv.min() < 0 and (uv.max() > 1 or name == "triangle"), name
        a, b = displace_ref.sources(uv, displace_ref.IDENTITY)
        assert a[2] == displace_ref.BELOW_ONE and a[0] == 0 and a[1] == 0, name  # (exactly 1 wraps to 0; -1e-20 is the BELOW_ONE case)
        assert a.min() >= 0 and a.max() < 1 and b.min() >= 0 and b.max() < 1
    # the wrap cell in x and in y, on the 16 x 16 image and on every smaller one (uvs 3 and 4 under the plain lookup)
    for c in cases:
        cells = host_case(c)["cells"]
        w, h = c["image"].shape[::-1]
        if c["mesh"] != "triangle" and c["uvxf"] == displace_ref.IDENTITY:
            assert (cells[:, 0] == w - 1).any() and (cells[:, 1] == 0).any() and (cells[:, 2] == h - 1).any() and (cells[:, 3] == 0).any(), c["name"]
    unused = next(m for m in displace_ref.meshes() if m[0] == "strip9-unused-vertex")
    assert 9 not in unused[3]


def test_host_build_equals_the_restatement_bit_for_bit():
    """positions, the own direction normals and the output normals, under the launch's own grid and under grids of 1, 2
    and 3 striding blocks (a guard element sits behind every output of the host build)"""
    for c in displace_ref.cases():
        want_p, want_d, want_n = restated()[c["name"]]
        for grid in (0, 1, 2, 3):
            got = host_case(c, grid)
            assert differing(got["positions"], want_p) == 0, f"{c['name']} grid {grid}: positions"
            assert differing(got["direction"], want_d) == 0, f"{c['name']} grid {grid}: direction"
            assert differing(got["normals"], want_n) == 0, f"{c['name']} grid {grid}: normals"


def test_own_direction_normals_are_the_normals_of_the_base_positions():
    for c in displace_ref.cases():
        if c["normals"] is None and c["mesh"] == "strip23-L2":
            mesh = next(m for m in displace_ref.meshes() if m[0] == c["mesh"])
            assert differing(host_case(c)["direction"], mesh[2]) == 0  # (the refined normals of the restatement)
            given = host_case(c, normals=mesh[2])
            assert differing(given["positions"], host_case(c)["positions"]) == 0


def test_control_the_colour_textures_seam_arithmetic_is_not_what_heights_use():
    """the comparison is not blind: eval_texture's formula in the wrap cell (x2 = 0: a cell width of 1 - width)
    extrapolates far outside the cell's texels, where the specification's stays between them"""
    img = np.array([[0.0, 1.0], [0.0, 1.0]])
    a, b = np.array([0.999]), np.array([0.25])
    # the height is tk_displace.h's: a triangle whose vertex 0 looks (a, b) up, through the host build
    got = host_apply([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], None, [[0, 1, 2]], [[a[0], b[0]], [0.5, 0.5], [0.5, 0.5]], img)
    h, (x1, x2, y1, y2) = got["fractions"][:1, 2], got["cells"][:1].astype(np.int64).T
    assert differing(h, displace_ref.heights(img, a, b)[0]) == 0 and differing(got["positions"][0], np.array([0.0, 0.0, h[0]])) == 0
    x, y = 2 * a, 2 * b
    X2, Y2 = np.where(x1 == x2, x2 + 1, x2), np.where(y1 == y2, y2 + 1, y2)
    seam = (img[y1, x1] * (X2 - x) * (Y2 - y) + img[y1, x2] * (x - x1) * (Y2 - y) + img[y2, x1] * (X2 - x) * (y - y1) + img[y2, x2] * (x - x1) * (y - y1)) / ((X2 - x1) * (Y2 - y1))
    q = np.array([img[y1, x1], img[y1, x2], img[y2, x1], img[y2, x2]])
    assert x1[0] == 1 and x2[0] == 0 and q.min() <= h[0] <= q.max() and abs(h[0] - 0.002) < 1e-12
    assert seam[0] > q.max() + 0.9  # (1.998 q11 - 0.998 q21: the seam formula divides by x2 - x1 = -1)


# ------------------------------------------------------------------------------------------------ properties
def test_every_height_lies_within_its_cells_four_texels():
    """h is two nested lerps of weights (1 - f, f) with f in [0, 1): exactly, a convex combination.  Rounded: 1 - f is one
    rounding, each lerp two products and a sum — three roundings on top of it —, and the lerps nest twice: at most 4 units
    in the last place of the largest texel outside the texels' range (measured on the CPU over random images from 1 x 1 to
    64 x 33: at most 2)."""
    worst = 0.0
    for c in displace_ref.cases():
        if c["nan"]:
            continue
        got = host_case(c)
        tex = c["image"].astype(np.float64)
        x1, x2, y1, y2 = got["cells"].T
        q = np.stack([tex[y1, x1], tex[y1, x2], tex[y2, x1], tex[y2, x2]])
        h = got["fractions"][:, 2]
        ulp = np.spacing(np.abs(q).max(axis=0))
        excess = np.maximum(q.min(axis=0) - h, h - q.max(axis=0)) / ulp
        worst = max(worst, float(excess.max()))
        assert (excess <= 4).all(), (c["name"], float(excess.max()))
    print(f"\nthe largest excess over the case list: {worst} ulp")


def test_scale_zero_moves_every_vertex_by_the_bias_alone():
    """p' = p + bias * n as values, whatever the image holds (the NaN image excepted: 0 * NaN is NaN)"""
    seen = 0
    for c in displace_ref.cases():
        if c["scale"] != 0 or c["nan"]:
            continue
        got = host_case(c)
        assert np.array_equal(got["positions"], c["positions"] + c["bias"] * got["direction"]), c["name"]
        seen += 1
    assert seen >= 8
    nan = next(c for c in displace_ref.cases() if c["nan"])
    assert np.isnan(host_case(nan, scale=0.0)["positions"]).any()


def test_fractions_lie_in_the_unit_interval_and_every_index_inside_the_image():
    for c in displace_ref.cases():
        got = host_case(c)
        w, h = c["image"].shape[::-1]
        fx, fy = got["fractions"][:, 0], got["fractions"][:, 1]
        assert (fx >= 0).all() and (fx < 1).all() and (fy >= 0).all() and (fy < 1).all(), c["name"]
        x1, x2, y1, y2 = got["cells"].T
        for i, n in ((x1, w), (x2, w), (y1, h), (y2, h)):
            assert (i >= 0).all() and (i < n).all(), c["name"]
        assert ((x2 == x1 + 1) | ((x1 == w - 1) & (x2 == 0))).all() and ((y2 == y1 + 1) | ((y1 == h - 1) & (y2 == 0))).all()


def test_output_normals_have_unit_length_or_are_exactly_zero():
    for c in displace_ref.cases():
        if c["nan"]:
            continue
        n = host_case(c)["normals"]
        length = np.sqrt((n * n).sum(axis=1))
        zero = ~n.any(axis=1)
        assert (np.abs(length[~zero] - 1.0) <= 2 * np.spacing(1.0)).all(), c["name"]
        assert zero.sum() == (1 if c["mesh"] == "strip9-unused-vertex" else 0), c["name"]


def test_a_vertex_no_face_uses_stays_where_it_is_under_its_own_zero_normal():
    c = next(c for c in displace_ref.cases() if c["mesh"] == "strip9-unused-vertex" and c["normals"] is None and not c["nan"] and c["scale"] != 0)
    got = host_case(c)
    assert differing(got["positions"][9], c["positions"][9]) == 0 and not got["direction"][9].any()
    assert np.abs(got["positions"][:9] - c["positions"][:9]).max() > 1e-3


def test_sanitizer_build_runs_clean():
    r = subprocess.run(["make", "-C", os.path.join(HERE, "displace_host"), "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
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
        assert getattr(lib, name).argtypes == D.DISPLACE_PROTOTYPES[name]
    assert sorted(D.DISPLACE_PROTOTYPES) == sorted(SYMBOLS)
    for method in ("info", "apply", "apply_device", "of_subdiv"):
        assert callable(getattr(capi.Displace, method))
    assert callable(capi.Scene.displace_meshes)
    assert lib.take_hip_abi_version() == 5


def test_the_prototypes_are_the_headers():
    """function by function, as tests/test_capi_cpu.py holds the whole table: pointer or scalar, and which scalar"""
    import re

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for name in SYMBOLS:
        ret, params = re.search(r"([A-Za-z_][\w \t*]*?)\b" + name + r"\s*\(([^()]*)\)\s*;", src).groups()
        params = [" ".join(p.split()) for p in params.split(",")]
        argtypes = D.PROTOTYPES[name]
        assert ret.strip() == "int" and len(params) == len(argtypes), name
        for param, t in zip(params, argtypes):
            if "*" in param:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, param)
            else:
                assert t is scalars[param.replace("const ", "").split()[0]], (name, param)


def test_struct_layouts_match_the_header():
    import tempfile

    fields = {"TakeDisplaceDesc": D.TakeDisplaceDesc, "TakeDisplaceBinding": D.TakeDisplaceBinding}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){"]
    for n, cls in fields.items():
        prog.append(f'printf("{n} %zu\\n", sizeof({n}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{n}.{fname} %zu\\n", offsetof({n}, {fname}));')
    prog.append('printf("flags %d\\n", TAKE_DISPLACE_DEVICE_ARRAYS);')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write("\n".join(prog))
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    lines = [line.split() for line in out.strip().splitlines()]
    assert lines[-1] == ["flags", str(D.TAKE_DISPLACE_DEVICE_ARRAYS)]
    want = dict(lines[:-1])
    for n, cls in fields.items():
        assert C.sizeof(cls) == int(want[n]), n
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == int(want[f"{n}.{fname}"]), f"{n}.{fname}"


STRIP_POS, STRIP = displace_ref.subdiv_ref.strip(9)
STRIP_UV = displace_ref.mesh_uvs(9)
IMAGE = displace_ref.image(5, 3, np.float32)


def desc(idx=STRIP, n_vertices=9, uvs=STRIP_UV, image=IMAGE, width=None, height=None, real=None, flags=0, uvxf=(1.0, 1.0, 0.0, 0.0)):
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
    uv = None if uvs is None else np.ascontiguousarray(uvs, np.float64)
    d = D.TakeDisplaceDesc()
    d.n_vertices, d.n_faces, d.indices, d.uvs = n_vertices, idx.shape[0], idx.ctypes.data, None if uv is None else uv.ctypes.data
    d.width, d.height = image.shape[1] if width is None else width, image.shape[0] if height is None else height
    d.texels, d.real, d.flags = image.ctypes.data, (D.TAKE_PRECISION_F64 if image.dtype == np.float64 else D.TAKE_PRECISION_F32) if real is None else real, flags
    d.uscale, d.vscale, d.uoffset, d.voffset = uvxf
    d._keep = (idx, uv, image)
    return d


def far_uvs():
    uv = STRIP_UV.copy()
    uv[4] = (1e300, 0.5)
    return uv


CREATE_REFUSALS = [
    ("index-range", lambda: desc(idx=[[0, 1, 2], [2, 1, 9]]), b"face 1: vertex index 9 out of range"),
    ("index-negative", lambda: desc(idx=[[0, -1, 2]]), b"face 0: vertex index -1 out of range"),
    ("no-uvs", lambda: desc(uvs=None), b"uvs are required"),
    ("no-vertices", lambda: desc(n_vertices=0), b"must be positive"),
    ("no-faces", lambda: desc(idx=np.zeros((0, 3), np.int32)), b"must be positive"),
    ("width-0", lambda: desc(width=0), b"width and height must be positive"),
    ("height-negative", lambda: desc(height=-3), b"width and height must be positive"),
    ("too-many-texels", lambda: desc(width=65536, height=32768), b"width * height must not pass INT32_MAX"),
    ("real-mixed", lambda: desc(real=D.TAKE_PRECISION_MIXED), b"unknown precision"),
    ("flags", lambda: desc(flags=2), b"unknown flag bits"),
    ("uscale-nan", lambda: desc(uvxf=(np.nan, 1.0, 0.0, 0.0)), b"uscale, vscale, uoffset and voffset must be finite"),
    ("voffset-inf", lambda: desc(uvxf=(1.0, 1.0, 0.0, np.inf)), b"uscale, vscale, uoffset and voffset must be finite"),
    ("s-overflows", lambda: desc(uvs=far_uvs(), uvxf=(1e300, 1.0, 0.0, 0.0)), b"vertex 4: its lookup coordinates are not finite"),
    ("uv-nan", lambda: desc(uvs=np.where(np.arange(18).reshape(9, 2) == 15, np.nan, STRIP_UV)), b"vertex 7: its lookup coordinates are not finite"),
]


@pytest.mark.parametrize("name,make,message", CREATE_REFUSALS, ids=[r[0] for r in CREATE_REFUSALS])
def test_refusals_of_a_description_before_a_device_is_looked_for(lib, name, make, message):
    out = C.c_void_p()
    d = make()
    assert lib.take_hip_displace_create(C.byref(d), C.byref(out)) == D.TAKE_E_INVALID
    assert message in lib.take_hip_last_error(), lib.take_hip_last_error()
    assert not out.value


def test_null_arguments_amplitudes_and_bindings_are_refused_before_a_device_is_looked_for(lib):
    out = C.c_void_p()
    d = desc()
    buf = np.zeros((64, 3))
    fake = C.c_void_p(buf.ctypes.data)  # (never dereferenced: refused first)
    no_indices, no_texels = desc(), desc()
    no_indices.indices, no_texels.texels = None, None
    p = buf.ctypes.data
    for rc in (lib.take_hip_displace_create(None, C.byref(out)), lib.take_hip_displace_create(C.byref(d), None), lib.take_hip_displace_create(C.byref(no_indices), C.byref(out)),
               lib.take_hip_displace_create(C.byref(no_texels), C.byref(out)), lib.take_hip_displace_destroy(None), lib.take_hip_displace_info(None, None, None, None, None, None),
               lib.take_hip_displace_apply(None, p, None, 1.0, 0.0, p, None), lib.take_hip_displace_apply(fake, None, None, 1.0, 0.0, p, None),
               lib.take_hip_displace_apply(fake, p, None, 1.0, 0.0, None, None), lib.take_hip_displace_apply_device(None, p, None, 0, 1.0, 0.0, p, None, None),
               lib.take_hip_displace_apply_device(fake, p, None, 0, 1.0, 0.0, None, None, None), lib.take_hip_scene_displace_meshes(None, None, 1),
               lib.take_hip_scene_displace_meshes(fake, None, 1)):
        assert rc == D.TAKE_E_INVALID
        assert b"null argument" in lib.take_hip_last_error()
    assert lib.take_hip_displace_apply_device(fake, p, None, 2, 1.0, 0.0, p, None, None) == D.TAKE_E_INVALID and b"unknown flag bits" in lib.take_hip_last_error()
    q, r = p + 512, p + 1024  # (other places in buf: distinct arrays)
    for pos, nrm, out_p, out_n in ((p, None, p, None), (p, q, q, None), (p, None, q, q), (p, None, q, p), (p, r, q, r)):  # an output that is an input, or the other output
        assert lib.take_hip_displace_apply_device(fake, pos, nrm, 0, 1.0, 0.0, out_p, out_n, None) == D.TAKE_E_INVALID
        assert b"an output array is an input" in lib.take_hip_last_error(), lib.take_hip_last_error()
    for scale, bias in ((np.nan, 0.0), (1.0, np.inf)):
        for rc in (lib.take_hip_displace_apply(fake, p, None, scale, bias, p, None), lib.take_hip_displace_apply_device(fake, p, None, 0, scale, bias, p, None, None)):
            assert rc == D.TAKE_E_INVALID and b"scale and bias must be finite" in lib.take_hip_last_error()
    b = (D.TakeDisplaceBinding * 2)()

    def refused(n, message):
        assert lib.take_hip_scene_displace_meshes(fake, b, n) == D.TAKE_E_INVALID
        assert message in lib.take_hip_last_error(), lib.take_hip_last_error()

    refused(0, b"n must be positive")
    b[0].mesh = -1
    refused(1, b"binding 0: mesh index out of range")
    b[0].mesh = 0
    refused(1, b"binding 0: null argument")  # (no handle)
    b[0].displace, b[0].flags = fake, 2
    refused(1, b"binding 0: unknown flag bits")
    b[0].flags, b[0].scale = 0, np.inf
    refused(1, b"binding 0: scale and bias must be finite")
    b[0].scale, b[0].bias = 1.0, np.nan
    refused(1, b"binding 0: scale and bias must be finite")
    b[0].bias = 0.0
    refused(1, b"binding 0: exactly one of positions and subdiv")  # neither
    b[0].positions, b[0].subdiv = p, fake
    refused(1, b"binding 0: exactly one of positions and subdiv")  # both
    b[0].positions, b[0].normals = None, p
    refused(1, b"binding 0: normals cannot be given with subdiv")
    b[0].normals = None
    refused(1, b"binding 0: exactly one of cage_positions and rig")  # neither
    b[0].cage_positions, b[0].rig = p, fake
    refused(1, b"binding 0: exactly one of cage_positions and rig")  # both
    b[0].subdiv, b[0].positions = None, p
    refused(1, b"binding 0: cage_positions and rig go with subdiv")
    b[0].cage_positions, b[0].rig = None, None
    b[1].mesh, b[1].displace, b[1].positions, b[1].scale = 0, p + 8, p, 1.0
    refused(2, b"mesh 0 appears more than once")
    b[1].mesh, b[1].displace = 1, fake
    refused(2, b"a displacement handle is bound more than once")
    b[1].displace = p + 8
    b[0].positions, b[0].subdiv, b[0].cage_positions = None, fake, p
    b[1].positions, b[1].subdiv, b[1].cage_positions = None, fake, p
    refused(2, b"a subdivision handle is bound more than once")


def test_valid_arguments_without_a_gpu_are_no_gpu(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the no-GPU contract is checked in the CPU container")
    out = C.c_void_p()
    d = desc()
    assert lib.take_hip_displace_create(C.byref(d), C.byref(out)) == D.TAKE_E_NO_GPU
    assert b"no CPU path" in lib.take_hip_last_error() and not out.value
    with pytest.raises(capi.TakeError) as e:
        capi.Displace(STRIP, 9, STRIP_UV, IMAGE)
    assert e.value.code == D.TAKE_E_NO_GPU


def test_python_wrapper_refuses_mismatched_shapes():
    with pytest.raises(ValueError, match="indices must have shape"):
        capi.Displace(np.zeros((4, 2), np.int32), 9, STRIP_UV, IMAGE)
    with pytest.raises(ValueError, match="uvs must have shape"):
        capi.Displace(STRIP, 9, STRIP_UV[:8], IMAGE)
    with pytest.raises(ValueError, match="uvs is required"):
        capi.Displace(STRIP, 9, None, IMAGE)
    with pytest.raises(ValueError, match="image must have shape"):
        capi.Displace(STRIP, 9, STRIP_UV, np.zeros((3, 5, 3), np.float32))


# ------------------------------------------------------------------------------------------------ the CLI's parameter
def test_the_displace_parameter_reads_its_file_scale_and_bias(tmp_path):
    from take_amd.render import parse_displace

    path = str(tmp_path / "height.npy")
    np.save(path, np.stack([IMAGE, IMAGE + 1.0, IMAGE + 2.0], axis=-1))  # (h, w, 3): the first channel is the height
    params = ["scene.tkscene", "-displace", f"{path},0.25,-0.5", "-max_depth", "5"]
    img, scale, bias = parse_displace(params)
    assert params == ["scene.tkscene", "-max_depth", "5"] and (scale, bias) == (0.25, -0.5)
    assert img.dtype == np.float32 and np.array_equal(img, IMAGE) and img.flags.c_contiguous
    assert parse_displace(["-displace", f"{path},2"])[1:] == (2.0, 0.0)
    assert parse_displace(["scene.tkscene"]) is None
    for bad in (["-displace"], ["-displace", path], ["-displace", f"{path},x"], ["-displace", "height.png,1"], ["-displace", f"{path}x.npy,1"]):
        with pytest.raises(SystemExit, match="-displace"):
            parse_displace(bad)

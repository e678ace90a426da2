"""CPU side of take_hip_scene_set_materials, take_hip_scene_set_light_intensities* and the test hook
take_hip_debug_shading_tables* (include/take_hip.h).

1. The kernels' bodies (take_amd/csrc/tk_shading_update.h) without a GPU: tests/shading_update_host builds them for the
   host and runs them in the launches' loop structure — blocks of 256 threads, the grid stride, the partly idle tail block
   — on a host-built scene, and holds the result byte for byte, for both Reals, to the scene the host makes from the edited
   description: material_table + shape_record's meta + the placements' tags, light_records + light_power_tables.  No
   tolerance anywhere.
2. The symbols are declared, exported and bound, struct and dtype layouts are the header's, every refusal that needs no
   device is TAKE_E_INVALID with its message before a device is looked for, and valid arguments — with no GPU in the
   process — are refused with TAKE_E_NO_GPU, never served by a fallback.  (The handle is never read before a device is
   found: any non-NULL pointer will do here.  A range that ends beyond the scene's own table needs the handle and is
   refused after the device was found: tests/test_gpu_shading_update.py.)"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import shading_update_cases as K
from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_scene_set_materials", "take_hip_scene_set_light_intensities", "take_hip_scene_set_light_intensities_device",
           "take_hip_debug_shading_tables_info", "take_hip_debug_shading_tables")
F32, F64 = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64
MATERIAL_CASES, LIGHT_CASES = K.material_cases(), K.light_cases()
_LIB = None


# ------------------------------------------------------------------ 1. the kernels' bodies on the host
def host():
    global _LIB
    if _LIB is None:
        d = os.path.join(HERE, "shading_update_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libshading_update_host.so"))
        L.shading_update_last_error.restype = C.c_char_p
        L.shading_update_materials.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        L.shading_update_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        _LIB = L
    return _LIB


def host_materials(sd, first, new, burley=False, real=0, grid=0):
    """-> (mismatching parts, records, retagged) of the update run on the host against the scene made from the edited description"""
    a, keep_a = sd.to_desc()
    b, keep_b = K.with_materials(sd, first, new).to_desc()
    n, retagged = C.c_int64(), C.c_int()
    rc = host().shading_update_materials(C.addressof(a), C.addressof(b), first, len(new), int(burley), real, grid, 0, C.byref(n), C.byref(retagged))
    assert rc >= 0, host().shading_update_last_error().decode()
    return rc, n.value, bool(retagged.value)


def host_lights(sd, first, rgb, real=0, grid=0):
    a, keep_a = sd.to_desc()
    b, keep_b = K.with_intensities(sd, first, rgb).to_desc()
    rc = host().shading_update_lights(C.addressof(a), C.addressof(b), first, len(rgb), real, grid)
    assert rc >= 0, host().shading_update_last_error().decode()
    return rc


@pytest.mark.parametrize("real", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("name", [n for n in MATERIAL_CASES if n != "flattened"])  # (flattening is creation's: the host twin builds descriptions as they are)
def test_the_retag_leaves_the_records_creation_makes(name, real):
    sd, first, new, kw, retag = MATERIAL_CASES[name]
    rc, records, retagged = host_materials(sd, first, new, kw.get("burley_lobes", False), real)
    assert rc == 0 and retagged == retag
    if name.endswith("-records"):
        assert records == int(name.split("-")[0])


@pytest.mark.parametrize("real", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("grid", [1, 2, 3])
def test_blocks_that_stride_over_the_records_retag_them_all(grid, real):
    """fewer blocks than 256-record groups: every block takes several; 1301 records leave the last pass partly idle"""
    new = [K.mat(D.MAT_MIRROR), K.mat(D.MAT_PHONG), K.mat(D.MAT_PLASTIC)]
    rc, records, retagged = host_materials(K.flat(1290, 11), 0, new, real=real, grid=grid)
    assert (rc, records, retagged) == (0, 1301, True)


@pytest.mark.parametrize("real", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(LIGHT_CASES))
def test_the_light_tables_are_creation_s(name, real):
    sd, first, rgb = LIGHT_CASES[name]
    assert host_lights(sd, first, rgb, real) == 0


@pytest.mark.parametrize("real", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("grid", [1, 2])
def test_blocks_that_stride_over_the_lights(grid, real):
    sd = K.lit(700)
    assert host_lights(sd, 0, K.intensities(702, 5), real, grid) == 0 and host_lights(sd, 3, K.intensities(601, 6), real, grid) == 0


def test_a_wrong_table_is_noticed():
    """the comparison can fail: the twin is given an edited description that is NOT what the update was told"""
    sd, first, new, kw, _ = MATERIAL_CASES["mirror"]
    a, keep_a = sd.to_desc()
    b, keep_b = K.with_materials(sd, first, new).to_desc()
    b.materials[1].tag = D.MAT_PHONG  # (outside the range the update is given)
    rc = host().shading_update_materials(C.addressof(a), C.addressof(b), first, len(new), 0, 0, 0, 0, None, None)
    assert rc > 0 and rc & 1 and rc & 2 and rc & 8
    sd, first, rgb = LIGHT_CASES["sub-range"]
    a, keep_a = sd.to_desc()
    b, keep_b = K.with_intensities(sd, first, rgb).to_desc()
    b.lights[0].intensity[1] = 7.5
    rc = host().shading_update_lights(C.addressof(a), C.addressof(b), first, len(rgb), 0, 0)
    assert rc > 0 and rc & 16 and rc & 32


# ------------------------------------------------------------------ 2. the ABI
@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


@pytest.fixture()
def handle():
    buf = (C.c_char * 4096)()
    return C.cast(buf, C.c_void_p)


def no_gpu():
    import torch

    return not torch.cuda.is_available()


def test_the_five_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.SHADING_UPDATE_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.SHADING_UPDATE_PROTOTYPES[name], name
        declared = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(declared.split(",")) == len(D.SHADING_UPDATE_PROTOTYPES[name]), name
    assert [len(D.SHADING_UPDATE_PROTOTYPES[n]) for n in SYMBOLS] == [4, 4, 5, 3, 7]
    assert callable(capi.Scene.set_materials) and callable(capi.Scene.set_light_intensities) and callable(capi.Scene.debug_shading_tables)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_struct_and_dtype_layouts_are_the_library_s():
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){", 'printf("info %zu\\n", sizeof(TakeDebugShadingTablesInfo));',
            'printf("TakeMaterial %zu\\n", sizeof(TakeMaterial));']
    prog += [f'printf("info.{f} %zu\\n", offsetof(TakeDebugShadingTablesInfo, {f}));' for f, _ in D.TakeDebugShadingTablesInfo._fields_]
    prog.append("return 0;}")
    sizes = ['#include <cstddef>', '#include <cstdio>', '#include "take_hip.h"', '#include "tk_scene.h"', "using namespace tk;", "int main(){"]
    for r, t in (("4", "float"), ("8", "double")):
        sizes.append(f'std::printf("{r} %zu %zu %zu\\n", sizeof(MaterialRec<{t}>), sizeof(LightRec<{t}>), sizeof(InstShade<{t}>));')
        sizes.append(f'std::printf("{r}.offsets %zu %zu %zu %zu\\n", offsetof(MaterialRec<{t}>, p), offsetof(LightRec<{t}>, n), offsetof(InstShade<{t}>, material), offsetof(InstShade<{t}>, shape_base));')
    sizes.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(c, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        want = dict(line.split() for line in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines())
        cc, exe2 = os.path.join(td, "s.cpp"), os.path.join(td, "s")
        open(cc, "w").write("\n".join(sizes))
        subprocess.run(["g++", "-std=c++17", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "take_amd", "csrc"), cc, "-o", exe2], check=True)
        recs = {line.split()[0]: [int(x) for x in line.split()[1:]] for line in subprocess.run([exe2], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()}
    assert C.sizeof(D.TakeDebugShadingTablesInfo) == int(want["info"]) and C.sizeof(D.TakeMaterial) == int(want["TakeMaterial"])
    for f, _ in D.TakeDebugShadingTablesInfo._fields_:
        assert getattr(D.TakeDebugShadingTablesInfo, f).offset == int(want[f"info.{f}"]), f
    for rb in (4, 8):
        material, light, inst = D.shading_table_dtypes(rb)
        assert [material.itemsize, light.itemsize, inst.itemsize] == recs[str(rb)]
        assert [material.fields["p"][1], light.fields["n"][1], inst.fields["material"][1], inst.fields["shape_base"][1]] == recs[f"{rb}.offsets"]


def calls(lib, h, values, first, count):
    """the three entry points' answers to the same range, with the message of each"""
    m = None if values is None else (D.TakeMaterial * max(count, 1))()
    for k in range(max(count, 0) if m is not None else 0):
        D.fill_material(m[k], K.mat(D.MAT_DIFFUSE))
    rgb = None if values is None else (C.c_double * (3 * max(count, 1)))(*([1.0] * (3 * max(count, 1))))
    out = []
    for call in (lambda: lib.take_hip_scene_set_materials(h, m, first, count), lambda: lib.take_hip_scene_set_light_intensities(h, rgb, first, count),
                 lambda: lib.take_hip_scene_set_light_intensities_device(h, rgb, first, count, None)):
        rc = call()
        out.append((rc, lib.take_hip_last_error().decode()))
    return out


def test_null_arguments_are_refused_before_a_device_is_looked_for(lib, handle):
    for h, values in ((None, True), (handle, None)):
        for rc, msg in calls(lib, h, values, 0, 1):
            assert rc == D.TAKE_E_INVALID and "null argument" in msg


@pytest.mark.parametrize("count", [0, -1, -(2 ** 31)])
def test_a_count_that_is_not_positive_is_refused_before_a_device_is_looked_for(lib, handle, count):
    for rc, msg in calls(lib, handle, True, 0, count):
        assert rc == D.TAKE_E_INVALID and "count must be positive" in msg, msg


@pytest.mark.parametrize("first,count", [(-1, 1), (-(2 ** 31), 4), (2 ** 31 - 1, 1), (2 ** 31 - 4, 5), (1, 2 ** 31 - 1)])
def test_a_range_no_table_can_hold_is_refused_before_a_device_is_looked_for(lib, handle, first, count):
    m = (D.TakeMaterial * 1)()
    rgb = (C.c_double * 3)(1.0, 1.0, 1.0)  # (never read: the range is refused first)
    for rc in (lib.take_hip_scene_set_materials(handle, m, first, count), lib.take_hip_scene_set_light_intensities_device(handle, rgb, first, count, None)):
        assert rc == D.TAKE_E_INVALID and "outside the table" in lib.take_hip_last_error().decode()
    if first < 0:
        assert lib.take_hip_scene_set_light_intensities(handle, rgb, first, count) == D.TAKE_E_INVALID and "outside the table" in lib.take_hip_last_error().decode()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_an_intensity_that_is_not_finite_is_refused_before_a_device_is_looked_for(lib, handle, bad):
    for at in range(6):
        rgb = (C.c_double * 6)(*[bad if k == at else 1.0 for k in range(6)])
        assert lib.take_hip_scene_set_light_intensities(handle, rgb, 3, 2) == D.TAKE_E_INVALID
        msg = lib.take_hip_last_error().decode()
        assert f"light {3 + at // 3}" in msg and "must be finite" in msg, msg


def test_the_hook_refuses_null_arguments_before_it_looks_for_a_device(lib, handle):
    out, info = (C.c_char * 256)(), D.TakeDebugShadingTablesInfo()
    rcs = [lib.take_hip_debug_shading_tables_info(None, F32, C.byref(info)), lib.take_hip_debug_shading_tables_info(handle, F32, None),
           lib.take_hip_debug_shading_tables(None, F32, out, out, out, out, out)]
    rcs += [lib.take_hip_debug_shading_tables(handle, F32, *[None if k == missing else out for k in range(5)]) for missing in range(5)]
    for rc in rcs:
        assert rc == D.TAKE_E_INVALID
    assert b"null argument" in lib.take_hip_last_error()


def test_valid_arguments_without_a_gpu_are_no_gpu_not_a_fallback(lib, handle):
    if not no_gpu():
        pytest.skip("a GPU is visible: the no-GPU contract is checked in the CPU container")
    out, info = (C.c_char * 256)(), D.TakeDebugShadingTablesInfo()
    for rc, msg in calls(lib, handle, True, 0, 2) + calls(lib, handle, True, 5, 1):
        assert rc == D.TAKE_E_NO_GPU and "no CPU path" in msg
    assert lib.take_hip_debug_shading_tables_info(handle, F32, C.byref(info)) == D.TAKE_E_NO_GPU
    assert lib.take_hip_debug_shading_tables(handle, F64, out, out, out, out, out) == D.TAKE_E_NO_GPU


def test_to_desc_and_set_materials_fill_a_material_with_one_text():
    sd = K.flat(3, 1, (D.MAT_DIFFUSE, D.MAT_DISNEY_BSDF, D.MAT_PLASTIC))
    sd.materials[0] = K.mat(D.MAT_DIFFUSE, tex_image=0)
    desc, keep = sd.to_desc()
    for k, m in enumerate(sd.materials):
        c = D.TakeMaterial()
        D.fill_material(c, m)
        assert bytes(c) == bytes(desc.materials[k])
    assert desc.materials[1].param[11] == 1.5 and desc.materials[0].reflectance.kind == 1

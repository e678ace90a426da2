"""CPU side of take_hip_scene_set_envmap* and its test hook take_hip_debug_env_tables* (include/take_hip.h; DESIGN.md
§4o): the symbols are declared, exported and bound, the two structs have the header's layout, every refusal that needs
no device is TAKE_E_INVALID with its message before a device is looked for, and valid arguments — with no GPU in the
process — are refused with TAKE_E_NO_GPU, never served by a fallback.  (The handle is never read before a device is
found: any non-NULL pointer will do here.)"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_scene_set_envmap", "take_hip_scene_set_envmap_device", "take_hip_debug_env_tables_info", "take_hip_debug_env_tables")
F32, F64 = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


@pytest.fixture()
def handle():
    buf = (C.c_char * 4096)()
    return C.cast(buf, C.c_void_p)


def env_image(w=4, h=2, real=F64, flags=0, data=True):
    a = np.ones((max(h, 1), max(w, 1), 3), np.float64 if real != F32 else np.float32)
    im = D.TakeEnvImage(w, h, a.ctypes.data if data else None, real, flags)
    im.keep = a
    return im


def no_gpu():
    import torch

    return not torch.cuda.is_available()


def test_the_four_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.ENVMAP_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.ENVMAP_PROTOTYPES[name], name
        declared = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(declared.split(",")) == len(D.ENVMAP_PROTOTYPES[name]), name
    assert [len(D.ENVMAP_PROTOTYPES[n]) for n in SYMBOLS] == [3, 4, 3, 8]
    assert callable(capi.Scene.set_envmap) and callable(capi.Scene.debug_env_tables)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_the_structs_have_the_header_s_layout():
    structs = {"TakeEnvImage": D.TakeEnvImage, "TakeDebugEnvTablesInfo": D.TakeDebugEnvTablesInfo}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){"]
    for n, cls in structs.items():
        prog.append(f'printf("{n} %zu\\n", sizeof({n}));')
        prog += [f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f, _ in cls._fields_]
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(c, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        want = dict(line.split() for line in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines())
    for n, cls in structs.items():
        assert C.sizeof(cls) == int(want[n]), n
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == int(want[f"{n}.{f}"]), f"{n}.{f}"
    assert np.dtype(D.IMAGE_INFO_DTYPE).itemsize == 16


def both(lib, h, im, scale):
    """the two entry points' answers to the same arguments, with the message of each"""
    im = None if im is None else C.byref(im)
    out = []
    for call in (lambda: lib.take_hip_scene_set_envmap(h, im, scale), lambda: lib.take_hip_scene_set_envmap_device(h, im, scale, None)):
        rc = call()
        out.append((rc, lib.take_hip_last_error().decode()))
    return out


def test_null_arguments_are_refused_before_a_device_is_looked_for(lib, handle):
    for h, im in ((None, env_image()), (handle, None), (handle, env_image(data=False))):
        for rc, msg in both(lib, h, im, None):
            assert rc == D.TAKE_E_INVALID and "null argument" in msg


@pytest.mark.parametrize("im,what", [(env_image(w=0), "width and height"), (env_image(h=0), "width and height"), (env_image(w=-3), "width and height"),
                                     (env_image(h=-1), "width and height"), (env_image(real=D.TAKE_PRECISION_MIXED), "unknown real"),
                                     (env_image(real=7), "unknown real"), (env_image(real=-1), "unknown real"), (env_image(flags=2), "unknown flag bits"),
                                     (env_image(flags=D.TAKE_MESH_DEVICE_ARRAYS | 4), "unknown flag bits")])
def test_bad_images_are_refused_before_a_device_is_looked_for(lib, handle, im, what):
    for rc, msg in both(lib, handle, im, None):
        assert rc == D.TAKE_E_INVALID and what in msg, msg


@pytest.mark.parametrize("scale", [(np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf)])
def test_a_scale_that_is_not_finite_is_refused_before_a_device_is_looked_for(lib, handle, scale):
    for rc, msg in both(lib, handle, env_image(), D.c_double3(*scale)):
        assert rc == D.TAKE_E_INVALID and "scale must be finite" in msg, msg


def test_the_hook_refuses_null_arguments_before_it_looks_for_a_device(lib, handle):
    out, info = (C.c_char * 64)(), D.TakeDebugEnvTablesInfo()
    calls = [lib.take_hip_debug_env_tables_info(None, F32, C.byref(info)), lib.take_hip_debug_env_tables_info(handle, F32, None),
             lib.take_hip_debug_env_tables(None, F32, out, out, out, out, out, out)]
    calls += [lib.take_hip_debug_env_tables(handle, F32, *[None if k == missing else out for k in range(6)]) for missing in range(6)]
    for rc in calls:
        assert rc == D.TAKE_E_INVALID
    assert b"null argument" in lib.take_hip_last_error()


def test_valid_arguments_without_a_gpu_are_no_gpu_not_a_fallback(lib, handle):
    if not no_gpu():
        pytest.skip("a GPU is visible: the no-GPU contract is checked in the CPU container")
    out, info = (C.c_char * 64)(), D.TakeDebugEnvTablesInfo()
    for im, scale in ((env_image(), None), (env_image(real=F32), D.c_double3(1.0, 2.0, 3.0)), (env_image(flags=D.TAKE_MESH_DEVICE_ARRAYS), None)):
        for rc, msg in both(lib, handle, im, scale):
            assert rc == D.TAKE_E_NO_GPU and "no CPU path" in msg
    assert lib.take_hip_debug_env_tables_info(handle, F32, C.byref(info)) == D.TAKE_E_NO_GPU
    assert lib.take_hip_debug_env_tables(handle, F64, out, out, out, out, out, out) == D.TAKE_E_NO_GPU


def test_the_cli_takes_an_envmap_and_a_scale():
    from take_amd import render

    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "sky.npy")
        np.save(path, np.ones((2, 4, 3), np.float32))
        params = ["scene.tkscene", "-envmap", path, "-envscale", "1,0.5,2", "-max_depth", "3"]
        img, scale = render.parse_envmap(params)
        assert params == ["scene.tkscene", "-max_depth", "3"] and img.shape == (2, 4, 3) and scale == (1.0, 0.5, 2.0)
        assert render.parse_envmap(["scene.tkscene"]) is None
        for bad in (["-envscale", "1,2,3"], ["-envmap", path, "-envscale", "1,2"], ["-envmap", os.path.join(td, "none.npy")], ["-envmap", "sky.png"], ["-envmap"]):
            with pytest.raises(SystemExit):
                render.parse_envmap(bad)

"""The device build of an environment map's sampling tables (take_amd/csrc/tk_envmap.h, what take_hip_scene_set_envmap
runs) against scene creation's host build (env_tables and guide_table of take_amd/csrc/tk_host_scene.h), without a GPU:
tests/envbuild_host builds the kernels' bodies for the host and runs them in the launches' loop structure — blocks of 16
rows, tiles of 64 columns, the load, scan and store phase of every tile, one lane per table entry.

The bar is byte identity, for both Reals, of the marginal CDF, the conditional CDF and both guide tables: every sum is
the serial sum in the host's order, in double, -ffp-contract=off holds on both sides, and a side's tables are the
doubles rounded once.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envmap_cases as M
from helpers import HERE

_LIB = None


def host():
    global _LIB
    if _LIB is None:
        d = os.path.join(HERE, "envbuild_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libenvbuild_host.so"))
        L.envbuild_guide_sizes.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.envbuild_guide_sizes.restype = None
        L.envbuild_device.argtypes = [C.c_int32, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.envbuild_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int, C.c_int] + [C.c_void_p] * 4
        _LIB = L
    return _LIB


def guide_sizes(w, h):
    gm, gc = C.c_int32(), C.c_int32()
    host().envbuild_guide_sizes(w, h, C.byref(gm), C.byref(gc))
    return gm.value, gc.value


def tables(h, w, gm, gc, side):
    real = np.float64 if side else np.float32
    return [np.full(h + 1, -1, real), np.full((h, w + 1), -1, real), np.full(gm + 1, -1, np.int32), np.full((h, gc + 1), -1, np.int32)]


def device_build(img, side, grid=0, texels=False):
    """-> (rc, [marginal, conditional, guide_m, guide_c], float texels, double texels) of the device's code run on the host"""
    h, w, _ = img.shape
    gm, gc = guide_sizes(w, h)
    out = tables(h, w, gm, gc, side)
    tf, td = (np.full((h, w, 3), -1, np.float32), np.full((h, w, 3), -1, np.float64)) if texels else (None, None)
    rc = host().envbuild_device(1 if img.dtype == np.float64 else 0, img.ctypes.data, w, h, grid, side, gm, gc, *(a.ctypes.data for a in out),
                                None if tf is None else tf.ctypes.data, None if td is None else td.ctypes.data)
    return rc, out, tf, td


def host_build(img, side):
    h, w, _ = img.shape
    gm, gc = guide_sizes(w, h)
    out = tables(h, w, gm, gc, side)
    return host().envbuild_host(img.ctypes.data, w, h, side, gm, gc, *(a.ctypes.data for a in out)), out


def same_bytes(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("side", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(M.CASES))
def test_device_build_is_the_host_build_byte_for_byte(name, side):
    img = M.image(name)
    rc, got, tf, td = device_build(img, side, texels=True)
    rc_host, want = host_build(img, side)
    assert (rc, rc_host) == (0, 0)
    for what, a, b in zip(("marginal", "conditional", "guide_m", "guide_c"), got, want):
        assert a.tobytes() == b.tobytes(), what
    assert td.tobytes() == img.tobytes() and tf.tobytes() == img.astype(np.float32).tobytes()
    assert got[0][0] == 0 and got[0][-1] == 1 and np.all(got[1][:, 0] == 0) and np.all(got[1][:, -1] == 1)


@pytest.mark.parametrize("side", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("grid", [1, 2, 3])
def test_blocks_that_stride_over_the_rows_build_the_same_tables(grid, side):
    """fewer blocks than groups of 16 rows: every block takes several, and the running sums start afresh for each"""
    img = M.image("130x67")
    assert same_bytes(device_build(img, side, grid)[1], host_build(img, side)[1])


@pytest.mark.parametrize("side", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["ragged", "range", "65x63", "130x67"])
def test_float_texels_are_taken_as_their_values_widened_to_double(name, side):
    img32 = M.image(name).astype(np.float32)
    rc, got, tf, td = device_build(img32, side, texels=True)
    rc_host, want = host_build(img32.astype(np.float64), side)
    assert (rc, rc_host) == (0, 0) and same_bytes(got, want)
    assert tf.tobytes() == img32.tobytes() and td.tobytes() == img32.astype(np.float64).tobytes()


@pytest.mark.parametrize("side", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("make", [M.black, M.one_nan], ids=["black", "nan"])
def test_a_map_without_positive_luminance_is_refused_by_both(make, side):
    img = make()
    assert device_build(img, side)[0] == 1 and host_build(img, side)[0] == 1


def test_the_guide_sizes_follow_creation_s_rule(monkeypatch):
    assert guide_sizes(2048, 1024) == (4096, 2048) and guide_sizes(9000, 2) == (8, 8192) and guide_sizes(2, 16500) == (65536, 2)
    monkeypatch.setenv("TAKE_HIP_ENV_GUIDE", "4,2")
    assert guide_sizes(2048, 1024) == (4, 2)
    monkeypatch.setenv("TAKE_HIP_ENV_GUIDE", "3,2")  # (not a power of two: ignored)
    assert guide_sizes(64, 32) == (128, 64)

"""CPU side of the double-precision device build: the take_hip_scene_build_info entry point keeps the library's
contract without a GPU, and the outward double -> float rounding the device builder's boxes rest on
(take_amd/csrc/tk_round.h, built for the host by tests/round_shim) brackets every double between two adjacent floats."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_build_info_is_exported_and_rejects_a_null_scene(lib):
    assert "take_hip_scene_build_info" in capi.EXPORTS and hasattr(lib, "take_hip_scene_build_info")
    f, d = C.c_int32(7), C.c_int32(7)
    assert lib.take_hip_scene_build_info(None, C.byref(f), C.byref(d)) == D.TAKE_E_INVALID
    assert b"null scene" in lib.take_hip_last_error()
    assert (f.value, d.value) == (7, 7)
    assert lib.take_hip_abi_version() == 5  # a new symbol is no new ABI version


def test_build_info_without_gpu_is_no_gpu(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the no-GPU contract is checked in the CPU container")
    handle = (C.c_char * 64)()  # never read: without a device no scene exists, and the entry point says so first
    f, d = C.c_int32(7), C.c_int32(7)
    assert lib.take_hip_scene_build_info(C.cast(handle, C.c_void_p), C.byref(f), C.byref(d)) == D.TAKE_E_NO_GPU
    assert (f.value, d.value) == (7, 7)


@pytest.fixture(scope="module")
def shim():
    d = os.path.join(HERE, "round_shim")
    subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    L = C.CDLL(os.path.join(d, "libround_shim.so"))
    L.round_shim_outward.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.round_shim_neighbours.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return L


def outward(shim, x):
    x = np.ascontiguousarray(x, np.float64)
    lo, hi = np.zeros(x.shape, np.float32), np.zeros(x.shape, np.float32)
    shim.round_shim_outward(x.ctypes.data, x.size, lo.ctypes.data, hi.ctypes.data)
    return lo, hi


F32 = np.finfo(np.float32)
TINY = float(np.float32(1e-45))  # the smallest float denormal, 2^-149


def edge_cases():
    rng = np.random.default_rng(1)
    f = np.concatenate([
        np.array([0.0, 1.0, 1.5, 0.1, 1000.3, 2000.7, 500.1, 1e-3, float(F32.tiny), float(F32.max), TINY, 3 * TINY, 1e-40, 16777216.0, 16777217.0],
                 np.float64),
        rng.uniform(-2500, 2500, 2000), 10.0 ** rng.uniform(-44, 38, 2000), rng.uniform(-1e-3, 1e-3, 500)])
    f32 = f.astype(np.float32).astype(np.float64)  # values a float holds exactly
    xs = [f, f32, np.nextafter(f32, np.inf), np.nextafter(f32, -np.inf),  # ... and the doubles just above / below them
          np.array([5e-324, 1e-310, 2.0 ** -150, 2.0 ** -149 * 0.75, 2.0 ** -126 * (1 - 2.0 ** -30)]),  # below the float denormals / denormal range
          np.array([float(F32.max) * (1 + 2.0 ** -30), 1e39, 1e300, np.finfo(np.float64).max])]  # beyond the largest float
    x = np.concatenate(xs)
    return np.concatenate([x, -x])


def test_outward_rounding_brackets_every_double(shim):
    x = edge_cases()
    lo, hi = outward(shim, x)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    assert not np.isnan(lo).any() and not np.isnan(hi).any()
    assert (lo64 <= x).all() and (x <= hi64).all()
    with np.errstate(over="ignore"):
        exact = x.astype(np.float32).astype(np.float64) == x
    assert exact.sum() > 4000 and (~exact).sum() > 4000
    # a float comes back as itself (the sign of a zero aside, which no comparison sees) ...
    assert np.array_equal(lo64[exact], x[exact]) and np.array_equal(hi64[exact], x[exact])
    # ... anything else lies strictly between two ADJACENT floats
    assert (lo64[~exact] < x[~exact]).all() and (x[~exact] < hi64[~exact]).all()
    with np.errstate(over="ignore"):
        assert np.array_equal(np.nextafter(lo[~exact], np.float32(np.inf)), hi[~exact])
    # the far ends: finite on the inner side, the infinity on the outer one; 0 and the smallest denormal around a tiny double
    big = np.array([1e39, -1e39, 1e-310, -1e-310])
    lo, hi = outward(shim, big)
    assert lo[0] == F32.max and np.isposinf(hi[0]) and np.isneginf(lo[1]) and hi[1] == -F32.max
    assert lo[2] == 0 and hi[2] == np.float32(TINY) and lo[3] == -np.float32(TINY) and hi[3] == 0


def test_zero_keeps_its_value(shim):
    lo, hi = outward(shim, np.array([0.0, -0.0]))
    assert (lo == 0).all() and (hi == 0).all()


def test_float_neighbours(shim):
    x = np.array([0.0, -0.0, 1.0, -1.0, TINY, -TINY, float(F32.max), -float(F32.max), np.inf, -np.inf, 1000.3], np.float32)
    below, above = np.zeros_like(x), np.zeros_like(x)
    shim.round_shim_neighbours(x.ctypes.data, x.size, below.ctypes.data, above.ctypes.data)
    with np.errstate(over="ignore"):
        assert np.array_equal(below, np.nextafter(x, np.float32(-np.inf)))
        assert np.array_equal(above, np.nextafter(x, np.float32(np.inf)))

"""CPU side of motion blur (take_hip_shutter_plan, _shutter_pose, _render_shutter*: include/take_hip.h; DESIGN.md par.
4l): the plan against the numpy restatement (tests/shutter_ref.py), bit for bit; the refusals that need no device, and
the struct; the pose text the device runs (take_amd/csrc/tk_shutter.h) built for the host (tests/shutter_host) against
the restatement, bit for bit — both are the same IEEE double operations in the same order, nothing else is involved."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import shutter_ref as S
from helpers import HERE
from take_amd import capi, render
from take_amd import cdefs as D
from test_gpu_features import placement_transforms

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_shutter_plan", "take_hip_shutter_pose", "take_hip_render_shutter_device", "take_hip_render_shutter")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "shutter_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        lib_ = C.CDLL(os.path.join(d, "libshutter_host.so"))
        lib_.shutter_host_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
        lib_.shutter_host_lerp.argtypes = [C.c_double, C.c_double, C.c_double]
        lib_.shutter_host_lerp.restype = C.c_double
        _HOST = lib_
    return _HOST


def host_pose(marked, current, t):
    a, b = np.ascontiguousarray(marked, np.float64), np.ascontiguousarray(current, np.float64)
    n = a.size // 12
    out, ok = np.full((n, 3, 4), 7.0), np.full(n, -1, np.int32)
    assert host_lib().shutter_host_pose(a.ctypes.data, b.ctypes.data, n, t, out.ctypes.data, ok.ctypes.data) == 0
    return out, ok


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------ the plan
def check_plan(lib, spp, open, close, slices, K):
    first, time = capi.shutter_plan(spp, open, close, slices)
    want_first, want_time = S.plan(spp, open, close, slices)
    assert len(time) == K == len(want_time) and len(first) == K + 1, (spp, slices)
    assert np.array_equal(first, want_first), (spp, slices)
    assert first[0] == 0 and first[-1] == spp and (np.diff(first) >= 1).all(), (spp, slices, first)  # contiguous, covering, none empty
    assert same_bits(time, want_time), (spp, slices)
    assert (time[:-1] < time[1:]).all() if close > open else (time == open).all()
    return first, time


def test_the_plan_is_the_restatement_s(lib):
    for spp in range(1, 10):
        for K in range(1, spp + 1):
            check_plan(lib, spp, 0.0, 1.0, K, K)
            check_plan(lib, spp, 0.125, 0.7, K, K)
    first, time = check_plan(lib, 256, 0.0, 1.0, 16, 16)
    assert (np.diff(first) == 16).all() and time[0] == 1.0 / 32 and time[-1] == 31.0 / 32
    for default in (0, -3):
        check_plan(lib, 256, 0.1, 0.9, default, 16)  # the default: min(spp, 16)
    check_plan(lib, 5, 0.0, 1.0, 0, 5)
    check_plan(lib, 5, 0.0, 1.0, 40, 5)  # capped at spp
    check_plan(lib, 7, 0.2, 1.0, 3, 3)
    assert list(capi.shutter_plan(7, slices=3)[0]) == [0, 2, 4, 7]
    for oc in (0.0, 0.3, 1.0):
        _, time = check_plan(lib, 9, oc, oc, 4, 4)
        assert (time == oc).all()
    # a NULL shutter is {0, 1, 0, 0}; the arrays are optional
    k = C.c_int32()
    assert lib.take_hip_shutter_plan(40, None, C.byref(k), None, None) == 0 and k.value == 16
    time = (C.c_double * 16)()
    assert lib.take_hip_shutter_plan(40, None, C.byref(k), None, time) == 0 and same_bits(np.array(time[:]), S.plan(40)[1])


# ------------------------------------------------------------------ the boundary
def test_the_symbols_and_the_struct(lib):
    assert set(D.SHUTTER_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.SHUTTER_PROTOTYPES[name], name
    assert all(callable(getattr(capi.Scene, n)) for n in ("render_shutter", "render_shutter_device", "shutter_pose")) and callable(capi.shutter_plan)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){", 'printf("%zu", sizeof(TakeShutter));']
    prog += [f'printf(" %zu", offsetof(TakeShutter, {f}));' for f, _ in D.TakeShutter._fields_] + ["return 0;}"]
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [C.sizeof(D.TakeShutter)] + [getattr(D.TakeShutter, f).offset for f, _ in D.TakeShutter._fields_] == [24, 0, 8, 16, 20]


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU (`scene` is not a scene: a call that
    went past the argument check would not survive it)"""
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    img = C.cast(C.create_string_buffer(64), C.c_void_p)
    nan, inf = float("nan"), float("inf")
    k, cam = C.c_int32(), D.TakeCamera()

    def opts(spp=4):
        o = D.TakeRenderOpts()
        o.spp, o.max_depth, o.strip_stride = spp, 4, 1
        return C.byref(o)

    def sh(*a):
        return C.byref(D.TakeShutter(*a))

    bad_shutters = [((nan, 1.0, 0, 0), b"0 <= open <= close <= 1"), ((0.0, nan, 0, 0), b"0 <= open <= close <= 1"), ((0.0, inf, 0, 0), b"0 <= open <= close <= 1"),
                    ((-0.1, 1.0, 0, 0), b"0 <= open <= close <= 1"), ((0.0, 1.5, 0, 0), b"0 <= open <= close <= 1"), ((0.6, 0.5, 0, 0), b"0 <= open <= close <= 1"),
                    ((0.0, 1.0, 0, 1), b"unknown flag bits"), ((0.0, 1.0, 3, -8), b"unknown flag bits")]
    calls = [(lambda: lib.take_hip_shutter_plan(4, sh(0.0, 1.0, 0, 0), None, None, None), b"null argument"),
             (lambda: lib.take_hip_shutter_plan(0, sh(0.0, 1.0, 0, 0), C.byref(k), None, None), b"spp must be positive"),
             (lambda: lib.take_hip_shutter_plan(-2, None, C.byref(k), None, None), b"spp must be positive"),
             (lambda: lib.take_hip_shutter_pose(None, 0.5, C.byref(cam), None), b"null argument"),
             (lambda: lib.take_hip_shutter_pose(scene, 0.5, None, None), b"null argument"),
             (lambda: lib.take_hip_shutter_pose(scene, 1.5, C.byref(cam), None), b"t must be in [0, 1]"),
             (lambda: lib.take_hip_shutter_pose(scene, nan, C.byref(cam), None), b"t must be in [0, 1]"),
             (lambda: lib.take_hip_render_shutter(None, opts(), sh(0.0, 1.0, 0, 0), img), b"null argument"),
             (lambda: lib.take_hip_render_shutter(scene, None, sh(0.0, 1.0, 0, 0), img), b"null argument"),
             (lambda: lib.take_hip_render_shutter(scene, opts(), sh(0.0, 1.0, 0, 0), None), b"null argument"),
             (lambda: lib.take_hip_render_shutter(scene, opts(0), None, img), b"spp must be positive"),
             (lambda: lib.take_hip_render_shutter_device(None, opts(), None, img, None), b"null argument"),
             (lambda: lib.take_hip_render_shutter_device(scene, None, None, img, None), b"null argument"),
             (lambda: lib.take_hip_render_shutter_device(scene, opts(), None, None, None), b"null argument"),
             (lambda: lib.take_hip_render_shutter_device(scene, opts(-1), None, img, None), b"spp must be positive")]
    for a, msg in bad_shutters:
        calls.append((lambda a=a: lib.take_hip_shutter_plan(4, sh(*a), C.byref(k), None, None), msg))
        calls.append((lambda a=a: lib.take_hip_render_shutter(scene, opts(), sh(*a), img), msg))
        calls.append((lambda a=a: lib.take_hip_render_shutter_device(scene, opts(), sh(*a), img, None), msg))
    for call, msg in calls:
        assert call() == D.TAKE_E_INVALID and msg in lib.take_hip_last_error(), msg


def test_the_command_line_reads_the_shutter():
    p = ["scene.tkscene", "-shutter", "0.25,0.75", "-max_depth", "4", "-from_camera", "0,0.5,3.9,0,0,-1"]
    assert render.parse_shutter(p) == (0.25, 0.75, 0, (0.0, 0.5, 3.9), (0.0, 0.0, -1.0)) and p == ["scene.tkscene", "-max_depth", "4"]
    assert render.parse_shutter(["-slices", "8", "s", "-from_camera", "1,2,3,4,5,6", "-shutter", "0,1"]) == (0.0, 1.0, 8, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0))
    assert render.parse_shutter(["s", "-features"]) is None
    for bad in (["s", "-slices", "2"], ["s", "-from_camera", "1,2,3,4,5,6"], ["s", "-shutter", "0,1"], ["s", "-shutter"],
                ["s", "-shutter", "0", "-from_camera", "1,2,3,4,5,6"], ["s", "-shutter", "0,1", "-from_camera", "1,2,3"],
                ["s", "-shutter", "0,1", "-from_camera", "1,2,3,4,5,x"], ["s", "-shutter", "0,1", "-slices", "k", "-from_camera", "1,2,3,4,5,6"]):
        with pytest.raises(SystemExit):
            render.parse_shutter(bad)


# ------------------------------------------------------------------ the host build of the device text
def test_the_host_build_of_the_pose_is_the_restatement_s():
    a, b = placement_transforms(1), placement_transforms(2)
    assert a.shape == b.shape == (5, 3, 4) and not np.signbit(a[a == 0]).any() and not np.signbit(b[b == 0]).any()  # (no -0: the ends come back bit for bit)
    for t in (0.0, 1.0 / 3.0, 0.5, 1.0):
        got, ok = host_pose(a, b, t)
        assert same_bits(got, S.pose_xforms(t, a, b)), t
        assert (ok == 1).all() and not any(S.singular(x) for x in got), t
    assert same_bits(host_pose(a, b, 0.0)[0], a) and same_bits(host_pose(a, b, 1.0)[0], b)  # the ends are the inputs
    assert not same_bits(host_pose(a, b, 0.5)[0], a)
    for t, x, y in ((0.3, 1.5, -2.25), (1.0 / 3.0, 0.1, 0.7), (0.0, 4.0, 1e300), (1.0, -1e300, 0.1)):
        assert host_lib().shutter_host_lerp(t, x, y) == float(S.lerp(t, x, y))
    # what did not move stays where it is at every t, bit for bit — the three roundings of (1 - t) a + t a would not
    rng = np.random.default_rng(5)
    still = rng.normal(size=(64, 3, 4))
    drift = 0
    for t in (1.0 / 6.0, 0.3, 0.5, 5.0 / 6.0):
        got, ok = host_pose(still, still, t)
        assert same_bits(got, still) and same_bits(S.pose_xforms(t, still, still), still) and (ok == 1).all(), t
        drift += int(((np.float64(1.0) - np.float64(t)) * still + np.float64(t) * still != still).sum())
    assert drift > 0


def test_a_half_turn_passes_through_a_singular_pose():
    """identity -> a half turn about z: the chord of the rotation goes through diag(0, 0, 1) at t = 0.5"""
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    turn = np.concatenate([np.diag([-1.0, -1.0, 1.0]), np.array([[0.2], [0.0], [0.1]])], 1)
    marked, current = np.stack([eye, eye, eye]), np.stack([eye, turn, eye])
    got, ok = host_pose(marked, current, 0.5)
    assert list(ok) == [1, 0, 1] and S.singular(got[1]) and same_bits(got, S.pose_xforms(0.5, marked, current))
    assert list(host_pose(marked, current, 0.25)[1]) == [1, 1, 1] and list(host_pose(marked, current, 1.0)[1]) == [1, 1, 1]
    bad = current.copy()
    bad[2, 1, 3] = np.inf
    assert list(host_pose(marked, bad, 0.25)[1]) == [1, 1, 0]  # not finite

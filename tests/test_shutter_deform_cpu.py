"""CPU side of motion blur for deforming meshes (take_hip_shutter_vertices*, take_hip_render_shutter_meshes*:
include/take_hip.h; DESIGN.md par. 4r): the lerp the device runs over arrays (take_amd/csrc/tk_shutter.h) built for the
host (tests/shutter_deform_host) against the numpy restatement (tests/shutter_deform_ref.py), bit for bit — both are the
same IEEE double operations in the same order —; the struct; the refusals that need no device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import shutter_deform_ref as V
from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_shutter_vertices", "take_hip_shutter_vertices_device", "take_hip_render_shutter_meshes", "take_hip_render_shutter_meshes_device")
TIMES = (0.0, 1.0 / 3.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "shutter_deform_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        lib_ = C.CDLL(os.path.join(d, "libshutter_deform_host.so"))
        lib_.shutter_deform_host_vertices.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.POINTER(C.c_int32)]
        _HOST = lib_
    return _HOST


def host_vertices(a, b, t):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    out, moved = np.full(a.shape, 7.0), C.c_int32(-1)
    assert host_lib().shutter_deform_host_vertices(a.ctypes.data, b.ctypes.data, a.size, t, out.ctypes.data, C.byref(moved)) == 0
    return out, moved.value


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------ the host build of the device text
def test_the_host_build_of_the_lerp_over_arrays_is_the_restatement_s():
    a, b = V.edge_values()
    assert np.isnan(a).any() and np.isinf(b).any() and (a == b).any() and (np.abs(a[a != 0]) < np.finfo(np.float64).tiny).any()
    assert ((a == 1e300) & (b == -1e300)).any() and (np.signbit(a) & (a == 0)).any() and (np.signbit(b) & (b == 0)).any()
    for t in TIMES:
        got, moved = host_vertices(a, b, t)
        want, want_moved = V.vertices(t, a, b)
        assert same_bits(got, want) and moved == want_moved, t
        # what did not move stays where it is, bit for bit (a zero keeps the CURRENT end's sign); NaN and inf pass through
        still = a == b
        assert same_bits(got[still], b[still]), t
        assert np.isnan(got[np.isnan(a) | np.isnan(b)]).all(), t
    for seed, n in enumerate((1, 2, 3, 255, 257, 3 * 4099)):
        x, y = V.edge_arrays(n, seed)
        for t in TIMES:
            got, moved = host_vertices(x, y, t)
            want, want_moved = V.vertices(t, x, y)
            assert same_bits(got, want) and moved == want_moved, (n, t)


def test_the_ends_are_the_inputs():
    """t = 0 gives the marked array and t = 1 the current one, bit for bit, wherever both ends are finite and no zero
    changes its sign on the way (a zero that is lerped comes out as +0, and zeros of both signs are equal ends: tk_shutter.h)"""
    a, b = V.edge_arrays(3 * 4099, 11)
    plain = np.isfinite(a) & np.isfinite(b) & ~((a == 0) & np.signbit(a) & (a != b) | (b == 0) & np.signbit(b) & (a != b))
    plain &= ~((a == b) & (np.signbit(a) != np.signbit(b)))  # (+0 and -0 are equal ends: the result is the current one at every t)
    assert plain.mean() > 0.9
    a, b = a[plain], b[plain]
    at0, moved0 = host_vertices(a, b, 0.0)
    at1, moved1 = host_vertices(a, b, 1.0)
    assert same_bits(at0, a) and same_bits(at1, b) and moved0 == 1 and moved1 == 0
    assert same_bits(V.vertices(0.0, a, b)[0], a) and V.vertices(1.0, a, b)[1] == 0
    mid, moved = host_vertices(a, b, 0.5)
    assert moved == 1 and not same_bits(mid, a) and not same_bits(mid, b)
    # a mesh that did not move: no entry differs at any t, and the flag says so
    for t in TIMES:
        got, moved = host_vertices(b, b.copy(), t)
        assert same_bits(got, b) and moved == 0, t
    # one entry differs in its last bit: moved
    c = b.copy()
    c[len(c) // 2] = np.nextafter(c[len(c) // 2], np.inf)
    assert host_vertices(c, b, 0.0)[1] == 1 and V.vertices(0.0, c, b)[1] == 1  # (t = 0: the output is c)


# ------------------------------------------------------------------ the boundary
def test_the_symbols_and_the_struct(lib):
    assert set(D.SHUTTER_MESHES_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.SHUTTER_MESHES_PROTOTYPES[name], name
    assert all(callable(getattr(capi.Scene, n)) for n in ("render_shutter_meshes", "render_shutter_meshes_device")) and callable(capi.shutter_vertices)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){", 'printf("%zu", sizeof(TakeMeshMotion));']
    prog += [f'printf(" %zu", offsetof(TakeMeshMotion, {f}));' for f, _ in D.TakeMeshMotion._fields_] + ["return 0;}"]
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [C.sizeof(D.TakeMeshMotion)] + [getattr(D.TakeMeshMotion, f).offset for f, _ in D.TakeMeshMotion._fields_] == [40, 0, 4, 8, 16, 24, 32]


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU (`scene` is not a scene and the arrays
    are not device memory: a call that went past the argument check would not survive it)"""
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    img = C.cast(C.create_string_buffer(64), C.c_void_p)
    arr = C.cast(C.create_string_buffer(64), C.c_void_p).value
    nan, inf = float("nan"), float("inf")
    moved = C.c_int32()

    def opts(spp=4):
        o = D.TakeRenderOpts()
        o.spp, o.max_depth, o.strip_stride = spp, 4, 1
        return C.byref(o)

    def sh(*a):
        return C.byref(D.TakeShutter(*a))

    def motions(*recs):
        m = (D.TakeMeshMotion * max(len(recs), 1))()
        for k, r in enumerate(recs):
            m[k] = D.TakeMeshMotion(*r)
        return m

    good = (0, 0, arr, arr, None, None)
    calls = []
    for render in (lambda *a: lib.take_hip_render_shutter_meshes(*a), lambda *a: lib.take_hip_render_shutter_meshes_device(*a, None)):
        # everything take_hip_render_shutter* refuses there
        calls += [(lambda r=render: r(None, opts(), None, motions(good), 1, img), b"null argument"),
                  (lambda r=render: r(scene, None, None, motions(good), 1, img), b"null argument"),
                  (lambda r=render: r(scene, opts(), None, motions(good), 1, None), b"null argument"),
                  (lambda r=render: r(scene, opts(0), None, motions(good), 1, img), b"spp must be positive"),
                  (lambda r=render: r(scene, opts(-1), None, None, 0, img), b"spp must be positive")]
        for a, msg in (((nan, 1.0, 0, 0), b"0 <= open <= close <= 1"), ((0.0, inf, 0, 0), b"0 <= open <= close <= 1"), ((-0.1, 1.0, 0, 0), b"0 <= open <= close <= 1"),
                       ((0.0, 1.5, 0, 0), b"0 <= open <= close <= 1"), ((0.6, 0.5, 0, 0), b"0 <= open <= close <= 1"), ((0.0, 1.0, 0, 1), b"unknown flag bits")):
            calls.append((lambda r=render, a=a: r(scene, opts(), sh(*a), motions(good), 1, img), msg))
        # the motions
        calls += [(lambda r=render: r(scene, opts(), None, motions(good), -1, img), b"n must not be negative"),
                  (lambda r=render: r(scene, opts(), None, None, 1, img), b"null argument"),
                  (lambda r=render: r(scene, opts(), None, motions((0, 0, None, arr, None, None)), 1, img), b"motion 0: positions0 or positions1 is null"),
                  (lambda r=render: r(scene, opts(), None, motions(good, (1, 0, arr, None, None, None)), 2, img), b"motion 1: positions0 or positions1 is null"),
                  (lambda r=render: r(scene, opts(), None, motions((0, 0, arr, arr, arr, None)), 1, img), b"motion 0: normals0 and normals1 must be given together"),
                  (lambda r=render: r(scene, opts(), None, motions((0, 1, arr, arr, None, arr)), 1, img), b"motion 0: normals0 and normals1 must be given together"),
                  (lambda r=render: r(scene, opts(), None, motions((0, 2, arr, arr, None, None)), 1, img), b"motion 0: unknown flag bits"),
                  (lambda r=render: r(scene, opts(), None, motions(good, (1, -4, arr, arr, None, None)), 2, img), b"motion 1: unknown flag bits"),
                  (lambda r=render: r(scene, opts(), None, motions((-1, 0, arr, arr, None, None)), 1, img), b"motion 0: mesh index out of range"),
                  (lambda r=render: r(scene, opts(), None, motions((3, 0, arr, arr, None, None), good, (3, 1, arr, arr, arr, arr)), 3, img), b"mesh 3 appears more than once")]
    for vertices in (lambda a, b, n, t, out: lib.take_hip_shutter_vertices(a, b, n, t, out, C.byref(moved)),
                     lambda a, b, n, t, out: lib.take_hip_shutter_vertices_device(a, b, n, t, out, C.byref(moved), None),
                     lambda a, b, n, t, out: lib.take_hip_shutter_vertices_device(a, b, n, t, out, None, None)):
        calls += [(lambda v=vertices: v(None, arr, 3, 0.5, arr), b"null argument"), (lambda v=vertices: v(arr, None, 3, 0.5, arr), b"null argument"),
                  (lambda v=vertices: v(arr, arr, 3, 0.5, None), b"null argument"), (lambda v=vertices: v(arr, arr, 0, 0.5, arr), b"n must be positive"),
                  (lambda v=vertices: v(arr, arr, -3, 0.5, arr), b"n must be positive"), (lambda v=vertices: v(arr, arr, 3, -0.1, arr), b"t must be in [0, 1]"),
                  (lambda v=vertices: v(arr, arr, 3, 1.5, arr), b"t must be in [0, 1]"), (lambda v=vertices: v(arr, arr, 3, nan, arr), b"t must be in [0, 1]")]
    for call, msg in calls:
        assert call() == D.TAKE_E_INVALID and msg in lib.take_hip_last_error(), msg


def test_python_refuses_malformed_motions_before_the_library_is_called():
    sc = capi.Scene.__new__(capi.Scene)  # (no handle: _motions reads none)
    with pytest.raises(ValueError, match="a motion is"):
        sc._motions([(0, np.zeros((3, 3)))], None)
    with pytest.raises(ValueError, match="a motion is"):
        sc._motions([(0, np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3)))], None)
    recs, n, keep = sc._motions([(2, np.zeros((3, 3)), np.ones((3, 3))), (0, [[0.0, 1.0, 2.0]], [[0.0, 1.0, 2.5]], [[0.0, 0.0, 1.0]], [[0.0, 1.0, 0.0]])], None)
    assert n == 2 and len(keep) == 6 and recs[0].mesh == 2 and recs[0].flags == 0 and recs[0].normals0 is None and recs[1].normals1 == keep[5].ctypes.data

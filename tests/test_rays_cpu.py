"""CPU side of the caller-supplied rays (take_hip_render_rays*, take_hip_camera_rays*: include/take_hip.h; DESIGN.md
par. 4n): the two per-ray functions the device runs (take_amd/csrc/tk_rays.h: ray record -> initial path record, and back)
built for the host (tests/rays_host) against their specification — bits of origin and direction kept both ways, the
normalise flag against a numpy restatement of normalize, every other word equal to what generate_path writes
(tests/lens_host) — and the refusals that need no device, the layout of TakeRayBatch, the symbols.

Every comparison here is on bits: the functions copy, or run the one restated normalize."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import lens_ref as L
from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D
from test_lens_cpu import host_records, small_camera

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_render_rays_device", "take_hip_render_rays", "take_hip_camera_rays_device", "take_hip_camera_rays")
PATH_REC = 32
S_OX, S_DX, S_HIT, S_CTR, S_FLAGS, S_TX, S_LX, S_OCC, S_CONV = 0, 3, 9, 10, 11, 13, 16, 30, 31
WRITTEN = (0, 1, 2, 3, 4, 5, 10, 11, 13, 14, 15, 16, 17, 18, 30, 31)  # the words generate_path writes
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "rays_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        lib_ = C.CDLL(os.path.join(d, "librays_host.so"))
        lib_.rays_host_to_path.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        lib_.rays_host_to_ray.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
        assert lib_.rays_host_path_rec() == PATH_REC
        assert (lib_.rays_host_ray_bytes(0), lib_.rays_host_ray_bytes(1)) == (C.sizeof(D.TakeRayF), C.sizeof(D.TakeRayD)) == (32, 64)
        _HOST = lib_
    return _HOST


def to_path(rays, normalise=False, fill=7):
    """ray_to_path on (n, 8) rays -> (n, 32) records; the words it does not write hold `fill`"""
    rays = np.ascontiguousarray(rays)
    rec = np.full((rays.shape[0], PATH_REC), fill, rays.dtype)
    assert host_lib().rays_host_to_path(int(rays.dtype == np.float64), rays.ctypes.data, rays.shape[0], int(normalise), rec.ctypes.data) == 0
    return rec


def to_ray(rec, tmin):
    rec = np.ascontiguousarray(rec)
    rays = np.full((rec.shape[0], 8), 7, rec.dtype)
    assert host_lib().rays_host_to_ray(int(rec.dtype == np.float64), rec.ctypes.data, rec.shape[0], float(tmin), rays.ctypes.data) == 0
    return rays


def int_words(rec):
    """the low 32 bits of every word of the records, as the kernels' I_ accessor reads them"""
    rec = np.ascontiguousarray(rec)
    if rec.dtype == np.float32:
        return rec.view(np.int32)
    return (rec.view(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def restated_normalize(d):
    """tk_common.h: normalize — length = sqrt(x * x + y * y + z * z), then v * (1 / length) — one operation of the dtype
    each, in that order; a length <= 0 gives the zero vector"""
    return L._norm(np.ascontiguousarray(d), d.dtype.type)


def lens_records(dtype, with_lens):
    """generate_path's records of a small camera, (n, 32): what a render's generate pass writes"""
    cam = small_camera(dtype) if with_lens else small_camera(dtype, radius=0.0)
    return np.ascontiguousarray(host_records(cam, 3, 9, dtype, with_lens=with_lens).reshape(-1, PATH_REC))


# ------------------------------------------------------------------ the two functions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_lens", [False, True])
def test_record_to_ray_to_record_keeps_the_bits_of_origin_and_direction(dtype, with_lens):
    rec = lens_records(dtype, with_lens)
    rays = to_ray(rec, 1e-4)
    assert rays[:, 0:3].tobytes() == rec[:, S_OX:S_OX + 3].tobytes() and rays[:, 4:7].tobytes() == rec[:, S_DX:S_DX + 3].tobytes()
    assert (rays[:, 3] == dtype(1e-4)).all() and np.isposinf(rays[:, 7]).all()
    back = to_path(rays)
    assert back[:, 0:6].tobytes() == rec[:, 0:6].tobytes()
    # and the other way round: ray -> record -> ray, on rays that are no camera rays (negative zeros, denormals, huge values)
    rng = np.random.default_rng(3)
    mine = rng.normal(size=(257, 8)).astype(dtype)
    mine[0, 0:3], mine[1, 4:7], mine[2, 0] = -0.0, (0.0, -0.0, 1.0), np.finfo(dtype).tiny / 4
    mine[3, 1] = np.finfo(dtype).max
    again = to_ray(to_path(mine), 0.25)
    assert again[:, 0:3].tobytes() == mine[:, 0:3].tobytes() and again[:, 4:7].tobytes() == mine[:, 4:7].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_normalise_flag_is_the_restated_normalize(dtype):
    rng = np.random.default_rng(5)
    rays = rng.normal(size=(1000, 8)).astype(dtype)
    rays[:, 4:7] *= rng.uniform(0.01, 50.0, (1000, 1)).astype(dtype)
    rays[0, 4:7] = 0.0  # a zero direction stays zero
    rays[1, 4:7] = (0.0, 0.0, 4.0)
    got = to_path(rays, normalise=True)
    want = restated_normalize(rays[:, 4:7])
    assert want.dtype == dtype and got[:, S_DX:S_DX + 3].tobytes() == want.tobytes()
    assert (got[0, S_DX:S_DX + 3] == 0).all() and tuple(got[1, S_DX:S_DX + 3]) == (0.0, 0.0, 1.0)
    assert got[:, 0:3].tobytes() == rays[:, 0:3].tobytes()  # the origin is never touched
    # without the flag the direction is taken as it is
    assert to_path(rays)[:, S_DX:S_DX + 3].tobytes() == rays[:, 4:7].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_lens", [False, True])
def test_the_record_of_a_caller_ray_is_the_record_generate_path_writes(dtype, with_lens):
    """for a ray taken from a generate_path record the new function writes that record again: the same words, with the
    same bits — throughput 1, radiance 0, stream counter 2 (CAMERA_DRAWS), flags 0, no previous occluder, not converted —
    and leaves the words generate_path leaves"""
    rec = lens_records(dtype, with_lens)
    mine = to_path(to_ray(rec, 1e-4))
    assert mine.tobytes() == rec.tobytes()
    assert (mine[:, S_TX:S_TX + 3] == 1).all() and (mine[:, S_LX:S_LX + 3] == 0).all()
    iw = int_words(mine)
    assert (iw[:, S_CTR] == 2).all() and (iw[:, S_FLAGS] == 0).all() and (iw[:, S_OCC] == -1).all() and (iw[:, S_CONV] == 0).all()
    # which words are written: two fills (whose low halves differ in both dtypes) differ exactly in the words left alone
    a, b = to_path(to_ray(rec, 1e-4), fill=0.1), to_path(to_ray(rec, 1e-4), fill=0.3)
    written = [c for c in range(PATH_REC) if (int_words(a)[:, c] == int_words(b)[:, c]).all()]
    assert tuple(written) == WRITTEN


# ------------------------------------------------------------------ the boundary
def test_the_symbols_and_the_struct(lib):
    assert set(D.RAYS_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.RAYS_PROTOTYPES[name], name
    assert all(callable(getattr(capi.Scene, n)) for n in ("render_rays", "render_rays_device", "camera_rays", "camera_rays_device"))
    assert not any(hasattr(capi.SceneGroup, n) for n in ("render_rays", "camera_rays"))  # not for scene groups
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){", 'printf("%d %zu", TAKE_RAYS_NORMALIZE, sizeof(TakeRayBatch));']
    prog += [f'printf(" %zu", offsetof(TakeRayBatch, {f}));' for f, _ in D.TakeRayBatch._fields_] + ["return 0;}"]
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [D.TAKE_RAYS_NORMALIZE, C.sizeof(D.TakeRayBatch)] + [getattr(D.TakeRayBatch, f).offset for f, _ in D.TakeRayBatch._fields_]
    assert got == [1, 32, 0, 8, 16, 20, 24, 28]


def fake_scene(precision):
    """memory that is no scene, with the precision word a handle starts with: a call that went past its argument checks
    would not survive it"""
    buf = C.create_string_buffer(4096)
    C.cast(buf, C.POINTER(C.c_int32))[0] = precision
    return buf, C.cast(buf, C.c_void_p)


def opts(spp=4, max_depth=3, integrator=0):
    o = D.TakeRenderOpts()
    o.spp, o.max_depth, o.integrator = spp, max_depth, integrator
    return o


def unit_rays(n, dtype):
    r = np.zeros((n, 8), dtype)
    r[:, 6], r[:, 7] = 1.0, np.inf
    return r


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU"""
    keep, scene = fake_scene(D.TAKE_PRECISION_F32)
    rays, out = unit_rays(8, np.float32), np.zeros((8, 3), np.float32)
    R, O = rays.ctypes.data, out.ctypes.data

    def batch(ptr=R, n=2, ray_sets=1, first_sample=0, flags=0, reserved=0):
        return C.byref(D.TakeRayBatch(ptr, n, ray_sets, first_sample, flags, reserved))

    o = C.byref(opts())
    for entry, tail in ((lib.take_hip_render_rays, ()), (lib.take_hip_render_rays_device, (None,))):
        for call, msg in ((lambda: entry(None, o, batch(), O, *tail), b"null argument"),
                          (lambda: entry(scene, None, batch(), O, *tail), b"null argument"),
                          (lambda: entry(scene, o, None, O, *tail), b"null argument"),
                          (lambda: entry(scene, o, batch(ptr=None), O, *tail), b"null argument"),
                          (lambda: entry(scene, o, batch(), None, *tail), b"null argument"),
                          (lambda: entry(scene, C.byref(opts(spp=0)), batch(), O, *tail), b"spp must be positive"),
                          (lambda: entry(scene, C.byref(opts(max_depth=-2)), batch(), O, *tail), b"max_depth must be >= -1"),
                          (lambda: entry(scene, C.byref(opts(integrator=4)), batch(), O, *tail), b"unknown integrator"),
                          (lambda: entry(scene, o, batch(n=-1), O, *tail), b"n must be in [0, 2^30)"),
                          (lambda: entry(scene, o, batch(n=2 ** 30), O, *tail), b"n must be in [0, 2^30)"),
                          (lambda: entry(scene, o, batch(ray_sets=2), O, *tail), b"ray_sets must be 1 or spp"),
                          (lambda: entry(scene, o, batch(ray_sets=0), O, *tail), b"ray_sets must be 1 or spp"),
                          (lambda: entry(scene, o, batch(first_sample=-1), O, *tail), b"first_sample must be >= 0"),
                          (lambda: entry(scene, o, batch(first_sample=2 ** 31 - 4), O, *tail), b"first_sample + spp must fit int32"),
                          (lambda: entry(scene, o, batch(flags=2), O, *tail), b"unknown flag bits"),
                          (lambda: entry(scene, o, batch(flags=3), O, *tail), b"unknown flag bits"),
                          (lambda: entry(scene, o, batch(reserved=1), O, *tail), b"reserved must be 0")):
            assert call() == D.TAKE_E_INVALID and msg in lib.take_hip_last_error(), (entry.__name__, msg, lib.take_hip_last_error())
        # no rays: nothing to do, nothing looked for, nothing written (the pointers may then be NULL)
        assert entry(scene, o, batch(ptr=None, n=0), None, *tail) == D.TAKE_OK
        assert entry(scene, o, batch(n=0, ray_sets=4), O, *tail) == D.TAKE_OK and not out.any()
    assert lib.take_hip_render_rays_device(scene, o, batch(ptr=R + 4), O, None) == D.TAKE_E_INVALID and b"16-byte aligned" in lib.take_hip_last_error()
    ro = np.zeros((4, 8), np.float32).ctypes.data
    for call, msg in ((lambda: lib.take_hip_camera_rays(None, o, 0, ro), b"null argument"),
                      (lambda: lib.take_hip_camera_rays(scene, None, 0, ro), b"null argument"),
                      (lambda: lib.take_hip_camera_rays(scene, o, 0, None), b"null argument"),
                      (lambda: lib.take_hip_camera_rays(scene, C.byref(opts(spp=0)), 0, ro), b"spp must be positive"),
                      (lambda: lib.take_hip_camera_rays(scene, o, -1, ro), b"first_sample must be >= 0"),
                      (lambda: lib.take_hip_camera_rays(scene, o, 2 ** 31 - 2, ro), b"first_sample + spp must fit int32"),
                      (lambda: lib.take_hip_camera_rays_device(None, o, 0, ro, None), b"null argument"),
                      (lambda: lib.take_hip_camera_rays_device(scene, None, 0, ro, None), b"null argument"),
                      (lambda: lib.take_hip_camera_rays_device(scene, o, 0, None, None), b"null argument"),
                      (lambda: lib.take_hip_camera_rays_device(scene, C.byref(opts(spp=-3)), 0, ro, None), b"spp must be positive"),
                      (lambda: lib.take_hip_camera_rays_device(scene, o, -7, ro, None), b"first_sample must be >= 0"),
                      (lambda: lib.take_hip_camera_rays_device(scene, o, 0, ro + 8, None), b"16-byte aligned")):
        assert call() == D.TAKE_E_INVALID and msg in lib.take_hip_last_error(), (msg, lib.take_hip_last_error())
    del keep


@pytest.mark.parametrize("precision,dtype", [(D.TAKE_PRECISION_F32, np.float32), (D.TAKE_PRECISION_F64, np.float64), (D.TAKE_PRECISION_MIXED, np.float64)])
def test_the_host_entry_names_the_first_ray_it_cannot_use(lib, precision, dtype):
    """a non-finite component of org or dir, or — without TAKE_RAYS_NORMALIZE — a direction with | |d|^2 - 1 | > 1e-3:
    TAKE_E_INVALID naming the first such ray, before a device is looked for; tmin and tmax are not looked at"""
    keep, scene = fake_scene(precision)
    out = np.zeros((12, 3), dtype)
    o = C.byref(opts(spp=2))

    def call(rays, ray_sets=1, flags=0):
        b = D.TakeRayBatch(rays.ctypes.data, rays.shape[0] // ray_sets, ray_sets, 0, flags, 0)
        return lib.take_hip_render_rays(scene, o, C.byref(b), out.ctypes.data), lib.take_hip_last_error()

    def bad(k, c, v):
        r = unit_rays(12, dtype)
        r[:, 3], r[:, 7] = np.nan, -np.inf  # (ignored)
        r[k, c] = v
        r[11, 5] = 1.0  # a later offender: the message names the first
        return r

    for k, c, v, flags, msg in ((5, 0, np.nan, 0, b"ray 5: org and dir must be finite"), (7, 2, np.inf, 0, b"ray 7: org and dir must be finite"),
                                (3, 4, -np.inf, 0, b"ray 3: org and dir must be finite"), (0, 6, np.nan, D.TAKE_RAYS_NORMALIZE, b"ray 0: org and dir must be finite"),
                                (4, 6, 1.001, 0, b"ray 4: the direction is not of unit length"), (9, 6, 0.999, 0, b"ray 9: the direction is not of unit length"),
                                (6, 6, 0.0, 0, b"ray 6: the direction is not of unit length"), (6, 6, 0.0, D.TAKE_RAYS_NORMALIZE, b"ray 6: the direction's length is zero or overflows"),
                                (2, 6, np.finfo(dtype).max, D.TAKE_RAYS_NORMALIZE, b"ray 2: the direction's length is zero or overflows")):
        rc, err = call(bad(k, c, v), flags=flags)
        assert rc == D.TAKE_E_INVALID and msg in err, (k, c, v, err)
    # the second set of a ray_sets == spp batch is looked at too: ray index = set * n + i
    rc, err = call(bad(8, 1, np.nan), ray_sets=2)
    assert rc == D.TAKE_E_INVALID and b"ray 8: org and dir must be finite" in err
    # within the bar the rays pass this check, and the call goes on to look for a device: never TAKE_E_INVALID about a ray
    import torch

    if not torch.cuda.is_available():
        r = unit_rays(12, dtype)
        r[:, 6] = np.sqrt(1.0 + 9e-4)
        rc, err = call(r)
        assert rc == D.TAKE_E_NO_GPU, err
        r[:, 6] = 3.7
        assert call(r, flags=D.TAKE_RAYS_NORMALIZE)[0] == D.TAKE_E_NO_GPU
    del keep

"""CPU side of the image-space denoiser (take_hip_denoise, take_hip_denoise_device, take_hip_render_denoised and its
_device twin: include/take_hip.h): the symbols are declared, exported and bound, TakeDenoiseOpts has the header's layout,
every refusal is TAKE_E_INVALID with its message before a device is looked for; the text the device runs
(take_amd/csrc/tk_denoise.h) built for the host (tests/denoise_host) against the numpy restatement
(tests/denoise_ref.py); and the properties of the specification the GPU tests lean on, on the restatement alone.

Bars.  Host build against the restatement in f64: 1e-12 * max(1, max|ref|) on every value — the same operations in the
same order, only the C library's exp against numpy's may differ by an ulp, and it enters through a convex combination.
In f32: 1e-5 * max(1, max|ref|) against the f64 restatement of the float-rounded inputs (the f32 restatement is 4.5e-7
from it on these inputs; tests/test_gpu_denoise.py has the same bar)."""
import ctypes as C
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import denoise_ref
from helpers import HERE, rmse
from take_amd import capi
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_denoise", "take_hip_denoise_device", "take_hip_render_denoised", "take_hip_render_denoised_device")
GUIDES = ("albedo", "normal", "depth")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ------------------------------------------------------------------ the boundary
def test_the_four_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.DENOISE_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.DENOISE_PROTOTYPES[name], name
    assert [len(D.DENOISE_PROTOTYPES[n]) for n in SYMBOLS] == [7, 8, 4, 5]
    for f in (capi.denoise, capi.denoise_device, capi.Scene.render_denoised, capi.Scene.render_denoised_device):
        assert callable(f)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_the_struct_has_the_header_s_layout():
    names = [n for n, _ in D.TakeDenoiseOpts._fields_]
    assert names == ["iterations", "flags", "sigma_color", "sigma_normal", "sigma_depth", "albedo_floor"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){",
            'printf("size %zu\\n", sizeof(TakeDenoiseOpts));', 'printf("keep %d\\n", TAKE_DENOISE_KEEP_ALBEDO);']
    prog += [f'printf("{n} %zu\\n", offsetof(TakeDenoiseOpts, {n}));' for n in names]
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(c, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        want = dict(line.split() for line in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines())
    assert C.sizeof(D.TakeDenoiseOpts) == int(want["size"]) == 40
    assert D.TAKE_DENOISE_KEEP_ALBEDO == int(want["keep"])
    for n in names:
        assert getattr(D.TakeDenoiseOpts, n).offset == int(want[n]), n


def test_the_defaults_are_the_same_in_every_place():
    hdr = open(os.path.join(ROOT, "include", "take_hip.h")).read()
    for field, text in (("iterations", "<= 0: 5 */"), ("sigma_color", "<= 0: 1.0  */"), ("sigma_normal", "<= 0: 0.3  */"),
                        ("sigma_depth", "<= 0: 0.05 */"), ("albedo_floor", "<= 0: 1e-3 */")):
        line = next(l for l in hdr.splitlines() if re.search(r"\b" + field + r";", l))
        assert text in line, line
        assert float(text.split(":")[1].split("*")[0]) == D.DENOISE_DEFAULTS[field] == denoise_ref.DEFAULTS[field], field


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU.  (`scene` and the planes below are
    not a scene and not device memory: a call that went past the argument check would not survive it.)"""
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    ro = D.TakeRenderOpts()
    ro.spp = 1
    F32 = D.TAKE_PRECISION_F32

    def dev(rgb=buf, precision=F32, w=2, h=2, opts=None, out=buf):
        return lib.take_hip_denoise_device(rgb, None, precision, w, h, None if opts is None else C.byref(opts), out, None)

    def host(rgb=buf, precision=F32, w=2, h=2, opts=None, out=buf):
        return lib.take_hip_denoise(rgb, None, precision, w, h, None if opts is None else C.byref(opts), out)

    def rd(sc=scene, o=ro, opts=None, out=buf):
        return lib.take_hip_render_denoised_device(sc, None if o is None else C.byref(o), None if opts is None else C.byref(opts), out, None)

    def rh(sc=scene, o=ro, opts=None, out=buf):
        return lib.take_hip_render_denoised(sc, None if o is None else C.byref(o), None if opts is None else C.byref(opts), out)

    bad_opts = [(D.denoise_opts(iterations=9), b"iterations"), (D.TakeDenoiseOpts(0, 2, 0, 0, 0, 0), b"unknown flag"),
                (D.TakeDenoiseOpts(0, -1, 0, 0, 0, 0), b"unknown flag")]
    for k, field in enumerate(("sigma_color", "sigma_normal", "sigma_depth", "albedo_floor")):
        for v in (float("nan"), float("inf"), -float("inf")):
            o = D.TakeDenoiseOpts()
            setattr(o, field, v)
            bad_opts.append((o, b"must be finite"))
    cases = []
    for f in (dev, host):
        cases += [(lambda f=f: f(rgb=None), b"null argument"), (lambda f=f: f(out=None), b"null argument"),
                  (lambda f=f: f(w=0), b"width and height"), (lambda f=f: f(h=-3), b"width and height"),
                  (lambda f=f: f(precision=D.TAKE_PRECISION_MIXED), b"unknown precision"), (lambda f=f: f(precision=-1), b"unknown precision")]
    for f in (rd, rh):
        cases += [(lambda f=f: f(sc=None), b"null argument"), (lambda f=f: f(o=None), b"null argument"), (lambda f=f: f(out=None), b"null argument")]
    for f in (dev, host, rd, rh):
        cases += [(lambda f=f, o=o: f(opts=o), msg) for o, msg in bad_opts]
    assert len(cases) == 2 * 6 + 2 * 3 + 4 * 15
    for call, msg in cases:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert b"null scene" in lib.take_hip_last_error()
        assert call() == D.TAKE_E_INVALID
        assert msg in lib.take_hip_last_error(), (msg, lib.take_hip_last_error())


def test_the_python_binding_checks_its_arrays():
    rgb = np.zeros((4, 5, 3), np.float32)
    for kw in (dict(rgb=np.zeros((4, 5, 3), np.int32)), dict(rgb=np.zeros((4, 5), np.float32)), dict(rgb=rgb, depth=np.zeros((4, 5, 1), np.float32)),
               dict(rgb=rgb, albedo=np.zeros((4, 5, 3), np.float64)), dict(rgb=rgb, opts=D.denoise_opts(), iterations=2)):
        with pytest.raises(ValueError):
            capi.denoise(**kw)


# ------------------------------------------------------------------ host execution of tk_denoise.h
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "denoise_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libdenoise_host.so"))
        L.denoise_host.argtypes = [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]
        _HOST = L
    return _HOST


def host_denoise(p, in_place=False, **opts):
    """p: contiguous planes of one dtype, a subset of rgb / albedo / normal / depth -> what the kernels' text computes"""
    o = dict(denoise_ref.DEFAULTS)
    o.update(opts)
    rgb = p["rgb"].copy()
    out = rgb if in_place else np.full_like(rgb, np.nan)
    sf = np.array([o["sigma_color"], o["sigma_normal"], o["sigma_depth"], o["albedo_floor"]], np.float64)
    rc = host_lib().denoise_host(int(rgb.dtype == np.float64), rgb.ctypes.data, *[p[g].ctypes.data if g in p else None for g in GUIDES],
                                 rgb.shape[1], rgb.shape[0], o["iterations"], int(o["keep_albedo"]), sf.ctypes.data, out.ctypes.data)
    assert rc == 0
    return out


_PLANES = {}


def noisy(size):
    """the synthetic planes with 30 % multiplicative noise, made once per size and never written to"""
    if size not in _PLANES:
        _PLANES[size] = denoise_ref.planes(*size, noise=0.3)
    return _PLANES[size]


def subsets():
    return [tuple(g for g, on in zip(GUIDES, mask) if on) for mask in itertools.product((0, 1), repeat=3)]


# (size, guides, options): every size with all guides and the defaults; on 37 x 23 the iteration counts, every subset of
# the guides, KEEP_ALBEDO and other sigmas — the cases of tests/test_gpu_denoise.py
CASES = [(s, GUIDES, {}) for s in denoise_ref.SIZES]
CASES += [((37, 23), GUIDES, dict(iterations=n)) for n in (1, 8)]
CASES += [((37, 23), g, {}) for g in subsets() if g != GUIDES]
CASES += [((37, 23), GUIDES, dict(keep_albedo=True)),
          ((37, 23), GUIDES, dict(sigma_color=0.4, sigma_normal=0.7, sigma_depth=0.2, albedo_floor=0.05, iterations=3))]


def case_id(c):
    (w, h), g, o = c
    return f"{w}x{h}-{'+'.join(g) or 'none'}-" + (",".join(f"{k}={v}" for k, v in o.items()) or "defaults")


def check(got, ref, bar, label):
    d = float(np.abs(got.astype(np.float64) - ref).max())
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"{label}: max |difference| {d:.3e}, bar {bar * scale:.3e}")
    assert np.isfinite(got).all() and d <= bar * scale, (label, d)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_build_against_the_restatement_f64(case):
    size, guides, opts = case
    p = denoise_ref.cast(noisy(size), np.float64)
    p = {k: v for k, v in p.items() if k == "rgb" or k in guides}
    check(host_denoise(p, **opts), denoise_ref.denoise(**p, **opts), 1e-12, "f64 " + case_id(case))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_host_build_against_the_restatement_f32(case):
    size, guides, opts = case
    p = denoise_ref.cast(noisy(size), np.float32)
    p = {k: v for k, v in p.items() if k == "rgb" or k in guides}
    got = host_denoise(p, **opts)
    assert got.dtype == np.float32
    ref64 = denoise_ref.denoise(**{k: v.astype(np.float64) for k, v in p.items()}, **opts)
    check(got, ref64, 1e-5, "f32 against f64 " + case_id(case))
    check(denoise_ref.denoise(**p, **opts), ref64, 1e-5, "f32 restatement against f64 " + case_id(case))


def test_host_build_in_place_and_repeated():
    p = denoise_ref.cast(noisy((37, 23)), np.float64)
    a = host_denoise(p)
    assert np.array_equal(a, host_denoise(p)) and np.array_equal(a, host_denoise(p, in_place=True))


def test_the_cases_can_tell_a_wrong_level_from_a_right_one():
    """one level fewer moves the result by four orders above either bar: a wrong tap, step, weight or level constant shows"""
    p = denoise_ref.cast(noisy((37, 23)), np.float64)
    d = float(np.abs(denoise_ref.denoise(**p, iterations=4) - denoise_ref.denoise(**p)).max())
    print(f"iterations 4 against 5: {d:.3e}")
    assert d > 1e-3


# ------------------------------------------------------------------ properties of the specification (the restatement alone)
def test_texture_detail_survives_demodulation():
    p = denoise_ref.cast(denoise_ref.planes(130, 70), np.float64)
    assert (p["albedo"] == 0).any() and len(np.unique(p["albedo"].reshape(-1, 3), axis=0)) == 3  # sky + the two checker colours
    kept = float(np.abs(denoise_ref.denoise(**p) - p["rgb"]).max())
    blurred = float(np.abs(denoise_ref.denoise(**p, keep_albedo=True) - p["rgb"]).max())
    print(f"demodulated: {kept:.3e}; KEEP_ALBEDO: {blurred:.3f}")
    assert kept <= 1e-12 and blurred > 0.1


def test_noise_goes_down():
    raw = noisy((130, 70))
    p = denoise_ref.cast(raw, np.float64)
    before, after = rmse(p["rgb"], raw["clean"]), rmse(denoise_ref.denoise(**p), raw["clean"])
    print(f"RMSE to the clean image: {before:.4f} -> {after:.4f}")
    assert after < before

"""CPU side of bloom and the image workspace (take_hip_image_workspace_*, take_hip_bloom_layer*, take_hip_tonemap_bloom*:
include/take_hip.h): the symbols are declared, exported and bound, TakeBloomOpts has the header's layout,
the defaults are the same in every place, every refusal is TAKE_E_INVALID with its message before a device is looked
for; the text the device runs (take_amd/csrc/tk_bloom.h) built for the host (tests/bloom_host) against the numpy
restatement (tests/bloom_ref.py); and the properties of the specification, on the restatement alone.

Bars.  The layer, and the composite with LINEAR transfer (REAL outputs and RGBA codes): bit-identical in f32 and in f64 —
there is no pow and no log before the transfer, and every order of additions is fixed.  SRGB: display_ref's bars
unchanged (A = 16 ulp of 1.0 on REAL outputs; RGBA codes differ by at most 1, only where the restatement's unrounded
value lies within 255 A of an integer, in at most 0.5 % of the channels, after the restatement alone has shown that at
most 0.5 % of its channels lie that close): what goes into pow is bit-identical, so nothing new enters."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import bloom_ref as ref
import display_ref as dref
from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_image_workspace_create", "take_hip_image_workspace_destroy", "take_hip_bloom_layer_device", "take_hip_bloom_layer",
           "take_hip_tonemap_bloom_device", "take_hip_tonemap_bloom")
BLOOM_FIELDS = ["threshold", "knee", "intensity", "levels", "reserved"]
F32, F64 = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ------------------------------------------------------------------ the boundary
def test_the_six_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.BLOOM_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.BLOOM_PROTOTYPES[name], name
        declared = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(declared.split(",")) == len(D.BLOOM_PROTOTYPES[name]), name
    assert [len(D.BLOOM_PROTOTYPES[n]) for n in SYMBOLS] == [1, 1, 9, 7, 10, 8]
    for f in (capi.ImageWorkspace, capi.bloom_layer, capi.bloom_layer_device, capi.tonemap_bloom, capi.tonemap_bloom_device):
        assert callable(f)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_the_struct_has_the_header_s_layout():
    assert [n for n, _ in D.TakeBloomOpts._fields_] == BLOOM_FIELDS
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){",
            'printf("TakeBloomOpts %zu\\n", sizeof(TakeBloomOpts));', 'printf("TAKE_BLOOM_MAX_LEVELS %d\\n", TAKE_BLOOM_MAX_LEVELS);']
    prog += [f'printf("b.{n} %zu\\n", offsetof(TakeBloomOpts, {n}));' for n in BLOOM_FIELDS]
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(c, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        want = dict(line.split() for line in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines())
    assert C.sizeof(D.TakeBloomOpts) == int(want["TakeBloomOpts"]) == 32
    assert D.TAKE_BLOOM_MAX_LEVELS == ref.MAX_LEVELS == int(want["TAKE_BLOOM_MAX_LEVELS"]) == 8
    for n in BLOOM_FIELDS:
        assert getattr(D.TakeBloomOpts, n).offset == int(want["b." + n]), n


def test_the_defaults_are_the_same_in_every_place():
    hdr = open(os.path.join(ROOT, "include", "take_hip.h")).read()
    hdr = hdr[hdr.index("typedef struct TakeBloomOpts"):hdr.index("} TakeBloomOpts;")]
    assert set(D.BLOOM_DEFAULTS) == set(ref.DEFAULTS) == {"threshold", "knee", "intensity"}
    for field in D.BLOOM_DEFAULTS:
        line = next(l for l in hdr.splitlines() if re.search(r"^\s+double " + field + r";", l))
        value = float(re.search(r"< 0: ([0-9.]+)", line).group(1))
        assert value == D.BLOOM_DEFAULTS[field] == ref.DEFAULTS[field], (field, line)
    line = next(l for l in hdr.splitlines() if re.search(r"^\s+int32_t levels;", l))
    assert "<= 0: all" in line
    o = D.bloom_opts()
    assert (o.threshold, o.knee, o.intensity, o.levels, o.reserved) == (-1.0, -1.0, -1.0, 0, 0)


def bad_bloom_opts():
    """(TakeBloomOpts, the message's part) for everything the calls refuse of their bloom options"""
    out = []
    for field in ("threshold", "knee", "intensity"):
        for v in (float("nan"), float("inf"), -float("inf")):
            o = D.bloom_opts()
            setattr(o, field, v)
            out.append((o, b"must be finite"))
    out += [(D.bloom_opts(threshold=0.25), b"knee"), (D.bloom_opts(knee=1.5), b"knee"), (D.bloom_opts(threshold=0.5, knee=0.75), b"knee"),
            (D.bloom_opts(threshold=0.0), b"knee"), (D.bloom_opts(levels=9), b"levels"), (D.bloom_opts(levels=1 << 20), b"levels")]
    reserved = D.bloom_opts()
    reserved.reserved = 1
    out.append((reserved, b"reserved"))
    assert len(out) == 9 + 7
    return out


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU.  (The planes below are not device
    memory: a call that went past the argument check would not survive it.)"""
    buf = C.cast(C.create_string_buffer(256), C.c_void_p)
    other = C.cast(C.create_string_buffer(256), C.c_void_p)
    E = C.c_double(0.0)

    def ref_(o):
        return None if o is None else C.byref(o)

    def ld(rgb=buf, precision=F32, w=2, h=2, exposure=1.0, bloom=None, out=other):
        return lib.take_hip_bloom_layer_device(rgb, precision, w, h, exposure, ref_(bloom), out, None, None)

    def lh(rgb=buf, precision=F32, w=2, h=2, exposure=1.0, bloom=None, out=other):
        return lib.take_hip_bloom_layer(rgb, precision, w, h, exposure, ref_(bloom), out)

    def td(rgb=buf, precision=F32, w=2, h=2, opts=None, bloom=None, out=other):
        return lib.take_hip_tonemap_bloom_device(rgb, precision, w, h, ref_(opts), ref_(bloom), out, None, None, None)

    def th(rgb=buf, precision=F32, w=2, h=2, opts=None, bloom=None, out=other):
        return lib.take_hip_tonemap_bloom(rgb, precision, w, h, ref_(opts), ref_(bloom), out, C.byref(E))

    def topts(**kw):
        o = D.tonemap_opts(exposure=1.0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    cases = [(lambda: lib.take_hip_image_workspace_create(None), b"null argument")]
    for f in (ld, lh, td, th):
        cases += [(lambda f=f: f(rgb=None), b"null argument"), (lambda f=f: f(out=None), b"null argument"),
                  (lambda f=f: f(w=0), b"width and height"), (lambda f=f: f(h=-3), b"width and height"),
                  (lambda f=f: f(precision=D.TAKE_PRECISION_MIXED), b"unknown precision"), (lambda f=f: f(precision=-1), b"unknown precision")]
        cases += [(lambda f=f, o=o: f(bloom=o), msg) for o, msg in bad_bloom_opts()]
    for f in (ld, lh):
        cases += [(lambda f=f, e=e: f(exposure=e), b"exposure") for e in (0.0, -1.0, float("nan"), float("inf"), -float("inf"))]
        # 2 x 2 pixels: 48 bytes of floats.  The layer on the input is allowed (refused later, for want of a device, or run)
        cases += [(lambda f=f: f(out=C.c_void_p(buf.value + 44)), b"partly overlap"), (lambda f=f: f(rgb=C.c_void_p(buf.value + 4), out=buf), b"partly overlap")]
    # everything take_hip_tonemap* refuses (tests/test_display_cpu.py has the full list; here one of each kind)
    bad_tonemap = [(topts(op=3), b"unknown tone operator"), (topts(transfer=2), b"unknown transfer"), (topts(format=-1), b"unknown output format"),
                   (topts(reserved=1), b"reserved"), (topts(exposure=float("nan")), b"must be finite"), (topts(white=float("inf")), b"must be finite"),
                   (topts(auto_opts=D.exposure_opts(rate=1.25)), b"rate"), (topts(exposure=0.0, auto_opts=D.exposure_opts(low_fraction=0.96)), b"low_fraction")]
    for f in (td, th):
        cases += [(lambda f=f, o=o: f(opts=o), msg) for o, msg in bad_tonemap]
        cases += [(lambda f=f: f(out=buf), b"overlap"), (lambda f=f: f(opts=topts(), out=C.c_void_p(buf.value + 44)), b"overlap"),
                  (lambda f=f: f(rgb=C.c_void_p(buf.value + 12), out=buf), b"overlap")]
    cases += [(lambda: td(out=C.c_void_p(other.value + 2)), b"4-byte aligned")]
    assert len(cases) == 1 + 4 * (6 + 16) + 2 * (5 + 2) + 2 * (8 + 3) + 1
    for call, msg in cases:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert b"null scene" in lib.take_hip_last_error()
        assert call() == D.TAKE_E_INVALID
        assert msg in lib.take_hip_last_error(), (msg, lib.take_hip_last_error())
    lib.take_hip_image_workspace_destroy(None)  # a no-op


def test_what_is_allowed_goes_on_to_look_for_a_device(lib):
    """intensity 0, knee == threshold, levels == TAKE_BLOOM_MAX_LEVELS and a layer written over its input pass the
    argument check: without a GPU the answer is TAKE_E_NO_GPU, never TAKE_E_INVALID.  (With one, the host twins run.)"""
    img = np.zeros((2, 2, 3), np.float32)
    out = np.zeros_like(img)
    for o in (D.bloom_opts(intensity=0.0), D.bloom_opts(threshold=0.5, knee=0.5), D.bloom_opts(threshold=0.0, knee=0.0), D.bloom_opts(levels=8)):
        for dst in (out, img):
            rc = lib.take_hip_bloom_layer(img.ctypes.data, F32, 2, 2, 1.0, C.byref(o), dst.ctypes.data)
            assert rc in (D.TAKE_OK, D.TAKE_E_NO_GPU), lib.take_hip_last_error()


def test_the_python_binding_checks_its_arguments():
    img = np.zeros((4, 5, 3), np.float32)
    for bad in (np.zeros((4, 5, 3), np.int32), np.zeros((4, 5), np.float32), np.zeros((4, 5, 4), np.float32)):
        with pytest.raises(ValueError):
            capi.bloom_layer(bad, 1.0)
        with pytest.raises(ValueError):
            capi.tonemap_bloom(bad)
    for kw in (dict(op="filmic"), dict(bloom=D.bloom_opts(), knee=0.1), dict(opts=D.tonemap_opts(), white=2.0), dict(opts=D.tonemap_opts(), exposure=1.0)):
        with pytest.raises(ValueError):
            capi.tonemap_bloom(img, **kw)
    with pytest.raises(ValueError):
        capi.bloom_layer(img, 1.0, white=2.0)
    with pytest.raises(ValueError):
        capi.tonemap_bloom_device(1 << 20, 2, 2, F32)  # RGBA without an output plane
    with pytest.raises(ValueError):
        capi.tonemap_bloom_device(1 << 20, 2, 2, F32, out=1 << 21, workspace=object())
    names = capi._bloom_opts(None, dict(threshold=2.0, levels=3))
    assert (names.threshold, names.knee, names.intensity, names.levels) == (2.0, -1.0, -1.0, 3) and capi._bloom_opts(None, {}) is None


def test_the_command_line_refuses_bloom_without_png():
    from take_amd import render

    with pytest.raises(SystemExit) as e:
        render.main(["scene.tkscene", "-bloom"])
    assert "-bloom needs -png" in str(e.value)
    with pytest.raises(SystemExit):
        render.main(["-bloom", "0.5", "scene.tkscene"])


# ------------------------------------------------------------------ host execution of tk_bloom.h
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "bloom_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libbloom_host.so"))
        L.bloom_pyramid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.bloom_layer.argtypes = [C.c_int32, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
        L.bloom_tonemap.argtypes = [C.c_int32, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                    C.c_double, C.c_int, C.c_void_p]
        _HOST = L
    return _HOST


def host_pyramid(w, h, levels=0):
    ws, hs = np.zeros(8, np.int32), np.zeros(8, np.int32)
    n = host_lib().bloom_pyramid(w, h, levels, ws.ctypes.data, hs.ctypes.data)
    assert n >= 1
    return [(int(a), int(b)) for a, b in zip(ws[:n], hs[:n])]


def host_layer(rgb, exposure, in_place=False, **bloom):
    threshold, knee, intensity, levels = ref.resolved(**bloom)
    rgb = np.ascontiguousarray(rgb).copy()
    out = rgb if in_place else np.full_like(rgb, np.nan)
    assert host_lib().bloom_layer(int(rgb.dtype == np.float64), rgb.ctypes.data, rgb.shape[1], rgb.shape[0], exposure, threshold, knee, intensity, levels,
                                  out.ctypes.data) == 0
    return out


def host_tonemap(rgb, exposure, op, transfer, format, white=dref.DEFAULTS["white"], in_place=False, **bloom):
    threshold, knee, intensity, levels = ref.resolved(**bloom)
    rgb = np.ascontiguousarray(rgb).copy()
    if format == D.TAKE_DISPLAY_RGBA:
        out = np.zeros(rgb.shape[:2] + (4,), np.uint8)
    else:
        out = rgb if in_place else np.full_like(rgb, np.nan)
    assert host_lib().bloom_tonemap(int(rgb.dtype == np.float64), rgb.ctypes.data, rgb.shape[1], rgb.shape[0], exposure, white, op, transfer, format, threshold,
                                    knee, intensity, levels, out.ctypes.data) == 0
    return out


def test_pyramid_sizes_follow_step_3():
    want = {(1, 1): [(1, 1)], (2, 1): [(1, 1)], (3, 5): [(2, 3), (1, 2), (1, 1)],
            (257, 3): [(129, 2), (65, 1), (33, 1), (17, 1), (9, 1), (5, 1), (3, 1), (2, 1)]}  # (the ninth would be 1 x 1: capped at 8)
    for (w, h), sizes in want.items():
        assert ref.pyramid(w, h) == host_pyramid(w, h) == sizes, (w, h)
        for levels in (1, 2, 3, 8):
            assert ref.pyramid(w, h, levels) == host_pyramid(w, h, levels) == sizes[:levels], (w, h, levels)
    for w, h in ref.SHAPES + [(1920, 1080), (100000, 7)]:
        sizes = ref.pyramid(w, h)
        assert sizes == host_pyramid(w, h) and 1 <= len(sizes) <= ref.MAX_LEVELS
        assert sizes[0] == ((w + 1) // 2, (h + 1) // 2) and (len(sizes) == ref.MAX_LEVELS or sizes[-1] == (1, 1))
        assert all(s != (1, 1) for s in sizes[:-1])


# the shapes and images of the host comparison: the GPU test's, all of them — 257 x 3 has the eight levels of the cap,
# 641 x 97 a wide level 0 — and 67 x 37, whose level 0 (34 x 19) has an even and an odd axis; and the midrange image
HOST_SHAPES = list(ref.SHAPES) + [(67, 37)]
HOST_CONTENTS = tuple(ref.CONTENTS) + ("midrange",)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("options", list(ref.OPTION_SETS))
def test_host_build_layer_is_bit_identical(options, dtype):
    kw = ref.OPTION_SETS[options]
    for shape in HOST_SHAPES:
        for content in HOST_CONTENTS:
            img = ref.image(content, shape, dtype)
            for exposure in (1.0, 0.37):
                want = ref.layer(img, exposure, **kw)
                got = host_layer(img, exposure, **kw)
                assert got.dtype == want.dtype and np.isfinite(want).all() and (want >= 0).all()
                assert np.array_equal(got, want), (shape, content, exposure, int((got != want).sum()))
            assert np.array_equal(host_layer(img, 1.0, in_place=True, **kw), ref.layer(img, 1.0, **kw))
    # the options reach the arithmetic
    img = ref.image("midrange", (67, 37), dtype)
    assert not np.array_equal(ref.layer(img, 1.0, **kw), ref.layer(img, 1.0, threshold=0.75, knee=0.25))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("op", list(dref.OPS))
def test_host_build_composite_with_linear_transfer_is_bit_identical(op, dtype):
    for shape in HOST_SHAPES:
        for content in HOST_CONTENTS:
            img = ref.image(content, shape, dtype)
            for exposure, bloom in ((1.0, {}), (0.37, dict(threshold=0.5, knee=0.25, intensity=0.6, levels=3))):
                kw = dict(op=dref.OPS[op], transfer=dref.TRANSFER_LINEAR)
                want = ref.tone(img, exposure, **kw, **bloom)
                got = host_tonemap(img, exposure, format=D.TAKE_DISPLAY_REAL, **kw, **bloom)
                assert got.dtype == want.dtype and np.isfinite(want).all() and np.array_equal(got, want), (shape, content)
                assert np.array_equal(host_tonemap(img, exposure, format=D.TAKE_DISPLAY_REAL, in_place=True, **kw, **bloom), want)
                assert np.array_equal(host_tonemap(img, exposure, format=D.TAKE_DISPLAY_RGBA, **kw, **bloom), ref.rgba(img, exposure, **kw, **bloom))
    if op == "reinhard":
        img = ref.image("midrange", (67, 37), dtype)
        want = ref.tone(img, 1.0, op=dref.REINHARD, transfer=dref.TRANSFER_LINEAR, white=1.5)
        assert np.array_equal(host_tonemap(img, 1.0, dref.REINHARD, dref.TRANSFER_LINEAR, D.TAKE_DISPLAY_REAL, white=1.5), want)
        assert not np.array_equal(want, ref.tone(img, 1.0, op=dref.REINHARD, transfer=dref.TRANSFER_LINEAR))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("op", list(dref.OPS))
def test_host_build_srgb_within_the_bars(op, dtype):
    for content in ("midrange", "salted", "log-uniform"):
        img = ref.image(content, (67, 37), dtype)
        y, near = ref.restated_srgb(img, 1.0, op=dref.OPS[op])
        label = f"{content} {op} {np.dtype(dtype).name}"
        dref.check_srgb_real(host_tonemap(img, 1.0, dref.OPS[op], dref.SRGB, D.TAKE_DISPLAY_REAL), y, label)
        dref.check_srgb_codes(host_tonemap(img, 1.0, dref.OPS[op], dref.SRGB, D.TAKE_DISPLAY_RGBA), y, near, label)


SRGB_CONTENTS = ("midrange", "salted", "log-uniform")  # what tests/test_gpu_bloom.py compares with the sRGB transfer


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_the_gpu_tests_images_keep_the_code_comparison_honest(dtype):
    """what tests/test_gpu_bloom.py asserts before it looks at the device, on every image it uses with the sRGB
    transfer: the seeds were chosen here, without a GPU"""
    for shape in ref.SHAPES:
        for content in SRGB_CONTENTS:
            for op in dref.OPS.values():
                img = ref.image(content, shape, dtype)
                y, near = ref.restated_srgb(img, 1.0, op=op)
                if shape[0] * shape[1] <= 9000:  # and the text the device runs meets the bars on them (the largest: the test above)
                    label = f"{content} {shape} {op} {np.dtype(dtype).name}"
                    dref.check_srgb_real(host_tonemap(img, 1.0, op, dref.SRGB, D.TAKE_DISPLAY_REAL), y, label)
                    dref.check_srgb_codes(host_tonemap(img, 1.0, op, dref.SRGB, D.TAKE_DISPLAY_RGBA), y, near, label)


# ------------------------------------------------------------------ properties of the specification: on the restatement, and
# — so that they hold the library's text too — on the host build of tk_bloom.h
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_an_image_below_the_knee_has_no_layer_and_the_plain_tonemap_s_bytes(dtype):
    """everywhere below t - k after exposure: s clamps to 0 and Y - t < 0, so m = 0, w = 0, b = 0 exactly, and sums of
    zeros are zero; x + 0 = x, so the composite is display_ref's tonemap"""
    for shape in ((7, 3), (33, 17), (67, 37)):
        for img, exposure in ((ref.image("below", shape, dtype), 1.0), (dref.log_uniform(shape[0], shape[1], dtype, 5, -12.0, 3.0), 2.0 ** -5)):
            assert dref.luminance(ref.exposed(img, exposure)).max() < 0.5
            assert not ref.layer(img, exposure).any() and not host_layer(img, exposure).any()
            for op in dref.OPS.values():
                got = host_tonemap(img, exposure, op, dref.TRANSFER_LINEAR, D.TAKE_DISPLAY_RGBA)
                assert got.tobytes() == dref.rgba(img, exposure, op=op, transfer=dref.TRANSFER_LINEAR).tobytes()
                for transfer in (dref.SRGB, dref.TRANSFER_LINEAR):
                    assert ref.tone(img, exposure, op=op, transfer=transfer).tobytes() == dref.tone(img, exposure, op=op, transfer=transfer).tobytes()
                assert ref.rgba(img, exposure, op=op).tobytes() == dref.rgba(img, exposure, op=op).tobytes()
        above = ref.image("above", shape, dtype)
        assert (ref.layer(above, 1.0) > 0).all() and ref.tone(above, 1.0, transfer=dref.TRANSFER_LINEAR).tobytes() != dref.tone(above, 1.0, transfer=dref.TRANSFER_LINEAR).tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_intensity_zero_is_the_plain_tonemap(dtype):
    """gain = 0: the layer is 0 * finite = 0 and x + 0 = x — for every image, the salted one included"""
    for content in ("log-uniform", "salted", "midrange", "above", "border"):
        img = ref.image(content, (67, 37), dtype)
        assert not ref.layer(img, 1.0, intensity=0.0).any()
        for op in dref.OPS.values():
            for exposure in (1.0, 0.37):
                assert ref.tone(img, exposure, op=op, intensity=0.0).tobytes() == dref.tone(img, exposure, op=op).tobytes()
                assert ref.rgba(img, exposure, op=op, intensity=0.0).tobytes() == dref.rgba(img, exposure, op=op).tobytes()
                got = host_tonemap(img, exposure, op, dref.TRANSFER_LINEAR, D.TAKE_DISPLAY_RGBA, intensity=0.0)
                assert got.tobytes() == dref.rgba(img, exposure, op=op, transfer=dref.TRANSFER_LINEAR).tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_an_impulse_s_layer_is_non_negative_symmetric_and_sums_to_intensity_times_it(dtype):
    """Non-negative: every weight is positive and b >= 0.

    The sum.  One bright pixel b at (64, 64) of a black 129 x 129 image, 4 levels, threshold 0 (the bright pass is then
    the identity on the impulse: m = Y, w = Y / Y = 1).  A downsample's 6 x 6 footprint is nine B means (weights 4/32,
    4 x 2/32, 4 x 1/32: together 1/2) and four C means (4 x 1/8: together 1/2), each spread evenly over a 2 x 2 block
    that holds one pixel of every parity class (row even or odd, column even or odd); so each class carries (1/2 + 1/2)
    / 4 = 1/4 of the footprint.  A source pixel is read by the destinations whose footprints hold it at the taps of its
    own parity class, once each: away from the edges its weights sum to 1/4, and sum(D_k) = b / 4^(k+1).  An upsample's
    source pixel n is near for the destinations 2 n and 2 n + 1 (3/4 each) and far for 2 n - 1 and 2 n + 2 (1/4 each):
    2 per axis, 4 in all, so sum(up(S)) = 4 sum(S).  Then sum(U_k) = sum(D_k) + 4 sum(U_k+1) gives sum(U_0) = L b / 4,
    and sum(layer) = gain * 4 * sum(U_0) = (intensity / L) * L * b = intensity * b: dividing the gain by L is what keeps
    the layer's energy independent of the number of levels.  The impulse is 64 pixels from every edge; after 4 levels
    the layer's support is columns and rows 17 .. 110 (asserted: the outer 8 are zero), so no clamp takes part and only
    rounding separates the two sides: a value's path has about 75 operations (the bright pass 8, a downsample 8, an
    upsample and its add 8, per level), each within half an ulp, and all terms are non-negative, so the sum is within
    75 * 2^-24 = 4.5e-6 relative in f32 and 75 * 2^-53 = 8.4e-15 in f64.  Bars: 1e-5 and 1e-13.

    Symmetry.  The pyramid's grid puts pixel n of a level at 2 n + 0.5 of the level below, and every filter is symmetric
    about its own centre on that grid; tk_bloom.h pairs its additions so that mirror images and transpositions give
    the same bits.  A single pixel is not a centre of that grid (in one dimension the impulse at 64 gives 9/64 at 62
    and 7/64 at 66 after one level down and up), so "symmetric about the impulse" holds exactly where the impulse is
    symmetric about the grid: a 2 x 2 block at the centre of a 128 x 128 image, whose mirror images (and whose clamps'
    mirror images) are itself at every level.  Asserted bit for bit: that block's layer equals its two mirror images
    and its transpose; and for single pixels anywhere, rectangular images included, the layer of the transposed image is
    the transposed layer."""
    L, intensity, b = 4, 0.25, np.array([40.0, 30.0, 20.0])
    bloom = dict(threshold=0.0, knee=0.0, intensity=intensity, levels=L)
    img = ref.impulse(129, 129, dtype, (64, 64), value=tuple(b))
    lay = ref.layer(img, 1.0, **bloom)
    assert (lay >= 0).all() and lay[64, 64].min() > 0
    assert not lay[:8].any() and not lay[-8:].any() and not lay[:, :8].any() and not lay[:, -8:].any()
    total = lay.astype(np.float64).sum(axis=(0, 1))
    bar = 1e-5 if dtype == np.float32 else 1e-13
    print(f"sum of the layer {total}, intensity * b {intensity * b}")
    assert np.all(np.abs(total - intensity * b) <= bar * intensity * b)

    def transposed(a):
        return np.ascontiguousarray(a.transpose(1, 0, 2))

    assert np.array_equal(transposed(lay), ref.layer(transposed(img), 1.0, **bloom))
    off = ref.impulse(129, 97, dtype, (40, 70))  # off centre, rectangular, the defaults' knee
    assert np.array_equal(transposed(ref.layer(off, 1.0, levels=L)), ref.layer(transposed(off), 1.0, levels=L))
    sym = np.zeros((128, 128, 3), dtype)
    sym[63:65, 63:65] = b
    for kw in (dict(levels=L), {}):  # all 7 levels: the clamps at the edges mirror too
        lay = ref.layer(sym, 1.0, **kw)
        assert lay.max() > 0 and np.array_equal(lay, lay[::-1]) and np.array_equal(lay, lay[:, ::-1]) and np.array_equal(lay, lay.transpose(1, 0, 2))
        assert np.array_equal(host_layer(sym, 1.0, **kw), lay)  # the host build agrees


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_the_layer_is_monotone_in_intensity(dtype):
    """the layer is gain * up(U_0) with up(U_0) >= 0 independent of the intensity, and rounding a product is monotone"""
    for content in ("log-uniform", "salted", "above", "centre"):
        img = ref.image(content, (67, 37), dtype)
        intensities = (0.0, 0.05, 0.25, 0.26, 1.0, 4.0)
        layers = [ref.layer(img, 1.0, intensity=i) for i in intensities]
        hosts = [host_layer(img, 1.0, intensity=i) for i in intensities]
        assert layers[-1].max() > 0
        for lo, hi in zip(layers, layers[1:]):
            assert (lo <= hi).all()
        for lo, hi in zip(hosts, hosts[1:]):
            assert (lo <= hi).all()
        tones = [ref.tone(img, 1.0, op=dref.REINHARD, transfer=dref.TRANSFER_LINEAR, intensity=i) for i in (0.0, 0.25, 1.0)]
        for lo, hi in zip(tones, tones[1:]):
            assert (lo <= hi + 4 * np.finfo(dtype).eps).all()

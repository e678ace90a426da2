"""CPU side of the display transform (take_hip_luminance_histogram*, take_hip_auto_exposure, take_hip_tonemap*:
include/take_hip.h): the symbols are declared, exported and bound, the two structs have the header's
layout, every refusal is TAKE_E_INVALID with its message before a device is looked for; take_hip_auto_exposure — host
arithmetic, it runs here — against the numpy restatement (tests/display_ref.py); the text the device runs
(take_amd/csrc/tk_display.h) built for the host (tests/display_host) against the restatement; the PNG writer; and the
properties of the specification, on the restatement alone.

Bars.  Auto-exposure: 1e-12 relative — the same operations in the same order in double, only libm's log2 / exp2 against
numpy's may differ by an ulp.  Luminance bins: equal.  LINEAR transfer: REAL outputs and RGBA codes bit-identical in f32
and in f64.  SRGB: A = 16 ulp of 1.0 (display_ref.allowance) on REAL outputs; RGBA codes differ by at most 1, only where
the restatement's unrounded value lies within 255 A of an integer, in at most 0.5 % of the channels — after the
restatement alone has shown that at most 0.5 % of its channels lie that close."""
import ctypes as C
import os
import re
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import display_ref as ref
from helpers import HERE
from take_amd import capi, png
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_luminance_histogram", "take_hip_luminance_histogram_device", "take_hip_auto_exposure", "take_hip_tonemap", "take_hip_tonemap_device")
EXPOSURE_FIELDS = ["key", "low_fraction", "high_fraction", "min_exposure", "max_exposure", "prev_exposure", "rate"]
TONEMAP_FIELDS = ["exposure", "white", "op", "transfer", "format", "reserved", "auto_opts"]
F32, F64 = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ------------------------------------------------------------------ the boundary
def test_the_five_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.DISPLAY_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.DISPLAY_PROTOTYPES[name], name
        declared = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(declared.split(",")) == len(D.DISPLAY_PROTOTYPES[name]), name
    assert [len(D.DISPLAY_PROTOTYPES[n]) for n in SYMBOLS] == [5, 6, 3, 7, 8]
    for f in (capi.luminance_histogram, capi.luminance_histogram_device, capi.auto_exposure, capi.tonemap, capi.tonemap_device, png.write_png, png.read_png):
        assert callable(f)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_the_structs_have_the_header_s_layout():
    assert [n for n, _ in D.TakeExposureOpts._fields_] == EXPOSURE_FIELDS
    assert [n for n, _ in D.TakeTonemapOpts._fields_] == TONEMAP_FIELDS
    consts = ["TAKE_LUMINANCE_BINS", "TAKE_LUMINANCE_SLOTS", "TAKE_TONEMAP_LINEAR", "TAKE_TONEMAP_REINHARD", "TAKE_TONEMAP_ACES", "TAKE_TRANSFER_SRGB",
              "TAKE_TRANSFER_LINEAR", "TAKE_DISPLAY_RGBA", "TAKE_DISPLAY_REAL"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){",
            'printf("TakeExposureOpts %zu\\n", sizeof(TakeExposureOpts));', 'printf("TakeTonemapOpts %zu\\n", sizeof(TakeTonemapOpts));']
    prog += [f'printf("{c} %d\\n", {c});' for c in consts]
    prog += [f'printf("e.{n} %zu\\n", offsetof(TakeExposureOpts, {n}));' for n in EXPOSURE_FIELDS]
    prog += [f'printf("t.{n} %zu\\n", offsetof(TakeTonemapOpts, {n}));' for n in TONEMAP_FIELDS]
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(c, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        want = dict(line.split() for line in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines())
    assert C.sizeof(D.TakeExposureOpts) == int(want["TakeExposureOpts"]) == 56
    assert C.sizeof(D.TakeTonemapOpts) == int(want["TakeTonemapOpts"]) == 88
    for c in consts:
        assert getattr(D, c) == int(want[c]), c
    for n in EXPOSURE_FIELDS:
        assert getattr(D.TakeExposureOpts, n).offset == int(want["e." + n]), n
    for n in TONEMAP_FIELDS:
        assert getattr(D.TakeTonemapOpts, n).offset == int(want["t." + n]), n
    assert (ref.BINS, ref.SLOTS, ref.NONPOSITIVE, ref.NONFINITE) == (D.TAKE_LUMINANCE_BINS, D.TAKE_LUMINANCE_SLOTS, 384, 385)
    assert ref.OPS == D.TONEMAP_OPS and (ref.SRGB, ref.TRANSFER_LINEAR) == (D.TAKE_TRANSFER_SRGB, D.TAKE_TRANSFER_LINEAR)


def test_the_defaults_are_the_same_in_every_place():
    hdr = open(os.path.join(ROOT, "include", "take_hip.h")).read()
    assert set(D.DISPLAY_DEFAULTS) == set(ref.DEFAULTS) == {"key", "low_fraction", "high_fraction", "min_exposure", "max_exposure", "rate", "white"}
    for field in D.DISPLAY_DEFAULTS:
        line = next(l for l in hdr.splitlines() if re.search(r"^\s+double " + field + r";", l))
        text = re.search(r"<=? 0: ([0-9.^-]+)", line).group(1)
        value = 2.0 ** int(text[2:]) if text.startswith("2^") else float(text)
        assert value == D.DISPLAY_DEFAULTS[field] == ref.DEFAULTS[field], (field, line)
    line = next(l for l in hdr.splitlines() if re.search(r"^\s+double prev_exposure;", l))
    assert "<= 0: none" in line


def bad_exposure_opts():
    """(TakeExposureOpts, the message's part) for everything take_hip_auto_exposure refuses of its options"""
    out = []
    for field in EXPOSURE_FIELDS:
        for v in (float("nan"), float("inf"), -float("inf")):
            o = D.exposure_opts()
            setattr(o, field, v)
            out.append((o, b"must be finite"))
    out += [(D.exposure_opts(low_fraction=0.5, high_fraction=0.5), b"low_fraction"), (D.exposure_opts(low_fraction=0.96), b"low_fraction"),
            (D.exposure_opts(low_fraction=0.3, high_fraction=0.2), b"low_fraction"), (D.exposure_opts(high_fraction=1.5), b"high_fraction"),
            (D.exposure_opts(high_fraction=0.04), b"low_fraction"), (D.exposure_opts(rate=1.25), b"rate"),
            (D.exposure_opts(min_exposure=2.0, max_exposure=1.0), b"min_exposure"), (D.exposure_opts(min_exposure=1e6), b"min_exposure"),
            (D.exposure_opts(max_exposure=1e-6), b"min_exposure")]
    assert len(out) == 21 + 9
    return out


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU.  (The planes below are not device
    memory: a call that went past the argument check would not survive it.)"""
    buf = C.cast(C.create_string_buffer(256), C.c_void_p)
    other = C.cast(C.create_string_buffer(256), C.c_void_p)
    hist = (C.c_int64 * D.TAKE_LUMINANCE_SLOTS)()
    E = C.c_double(0.0)

    def hd(rgb=buf, precision=F32, w=2, h=2, out=hist):
        return lib.take_hip_luminance_histogram_device(rgb, precision, w, h, out, None)

    def hh(rgb=buf, precision=F32, w=2, h=2, out=hist):
        return lib.take_hip_luminance_histogram(rgb, precision, w, h, out)

    def ae(h=hist, opts=None, out=E):
        return lib.take_hip_auto_exposure(h, None if opts is None else C.byref(opts), None if out is None else C.byref(out))

    def td(rgb=buf, precision=F32, w=2, h=2, opts=None, out=other):
        return lib.take_hip_tonemap_device(rgb, precision, w, h, None if opts is None else C.byref(opts), out, None, None)

    def th(rgb=buf, precision=F32, w=2, h=2, opts=None, out=other):
        return lib.take_hip_tonemap(rgb, precision, w, h, None if opts is None else C.byref(opts), out, C.byref(E))

    def topts(**kw):
        o = D.tonemap_opts(exposure=1.0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    cases = []
    for f in (hd, hh, td, th):
        cases += [(lambda f=f: f(rgb=None), b"null argument"), (lambda f=f: f(out=None), b"null argument"),
                  (lambda f=f: f(w=0), b"width and height"), (lambda f=f: f(h=-3), b"width and height"),
                  (lambda f=f: f(precision=D.TAKE_PRECISION_MIXED), b"unknown precision"), (lambda f=f: f(precision=-1), b"unknown precision")]
    cases += [(lambda: ae(h=None), b"null argument"), (lambda: ae(out=None), b"null argument")]
    for slot in (0, 200, 383, 384, 385):
        neg = (C.c_int64 * D.TAKE_LUMINANCE_SLOTS)()
        neg[5] = 7
        neg[slot] = -1
        cases.append((lambda neg=neg: ae(h=neg), b"negative histogram count"))
    cases += [(lambda o=o: ae(opts=o), msg) for o, msg in bad_exposure_opts()]
    bad_tonemap = [(topts(op=3), b"unknown tone operator"), (topts(op=-1), b"unknown tone operator"), (topts(transfer=2), b"unknown transfer"),
                   (topts(transfer=-1), b"unknown transfer"), (topts(format=2), b"unknown output format"), (topts(format=-1), b"unknown output format"),
                   (topts(reserved=1), b"reserved")]
    for field in ("exposure", "white"):
        bad_tonemap += [(topts(**{field: v}), b"must be finite") for v in (float("nan"), float("inf"), -float("inf"))]
    for o, msg in bad_exposure_opts():  # with an explicit exposure and with an automatic one
        bad_tonemap += [(topts(auto_opts=o), msg), (topts(exposure=0.0, auto_opts=o), msg)]
    for f in (td, th):
        cases += [(lambda f=f, o=o: f(opts=o), msg) for o, msg in bad_tonemap]
        # RGBA output on the input, and overlapping it from either side (2 x 2 pixels: 48 bytes of floats, 16 of codes)
        cases += [(lambda f=f: f(out=buf), b"overlap"), (lambda f=f: f(opts=topts(), out=C.c_void_p(buf.value + 44)), b"overlap"),
                  (lambda f=f: f(rgb=C.c_void_p(buf.value + 12), out=buf), b"overlap")]
    cases += [(lambda: td(out=C.c_void_p(other.value + 2)), b"4-byte aligned")]
    assert len(cases) == 4 * 6 + 2 + 5 + 30 + 2 * (7 + 6 + 60 + 3) + 1
    for call, msg in cases:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert b"null scene" in lib.take_hip_last_error()
        assert call() == D.TAKE_E_INVALID
        assert msg in lib.take_hip_last_error(), (msg, lib.take_hip_last_error())


def test_the_python_binding_checks_its_arguments():
    img = np.zeros((4, 5, 3), np.float32)
    for bad in (np.zeros((4, 5, 3), np.int32), np.zeros((4, 5), np.float32), np.zeros((4, 5, 4), np.float32)):
        with pytest.raises(ValueError):
            capi.luminance_histogram(bad)
        with pytest.raises(ValueError):
            capi.tonemap(bad)
    for kw in (dict(op="filmic"), dict(transfer="gamma"), dict(format="rgb"), dict(opts=D.tonemap_opts(), exposure=1.0), dict(opts=D.tonemap_opts(), white=2.0)):
        with pytest.raises(ValueError):
            capi.tonemap(img, **kw)
    for bad in (np.zeros(386, np.int32), np.zeros(384, np.int64)):
        with pytest.raises(ValueError):
            capi.auto_exposure(bad)
    with pytest.raises(ValueError):
        capi.auto_exposure(np.zeros(386, np.int64), opts=D.exposure_opts(), key=0.2)
    with pytest.raises(ValueError):
        capi.tonemap_device(1 << 20, 2, 2, F32)  # RGBA without an output plane


# ------------------------------------------------------------------ take_hip_auto_exposure against the restatement
def hist_of(counts):
    h = np.zeros(ref.SLOTS, np.int64)
    for b, c in counts.items():
        h[b] = c
    return h


def random_hist(seed, scale=1000):
    rng = np.random.default_rng(seed)
    h = np.zeros(ref.SLOTS, np.int64)
    lo = int(rng.integers(120, 200))  # (the target stays inside the default clamps)
    h[lo:lo + 80] = rng.integers(0, scale, 80)
    h[ref.NONPOSITIVE], h[ref.NONFINITE] = 12345, 678  # (left out of N)
    return h


HISTOGRAMS = {
    "empty": hist_of({}),
    "only the extra slots": hist_of({ref.NONPOSITIVE: 100, ref.NONFINITE: 5}),
    "one bin": hist_of({200: 4096}),
    "one pixel": hist_of({17: 1}),
    "the two end bins": hist_of({0: 500, 383: 700}),
    "two bins, cut inside both": hist_of({150: 10, 190: 10}),
    "three bins, cuts inside the outer two": hist_of({100: 7, 101: 50, 102: 9}),
    "near 2^40": hist_of({180: (1 << 40) - 3, 181: (1 << 40) + 11, 250: (1 << 39) + 1}),
    "random": random_hist(1),
    "random, large": random_hist(2, 1 << 36),
}
OPTIONS = [{}, dict(low_fraction=0.0, high_fraction=1.0), dict(low_fraction=0.25, high_fraction=0.5), dict(low_fraction=0.49, high_fraction=0.51),
           dict(key=0.36), dict(low_fraction=0.999, high_fraction=0.9995)]


def check_exposure(got, want, label):
    print(f"{label}: {got!r} against {want!r}")
    assert got > 0 and abs(got - want) <= 1e-12 * want, (label, got, want)


@pytest.mark.parametrize("name", list(HISTOGRAMS))
def test_auto_exposure_against_the_restatement(lib, name):
    h = HISTOGRAMS[name]
    check_exposure(capi.auto_exposure(h), ref.auto_exposure(h), name + ", defaults (NULL)")
    for o in OPTIONS:
        check_exposure(capi.auto_exposure(h, **o), ref.auto_exposure(h, **o), f"{name}, {o}")


def test_auto_exposure_of_known_histograms(lib):
    """values that follow from the specification by hand, so that the restatement is held to something too"""
    assert capi.auto_exposure(HISTOGRAMS["empty"]) == ref.auto_exposure(HISTOGRAMS["empty"]) == 1.0
    assert capi.auto_exposure(HISTOGRAMS["only the extra slots"]) == 1.0
    # bin 200: e = 1, m = 0: 2^1 * (1 + 0.5 / 8) = 2.125
    check_exposure(capi.auto_exposure(HISTOGRAMS["one bin"]), 0.18 / 2.125, "one bin")
    # the end bins, nothing cut off: the count-weighted mean of their log2 values
    l0, l1 = -24 + np.log2(1.0625), 23 + np.log2(1.9375)
    check_exposure(capi.auto_exposure(HISTOGRAMS["the two end bins"], low_fraction=0.0, high_fraction=1.0, min_exposure=1e-30, max_exposure=1e30),
                   0.18 / 2.0 ** ((500 * l0 + 700 * l1) / 1200), "end bins")
    # 20 pixels, fractions 0.25 .. 0.5: pixels 5 .. 10, all inside the first bin
    check_exposure(capi.auto_exposure(HISTOGRAMS["two bins, cut inside both"], low_fraction=0.25, high_fraction=0.5),
                   0.18 / 2.0 ** ref.bin_log2(150), "cut inside one bin")


def test_auto_exposure_clamps(lib):
    dark, bright = hist_of({0: 10}), hist_of({383: 10})  # targets 0.18 * 2^24 / 1.0625 and 0.18 / (2^23 * 1.9375)
    assert capi.auto_exposure(dark) == ref.auto_exposure(dark) == 2.0 ** 16
    assert capi.auto_exposure(bright) == ref.auto_exposure(bright) == 2.0 ** -16
    assert capi.auto_exposure(dark, max_exposure=100.0) == 100.0 and capi.auto_exposure(bright, min_exposure=0.5) == 0.5
    assert capi.auto_exposure(HISTOGRAMS["one bin"], min_exposure=3.0, max_exposure=3.0) == 3.0
    # the clamp comes after the adaptation
    assert capi.auto_exposure(dark, prev_exposure=1.0, rate=0.5, max_exposure=8.0) == ref.auto_exposure(dark, prev_exposure=1.0, rate=0.5, max_exposure=8.0) == 8.0


@pytest.mark.parametrize("rate", [0.25, 1.0])
def test_auto_exposure_adapts(lib, rate):
    h = HISTOGRAMS["random"]
    target = ref.auto_exposure(h)
    for prev in (target / 37.0, target * 5.0, target, 1.0):
        got = capi.auto_exposure(h, prev_exposure=prev, rate=rate)
        check_exposure(got, ref.auto_exposure(h, prev_exposure=prev, rate=rate), f"rate {rate}, from {prev}")
        check_exposure(got, prev * (target / prev) ** rate, f"rate {rate}, from {prev}, by hand")
    check_exposure(capi.auto_exposure(h, prev_exposure=1.0, rate=1.0), target, "rate 1 jumps to the target")
    assert capi.auto_exposure(h, prev_exposure=0.0, rate=rate) == capi.auto_exposure(h, prev_exposure=-1.0, rate=rate) == capi.auto_exposure(h)


@pytest.mark.parametrize("start", [1e-3, 40.0])
def test_adaptation_converges_monotonically_to_the_target(lib, start):
    h = HISTOGRAMS["random"]
    target = capi.auto_exposure(h)
    e, gaps = start, []
    for _ in range(200):
        e = capi.auto_exposure(h, prev_exposure=e, rate=0.25)
        gaps.append(np.log2(e) - np.log2(target))
    gaps = np.array(gaps)
    print(f"from {start}: log2 distance to the target {gaps[0]:.3f} -> {gaps[-1]:.3e}")
    assert (np.sign(gaps[:60]) == np.sign(gaps[0])).all()  # from one side
    assert (np.abs(gaps[1:]) <= np.abs(gaps[:-1]) + 1e-14).all()  # never away from it
    assert (np.abs(gaps[1:60]) < np.abs(gaps[:59]) * 0.76).all()  # each step takes a quarter of the distance
    assert abs(gaps[-1]) <= 1e-13
    check_exposure(capi.auto_exposure(h, prev_exposure=target, rate=0.25), target, "the target is a fixed point")


# ------------------------------------------------------------------ host execution of tk_display.h
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "display_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libdisplay_host.so"))
        L.display_slots.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.display_luminance_slots.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.display_tonemap.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        _HOST = L
    return _HOST


def host_slots(rgb):
    rgb = np.ascontiguousarray(rgb)
    out = np.full(rgb.shape[:-1], -1, np.int32)
    assert host_lib().display_slots(int(rgb.dtype == np.float64), rgb.ctypes.data, out.size, out.ctypes.data) == 0
    return out


def host_luminance_slots(y):
    y = np.ascontiguousarray(y)
    out = np.full(y.shape, -1, np.int32)
    assert host_lib().display_luminance_slots(int(y.dtype == np.float64), y.ctypes.data, y.size, out.ctypes.data) == 0
    return out


def host_tonemap(rgb, exposure, op, transfer, format, white=ref.DEFAULTS["white"], in_place=False):
    rgb = np.ascontiguousarray(rgb).copy()
    if format == D.TAKE_DISPLAY_RGBA:
        out = np.zeros(rgb.shape[:2] + (4,), np.uint8)
    else:
        out = rgb if in_place else np.full_like(rgb, np.nan)
    assert host_lib().display_tonemap(int(rgb.dtype == np.float64), rgb.ctypes.data, rgb.shape[0] * rgb.shape[1], exposure, white, op, transfer, format,
                                      out.ctypes.data) == 0
    return out


def edge_luminances(dtype):
    """every bin's lower edge and its neighbours on both sides (in float, and in `dtype`), both zeros, negatives, the
    non-finite values, values below 2^-24 and above 2^24 and — in float64 — beyond float's range and at its roundings"""
    edges = (np.arange(ref.BINS + 1, dtype=np.uint32) + 8 * (127 - 24) << 20).astype(np.uint32).view(np.float32)
    assert edges[0] == 2.0 ** -24 and edges[-1] == 2.0 ** 24 and edges[8] == 2.0 ** -23
    vals = [edges, np.nextafter(edges, np.float32(0)), np.nextafter(edges, np.float32(np.inf))]
    vals = [v.astype(dtype) for v in vals]
    if dtype == np.float64:  # doubles that round to the edge from either side, and the first ones that do not
        e = edges.astype(np.float64)
        half_below = e - (e - np.nextafter(edges, np.float32(0)).astype(np.float64)) / 2  # the tie: to even, which is the edge
        vals += [np.nextafter(e, 0), np.nextafter(e, np.inf), half_below, np.nextafter(half_below, 0), np.nextafter(half_below, np.inf)]
    special = [0.0, -0.0, -1.0, -2.0 ** -30, -3e38, np.nan, np.inf, -np.inf, 2.0 ** -25, 2.0 ** -30, 2.0 ** -100, 1.2e-38, 2.0 ** 25, 2.0 ** 30, 3e38, 1.0, 0.18]
    if dtype == np.float64:
        special += [1e300, -1e300, 1e39, -1e39, 3.4028235677973366e38, 3.4028234e38, 1e-300, 2.0 ** -140, 2.0 ** -150, 5e-324]
    return np.concatenate(vals + [np.array(special, dtype)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_build_bins_luminances_as_the_restatement(dtype):
    y = edge_luminances(dtype)
    got, want = host_luminance_slots(y), ref.luminance_slots(y)
    assert np.array_equal(got, want), [(float(v), int(g), int(w)) for v, g, w in zip(y, got, want) if g != w][:8]
    # and the restatement is held to the specification's words: an edge opens its bin, the value below it closes the one before
    edges = y[:ref.BINS + 1].astype(np.float32)
    assert np.array_equal(want[:ref.BINS], np.arange(ref.BINS)) and want[ref.BINS] == ref.BINS - 1  # 2^24 lands in the end bin
    below = ref.luminance_slots(np.nextafter(edges, np.float32(0)).astype(dtype))
    assert np.array_equal(below[1:], np.arange(ref.BINS)) and below[0] == 0
    named = {0.0: ref.NONPOSITIVE, -0.0: ref.NONPOSITIVE, -1.0: ref.NONPOSITIVE, np.inf: ref.NONFINITE, -np.inf: ref.NONFINITE, np.nan: ref.NONFINITE,
             2.0 ** -30: 0, 2.0 ** 30: ref.BINS - 1, 1.0: 8 * 24, 1.5: 8 * 24 + 4}
    if dtype == np.float64:
        named.update({1e300: ref.NONFINITE, -1e300: ref.NONFINITE, 1e39: ref.NONFINITE, 1e-300: ref.NONPOSITIVE})
    for v, slot in named.items():
        assert ref.luminance_slots(np.array([v], dtype))[0] == host_luminance_slots(np.array([v], dtype))[0] == slot, v


IMAGES = {"log-uniform": lambda dt: ref.log_uniform(67, 13, dt, 11), "midrange": lambda dt: ref.midrange(67, 13, dt, 12),
          "salted": lambda dt: ref.salted(67, 13, dt, 13), "constant": lambda dt: ref.constant(7, 3, dt)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("content", list(IMAGES))
def test_host_build_bins_pixels_as_the_restatement(content, dtype):
    img = IMAGES[content](dtype)
    got = host_slots(img)
    assert np.array_equal(got, ref.slots(img))
    h = ref.histogram(img)
    assert h.sum() == img.shape[0] * img.shape[1] and np.array_equal(h, np.bincount(got.ravel(), minlength=ref.SLOTS))
    if content == "salted":
        assert h[ref.NONPOSITIVE] > 0 and h[ref.NONFINITE] > 0
    if content == "log-uniform":
        assert h[0] > 0 and h[ref.BINS - 1] > 0 and (h[:ref.BINS] > 0).sum() > 200  # the end bins and most between


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(ref.OPS))
@pytest.mark.parametrize("content", ["log-uniform", "midrange", "salted"])
def test_host_build_linear_transfer_is_bit_identical(content, op, dtype):
    img = IMAGES[content](dtype)
    for exposure in (1.0, 0.37):
        kw = dict(op=ref.OPS[op], transfer=ref.TRANSFER_LINEAR)
        want = ref.tone(img, exposure, **kw)
        got = host_tonemap(img, exposure, format=D.TAKE_DISPLAY_REAL, **kw)
        assert got.dtype == want.dtype and np.isfinite(want).all() and np.array_equal(got, want)
        assert np.array_equal(host_tonemap(img, exposure, format=D.TAKE_DISPLAY_REAL, in_place=True, **kw), want)
        assert np.array_equal(host_tonemap(img, exposure, format=D.TAKE_DISPLAY_RGBA, **kw), ref.rgba(img, exposure, **kw))
    if op == "reinhard":
        want = ref.tone(img, 1.0, op=ref.REINHARD, transfer=ref.TRANSFER_LINEAR, white=1.5)
        assert np.array_equal(host_tonemap(img, 1.0, ref.REINHARD, ref.TRANSFER_LINEAR, D.TAKE_DISPLAY_REAL, white=1.5), want)
        assert not np.array_equal(want, ref.tone(img, 1.0, op=ref.REINHARD, transfer=ref.TRANSFER_LINEAR))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", list(ref.OPS))
@pytest.mark.parametrize("content", ["midrange", "salted"])
def test_host_build_srgb_within_the_bars(content, op, dtype):
    img = IMAGES[content](dtype)
    y, near = ref.restated_srgb(img, 1.0, op=ref.OPS[op])
    label = f"{content} {op} {np.dtype(dtype).name}"
    ref.check_srgb_real(host_tonemap(img, 1.0, ref.OPS[op], ref.SRGB, D.TAKE_DISPLAY_REAL), y, label)
    ref.check_srgb_codes(host_tonemap(img, 1.0, ref.OPS[op], ref.SRGB, D.TAKE_DISPLAY_RGBA), y, near, label)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_gpu_tests_images_keep_the_code_comparison_honest(dtype):
    """what tests/test_gpu_display.py asserts before it looks at the device, on every image it uses: the seeds were chosen
    here, without a GPU"""
    for shape in ref.SHAPES:
        for content in ("midrange", "salted"):
            for op in ref.OPS.values():
                ref.restated_srgb(ref.image(content, shape, dtype), 1.0, op=op)


def test_the_srgb_bars_can_tell_a_wrong_exponent():
    """1 / 2.2 for 1 / 2.4 moves the output by four orders above the bar"""
    img = IMAGES["midrange"](np.float32)
    y = ref.tone(img, 1.0)
    t = ref.tone(img, 1.0, transfer=ref.TRANSFER_LINEAR)
    wrong = np.where(t <= np.float32(0.0031308), np.float32(12.92) * t, np.float32(1.055) * np.power(t, np.float32(1 / 2.2)) - np.float32(0.055))
    assert np.abs(wrong - y).max() > 1e4 * ref.allowance(np.float32)


# ------------------------------------------------------------------ PNG
def parse_png(data):
    """hand-written: -> (IHDR fields, [(kind, body)]), every CRC checked"""
    assert data[:8] == bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])
    chunks, pos = [], 8
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert len(body) == n and crc == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    assert chunks[0][0] == b"IHDR" and len(chunks[0][1]) == 13 and chunks[-1] == (b"IEND", b"")
    return struct.unpack(">IIBBBBB", chunks[0][1]), chunks


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", [(1, 1), (3, 2), (300, 5)])
def test_png_round_trip(tmp_path, size, channels):
    w, h = size
    a = np.random.default_rng(w * 10 + channels).integers(0, 256, (h, w, channels)).astype(np.uint8)
    a[0, 0, 0], a[-1, -1, -1] = 0, 255
    path = tmp_path / "t.png"
    png.write_png(path, a)
    back = png.read_png(path)
    assert back.dtype == np.uint8 and back.shape == a.shape and np.array_equal(back, a)
    ihdr, chunks = parse_png(path.read_bytes())
    assert ihdr == (w, h, 8, 2 if channels == 3 else 6, 0, 0, 0)  # 8-bit truecolour (with alpha), deflate, filter method 0, no interlace
    assert [k for k, _ in chunks].count(b"IDAT") >= 1 and {k for k, _ in chunks} == {b"IHDR", b"IDAT", b"IEND"}
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))
    assert len(raw) == h * (1 + w * channels)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * channels)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(h, w, channels), a)  # filter type 0 on every scanline


def test_png_refuses_what_it_does_not_handle(tmp_path):
    for bad in (np.zeros((2, 2, 3), np.float32), np.zeros((2, 2), np.uint8), np.zeros((2, 2, 2), np.uint8), np.zeros((0, 2, 3), np.uint8)):
        with pytest.raises(ValueError):
            png.write_png(tmp_path / "bad.png", bad)
    path = tmp_path / "t.png"
    png.write_png(path, np.full((2, 3, 3), 9, np.uint8))
    data = bytearray(path.read_bytes())
    (tmp_path / "sig.png").write_bytes(b"JUNK" + bytes(data[4:]))
    data[-20] ^= 1  # inside IDAT: its CRC no longer holds
    (tmp_path / "crc.png").write_bytes(bytes(data))
    for name in ("sig.png", "crc.png"):
        with pytest.raises(ValueError):
            png.read_png(tmp_path / name)


# ------------------------------------------------------------------ properties of the specification (the restatement alone)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transfer", [ref.SRGB, ref.TRANSFER_LINEAR])
@pytest.mark.parametrize("op", list(ref.OPS))
def test_operators_are_monotone_map_zero_to_zero_and_stay_in_range(op, transfer, dtype):
    rng = np.random.default_rng(5)
    x = np.sort(np.concatenate([np.exp2(rng.uniform(-30, 17, 20000)), np.linspace(0, 4, 20001), [65504.0, 1e6, 3e38]])).astype(dtype)
    for exposure in (1.0, 0.37, 23.0):
        y = ref.tone(x, exposure, op=ref.OPS[op], transfer=transfer)
        assert y[0] == 0 and ref.tone(np.zeros(1, dtype), exposure, op=ref.OPS[op], transfer=transfer)[0] == 0
        assert y.min() >= 0 and y.max() <= 1 and np.isfinite(y).all()
        c = ref.codes(y).astype(np.int32)
        assert c[0] == 0 and c[-1] == 255 and (np.diff(c) >= 0).all()
        # the values themselves: monotone up to the rounding of the operator's quotient (a few ulp of the value)
        d = np.diff(y.astype(np.float64))
        assert (d >= -4 * np.finfo(dtype).eps * y[1:]).all(), float((d / np.maximum(y[1:], 1e-300)).min())
    for bad in (np.nan, -1.0, -np.inf):
        assert ref.tone(np.array([bad], dtype), 1.0, op=ref.OPS[op], transfer=transfer)[0] == 0
    top = ref.tone(np.array([np.inf], dtype), 1.0, op=ref.OPS[op], transfer=transfer)  # (1.055 - 0.055 need not round to 1)
    assert ref.codes(top)[0] == 255 and 1 - 2 * np.finfo(dtype).eps <= top[0] <= 1

"""CPU side of adaptive sampling (take_hip_render_adaptive and its _device twin: include/take_hip.h): the symbols are
declared, exported and bound, the two structs have the header's layout, every refusal is TAKE_E_INVALID with its
message before a device is looked for; and the text the device runs (take_amd/csrc/tk_adaptive.h) built for the host
(tests/adaptive_host) against the numpy restatement (tests/adaptive_ref.py): the stopping rule bit for bit — everything
is double, and / and sqrt are correctly rounded on both sides —, the moments, the ordered compaction and the work-list
index arithmetic exactly."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import adaptive_ref
from helpers import HERE
from take_amd import capi
from take_amd import cdefs as D

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_render_adaptive_device", "take_hip_render_adaptive")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ------------------------------------------------------------------ the boundary
def test_the_two_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.ADAPTIVE_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.ADAPTIVE_PROTOTYPES[name], name
    assert [len(D.ADAPTIVE_PROTOTYPES[n]) for n in SYMBOLS] == [6, 5]
    for f in (capi.Scene.render_adaptive, capi.Scene.render_adaptive_device):
        assert callable(f)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_the_structs_have_the_header_s_layout():
    fields = {"TakeAdaptiveOpts": [n for n, _ in D.TakeAdaptiveOpts._fields_], "TakeAdaptiveStats": [n for n, _ in D.TakeAdaptiveStats._fields_]}
    assert fields == {"TakeAdaptiveOpts": ["min_spp", "step_spp", "threshold", "floor", "flags", "reserved"], "TakeAdaptiveStats": ["count", "m1", "m2"]}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "take_hip.h"', "int main(void){"]
    for s, names in fields.items():
        prog.append(f'printf("{s} %zu\\n", sizeof({s}));')
        prog += [f'printf("{s}.{n} %zu\\n", offsetof({s}, {n}));' for n in names]
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(c, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        want = dict(line.split() for line in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.strip().splitlines())
    assert C.sizeof(D.TakeAdaptiveOpts) == int(want["TakeAdaptiveOpts"]) == 32
    assert C.sizeof(D.TakeAdaptiveStats) == int(want["TakeAdaptiveStats"]) == 24
    for s, names in fields.items():
        for n in names:
            assert getattr(getattr(D, s), n).offset == int(want[f"{s}.{n}"]), (s, n)


def test_the_defaults_are_the_same_in_every_place():
    hdr = open(os.path.join(ROOT, "include", "take_hip.h")).read()
    for field, text in (("min_spp", "<= 0: 16;"), ("step_spp", "<= 0: 8 */"), ("threshold", "< 0: 0.05;"), ("floor", "<= 0: 1e-3 */")):
        line = next(l for l in hdr.splitlines() if re.search(r"^\s+(int32_t|double) " + field + r";", l))
        assert text in line, line
        assert float(re.split(r"[;*]", text.split(":")[1])[0]) == D.ADAPTIVE_DEFAULTS[field] == adaptive_ref.DEFAULTS[field], field
    assert adaptive_ref.resolve(64) == adaptive_ref.DEFAULTS
    assert adaptive_ref.resolve(5)["min_spp"] == 5 and adaptive_ref.resolve(64, threshold=0.0)["threshold"] == 0.0


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU.  (`scene` and the planes below are
    not a scene and not device memory: a call that went past the argument check would not survive it.)"""
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    ro = D.TakeRenderOpts()
    ro.spp = 4

    def dev(sc=scene, o=ro, a=None, out=buf):
        return lib.take_hip_render_adaptive_device(sc, None if o is None else C.byref(o), None if a is None else C.byref(a), out, None, None)

    def host(sc=scene, o=ro, a=None, out=buf):
        return lib.take_hip_render_adaptive(sc, None if o is None else C.byref(o), None if a is None else C.byref(a), out, None)

    bad = [(D.TakeAdaptiveOpts(0, 0, -1.0, 0.0, 1, 0), b"unknown flag"), (D.TakeAdaptiveOpts(0, 0, -1.0, 0.0, -1, 0), b"unknown flag")]
    for field in ("threshold", "floor"):
        for v in (float("nan"), float("inf"), -float("inf")):
            a = D.adaptive_opts()
            setattr(a, field, v)
            bad.append((a, b"must be finite"))
    cases = []
    for f in (dev, host):
        cases += [(lambda f=f: f(sc=None), b"null argument"), (lambda f=f: f(o=None), b"null argument"), (lambda f=f: f(out=None), b"null argument")]
        cases += [(lambda f=f, a=a: f(a=a), msg) for a, msg in bad]
    assert len(cases) == 2 * (3 + 8)
    for call, msg in cases:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert b"null scene" in lib.take_hip_last_error()
        assert call() == D.TAKE_E_INVALID
        assert msg in lib.take_hip_last_error(), (msg, lib.take_hip_last_error())


# ------------------------------------------------------------------ host execution of tk_adaptive.h
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "adaptive_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libadaptive_host.so"))
        L.adaptive_host_test.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        L.adaptive_host_test.restype = None
        L.adaptive_host_moments.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
        L.adaptive_host_moments.restype = None
        L.adaptive_host_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.adaptive_host_compact.restype = C.c_int32
        L.adaptive_host_worklist.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.adaptive_host_worklist.restype = None
        _HOST = L
    return _HOST


def host_test(n, m1, m2, spp, threshold, floor):
    n, m1, m2 = np.ascontiguousarray(n, np.int32), np.ascontiguousarray(m1, np.float64), np.ascontiguousarray(m2, np.float64)
    err, stop = np.full(n.size, -7.0), np.full(n.size, -7, np.int32)
    host_lib().adaptive_host_test(n.size, n.ctypes.data, m1.ctypes.data, m2.ctypes.data, spp, threshold, floor, err.ctypes.data, stop.ctypes.data)
    return err, stop


def same_bits(a, b):
    """equal bit for bit; a NaN matches any NaN (its payload is not the rule's)"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def rule_inputs():
    """(n, m1, m2): moments of random samples at random counts, then the edge cases by hand"""
    rng = np.random.default_rng(11)
    spp = 13
    n = rng.integers(1, spp + 1, 4000).astype(np.int32)
    scale = 10.0 ** rng.uniform(-6, 3, n.size)
    spread = 10.0 ** rng.uniform(-9, 0, n.size)
    m1, m2 = np.zeros(n.size), np.zeros(n.size)
    for s in range(spp):
        v = np.where(s < n, scale * (1.0 + spread * rng.standard_normal(n.size)), 0.0)
        m1, m2 = m1 + v, m2 + v * v
    extra = [(1, 0.5, 0.25), (1, 0.0, 0.0), (1, 2.0, 5.0),                       # n == 1: a division by zero, never a stop on err
             (4, 4.0, 4.0 - 1e-15), (4, 0.4, 0.04 - 1e-18), (7, 7e8, 7e16 * (1 - 2e-16)),  # v slightly negative -> 0
             (4, 0.0, 0.0), (13, 13.0, 13.0), (13, 1.0, 50.0), (13, float("nan"), 1.0),     # zero variance; n == spp
             (5, float("nan"), 1.0), (5, 1.0, float("nan")), (5, float("inf"), 1.0), (5, 1.0, float("inf")), (5, float("inf"), float("inf")),
             (5, -float("inf"), float("inf")), (6, -3.0, 1.6), (2, 1.0, 1.0)]
    e = np.array(extra, np.float64)
    return spp, np.concatenate([n, e[:, 0].astype(np.int32)]), np.concatenate([m1, e[:, 1]]), np.concatenate([m2, e[:, 2]])


@pytest.mark.parametrize("threshold, floor", [(0.05, 1e-3), (0.0, 1e-3), (0.3, 0.5), (1e-4, 1e-9), (1e30, 1e-3)])
def test_the_stopping_rule_against_the_restatement_bit_for_bit(threshold, floor):
    spp, n, m1, m2 = rule_inputs()
    err, stop = host_test(n, m1, m2, spp, threshold, floor)
    ref = adaptive_ref.rel_error(n, m1, m2, floor)
    assert same_bits(err, ref)
    want = adaptive_ref.stops(n, ref, spp, threshold)
    assert np.array_equal(stop, want.astype(np.int32))
    assert not want[n == 1].any() and want[n == spp].all()
    assert not want[np.isnan(ref) & (n < spp)].any()  # a NaN err runs to spp
    print(f"threshold {threshold}: {int(want.sum())} of {n.size} stop; NaN errs {int(np.isnan(ref).sum())}, inf errs {int(np.isinf(ref).sum())}")
    if threshold in (0.05, 0.3):
        assert 0.05 < want[:4000].mean() < 0.95  # the random part decides both ways


def test_a_tie_stops():
    """err == threshold exactly: the threshold is the err the rule computes, and one ulp below it the pixel goes on"""
    spp, n, m1, m2 = rule_inputs()
    n, m1, m2 = n[:200], m1[:200], m2[:200]
    err = adaptive_ref.rel_error(n, m1, m2, 1e-3)
    pick = np.flatnonzero((n >= 2) & (n < spp) & np.isfinite(err) & (err > 0))
    assert pick.size > 50
    for i in pick[:40]:
        t = float(err[i])
        for thr, want in ((t, 1), (float(np.nextafter(t, 0.0)), 0), (float(np.nextafter(t, 1.0)), 1)):
            got_err, got = host_test(n[i:i + 1], m1[i:i + 1], m2[i:i + 1], spp, thr, 1e-3)
            assert same_bits(got_err, err[i:i + 1]) and got[0] == want == int(adaptive_ref.stops(n[i], err[i], spp, thr))


def test_the_moments_against_the_restatement():
    rng = np.random.default_rng(5)
    rgb32 = (rng.random((23, 3)) * 10.0 ** rng.uniform(-3, 2, (23, 1))).astype(np.float32)
    for rgb in (rgb32.astype(np.float64), rng.random((23, 3))):
        m = np.zeros(2)
        host_lib().adaptive_host_moments(rgb.shape[0], np.ascontiguousarray(rgb).ctypes.data, m.ctypes.data)
        assert same_bits(m, adaptive_ref.moments(adaptive_ref.sample_value(rgb)))
    v = adaptive_ref.sample_value(rgb32)  # the float image's channels are widened before they are added
    assert same_bits(v, (rgb32[:, 0].astype(np.float64) + rgb32[:, 1].astype(np.float64)) + rgb32[:, 2].astype(np.float64))


SIZES = (1, 63, 64, 65, 257, 1025, 64 * 1024 + 1)  # 1025, 65537: one above a multiple of the block / of the scan's 1024 runs


def flag_patterns(n):
    rng = np.random.default_rng(n)
    return {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8),
            "alternating-from-0": ((np.arange(n) + 1) % 2).astype(np.uint8), "random": (rng.random(n) < 0.3).astype(np.uint8)}


def host_compact(keep, pixels, threads):
    n = keep.size
    groups = (n + 63) // 64
    mask, base, out = np.zeros(groups, np.uint64), np.full(groups, -1, np.int32), np.full(n, -1, np.int32)
    total = host_lib().adaptive_host_compact(keep.ctypes.data, None if pixels is None else pixels.ctypes.data, n, threads, mask.ctypes.data,
                                             base.ctypes.data, out.ctypes.data)
    assert (out[total:] == -1).all()  # nothing written past the end
    return out[:total]


@pytest.mark.parametrize("n", SIZES)
def test_the_compaction_is_ascending_and_exact(n):
    rng = np.random.default_rng(100 + n)
    sparse = np.sort(rng.choice(4 * n + 7, n, replace=False)).astype(np.int32)  # an ascending list with gaps, as a later pass meets it
    for name, keep in flag_patterns(n).items():
        for pixels in (None, sparse):
            for threads in (1024, 1, 3):  # the kernel's block, and partitions that leave runs of every length
                got = host_compact(keep, pixels, threads)
                want = adaptive_ref.compact(keep, pixels)
                assert np.array_equal(got, want), (n, name, threads)
                assert (np.diff(got) > 0).all()


@pytest.mark.parametrize("n_active", SIZES[:6])
def test_the_work_list_produces_every_slot_once(n_active):
    rng = np.random.default_rng(200 + n_active)
    npix = 3 * n_active + 5
    pixels = np.sort(rng.choice(npix, n_active, replace=False)).astype(np.int32)
    for nb in (1, 3, 8):
        slot = np.full(nb * n_active, -1, np.int64)
        host_lib().adaptive_host_worklist(pixels.ctypes.data, n_active, nb, npix, slot.ctypes.data)
        assert np.array_equal(slot, adaptive_ref.worklist(pixels, nb, npix))
        assert np.unique(slot).size == slot.size and slot.max() < nb * npix
        assert np.array_equal(slot % npix, np.tile(pixels, nb)) and np.array_equal(slot // npix, np.repeat(np.arange(nb), n_active))


def test_the_work_list_at_full_size():
    """the reciprocal-divisor division with a divisor of the flagship image's size (one pixel stopped)"""
    npix = 1920 * 1080
    pixels = np.arange(1, npix, dtype=np.int32)
    slot = np.zeros(2 * pixels.size, np.int64)
    host_lib().adaptive_host_worklist(pixels.ctypes.data, pixels.size, 2, npix, slot.ctypes.data)
    assert np.array_equal(slot, adaptive_ref.worklist(pixels, 2, npix))


def test_the_schedule():
    assert adaptive_ref.schedule(13, 4, 3) == [4, 7, 10, 13]
    assert adaptive_ref.schedule(16, 16, 8) == [16] and adaptive_ref.schedule(12, 4, 5) == [4, 9, 12]

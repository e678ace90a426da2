"""CPU side of the variance-guided denoiser (take_hip_denoise_variance, take_hip_render_adaptive_denoised and their
_device twins: include/take_hip.h): the symbols are declared, exported and bound, the new default of sigma_color is the
same in every place, every refusal is TAKE_E_INVALID with its message before a device is looked for; the text the device
runs (take_amd/csrc/tk_denoise_var.h) built for the host (tests/denoise_var_host) against the numpy restatement
(tests/denoise_var_ref.py); and the properties of the specification (DESIGN.md par. 4h), on the restatement alone.

Bars, those of tests/test_denoise_cpu.py.  Host build against the restatement in f64: 1e-12 * max(1, max|ref|) on every
value of the image — the same operations in the same order, only the C library's exp against numpy's may differ by an
ulp.  In f32: 1e-5 * max(1, max|ref|) against the f64 restatement of the float-rounded inputs, the numpy f32 restatement
held to the same bar (it is 1.3e-6 from it at 130 x 70).  variance_out: the same two bars relative to max|V_ref|, not to
max(1, .), because V is small."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref
import denoise_var_ref as V
from helpers import HERE, rmse
from take_amd import capi
from take_amd import cdefs as D
from test_denoise_cpu import CASES, GUIDES, case_id

ROOT = os.path.dirname(HERE)
SYMBOLS = ("take_hip_denoise_variance", "take_hip_denoise_variance_device", "take_hip_render_adaptive_denoised", "take_hip_render_adaptive_denoised_device")
STATS = ("count", "m1", "m2")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ------------------------------------------------------------------ the boundary
def test_the_four_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "take_hip.h")).read(), flags=re.S)
    assert set(D.DENOISE_VARIANCE_PROTOTYPES) == set(SYMBOLS)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == D.DENOISE_VARIANCE_PROTOTYPES[name], name
    assert [len(D.DENOISE_VARIANCE_PROTOTYPES[n]) for n in SYMBOLS] == [9, 10, 7, 8]
    for f in (capi.denoise_variance, capi.denoise_variance_device, capi.Scene.render_adaptive_denoised, capi.Scene.render_adaptive_denoised_device):
        assert callable(f)
    assert lib.take_hip_abi_version() == 5  # new symbols are no new ABI version


def test_the_new_default_is_the_same_in_every_place():
    hdr = open(os.path.join(ROOT, "include", "take_hip.h")).read()
    assert "sigma_color <= 0 means 4.0 in these calls" in hdr
    assert D.DENOISE_VARIANCE_DEFAULTS == {k: v for k, v in V.DEFAULTS.items() if k != "keep_albedo"}
    assert V.DEFAULTS["sigma_color"] == 4.0
    assert {k: v for k, v in V.DEFAULTS.items() if k != "sigma_color"} == {k: v for k, v in denoise_ref.DEFAULTS.items() if k != "sigma_color"}
    assert D.DENOISE_DEFAULTS["sigma_color"] == 1.0  # the fixed-sigma filter keeps its own
    src = open(os.path.join(ROOT, "take_amd", "csrc", "tk_denoise.hip")).read()
    assert "SIGMA_COLOR = 1.0, SIGMA_COLOR_VARIANCE = 4.0" in src
    # a value <= 0 and a missing one are the default: the restatement, as the library
    p = V.cast(V.sampled_planes(7, 5), np.float64)
    first = V.denoise_variance(**p)
    assert np.array_equal(first, V.denoise_variance(**p, sigma_color=4.0)) and np.array_equal(first, V.denoise_variance(**p, sigma_color=-1.0))
    assert not np.array_equal(first, V.denoise_variance(**p, sigma_color=1.0))


def test_refusals_come_before_the_device_is_looked_for(lib):
    """TAKE_E_INVALID with its message, never TAKE_E_NO_GPU, with or without a GPU.  (`scene` and the planes below are
    not a scene and not device memory: a call that went past the argument check would not survive it.)"""
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    scene = C.cast(C.create_string_buffer(64), C.c_void_p)
    ro = D.TakeRenderOpts()
    ro.spp = 1
    F32 = D.TAKE_PRECISION_F32
    full = D.TakeAdaptiveStats(buf.value, buf.value, buf.value)

    def ref(x):
        return None if x is None else C.byref(x)

    def dev(rgb=buf, stats=full, precision=F32, w=2, h=2, opts=None, out=buf):
        return lib.take_hip_denoise_variance_device(rgb, None, ref(stats), precision, w, h, ref(opts), out, None, None)

    def host(rgb=buf, stats=full, precision=F32, w=2, h=2, opts=None, out=buf):
        return lib.take_hip_denoise_variance(rgb, None, ref(stats), precision, w, h, ref(opts), out, None)

    def rd(sc=scene, o=ro, a=None, opts=None, out=buf):
        return lib.take_hip_render_adaptive_denoised_device(sc, ref(o), ref(a), ref(opts), out, None, None, None)

    def rh(sc=scene, o=ro, a=None, opts=None, out=buf):
        return lib.take_hip_render_adaptive_denoised(sc, ref(o), ref(a), ref(opts), out, None, None)

    bad_opts = [(D.denoise_opts(iterations=9), b"iterations"), (D.TakeDenoiseOpts(0, 2, 0, 0, 0, 0), b"unknown flag"),
                (D.TakeDenoiseOpts(0, -1, 0, 0, 0, 0), b"unknown flag")]
    for field in ("sigma_color", "sigma_normal", "sigma_depth", "albedo_floor"):
        for v in (float("nan"), float("inf"), -float("inf")):
            o = D.TakeDenoiseOpts()
            setattr(o, field, v)
            bad_opts.append((o, b"must be finite"))
    bad_adaptive = [(D.adaptive_opts(threshold=float("nan")), b"threshold and floor must be finite"), (D.adaptive_opts(floor=float("inf")), b"threshold and floor must be finite"),
                    (D.TakeAdaptiveOpts(0, 0, -1.0, 0.0, 1, 0), b"unknown flag bits")]
    partial = [D.TakeAdaptiveStats(*[None if j == k else buf.value for j in range(3)]) for k in range(3)]
    cases = []
    for f in (dev, host):
        cases += [(lambda f=f: f(rgb=None), b"null argument"), (lambda f=f: f(out=None), b"null argument"), (lambda f=f: f(stats=None), b"null argument")]
        cases += [(lambda f=f, s=s: f(stats=s), b"null argument") for s in partial]
        cases += [(lambda f=f: f(w=0), b"width and height"), (lambda f=f: f(h=-3), b"width and height"),
                  (lambda f=f: f(precision=D.TAKE_PRECISION_MIXED), b"unknown precision"), (lambda f=f: f(precision=-1), b"unknown precision")]
    for f in (rd, rh):
        cases += [(lambda f=f: f(sc=None), b"null argument"), (lambda f=f: f(o=None), b"null argument"), (lambda f=f: f(out=None), b"null argument")]
        cases += [(lambda f=f, a=a: f(a=a), msg) for a, msg in bad_adaptive]
        # the refusals of the two parts in that order: the sampler's options before the denoiser's
        cases.append((lambda f=f: f(a=bad_adaptive[0][0], opts=bad_opts[0][0]), bad_adaptive[0][1]))
    for f in (dev, host, rd, rh):
        cases += [(lambda f=f, o=o: f(opts=o), msg) for o, msg in bad_opts]
    assert len(cases) == 2 * 10 + 2 * 7 + 4 * 15
    for call, msg in cases:
        lib.take_hip_scene_build_info(None, None, None)  # (leaves another message behind)
        assert b"null scene" in lib.take_hip_last_error()
        assert call() == D.TAKE_E_INVALID
        assert msg in lib.take_hip_last_error(), (msg, lib.take_hip_last_error())


def test_the_python_binding_checks_its_arrays():
    rgb = np.zeros((4, 5, 3), np.float32)
    st = dict(count=np.zeros((4, 5), np.int32), m1=np.zeros((4, 5)), m2=np.zeros((4, 5)))
    for kw in (dict(st, rgb=np.zeros((4, 5, 3), np.int32)), dict(st, rgb=np.zeros((4, 5), np.float32)), dict(st, rgb=rgb, depth=np.zeros((4, 5, 1), np.float32)),
               dict(st, rgb=rgb, albedo=np.zeros((4, 5, 3), np.float64)), dict(st, rgb=rgb, opts=D.denoise_opts(), iterations=2),
               dict(st, rgb=rgb, count=np.zeros((4, 5), np.int64)), dict(st, rgb=rgb, m1=np.zeros((4, 5), np.float32)), dict(st, rgb=rgb, m2=np.zeros((5, 4))),
               dict(st, rgb=rgb, m2=None)):
        with pytest.raises(ValueError):
            capi.denoise_variance(**kw)


# ------------------------------------------------------------------ host execution of tk_denoise_var.h
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        d = os.path.join(HERE, "denoise_var_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libdenoise_var_host.so"))
        L.denoise_var_host.argtypes = [C.c_int32] + [C.c_void_p] * 7 + [C.c_int32] * 4 + [C.c_void_p] * 3
        _HOST = L
    return _HOST


def host_denoise(p, in_place=False, variance=True, **opts):
    """p: contiguous planes, rgb and a subset of albedo / normal / depth in one dtype, count / m1 / m2 -> what the kernels'
    text computes: (image, variance_out), or the image alone"""
    o = dict(V.DEFAULTS)
    o.update(opts)
    rgb = p["rgb"].copy()
    out = rgb if in_place else np.full_like(rgb, np.nan)
    var = np.full(rgb.shape[:2], np.nan, rgb.dtype) if variance else None
    sf = np.array([o["sigma_color"], o["sigma_normal"], o["sigma_depth"], o["albedo_floor"]], np.float64)
    rc = host_lib().denoise_var_host(int(rgb.dtype == np.float64), rgb.ctypes.data, *[p[g].ctypes.data if g in p else None for g in GUIDES],
                                     *[p[s].ctypes.data for s in STATS], rgb.shape[1], rgb.shape[0], o["iterations"], int(o["keep_albedo"]), sf.ctypes.data,
                                     out.ctypes.data, None if var is None else var.ctypes.data)
    assert rc == 0
    return (out, var) if variance else out


_PLANES = {}


def sampled(size, variant=False):
    """the sampled planes, made once per size and never written to"""
    if (size, variant) not in _PLANES:
        _PLANES[size, variant] = V.sampled_planes(*size, variant=variant)
    return _PLANES[size, variant]


def subset(p, guides):
    return {k: v for k, v in p.items() if k == "rgb" or k in STATS or k in guides}


def widen(p):
    """the planes of a float32 case as the f64 restatement takes them"""
    return {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in p.items()}


# the cases of tests/test_denoise_cpu.py on the sampled planes, and the variant (a column of single samples, a block of
# rows without variance) at the two sizes that have room for it
VAR_CASES = [(c, False) for c in CASES] + [((s, GUIDES, {}), True) for s in ((37, 23), (130, 70))]


def var_case_id(vc):
    return case_id(vc[0]) + ("-variant" if vc[1] else "")


def check(got, ref, bar, label):
    """(image, variance) against (image, variance): the image on max(1, max|ref|), the variance on max|V_ref|"""
    for what, g, r, scale in (("image", got[0], ref[0], max(1.0, float(np.abs(ref[0]).max()))), ("variance", got[1], ref[1], float(np.abs(ref[1]).max()))):
        d = float(np.abs(g.astype(np.float64) - r).max())
        print(f"{label} {what}: max |difference| {d:.3e}, bar {bar * scale:.3e}")
        assert np.isfinite(g).all() and d <= bar * scale, (label, what, d)


@pytest.mark.parametrize("vc", VAR_CASES, ids=var_case_id)
def test_host_build_against_the_restatement_f64(vc):
    (size, guides, opts), variant = vc
    p = subset(V.cast(sampled(size, variant), np.float64), guides)
    check(host_denoise(p, **opts), V.denoise_variance(**p, variance=True, **opts), 1e-12, "f64 " + var_case_id(vc))


@pytest.mark.parametrize("vc", VAR_CASES, ids=var_case_id)
def test_host_build_against_the_restatement_f32(vc):
    (size, guides, opts), variant = vc
    p = subset(V.cast(sampled(size, variant), np.float32), guides)
    got = host_denoise(p, **opts)
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    ref64 = V.denoise_variance(**widen(p), variance=True, **opts)
    check(got, ref64, 1e-5, "f32 against f64 " + var_case_id(vc))
    check(V.denoise_variance(**p, variance=True, **opts), ref64, 1e-5, "f32 restatement against f64 " + var_case_id(vc))


def test_host_build_in_place_repeated_and_without_the_variance_plane():
    p = V.cast(sampled((37, 23), True), np.float64)
    a, va = host_denoise(p)
    b, vb = host_denoise(p)
    c, vc = host_denoise(p, in_place=True)
    assert np.array_equal(a, b) and np.array_equal(va, vb) and np.array_equal(a, c) and np.array_equal(va, vc)
    assert np.array_equal(a, host_denoise(p, variance=False))


def test_the_cases_can_tell_a_wrong_level_from_a_right_one():
    """one level fewer, or the fixed filter's sigma, moves image and variance by orders above either bar"""
    p = V.cast(sampled((37, 23)), np.float64)
    a, va = V.denoise_variance(**p, variance=True)
    b, vb = V.denoise_variance(**p, variance=True, iterations=4)
    d, dv = float(np.abs(a - b).max()), float(np.abs(va - vb).max() / np.abs(va).max())
    print(f"iterations 4 against 5: image {d:.3e}, variance {dv:.3e} of its maximum")
    assert d > 1e-3 and dv > 1e-3


# ------------------------------------------------------------------ properties of the specification (the restatement alone)
@pytest.mark.parametrize("size", [(37, 23), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_low_noise_edge_is_cleaned_where_the_fixed_filter_blurs_it(size):
    """the case the feature exists for: a 20 % illumination step under 2 % noise, no guides"""
    e = V.edge_planes(*size)
    raw = rmse(e["rgb"], e["clean"])
    new = rmse(V.denoise_variance(e["rgb"], e["count"], e["m1"], e["m2"]), e["clean"])
    old = rmse(denoise_ref.denoise(e["rgb"]), e["clean"])
    print(f"step plane {size}: RMSE to clean: raw {raw:.5f}, variance-guided {new:.5f} (raw / {raw / new:.1f}), fixed filter {old:.5f} ({old / raw:.1f} x raw)")
    assert new < raw / 4 and old > 2 * raw


@pytest.mark.parametrize("size", [(37, 23), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_sky_band_is_filtered_and_the_whole_image_beats_the_fixed_filter(size):
    p = sampled(size)
    g = {k: p[k] for k in GUIDES}
    new = V.denoise_variance(p["rgb"], p["count"], p["m1"], p["m2"], **g)
    old = denoise_ref.denoise(p["rgb"], **g)
    sky = slice(0, size[1] // 5)
    assert (p["albedo"][sky] == 0).all() and (p["albedo"][size[1] // 5:] > 0).all()
    raw_s, new_s, old_s = (rmse(a[sky], p["clean"][sky]) for a in (p["rgb"], new, old))
    raw_w, new_w, old_w = (rmse(a, p["clean"]) for a in (p["rgb"], new, old))
    print(f"{size}: sky band: raw {raw_s:.4f}, variance-guided {new_s:.4f} (raw / {raw_s / new_s:.1f}), fixed {old_s:.4f}; "
          f"whole image: raw {raw_w:.4f}, fixed {old_w:.4f}, variance-guided {new_w:.4f}")
    assert new_s < raw_s / 4
    assert new_w < old_w


def test_zero_variance_gives_the_image_back():
    p = V.cast(sampled((37, 23)), np.float64)
    p["count"] = np.full_like(p["count"], 4)
    p["m2"] = p["m1"] * p["m1"] / 4.0
    out, var = V.denoise_variance(**p, variance=True)
    d = float(np.abs(out - p["rgb"]).max())
    print(f"zero variance: max |out - rgb| {d:.3e}")
    assert d <= 1e-15 * max(1.0, float(np.abs(p["rgb"]).max()))
    assert (var == 0).all()
    host_out, host_var = host_denoise(p)
    assert float(np.abs(host_out - p["rgb"]).max()) <= 1e-15 * max(1.0, float(np.abs(p["rgb"]).max())) and (host_var == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_single_sample_everywhere_gives_a_finite_result(dtype):
    raw = sampled((37, 23))
    rgb = raw["rgb"]
    L = (rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]
    p = V.cast(dict(raw, count=np.ones_like(raw["count"]), m1=L, m2=L * L), dtype)
    for out, var in (V.denoise_variance(**p, variance=True), host_denoise(p)):
        assert np.isfinite(out).all() and np.isfinite(var).all() and (var > 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_variance_of_a_constant_image_propagates_exactly(dtype):
    """held to arithmetic, not to the restatement: on a constant image every weight is its kernel value, the weights sum
    to 1, and one level leaves V0 * sum(k^2) = V0 * (sum(h^2))^2 = V0 * 0.2734375^2 — exact in binary"""
    w, h = 11, 9
    L0, d = 1.5, 2.0 ** -5  # two samples L0 +- d: mean L0, v = d^2, and count 2 gives s2 = v
    p = dict(rgb=np.full((h, w, 3), 0.5, dtype), count=np.full((h, w), 2, np.int32), m1=np.full((h, w), 2 * L0),
             m2=np.full((h, w), (L0 + d) * (L0 + d) + (L0 - d) * (L0 - d)))
    assert (V.initial_variance(p["count"], p["m1"], p["m2"]) == 2.0 ** -10).all()
    want = dtype(2.0 ** -10 * 0.07476806640625)
    assert 0.07476806640625 == 0.2734375 ** 2 == sum(a * b * a * b for a in (0.0625, 0.25, 0.375, 0.25, 0.0625) for b in (0.0625, 0.25, 0.375, 0.25, 0.0625))
    for out, var in (V.denoise_variance(**p, variance=True, iterations=1), host_denoise(p, iterations=1)):
        assert var.dtype == dtype and (var[2:-2, 2:-2] == want).all()
        assert (var[0] > want).all()  # (fewer taps at the border: the weights are renormalised)
        assert np.array_equal(out, p["rgb"])

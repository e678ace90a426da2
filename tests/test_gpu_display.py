"""The display transform on the device (take_hip_luminance_histogram*, take_hip_tonemap*: include/take_hip.h; kernels:
take_amd/csrc/tk_display.h) against the numpy restatement of its specification (tests/display_ref.py), in the image's
own precision.

Shapes (display_ref.SHAPES, width x height): 1x1; 7x3 (under one wave); 65x5 (a wave plus one); 257x3 (a block plus one);
641x97 (243 blocks, a ragged last one); 1024x600 — 614400 pixels against the launch's cap of 2048 blocks x 256 threads =
524288, so that the grid-stride loops of all three kernels go round a second time, and the sum kernel reads all 2048 rows.
Contents: log-uniform luminance over 2^-30 .. 2^30 with a random hue (every f32 value normal); a constant image (every
lane of a wave in one bin: the contention case and the lane-count path); an image salted with NaN, +Inf, -Inf, negatives,
both zeros and, in f64, values beyond float's range; and, for the operators, luminance over the 14 octaves a display
shows at exposure 1.

Bars.  Histogram: equal.  LINEAR transfer: REAL outputs and RGBA codes bit-identical.  SRGB (display_ref.allowance: A =
16 ulp of 1.0, 2^-20 in f32 and 2^-49 in f64): REAL within A; RGBA codes differ by at most 1, only where the
restatement's unrounded value lies within 255 A of an integer, in at most 0.5 % of the channels — after the restatement
alone has shown that at most 0.5 % of its channels lie that close.  Auto-exposure: 1e-12 relative.  Everything the library
is compared with itself on is np.array_equal."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the library is loaded: the two share one HIP runtime only in this order)

import display_ref as ref
from helpers import GOLD, golden_scene
from take_amd import capi, png
from take_amd import cdefs as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64
DTYPES = (np.float32, np.float64)


def precision_of(dtype):
    return F32 if np.dtype(dtype) == np.float32 else F64


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def on_device(img):
    return torch.from_numpy(np.array(img)).cuda()


# ------------------------------------------------------------------ the histogram
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("content", ["log-uniform", "constant", "salted"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_histogram_equals_the_restatement(shape, content, dtype):
    img = ref.image(content, shape, dtype)
    want = ref.histogram(img)
    got = capi.luminance_histogram(img)
    assert got.dtype == np.int64 and got.shape == (ref.SLOTS,)
    assert got.sum() == shape[0] * shape[1]
    assert np.array_equal(got, want), [(int(s), int(g), int(w)) for s, (g, w) in enumerate(zip(got, want)) if g != w][:8]
    if content == "constant":
        assert (got > 0).sum() == 1
    if content == "salted":
        assert got[ref.NONFINITE] > 0 and (shape[0] * shape[1] < 300 or got[ref.NONPOSITIVE] > 0)  # (the salt reaches both extra slots)
    # the device twin, and again: the same counts
    t = on_device(img)
    for _ in range(2):
        assert np.array_equal(capi.luminance_histogram_device(t, shape[0], shape[1], precision_of(dtype)), want)
    assert np.array_equal(t.cpu().numpy(), img, equal_nan=True)  # the input is left alone


# ------------------------------------------------------------------ the fused pass
def tonemap_all_ways(img, exposure, op, transfer):
    """-> (REAL, RGBA) of the host-plane calls, after the device twins — out of place, and REAL in place — and the
    host-plane call with out == rgb have given the same bits"""
    h, w = img.shape[:2]
    kw = dict(exposure=exposure, op=op, transfer=transfer)
    real, used = capi.tonemap(img, format="real", **kw)
    rgba, used2 = capi.tonemap(img, format="rgba", **kw)
    assert used == used2 == exposure
    assert real.dtype == img.dtype and real.shape == img.shape and rgba.dtype == np.uint8 and rgba.shape == (h, w, 4)
    t = on_device(img)
    d_real, d_rgba = torch.full_like(t, -7.0), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    assert capi.tonemap_device(t, w, h, precision_of(img.dtype), out=d_real, format="real", **kw) == exposure
    assert capi.tonemap_device(t, w, h, precision_of(img.dtype), out=d_rgba, format="rgba", **kw) == exposure
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), img, equal_nan=True)
    assert np.array_equal(d_real.cpu().numpy(), real) and np.array_equal(d_rgba.cpu().numpy(), rgba)
    capi.tonemap_device(t, w, h, precision_of(img.dtype), format="real", **kw)  # in place
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), real)
    buf = np.array(img)  # the host-plane call, out == rgb
    o = D.tonemap_opts(format="real", **kw)
    capi._check(capi.lib().take_hip_tonemap(buf.ctypes.data, precision_of(img.dtype), w, h, C.byref(o), buf.ctypes.data, None))
    assert np.array_equal(buf, real)
    return real, rgba


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("op", list(ref.OPS))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_linear_transfer_is_bit_identical_to_the_restatement(shape, op, dtype):
    for content, exposure in (("salted", 1.0), ("midrange", 0.37), ("log-uniform", 1.0)):
        img = ref.image(content, shape, dtype)
        real, rgba = tonemap_all_ways(img, exposure, op, "linear")
        want = ref.tone(img, exposure, op=ref.OPS[op], transfer=ref.TRANSFER_LINEAR)
        assert np.isfinite(want).all()
        assert np.array_equal(real, want), f"{content}: {int((real != want).sum())} values differ, by at most {np.abs(real - want).max():.3e}"
        assert np.array_equal(rgba, ref.rgba(img, exposure, op=ref.OPS[op], transfer=ref.TRANSFER_LINEAR)), content


def test_reinhard_white_reaches_the_kernel():
    img = ref.image("midrange", (65, 5), np.float32)
    got, _ = capi.tonemap(img, exposure=1.0, op="reinhard", transfer="linear", format="real", white=1.5)
    assert np.array_equal(got, ref.tone(img, 1.0, op=ref.REINHARD, transfer=ref.TRANSFER_LINEAR, white=1.5))
    assert not np.array_equal(got, capi.tonemap(img, exposure=1.0, op="reinhard", transfer="linear", format="real")[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("op", list(ref.OPS))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_srgb_within_the_bars(shape, op, dtype):
    for content in ("midrange", "salted"):
        img = ref.image(content, shape, dtype)
        y, near = ref.restated_srgb(img, 1.0, op=ref.OPS[op])  # (asserts on the restatement alone, before the device is looked at)
        real, rgba = tonemap_all_ways(img, 1.0, op, "srgb")
        label = f"{content} {shape_id(shape)} {op} {np.dtype(dtype).name}"
        ref.check_srgb_real(real, y, label)
        ref.check_srgb_codes(rgba, y, near, label)


# ------------------------------------------------------------------ automatic against explicit exposure
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("content", ["midrange", "salted", "constant"])
def test_automatic_exposure_is_the_histogram_s_and_the_same_pixels(content, dtype):
    shape = (641, 97)
    img = ref.image(content, shape, dtype)
    hist = capi.luminance_histogram(img)
    for auto in ({}, dict(key=0.3, low_fraction=0.2, high_fraction=0.7), dict(prev_exposure=0.01, rate=0.25)):
        want = capi.auto_exposure(hist, **auto)
        assert abs(want - ref.auto_exposure(ref.histogram(img), **auto)) <= 1e-12 * want
        for fmt in ("rgba", "real"):
            got, used = capi.tonemap(img, format=fmt, **auto)
            print(f"{content} {auto} {fmt}: exposure {used!r}, auto_exposure {want!r}")
            assert abs(used - want) <= 1e-12 * want
            again, used2 = capi.tonemap(img, exposure=used, format=fmt)
            assert used2 == used and np.array_equal(got, again)
    # NULL options: ACES, sRGB, RGBA, automatic with the defaults; and the device twin
    out, used = np.zeros(img.shape[:2] + (4,), np.uint8), C.c_double(0.0)
    capi._check(capi.lib().take_hip_tonemap(img.ctypes.data, precision_of(dtype), shape[0], shape[1], None, out.ctypes.data, C.byref(used)))
    got, want = capi.tonemap(img)
    assert used.value == want and np.array_equal(out, got)
    t, d_out = on_device(img), torch.zeros(img.shape[:2] + (4,), dtype=torch.uint8, device="cuda")
    assert capi.tonemap_device(t, shape[0], shape[1], precision_of(dtype), out=d_out) == want
    assert np.array_equal(d_out.cpu().numpy(), got)


# ------------------------------------------------------------------ command line, in a fresh process
def run_cli(cwd, *flags):
    scene = os.path.join(GOLD, "scenes", "cbox.tkscene")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "take_amd.render", scene, "-max_depth", "5", *flags], cwd=cwd, env=env, timeout=120, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout


def test_cli_png_writes_a_png_beside_every_exr_with_one_exposure(tmp_path):
    for d in ("without", "with", "reinhard"):
        (tmp_path / d).mkdir()
    run_cli(tmp_path / "without", "-denoise")
    out = run_cli(tmp_path / "with", "-denoise", "-png")
    assert sorted(p.name for p in (tmp_path / "without").iterdir()) == ["denoised.exr", "image.exr"]
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == ["denoised.exr", "denoised.png", "image.exr", "image.png"]
    for name in ("image.exr", "denoised.exr"):
        assert (tmp_path / "with" / name).read_bytes() == (tmp_path / "without" / name).read_bytes(), name
    lines = [l for l in out.splitlines() if l.startswith("png: exposure ")]
    assert len(lines) == 1 and lines[0].endswith("(aces)"), out
    E = float(re.match(r"png: exposure (\S+) ", lines[0]).group(1))
    sd = golden_scene("cbox")
    sc = capi.Scene(sd)
    try:
        image = sc.render(spp=sd.spp, max_depth=5, seed=0)
        denoised = sc.render_denoised(spp=sd.spp, max_depth=5, seed=0)
    finally:
        sc.close()
    assert E == capi.auto_exposure(capi.luminance_histogram(image))
    for name, img in (("image.png", image), ("denoised.png", denoised)):  # both with the one exposure
        got = png.read_png(tmp_path / "with" / name)
        assert got.shape == (sd.height, sd.width, 4) and np.array_equal(got, capi.tonemap(img, exposure=E)[0]), name
    # the operator is the next parameter if it is one of the three words; the scene file may follow it
    out = run_cli(tmp_path / "reinhard", "-png", "reinhard")
    assert [l for l in out.splitlines() if l.startswith("png: exposure ")] == [f"png: exposure {E!r} (reinhard)"]
    assert np.array_equal(png.read_png(tmp_path / "reinhard" / "image.png"), capi.tonemap(image, exposure=E, op="reinhard")[0])
    assert (tmp_path / "reinhard" / "image.exr").read_bytes() == (tmp_path / "without" / "image.exr").read_bytes()

"""Bloom on the device (take_hip_bloom_layer*, take_hip_tonemap_bloom*, take_hip_image_workspace_*: include/take_hip.h;
kernels: take_amd/csrc/tk_bloom.h) against the numpy restatement of its specification (tests/bloom_ref.py), in the
image's own precision, through the C ABI.

Shapes (bloom_ref.SHAPES, width x height), chosen for where the kernels can go wrong: 1x1, 2x2, 3x5, 7x3 (levels of size
1, odd sizes, clamps on every side); 33x17 and 65x5 (one 16 x 16 tile plus a sliver); 130x70 (level 0 is 65 x 35: several
tiles, halos crossing tile borders, a partial last tile on both axes); 257x3 (eight levels, the cap); 641x97.
Contents: log-uniform luminance over 2^-30 .. 2^30; constants below t - k and above t; impulses at a corner, at the
centre and at (32, 32), where four staged tiles meet; an image salted with NaN, +Inf, -Inf, negatives, zeros and, in
f64, values beyond float's range; and, for the operators, luminance over the 14 octaves a display shows.
Option sets (bloom_ref.OPTION_SETS): the defaults; knee 0; threshold 0; levels 1, 3 and all.

Bars.  The layer, and the composite with LINEAR transfer (REAL and RGBA): bit-identical to the restatement.  SRGB:
display_ref's bars unchanged (A = 16 ulp of 1.0; codes differ by at most 1, only where the restatement's unrounded value
lies within 255 A of an integer, in at most 0.5 % of the channels, after the restatement alone has shown that at most
0.5 % lie that close — tests/test_bloom_cpu.py asserts that for every image used here, without a GPU).  Auto-exposure:
equal to capi.auto_exposure of capi.luminance_histogram.  Everything the library is compared with itself on — host and
device twin, a repeated call, with a workspace and without, in place and out of place — is np.array_equal."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch  # (before the library is loaded: the two share one HIP runtime only in this order)

import bloom_ref as ref
import display_ref as dref
from helpers import GOLD, golden_scene
from take_amd import capi, png
from take_amd import cdefs as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64
DTYPES = (np.float32, np.float64)
OTHER_BLOOM = dict(threshold=0.5, knee=0.25, intensity=0.6, levels=3)


def precision_of(dtype):
    return F32 if np.dtype(dtype) == np.float32 else F64


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def on_device(img):
    return torch.from_numpy(np.array(img)).cuda()


@pytest.fixture(scope="module")
def workspace():
    with capi.ImageWorkspace() as ws:
        yield ws


def device_layer(img, exposure, workspace=None, in_place=False, **bloom):
    h, w = img.shape[:2]
    t = on_device(img)
    out = t if in_place else torch.full_like(t, -7.0)
    capi.bloom_layer_device(t, w, h, precision_of(img.dtype), exposure, out, workspace=workspace, **bloom)
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(t.cpu().numpy(), img, equal_nan=True)  # the input is left alone
    return out.cpu().numpy()


# ------------------------------------------------------------------ the layer
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_layer_is_bit_identical_to_the_restatement(shape, dtype, workspace):
    cases = [(content, "defaults") for content in ref.CONTENTS] + [(content, name) for content in ("log-uniform", "salted", "above", "border") for name in ref.OPTION_SETS if name != "defaults"]
    for content, name in cases:
        img, bloom = ref.image(content, shape, dtype), ref.OPTION_SETS[name]
        exposure = 0.37 if content == "log-uniform" else 1.0
        want = ref.layer(img, exposure, **bloom)
        got = capi.bloom_layer(img, exposure, **bloom)
        label = f"{content}, {name}"
        assert got.dtype == want.dtype and got.shape == want.shape and np.isfinite(got).all(), label
        assert np.array_equal(got, want), f"{label}: {int((got != want).sum())} values differ, by at most {np.abs(got - want).max():.3e}"
        if content == "below":
            assert not got.any()
        if content in ("above", "corner", "centre"):
            assert got.max() > 0
        # the device twin without a workspace, with one, again with it, and over its input: the same bytes
        assert np.array_equal(device_layer(img, exposure, **bloom), want), label
        for _ in range(2):
            assert np.array_equal(device_layer(img, exposure, workspace=workspace, **bloom), want), label
        assert np.array_equal(device_layer(img, exposure, workspace=workspace, in_place=True, **bloom), want), label


# ------------------------------------------------------------------ the composite
def tonemap_bloom_all_ways(img, exposure, op, transfer, workspace, **bloom):
    """-> (REAL, RGBA) of the host-plane calls, after the device twins — with a workspace and without, out of place, and
    REAL in place — have given the same bits"""
    h, w = img.shape[:2]
    kw = dict(exposure=exposure, op=op, transfer=transfer, **bloom)
    real, used = capi.tonemap_bloom(img, format="real", **kw)
    rgba, used2 = capi.tonemap_bloom(img, format="rgba", **kw)
    assert used == used2 == exposure
    assert real.dtype == img.dtype and real.shape == img.shape and rgba.dtype == np.uint8 and rgba.shape == (h, w, 4)
    t = on_device(img)
    for ws in (None, workspace):
        d_real, d_rgba = torch.full_like(t, -7.0), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        assert capi.tonemap_bloom_device(t, w, h, precision_of(img.dtype), out=d_real, format="real", workspace=ws, **kw) == exposure
        assert capi.tonemap_bloom_device(t, w, h, precision_of(img.dtype), out=d_rgba, format="rgba", workspace=ws, **kw) == exposure
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), img, equal_nan=True)
        assert np.array_equal(d_real.cpu().numpy(), real) and np.array_equal(d_rgba.cpu().numpy(), rgba)
    capi.tonemap_bloom_device(t, w, h, precision_of(img.dtype), format="real", workspace=workspace, **kw)  # in place
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), real)
    return real, rgba


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_linear_transfer_is_bit_identical_to_the_restatement(shape, dtype, workspace):
    sets = ref.OPTION_SETS
    for content, exposure, bloom in (("salted", 1.0, {}), ("midrange", 0.37, OTHER_BLOOM), ("log-uniform", 1.0, {}), ("above", 1.0, sets["levels 1"]), ("border", 1.0, {}),
                                     ("salted", 0.37, sets["knee 0"]), ("log-uniform", 0.37, sets["threshold 0"]), ("midrange", 1.0, sets["threshold 0"])):
        img = ref.image(content, shape, dtype)
        x = ref.composite_input(img, exposure, **bloom)
        for op in dref.OPS:
            real, rgba = tonemap_bloom_all_ways(img, exposure, op, "linear", workspace, **bloom)
            want = ref.tail(x, dref.OPS[op], dref.TRANSFER_LINEAR)
            assert np.isfinite(want).all()
            assert np.array_equal(real, want), f"{content} {op}: {int((real != want).sum())} values differ, by at most {np.abs(real - want).max():.3e}"
            assert (rgba[..., 3] == 255).all() and np.array_equal(rgba[..., :3], dref.codes(want)), (content, op)


def test_reinhard_white_reaches_the_kernel():
    img = ref.image("midrange", (65, 5), np.float32)
    got, _ = capi.tonemap_bloom(img, exposure=1.0, op="reinhard", transfer="linear", format="real", white=1.5)
    assert np.array_equal(got, ref.tone(img, 1.0, op=dref.REINHARD, transfer=dref.TRANSFER_LINEAR, white=1.5))
    assert not np.array_equal(got, capi.tonemap_bloom(img, exposure=1.0, op="reinhard", transfer="linear", format="real")[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=shape_id)
def test_srgb_within_the_bars(shape, dtype, workspace):
    for content in ("midrange", "salted", "log-uniform"):
        img = ref.image(content, shape, dtype)
        for op in dref.OPS:
            y, near = ref.restated_srgb(img, 1.0, op=dref.OPS[op])  # (asserts on the restatement alone, before the device is looked at)
            real, rgba = tonemap_bloom_all_ways(img, 1.0, op, "srgb", workspace)
            label = f"{content} {shape_id(shape)} {op} {np.dtype(dtype).name}"
            dref.check_srgb_real(real, y, label)
            dref.check_srgb_codes(rgba, y, near, label)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_intensity_zero_is_take_hip_tonemap_device(dtype, workspace):
    for shape in ((7, 3), (130, 70), (641, 97)):
        for content in ("salted", "log-uniform", "above"):
            img = ref.image(content, shape, dtype)
            h, w = img.shape[:2]
            t = on_device(img)
            for fmt, op, transfer in (("rgba", "aces", "srgb"), ("real", "reinhard", "srgb"), ("real", "linear", "linear"), ("rgba", "linear", "linear")):
                def out():
                    return torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") if fmt == "rgba" else torch.full_like(t, -7.0)

                plain, bloomed = out(), out()
                kw = dict(exposure=0.8, op=op, transfer=transfer, format=fmt)
                capi.tonemap_device(t, w, h, precision_of(dtype), out=plain, **kw)
                capi.tonemap_bloom_device(t, w, h, precision_of(dtype), out=bloomed, intensity=0.0, workspace=workspace, **kw)
                torch.cuda.synchronize()
                assert torch.equal(plain, bloomed), (shape, content, fmt, op)


# ------------------------------------------------------------------ the workspace
def test_one_workspace_across_growing_then_shrinking_images():
    """the workspace grows, never shrinks, and what an earlier, larger image left in it does not reach a later one"""
    sizes = [(7, 3), (130, 70), (641, 97), (33, 17), (1, 1), (257, 3), (2, 2)]
    with capi.ImageWorkspace() as ws:
        for dtype in DTYPES:
            for shape in sizes:
                img = ref.image("log-uniform", shape, dtype)
                h, w = img.shape[:2]
                t = on_device(img)
                assert np.array_equal(device_layer(img, 0.37, workspace=ws), device_layer(img, 0.37))
                with_ws, without = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda"), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
                e1 = capi.tonemap_bloom_device(t, w, h, precision_of(dtype), out=with_ws, workspace=ws)  # automatic: the histogram's rows too
                e2 = capi.tonemap_bloom_device(t, w, h, precision_of(dtype), out=without)
                torch.cuda.synchronize()
                assert e1 == e2 and torch.equal(with_ws, without), shape
    with pytest.raises(ValueError):
        capi.tonemap_bloom_device(t, w, h, precision_of(dtype), out=without, workspace=ws)  # closed


# ------------------------------------------------------------------ automatic against explicit exposure
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("content", ["midrange", "salted", "above"])
def test_automatic_exposure_is_the_histogram_s_and_the_same_pixels(content, dtype, workspace):
    shape = (641, 97)
    img = ref.image(content, shape, dtype)
    h, w = img.shape[:2]
    hist = capi.luminance_histogram(img)
    assert np.array_equal(hist, dref.histogram(img))
    t = on_device(img)
    for auto in ({}, dict(key=0.3, low_fraction=0.2, high_fraction=0.7), dict(prev_exposure=0.01, rate=0.25)):
        want = capi.auto_exposure(hist, **auto)
        for fmt in ("rgba", "real"):
            got, used = capi.tonemap_bloom(img, format=fmt, **auto)
            print(f"{content} {auto} {fmt}: exposure {used!r}, auto_exposure {want!r}")
            assert used == want
            again, used2 = capi.tonemap_bloom(img, exposure=used, format=fmt)
            assert used2 == used and np.array_equal(got, again)
        d_out = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        assert capi.tonemap_bloom_device(t, w, h, precision_of(dtype), out=d_out, workspace=workspace, **auto) == want
        assert np.array_equal(d_out.cpu().numpy(), capi.tonemap_bloom(img, exposure=want)[0])
    # the plain call picks the same exposure: the histogram is of the input image, not of the composite
    assert capi.tonemap(img)[1] == capi.tonemap_bloom(img)[1]


# ------------------------------------------------------------------ command line, in a fresh process
def run_cli(cwd, *flags):
    scene = os.path.join(GOLD, "scenes", "cbox.tkscene")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "take_amd.render", scene, "-max_depth", "5", *flags], cwd=cwd, env=env, timeout=120, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout


def test_cli_png_bloom_writes_the_composite_with_the_one_exposure(tmp_path):
    for d in ("plain", "bloom"):
        (tmp_path / d).mkdir()
    run_cli(tmp_path / "plain", "-denoise", "-png")
    out = run_cli(tmp_path / "bloom", "-denoise", "-png", "-bloom", "0.5")
    assert sorted(p.name for p in (tmp_path / "bloom").iterdir()) == ["denoised.exr", "denoised.png", "image.exr", "image.png"]
    for name in ("image.exr", "denoised.exr"):
        assert (tmp_path / "bloom" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    lines = [l for l in out.splitlines() if l.startswith("png: ")]
    assert len(lines) == 2 and lines[0].endswith("(aces)") and lines[1] == "png: bloom intensity 0.5", out
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
        got = png.read_png(tmp_path / "bloom" / name)
        assert got.shape == (sd.height, sd.width, 4) and np.array_equal(got, capi.tonemap_bloom(img, exposure=E, intensity=0.5)[0]), name
        assert np.array_equal(png.read_png(tmp_path / "plain" / name), capi.tonemap(img, exposure=E)[0]), name
    # the light of the box exceeds the display range at that exposure: the glare is there
    assert not np.array_equal(png.read_png(tmp_path / "bloom" / "image.png"), png.read_png(tmp_path / "plain" / "image.png"))
    # the intensity is optional
    (tmp_path / "default").mkdir()
    out = run_cli(tmp_path / "default", "-png", "reinhard", "-bloom")
    assert f"png: exposure {E!r} (reinhard)" in out and "png: bloom intensity 0.25" in out
    assert np.array_equal(png.read_png(tmp_path / "default" / "image.png"), capi.tonemap_bloom(image, exposure=E, op="reinhard")[0])

"""The image-space denoiser on the device (take_hip_denoise*, take_hip_render_denoised*: include/take_hip.h; kernels:
take_amd/csrc/tk_denoise.h) against the numpy restatement of its specification (tests/denoise_ref.py) in f64.

Planes: the synthetic ones of denoise_ref.planes with 30 % multiplicative noise, at 1x1, 7x1 and 1x7 (every tap but the
centre's row or column is outside), 37x23 (smaller than the footprint from level 3 on) and 130x70 (more than one wave per
row, no multiple of the 64 x 4 block, every level's halo crossing block boundaries); on 37x23 also iterations 1, 5 and
8, every subset of the three guides, KEEP_ALBEDO and other sigmas — the cases of tests/test_denoise_cpu.py.

Bars, on every value (there is no discrete decision in the filter, so no pixel is left out):
  f64 planes: 1e-9 * max(1, max|ref|) — the project's rounding-level bar; only exp differs.
  f32 planes, against the f64 restatement of the float-rounded inputs: 1e-5 * max(1, max|ref|) — the numpy f32
  restatement is 4.5e-7 from it on these inputs; about 20 x that for a device expf that differs from numpy's.
One level fewer moves these results by 9e-3 (test_denoise_cpu.py): a wrong tap, step, weight or level constant is
orders above either bar.  Everything the library is compared with itself on is np.array_equal."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch  # (before the library is loaded: the two share one HIP runtime only in this order)

import denoise_ref
from helpers import GOLD, golden_scene, rmse
from take_amd import capi, scenes
from take_amd import cdefs as D
from test_denoise_cpu import CASES, GUIDES, case_id, check, noisy

pytestmark = pytest.mark.gpu
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED


def subset(p, guides):
    return {k: v for k, v in p.items() if k == "rgb" or k in guides}


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_f64_against_the_restatement(case):
    size, guides, opts = case
    p = subset(denoise_ref.cast(noisy(size), np.float64), guides)
    got = capi.denoise(**p, **opts)
    assert got.dtype == np.float64 and got.shape == p["rgb"].shape
    check(got, denoise_ref.denoise(**p, **opts), 1e-9, "device f64 " + case_id(case))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_f32_against_the_f64_restatement(case):
    size, guides, opts = case
    p = subset(denoise_ref.cast(noisy(size), np.float32), guides)
    got = capi.denoise(**p, **opts)
    assert got.dtype == np.float32
    check(got, denoise_ref.denoise(**{k: v.astype(np.float64) for k, v in p.items()}, **opts), 1e-5, "device f32 " + case_id(case))


def test_texture_detail_survives_on_the_device_in_f32():
    p = denoise_ref.cast(denoise_ref.planes(130, 70), np.float32)
    check(capi.denoise(**p), p["rgb"].astype(np.float64), 1e-5, "texture detail, f32")
    blurred = float(np.abs(capi.denoise(**p, keep_albedo=True) - p["rgb"]).max())
    print(f"KEEP_ALBEDO: {blurred:.3f}")
    assert blurred > 0.1


# ------------------------------------------------------------------ the library against itself
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_repeats_twins_in_place_and_null_options_are_the_same_bits(dtype):
    w, h = 130, 70
    p = denoise_ref.cast(noisy((w, h)), dtype)
    first = capi.denoise(**p)
    assert np.array_equal(first, capi.denoise(**p)), "a repeated call"
    assert np.array_equal(first, capi.denoise(**p, **D.DENOISE_DEFAULTS)), "opts = NULL against the explicit defaults"
    assert np.array_equal(first, capi.denoise(**p, opts=D.TakeDenoiseOpts())), "opts = NULL against all fields 0"
    precision = F32 if dtype == np.float32 else F64
    t = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    out = torch.full_like(t["rgb"], -7.0)
    guides = {g: t[g] for g in GUIDES}
    capi.denoise_device(t["rgb"], w, h, precision, out=out, **guides)
    torch.cuda.synchronize()
    assert np.array_equal(first, out.cpu().numpy()), "host twin against device twin"
    assert np.array_equal(t["rgb"].cpu().numpy(), p["rgb"]), "out of place leaves rgb alone"
    capi.denoise_device(t["rgb"], w, h, precision, **guides)  # out = None: d_out == d_rgb
    torch.cuda.synchronize()
    assert np.array_equal(first, t["rgb"].cpu().numpy()), "in place against out of place"
    assert not np.array_equal(first, capi.denoise(**p, iterations=4))


# ------------------------------------------------------------------ the scene-bound calls
def two_level_scene():
    return scenes.instanced_scene(12, 300, 48, 32, spp=2, max_depth=6)


SCENES = [("cbox", F32), ("cbox", F64), ("mats", F32), ("mats", F64), ("mats", MIXED), ("two-level", F32)]


@pytest.mark.parametrize("name,precision", SCENES, ids=[f"{n}-{p}" for n, p in SCENES])
def test_render_denoised_is_the_three_calls_made_by_hand(name, precision):
    sd = two_level_scene() if name == "two-level" else golden_scene(name)
    spp, depth, seed = 3, 6, 5
    opts = dict(iterations=4, sigma_color=0.8)
    sc = capi.Scene(sd, precision=precision)
    try:
        plain = sc.render(spp=spp, max_depth=depth, seed=seed)
        planes = sc.render_features(spp, seed=seed, want=GUIDES)
        by_hand = capi.denoise(plain, **planes, **opts)
        assert by_hand.dtype == (np.float32 if precision == F32 else np.float64) and not np.array_equal(by_hand, plain)
        buf = torch.zeros(plain.shape, dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 2, depth, seed=seed, restart=True) == 2
        got = sc.render_denoised(spp=spp, max_depth=depth, seed=seed, **opts)
        assert np.array_equal(got, by_hand), "host call"
        assert capi.lib().take_hip_accumulated_samples(sc.h) == 0  # a progressive sequence ends as after render_device
        assert np.array_equal(sc.render(spp=spp, max_depth=depth, seed=seed), plain), "a plain render afterwards"
        sc.render_denoised_device(buf, spp, depth, seed=seed, **opts)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), by_hand), "device call"
        assert np.array_equal(sc.render_denoised(spp=spp, max_depth=depth, seed=seed), capi.denoise(plain, **planes)), "default options"
        # strips are ignored: the whole image
        o = sc._opts(spp, depth, seed, 0.0, 1, 2, 0)
        out = np.zeros_like(plain)
        assert capi.lib().take_hip_render_denoised(sc.h, C.byref(o), C.byref(D.denoise_opts(**opts)), out.ctypes.data) == 0
        assert np.array_equal(out, by_hand), "strips are ignored"
        with pytest.raises(capi.TakeError) as e:
            sc.render_denoised(spp=0, max_depth=depth)
        assert e.value.code == D.TAKE_E_INVALID
    finally:
        sc.close()


# ------------------------------------------------------------------ end to end
def test_a_denoised_4_spp_cornell_box_is_closer_to_its_1024_spp_render():
    """a condition on the default options, not a measurement (the two RMSEs are in DESIGN.md par. 4f)"""
    sd = copy.copy(golden_scene("cbox"))
    sd.width, sd.height = 128, 96
    sc = capi.Scene(sd, precision=F32)
    try:
        truth = sc.render(spp=1024, max_depth=8, seed=11)
        raw = sc.render(spp=4, max_depth=8, seed=3)
        den = sc.render_denoised(spp=4, max_depth=8, seed=3)
    finally:
        sc.close()
    before, after = rmse(raw, truth), rmse(den, truth)
    print(f"cbox 128x96: RMSE to 1024 spp: raw 4 spp {before:.4f}, denoised {after:.4f}")
    assert np.isfinite(den).all() and after < before


# ------------------------------------------------------------------ command line
def test_cli_denoise_writes_denoised_exr_and_leaves_image_exr_alone(tmp_path, monkeypatch):
    from take_amd import render as R
    from take_amd.exr import float_to_half, read_exr

    scene = os.path.join(GOLD, "scenes", "cbox.tkscene")
    files = {}
    for flag in ("without", "with"):
        d = tmp_path / flag
        d.mkdir()
        monkeypatch.chdir(d)
        assert R.main([scene, "-max_depth", "5"] + (["-denoise"] if flag == "with" else [])) == 0
        files[flag] = (d / "image.exr").read_bytes()
    assert files["with"] == files["without"]
    assert not (tmp_path / "without" / "denoised.exr").exists()
    ch, _ = read_exr(str(tmp_path / "with" / "denoised.exr"))
    sd = golden_scene("cbox")
    sc = capi.Scene(sd)
    try:
        want = float_to_half(sc.render_denoised(spp=sd.spp, max_depth=5, seed=0))
    finally:
        sc.close()
    for c, k in (("R", 0), ("G", 1), ("B", 2)):
        assert ch[c].shape == (sd.height, sd.width) and np.array_equal(ch[c].view(np.uint16), want[..., k]), c

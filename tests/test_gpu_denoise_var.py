"""The variance-guided denoiser on the device (take_hip_denoise_variance*, take_hip_render_adaptive_denoised*:
include/take_hip.h; kernels: take_amd/csrc/tk_denoise_var.h) against the numpy restatement of its specification
(tests/denoise_var_ref.py) in f64.

Planes: the sampled ones of denoise_var_ref.sampled_planes at the sizes and option cases of tests/test_denoise_var_cpu.py
(1x1, 7x1, 1x7, 37x23, 130x70 — more than one wave per row, no multiple of the 64 x 4 block; on 37x23 iterations 1 and 8,
every subset of the guides, KEEP_ALBEDO, other sigmas; the variant with a column of single samples and a block of rows
without variance).

Bars, those of tests/test_gpu_denoise.py, on every value of the image: f64 planes 1e-9 * max(1, max|ref|); f32 planes,
against the f64 restatement of the float-rounded inputs, 1e-5 * max(1, max|ref|).  variance_out: the same two bars relative
to max|V_ref|.  Everything the library is compared with itself on is np.array_equal.

Measured on an MI355X (largest differences over the cases): DESIGN.md par. 4h."""
import copy
import os

import numpy as np
import pytest
import torch  # (before the library is loaded: the two share one HIP runtime only in this order)

import denoise_ref
import denoise_var_ref as V
from helpers import GOLD, golden_scene, rmse
from take_amd import capi, scenes
from take_amd import cdefs as D
from test_denoise_var_cpu import GUIDES, STATS, VAR_CASES, check, sampled, subset, var_case_id, widen

pytestmark = pytest.mark.gpu
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
DEPTH, SEED = 6, 5
MIN, STEP, SPP = 4, 3, 13
RULE = dict(min_spp=MIN, step_spp=STEP, max_depth=DEPTH, seed=SEED)


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("vc", VAR_CASES, ids=var_case_id)
def test_f64_against_the_restatement(vc):
    (size, guides, opts), variant = vc
    p = subset(V.cast(sampled(size, variant), np.float64), guides)
    got = capi.denoise_variance(**p, variance=True, **opts)
    assert got[0].dtype == np.float64 and got[0].shape == p["rgb"].shape and got[1].dtype == np.float64 and got[1].shape == p["count"].shape
    check(got, V.denoise_variance(**p, variance=True, **opts), 1e-9, "device f64 " + var_case_id(vc))


@pytest.mark.parametrize("vc", VAR_CASES, ids=var_case_id)
def test_f32_against_the_f64_restatement(vc):
    (size, guides, opts), variant = vc
    p = subset(V.cast(sampled(size, variant), np.float32), guides)
    got = capi.denoise_variance(**p, variance=True, **opts)
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    check(got, V.denoise_variance(**widen(p), variance=True, **opts), 1e-5, "device f32 " + var_case_id(vc))


@pytest.mark.parametrize("size", [(37, 23), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_low_noise_edge_is_cleaned_on_the_device_in_f32(size):
    e = V.edge_planes(*size)
    p = V.cast(e, np.float32)
    raw = rmse(p["rgb"], e["clean"])
    new = rmse(capi.denoise_variance(**p), e["clean"])
    old = rmse(capi.denoise(p["rgb"]), e["clean"])
    print(f"step plane {size}, f32 on the device: RMSE to clean: raw {raw:.5f}, variance-guided {new:.5f} (raw / {raw / new:.1f}), fixed filter {old:.5f} ({old / raw:.1f} x raw)")
    assert new < raw / 4 and old > 2 * raw


# ------------------------------------------------------------------ the library against itself
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_repeats_twins_in_place_null_options_and_the_variance_plane_are_the_same_bits(dtype):
    w, h = 130, 70
    p = V.cast(sampled((w, h), True), dtype)
    first, var = capi.denoise_variance(**p, variance=True)
    again, var_again = capi.denoise_variance(**p, variance=True)
    assert np.array_equal(first, again) and np.array_equal(var, var_again), "a repeated call"
    assert np.array_equal(first, capi.denoise_variance(**p)), "the image with and without variance_out"
    for label, kw in (("opts = NULL against the explicit defaults", D.DENOISE_VARIANCE_DEFAULTS), ("opts = NULL against all fields 0", dict(opts=D.TakeDenoiseOpts()))):
        a, va = capi.denoise_variance(**p, variance=True, **kw)
        assert np.array_equal(first, a) and np.array_equal(var, va), label
    assert not np.array_equal(first, capi.denoise_variance(**p, sigma_color=D.DENOISE_DEFAULTS["sigma_color"]))  # (the fixed filter's default is not this one's)
    precision = F32 if dtype == np.float32 else F64
    t = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    out, vout = torch.full_like(t["rgb"], -7.0), torch.full_like(t["depth"], -7.0)
    planes = {k: t[k] for k in GUIDES + STATS}
    capi.denoise_variance_device(t["rgb"], width=w, height=h, precision=precision, out=out, variance=vout, **planes)
    torch.cuda.synchronize()
    assert np.array_equal(first, out.cpu().numpy()) and np.array_equal(var, vout.cpu().numpy()), "host twin against device twin"
    assert np.array_equal(t["rgb"].cpu().numpy(), p["rgb"]), "out of place leaves rgb alone"
    capi.denoise_variance_device(t["rgb"], width=w, height=h, precision=precision, **planes)  # out = None: d_out == d_rgb, no variance plane
    torch.cuda.synchronize()
    assert np.array_equal(first, t["rgb"].cpu().numpy()), "in place against out of place"
    assert not np.array_equal(first, capi.denoise_variance(**p, iterations=4))


# ------------------------------------------------------------------ the scene-bound calls
def two_level_scene():
    return scenes.instanced_scene(12, 300, 48, 32, spp=2, max_depth=DEPTH)


def calibrate(sc):
    """as tests/test_gpu_adaptive.py: the median of err after min_spp samples, from the planes of a run with spp = min_spp"""
    _, st = sc.render_adaptive(spp=MIN, stats=True, **RULE)
    assert (st["count"] == MIN).all()
    mean = st["m1"] / MIN
    v = np.maximum(st["m2"] / MIN - mean * mean, 0.0)
    return float(np.median(np.sqrt(v / (MIN - 1)) / (np.abs(mean) + D.ADAPTIVE_DEFAULTS["floor"])))


SCENES = [("cbox", F32), ("cbox", F64), ("mats", F32), ("mats", F64), ("mats", MIXED), ("two-level", F32)]


@pytest.mark.parametrize("name,precision", SCENES, ids=[f"{n}-{p}" for n, p in SCENES])
def test_render_adaptive_denoised_is_the_three_calls_made_by_hand(name, precision):
    sd = two_level_scene() if name == "two-level" else golden_scene(name)
    opts = dict(iterations=4, sigma_color=3.0)
    dtype = np.float32 if precision == F32 else np.float64
    sc = capi.Scene(sd, precision=precision)
    try:
        thr = calibrate(sc)
        plain = sc.render(spp=3, max_depth=DEPTH, seed=SEED)
        adaptive, st = sc.render_adaptive(spp=SPP, threshold=thr, stats=True, **RULE)
        assert len(np.unique(st["count"])) >= 2, "the threshold leaves pixels at several counts"
        planes = sc.render_features(MIN, seed=SEED, want=GUIDES)
        by_hand, var_by_hand = capi.denoise_variance(adaptive, **st, **planes, variance=True, **opts)
        assert by_hand.dtype == dtype and var_by_hand.dtype == dtype and not np.array_equal(by_hand, adaptive)
        tdtype = torch.float32 if precision == F32 else torch.float64
        buf = torch.zeros(plain.shape, dtype=tdtype, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED, restart=True) == 2
        got, got_st, got_var = sc.render_adaptive_denoised(spp=SPP, threshold=thr, stats=True, variance=True, **RULE, **opts)
        assert np.array_equal(got, by_hand) and np.array_equal(got_var, var_by_hand), "host call"
        for k in STATS:
            assert got_st[k].dtype == st[k].dtype and np.array_equal(got_st[k], st[k]), k
        assert capi.lib().take_hip_accumulated_samples(sc.h) == 0  # a progressive sequence has ended
        assert np.array_equal(sc.render(spp=3, max_depth=DEPTH, seed=SEED), plain), "a plain render afterwards"
        again, st_again = sc.render_adaptive(spp=SPP, threshold=thr, stats=True, **RULE)
        assert np.array_equal(again, adaptive) and all(np.array_equal(st_again[k], st[k]) for k in STATS), "render_adaptive alone afterwards"
        # no optional output asked for: the statistics planes are the handle's own
        assert np.array_equal(sc.render_adaptive_denoised(spp=SPP, threshold=thr, **RULE, **opts), by_hand), "without the optional outputs"
        d_st = {"count": torch.zeros(plain.shape[:2], dtype=torch.int32, device="cuda"), "m2": torch.zeros(plain.shape[:2], dtype=torch.float64, device="cuda")}
        d_var = torch.zeros(plain.shape[:2], dtype=tdtype, device="cuda")
        sc.render_adaptive_denoised_device(buf, SPP, threshold=thr, stats=d_st, variance=d_var, **RULE, **opts)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), by_hand) and np.array_equal(d_var.cpu().numpy(), var_by_hand), "device call"
        assert np.array_equal(d_st["count"].cpu().numpy(), st["count"]) and np.array_equal(d_st["m2"].cpu().numpy(), st["m2"]), "device call, a subset of the planes"
        assert np.array_equal(sc.render_adaptive_denoised(spp=SPP, threshold=thr, **RULE), capi.denoise_variance(adaptive, **st, **planes)), "default options"
        if name == "cbox":  # the device's image held to the restatement applied to the device's own planes
            ref = V.denoise_variance(**widen(dict(planes, rgb=adaptive, **st)), variance=True, **opts)
            check((by_hand, var_by_hand), ref, 1e-5 if precision == F32 else 1e-9, f"{name}-{precision} against the restatement")
        with pytest.raises(capi.TakeError) as e:
            sc.render_adaptive_denoised(spp=0, max_depth=DEPTH)
        assert e.value.code == D.TAKE_E_INVALID
    finally:
        sc.close()


# ------------------------------------------------------------------ end to end
def test_a_variance_guided_8_spp_cornell_box_is_closer_to_its_1024_spp_render():
    """the one condition the default options are held to, not a measurement (the three RMSEs are in DESIGN.md par. 4h);
    spp = min_spp = 8, so every count is 8 and the raw image is render(spp=8)"""
    sd = copy.copy(golden_scene("cbox"))
    sd.width, sd.height = 128, 96
    sc = capi.Scene(sd, precision=F32)
    try:
        truth = sc.render(spp=1024, max_depth=8, seed=11)
        raw, st = sc.render_adaptive(spp=8, min_spp=8, max_depth=8, seed=3, stats=True)
        new = sc.render_adaptive_denoised(spp=8, min_spp=8, max_depth=8, seed=3)
        old = sc.render_denoised(spp=8, max_depth=8, seed=3)
    finally:
        sc.close()
    assert (st["count"] == 8).all()
    before, after, fixed = rmse(raw, truth), rmse(new, truth), rmse(old, truth)
    print(f"cbox 128x96: RMSE to 1024 spp: raw 8 spp {before:.4f}, variance-guided {after:.4f}, fixed-sigma filter {fixed:.4f} (not asserted)")
    assert np.isfinite(new).all() and after < before


# ------------------------------------------------------------------ command line
def test_cli_both_flags_write_adaptive_denoised_exr_and_leave_the_other_files_alone(tmp_path, monkeypatch):
    from take_amd import render as R
    from take_amd.exr import float_to_half, read_exr

    scene = os.path.join(GOLD, "scenes", "cbox.tkscene")
    runs = {"none": [], "adaptive": ["-adaptive", "0.2"], "denoise": ["-denoise"], "both": ["-adaptive", "0.2", "-denoise"]}
    files = {}
    for name, flags in runs.items():
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        assert R.main([scene, "-max_depth", "5"] + flags) == 0
        files[name] = {f: (d / f).read_bytes() for f in os.listdir(d)}
    assert set(files["none"]) == {"image.exr"} and set(files["adaptive"]) == {"image.exr", "adaptive.exr"} and set(files["denoise"]) == {"image.exr", "denoised.exr"}
    assert set(files["both"]) == {"image.exr", "adaptive.exr", "denoised.exr", "adaptive_denoised.exr"}
    assert files["both"]["image.exr"] == files["none"]["image.exr"] == files["adaptive"]["image.exr"] == files["denoise"]["image.exr"]
    assert files["both"]["adaptive.exr"] == files["adaptive"]["adaptive.exr"] and files["both"]["denoised.exr"] == files["denoise"]["denoised.exr"]
    ch, _ = read_exr(str(tmp_path / "both" / "adaptive_denoised.exr"))
    sd = golden_scene("cbox")
    sc = capi.Scene(sd)
    try:
        want = float_to_half(sc.render_adaptive_denoised(spp=sd.spp, max_depth=5, seed=0, threshold=0.2))
    finally:
        sc.close()
    for c, k in (("R", 0), ("G", 1), ("B", 2)):
        assert ch[c].shape == (sd.height, sd.width) and np.array_equal(ch[c].view(np.uint16), want[..., k]), c

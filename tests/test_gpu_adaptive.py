"""Adaptive sampling on the device (take_hip_render_adaptive*: include/take_hip.h; kernels: take_amd/csrc/tk_adaptive.h;
driver: tk_render.hip).  The main pin is an equality, not a tolerance: a pixel that received c samples is that pixel of
render(spp = c), np.array_equal — so the feature is held to code that is itself held to the reference.  The stopping
decisions are replayed from the returned planes by the numpy restatement (tests/adaptive_ref.py) and must give the
count map exactly.

Options of the pins: min_spp 4, step_spp 3, spp 13 — counts in {4, 7, 10, 13}, the last pass short.  The threshold is
calibrated by each test itself: the median over the pixels of err after min_spp samples.  The same rule run on the CPU
over the per-sample values of hostsim's f64 renders gives the shares 4 / 7 / 10 / 13: cbox 0.50 / 0.13 / 0.05 / 0.32,
mats 0.50 / 0.25 / 0.12 / 0.13, the two-level scene 0.50 / 0.25 / 0.11 / 0.15, the 2000-triangle soup 0.50 / 0.23 /
0.12 / 0.16 — the condition below (three of the four counts on >= 2 % of the pixels each) has room.

Bars of the two moment comparisons that are not equalities (test_the_moments...): what the numpy restatement alone
loses when the same formulas are evaluated on samples of the same size run through it, times 4.  Measured on the
device (largest differences / bars, relative to the largest moment): see DESIGN.md par. 4g."""
import os

import numpy as np
import pytest
import torch  # (before the library is loaded: the two share one HIP runtime only in this order)

import adaptive_ref as A
from helpers import GOLD, golden_scene
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import SceneData

pytestmark = pytest.mark.gpu
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
DEPTH, SEED = 6, 5
MIN, STEP, SPP = 4, 3, 13
SCHEDULE = A.schedule(SPP, MIN, STEP)
FLOOR = A.DEFAULTS["floor"]
RULE = dict(min_spp=MIN, step_spp=STEP, max_depth=DEPTH, seed=SEED)


def two_level_scene():
    return scenes.instanced_scene(12, 300, 48, 32, spp=2, max_depth=DEPTH)


def open_scene(width=48, height=32):
    """the lit box seen from far through a wide lens, in front of a constant sky: most camera rays reach nothing"""
    sd = SceneData(width=width, height=height, lookfrom=(0.0, 0.0, 3.9), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0),
                   vfov=scenes.vfov_from_xfov(100.0, width, height), background=(0.2, 0.3, 0.4), spp=2, max_depth=DEPTH)
    white = sd.add_material(D.MAT_DIFFUSE, (0.73, 0.73, 0.73))
    scenes.box_with_light(sd, white, sd.add_material(D.MAT_DIFFUSE, (0.65, 0.05, 0.05)), sd.add_material(D.MAT_DIFFUSE, (0.12, 0.45, 0.15)))
    pos, idx = scenes.soup_triangles(200, 7, 0.8, 0.05)
    sd.add_mesh(pos, idx, white)
    return sd


def calibrate(sc, **kw):
    """the median of err after min_spp samples, from the planes of a run with spp = min_spp"""
    _, st = sc.render_adaptive(spp=MIN, stats=True, **RULE, **kw)
    assert (st["count"] == MIN).all()
    err = A.rel_error(MIN, st["m1"], st["m2"], FLOOR)
    return float(np.median(err))


def check_counts_are_renders(sc, img, count, schedule=SCHEDULE, **kw):
    """the pixels with count c are those pixels of render(spp = c), bit for bit -> the share of each count"""
    assert set(np.unique(count).tolist()) <= set(schedule)
    share = {}
    for c in schedule:
        at = count == c
        share[c] = float(at.mean())
        if at.any():
            ref = sc.render(spp=c, max_depth=DEPTH, seed=SEED, **kw)
            assert ref.dtype == img.dtype and np.array_equal(img[at], ref[at]), f"pixels that stopped at {c} samples"
    return share


def per_count_identity(sd, precision, **scene_kw):
    sc = capi.Scene(sd, precision=precision, **scene_kw)
    try:
        thr = calibrate(sc)
        img, st = sc.render_adaptive(spp=SPP, threshold=thr, stats=True, **RULE)
        share = check_counts_are_renders(sc, img, st["count"])
        print(f"threshold {thr:.4f}; share of the pixels per count: " + ", ".join(f"{c}: {s:.3f}" for c, s in share.items()))
        assert sum(s >= 0.02 for s in share.values()) >= 3, share
    finally:
        sc.close()


# ------------------------------------------------------------------ 1. per-count identity
CASES = [(n, p) for n in ("cbox", "mats") for p in (F32, F64, MIXED)]


@pytest.mark.parametrize("name,precision", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_a_pixel_with_count_c_is_that_pixel_of_the_c_spp_render(name, precision):
    per_count_identity(golden_scene(name), precision)


# ------------------------------------------------------------------ 2. the decisions, replayed
@pytest.mark.parametrize("name,precision", [("cbox", F32), ("mats", MIXED)], ids=["cbox-f32", "mats-mixed"])
def test_the_count_map_is_the_restatement_s_decisions_on_the_planes(name, precision):
    sc = capi.Scene(golden_scene(name), precision=precision)
    try:
        thr = calibrate(sc)
        runs = [sc.render_adaptive(spp=c, threshold=thr, stats=True, **RULE)[1] for c in SCHEDULE]
    finally:
        sc.close()
    final = runs[-1]
    for a in range(len(runs)):  # a pixel that reaches count c in two runs has the same moments there
        for b in range(a + 1, len(runs)):
            both = runs[a]["count"] == runs[b]["count"]
            assert both.any()
            for m in ("m1", "m2"):
                assert np.array_equal(runs[a][m][both], runs[b][m][both]), (SCHEDULE[a], SCHEDULE[b], m)
    want = np.zeros_like(final["count"])
    active = np.ones(want.shape, bool)
    for c, run in zip(SCHEDULE, runs):
        assert (run["count"][active] == c).all()  # run k gave every pixel still active c_k samples (it stops them at spp = c_k)
        err = A.rel_error(c, run["m1"], run["m2"], FLOOR)
        stop = active & A.stops(c, err, SPP, thr)
        want[stop] = c
        active &= ~stop
    assert not active.any()
    assert np.array_equal(final["count"], want)
    print("pixels per count: " + ", ".join(f"{c}: {int((want == c).sum())}" for c in SCHEDULE))


# ------------------------------------------------------------------ 3. the moments
def restatement_loss(samples, dtype):
    """what the two comparisons below lose in the restatement alone: samples (n, pixels, 3) of `dtype` run through the
    sums as the kernels order them -> (step figure, image figure), each relative to the largest moment involved"""
    n = samples.shape[0]
    L = A.sample_value(samples)
    m1s, m2s = [], []
    for k in range(1, n + 1):
        a, b = A.moments(L[:k])
        m1s.append(a), m2s.append(b)
    step = max(float(np.abs((m2s[k] - m2s[k - 1]) - (m1s[k] - m1s[k - 1]) ** 2).max() / m2s[k].max()) for k in range(1, n))
    image = 0.0
    for k in range(1, n + 1):
        s = np.zeros(samples.shape[1:], dtype)
        for j in range(k):
            s = s + samples[j]
        img = s * (dtype(1) / dtype(k))
        image = max(image, float(np.abs(m1s[k - 1] - k * A.sample_value(img)).max() / np.abs(m1s[k - 1]).max()))
    return step, image


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
def test_the_moments_are_the_sums_of_the_samples_the_image_takes(precision):
    N = 5
    sc = capi.Scene(golden_scene("cbox"), precision=precision)
    try:
        one = sc.render(spp=1, max_depth=DEPTH, seed=SEED)
        kw = dict(min_spp=1, step_spp=1, threshold=0.0, max_depth=DEPTH, seed=SEED, stats=True)
        walk = [sc.render_adaptive(spp=n, **kw) for n in range(1, N + 1)]  # (zero-variance pixels stop at 2: masked out below)
        full = [sc.render_adaptive(spp=n, min_spp=n, max_depth=DEPTH, seed=SEED, stats=True) for n in range(1, N + 1)]
        plain = [sc.render(spp=n, max_depth=DEPTH, seed=SEED) for n in range(1, N + 1)]
    finally:
        sc.close()
    img1, st1 = walk[0]
    assert np.array_equal(img1, one) and (st1["count"] == 1).all()
    assert np.array_equal(st1["m1"], A.sample_value(one)) and np.array_equal(st1["m2"], st1["m1"] * st1["m1"])
    # pseudo-samples of the data's size for the restatement's own loss: the differences of the images' sums
    dtype = one.dtype.type
    sums = [np.zeros_like(one, np.float64)] + [p.astype(np.float64) * (k + 1) for k, p in enumerate(plain)]
    samples = np.stack([np.maximum(sums[k + 1] - sums[k], 0.0).astype(dtype) for k in range(N)]).reshape(N, -1, 3)
    loss_step, loss_image = restatement_loss(samples, dtype)
    bar_step, bar_image = 4 * loss_step, 4 * loss_image
    worst_step = worst_image = 0.0
    for k in range(1, N):
        (_, a), (_, b) = walk[k - 1], walk[k]
        at = (a["count"] == k) & (b["count"] == k + 1)
        assert at.mean() > 0.25
        d = (b["m2"][at] - a["m2"][at]) - (b["m1"][at] - a["m1"][at]) ** 2
        worst_step = max(worst_step, float(np.abs(d).max() / b["m2"][at].max()))
    for n, ((img, st), ref) in enumerate(zip(full, plain), 1):
        assert (st["count"] == n).all() and np.array_equal(img, ref)
        worst_image = max(worst_image, float(np.abs(st["m1"] - n * A.sample_value(img)).max() / np.abs(st["m1"]).max()))
    print(f"m2 steps against squared m1 steps: {worst_step:.3e} (bar {bar_step:.3e}); m1 against n * the image's value: {worst_image:.3e} (bar {bar_image:.3e})")
    assert bar_step > 0 and bar_image > 0
    assert worst_step <= bar_step and worst_image <= bar_image


# ------------------------------------------------------------------ 4. where it stops
def test_pixels_no_camera_ray_reaches_stop_at_min_spp():
    sc = capi.Scene(open_scene(), precision=F32)
    try:
        alpha = sc.render_features(SPP, seed=SEED, want=("alpha",))["alpha"]
        img, st = sc.render_adaptive(spp=SPP, stats=True, **RULE)  # (the default threshold)
        unreached = alpha == 0
        print(f"pixels no camera ray reaches: {unreached.mean():.3f}; per count: " + ", ".join(f"{c}: {int((st['count'] == c).sum())}" for c in SCHEDULE))
        assert unreached.mean() >= 0.05
        assert (st["count"][unreached] == MIN).all() and (st["count"] == SPP).any()
        check_counts_are_renders(sc, img, st["count"])
        huge, hs = sc.render_adaptive(spp=SPP, threshold=1e30, stats=True, **RULE)
        assert (hs["count"] == MIN).all() and np.array_equal(huge, sc.render(spp=MIN, max_depth=DEPTH, seed=SEED))
        whole, ws = sc.render_adaptive(spp=SPP, min_spp=SPP, step_spp=STEP, max_depth=DEPTH, seed=SEED, stats=True)
        assert (ws["count"] == SPP).all() and np.array_equal(whole, sc.render(spp=SPP, max_depth=DEPTH, seed=SEED))
    finally:
        sc.close()


# ------------------------------------------------------------------ 5. invariance
def same(a, b):
    return np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in ("count", "m1", "m2"))


@pytest.mark.parametrize("precision", [F32, MIXED], ids=["f32", "mixed"])
def test_image_counts_and_moments_do_not_depend_on_how_the_call_is_made(precision):
    sd = golden_scene("mats")
    sc = capi.Scene(sd, precision=precision)
    try:
        before = sc.render(spp=3, max_depth=DEPTH, seed=SEED)
        kw = dict(spp=SPP, threshold=0.3, stats=True, **RULE)
        first = sc.render_adaptive(**kw)
        assert len(np.unique(first[1]["count"])) >= 3
        assert sc.counters()["samples"] == int(first[1]["count"].sum())
        assert same(first, sc.render_adaptive(**kw)), "a repeated call"
        for spb in (1, 2):
            assert same(first, sc.render_adaptive(samples_per_batch=spb, **kw)), f"samples_per_batch {spb}"
        whole = (np.zeros_like(first[0]), {k: np.zeros_like(v) for k, v in first[1].items()})
        for k in range(3):
            part = sc.render_adaptive(strip_first=k, strip_stride=3, **kw)
            rows = sc.rows(k, 3)
            assert sc.counters()["samples"] == int(part[1]["count"].sum())
            whole[0][rows] = part[0]
            for name in whole[1]:
                whole[1][name][rows] = part[1][name]
        assert same(first, whole), "strips re-assembled"
        h, w = first[1]["count"].shape
        buf = torch.full((h, w, 3), -7.0, dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        planes = {"count": torch.zeros((h, w), dtype=torch.int32, device="cuda"), "m1": torch.zeros((h, w), dtype=torch.float64, device="cuda"),
                  "m2": torch.zeros((h, w), dtype=torch.float64, device="cuda")}
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED, restart=True) == 2
        sc.render_adaptive_device(buf, SPP, DEPTH, seed=SEED, min_spp=MIN, step_spp=STEP, threshold=0.3, stats=planes)
        torch.cuda.synchronize()
        assert capi.lib().take_hip_accumulated_samples(sc.h) == 0  # a progressive sequence ends as after render_device
        assert same(first, (buf.cpu().numpy(), {k: v.cpu().numpy() for k, v in planes.items()})), "host twin against device twin"
        sc.render_adaptive_device(buf, SPP, DEPTH, seed=SEED, min_spp=MIN, step_spp=STEP, threshold=0.3)  # no planes wanted
        torch.cuda.synchronize()
        assert np.array_equal(first[0], buf.cpu().numpy())
        defaults = sc.render_adaptive(spp=16, max_depth=DEPTH, seed=SEED, stats=True, opts=None)
        assert same(defaults, sc.render_adaptive(spp=16, max_depth=DEPTH, seed=SEED, stats=True, **A.DEFAULTS)), "opts = NULL against the explicit defaults"
        assert same(defaults, sc.render_adaptive(spp=16, max_depth=DEPTH, seed=SEED, stats=True, opts=D.adaptive_opts())), "against all fields at their 'default' values"
        assert np.array_equal(before, sc.render(spp=3, max_depth=DEPTH, seed=SEED)), "a plain render afterwards"
    finally:
        sc.close()


# ------------------------------------------------------------------ 6. other scene kinds
def test_per_count_identity_on_a_two_level_scene():
    per_count_identity(two_level_scene(), F32)


def test_per_count_identity_on_a_device_built_scene():
    sd = scenes.soup_scene(2000, 48, 32, 2, max_depth=DEPTH)
    sc = capi.Scene(sd, precision=MIXED, builder=D.TAKE_BUILDER_DEVICE_LBVH)
    try:
        assert sc.build_info() == {"f32": D.TAKE_BUILDER_DEVICE_LBVH, "f64": D.TAKE_BUILDER_DEVICE_LBVH}
    finally:
        sc.close()
    per_count_identity(sd, MIXED, builder=D.TAKE_BUILDER_DEVICE_LBVH)


# ------------------------------------------------------------------ 7. sizes
@pytest.mark.parametrize("size", [(1, 1), (7, 1), (1, 7), (37, 23), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_across_wave_and_block_boundaries(size):
    """n_active crosses wave and block boundaries in both directions: 130 x 70 = 9100 pixels shrink through several
    blocks' worth, 37 x 23 = 851 through waves', the smallest lists are shorter than a wave from the start"""
    w, h = size
    sc = capi.Scene(scenes.soup_scene(500, w, h, 2, max_depth=DEPTH), precision=F32)
    try:
        img, st = sc.render_adaptive(spp=SPP, threshold=0.25, stats=True, **RULE)
        assert img.shape == (h, w, 3) and st["count"].shape == (h, w)
        assert sc.counters()["samples"] == int(st["count"].sum())  # (before the renders below count their own)
        share = check_counts_are_renders(sc, img, st["count"])
        print(f"{w}x{h}: pixels per count " + ", ".join(f"{c}: {int(round(s * w * h))}" for c, s in share.items()))
        if w * h > 64:
            assert sum(s > 0 for s in share.values()) >= 3
    finally:
        sc.close()


# ------------------------------------------------------------------ 8. refusals that need the scene
def test_the_other_integrators_are_refused():
    sc = capi.Scene(golden_scene("cbox"), precision=F32)
    try:
        for integrator in (1, 2, 3):
            with pytest.raises(capi.TakeError) as e:
                sc.render_adaptive(spp=SPP, integrator=integrator, **RULE)
            assert e.value.code == D.TAKE_E_INVALID and "integrator" in str(e.value)
        with pytest.raises(capi.TakeError) as e:
            sc.render_adaptive(spp=0, **RULE)
        assert e.value.code == D.TAKE_E_INVALID and "spp must be positive" in str(e.value)
    finally:
        sc.close()


# ------------------------------------------------------------------ command line
def test_cli_adaptive_writes_adaptive_exr_and_leaves_image_exr_alone(tmp_path, monkeypatch, capsys):
    from take_amd import render as R
    from take_amd.exr import float_to_half, read_exr

    scene = os.path.join(GOLD, "scenes", "cbox.tkscene")
    files = {}
    for name, flags in (("without", []), ("with", ["-adaptive", "0.2"]), ("default", ["-adaptive"])):
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        assert R.main([scene] + flags + ["-max_depth", "5"]) == 0
        files[name] = (d / "image.exr").read_bytes()
    assert files["with"] == files["without"] == files["default"]
    assert not (tmp_path / "without" / "adaptive.exr").exists() and (tmp_path / "default" / "adaptive.exr").exists()
    sd = golden_scene("cbox")  # (8 spp: below the default min_spp, so every pixel gets them all unless min_spp is given)
    sc = capi.Scene(sd)
    try:
        img, st = sc.render_adaptive(spp=sd.spp, max_depth=5, seed=0, threshold=0.2, stats=True)
    finally:
        sc.close()
    ch, _ = read_exr(str(tmp_path / "with" / "adaptive.exr"))
    want = float_to_half(img)
    for c, k in (("R", 0), ("G", 1), ("B", 2)):
        assert ch[c].shape == (sd.height, sd.width) and np.array_equal(ch[c].view(np.uint16), want[..., k]), c
    total = sd.width * sd.height * sd.spp
    assert f"adaptive: {int(st['count'].sum())} of {total} samples" in capsys.readouterr().out

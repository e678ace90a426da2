"""The thin-lens camera on the device (take_hip_scene_set_lens, _get_lens, _focus_distance_at: include/take_hip.h; the
lens ray: take_amd/csrc/tk_lens.h, made by the generate pass — k_generate_lens, k_generate_list_lens —; DESIGN.md par. 4k).

Bars.  A scene that never had a lens, one with radius 0 and one whose lens was set and cleared: np.array_equal.  Feature
planes against the oracle (lens rays from tests/lens_ref.py, hits from OracleScene.isect, summed in sample order):
tests/test_gpu_features.py's own — f64: ids equal on every pixel and every Real plane within 1e-9 on >= 99.5 % of the
pixels; f32: >= 99 % of the pixels within 1e-3, ids equal on >= 99 % (tests/test_lens_cpu.py shows the reference alone
flips no pixel for this radius and seed).  Everything the library is compared with itself on is np.array_equal.  The
blur test's sets and its 64 samples: see there."""
import copy
import math
import os

import numpy as np
import pytest

import lens_ref as L
import oracle
from helpers import HERE, golden_scene
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import SceneData
from test_gpu_features import IDS, REAL, SEED, SPP, placed_scene, rounding_level, same_planes, share_within
from test_lens_cpu import GPU_RADIUS, GPU_SEED, GPU_SPP

pytestmark = pytest.mark.gpu
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
ROOT = os.path.dirname(HERE)
assert (GPU_SPP, GPU_SEED) == (SPP, SEED) == (4, 5)


def look_distance(a, b):
    """|lookat - lookfrom| as the library sums it"""
    x, y, z = (float(q) - float(p) for p, q in zip(a, b))
    return math.sqrt(x * x + y * y + z * z)


def all_three(sc, spp=3, max_depth=4, seed=SEED):
    """render, render_features and render_adaptive of the scene as it is"""
    img, stats = sc.render_adaptive(spp=8, max_depth=max_depth, seed=seed, min_spp=4, step_spp=2, threshold=0.05, stats=True)
    return {"render": sc.render(spp=spp, max_depth=max_depth, seed=seed), "adaptive": img, "count": stats["count"], **sc.render_features(SPP, seed=seed)}


# ------------------------------------------------------------------ 1. radius 0 is the pinhole camera
@pytest.mark.parametrize("levels", ["one-level", "two-level"])
@pytest.mark.parametrize("precision", [F32, F64, MIXED])
def test_never_set_radius_zero_and_set_then_cleared_are_the_same_scene(precision, levels):
    sd = golden_scene("cbox") if levels == "one-level" else placed_scene()
    sc = capi.Scene(sd, precision=precision)
    try:
        assert sc.get_lens() == {"aperture_radius": 0.0, "focus_distance": 0.0}
        never = all_three(sc)
        sc.set_lens(0.0, 2.0)
        assert sc.get_lens() == {"aperture_radius": 0.0, "focus_distance": 2.0}
        same_planes(never, all_three(sc), "radius 0")
        sc.set_lens(GPU_RADIUS)
        look = look_distance(sd.lookfrom, sd.lookat)
        assert sc.get_lens() == {"aperture_radius": GPU_RADIUS, "focus_distance": look}
        lens = all_three(sc)
        for n in ("render", "adaptive", "depth", "normal"):
            assert not np.array_equal(lens[n], never[n]), n
        sc.set_lens(0.0)
        same_planes(never, all_three(sc), "set, then cleared")
    finally:
        sc.close()


# ------------------------------------------------------------------ 2. the feature planes against the oracle
_EXPECTED = {}


def expected_lens_planes(name):
    """computed once per scene, shared by the f64 and f32 tests, never written to"""
    if name not in _EXPECTED:
        sd = golden_scene(name)
        rays = L.lens_rays(L.camera(sd, np.float64, GPU_RADIUS, 0.0), SPP, SEED, np.float64)
        _EXPECTED[name] = L.oracle_planes(sd, L.rays8(rays["o"], rays["d"], 1e-7), SPP, SEED)
    return _EXPECTED[name]


def lens_features(sd, precision, **kw):
    sc = capi.Scene(sd, precision=precision)
    try:
        sc.set_lens(GPU_RADIUS)
        return sc.render_features(SPP, seed=SEED, **kw)
    finally:
        sc.close()


@pytest.mark.parametrize("name", ["cbox", "mats"])
def test_f64_planes_against_the_oracle(name):
    got = lens_features(golden_scene(name), F64)
    want = expected_lens_planes(name)
    assert (want["shape_id"] >= 0).mean() > 0.5
    rounding_level(got, want, name + " with a lens")


@pytest.mark.parametrize("name", ["cbox", "mats"])
def test_f32_planes_against_the_f64_oracle(name):
    got = lens_features(golden_scene(name), F32)
    want = expected_lens_planes(name)
    for n in REAL:
        share = share_within(got[n], want[n], 1e-3)
        print(f"{name}: {n} within 1e-3 on {100 * share:.3f} % of the pixels")
        assert got[n].dtype == np.float32 and share >= 0.99, (name, n, share)
    for n in IDS:
        share = float((got[n] == want[n]).mean())
        print(f"{name}: {n} equal on {100 * share:.3f} % of the pixels")
        assert got[n].dtype == np.int32 and share >= 0.99, (name, n, share)


# ------------------------------------------------------------------ 3. the lens rays do not depend on how they are asked for
@pytest.mark.parametrize("precision", [F32, F64])
def test_the_counting_instances_change_nothing(precision):
    sc = capi.Scene(golden_scene("mats"), precision=precision)
    try:
        sc.set_lens(GPU_RADIUS)
        plain = sc.render_features(SPP, seed=SEED)
        sc.set_instrumentation(timing=False, counting=True)
        same_planes(plain, sc.render_features(SPP, seed=SEED, samples_per_batch=3), "counting")
    finally:
        sc.close()


@pytest.mark.parametrize("precision", [F32, MIXED])
def test_batches_strips_and_progressive_calls_change_nothing(precision):
    import torch

    sd = golden_scene("mats")
    sc = capi.Scene(sd, precision=precision)
    try:
        sc.set_lens(GPU_RADIUS)
        image, planes = sc.render(spp=6, max_depth=4, seed=SEED), sc.render_features(6, seed=SEED)
        for spb in (1, 4):
            assert np.array_equal(image, sc.render(spp=6, max_depth=4, seed=SEED, samples_per_batch=spb)), spb
            same_planes(planes, sc.render_features(6, seed=SEED, samples_per_batch=spb), f"samples_per_batch {spb}")
        for first, stride in ((1, 3), (0, 2)):
            rows = sc.rows(first, stride)
            assert np.array_equal(image[rows], sc.render(spp=6, max_depth=4, seed=SEED, strip_first=first, strip_stride=stride, samples_per_batch=4))
            same_planes({n: a[rows] for n, a in planes.items()}, sc.render_features(6, seed=SEED, strip_first=first, strip_stride=stride), f"strips {first} of {stride}")
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 2, 4, seed=SEED, restart=True) == 2
        assert sc.render_accumulate(buf.data_ptr(), 4, 4, seed=SEED) == 6
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), image)
    finally:
        sc.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_an_adaptive_pixel_with_c_samples_is_the_c_sample_render(precision):
    sc = capi.Scene(golden_scene("cbox"), precision=precision)
    try:
        sc.set_lens(GPU_RADIUS)
        img, stats = sc.render_adaptive(spp=8, max_depth=4, seed=SEED, min_spp=4, step_spp=2, threshold=0.2, stats=True)
        counts = np.unique(stats["count"])
        assert len(counts) >= 2 and counts.min() >= 4 and counts.max() <= 8, counts  # listed passes ran
        for c in counts:
            sel = stats["count"] == c
            assert np.array_equal(img[sel], sc.render(spp=int(c), max_depth=4, seed=SEED)[sel]), int(c)
    finally:
        sc.close()


# ------------------------------------------------------------------ 4. the blur has the right size
BLUR_W, BLUR_H, BLUR_SPP = 64, 16, 64
BLUR_D, BLUR_A, BLUR_EDGE = 2.0, 0.75, 0.0125  # focus distance, aperture radius, x of the edge


def edge_scene(z):
    """a black quad (x < BLUR_EDGE) and a white one meeting in a vertical edge, perpendicular to the view axis at
    distance z, overfilling the view; the viewport is 1 wide at distance 1"""
    sd = SceneData(width=BLUR_W, height=BLUR_H, lookfrom=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0),
                   vfov=math.degrees(2 * math.atan(0.5 * BLUR_H / BLUR_W)), background=(0.5, 0.5, 0.5), spp=BLUR_SPP, max_depth=0)
    black, white = sd.add_material(D.MAT_DIFFUSE, (0.0, 0.0, 0.0)), sd.add_material(D.MAT_DIFFUSE, (1.0, 1.0, 1.0))
    for x0, x1, mat in ((-100.0, BLUR_EDGE, black), (BLUR_EDGE, 100.0, white)):
        pos = np.array([[x0, -100.0, -z], [x1, -100.0, -z], [x1, 100.0, -z], [x0, 100.0, -z]])
        sd.add_mesh(pos, np.array([[0, 1, 2], [0, 2, 3]], np.int32), mat)
    return sd


def column_spans(z):
    """x of the two sides of every pixel column's footprint on the plane at distance z, and of its centre"""
    lo = (np.arange(BLUR_W) / BLUR_W - 0.5) * z
    hi = ((np.arange(BLUR_W) + 1) / BLUR_W - 0.5) * z
    return lo, hi, 0.5 * (lo + hi)


@pytest.mark.parametrize("precision", [F32, F64])
def test_the_blur_circle_has_the_size_the_geometry_gives(precision):
    """At z = D every lens ray of a sample meets the quads where its pinhole ray does: only the column the edge crosses
    mixes the two colours.  At z = 2 D the lens ray through the focus point P lands at 2 P - L (L on the lens): within
    A = A |z - D| / D of the pinhole ray's point.  A pixel whose footprint is farther than A (+ one pixel width) from
    the edge therefore sees one colour — the pinhole plane exactly, 64 equal samples —; one whose centre is nearer than
    A / 2 sees both: the colour of the other side has a share >= 0.2 there, and misses all 64 samples with
    probability 0.8^64 = 6e-7."""
    planes = {}
    for z in (BLUR_D, 2 * BLUR_D):
        sc = capi.Scene(edge_scene(z), precision=precision)
        try:
            pinhole = sc.render_features(BLUR_SPP, seed=SEED, want=("albedo",))["albedo"][..., 0]
            sc.set_lens(BLUR_A, BLUR_D)
            planes[z] = (pinhole, sc.render_features(BLUR_SPP, seed=SEED, want=("albedo",))["albedo"][..., 0])
        finally:
            sc.close()
    mixed = lambda a: (a > 0) & (a < 1)
    # in focus
    pinhole, lens = planes[BLUR_D]
    lo, hi, _ = column_spans(BLUR_D)
    crossed = (lo < BLUR_EDGE) & (BLUR_EDGE < hi)
    assert crossed.sum() == 1
    assert mixed(lens[:, crossed]).all() and not mixed(lens[:, ~crossed]).any()
    assert np.array_equal(lens[:, ~crossed], pinhole[:, ~crossed])
    # out of focus
    pinhole, lens = planes[2 * BLUR_D]
    lo, hi, mid = column_spans(2 * BLUR_D)
    circle, pixel = BLUR_A * abs(2 * BLUR_D - BLUR_D) / BLUR_D, 2 * BLUR_D / BLUR_W
    far = np.minimum(np.abs(lo - BLUR_EDGE), np.abs(hi - BLUR_EDGE)) > circle + pixel
    far &= ~((lo < BLUR_EDGE) & (BLUR_EDGE < hi))
    near = np.abs(mid - BLUR_EDGE) < 0.5 * circle
    assert far.sum() >= 8 and near.sum() >= 8 and (far & (mid < 0)).any() and (far & (mid > 0)).any()
    assert np.array_equal(lens[:, far], pinhole[:, far]) and not mixed(lens[:, far]).any()
    assert mixed(lens[:, near]).all()
    assert mixed(pinhole).any(axis=0).sum() == 1  # (the pinhole camera: sharp at every distance)


# ------------------------------------------------------------------ 5. emission does not depend on the lens in focus
def test_an_emitter_on_the_plane_of_focus_looks_the_same_through_the_lens():
    sd = SceneData(width=48, height=32, lookfrom=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=40.0,
                   background=(0.1, 0.1, 0.1), spp=4, max_depth=0)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.5, 0.5, 0.5))
    pos, idx, nrm, uv = scenes._quad((0.0, 0.0, -BLUR_D), (50.0, 0.0, 0.0), (0.0, 50.0, 0.0), (0.0, 0.0, 1.0))
    sd.add_mesh(pos, idx, grey, normals=nrm, uvs=uv, emission=(3.0, 2.0, 1.0))
    sc = capi.Scene(sd, precision=F64)
    try:
        pinhole = sc.render(spp=4, max_depth=0, seed=SEED)
        sc.set_lens(0.3, BLUR_D)
        lens = sc.render(spp=4, max_depth=0, seed=SEED)
    finally:
        sc.close()
    assert (pinhole >= np.array([3.0, 2.0, 1.0]) - 1e-12).all()
    err = float(np.abs(lens - pinhole).max())
    print(f"the emitter through the lens and through the pinhole: within {err:.3e}")
    assert err <= 1e-9


# ------------------------------------------------------------------ 6. no geometry
@pytest.mark.parametrize("precision", [F32, F64])
def test_without_geometry_the_render_is_the_background(precision):
    sd = SceneData(width=16, height=12, lookfrom=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=30.0,
                   background=(0.3, 0.2, 0.1), spp=2, max_depth=3)
    sd.add_material(D.MAT_DIFFUSE, (0.5, 0.5, 0.5))
    sc = capi.Scene(sd, precision=precision)
    try:
        sc.set_lens(0.2, 1.5)
        img = sc.render(spp=2, max_depth=3, seed=SEED)
        assert np.array_equal(img, np.broadcast_to(np.asarray(sd.background, img.dtype), img.shape))
        assert sc.focus_distance_at(3, 4) == 0.0
    finally:
        sc.close()


# ------------------------------------------------------------------ 7. focus_distance_at
def oracle_focus_distances(sd, pixels):
    """t * -(w . d) of the oracle's hit along the centre ray from lookfrom of every (column, row), 0 for a miss"""
    cam = L.camera(sd, np.float64)
    W, H = sd.width, sd.height
    dirs = []
    for c, r in pixels:
        y = H - 1 - r
        p = (cam["u"] * (((c + 0.5) / W - 0.5) * cam["vw"]) + cam["v"] * (((y + 0.5) / H - 0.5) * cam["vh"])) - cam["w"]
        dirs.append(p / np.sqrt((p * p).sum()))
    dirs = np.array(dirs)
    osc = oracle.OracleScene(sd, 1)
    try:
        hit = osc.isect(L.rays8(np.broadcast_to(cam["lookfrom"], dirs.shape), dirs, 1e-7))
    finally:
        osc.close()
    return np.where(hit[:, 0] != 0, hit[:, 1] * -(dirs @ cam["w"]), 0.0)


def test_focus_distance_at_is_the_oracle_s_hit_along_the_view_axis():
    sd = golden_scene("cbox")
    W, H = sd.width, sd.height
    pixels = [(c, r) for r in (3, H // 3, H // 2, H - 5) for c in (2, W // 3, W // 2 + 1, W - 4)]
    assert len(pixels) == 16
    want = oracle_focus_distances(sd, pixels)
    assert (want > 0).sum() >= 12
    sc = capi.Scene(sd, precision=F64)
    try:
        got = np.array([sc.focus_distance_at(c, r) for c, r in pixels])
        assert float(np.abs(got - want).max()) <= 1e-9
        d = float(got[got > 0][0])
        sc.set_lens(0.02, d)
        assert sc.get_lens() == {"aperture_radius": 0.02, "focus_distance": d}
        assert np.array_equal(got, [sc.focus_distance_at(c, r) for c, r in pixels])  # the pinhole ray, with or without a lens
        for c, r in ((-1, 0), (0, -1), (W, 0), (0, H)):
            with pytest.raises(capi.TakeError) as e:
                sc.focus_distance_at(c, r)
            assert e.value.code == D.TAKE_E_INVALID and "outside" in str(e.value)
    finally:
        sc.close()
    for precision in (F32, MIXED):
        sc = capi.Scene(sd, precision=precision)
        try:
            other = np.array([sc.focus_distance_at(c, r) for c, r in pixels])
            if precision == MIXED:
                assert np.array_equal(other, got)  # its f64 side
            else:
                assert float(np.abs(other - want).max()) <= 1e-3
        finally:
            sc.close()


def test_focus_distance_at_is_zero_on_the_background():
    sd = golden_scene("mats")
    sc = capi.Scene(sd, precision=F64)
    try:
        # pixels none of whose jittered samples hits anything (the scene's background shows in its outermost columns)
        clear = np.argwhere(sc.render_features(SPP, seed=SEED, want=("alpha",))["alpha"] == 0)
        assert len(clear) >= 4
        pixels = [(int(c), int(r)) for r, c in clear[:: len(clear) // 4][:4]]
        assert not oracle_focus_distances(sd, pixels).any()  # the reference's centre rays miss there too
        for c, r in pixels:
            assert sc.focus_distance_at(c, r) == 0.0
    finally:
        sc.close()


# ------------------------------------------------------------------ 8. the refusals that need a scene
@pytest.mark.parametrize("precision", [F32, MIXED])
def test_refusals_leave_the_scene_as_it_was(precision):
    import torch

    sd = golden_scene("cbox")
    sc = capi.Scene(sd, precision=precision)
    try:
        sc.set_lens(GPU_RADIUS, 2.5)
        image = sc.render(spp=2, max_depth=4, seed=3)
        for kw in (dict(aperture_radius=-1.0), dict(aperture_radius=float("nan")), dict(aperture_radius=0.1, focus_distance=float("inf")),
                   dict(aperture_radius=0.1, focus_distance=1e300)):
            with pytest.raises(capi.TakeError) as e:
                sc.set_lens(**kw)
            assert e.value.code == D.TAKE_E_INVALID, kw
        assert sc.get_lens() == {"aperture_radius": GPU_RADIUS, "focus_distance": 2.5}
        assert np.array_equal(image, sc.render(spp=2, max_depth=4, seed=3))
        # an automatic focus and a new lookat that is the lookfrom: the effective focus distance would not be > 0
        sc.set_lens(GPU_RADIUS)
        image = sc.render(spp=2, max_depth=4, seed=3)
        with pytest.raises(capi.TakeError) as e:
            sc.set_camera(sd.lookfrom, sd.lookfrom, sd.up, sd.vfov)
        assert e.value.code == D.TAKE_E_INVALID
        assert sc.get_lens() == {"aperture_radius": GPU_RADIUS, "focus_distance": look_distance(sd.lookfrom, sd.lookat)}
        assert np.array_equal(image, sc.render(spp=2, max_depth=4, seed=3))
        # a progressive sequence has to restart after set_lens
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 2, 4, seed=3, restart=True) == 2
        sc.set_lens(GPU_RADIUS, 2.0)
        assert capi.lib().take_hip_accumulated_samples(sc.h) == 0
        with pytest.raises(capi.TakeError) as e:
            sc.render_accumulate(buf.data_ptr(), 2, 4, seed=3)
        assert e.value.code == D.TAKE_E_INVALID
        assert sc.render_accumulate(buf.data_ptr(), 2, 4, seed=3, restart=True) == 2
        # the camera moves: the lens stays, an automatic focus follows the new lookat
        sc.set_lens(GPU_RADIUS)
        sc.set_camera((0.2, 0.1, 3.0), (0.0, 0.0, 0.5), sd.up, sd.vfov)
        assert sc.get_lens() == {"aperture_radius": GPU_RADIUS, "focus_distance": look_distance((0.2, 0.1, 3.0), (0.0, 0.0, 0.5))}
        sc.set_lens(GPU_RADIUS, 1.25)
        sc.set_camera(sd.lookfrom, sd.lookat, sd.up, sd.vfov)
        assert sc.get_lens() == {"aperture_radius": GPU_RADIUS, "focus_distance": 1.25}
    finally:
        sc.close()


def test_an_effective_focus_that_is_not_positive_is_refused():
    sd = copy.copy(golden_scene("cbox"))
    sd.lookat = sd.lookfrom
    sc = capi.Scene(sd, precision=F64)
    try:
        with pytest.raises(capi.TakeError) as e:
            sc.set_lens(0.1)  # |lookat - lookfrom| = 0
        assert e.value.code == D.TAKE_E_INVALID and "focus distance" in str(e.value)
        sc.set_lens(0.0)   # the pinhole camera needs no focus
        sc.set_lens(0.1, 2.0)
    finally:
        sc.close()

"""The environment-map light against tests/env_ref.py, without a GPU: the reference's own self-checks, and every
kernel-level check of tests/env_checks.py on the device code executed on the host (hostsim_env: host libm).
test_gpu_env.py runs the same checks on the device.

Measured here, hostsim_env against env_ref (f64 / f32, maximum over the maps, the worst map in brackets; also in
DESIGN.md §4b): sampled pdf relative 6.1e-16 (8x1) / 4.4e-7 (wide); sampled direction absolute 7.5e-16 (tall) / 7.0e-7
(wide); round-trip pdf beyond the direction's own rounding 2.5e-16 / 1.4e-7 (tall); pdf of random directions 0 / 2.8e-7
(ragged); normalisation terms 3.7e-16 (wide) / 3.1e-7 (tall), |sum - 1| 1.1e-16 (edges_black) / 1.2e-7 (wide).
Irradiance on a diffuse plane, 8 x 8 at 64 spp, image mean against the closed form in oracle sigmas: sun 1.3, halves 1.1,
sun flipped exactly black, sun tilted 1.4, ragged 2.2 (f64 and f32 alike).
"""
import numpy as np
import pytest

import env_checks as K
import env_irradiance as I
import env_maps
import env_ref
from helpers import hostsim_env, hostsim_render

ALL = list(env_maps.MAPS)
PRECISIONS = [1, 0]


def runner(name, precision):
    sd = env_maps.env_scene(env_maps.image(name), env_maps.SCALES[name])
    return lambda kind, rows: hostsim_env(sd, precision, kind, rows)


# ------------------------------------------------------------------ the reference alone
@pytest.mark.parametrize("name", ALL)
def test_reference_tables_are_cdfs_and_probabilities_sum_to_one(name):
    img = env_maps.image(name)
    for dtype in (np.float64, np.float32):
        marg, cond = env_ref.tables_as(img, dtype)
        assert marg[0] == 0 and marg[-1] == 1 and (cond[:, 0] == 0).all() and (cond[:, -1] == 1).all()
        assert (np.diff(marg) >= 0).all() and (np.diff(cond, axis=1) >= 0).all()
        p = env_ref.texel_prob((marg, cond))
        assert abs(p.sum() - 1.0) < 1e-6 if dtype == np.float32 else abs(p.sum() - 1.0) < 1e-12
        lum = img @ np.array(env_ref.LUM)
        assert (p[lum <= 0][np.diff(marg)[np.nonzero(lum <= 0)[0]] > 0] == 0).all()  # black texels of a lit row: never drawn
    h, w = img.shape[:2]
    assert abs((env_ref.texel_solid_angle(w, h) * w).sum() - 4 * np.pi) < 1e-12


def test_reference_range_map_collapses_positive_texels_in_float32():
    img = env_maps.image("range")
    lum = img @ np.array(env_ref.LUM)
    p64, p32 = env_ref.texel_prob(env_ref.tables(img)), env_ref.texel_prob(env_ref.tables_as(img, np.float32))
    assert (lum > 0).all()
    assert np.count_nonzero(p32 == 0) >= 32  # (1e-12 beside 1e6 is below float64's resolution as well)
    assert np.count_nonzero((p32 == 0) & (p64 > 0)) + np.count_nonzero(p64 == 0) == np.count_nonzero(p32 == 0)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_reference_puts_sample_inputs_inside_their_texels(name, precision):
    c = K.case(name, precision)
    rows, made_for = K.sample_inputs(c)
    x, y, _, _, _, (du, dv) = env_ref.sample(c.tabs, c.texels, c.scale, rows[:, 0], rows[:, 1])
    assert np.array_equal(y * c.w + x, made_for)
    for t in (du, dv):
        assert t.min() >= 0.05 and t.max() <= 0.95
    # the 64-ulp rule leaves out nothing, except in float32 the polar rows of `tall`: under 2 % of its drawable texels
    left_out, drawable = np.count_nonzero((c.prob > 0) & ~K.wide_steps(c)), np.count_nonzero(c.prob > 0)
    assert left_out == 0 or (name == "tall" and precision == 0 and left_out < 0.02 * drawable), left_out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_reference_drops_few_random_directions(name, precision):
    c = K.case(name, precision)
    _, rnd = K.directions(c)
    assert np.count_nonzero(~K.interior(c, rnd)) < 0.02 * rnd.shape[0]


# ------------------------------------------------------------------ the device code on the host against the reference
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_hostsim_samples_and_round_trip(name, precision):
    c, run = K.case(name, precision), runner(name, precision)
    sampled, _, _ = K.check_samples(c, run)
    K.check_round_trip(c, run, sampled)
    K.check_lower_edges(c, run)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_hostsim_directions(name, precision):
    K.check_directions(K.case(name, precision), runner(name, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_hostsim_stratified_histogram(name, precision):
    K.check_histogram(K.case(name, precision), runner(name, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL)
def test_hostsim_normalisation(name, precision):
    K.check_normalisation(K.case(name, precision), runner(name, precision))


@pytest.mark.parametrize("guide", ["1,1", "4,2", "65536,65536"])
@pytest.mark.parametrize("name", ["sun", "ragged", "wide", "tall"])
def test_hostsim_guide_independence(name, guide, monkeypatch):
    for precision in PRECISIONS:
        rows, _ = K.sample_inputs(K.case(name, precision))
        want = runner(name, precision)(0, rows)
        monkeypatch.setenv("TAKE_HIP_ENV_GUIDE", guide)
        got = runner(name, precision)(0, rows)
        monkeypatch.delenv("TAKE_HIP_ENV_GUIDE")
        assert np.array_equal(got, want)


# ------------------------------------------------------------------ render level: an empty scene shows the map
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hostsim_empty_scene_shows_the_map(precision):
    """looking along the centre direction of each texel, every pixel is that texel x scale (test_gpu_env.py: on the GPU)"""
    img, dt = env_maps.colours(), K.DTYPE[precision]
    want = (img.astype(dt) * np.asarray(env_maps.COLOURS_SCALE, dt)).astype(np.float64)
    assert np.unique(want.reshape(-1, 3), axis=0).shape[0] == 32
    for y in range(4):
        for x in range(8):
            sd = env_maps.env_scene(img, env_maps.COLOURS_SCALE)
            sd.lookfrom, sd.lookat, sd.up = env_maps.look_along(env_ref.direction((x + 0.5) / 8, (y + 0.5) / 4))
            got, _ = hostsim_render(sd, precision, 1, 2)
            assert got.shape == (4, 4, 3) and np.array_equal(got.astype(np.float64), np.broadcast_to(want[y, x], (4, 4, 3))), (x, y)


# ------------------------------------------------------------------ render level: irradiance on a diffuse plane
def test_reference_irradiance_midpoint_rule_against_closed_forms():
    """env_ref.irradiance's general branch against what is known in closed form: a constant sky gives pi c for any
    normal; for a normal next to +y it gives the exact per-texel form; and for one lit texel it gives that texel's
    own integral, taken here directly on a fine grid (which pins the per-texel bookkeeping, phi included)"""
    for n in ((1.0, 0.0, 0.0), (0.3, -0.5, 0.8), (0.0, -1.0, 0.0)):
        assert np.allclose(env_ref.irradiance(np.full((6, 11, 3), 0.7), (2.0, 0.5, 1.0), n, k=16), np.pi * 0.7 * np.array([2.0, 0.5, 1.0]), rtol=1e-3, atol=0)
    for name in ("halves", "ragged", "sun"):
        img = env_maps.image(name)
        exact = env_ref.irradiance(img, (1.0, 1.0, 1.0), (0.0, 1.0, 0.0))
        assert np.allclose(env_ref.irradiance(img, (1.0, 1.0, 1.0), (1e-9, 1.0, 0.0), k=32), exact, rtol=1e-3, atol=0)
    (x, y), m = env_maps.SUN_XY, 256
    u, v = np.meshgrid((x + (np.arange(m) + 0.5) / m) / 64, (y + (np.arange(m) + 0.5) / m) / 32)
    d = env_ref.direction(u, v)
    for n in (I.CASES["sun_tilted"][1], (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.2, 0.0)):
        nn = np.asarray(n) / np.linalg.norm(n)
        direct = (np.maximum(0.0, d @ nn) * np.sin(v * np.pi)).sum() * 2.0 * np.pi ** 2 / (64 * 32 * m * m)
        got = env_ref.irradiance(env_maps.image("sun"), (1.0, 1.0, 1.0), n, k=32)
        assert np.allclose(got, direct * np.array([3e3, 2e3, 1e3]), rtol=1e-4, atol=1e-9), n


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(I.CASES))
def test_reference_irradiance_quadrature_error_and_oracle_mean(name, precision):
    """at the size the GPU test renders (24 x 24, 256 spp): the quadrature error of the closed form is under a tenth of
    the oracle's sigma, and the oracle's own 8-seed mean is within 5 sigma / sqrt(8) of the closed form"""
    I.check_reference(I.case(name, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(I.CASES))
def test_hostsim_irradiance_on_a_diffuse_plane(name, precision):
    """the GPU test's check on the device code executed on the host, at 8 x 8 pixels and 64 spp (sigma from the oracle
    at that size)"""
    c = I.case(name, precision, res=8, spp=64)
    I.check_reference(c)
    img, _ = hostsim_render(c.sd, precision, c.spp, 3, seed=7)
    I.check_render(c, img)

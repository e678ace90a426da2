"""The environment-map light on the GPU against tests/env_ref.py (an independent float64 reference): the shade kernel's
own env_sample / env_eval / env_lookup, run row by row on the resident tables and guide tables of a scene
(take_hip_debug_env), on maps chosen to be awkward (tests/env_maps.py).  The checks are those of tests/env_checks.py,
which test_env_cpu.py runs on the same device code executed on the host; the bars are derived there.

Measured on an MI355X against env_ref (f64 / f32, the worst map in brackets), all inside the bars of the number formats
(1e-13 / 2e-6), none widened: sampled pdf relative 6.1e-16 (8x1) / 4.4e-7 (wide); sampled direction absolute 7.5e-16 (tall)
/ 7.0e-7 (wide); round-trip pdf beyond the direction's own rounding 2.5e-16 / 1.3e-7 (tall); pdf of random directions
0 / 2.8e-7 (ragged); normalisation terms 3.7e-16 (wide) / 3.1e-7 (tall), |sum - 1| 1.1e-16 / 1.2e-7.
"""
import numpy as np
import pytest

import env_checks as K
import env_irradiance as I
import env_maps
import env_ref
from take_amd import capi
from take_amd import cdefs as D

pytestmark = pytest.mark.gpu

ALL = list(env_maps.MAPS)
PRECISIONS = [1, 0]
MIXED = ["sun", "halves", "ragged"]
SIDES = [(n, p, False) for n in ALL for p in PRECISIONS] + [(n, p, True) for n in MIXED for p in PRECISIONS]
IDS = [f"{n}-{'mixed-' if m else ''}f{32 * (1 + p)}" for n, p, m in SIDES]


@pytest.fixture(scope="module")
def scenes():
    """name, side precision, mixed -> run(kind, rows) on that side of a resident scene holding the map"""
    made = {}

    def get(name, precision, mixed=False):
        key = (name, D.TAKE_PRECISION_MIXED if mixed else precision)
        if key not in made:
            made[key] = capi.Scene(env_maps.env_scene(env_maps.image(name), env_maps.SCALES[name]), precision=key[1])
        return lambda kind, rows: made[key].debug_env(kind, rows, side=precision)

    yield get
    for sc in made.values():
        sc.close()


@pytest.mark.parametrize("name,precision,mixed", SIDES, ids=IDS)
def test_gpu_samples_and_round_trip(scenes, name, precision, mixed):
    c, run = K.case(name, precision), scenes(name, precision, mixed)
    sampled, _, _ = K.check_samples(c, run)
    K.check_round_trip(c, run, sampled)
    K.check_lower_edges(c, run)


@pytest.mark.parametrize("name,precision,mixed", SIDES, ids=IDS)
def test_gpu_directions(scenes, name, precision, mixed):
    K.check_directions(K.case(name, precision), scenes(name, precision, mixed))


@pytest.mark.parametrize("name,precision,mixed", SIDES, ids=IDS)
def test_gpu_stratified_histogram(scenes, name, precision, mixed):
    K.check_histogram(K.case(name, precision), scenes(name, precision, mixed))


@pytest.mark.parametrize("name,precision,mixed", SIDES, ids=IDS)
def test_gpu_normalisation(scenes, name, precision, mixed):
    K.check_normalisation(K.case(name, precision), scenes(name, precision, mixed))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["sun", "ragged", "wide", "tall"])
def test_gpu_guide_independence(scenes, name, precision, monkeypatch):
    """guide tables of 1, a few and the most entries: the samples are those of the default sizes, bit for bit"""
    rows, _ = K.sample_inputs(K.case(name, precision))
    want = scenes(name, precision)(0, rows)
    for guide in ("1,1", "4,2", "65536,65536"):
        monkeypatch.setenv("TAKE_HIP_ENV_GUIDE", guide)
        sc = capi.Scene(env_maps.env_scene(env_maps.image(name), env_maps.SCALES[name]), precision=precision)
        monkeypatch.delenv("TAKE_HIP_ENV_GUIDE")
        try:
            assert np.array_equal(sc.debug_env(0, rows), want), guide
        finally:
            sc.close()


def test_gpu_debug_env_refuses_what_it_cannot_do():
    from take_amd import scenes as S

    rows = np.full((4, 2), 0.5)
    sc = capi.Scene(env_maps.env_scene(env_maps.image("sun")), precision=D.TAKE_PRECISION_F32)
    plain = capi.Scene(S.soup_scene(50, 8, 8, spp=1))
    try:
        with pytest.raises(capi.TakeError, match="no such side"):
            sc.debug_env(0, rows, side=D.TAKE_PRECISION_F64)
        with pytest.raises(capi.TakeError, match="no environment map"):
            plain.debug_env(0, rows)
        assert capi.lib().take_hip_debug_env(sc.h, 0, 0, None, 4, None) == -1
    finally:
        sc.close()
        plain.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_gpu_empty_scene_shows_the_map(precision):
    """32 renders of one resident scene, the camera turned to the centre of each texel of an 8x4 map of distinct colours:
    all 16 pixels are that texel x scale — exactly in f64, to float rounding in f32"""
    img, dt = env_maps.colours(), K.DTYPE[precision]
    want = (img.astype(dt) * np.asarray(env_maps.COLOURS_SCALE, dt)).astype(np.float64)
    sc = capi.Scene(env_maps.env_scene(img, env_maps.COLOURS_SCALE), precision=precision)
    try:
        for y in range(4):
            for x in range(8):
                sc.set_camera(*env_maps.look_along(env_ref.direction((x + 0.5) / 8, (y + 0.5) / 4)), vfov=2.0)
                got = sc.render(spp=1, max_depth=2, seed=x + 8 * y).astype(np.float64)
                assert got.shape == (4, 4, 3)
                if precision == 1:
                    assert np.array_equal(got, np.broadcast_to(want[y, x], (4, 4, 3))), (x, y)
                else:
                    assert np.abs(got / want[y, x] - 1.0).max() <= 2.0 ** -23, (x, y)
    finally:
        sc.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(I.CASES))
def test_gpu_irradiance_on_a_diffuse_plane(name, precision):
    """a diffuse plane (rho 0.6, normal n) under a map alone, 24 x 24 at 256 spp, max_depth 3: the image mean is within
    5 sigma (+ the quadrature error, < sigma / 10) of rho / pi * env_ref.irradiance(n), sigma = the standard deviation
    of the oracle's image means at 8 seeds; the oracle's own mean is held to 5 sigma / sqrt(8).  Measured sigma (f64 and
    f32 alike to three digits), expectation in brackets: sun, n = +y 1.03e-4 (1.7587); halves, n = +y 6.89e-4 (0.13108);
    sun flipped, n = +y 0 (0: the image is exactly black); sun, n tilted off the sun's direction 2.49e-4 (2.9046);
    ragged, n = +x 6.56e-3 (1.9355)."""
    c = I.case(name, precision)
    I.check_reference(c)
    sc = capi.Scene(c.sd, precision=precision)
    try:
        img = sc.render(spp=c.spp, max_depth=3, seed=7)
    finally:
        sc.close()
    I.check_render(c, img)

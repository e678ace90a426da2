"""Mixed precision (TAKE_PRECISION_MIXED) on the CPU: the device code's mixed render loop executed on the host
(tests/hostsim: rounds k < E on f64 records and the f64 scene, the conversion of the last exact shade round, the rest
on f32 records and the f32 scene, k_accumulate_mixed) against the oracle's restatement of the same split
(oracle/take_oracle.hpp path_tracing_mixed: the reference's path_tracing run in double and finished in float where
the device hands over).  Same libm on both sides: the bar is BIT equality, per sample, on every golden scene.

What these catch that the statistical GPU bars cannot: a handover one round early or late, a record word not moved
(S_FLAGS: the specular weight of the pending sample; S_CTR: the random stream), the last exact shadow contribution
counted twice or lost, an S_CONV flag left over from an earlier batch in the same slot."""
import numpy as np
import pytest

import oracle
from helpers import GOLDEN_SCENES, golden_scene, hostsim_render, mirror_box_scene
from take_amd import scenes
from take_amd.dist import strip_rows


def env_soup():
    return scenes.soup_scene(300, 32, 32, spp=4, envmap=(64, 32))  # the env-map case of test_envmap.py


SCENES = {**{n: golden_scene for n in GOLDEN_SCENES}, "envsoup": lambda n: env_soup(), "mirrorbox": lambda n: mirror_box_scene()}


def oracle_mixed(sd, spp, depth, seed, E, threads=8):
    osc = oracle.OracleScene(sd, precision=oracle.PRECISION_MIXED)
    try:
        return osc.render(spp, depth, rng_mode=oracle.RNG_COUNTER, seed=seed, threads=threads, exact_bounces=E)
    finally:
        osc.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_host_mixed_equals_oracle_mixed(name):
    sd = SCENES[name](name)
    osc = oracle.OracleScene(sd, precision=oracle.PRECISION_MIXED)
    try:
        for depth in (-1, 0, 1, 5, 50):
            rounds = depth + 2
            for E in sorted({1, 2, 3, rounds - 1}):
                if E < 1:
                    continue
                want = osc.render(2, depth, rng_mode=oracle.RNG_COUNTER, seed=11, threads=8, exact_bounces=E)
                got, _ = hostsim_render(sd, 2, 2, depth, seed=11, exact_bounces=E)
                assert got.dtype == np.float64
                assert np.array_equal(got, want), f"{name} depth {depth} E {E}"
    finally:
        osc.close()


@pytest.mark.parametrize("name", ["cbox", "mats", "spherelight", "envsoup"])
def test_all_rounds_exact_is_the_f64_render(name):
    sd = SCENES[name](name)
    for depth in (0, 4):
        rounds = depth + 2
        f64_host, _ = hostsim_render(sd, 1, 2, depth, seed=5)
        osc = oracle.OracleScene(sd, precision=1)
        f64_oracle = osc.render(2, depth, rng_mode=oracle.RNG_COUNTER, seed=5, threads=8)
        osc.close()
        for E in (rounds, rounds + 3):
            got, _ = hostsim_render(sd, 2, 2, depth, seed=5, exact_bounces=E)
            assert np.array_equal(got, f64_host)
            assert np.array_equal(oracle_mixed(sd, 2, depth, 5, E), f64_oracle)


def test_default_exact_bounces_is_three():
    sd = golden_scene("mats")
    want_host, _ = hostsim_render(sd, 2, 2, 8, seed=3, exact_bounces=3)
    want_oracle = oracle_mixed(sd, 2, 8, 3, 3)
    assert np.array_equal(want_host, want_oracle)
    for E in (0, -1, -7):
        got, _ = hostsim_render(sd, 2, 2, 8, seed=3, exact_bounces=E)
        assert np.array_equal(got, want_host)
        assert np.array_equal(oracle_mixed(sd, 2, 8, 3, E), want_oracle)


@pytest.mark.parametrize("name", ["mats", "mirrorbox"])
def test_the_handover_round_shows_in_the_image(name):
    """the yardstick separates neighbours: the oracle's images at E and E +- 1 differ (else the bit-equality tests above
    could not tell a handover one round off)"""
    sd = SCENES[name](name)
    imgs = {E: oracle_mixed(sd, 2, 50, 11, E) for E in (1, 2, 3, 4)}
    osc = oracle.OracleScene(sd, precision=0)
    imgs[0] = osc.render(2, 50, rng_mode=oracle.RNG_COUNTER, seed=11, threads=8)  # E = 0 is the default: f32 below E = 1
    osc.close()
    for E in (1, 2, 3):
        assert not np.array_equal(imgs[E], imgs[E + 1]) and not np.array_equal(imgs[E], imgs[E - 1]), E


@pytest.mark.parametrize("E", [1, 2, 4])
def test_batches_and_strips_reassemble_the_mixed_image(E):
    """batches reuse the path slots: a slot converted in one batch and not in the next must not add the stale f32
    radiance (S_CONV is reset by round 0)"""
    sd = golden_scene("mats")  # 64 x 48: every reference material, lights, three strips
    spp = 4
    want = oracle_mixed(sd, spp, 6, 9, E)
    for spb in (1, 3, spp):
        got, _ = hostsim_render(sd, 2, spp, 6, seed=9, samples_per_batch=spb, exact_bounces=E)
        assert np.array_equal(got, want), spb
    img = np.zeros_like(want)
    for r in range(3):
        img[strip_rows(sd.height, r, 3)], _ = hostsim_render(sd, 2, spp, 6, seed=9, strip_first=r, strip_stride=3,
                                                              samples_per_batch=3, exact_bounces=E)
    assert np.array_equal(img, want)


def test_ragged_image_mixed():
    sd = mirror_box_scene(37, 21)
    for E in (1, 3):
        got, _ = hostsim_render(sd, 2, 2, 50, seed=2, exact_bounces=E)
        assert np.array_equal(got, oracle_mixed(sd, 2, 50, 2, E))


def test_oracle_mixed_refuses_what_it_does_not_restate():
    osc = oracle.OracleScene(golden_scene("cbox"), precision=oracle.PRECISION_MIXED)
    try:
        with pytest.raises(ValueError):
            osc.render(1, 2, rng_mode=oracle.RNG_MT_PER_TILE)
        with pytest.raises(ValueError):
            osc.render(1, 2, integrator=1)
    finally:
        osc.close()

"""Render-level check of the environment-map light against a closed form, independent of the oracle: a big diffuse
plane of albedo rho with normal n under a map alone.  Every pixel's expectation is rho / pi * E(n), with
E(n) = env_ref.irradiance (exact per texel for n = +y, a midpoint rule otherwise).  Shared by test_env_cpu.py (the device
code on the host, at a smaller size) and test_gpu_env.py.

The bar comes from the oracle's own noise, not from the code under test: the scene is rendered by the oracle at 8
seeds, sigma = the standard deviation of the 8 image means, quad = the quadrature error of E (k = 32 against k = 64;
asserted under sigma / 10).  The render under test must have its image mean within 5 sigma + quad of the closed form,
and the oracle's own 8-seed mean within 5 sigma / sqrt(8) + quad — so a convention error that the oracle and the device
share (phi origin, row order, Jacobian) fails here although the two agree with each other.
"""
import numpy as np

import env_maps
import env_ref
import oracle
from test_envmap import plane_under_sky

RHO = 0.6
SEEDS = tuple(range(101, 109))
DTYPE = {0: np.float32, 1: np.float64}


def sun_direction():
    return env_ref.direction((env_maps.SUN_XY[0] + 0.5) / 64, (env_maps.SUN_XY[1] + 0.5) / 32)


# name -> (image, plane normal)
CASES = {
    "sun_up": (lambda: env_maps.image("sun"), (0.0, 1.0, 0.0)),
    "halves_up": (lambda: env_maps.image("halves"), (0.0, 1.0, 0.0)),
    "sun_flipped_up": (lambda: env_maps.image("sun")[::-1], (0.0, 1.0, 0.0)),  # the sun below the horizon: exactly black
    "sun_tilted": (lambda: env_maps.image("sun"), tuple(sun_direction() + np.array([0.3, 0.0, 0.2]))),  # pins phi
    "ragged_x": (lambda: env_maps.image("ragged"), (1.0, 0.0, 0.0)),
}
_MADE = {}


class Case:
    """one plane under one map at one size: the scene, the closed form and the oracle's statistics"""

    def __init__(self, name, precision, res, spp):
        make, self.normal = CASES[name]
        img = np.asarray(make(), np.float64).astype(DTYPE[precision]).astype(np.float64)  # the texels as the scene holds them
        self.name, self.precision, self.res, self.spp = name, precision, res, spp
        self.sd = plane_under_sky(0.0, RHO, True, img=img, normal=self.normal, res=res)
        fine = env_ref.irradiance(img, (1.0, 1.0, 1.0), self.normal, k=64)
        coarse = env_ref.irradiance(img, (1.0, 1.0, 1.0), self.normal, k=32)
        self.expect = float((RHO / np.pi * fine).mean())  # of the image mean: all pixels alike, the three channels averaged
        self.quad = float(np.abs(RHO / np.pi * (fine - coarse)).mean())
        self.oracle_means = []
        osc = oracle.OracleScene(self.sd, precision=precision)
        try:
            for seed in SEEDS:
                self.oracle_means.append(float(osc.render(spp=spp, max_depth=3, rng_mode=oracle.RNG_COUNTER, seed=seed).mean()))
        finally:
            osc.close()
        self.sigma = float(np.std(self.oracle_means, ddof=1))
        self.oracle_mean = float(np.mean(self.oracle_means))


def case(name, precision, res=24, spp=256):
    key = (name, precision, res, spp)
    if key not in _MADE:
        _MADE[key] = Case(*key)
    return _MADE[key]


def check_reference(c):
    """the yardstick itself: the quadrature error is far below the noise, and the oracle's mean agrees with the closed form"""
    print(f"ENV irradiance {c.name} f{32 * (1 + c.precision)} {c.res}x{c.res}x{c.spp}: expect {c.expect:.6e} sigma {c.sigma:.3e} "
          f"quad {c.quad:.3e} oracle mean off by {abs(c.oracle_mean - c.expect):.3e}")
    if c.expect == 0.0:
        assert c.sigma == 0.0 and c.quad == 0.0 and c.oracle_mean == 0.0
        return
    assert c.sigma > 0 and c.quad < c.sigma / 10, (c.quad, c.sigma)
    assert abs(c.oracle_mean - c.expect) <= 5 * c.sigma / np.sqrt(len(SEEDS)) + c.quad, (c.oracle_mean, c.expect, c.sigma)


def check_render(c, img):
    """img: the render under test of c.sd at c.spp samples, max_depth 3"""
    img = np.asarray(img, np.float64)
    assert img.shape == (c.res, c.res, 3) and np.isfinite(img).all()
    off = abs(float(img.mean()) - c.expect)
    print(f"ENV irradiance {c.name} f{32 * (1 + c.precision)} {c.res}x{c.res}x{c.spp}: render mean off by {off:.3e} "
          f"= {off / c.sigma if c.sigma else 0.0:.2f} sigma")
    if c.expect == 0.0:
        assert np.array_equal(img, np.zeros_like(img))
        return
    assert off <= 5 * c.sigma + c.quad, (float(img.mean()), c.expect, c.sigma)

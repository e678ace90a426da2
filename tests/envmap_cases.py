"""The maps of test_envbuild_cpu.py / test_gpu_envmap_update.py (take_hip_scene_set_envmap): the awkward maps of
tests/env_maps.py, `colours`, and a seeded random family at the sizes where the row scan of take_amd/csrc/tk_envmap.h takes
another path — one column, one row, one short of / exactly / one past a tile of 64 columns or a block of 16 rows (63,
64, 65), two tiles and a column (129), 130 x 67 (past a tile in both directions).  CASES[name]() -> (h, w, 3) float64."""
import numpy as np

import env_maps

WIDTHS, HEIGHTS = (1, 63, 64, 65, 129), (1, 2, 63, 64, 65)
SCALE = (1.5, 0.75, 2.0)  # what the tests replace the light's intensity by


def random_map(w, h):
    """uniform in [0.05, 2), a fifth of the texels exactly 0, row h // 2 all black (not of a one-row map); texel (0, 0)
    stays lit, so that no map of the family is all black"""
    rng = np.random.default_rng(1000 * w + h)
    img = rng.uniform(0.05, 2.0, (h, w, 3))
    zero = rng.uniform(size=(h, w)) < 0.2
    zero[0, 0] = False
    img[zero] = 0.0
    if h > 1:
        img[h // 2] = 0.0
    return img


def _family(w, h):
    return lambda: random_map(w, h)


CASES = {name: (lambda name=name: np.array(env_maps.image(name))) for name in env_maps.MAPS}
CASES["colours"] = env_maps.colours
FAMILY = [f"{w}x{h}" for w in WIDTHS for h in HEIGHTS] + ["130x67"]
for _name in FAMILY:
    CASES[_name] = _family(*(int(v) for v in _name.split("x")))
_CACHE = {}


def image(name):
    if name not in _CACHE:
        _CACHE[name] = np.ascontiguousarray(CASES[name](), np.float64)
        _CACHE[name].setflags(write=False)
    return _CACHE[name]


def black(w=65, h=17):
    return np.zeros((h, w, 3))


def one_nan(w=65, h=17):
    """black but for one NaN channel: the texel's luminance is NaN, which counts as 0 — the total stays 0, and scene
    creation refuses the map as it refuses the black one"""
    img = black(w, h)
    img[1, 5, 1] = np.nan
    return img

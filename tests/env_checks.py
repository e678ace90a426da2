"""The kernel-level checks of the environment map, shared by test_env_cpu.py (the device code on the host, hostsim_env)
and test_gpu_env.py (take_hip_debug_env): each takes a Case and `run(kind, rows) -> table`, the device functions on one
side of a scene that holds the case's map, and compares with tests/env_ref.py.

Bars (BAR[precision] = (pdf relative, dir absolute)): the reference works in float64 on the scene's own rounded tables
and inputs, so what is left is a handful of roundings in the scene's type and its sin / cos / acos / atan2.
f64: 1e-13 (a few hundred ulps of 2^-53); f32: 2e-6 = 32 * 2^-24, which covers a rounding of phi up to pi
(ulp 2.4e-7) carried through sin and cos.  They are set from the number formats, not from the code under test.

Which inputs are used (sample_inputs): every texel of positive probability whose two CDF steps are at least 64 ulps
of the scene's type wide (ulp = the spacing at the step's upper end).  A narrower step cannot hold a draw that is
0.05 of a texel away from both its edges once the draw is rounded to the type: the rounding alone moves it by up to
half an ulp.  On these maps the rule leaves out nothing in float64 and, in float32, only 371 of the 26425 drawable
texels of `tall` (polar rows, whose marginal step is a few ulps at a CDF value near 1); test_env_cpu.py asserts both.
"""
import numpy as np

import env_maps
import env_ref

BAR = {0: (2e-6, 2e-6), 1: (1e-13, 1e-13)}
DTYPE = {0: np.float32, 1: np.float64}
FRACTIONS = (0.1, 0.5, 0.9)
MIN_STEP_ULPS = 64
SUBSET = 4096  # texels of `wide` and `tall`
POLAR_ROWS = 34  # of float32 `tall`, at each pole: where a direction's rounding moves theta by 0.05 of a row or more
EDGE_MARGIN = 1e-3  # of a texel: random directions closer to a texel edge are dropped


class Case:
    """a map as a scene of the given Real holds it: texels, scale and CDF tables rounded to the type (kept as float64)"""

    def __init__(self, name, precision):
        self.name, self.precision, self.dtype = name, precision, DTYPE[precision]
        self.img = env_maps.image(name)
        self.scale = env_maps.SCALES[name]
        self.h, self.w = self.img.shape[:2]
        self.tabs = env_ref.tables_as(self.img, self.dtype)
        self.texels = self.img.astype(self.dtype).astype(np.float64)
        # radiance as the scene's type multiplies it: texel * scale, one rounding
        self.radiance = (self.img.astype(self.dtype) * np.asarray(self.scale, self.dtype)).astype(np.float64)
        self.prob = env_ref.texel_prob(self.tabs)

    def r(self, a):
        return np.asarray(a, np.float64).astype(self.dtype).astype(np.float64)


_CASES = {}


def case(name, precision):
    if (name, precision) not in _CASES:
        _CASES[name, precision] = Case(name, precision)
    return _CASES[name, precision]


def wide_steps(c):
    """(h, w) mask: texels whose marginal and conditional steps are both >= MIN_STEP_ULPS ulps of the type"""
    marg, cond = c.tabs
    ulp_m = np.spacing(marg[1:].astype(c.dtype)).astype(np.float64)
    ulp_c = np.spacing(cond[:, 1:].astype(c.dtype)).astype(np.float64)
    return (np.diff(marg) >= MIN_STEP_ULPS * ulp_m)[:, None] & (np.diff(cond, axis=1) >= MIN_STEP_ULPS * ulp_c)


def sample_inputs(c):
    """-> (rows of (u1, u2) in the type, the texel index y * w + x each row was made for)"""
    marg, cond = c.tabs
    y, x = np.nonzero((c.prob > 0) & wide_steps(c))
    if y.size > SUBSET:
        keep = np.sort(np.random.default_rng(21).choice(y.size, SUBSET, replace=False))
        y, x = y[keep], x[keep]
    f, g = [a.ravel() for a in np.meshgrid(FRACTIONS, FRACTIONS, indexing="ij")]
    u1 = marg[y][:, None] + f[None, :] * (marg[y + 1] - marg[y])[:, None]
    u2 = cond[y, x][:, None] + g[None, :] * (cond[y, x + 1] - cond[y, x])[:, None]
    idx = np.repeat(y * c.w + x, f.size)
    return np.stack([c.r(u1.ravel()), c.r(u2.ravel())], 1), idx


def relerr(got, want):
    return np.abs(got - want) / np.abs(want)


def check_samples(c, run):
    """test 1 -> (kind 0's table, max pdf relative error, max dir absolute error)"""
    rows, made_for = sample_inputs(c)
    assert rows.shape[0] >= 9
    got = run(0, rows)
    x, y, d, _, pdf, _ = env_ref.sample(c.tabs, c.texels, c.scale, rows[:, 0], rows[:, 1])
    assert np.array_equal(y * c.w + x, made_for)  # (the reference finds the texel each draw was made for)
    assert np.array_equal(got[:, 7], made_for), f"{np.count_nonzero(got[:, 7] != made_for)} of {rows.shape[0]} rows in another texel"
    assert np.array_equal(got[:, 3:6], c.radiance[y, x])
    e_pdf, e_dir = relerr(got[:, 6], pdf).max(), np.abs(got[:, 0:3] - d).max()
    print(f"ENV samples {c.name} f{32 * (1 + c.precision)}: rows {rows.shape[0]} pdf rel {e_pdf:.3e} dir abs {e_dir:.3e}")
    assert e_pdf <= BAR[c.precision][0] and e_dir <= BAR[c.precision][1], (e_pdf, e_dir)
    return got, e_pdf, e_dir


def check_lower_edges(c, run):
    """draws that ARE table values: (marginal[y], conditional[y][x]) for every texel of positive probability (a subset on
    `wide` / `tall`) belong to the texel that starts there — "the largest i with cdf[i] <= xi", past every zero-width
    interval that ends at the same value"""
    marg, cond = c.tabs
    y, x = np.nonzero(c.prob > 0)
    if y.size > SUBSET:
        keep = np.sort(np.random.default_rng(23).choice(y.size, SUBSET, replace=False))
        y, x = y[keep], x[keep]
    rows = np.stack([marg[y], cond[y, x]], 1)
    rx, ry = env_ref.find_texel(c.tabs, rows[:, 0], rows[:, 1])
    assert np.array_equal(rx, x) and np.array_equal(ry, y)
    got = run(0, rows)
    bad = np.count_nonzero(got[:, 7] != y * c.w + x)
    assert bad == 0, f"{bad} of {y.size} draws on a texel's lower edge in another texel"
    assert np.array_equal(got[:, 3:6], c.radiance[y, x])


def check_round_trip(c, run, sampled):
    """test 2: kind 0's directions through kind 1 give the texel, the radiance and the pdf back.
    What a direction of the scene's type can carry bounds this, and the bound is derived, not measured: its y component
    is cos(theta) rounded by up to eps = half an ulp at 1 (2^-24 / 2^-53), which moves theta by eps / sin(theta) and
    sin(theta) — hence the pdf — by the fraction eps / sin^2(theta).  So the pdf must agree within the bar
    + eps / sin^2(theta), and the texel must be the same wherever that shift is under 0.05 of a row —
    everywhere but next to the poles of the float32 `tall` map, whose rows are 1.9e-4 rad high."""
    eps = 2.0 ** -24 if c.precision == 0 else 2.0 ** -53
    sin_theta = np.hypot(sampled[:, 0], sampled[:, 2])
    carried = eps / sin_theta * c.h / np.pi < 0.05
    assert carried.all() or (c.name == "tall" and c.precision == 0)
    # (under 34 rows at each pole: (y + dv) pi / h < 6.3e-3 rad, each texel drawn at 9 points)
    assert np.count_nonzero(~carried) <= 2 * POLAR_ROWS * c.w * len(FRACTIONS) ** 2
    back = run(1, sampled[:, 0:3])
    bad = np.count_nonzero(back[carried, 4] != sampled[carried, 7])
    assert bad == 0, f"{bad} of {carried.size} rows in another texel"
    assert np.array_equal(back[carried, 0:3], sampled[carried, 3:6])
    excess = relerr(back[carried, 3], sampled[carried, 6]) - eps / sin_theta[carried] ** 2
    print(f"ENV round trip {c.name} f{32 * (1 + c.precision)}: pdf rel beyond the direction's own rounding {excess.max():.3e}")
    assert excess.max() <= BAR[c.precision][0], excess.max()
    return excess.max()


def directions(c):
    """-> (fixed (10, 3): six axes, the seam with z = +0 / -0, the poles again; random (4096, 3) unit vectors in the type)"""
    fixed = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 0.0], [-1, 0, -0.0],
                      [0, 1, 0], [0, -1, 0]], np.float64)
    v = np.random.default_rng(22).normal(size=(4096, 3))
    return fixed, c.r(v / np.linalg.norm(v, axis=1, keepdims=True))


def interior(c, d):
    """mask: directions the reference places at least EDGE_MARGIN of a texel from every texel edge"""
    _, _, _, (fx, fy) = env_ref.lookup(c.w, c.h, d)
    m = np.ones(fx.shape, bool)
    for t in (fx, fy):
        m &= np.abs(t - np.round(t)) >= EDGE_MARGIN
    return m


def check_directions(c, run):
    """test 3 -> max pdf relative error over the directions of positive probability"""
    fixed, rnd = directions(c)
    got = run(1, fixed)
    w, h = c.w, c.h
    # the axes: +x u = 1/2, -x the seam, +-z u = 3/4 / 1/4 — on texel edges unless the width is odd, so only where the
    # contract decides: the seam clamps to the last (z = +0: atan2 = +pi, u = 1) and first (z = -0: u = 0) column
    row_h = (h - 1) // 2 if h % 2 else None  # theta = pi/2 falls inside a row only when the height is odd
    if row_h is not None:
        assert got[6, 4] == row_h * w + (w - 1) and got[7, 4] == row_h * w
        assert np.array_equal(got[6, 0:3], c.radiance[row_h, w - 1]) and np.array_equal(got[7, 0:3], c.radiance[row_h, 0])
    else:
        assert got[6, 4] % w == w - 1 and got[7, 4] % w == 0
    assert np.array_equal(got[1], got[6])
    # the poles: pdf exactly 0, radiance of row 0 / row h - 1 (which column atan2(0, 0) picks: u = 1/2)
    for k, row in ((2, 0), (3, h - 1), (8, 0), (9, h - 1)):
        assert got[k, 3] == 0.0 and got[k, 4] // w == row
        assert np.array_equal(got[k, 0:3], c.radiance[row, int(got[k, 4]) % w])
    assert np.isfinite(got).all()
    # +x, +z, -z (u = 1/2, 3/4, 1/4; theta = pi/2): wherever the map's size puts them inside a texel, as the reference
    axes = np.array([0, 4, 5])[interior(c, fixed[[0, 4, 5]])]
    if axes.size:
        x, y, rad, pdf = env_ref.eval(c.tabs, c.texels, c.scale, fixed[axes])
        assert np.array_equal(got[axes, 4], y * w + x) and np.array_equal(got[axes, 0:3], c.radiance[y, x])
        assert np.array_equal(got[axes, 3][pdf == 0], pdf[pdf == 0])
        assert (relerr(got[axes, 3][pdf > 0], pdf[pdf > 0]) <= BAR[c.precision][0]).all()
    keep = interior(c, rnd)
    d = rnd[keep]
    got = run(1, d)
    x, y, rad, pdf = env_ref.eval(c.tabs, c.texels, c.scale, d)
    bad = np.count_nonzero(got[:, 4] != y * w + x)
    assert bad == 0, f"{bad} of {d.shape[0]} directions in another texel"
    assert np.array_equal(got[:, 0:3], c.radiance[y, x])
    zero = pdf == 0
    assert np.array_equal(got[zero, 3], np.zeros(np.count_nonzero(zero)))  # zero probability: pdf exactly 0
    e = relerr(got[~zero, 3], pdf[~zero]).max() if (~zero).any() else 0.0
    print(f"ENV directions {c.name} f{32 * (1 + c.precision)}: kept {d.shape[0]} zero {np.count_nonzero(zero)} pdf rel {e:.3e}")
    assert e <= BAR[c.precision][0], e
    return e


def grid_n(c):
    """N of the N x N stratified grid: 1024, scaled down so that the `wide` / `tall` maps draw at most 2^21 rows"""
    return 1024 if c.name not in ("wide", "tall") else 1448


def check_histogram(c, run):
    """test 4: an N x N midpoint grid of draws; a texel with CDF steps dm, dc receives between (dm N - 1)(dc N - 1) and
    (dm N + 1)(dc N + 1) of them (an interval of length d holds between d N - 1 and d N + 1 of the N midpoints, and the
    columns are searched within the row the first draw picked), clipped at 0; a zero-width texel receives none"""
    n = grid_n(c)
    assert n * n <= 1 << 21
    t = c.r((np.arange(n) + 0.5) / n)
    rows = np.stack([np.repeat(t, n), np.tile(t, n)], 1)
    got = run(0, rows)
    counts = np.bincount(got[:, 7].astype(np.int64), minlength=c.w * c.h).reshape(c.h, c.w)
    assert counts.sum() == n * n
    marg, cond = c.tabs
    dm, dc = np.diff(marg)[:, None] * n, np.diff(cond, axis=1) * n
    lo = np.maximum(dm - 1, 0) * np.maximum(dc - 1, 0)
    hi = (dm + 1) * (dc + 1)
    assert np.array_equal(counts[c.prob == 0], np.zeros(np.count_nonzero(c.prob == 0), counts.dtype))
    bad = np.count_nonzero((counts < lo) | (counts > hi))
    assert bad == 0, f"{bad} texels outside their bounds"


def check_normalisation(c, run):
    """test 6: the device pdf at every texel centre gives back P(texel) = pdf * 2 pi^2 sin(theta) / (w h)"""
    w, h = c.w, c.h
    u, v = np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h)
    d = c.r(env_ref.direction(u.ravel(), v.ravel()))
    got = run(1, d)
    # sin(theta) of the direction the device was given (rounded to its type)
    sin_theta = np.sqrt((1.0 - d[:, 1]) * (1.0 + d[:, 1]))
    # a centre is used where its direction, rounded to the type, still names its row: the rule of check_round_trip
    # (cos(theta) rounded by eps moves theta by eps / sin(theta); under 0.05 of a row).  That is every centre but
    # those of the rows next to the poles of the float32 `tall` map (33 of 16500 at each end; the outermost 2 round
    # to the pole itself); those terms are left out of both sums that are compared.
    eps = 2.0 ** -24 if c.precision == 0 else 2.0 ** -53
    carried = eps * h / np.pi < 0.05 * sin_theta
    assert carried.all() or (c.name == "tall" and c.precision == 0)
    assert np.count_nonzero(~carried) <= 2 * POLAR_ROWS * w
    assert np.array_equal(got[carried, 4], np.arange(w * h)[carried])
    want = c.prob.ravel()[carried]
    p = (got[:, 3] * 2.0 * np.pi ** 2 * sin_theta / (w * h))[carried]
    assert np.array_equal(p[want == 0], np.zeros(np.count_nonzero(want == 0)))
    e = relerr(p[want > 0], want[want > 0]).max()
    total = abs(p.sum() - (1.0 if carried.all() else want.sum()))  # every centre: the sum is 1; else the partial sums agree
    print(f"ENV normalisation {c.name} f{32 * (1 + c.precision)}: term rel {e:.3e} |sum - 1| {total:.3e}")
    assert e <= BAR[c.precision][0] and total <= w * h * BAR[c.precision][0], (e, total)
    return e

"""Data for the texture-lookup tests (tests/test_texture_cpu.py, tests/test_gpu_texture_edges.py): image shapes and rows
(u, v, uscale, vscale, uoffset, voffset) per precision (real: 0 = f32, 1 = f64), every value exactly representable in it.

Exact rows: a = scale * x + offset is itself a value of the precision and the device computes it without rounding, so
only the wrap and the interpolation round.  They sit where the wrap goes wrong: a in (-eps/4, 0), where r + 1 of a
floating modulo rounds to 1 (f32: -2^-26, -2^-30, -2^-100 and the tie -2^-25; f64 also -2^-54, -2^-60, -2^-1000), the
first value outside that window, signed zeros, the integers and their neighbours, every texel boundary k/W that is a
binary fraction (W = 1, 2, 4, 8) with its two neighbours — each on u alone, on v alone and on both — and the same `a`
reached through a scale or an offset.  No exact row is ever left out of a comparison.  No denormal `a`: whether a device
flushes it decides between the cells 0 and W-1 (tests/texture_host's program has them, for bounds only).

Generic rows: 512 with u, v uniform in [-2, 3] and 128 with |a| up to 2^20, the transforms drawn per axis from
{1, 2, 0.5, -1} x {0, 0.25, -0.4}, fixed seed.  The f32 a of such a row carries a rounding error; a row whose cell is
not the same over that error (texture_ref.is_stable) is left out, at most 5 % of them.  The 128 large rows are drawn as
an `a` of the precision and solved for x with the offsets 0 and 0.25 only, so that a is exact: with -0.4 the sum rounds,
and from |a| ~ 2^9 in f32 (2^12 in f64) that rounding alone — 2^-16 (2^-42) of a texture period — moves the result by
more than the precision's bar inside one cell.

Images: (H, W) = 1x1, 6x1, 1x6, 2x2, 4x5 and 4x8 (the issue's W x H: 1x1, 1x6, 6x1, 2x2, 5x4, 8x4); the 207 texel
values are a fixed permutation of k / 209: none occurs twice anywhere, so a read from a neighbouring row or image shows,
and none of the images is affine in (x, y), so a wrong cell cannot extrapolate to the right value."""
from fractions import Fraction

import numpy as np

F32, F64 = 0, 1
SHAPES = [(1, 1), (6, 1), (1, 6), (2, 2), (4, 5), (4, 8)]  # (H, W), in pool order
OTHER = 0.3125  # the axis that is not under test: inside a cell of every shape
SCALES, OFFSETS = (1.0, 2.0, 0.5, -1.0), (0.0, 0.25, -0.4)


def images():
    """the six images, float64 (H, W, 3) in [0, 1]"""
    n = sum(3 * h * w for h, w in SHAPES)
    values = (np.random.default_rng(77).permutation(n) + 1.0) / (n + 2.0)
    out, at = [], 0
    for h, w in SHAPES:
        out.append(values[at:at + 3 * h * w].reshape(h, w, 3).copy())
        at += 3 * h * w
    return out


def table_image():
    """the fixed 5x4 image of take_hip_debug_table and oracle.table("texture" / "material") (oracle/take_oracle.cpp)"""
    img = np.zeros((4, 5, 3))
    for y in range(4):
        for x in range(5):
            img[y, x] = (0.1 + 0.15 * x + 0.01 * y, 0.9 - 0.2 * y + 0.02 * x, 0.3 + 0.05 * ((x * 3 + y * 7) % 5))
    return img


def _ftype(real):
    return np.float32 if real == F32 else np.float64


def exact_values(real):
    """the `a` of the exact rows, float64 that hold values of the precision"""
    t = _ftype(real)
    a = [-2.0 ** -26, -2.0 ** -30, -2.0 ** -100, -2.0 ** -25, -2.0 ** -24]
    if real == F64:
        a += [-2.0 ** -54, -2.0 ** -60, -2.0 ** -1000]
    a += [-0.0, 0.0, 2.0 ** -26]
    a += [float(np.nextafter(t(1), t(0))), 1.0, 1.0 + 2.0 ** -23, -1.0, -1.0 - 2.0 ** -23, -3.0, 2.0, 2.0 ** 20, 0.5]
    for w in (1, 2, 4, 8):
        for k in range(w + 1):
            b = t(k) / t(w)
            a += [float(b)] + [float(n) for n in (np.nextafter(b, t(-9)), np.nextafter(b, t(9))) if abs(n) >= np.finfo(t).tiny]
    seen, out = set(), []
    for v in a:
        key = (v, bool(np.signbit(v)))
        if key not in seen:
            seen.add(key)
            out.append(v)
    assert all(float(t(v)) == v and (v == 0 or abs(v) >= np.finfo(t).tiny) for v in out)
    return out


def _transformed(real):
    """(x, scale, offset) that reach an `a` inside the window through the transform, exactly"""
    out = [(2.0 ** -26, -1.0, 0.0), (-2.0 ** -27, 2.0, 0.0), (-2.0 ** -24, 0.5, 0.0)]
    out.append((0.5 - 2.0 ** -25, 1.0, -0.5))  # a = -2^-25, the tie of f32
    if real == F64:
        out += [(0.5 - 2.0 ** -26, 1.0, -0.5), (0.5 - 2.0 ** -54, 1.0, -0.5), (2.0 ** -60, -1.0, 0.0)]
    return out


def exact_rows(real):
    rows = []
    for a in exact_values(real):
        rows += [(a, OTHER, 1, 1, 0, 0), (OTHER, a, 1, 1, 0, 0), (a, a, 1, 1, 0, 0)]
    for x, s, o in _transformed(real):
        rows += [(x, OTHER, s, 1, o, 0), (OTHER, x, 1, s, 0, o), (x, x, s, s, o, o)]
    rows = np.array(rows, np.float64)
    assert np.array_equal(rows.astype(_ftype(real)).astype(np.float64), rows)
    return rows


def generic_rows(real):
    t = _ftype(real)
    rng = np.random.default_rng(4100 + real)
    rows = np.zeros((640, 6))
    rows[:512, 0:2] = rng.uniform(-2.0, 3.0, (512, 2))
    rows[:, 2:4] = rng.choice(SCALES, (640, 2))
    rows[:512, 4:6] = rng.choice(OFFSETS, (512, 2))
    big = np.exp2(rng.uniform(2.0, 20.0, (128, 2))) * rng.choice((-1.0, 1.0), (128, 2))
    off = rng.choice(OFFSETS[:2], (128, 2))
    a = big.astype(t).astype(np.float64)
    x = (a - off).astype(t).astype(np.float64)
    exact = np.array([[Fraction(x[i, j]) + Fraction(off[i, j]) == Fraction(a[i, j]) for j in range(2)] for i in range(128)])
    rows[512:, 4:6] = np.where(exact, off, 0.0)
    rows[512:, 0:2] = np.where(exact, x, a) / rows[512:, 2:4]  # (a power of two: exact)
    rows = rows.astype(t).astype(np.float64)
    assert np.isfinite(rows).all()
    return rows

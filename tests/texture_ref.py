"""The bilinear wrap lookup of src/texture.cpp:3-25 in exact rational arithmetic (fractions.Fraction): no fmod, no float
until the result.  Independent of take_amd/csrc/tk_shade.h (eval_texture), oracle/take_oracle.hpp and the reference:
the wrap is a - floor(a), which lies in [0, 1) for every finite a, so the cell is the one exact arithmetic picks —
in particular the seam cell width-1 -> 0 for an `a` just below an integer, where r + 1 of a floating modulo rounds to 1.

The inputs (u, v, uscale, vscale, uoffset, voffset and the texels) are rounded to the precision under test first
(real: 0 = f32, 1 = f64); everything after is exact.  The reference's seam weights are kept as written: x2 - x with
x2 = 0 at the seam, the divisor (x2 - x1) * (y2 - y1), and x1 == x2 -> x2 += 1 for a width of 1."""
import math
from fractions import Fraction

import numpy as np

F32, F64 = 0, 1
PRED1 = {F32: 1.0 - 2.0 ** -24, F64: 1.0 - 2.0 ** -53}  # the largest value of the precision below 1


def rounded(x, real):
    """x rounded to the precision, as a float64 that holds it exactly"""
    return float(np.float32(x)) if real == F32 else float(x)


def representable(q, real):
    """whether the Fraction q is a (normal or zero) value of the precision"""
    try:
        f = float(q)
    except OverflowError:
        return False
    return Fraction(rounded(f, real)) == q


def ulp(q, real):
    """spacing of the precision at |q|"""
    f = abs(float(q))
    return Fraction(float(np.spacing(np.float32(f)))) if real == F32 else Fraction(float(np.spacing(f)))


def coordinate(x, scale, offset, real):
    """a = scale * x + offset of one axis, exactly, from the rounded inputs"""
    return Fraction(rounded(scale, real)) * Fraction(rounded(x, real)) + Fraction(rounded(offset, real))


def axis(a, n):
    """-> (x, x1, x2): the position in texels and the two columns (rows) the filter reads, x2 wrapped to 0 at n"""
    w = a - math.floor(a)  # in [0, 1)
    x = n * w
    x1 = math.floor(x)  # in [0, n - 1]
    assert 0 <= x1 < n
    return x, x1, (0 if x1 + 1 == n else x1 + 1)


def lookup_at(img, ax, ay):
    """the lookup at the exact coordinates (ax, ay) on img (H, W, 3), texels already in the precision -> float64[3]"""
    h, w = len(img), len(img[0])
    x, x1, x2 = axis(ax, w)
    y, y1, y2 = axis(ay, h)
    q11, q12, q21, q22 = img[y1][x1], img[y2][x1], img[y1][x2], img[y2][x2]
    if x1 == x2:
        x2 += 1
    if y1 == y2:
        y2 += 1
    fx2, fx1, fy2, fy1 = x2 - x, x - x1, y2 - y, y - y1
    div = (x2 - x1) * (y2 - y1)
    return np.array([float((Fraction(q11[c]) * fx2 * fy2 + Fraction(q21[c]) * fx1 * fy2 + Fraction(q12[c]) * fx2 * fy1 + Fraction(q22[c]) * fx1 * fy1) / div)
                     for c in range(3)])


def texels(img, real):
    """img (H, W, 3) rounded to the precision, as nested lists of float64"""
    a = np.asarray(img, np.float64)
    return (a.astype(np.float32).astype(np.float64) if real == F32 else a).tolist()


def lookup(img, row, real):
    """row = (u, v, uscale, vscale, uoffset, voffset) -> float64[3]"""
    u, v, us, vs, uo, vo = (float(t) for t in row)
    return lookup_at(texels(img, real), coordinate(u, us, uo, real), coordinate(v, vs, vo, real))


def lookup_rows(img, rows, real):
    t = texels(img, real)
    out = np.zeros((len(rows), 3))
    for k, (u, v, us, vs, uo, vo) in enumerate(np.asarray(rows, np.float64).tolist()):
        out[k] = lookup_at(t, coordinate(u, us, uo, real), coordinate(v, vs, vo, real))
    return out


def cell(shape, row, real):
    """(x1, y1) of the row on an image of shape (H, W)"""
    u, v, us, vs, uo, vo = (float(t) for t in row)
    return axis(coordinate(u, us, uo, real), shape[1])[1], axis(coordinate(v, vs, vo, real), shape[0])[1]


def axis_is_stable(x, scale, offset, n, real):
    """Whether the cell of one axis survives the rounding of a in the precision.  The device computes
    a' = fl(fl(scale * x) + offset).  Where both operations are exact, a' = a and there is nothing to survive.
    Otherwise the two roundings together stay within one ulp of the larger of |scale * x| and |a|: the cell has to be the
    same at a and one such ulp to either side."""
    p = Fraction(rounded(scale, real)) * Fraction(rounded(x, real))
    a = p + Fraction(rounded(offset, real))
    if representable(p, real) and representable(a, real):
        return True
    d = ulp(max(abs(p), abs(a)), real)
    return axis(a - d, n)[1] == axis(a, n)[1] == axis(a + d, n)[1]


def is_stable(shape, row, real):
    """a generic row is compared only where its cell is the same on both axes over the rounding of a"""
    u, v, us, vs, uo, vo = (float(t) for t in row)
    return axis_is_stable(u, us, uo, shape[1], real) and axis_is_stable(v, vs, vo, shape[0], real)

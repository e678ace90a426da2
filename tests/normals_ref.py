"""numpy restatement of the reference's compute_normals (src/compute_normals.cpp:12-47, src/vector.h), for the tests of
take_hip_compute_normals: every operation of the reference in its order, vectorised over faces.  asin is math.asin,
the C library's, as the reference's; the vertex sums are np.add.at (unbuffered: applied one by one in index order =
increasing face, then corner 0, 1, 2), starting from +0.0.  Faces whose normal has length 0 are left out, not added
as zeros: -0.0 + +0.0 is +0.0."""
import math

import numpy as np

C_PI = 3.14159265358979323846
_asin = np.frompyfunc(math.asin, 1, 1)


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def length(a):
    return np.sqrt(dot(a, a))


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def div(a, s):
    """Vector3 / Real: one reciprocal, three multiplies (src/vector.h:194-197)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return a * (1.0 / s)[..., None]


def normalize(a):
    l = length(a)
    out = div(a, l)
    out[l <= 0] = 0.0  # (a NaN length takes the division, as in the reference)
    return out


def asin(x):
    return _asin(x).astype(np.float64)


def unit_angle(u, v):
    """(pi - 2) * asin(...) on the obtuse branch: the reference's formula as written"""
    obtuse = dot(u, v) < 0
    a = np.empty(u.shape[:-1])
    a[obtuse] = (C_PI - 2) * asin(0.5 * length(v[obtuse] + u[obtuse]))
    a[~obtuse] = 2 * asin(0.5 * length(v[~obtuse] - u[~obtuse]))
    return a


def contributions(positions, indices):
    """-> (kept: faces whose normal has a non-zero length, (nf, 3, 3) products n * angle per corner)"""
    p = positions[indices]  # (nf, 3 corners, 3)
    n = cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    l = length(n)
    kept = ~(l == 0)
    n = div(n, l)
    c = np.empty(p.shape)
    for i in range(3):
        v0, v1, v2 = p[:, i], p[:, (i + 1) % 3], p[:, (i + 2) % 3]
        c[:, i] = n * unit_angle(normalize(v1 - v0), normalize(v2 - v0))[:, None]
    return kept, c


def compute_normals(positions, indices):
    positions = np.asarray(positions, np.float64).reshape(-1, 3)
    indices = np.asarray(indices, np.int64).reshape(-1, 3)
    if indices.size and (indices.min() < 0 or indices.max() >= len(positions)):
        raise IndexError("vertex index out of range")
    out = np.zeros(positions.shape)
    if len(indices):
        kept, c = contributions(positions, indices)
        np.add.at(out, indices[kept].reshape(-1), c[kept].reshape(-1, 3))
    l = length(out)
    nz = l != 0
    res = np.zeros(out.shape)
    res[nz] = div(out[nz], l[nz])
    return res


def condition(positions, indices):
    """per vertex sum |c_i| / |sum c_i| over its contributions c_i = n * angle (inf / nan where the sum is zero or there
    is none): the factor by which rounding in the contributions — an asin one ulp apart — is magnified in the normal"""
    positions = np.asarray(positions, np.float64).reshape(-1, 3)
    indices = np.asarray(indices, np.int64).reshape(-1, 3)
    nv = len(positions)
    kept, c = contributions(positions, indices)
    v, c = indices[kept].reshape(-1), c[kept].reshape(-1, 3)
    mag = np.bincount(v, length(c), minlength=nv)
    s = np.stack([np.bincount(v, c[:, k], minlength=nv) for k in range(3)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return mag / length(s)

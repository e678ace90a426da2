"""Independent float64 reference of the environment-map light (TakeLight kind 2), written from its documented contract
and not from the device code or the oracle:

  * include/take_hip.h: an equirectangular image, y up, row 0 = zenith, importance-sampled by luminance * sin(theta);
    `intensity` scales the image;
  * take_amd.scenes.sky_envmap: u = atan2(z, x) / 2pi + 1/2, v = theta / pi, so that a point (u, v) of the unit square is
    the direction (sin(theta) cos(phi), cos(theta), sin(theta) sin(phi)) with theta = v pi, phi = (u - 1/2) 2pi;
  * the recipe above env_tables (take_amd/csrc/tk_host_scene.h): per texel f = luminance * sin(theta of the row centre),
    luminance = 0.2126 r + 0.7152 g + 0.0722 b with negatives counting as 0; conditional CDF per row (uniform for an
    all-black row), marginal CDF over the rows; both start at 0 and end at exactly 1.

Everything is piecewise constant per texel.  A texel is drawn with probability P = (marginal step) * (conditional step),
uniformly over its rectangle of the unit square; the density over the sphere follows from d(omega) = sin(theta) dtheta
dphi = 2 pi^2 sin(theta) du dv:  pdf(d) = P * w * h / (2 pi^2 sin(theta)).

The searches are plain: the largest i with cdf[i] <= xi.  No guide tables.  All arithmetic after the tables is float64;
for a float32 scene the tables are rounded first (tables_as), as the scene holds them, and the caller rounds the draws,
directions and texels it feeds in.
"""
import math

import numpy as np

LUM = (0.2126, 0.7152, 0.0722)


def tables(img):
    """img (h, w, 3) -> (marginal (h + 1,), conditional (h, w + 1)) in float64"""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    lum = LUM[0] * img[..., 0] + LUM[1] * img[..., 1] + LUM[2] * img[..., 2]
    lum = np.where(lum > 0, lum, 0.0)
    row_sin = np.array([math.sin(math.pi * (y + 0.5) / h) for y in range(h)])
    f = lum * row_sin[:, None]
    run = np.concatenate([np.zeros((h, 1)), np.cumsum(f, axis=1)], axis=1)  # sums left of x, in order
    row_sum = run[:, -1]
    cond = np.empty((h, w + 1))
    for y in range(h):
        cond[y] = run[y] / row_sum[y] if row_sum[y] > 0 else np.arange(w + 1) / w
    cond[:, w] = 1.0
    above = np.concatenate([[0.0], np.cumsum(row_sum)])
    if not above[-1] > 0:
        raise ValueError("no positive luminance")
    marg = above / above[-1]
    marg[h] = 1.0
    return marg, cond


def tables_as(img, dtype):
    """the tables as a scene of that Real holds them: rounded to `dtype`, returned as float64 arrays"""
    marg, cond = tables(img)
    return marg.astype(dtype).astype(np.float64), cond.astype(dtype).astype(np.float64)


def texel_prob(tabs):
    """(h, w) probability with which a sample lands in each texel"""
    marg, cond = tabs
    return np.diff(marg)[:, None] * np.diff(cond, axis=1)


def texel_solid_angle(w, h):
    """(h,) solid angle of one texel of each row: (2 pi / w) * (cos(theta0) - cos(theta1))"""
    edges = np.cos(np.pi * np.arange(h + 1) / h)
    return (2.0 * np.pi / w) * (edges[:-1] - edges[1:])


def find(cdf, n, xi):
    """largest i in [0, n) with cdf[i] <= xi"""
    return np.clip(np.searchsorted(cdf[:n], xi, side="right") - 1, 0, n - 1)


def find_texel(tabs, u1, u2):
    marg, cond = tabs
    h, w = cond.shape[0], cond.shape[1] - 1
    y = find(marg, h, u1)
    x = np.zeros_like(y)
    for row in np.unique(y):
        k = y == row
        x[k] = find(cond[row], w, u2[k])
    return x, y


def direction(u, v):
    theta, phi = v * np.pi, (u - 0.5) * 2.0 * np.pi
    st = np.sin(theta)
    return np.stack([st * np.cos(phi), np.cos(theta), st * np.sin(phi)], -1)


def _pdf(p, w, h, sin_theta):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sin_theta > 0, p * w * h / (2.0 * np.pi ** 2 * sin_theta), 0.0)


def sample(tabs, img, scale, u1, u2):
    """-> (x, y, dir (n, 3), radiance (n, 3), pdf (n,)); also the position (du, dv) in the texel as a sixth value"""
    marg, cond = tabs
    h, w = cond.shape[0], cond.shape[1] - 1
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    x, y = find_texel(tabs, u1, u2)
    m0, m1, c0, c1 = marg[y], marg[y + 1], cond[y, x], cond[y, x + 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        dv = np.where(m1 > m0, (u1 - m0) / (m1 - m0), 0.5)
        du = np.where(c1 > c0, (u2 - c0) / (c1 - c0), 0.5)
    d = direction((x + du) / w, (y + dv) / h)
    # sin(theta) to full relative accuracy: from the nearer pole (sin(pi - a) = sin(a); next to pi, theta itself is rounded)
    sin_theta = np.sin(np.minimum(y + dv, (h - 1 - y) + (1.0 - dv)) / h * np.pi)
    rad = np.asarray(img, np.float64)[y, x] * np.asarray(scale, np.float64)
    return x, y, d, rad, _pdf((m1 - m0) * (c1 - c0), w, h, sin_theta), (du, dv)


def lookup(w, h, d):
    """direction(s) -> (x, y, sin_theta, (fx, fy)): the texel and the continuous texel coordinates it was floored from"""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    cy = np.clip(d[:, 1], -1.0, 1.0)
    fx = (np.arctan2(d[:, 2], d[:, 0]) / (2.0 * np.pi) + 0.5) * w
    fy = np.arccos(cy) / np.pi * h
    x = np.clip(np.floor(fx).astype(np.int64), 0, w - 1)
    y = np.clip(np.floor(fy).astype(np.int64), 0, h - 1)
    return x, y, np.sqrt(np.maximum(0.0, (1.0 - cy) * (1.0 + cy))), (fx, fy)


def eval(tabs, img, scale, d):
    """-> (x, y, radiance (n, 3), pdf (n,)) for unit directions d"""
    h, w = tabs[1].shape[0], tabs[1].shape[1] - 1
    x, y, sin_theta, _ = lookup(w, h, d)
    rad = np.asarray(img, np.float64)[y, x] * np.asarray(scale, np.float64)
    return x, y, rad, _pdf(texel_prob(tabs)[y, x], w, h, sin_theta)


def irradiance(img, scale, n, k=32):
    """integral of L(d) max(0, n.d) d(omega) over the sphere -> (3,).  n = +y: the closed form per texel,
    (2 pi / w) * (sin^2(theta1) - sin^2(theta0)) / 2 over the upper hemisphere's part of each row; any other n: the midpoint
    rule at k x k points per texel (in (u, v), with the sin(theta) of the measure)"""
    img = np.asarray(img, np.float64) * np.asarray(scale, np.float64)
    h, w = img.shape[:2]
    n = np.asarray(n, np.float64)
    n = n / np.linalg.norm(n)
    if np.array_equal(n, [0.0, 1.0, 0.0]):
        t = np.minimum(np.pi * np.arange(h + 1) / h, np.pi / 2)
        row = (2.0 * np.pi / w) * 0.5 * (np.sin(t[1:]) ** 2 - np.sin(t[:-1]) ** 2)
        return (img * row[:, None, None]).sum(axis=(0, 1))
    total = np.zeros(3)
    v = (np.arange(h * k) + 0.5) / (h * k)
    u = (np.arange(w * k) + 0.5) / (w * k)
    cell = 2.0 * np.pi ** 2 / (w * k * h * k)
    for y in range(h):
        vv = v[y * k:(y + 1) * k]
        d = direction(*np.broadcast_arrays(u[None, :], vv[:, None]))  # (k, w k, 3)
        g = np.maximum(0.0, d @ n) * np.sin(vv * np.pi)[:, None] * cell
        total += (g.reshape(k, w, k).sum(axis=(0, 2))[:, None] * img[y]).sum(axis=0)
    return total

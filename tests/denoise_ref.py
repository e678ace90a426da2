"""numpy restatement of the image-space denoiser (include/take_hip.h: take_hip_denoise*; take_amd/csrc/tk_denoise.h),
templated on the dtype: the edge-avoiding A-trous wavelet filter of Dammertz et al. 2010 with the slices and the
operation order of the specification (DESIGN.md par. 4f) — demodulate, `iterations` levels of 5 x 5 taps with holes of
2^i pixels (dy outer, dx inner, taps outside the image skipped), remodulate.  Every constant is computed in double and
rounded to the dtype once; every + - * / below is one operation of the dtype.  Also the synthetic planes the CPU and GPU
tests share."""
import numpy as np

H = (0.375, 0.25, 0.0625)  # the B3 spline, exact in binary
DEFAULTS = dict(iterations=5, keep_albedo=False, sigma_color=1.0, sigma_normal=0.3, sigma_depth=0.05, albedo_floor=1e-3)


def denoise(rgb, albedo=None, normal=None, depth=None, dtype=None, **opts):
    """rgb (H, W, 3), optional guides albedo / normal (H, W, 3) and depth (H, W) -> (H, W, 3) of `dtype` (default: rgb's);
    options as DEFAULTS (a value <= 0 takes the default, as in TakeDenoiseOpts)"""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in opts.items() if k == "keep_albedo" or v > 0})
    assert set(o) == set(DEFAULTS) and 1 <= o["iterations"] <= 8
    T = np.dtype(dtype or np.asarray(rgb).dtype).type
    C = np.array(rgb, T)
    N = None if normal is None else np.array(normal, T)
    Z = None if depth is None else np.array(depth, T)
    h, w = C.shape[:2]
    demod = albedo is not None and not o["keep_albedo"]
    if demod:
        A = np.fmax(np.array(albedo, T), T(o["albedo_floor"]))
        C = C / A
    inv_n, inv_d = T(1.0 / (o["sigma_normal"] * o["sigma_normal"])), T(1.0 / (o["sigma_depth"] * o["sigma_depth"]))
    tiny = np.finfo(T).tiny
    for i in range(o["iterations"]):
        s = 1 << i
        inv_c = T(4.0 ** i / (o["sigma_color"] * o["sigma_color"]))
        num, den = np.zeros_like(C), np.zeros((h, w), T)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                if y0 >= y1 or x0 >= x1:
                    continue  # every tap of this offset is outside
                P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                k = T(H[abs(dx)]) * T(H[abs(dy)])
                dc = C[P] - C[Q]
                x = ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) * inv_c
                if N is not None:
                    dn = N[P] - N[Q]
                    x = x + ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) * inv_n
                if Z is not None:
                    m = np.fmax(np.fmax(np.abs(Z[P]), np.abs(Z[Q])), tiny)
                    r = (Z[P] - Z[Q]) / m
                    x = x + (r * r) * inv_d
                wgt = k * np.exp(-x)
                num[P] += wgt[..., None] * C[Q]
                den[P] += wgt
        C = num / den[..., None]
    out = C * A if demod else C
    assert out.dtype == T
    return out


# ------------------------------------------------------------------ the synthetic planes of the tests
SIZES = [(1, 1), (7, 1), (1, 7), (37, 23), (130, 70)]  # (width, height)


def planes(width, height, noise=0.0, seed=1):
    """A checker albedo times an illumination that is constant per region: a left and a right region separated by a
    normal and depth edge, and above them a zero-albedo "sky" band (a miss: albedo, normal and depth 0, a constant
    radiance).  Inside a region normal and depth vary smoothly, so that their weights are not all 1.  noise > 0:
    multiplicative noise on rgb, uniform in 1 +- noise per pixel and channel.
    -> dict of float64 arrays rgb, albedo, normal (H, W, 3), depth (H, W) and clean (rgb without the noise)"""
    y, x = np.mgrid[0:height, 0:width]
    sky = y < height // 5
    right = x >= (9 * width) // 20
    checker = ((x // 3 + y // 2) % 2 == 1)[..., None]
    albedo = np.where(checker, (0.8, 0.6, 0.3), (0.2, 0.35, 0.7))
    illum = np.where(right[..., None], (0.3, 0.5, 0.8), (1.5, 1.2, 0.9))
    n = np.where(right[..., None], np.stack([1.0 + 0 * x, 0.004 * y, 0.002 * x], -1), np.stack([0.003 * x, 0.002 * y, 1.0 + 0 * x], -1))
    n = n / np.sqrt((n * n).sum(-1, keepdims=True))
    depth = np.where(right, 3.0 + 0.002 * y, 2.0 + 0.001 * x)
    albedo = np.where(sky[..., None], 0.0, albedo)
    n = np.where(sky[..., None], 0.0, n)
    depth = np.where(sky, 0.0, depth)
    clean = np.where(sky[..., None], (0.4, 0.6, 0.9), albedo * illum)
    rgb = clean
    if noise > 0:
        rgb = clean * np.random.default_rng(seed).uniform(1.0 - noise, 1.0 + noise, clean.shape)
    return {"rgb": rgb, "albedo": albedo, "normal": n, "depth": depth, "clean": clean}


def cast(p, dtype):
    """the four input planes in `dtype`, contiguous"""
    return {k: np.ascontiguousarray(p[k], dtype) for k in ("rgb", "albedo", "normal", "depth")}

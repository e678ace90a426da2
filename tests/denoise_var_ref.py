"""numpy restatement of the variance-guided denoiser (include/take_hip.h: take_hip_denoise_variance*;
take_amd/csrc/tk_denoise_var.h), templated on the dtype, with the slices and the operation order of the specification
(DESIGN.md par. 4h): the initial variance of the pixel mean from the adaptive sampler's count / m1 / m2 planes (in
double, rounded once), demodulate, `iterations` levels — a 3 x 3 blur of the variance at unit spacing, then the 5 x 5 taps
of denoise_ref.denoise with the squared luminance difference over sigma_color^2 times that blurred variance as the colour
term, the variance filtered along with the colour by the squared weights — and remodulate.  Every constant is computed in
double and rounded to the dtype once; every + - * / below is one operation of the dtype.  Also the sampled planes the CPU
and GPU tests share."""
import numpy as np

from denoise_ref import H, planes

G = (0.5, 0.25)  # the 3 x 3 blur of the variance, exact in binary
DEFAULTS = dict(iterations=5, keep_albedo=False, sigma_color=4.0, sigma_normal=0.3, sigma_depth=0.05, albedo_floor=1e-3)


def initial_variance(count, m1, m2):
    """the variance of the pixel mean, float64: the operations of the adaptive rule; a single sample counts as 100 %
    relative error; count <= 0 gives 0 / 0 = NaN"""
    count = np.asarray(count, np.int32)
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    with np.errstate(all="ignore"):
        n = count.astype(np.float64)
        mean = m1 / n
        v = m2 / n - mean * mean
        v = np.where(v > 0, v, 0.0)
        return np.where(count >= 2, v / (n - 1), mean * mean)


def _offsets(h, w, oy, ox):
    """the slices of the pixels whose tap at offset (oy, ox) is inside the image, and of those taps; None: there are none"""
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def denoise_variance(rgb, count, m1, m2, albedo=None, normal=None, depth=None, dtype=None, variance=False, **opts):
    """rgb (H, W, 3), count int32 / m1, m2 float64 (H, W), optional guides albedo / normal (H, W, 3) and depth (H, W)
    -> (H, W, 3) of `dtype` (default: rgb's), with variance=True -> (image, variance_out (H, W)); options as DEFAULTS
    (a value <= 0 takes the default, as in TakeDenoiseOpts)"""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in opts.items() if k == "keep_albedo" or v > 0})
    assert set(o) == set(DEFAULTS) and 1 <= o["iterations"] <= 8
    T = np.dtype(dtype or np.asarray(rgb).dtype).type
    C = np.array(rgb, T)
    V = initial_variance(count, m1, m2).astype(T)
    N = None if normal is None else np.array(normal, T)
    Z = None if depth is None else np.array(depth, T)
    h, w = C.shape[:2]
    demod = albedo is not None and not o["keep_albedo"]
    with np.errstate(over="ignore"):  # (a colour term that overflows to +inf is the specified outcome: weight 0)
        if demod:
            A = np.fmax(np.array(albedo, T), T(o["albedo_floor"]))
            C = C / A
            Am = ((A[..., 0] + A[..., 1]) + A[..., 2]) * T(1.0 / 3.0)
            V = V / (Am * Am)
        sl2 = T(o["sigma_color"] * o["sigma_color"])
        inv_n, inv_d = T(1.0 / (o["sigma_normal"] * o["sigma_normal"])), T(1.0 / (o["sigma_depth"] * o["sigma_depth"]))
        tiny = np.finfo(T).tiny
        for i in range(o["iterations"]):
            s = 1 << i
            gn, gd = np.zeros((h, w), T), np.zeros((h, w), T)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    pq = _offsets(h, w, dy, dx)
                    if pq is None:
                        continue
                    P, Q = pq
                    k3 = T(G[abs(dx)]) * T(G[abs(dy)])
                    gn[P] += k3 * V[Q]
                    gd[P] += k3
            gv = gn / gd
            inv_c = T(1) / (sl2 * gv + tiny)
            L = (C[..., 0] + C[..., 1]) + C[..., 2]
            num, nv, den = np.zeros_like(C), np.zeros((h, w), T), np.zeros((h, w), T)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = _offsets(h, w, s * dy, s * dx)
                    if pq is None:
                        continue  # every tap of this offset is outside
                    P, Q = pq
                    k = T(H[abs(dx)]) * T(H[abs(dy)])
                    dl = L[P] - L[Q]
                    x = (dl * dl) * inv_c[P]
                    if N is not None:
                        dn = N[P] - N[Q]
                        x = x + ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) * inv_n
                    if Z is not None:
                        m = np.fmax(np.fmax(np.abs(Z[P]), np.abs(Z[Q])), tiny)
                        r = (Z[P] - Z[Q]) / m
                        x = x + (r * r) * inv_d
                    wgt = k * np.exp(-x)
                    num[P] += wgt[..., None] * C[Q]
                    nv[P] += (wgt * wgt) * V[Q]
                    den[P] += wgt
            C = num / den[..., None]
            V = nv / (den * den)
        out = C * A if demod else C
        vout = V * (Am * Am) if demod else V
    assert out.dtype == T and vout.dtype == T
    return (out, vout) if variance else out


# ------------------------------------------------------------------ the sampled planes of the tests
NMAX = 16


def moments(samples, count):
    """samples (n, H, W, 3) float64, count (H, W) -> rgb (the mean of each pixel's first `count` samples), m1, m2 (the
    sums of L_s = (r + g) + b and of L_s * L_s over them, in sample order)"""
    n = samples.shape[0]
    used = (np.arange(n)[:, None, None] < count[None]).astype(np.float64)
    rgb = np.zeros(samples.shape[1:])
    m1, m2 = np.zeros(count.shape), np.zeros(count.shape)
    for s in range(n):
        L = (samples[s, ..., 0] + samples[s, ..., 1]) + samples[s, ..., 2]
        rgb += samples[s] * used[s][..., None]
        m1 += L * used[s]
        m2 += (L * L) * used[s]
    return rgb / count[..., None], m1, m2


def sampled_planes(width, height, variant=False):
    """denoise_ref.planes as a sampler would deliver them: per pixel NMAX samples clean * (1 + amp * u), u uniform in
    [-1, 1] per sample and channel, amp 0.9 left of the region edge and 0.1 right of it; count is 4 where (x + y) % 3 ==
    0, else 16 on the right and 8 on the left; the first `count` samples give rgb, m1, m2.  variant: count 1 in one
    column and m2 = m1^2 / n (zero variance) in one block of rows, so that both branches of the initial variance run.
    -> dict of float64 rgb, albedo, normal, depth, clean and int32 count, float64 m1, m2"""
    p = planes(width, height)
    y, x = np.mgrid[0:height, 0:width]
    right = x >= (9 * width) // 20
    amp = np.where(right, 0.1, 0.9)
    u = np.random.default_rng(1).uniform(-1.0, 1.0, (NMAX, height, width, 3))
    samples = p["clean"][None] * (1.0 + amp[None, ..., None] * u)
    count = np.where((x + y) % 3 == 0, 4, np.where(right, 16, 8)).astype(np.int32)
    if variant:
        count[:, width // 3] = 1
    rgb, m1, m2 = moments(samples, count)
    if variant:
        rows = slice(height // 2, height // 2 + max(1, height // 8))
        m2[rows] = m1[rows] * m1[rows] / count[rows]
    return {"rgb": rgb, "albedo": p["albedo"], "normal": p["normal"], "depth": p["depth"], "clean": p["clean"], "count": count, "m1": m1, "m2": m2}


def edge_planes(width, height):
    """the low-noise edge: a flat grey plane, no guides, illumination 1.0 for x < width // 2 and 1.2 otherwise in all
    three channels, NMAX samples 1 + 0.02 u with one u per sample and pixel -> dict of rgb, clean, count, m1, m2"""
    y, x = np.mgrid[0:height, 0:width]
    clean = np.repeat(np.where(x < width // 2, 1.0, 1.2)[..., None], 3, -1)
    u = np.random.default_rng(3).uniform(-1.0, 1.0, (NMAX, height, width))
    samples = clean[None] * (1.0 + 0.02 * u)[..., None]
    count = np.full((height, width), NMAX, np.int32)
    rgb, m1, m2 = moments(samples, count)
    return {"rgb": rgb, "clean": clean, "count": count, "m1": m1, "m2": m2}


def cast(p, dtype):
    """the input planes that are there, contiguous: the image and the guides in `dtype`, count int32, the moments float64"""
    out = {k: np.ascontiguousarray(p[k], dtype) for k in ("rgb", "albedo", "normal", "depth") if k in p}
    out["count"] = np.ascontiguousarray(p["count"], np.int32)
    out["m1"], out["m2"] = np.ascontiguousarray(p["m1"], np.float64), np.ascontiguousarray(p["m2"], np.float64)
    return out

"""The display transform (include/take_hip.h: take_hip_luminance_histogram*, take_hip_auto_exposure, take_hip_tonemap*;
DESIGN.md §4j) restated in numpy, operation by operation in the image's own dtype: the single source of the expected
values of tests/test_display_cpu.py and tests/test_gpu_display.py.  Every + - * / below is one numpy operation on
arrays (or scalars) of np.float32 / np.float64, in the order take_amd/csrc/tk_display.h writes them, so that the f32
restatement can be compared bit for bit; pow is numpy's.  Also the images the tests use (made from a seed, never
written to)."""
import numpy as np

BINS, SLOTS = 384, 386
NONPOSITIVE, NONFINITE = 384, 385
LINEAR, REINHARD, ACES = 0, 1, 2  # TAKE_TONEMAP_*
SRGB, TRANSFER_LINEAR = 0, 1  # TAKE_TRANSFER_*
OPS = {"linear": LINEAR, "reinhard": REINHARD, "aces": ACES}
# mirrored from include/take_hip.h (tests/test_display_cpu.py compares the three places)
DEFAULTS = {"key": 0.18, "low_fraction": 0.05, "high_fraction": 0.95, "min_exposure": 2.0 ** -16, "max_exposure": 2.0 ** 16, "rate": 1.0,
            "white": 4.0}


# ------------------------------------------------------------------ luminance, bin, histogram
def luminance(rgb):
    t = rgb.dtype.type
    with np.errstate(all="ignore"):
        return ((t(0.2126) * rgb[..., 0]) + (t(0.7152) * rgb[..., 1])) + (t(0.0722) * rgb[..., 2])


def luminance_slots(y):
    """luminances, float32 or float64 -> their slots, int64"""
    with np.errstate(all="ignore"):
        yf = np.ascontiguousarray(np.asarray(y).astype(np.float32))
    k = (yf.view(np.uint32) >> 20).astype(np.int64) - 8 * (127 - 24)
    out = np.clip(k, 0, BINS - 1)
    out[yf <= 0] = NONPOSITIVE
    out[~np.isfinite(yf)] = NONFINITE  # (after the line above: -inf <= 0)
    return out


def slots(rgb):
    """(..., 3) float32 or float64 -> the slot of every pixel, int64"""
    return luminance_slots(luminance(rgb))


def histogram(rgb):
    return np.bincount(slots(rgb).ravel(), minlength=SLOTS).astype(np.int64)


# ------------------------------------------------------------------ auto-exposure (double)
def bin_log2(b):
    """the representative log2 luminance of bin b"""
    return np.float64(b // 8 - 24) + np.log2(np.float64(1.0) + (np.float64(b % 8) + 0.5) / 8.0)


def exposure_target(hist, key=DEFAULTS["key"], low_fraction=DEFAULTS["low_fraction"], high_fraction=DEFAULTS["high_fraction"]):
    n = int(np.asarray(hist[:BINS], np.int64).sum())
    if n == 0:
        return np.float64(1.0)
    a, z = np.float64(low_fraction) * np.float64(n), np.float64(high_fraction) * np.float64(n)
    sw = swl = sn = snl = np.float64(0.0)
    cum = 0
    for b in range(BINS):
        c0 = np.float64(cum)
        cum += int(hist[b])
        c1 = np.float64(cum)
        w = max(np.float64(0.0), min(c1, z) - max(c0, a))
        l = bin_log2(b)
        sw, swl = sw + w, swl + w * l
        sn, snl = sn + np.float64(int(hist[b])), snl + np.float64(int(hist[b])) * l
    mean = swl / sw if sw > 0 else snl / sn
    return np.float64(key) / np.exp2(mean)


def auto_exposure(hist, key=DEFAULTS["key"], low_fraction=DEFAULTS["low_fraction"], high_fraction=DEFAULTS["high_fraction"],
                  min_exposure=DEFAULTS["min_exposure"], max_exposure=DEFAULTS["max_exposure"], prev_exposure=None, rate=DEFAULTS["rate"]):
    e = exposure_target(hist, key, low_fraction, high_fraction)
    if prev_exposure is not None and prev_exposure > 0:
        lp = np.log2(np.float64(prev_exposure))
        e = np.exp2(lp + np.float64(rate) * (np.log2(e) - lp))
    return float(min(max(e, np.float64(min_exposure)), np.float64(max_exposure)))


# ------------------------------------------------------------------ operators, transfer, quantisation
def tone(c, exposure, op=ACES, transfer=SRGB, white=DEFAULTS["white"]):
    """c: an array of channel values (any shape) -> y in [0, 1], same dtype"""
    t = c.dtype.type
    with np.errstate(all="ignore"):
        x = c * t(exposure)
        x = np.where(x > 0, x, t(0))
        x = np.minimum(x, t(65504))
        if op == REINHARD:
            y = x * (t(1) + x * t(1.0 / (white * white))) / (t(1) + x)
        elif op == ACES:
            y = (x * (t(2.51) * x + t(0.03))) / (x * (t(2.43) * x + t(0.59)) + t(0.14))
        else:
            y = x
        y = np.minimum(y, t(1))
        if transfer == SRGB:
            y = np.where(y <= t(0.0031308), t(12.92) * y, t(1.055) * np.power(y, t(1.0 / 2.4)) - t(0.055))
    assert y.dtype == c.dtype
    return y


def unrounded(y):
    """y * 255 + 0.5, what the 8-bit code truncates"""
    t = y.dtype.type
    return y * t(255) + t(0.5)


def codes(y):
    return unrounded(y).astype(np.int32).astype(np.uint8)


def rgba(rgb, exposure, **kw):
    """(H, W, 3) -> uint8 (H, W, 4): the codes, alpha 255"""
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = codes(tone(rgb, exposure, **kw))
    return out


# ------------------------------------------------------------------ the bars of the sRGB branch
def allowance(dtype):
    """A = 16 ulp of 1.0: the library's pow plus the multiply and the subtract after it.  (The HIP documentation that
    comes with the toolchain states no bound for pow / powf, so A is not doubled.)"""
    return 2.0 ** -20 if np.dtype(dtype) == np.float32 else 2.0 ** -49


MAX_NEAR_SHARE = 0.005  # of all channels: may lie within 255 A of a rounding boundary / may differ by one code


def near_integer(y):
    """channels whose unrounded y * 255 + 0.5 lies within 255 A of an integer: where a code may differ by one"""
    u = unrounded(y).astype(np.float64)
    return np.abs(u - np.rint(u)) <= 255.0 * allowance(y.dtype)


def restated_srgb(rgb, exposure, **kw):
    """-> (y, the mask of near_integer), after asserting — on the restatement alone — that the mask is small enough to
    keep the comparison of the codes honest"""
    y = tone(rgb, exposure, transfer=SRGB, **kw)
    near = near_integer(y)
    share = float(near.mean())
    print(f"channels within 255 A of a rounding boundary: {share:.2e} of {near.size}")
    assert share <= MAX_NEAR_SHARE, share
    return y, near


def check_srgb_real(got, y, label):
    d = float(np.abs(got.astype(np.float64) - y.astype(np.float64)).max())
    print(f"{label}: max |difference| {d:.3e}, bar {allowance(y.dtype):.3e}")
    assert got.dtype == y.dtype and np.isfinite(got).all() and d <= allowance(y.dtype), (label, d)


def check_srgb_codes(got, y, near, label):
    """got: uint8 (H, W, 4)"""
    want = codes(y)
    diff = got[..., :3].astype(np.int32) - want.astype(np.int32)
    differing = diff != 0
    print(f"{label}: {int(differing.sum())} of {differing.size} codes differ, all by at most {int(np.abs(diff).max())}")
    assert (got[..., 3] == 255).all(), label
    assert np.abs(diff).max() <= 1, label
    assert not (differing & ~near).any(), label
    assert differing.mean() <= MAX_NEAR_SHARE, label


# ------------------------------------------------------------------ the tests' images
def log_uniform(width, height, dtype, seed, lo=-30.0, hi=30.0):
    """luminance 2^u, u uniform over [lo, hi], with a random hue; every value a normal float"""
    rng = np.random.default_rng(seed)
    hue = rng.uniform(0.05, 1.0, (height, width, 3))
    hue /= (hue * np.array([0.2126, 0.7152, 0.0722])).sum(-1, keepdims=True)
    return np.ascontiguousarray((hue * np.exp2(rng.uniform(lo, hi, (height, width, 1)))).astype(dtype))


def midrange(width, height, dtype, seed):
    """the same over the 14 octaves a display shows at exposure 1: what exercises the operators and the transfer"""
    return log_uniform(width, height, dtype, seed, -11.0, 3.0)


def constant(width, height, dtype, value=(0.25, 0.5, 0.125)):
    return np.ascontiguousarray(np.broadcast_to(np.array(value, dtype), (height, width, 3)))


# The shapes of tests/test_gpu_display.py (width, height): one pixel; under one wave; a wave plus one; a block plus one;
# many blocks with a ragged end; and more pixels (614400) than the capped launch has threads (2048 blocks x 256), so
# that the grid-stride loops go round twice
SHAPES = [(1, 1), (7, 3), (65, 5), (257, 3), (641, 97), (1024, 600)]
CONTENTS = ("log-uniform", "midrange", "constant", "salted")
_IMAGES = {}


def image(content, shape, dtype):
    """the tests' image of that content, shape (width, height) and dtype: made once, never written to"""
    key = (content, tuple(shape), np.dtype(dtype).name)
    if key not in _IMAGES:
        w, h = shape
        seed = 1000 + 7 * w + h
        img = {"log-uniform": lambda: log_uniform(w, h, dtype, seed), "midrange": lambda: midrange(w, h, dtype, seed),
               "constant": lambda: constant(w, h, dtype), "salted": lambda: salted(w, h, dtype, seed)}[content]()
        img.setflags(write=False)
        _IMAGES[key] = img
    return _IMAGES[key]


def salted(width, height, dtype, seed):
    """log_uniform with every fifth channel value (at least the first nine) replaced by NaN, +Inf, -Inf, negatives, either
    zero and — in float64 — values beyond float's range"""
    img = log_uniform(width, height, dtype, seed)
    salt = [np.nan, np.inf, -np.inf, -1.0, -2.5e-3, 0.0, -0.0, 3.0e4, 7.0e4]
    if np.dtype(dtype) == np.float64:
        salt += [1e300, -1e300, 1e39, 3.5e38, 1e-300]
    rng = np.random.default_rng(seed + 1)
    flat = img.reshape(-1)
    n = max(len(salt), flat.size // 5) if flat.size >= len(salt) else flat.size
    where = rng.choice(flat.size, n, replace=False)
    flat[where] = np.resize(np.array(salt, dtype), n)
    return img

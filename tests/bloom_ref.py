"""Bloom for the display transform (include/take_hip.h: take_hip_bloom_layer*, take_hip_tonemap_bloom*)
restated in numpy, operation by operation in the image's own dtype: the single source of the expected values of
tests/test_bloom_cpu.py and tests/test_gpu_bloom.py.  Every + - * / below is one numpy operation on arrays of
np.float32 / np.float64, in the order take_amd/csrc/tk_bloom.h writes them — the orders of additions it fixes are
restated in `mean4`, `down` and `up` — so that the restatement can be compared bit for bit.  The tone operator, the
transfer and the bars of the sRGB branch are display_ref's.  Also the images the tests use (made from a seed, never
written to)."""
import numpy as np

import display_ref as dref

MAX_LEVELS = 8
# mirrored from include/take_hip.h (tests/test_bloom_cpu.py compares the three places)
DEFAULTS = {"threshold": 1.0, "knee": 0.5, "intensity": 0.25}


# ------------------------------------------------------------------ step 3: the pyramid's sizes
def pyramid(width, height, levels=0):
    """-> [(w, h)] of the levels: the ceil-halvings of the image until both axes are 1, at most MAX_LEVELS, and at most
    `levels` if that is positive"""
    cap = min(levels, MAX_LEVELS) if levels > 0 else MAX_LEVELS
    out = []
    while len(out) < cap:
        width, height = (width + 1) // 2, (height + 1) // 2
        out.append((width, height))
        if width == 1 and height == 1:
            break
    return out


# ------------------------------------------------------------------ steps 1 and 2: exposed pixel, bright pass
def exposed(rgb, exposure):
    t = rgb.dtype.type
    with np.errstate(all="ignore"):
        x = rgb * t(exposure)
        x = np.where(x > 0, x, t(0))
        return np.minimum(x, t(65504))


def bright(x, threshold, knee):
    """x: exposed (H, W, 3) -> b"""
    t = x.dtype.type
    th, k = t(threshold), t(knee)
    with np.errstate(all="ignore"):
        Y = dref.luminance(x)
        s = Y - (th - k)
        s = np.minimum(np.maximum(s, t(0)), t(2) * k)
        s = (s * s) / (t(4) * k) if k > 0 else np.zeros_like(Y)
        m = np.maximum(s, Y - th)
        w = np.where(m > 0, m / Y, t(0))
    assert w.dtype == x.dtype
    return x * w[..., None]


# ------------------------------------------------------------------ step 4: the 13-tap downsample
def mean4(s00, s01, s10, s11):
    return ((s00 + s11) + (s01 + s10)) * s00.dtype.type(0.25)


def down(src):
    """(h, w, 3) -> (ceil(h / 2), ceil(w / 2), 3)"""
    t = src.dtype.type
    sh, sw = src.shape[:2]
    dh, dw = (sh + 1) // 2, (sw + 1) // 2
    rows = [np.clip(2 * np.arange(dh) - 2 + i, 0, sh - 1) for i in range(6)]
    cols = [np.clip(2 * np.arange(dw) - 2 + j, 0, sw - 1) for j in range(6)]

    def v(i, j):
        return src[rows[i][:, None], cols[j][None, :]]

    def M(i, j):
        return mean4(v(i, j), v(i, j + 1), v(i + 1, j), v(i + 1, j + 1))

    B = [[M(2 * a, 2 * b) for b in range(3)] for a in range(3)]
    C = [[M(1 + 2 * a, 1 + 2 * b) for b in range(2)] for a in range(2)]
    centre = t(0.125) * ((C[0][0] + C[1][1]) + (C[0][1] + C[1][0])) + t(0.125) * B[1][1]
    out = (centre + t(0.0625) * ((B[0][1] + B[2][1]) + (B[1][0] + B[1][2]))) + t(0.03125) * ((B[0][0] + B[2][2]) + (B[0][2] + B[2][0]))
    assert out.dtype == src.dtype and out.shape == (dh, dw, 3)
    return out


# ------------------------------------------------------------------ step 5: the bilinear upsample
def near_far(n_dst, n_src):
    x = np.arange(n_dst)
    near = x // 2
    far = np.where(x % 2 == 1, np.minimum(near + 1, n_src - 1), np.maximum(near - 1, 0))
    return near, far


def up(src, width, height):
    """(sh, sw, 3), the ceil-halving of (height, width) -> (height, width, 3)"""
    t = src.dtype.type
    sh, sw = src.shape[:2]
    assert (sw, sh) == ((width + 1) // 2, (height + 1) // 2)
    nx, fx = near_far(width, sw)
    ny, fy = near_far(height, sh)
    nn, nf = src[ny[:, None], nx[None, :]], src[ny[:, None], fx[None, :]]
    fn, ff = src[fy[:, None], nx[None, :]], src[fy[:, None], fx[None, :]]
    return (t(0.5625) * nn + t(0.0625) * ff) + (t(0.1875) * nf + t(0.1875) * fn)


# ------------------------------------------------------------------ steps 1 to 6
def resolved(threshold=None, knee=None, intensity=None, levels=0):
    d = DEFAULTS
    return (d["threshold"] if threshold is None else threshold, d["knee"] if knee is None else knee,
            d["intensity"] if intensity is None else intensity, levels)


def u0_and_gain(rgb, exposure, threshold=None, knee=None, intensity=None, levels=0):
    """-> (x: the exposed image, U_0, gain in the image's dtype)"""
    threshold, knee, intensity, levels = resolved(threshold, knee, intensity, levels)
    h, w = rgb.shape[:2]
    sizes = pyramid(w, h, levels)
    x = exposed(rgb, exposure)
    D = [down(bright(x, threshold, knee))]
    for _ in sizes[1:]:
        D.append(down(D[-1]))
    assert [(d.shape[1], d.shape[0]) for d in D] == sizes
    U = D[-1]
    for k in range(len(D) - 2, -1, -1):
        U = D[k] + up(U, D[k].shape[1], D[k].shape[0])
    return x, U, rgb.dtype.type(np.float64(intensity) / np.float64(len(sizes)))


def layer(rgb, exposure, **bloom):
    """the full-resolution layer of step 6, (H, W, 3) of rgb's dtype"""
    _, U, gain = u0_and_gain(rgb, exposure, **bloom)
    out = gain * up(U, rgb.shape[1], rgb.shape[0])
    assert out.dtype == rgb.dtype
    return out


def tail(x, op=dref.ACES, transfer=dref.SRGB, white=dref.DEFAULTS["white"]):
    """display_ref.tone from its min(x, 65504) onward, on x >= 0: exposure 1 changes nothing of such an x"""
    return dref.tone(x, 1.0, op=op, transfer=transfer, white=white)


def composite_input(rgb, exposure, **bloom):
    """x' = x + layer: what the tail of the tone pass is given (a test that compares several operators makes it once)"""
    x, U, gain = u0_and_gain(rgb, exposure, **bloom)
    return x + gain * up(U, rgb.shape[1], rgb.shape[0])


def tone(rgb, exposure, op=dref.ACES, transfer=dref.SRGB, white=dref.DEFAULTS["white"], **bloom):
    """the composite -> y in [0, 1], (H, W, 3) of rgb's dtype"""
    return tail(composite_input(rgb, exposure, **bloom), op, transfer, white)


def rgba(rgb, exposure, **kw):
    out = np.full(rgb.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = dref.codes(tone(rgb, exposure, **kw))
    return out


def restated_srgb(rgb, exposure, **kw):
    """display_ref.restated_srgb for the composite: -> (y, the mask of near_integer), after asserting — on the
    restatement alone — that at most 0.5 % of the channels lie within 255 A of a rounding boundary"""
    y = tone(rgb, exposure, transfer=dref.SRGB, **kw)
    near = dref.near_integer(y)
    share = float(near.mean())
    print(f"channels within 255 A of a rounding boundary: {share:.2e} of {near.size}")
    assert share <= dref.MAX_NEAR_SHARE, share
    return y, near


# ------------------------------------------------------------------ the tests' images
# The shapes of tests/test_gpu_bloom.py (width, height): levels of size 1, odd sizes and clamps on every side; one
# 16 x 16 tile plus a sliver; 130 x 70 — level 0 is 65 x 35: several tiles, halos crossing tile borders, a partial last
# tile on both axes; a long thin one; and one with many tiles
SHAPES = [(1, 1), (2, 2), (3, 5), (7, 3), (33, 17), (65, 5), (130, 70), (257, 3), (641, 97)]
CONTENTS = ("log-uniform", "below", "above", "corner", "centre", "border", "salted")
_IMAGES = {}


def impulse(width, height, dtype, at, value=(40.0, 30.0, 20.0), floor=0.0):
    img = np.full((height, width, 3), floor, dtype)
    img[min(at[1], height - 1), min(at[0], width - 1)] = value
    return img


def image(content, shape, dtype):
    """the tests' image of that content, shape (width, height) and dtype: made once, never written to.  "below" and
    "above": constants below t - k and above t of the defaults at exposure 1; the impulses: one bright pixel on black at
    a corner, at the centre, and at (32, 32) — where four tiles of level 0's staging meet"""
    key = (content, tuple(shape), np.dtype(dtype).name)
    if key not in _IMAGES:
        w, h = shape
        seed = 2000 + 7 * w + h
        img = {"log-uniform": lambda: dref.log_uniform(w, h, dtype, seed), "salted": lambda: dref.salted(w, h, dtype, seed),
               "midrange": lambda: dref.midrange(w, h, dtype, seed),
               "below": lambda: dref.constant(w, h, dtype, (0.25, 0.5, 0.125)), "above": lambda: dref.constant(w, h, dtype, (3.0, 2.0, 5.0)),
               "corner": lambda: impulse(w, h, dtype, (w - 1, 0)), "centre": lambda: impulse(w, h, dtype, (w // 2, h // 2)),
               "border": lambda: impulse(w, h, dtype, (32, 32))}[content]()
        img = np.ascontiguousarray(img)
        img.setflags(write=False)
        _IMAGES[key] = img
    return _IMAGES[key]


# the option sets of the tests: the defaults; no knee; no threshold (everything blooms); one, three and all levels
OPTION_SETS = {"defaults": {}, "knee 0": dict(knee=0.0), "threshold 0": dict(threshold=0.0, knee=0.0), "levels 1": dict(levels=1),
               "levels 3": dict(levels=3), "levels 8": dict(levels=MAX_LEVELS)}

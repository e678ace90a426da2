"""numpy restatement of the adaptive sampler's rule (include/take_hip.h: take_hip_render_adaptive; DESIGN.md §4g;
the text the device runs: take_amd/csrc/tk_adaptive.h).  TEST INFRASTRUCTURE: every operation below is one IEEE double
operation in the order the header states, so the results are comparable bit for bit."""
import numpy as np

DEFAULTS = {"min_spp": 16, "step_spp": 8, "threshold": 0.05, "floor": 1e-3}


def resolve(spp, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0):
    """the options with the defaults filled in, min_spp clamped to spp"""
    o = dict(DEFAULTS)
    if min_spp > 0:
        o["min_spp"] = int(min_spp)
    if step_spp > 0:
        o["step_spp"] = int(step_spp)
    if threshold >= 0:
        o["threshold"] = float(threshold)
    if floor > 0:
        o["floor"] = float(floor)
    o["min_spp"] = min(o["min_spp"], int(spp))
    return o


def sample_value(rgb):
    """L_s of samples (..., 3): ((double)r + (double)g) + (double)b"""
    c = np.asarray(rgb).astype(np.float64)
    return (c[..., 0] + c[..., 1]) + c[..., 2]


def moments(values):
    """(m1, m2) of the sample values (n, ...) added in sample order"""
    v = np.asarray(values, np.float64)
    m1, m2 = np.zeros(v.shape[1:]), np.zeros(v.shape[1:])
    for s in range(v.shape[0]):
        m1 = m1 + v[s]
        m2 = m2 + v[s] * v[s]
    return m1, m2


def rel_error(n, m1, m2, floor):
    """the relative standard error of the mean after n samples (n: scalar or array)"""
    n = np.asarray(n, np.float64)
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    with np.errstate(all="ignore"):
        mean = m1 / n
        v = m2 / n - mean * mean
        v = np.where(v > 0, v, 0.0)
        return np.sqrt(v / (n - 1.0)) / (np.abs(mean) + floor)


def stops(n, err, spp, threshold):
    """the stop decision (a NaN err never satisfies <=)"""
    n = np.asarray(n)
    with np.errstate(invalid="ignore"):
        return ((n >= 2) & (np.asarray(err) <= threshold)) | (n == spp)


def schedule(spp, min_spp, step_spp):
    """the counts a pixel can stop at: min_spp, then + min(step_spp, spp - n) up to spp"""
    out, n = [], min_spp
    while True:
        out.append(n)
        if n >= spp:
            return out
        n += min(step_spp, spp - n)


def compact(keep, pixels=None):
    """the next list: the kept entries of `pixels` (None: the identity) in their order"""
    keep = np.asarray(keep).astype(bool)
    src = np.arange(keep.size, dtype=np.int32) if pixels is None else np.asarray(pixels, np.int32)
    return src[keep]


def worklist(pixels, nb, npix):
    """slot of entry j < nb * len(pixels): sample-major, sample * npix + pixel"""
    pixels = np.asarray(pixels, np.int64)
    return (np.arange(nb, dtype=np.int64)[:, None] * npix + pixels[None, :]).reshape(-1)

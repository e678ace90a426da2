"""numpy restatement of the thin-lens camera ray (take_amd/csrc/tk_lens.h, lens_camera_ray in tk_integrate.h; DESIGN.md
par. 4k), in float64 and float32: every + - * / one operation of the dtype in the order the header writes it.  The
counter-based random stream is restated here in uint64 arithmetic (tests/test_lens_cpu.py holds it to
oracle.counter_words), because the lens draws sit at counters the oracle's helper would have to walk 2^32 words to
reach."""
import numpy as np

GOLDEN, SAMPLE_STEP = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD1B54A32D192ED03)
LENS_COUNTER = 0xFFFFFFFE


def rng_mix(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rng_key(seed, pixel, sample):
    """tk_common.h: rng_key; pixel = y * width + x with y = 0 the bottom row"""
    seed, pixel, sample = (np.asarray(v, np.uint64) for v in (seed, pixel, sample))
    with np.errstate(over="ignore"):
        return rng_mix(rng_mix(seed + GOLDEN * (pixel + np.uint64(1))) + SAMPLE_STEP * (sample + np.uint64(1)))


def counter_word(key, ctr):
    with np.errstate(over="ignore"):
        return rng_mix(np.asarray(key, np.uint64) + GOLDEN * np.asarray(ctr, np.uint64))


def real(word, dtype):
    """random_real<R>: the top 24 bits (float32) or the top 53 (float64)"""
    if dtype == np.float32:
        return (word >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (word >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _norm(v, T):
    l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((l <= 0)[..., None], T(0), v * (T(1) / l)[..., None])


def camera(sd, dtype, radius=0.0, focus=0.0):
    """make_camera (tk_host_scene.h) in dtype, with the lens as take_hip_scene_set_lens rounds it: focus <= 0 is
    |lookat - lookfrom| computed in double"""
    T = dtype
    h = np.tan(T(sd.vfov) / T(180) * T(np.pi) / T(2))
    vh = T(2) * h
    vw = vh / T(sd.height) * T(sd.width)
    origin, at, up = (np.asarray(v, np.float64).astype(T) for v in (sd.lookfrom, sd.lookat, sd.up))
    w = _norm(origin - at, T)
    u = _norm(np.cross(up, w).astype(T), T)
    v = np.cross(w, u).astype(T)
    look = float(np.sqrt(((np.asarray(sd.lookat, np.float64) - np.asarray(sd.lookfrom, np.float64)) ** 2).sum()))
    return {"u": u, "v": v, "w": w, "lookfrom": origin, "vw": T(vw), "vh": T(vh), "width": int(sd.width), "height": int(sd.height),
            "radius": T(radius), "focus": T(focus if focus > 0 else look)}


def camera_words(cam, dtype):
    """the 16 Reals tests/lens_host reads"""
    return np.concatenate([cam["u"], cam["v"], cam["w"], cam["lookfrom"], [cam["vw"], cam["vh"], cam["radius"], cam["focus"]]]).astype(dtype)


def concentric_disc(r1, r2, T):
    a, b = T(2) * r1 - T(1), T(2) * r2 - T(1)
    quarter, half = T(np.pi) / T(4), T(np.pi) / T(2)
    wide = np.abs(a) > np.abs(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(wide, a, b)
        phi = np.where(wide, quarter * (b / a), half - quarter * (a / b))
        x, y = r * np.cos(phi), r * np.sin(phi)
    zero = (a == 0) & (b == 0)
    return np.where(zero, T(0), x).astype(T), np.where(zero, T(0), y).astype(T)


def lens_rays(cam, spp, seed, dtype, first_sample=0):
    """-> dict of (H, W, spp, ...) arrays, image row 0 = top: o and d (the ray), off (the lens point - lookfrom), p (the
    pinhole direction before its normalise), sx, sy.  radius 0 gives o = lookfrom and d = normalize(p * focus)."""
    T = dtype
    W, H = cam["width"], cam["height"]
    rows, xs, ss = np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij")
    ys = H - 1 - rows  # the render loop's y: 0 = the bottom row
    key = rng_key(np.uint64(seed), (ys * W + xs).astype(np.uint64), (ss + first_sample).astype(np.uint64))
    ry, rx = real(counter_word(key, 0), T), real(counter_word(key, 1), T)  # y is drawn first
    sx = (xs.astype(T) + rx) / T(W) - T(0.5)
    sy = (ys.astype(T) + ry) / T(H) - T(0.5)
    u, v, w = cam["u"], cam["v"], cam["w"]
    p = (u * (sx * cam["vw"])[..., None] + v * (sy * cam["vh"])[..., None]) - w
    r1, r2 = real(counter_word(key, LENS_COUNTER), T), real(counter_word(key, LENS_COUNTER + 1), T)
    dx, dy = concentric_disc(r1, r2, T)
    lx, ly = cam["radius"] * dx, cam["radius"] * dy
    off = u * lx[..., None] + v * ly[..., None]
    o = cam["lookfrom"] + off
    d = _norm(p * cam["focus"] - off, T)
    out = {"o": o, "d": d, "off": off, "p": p, "sx": sx, "sy": sy}
    assert all(a.dtype == T for a in out.values())
    return out


def oracle_planes(sd, rays, spp, seed):
    """tests/test_gpu_features.py's expected_planes — hits from OracleScene.isect, planes summed in sample order — for
    `rays` ((H * W * spp, 8), the samples of a pixel adjacent) in place of its own pinhole camera rays"""
    import test_gpu_features as F

    saved = F.camera_rays
    F.camera_rays = lambda *_: rays
    try:
        return F.expected_planes(sd, spp, seed)
    finally:
        F.camera_rays = saved


def rays8(o, d, tmin):
    """(n, 8) org3 dir3 tmin tmax for OracleScene.isect, in the order of o's leading axes flattened"""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    n = o.shape[0]
    return np.concatenate([o, d, np.full((n, 1), tmin), np.full((n, 1), np.inf)], 1)

"""The image-space calls that need no scene (include/take_hip.h): the denoisers, temporal accumulation, the display
transform and bloom, on host arrays or on planes in device memory, and the workspace the display calls may keep."""
import ctypes as C

import numpy as np

from . import cdefs as D
from ._lib import _check, lib
from ._marshal import Handle, handle_of, pointer, ref


def _keyword_opts(make, opts, kw):
    """an options struct, keywords of `make` (cdefs.denoise_opts, cdefs.temporal_opts), or neither (None: the library's
    defaults, a NULL pointer)"""
    if kw and opts is not None:
        raise ValueError("give opts or keywords, not both")
    return make(**kw) if kw else opts


def _precision(dtype):
    return D.TAKE_PRECISION_F32 if dtype == np.float32 else D.TAKE_PRECISION_F64


def _image(img, name="the image"):
    """a host image as the image-space calls take it -> (contiguous (H, W, 3) array, its TAKE_PRECISION_*)"""
    img = np.asarray(img)
    if img.dtype not in (np.float32, np.float64) or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"{name} must be a (H, W, 3) float32 or float64 array")
    return np.ascontiguousarray(img), _precision(img.dtype)


def _rgb_and_guides(rgb, albedo, normal, depth):
    """host arrays as denoise() takes them -> (contiguous rgb, its TAKE_PRECISION_*, a TakeFeatureBuffers over the guides that
    were given, the arrays it points into: empty = no guides)"""
    rgb, precision = _image(rgb, "rgb")
    h, w = rgb.shape[:2]
    bufs, keep = D.TakeFeatureBuffers(), []
    for name, a, shape in (("albedo", albedo, (h, w, 3)), ("normal", normal, (h, w, 3)), ("depth", depth, (h, w))):
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        if a.dtype != rgb.dtype or a.shape != shape:
            raise ValueError(f"{name} must be a {shape} array of rgb's dtype")
        keep.append(a)
        setattr(bufs, name, a.ctypes.data)
    return rgb, precision, bufs, keep


def _device_guides(albedo, normal, depth):
    return D.TakeFeatureBuffers(pointer(albedo), pointer(normal), pointer(depth), None, None, None)


def denoise(rgb, albedo=None, normal=None, depth=None, opts=None, **kw):
    """the image-space denoiser on host arrays (take_hip_denoise: the edge-avoiding A-trous filter, include/take_hip.h):
    rgb (H, W, 3) float32 or float64 — the dtype picks the precision —, the optional guides albedo and normal (H, W, 3)
    and depth (H, W) in the same dtype -> the filtered (H, W, 3) image.  Options: keywords of cdefs.denoise_opts
    (iterations, keep_albedo, sigma_color, sigma_normal, sigma_depth, albedo_floor), or opts = a TakeDenoiseOpts;
    neither = the library's defaults (a NULL pointer)."""
    rgb, precision, bufs, keep = _rgb_and_guides(rgb, albedo, normal, depth)
    h, w = rgb.shape[:2]
    opts = _keyword_opts(D.denoise_opts, opts, kw)
    out = np.zeros_like(rgb)
    _check(lib().take_hip_denoise(rgb.ctypes.data, C.byref(bufs) if keep else None, precision, w, h, ref(opts), out.ctypes.data))
    return out


def denoise_device(rgb, width, height, precision, out=None, albedo=None, normal=None, depth=None, opts=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_denoise_device): rgb, out and the guides are torch device tensors or
    integer device pointers of `precision`'s Real (TAKE_PRECISION_F32 / _F64); out = None filters in place; blocks until
    done.  Needs no scene: also for what render_accumulate or a scene group left on the device."""
    bufs = _device_guides(albedo, normal, depth)
    opts = _keyword_opts(D.denoise_opts, opts, kw)
    _check(lib().take_hip_denoise_device(C.c_void_p(pointer(rgb)), C.byref(bufs), int(precision), int(width), int(height), ref(opts),
                                         C.c_void_p(pointer(rgb if out is None else out)), C.c_void_p(stream or 0)))


def denoise_variance(rgb, count, m1, m2, albedo=None, normal=None, depth=None, variance=False, opts=None, **kw):
    """the variance-guided denoiser on host arrays (take_hip_denoise_variance: the A-trous filter with the pixel's own
    standard deviation as its colour sigma, include/take_hip.h): rgb and the guides as denoise() takes them, and the three
    planes an adaptive render leaves (Scene.render_adaptive(stats=True)): count (H, W) int32, m1 and m2 (H, W) float64
    -> the filtered (H, W, 3) image; variance=True: -> (image, the filter's (H, W) estimate of the variance of the
    result's r + g + b, in rgb's dtype).  Options as denoise(), but sigma_color (default 4.0) counts standard deviations."""
    rgb, precision, bufs, keep = _rgb_and_guides(rgb, albedo, normal, depth)
    h, w = rgb.shape[:2]
    stats, moments = D.TakeAdaptiveStats(), []
    for name, a, dtype in (("count", count, np.int32), ("m1", m1, np.float64), ("m2", m2, np.float64)):
        a = None if a is None else np.ascontiguousarray(a)
        if a is None or a.dtype != dtype or a.shape != (h, w):
            raise ValueError(f"{name} must be a {(h, w)} {np.dtype(dtype).name} array")
        moments.append(a)
        setattr(stats, name, a.ctypes.data)
    opts = _keyword_opts(D.denoise_opts, opts, kw)
    out = np.zeros_like(rgb)
    var = np.zeros((h, w), rgb.dtype) if variance else None
    _check(lib().take_hip_denoise_variance(rgb.ctypes.data, C.byref(bufs) if keep else None, C.byref(stats), precision, w, h, ref(opts), out.ctypes.data,
                                           None if var is None else var.ctypes.data))
    return (out, var) if variance else out


def denoise_variance_device(rgb, count, m1, m2, width, height, precision, out=None, albedo=None, normal=None, depth=None, variance=None, opts=None,
                            stream=None, **kw):
    """the same on planes in device memory (take_hip_denoise_variance_device): rgb, out, the guides and variance (the
    optional output plane) are torch device tensors or integer device pointers of `precision`'s Real, count int32, m1 and
    m2 float64; out = None filters in place; blocks until done.  Needs no scene."""
    bufs = _device_guides(albedo, normal, depth)
    stats = D.TakeAdaptiveStats(pointer(count), pointer(m1), pointer(m2))
    opts = _keyword_opts(D.denoise_opts, opts, kw)
    _check(lib().take_hip_denoise_variance_device(C.c_void_p(pointer(rgb)), C.byref(bufs), C.byref(stats), int(precision), int(width), int(height), ref(opts),
                                                  C.c_void_p(pointer(rgb if out is None else out)), C.c_void_p(pointer(variance)), C.c_void_p(stream or 0)))


STATS_PLANES = ("count", "m1", "m2")


def _host_stats(shape):
    """zeroed count / m1 / m2 host planes of `shape` -> ({name: array}, the TakeAdaptiveStats over them)"""
    planes = {"count": np.zeros(shape, np.int32), "m1": np.zeros(shape, np.float64), "m2": np.zeros(shape, np.float64)}
    return planes, D.TakeAdaptiveStats(*[planes[k].ctypes.data for k in STATS_PLANES])


def _device_stats(stats):
    """{"count" / "m1" / "m2": device tensor or pointer} for the planes wanted -> TakeAdaptiveStats; None or empty -> None"""
    if not stats:
        return None
    unknown = set(stats) - set(STATS_PLANES)
    if unknown:
        raise ValueError(f"unknown statistics plane {sorted(unknown)[0]!r}: one of ('count', 'm1', 'm2')")
    return D.TakeAdaptiveStats(*[pointer(stats.get(k)) for k in STATS_PLANES])


def _adaptive_opts(opts, min_spp, step_spp, threshold, floor):
    """opts = "keywords": the sampler's keywords as a TakeAdaptiveOpts; else opts itself (a TakeAdaptiveOpts, or None)"""
    return D.adaptive_opts(min_spp, step_spp, threshold, floor) if isinstance(opts, str) else opts


TEMPORAL_PLANES = ("rgb", "count", "m1", "m2", "depth", "shape_id")


def _known_temporal_planes(name, f):
    unknown = set(f) - set(TEMPORAL_PLANES)
    if unknown:
        raise ValueError(f"{name}: unknown plane {sorted(unknown)[0]!r}: one of {TEMPORAL_PLANES}")


def _temporal_frame(name, f, dtype, shape, keep):
    """{plane: host array} -> TakeTemporalFrame over contiguous arrays (kept alive in `keep`); rgb fixes dtype and shape"""
    _known_temporal_planes(name, f)
    h, w = shape
    want = {"rgb": (dtype, (h, w, 3)), "count": (np.int32, (h, w)), "m1": (np.float64, (h, w)), "m2": (np.float64, (h, w)),
            "depth": (dtype, (h, w)), "shape_id": (np.int32, (h, w))}
    out = D.TakeTemporalFrame()
    for k in TEMPORAL_PLANES:
        a = f.get(k)
        if a is None:
            if k in ("rgb", "count", "m1", "m2"):
                raise ValueError(f"{name}: {k} is required")
            continue
        a = np.ascontiguousarray(a)
        if a.dtype != want[k][0] or a.shape != want[k][1]:
            raise ValueError(f"{name}: {k} must be a {want[k][1]} {np.dtype(want[k][0]).name} array")
        keep.append(a)
        setattr(out, k, a.ctypes.data)
    return out


def temporal_accumulate(cur, hist, prev_xy, prev_depth=None, opts=None, **kw):
    """temporal accumulation on host arrays (take_hip_temporal_accumulate, include/take_hip.h): cur and hist are
    {"rgb": (H, W, 3) float32 or float64 — cur's dtype picks the precision —, "count": int32 (H, W), "m1", "m2": float64
    (H, W), and optionally "depth": (H, W) of rgb's dtype, "shape_id": int32 (H, W)}; hist = None: no history.  prev_xy
    (H, W, 2) and the optional prev_depth (H, W), of rgb's dtype, as Scene.render_motion leaves them -> the accumulated
    frame, a dict of the same planes (depth and shape_id where cur has them).  Options: keywords of cdefs.temporal_opts
    (max_history, depth_tol), or opts = a TakeTemporalOpts; neither = the library's defaults (a NULL pointer)."""
    rgb, precision = _image(cur.get("rgb") if isinstance(cur, dict) else None, "cur['rgb']")
    h, w = rgb.shape[:2]
    keep = []
    c = _temporal_frame("cur", cur, rgb.dtype, (h, w), keep)
    hf = None if hist is None else _temporal_frame("hist", hist, rgb.dtype, (h, w), keep)
    xy = None if prev_xy is None else np.ascontiguousarray(prev_xy)
    if xy is None or xy.dtype != rgb.dtype or xy.shape != (h, w, 2):
        raise ValueError(f"prev_xy must be a {(h, w, 2)} array of rgb's dtype")
    pd = None if prev_depth is None else np.ascontiguousarray(prev_depth)
    if pd is not None and (pd.dtype != rgb.dtype or pd.shape != (h, w)):
        raise ValueError(f"prev_depth must be a {(h, w)} array of rgb's dtype")
    opts = _keyword_opts(D.temporal_opts, opts, kw)
    out = {"rgb": np.zeros_like(rgb), "count": np.zeros((h, w), np.int32), "m1": np.zeros((h, w)), "m2": np.zeros((h, w))}
    if cur.get("depth") is not None:
        out["depth"] = np.zeros((h, w), rgb.dtype)
    if cur.get("shape_id") is not None:
        out["shape_id"] = np.zeros((h, w), np.int32)
    o = D.TakeTemporalFrame(*[out[k].ctypes.data if k in out else None for k in TEMPORAL_PLANES])
    _check(lib().take_hip_temporal_accumulate(C.byref(c), ref(hf), xy.ctypes.data, None if pd is None else pd.ctypes.data, precision, w, h, ref(opts),
                                              C.byref(o)))
    return out


def temporal_accumulate_device(cur, hist, prev_xy, prev_depth, width, height, precision, out=None, opts=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_temporal_accumulate_device): cur, hist (or None) and out are
    {plane: torch device tensor or integer device pointer}, prev_xy and prev_depth (or None) tensors or pointers, of
    `precision`'s Real (count and shape_id int32, m1 and m2 float64); out = None accumulates into cur's planes (out must
    never be hist: the taps gather); blocks until done.  Needs no scene."""
    def frame(name, f):
        _known_temporal_planes(name, f)
        return D.TakeTemporalFrame(*[pointer(f.get(k)) for k in TEMPORAL_PLANES])

    c = frame("cur", cur)
    hf = None if hist is None else frame("hist", hist)
    o = c if out is None else frame("out", out)
    opts = _keyword_opts(D.temporal_opts, opts, kw)
    _check(lib().take_hip_temporal_accumulate_device(C.byref(c), ref(hf), C.c_void_p(pointer(prev_xy)), C.c_void_p(pointer(prev_depth)),
                                                     int(precision), int(width), int(height), ref(opts), C.byref(o), C.c_void_p(stream or 0)))


def luminance_histogram(img):
    """the luminance histogram of a host image (take_hip_luminance_histogram, include/take_hip.h), made on the device:
    img (H, W, 3) float32 or float64 -> int64 (386,): 384 bins, 8 per octave over [2^-24, 2^24), then the counts of
    the non-positive and of the non-finite luminances"""
    img, precision = _image(img)
    hist = np.zeros(D.TAKE_LUMINANCE_SLOTS, np.int64)
    _check(lib().take_hip_luminance_histogram(img.ctypes.data, precision, img.shape[1], img.shape[0], hist.ctypes.data_as(C.POINTER(C.c_int64))))
    return hist


def luminance_histogram_device(ptr, width, height, precision, stream=None):
    """the same of an image in device memory (take_hip_luminance_histogram_device): ptr is a torch device tensor or an
    integer device pointer of `precision`'s Real -> the host histogram; blocks until done"""
    hist = np.zeros(D.TAKE_LUMINANCE_SLOTS, np.int64)
    _check(lib().take_hip_luminance_histogram_device(C.c_void_p(pointer(ptr)), int(precision), int(width), int(height),
                                                     hist.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(stream or 0)))
    return hist


def auto_exposure(hist, opts=None, **kw):
    """the exposure that takes the log-average luminance between two percentiles of `hist` (a luminance_histogram) to
    the key (take_hip_auto_exposure: host arithmetic, needs no GPU).  Options: keywords of cdefs.exposure_opts (key,
    low_fraction, high_fraction, min_exposure, max_exposure, prev_exposure, rate), or opts = a TakeExposureOpts; neither
    = the library's defaults (a NULL pointer).  With prev_exposure the result moves from it towards the target by `rate`
    in log2: feed each frame's result to the next."""
    h = np.ascontiguousarray(hist)
    if h.dtype != np.int64 or h.shape != (D.TAKE_LUMINANCE_SLOTS,):
        raise ValueError(f"hist must be an int64 array of {D.TAKE_LUMINANCE_SLOTS} counts")
    opts = _keyword_opts(D.exposure_opts, opts, kw)
    out = C.c_double(0.0)
    _check(lib().take_hip_auto_exposure(h.ctypes.data_as(C.POINTER(C.c_int64)), ref(opts), C.byref(out)))
    return out.value


def _tonemap_opts(opts, exposure, op, transfer, format, kw):
    if opts is not None:
        if kw or exposure is not None:
            raise ValueError("give opts or keywords, not both")
        return opts
    return D.tonemap_opts(exposure, op, transfer, format, **kw)


def _display_out(img, o):
    """the zeroed host array a display transform of `img` under the TakeTonemapOpts `o` fills"""
    return np.zeros(img.shape[:2] + (4,), np.uint8) if o.format == D.TAKE_DISPLAY_RGBA else np.zeros_like(img)


def _device_display_out(rgb, out, o):
    """the output plane of a display transform in device memory: `out`, or rgb itself where the format allows it"""
    if out is None and o.format == D.TAKE_DISPLAY_RGBA:
        raise ValueError("format 'rgba' needs an output plane")
    return C.c_void_p(pointer(rgb if out is None else out))


def tonemap(img, exposure=None, op="aces", transfer="srgb", format="rgba", opts=None, **kw):
    """the display transform of a host image (take_hip_tonemap, include/take_hip.h): exposure, tone operator ("linear",
    "reinhard", "aces"), transfer ("srgb", "linear"), on the device -> (array, exposure_used): uint8 (H, W, 4) for
    format "rgba", (H, W, 3) of img's dtype for "real".  exposure None = automatic: the auto_exposure of the image's
    luminance_histogram, with the further keywords (white for "reinhard", and those of cdefs.exposure_opts); or opts = a
    TakeTonemapOpts instead of all keywords."""
    img, precision = _image(img)
    o = _tonemap_opts(opts, exposure, op, transfer, format, kw)
    out, used = _display_out(img, o), C.c_double(0.0)
    _check(lib().take_hip_tonemap(img.ctypes.data, precision, img.shape[1], img.shape[0], C.byref(o), out.ctypes.data, C.byref(used)))
    return out, used.value


def tonemap_device(rgb, width, height, precision, out=None, exposure=None, op="aces", transfer="srgb", format="rgba", opts=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_tonemap_device): rgb is a torch device tensor or an integer device
    pointer of `precision`'s Real, out one of height * width * 4 bytes ("rgba") or height * width * 3 Reals ("real":
    out = None transforms in place) -> exposure_used; blocks until done.  Needs no scene."""
    o = _tonemap_opts(opts, exposure, op, transfer, format, kw)
    d_out, used = _device_display_out(rgb, out, o), C.c_double(0.0)
    _check(lib().take_hip_tonemap_device(C.c_void_p(pointer(rgb)), int(precision), int(width), int(height), C.byref(o), d_out, C.byref(used),
                                         C.c_void_p(stream or 0)))
    return used.value


class ImageWorkspace(Handle):
    """the workspace of the scene-free image-space calls (take_hip_image_workspace_create): it owns the histogram's block
    rows and the bloom pyramid, grows on demand and never shrinks, so that a sequence of frames allocates nothing after
    its first.  Bound to the device current at its creation; not thread-safe.  A context manager: `with ImageWorkspace()
    as ws: tonemap_bloom_device(..., workspace=ws)`."""
    _destroy = "take_hip_image_workspace_destroy"

    def __init__(self):
        _check(lib().take_hip_image_workspace_create(self._new()))


def _workspace(workspace):
    return None if workspace is None else handle_of(workspace, ImageWorkspace, "workspace")


def _bloom_opts(bloom, kw):
    """the bloom options of a call: a TakeBloomOpts, or the keywords of cdefs.bloom_opts taken out of `kw`, or neither
    (None: the library's defaults, a NULL pointer)"""
    names = [k for k in ("threshold", "knee", "intensity", "levels") if k in kw]
    if bloom is not None:
        if names:
            raise ValueError("give bloom or its keywords, not both")
        return bloom
    return D.bloom_opts(**{k: kw.pop(k) for k in names}) if names else None


def _only_bloom_opts(bloom, kw):
    b = _bloom_opts(bloom, kw)
    if kw:
        raise ValueError(f"unknown keywords {sorted(kw)}")
    return b


def bloom_layer(img, exposure, bloom=None, **kw):
    """the bloom layer of a host image at that exposure (take_hip_bloom_layer, include/take_hip.h): what
    tonemap_bloom adds to the exposed image before the tone operator -> (H, W, 3) of img's dtype.  Options: threshold,
    knee, intensity, levels (cdefs.bloom_opts), or bloom = a TakeBloomOpts; neither = the library's defaults."""
    img, precision = _image(img)
    b = _only_bloom_opts(bloom, kw)
    out = np.zeros_like(img)
    _check(lib().take_hip_bloom_layer(img.ctypes.data, precision, img.shape[1], img.shape[0], float(exposure), ref(b), out.ctypes.data))
    return out


def bloom_layer_device(rgb, width, height, precision, exposure, out, bloom=None, workspace=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_bloom_layer_device): rgb and out are torch device tensors or integer
    device pointers of height * width * 3 of `precision`'s Real (out may be rgb); workspace: an ImageWorkspace, or None =
    the pyramid is allocated per call; blocks until done.  Needs no scene."""
    b = _only_bloom_opts(bloom, kw)
    _check(lib().take_hip_bloom_layer_device(C.c_void_p(pointer(rgb)), int(precision), int(width), int(height), float(exposure), ref(b),
                                             C.c_void_p(pointer(out)), _workspace(workspace), C.c_void_p(stream or 0)))


def tonemap_bloom(img, exposure=None, op="aces", transfer="srgb", format="rgba", opts=None, bloom=None, **kw):
    """tonemap with bloom (take_hip_tonemap_bloom, include/take_hip.h): the layer of what exceeds the threshold after
    exposure, blurred over a pyramid, added before the tone operator -> (array, exposure_used) as tonemap.  The further
    keywords: threshold, knee, intensity, levels (cdefs.bloom_opts; or bloom = a TakeBloomOpts), and tonemap's."""
    img, precision = _image(img)
    b = _bloom_opts(bloom, kw)
    o = _tonemap_opts(opts, exposure, op, transfer, format, kw)
    out, used = _display_out(img, o), C.c_double(0.0)
    _check(lib().take_hip_tonemap_bloom(img.ctypes.data, precision, img.shape[1], img.shape[0], C.byref(o), ref(b), out.ctypes.data, C.byref(used)))
    return out, used.value


def tonemap_bloom_device(rgb, width, height, precision, out=None, exposure=None, op="aces", transfer="srgb", format="rgba", opts=None, bloom=None,
                         workspace=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_tonemap_bloom_device), as tonemap_device; workspace: an
    ImageWorkspace that keeps the histogram's rows and the pyramid between calls, or None = allocated per call
    -> exposure_used; blocks until done.  Needs no scene."""
    b = _bloom_opts(bloom, kw)
    o = _tonemap_opts(opts, exposure, op, transfer, format, kw)
    d_out, used = _device_display_out(rgb, out, o), C.c_double(0.0)
    _check(lib().take_hip_tonemap_bloom_device(C.c_void_p(pointer(rgb)), int(precision), int(width), int(height), C.byref(o), ref(b), d_out, C.byref(used),
                                               _workspace(workspace), C.c_void_p(stream or 0)))
    return used.value

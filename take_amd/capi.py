"""ctypes binding of libtake_hip.so (include/take_hip.h).

The library is the product; this module only marshals.  There is no fallback: if the shared object is
missing or no HIP device is visible every call raises `TakeError`.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import cdefs as D

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TAKE_HIP_LIB") or os.path.join(_PKG, "libtake_hip.so")  # TAKE_HIP_LIB: tuning builds
_LIB = None

EXPORTS = [
    "take_hip_last_error", "take_hip_abi_version", "take_hip_device_count", "take_hip_scene_create",
    "take_hip_scene_destroy", "take_hip_render", "take_hip_render_device", "take_hip_render_rows",
    "take_hip_render_accumulate", "take_hip_accumulated_samples",
    "take_hip_trace_closest", "take_hip_trace_any", "take_hip_trace_closest_device", "take_hip_get_counters",
    "take_hip_set_instrumentation", "take_hip_scene_stats", "take_hip_debug_table", "take_hip_debug_env",
    "take_hip_group_create", "take_hip_group_destroy", "take_hip_group_render", "take_hip_group_render_device",
    "take_hip_group_size", "take_hip_group_get_counters", "take_hip_pack_exr_scanlines", "take_hip_render_exr_scanlines",
    "take_hip_ply_layout", "take_hip_mesh_from_ply", "take_hip_mesh_from_ply_file",
    "take_hip_mesh_from_serialized", "take_hip_mesh_from_serialized_file", "take_hip_mesh_download", "take_hip_mesh_release",
    "take_hip_mesh_from_obj", "take_hip_mesh_from_obj_file", "take_hip_mesh_compute_normals", "take_hip_compute_normals",
    "take_hip_scene_build_info",
    "take_hip_scene_set_instance_transforms", "take_hip_scene_set_instance_transforms_device", "take_hip_scene_set_camera",
    "take_hip_scene_set_mesh_vertices", "take_hip_scene_update_meshes",
    "take_hip_render_features", "take_hip_render_features_device",
    "take_hip_debug_tree_info", "take_hip_debug_tree",
    "take_hip_denoise", "take_hip_denoise_device", "take_hip_render_denoised", "take_hip_render_denoised_device",
    "take_hip_render_adaptive", "take_hip_render_adaptive_device",
    "take_hip_denoise_variance", "take_hip_denoise_variance_device", "take_hip_render_adaptive_denoised", "take_hip_render_adaptive_denoised_device",
    "take_hip_scene_mark_frame", "take_hip_render_motion", "take_hip_render_motion_device",
    "take_hip_temporal_accumulate", "take_hip_temporal_accumulate_device", "take_hip_render_temporal", "take_hip_render_temporal_device",
    "take_hip_scene_track_vertices", "take_hip_scene_tracking_info",
    "take_hip_luminance_histogram", "take_hip_luminance_histogram_device", "take_hip_auto_exposure", "take_hip_tonemap", "take_hip_tonemap_device",
    "take_hip_scene_set_lens", "take_hip_scene_get_lens", "take_hip_scene_focus_distance_at",
    "take_hip_shutter_plan", "take_hip_shutter_pose", "take_hip_render_shutter", "take_hip_render_shutter_device",
    "take_hip_shutter_vertices", "take_hip_shutter_vertices_device", "take_hip_render_shutter_meshes", "take_hip_render_shutter_meshes_device",
    "take_hip_image_workspace_create", "take_hip_image_workspace_destroy", "take_hip_bloom_layer", "take_hip_bloom_layer_device",
    "take_hip_tonemap_bloom", "take_hip_tonemap_bloom_device",
    "take_hip_render_rays", "take_hip_render_rays_device", "take_hip_camera_rays", "take_hip_camera_rays_device",
    "take_hip_scene_set_envmap", "take_hip_scene_set_envmap_device", "take_hip_debug_env_tables_info", "take_hip_debug_env_tables",
    "take_hip_scene_set_materials", "take_hip_scene_set_light_intensities", "take_hip_scene_set_light_intensities_device",
    "take_hip_debug_shading_tables_info", "take_hip_debug_shading_tables",
    "take_hip_rig_create", "take_hip_rig_destroy", "take_hip_rig_info", "take_hip_rig_pose_device", "take_hip_rig_pose", "take_hip_scene_pose_meshes",
    "take_hip_subdiv_counts", "take_hip_subdiv_topology", "take_hip_subdiv_create", "take_hip_subdiv_destroy", "take_hip_subdiv_info",
    "take_hip_subdiv_refine_device", "take_hip_subdiv_refine", "take_hip_scene_subdivide_meshes",
]


class TakeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"take_hip error {code}: {msg}")
        self.code = code


def build(force=False):
    """Compile libtake_hip.so for gfx950 with hipcc (take_amd/csrc/Makefile).  Cross-compiles without a GPU."""
    src = os.path.join(_PKG, "csrc")
    args = ["make", "-C", src]
    if force:
        args.append("-B")
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libtake_hip.so failed:\n" + r.stdout[-4000:])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise TakeError(-3, f"{LIB_PATH} not built (run __graft_entry__.build() / make -C take_amd/csrc)")
        L = C.CDLL(LIB_PATH)
        L.take_hip_last_error.restype = C.c_char_p
        L.take_hip_scene_create.argtypes = [C.POINTER(D.TakeSceneDesc), C.POINTER(D.TakeBuildOpts),
                                            C.POINTER(C.c_void_p)]
        L.take_hip_scene_destroy.argtypes = [C.c_void_p]
        L.take_hip_render.argtypes = [C.c_void_p, C.POINTER(D.TakeRenderOpts), C.c_void_p]
        L.take_hip_render_device.argtypes = [C.c_void_p, C.POINTER(D.TakeRenderOpts), C.c_void_p, C.c_void_p]
        L.take_hip_render_accumulate.argtypes = [C.c_void_p, C.POINTER(D.TakeRenderOpts), C.c_int32, C.c_void_p, C.c_void_p]
        L.take_hip_accumulated_samples.argtypes = [C.c_void_p]
        L.take_hip_accumulated_samples.restype = C.c_int64
        L.take_hip_render_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
        L.take_hip_trace_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.take_hip_trace_any.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.take_hip_trace_closest_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                                    C.c_void_p]
        L.take_hip_get_counters.argtypes = [C.c_void_p, C.POINTER(D.TakeCounters)]
        L.take_hip_set_instrumentation.argtypes = [C.c_void_p, C.c_int32]
        L.take_hip_scene_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.take_hip_scene_build_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.take_hip_debug_env.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        for name, argtypes in list(D.SCENE_UPDATE_PROTOTYPES.items()) + list(D.FEATURE_PROTOTYPES.items()) + list(D.DEBUG_TREE_PROTOTYPES.items()) + list(D.DENOISE_PROTOTYPES.items()) + list(D.ADAPTIVE_PROTOTYPES.items()) + list(D.DENOISE_VARIANCE_PROTOTYPES.items()) + list(D.TEMPORAL_PROTOTYPES.items()) + list(D.TRACKING_PROTOTYPES.items()) + list(D.DISPLAY_PROTOTYPES.items()) + list(D.LENS_PROTOTYPES.items()) + list(D.SHUTTER_PROTOTYPES.items()) + list(D.SHUTTER_MESHES_PROTOTYPES.items()) + list(D.BLOOM_PROTOTYPES.items()) + list(D.RAYS_PROTOTYPES.items()) + list(D.ENVMAP_PROTOTYPES.items()) + list(D.SHADING_UPDATE_PROTOTYPES.items()) + list(D.RIG_PROTOTYPES.items()) + list(D.SUBDIV_PROTOTYPES.items()):
            getattr(L, name).argtypes = argtypes
        L.take_hip_image_workspace_destroy.restype = None
        L.take_hip_pack_exr_scanlines.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.take_hip_render_exr_scanlines.argtypes = [C.c_void_p, C.POINTER(D.TakeRenderOpts), C.c_void_p]
        L.take_hip_group_create.argtypes = [C.POINTER(D.TakeSceneDesc), C.POINTER(D.TakeBuildOpts), C.c_int32,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]
        L.take_hip_group_destroy.argtypes = [C.c_void_p]
        L.take_hip_group_render.argtypes = [C.c_void_p, C.POINTER(D.TakeRenderOpts), C.c_void_p]
        L.take_hip_group_render_device.argtypes = [C.c_void_p, C.POINTER(D.TakeRenderOpts), C.c_void_p]
        L.take_hip_group_size.argtypes = [C.c_void_p]
        L.take_hip_group_get_counters.argtypes = [C.c_void_p, C.c_int32, C.POINTER(D.TakeCounters)]
        L.take_hip_ply_layout.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(D.TakePlyLayout)]
        L.take_hip_mesh_from_ply.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(D.TakeMesh)]
        L.take_hip_mesh_from_ply_file.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(D.TakeMesh)]
        L.take_hip_mesh_from_serialized.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(D.TakeMesh)]
        L.take_hip_mesh_from_serialized_file.argtypes = [C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(D.TakeMesh)]
        L.take_hip_mesh_from_obj.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(D.TakeMesh)]
        L.take_hip_mesh_from_obj_file.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(D.TakeMesh)]
        L.take_hip_mesh_download.argtypes = [C.POINTER(D.TakeMesh), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.take_hip_mesh_release.argtypes = [C.POINTER(D.TakeMesh)]
        L.take_hip_mesh_compute_normals.argtypes = [C.POINTER(D.TakeMesh)]
        L.take_hip_compute_normals.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        _LIB = L
    return _LIB


def _check(rc):
    if rc < 0:
        raise TakeError(rc, lib().take_hip_last_error().decode())
    return rc


def device_count():
    return _check(lib().take_hip_device_count())


def shutter_plan(spp, open=0.0, close=1.0, slices=0):
    """how a render over the shutter [open, close] cuts `spp` samples into slices (take_hip_shutter_plan; no scene, no
    GPU) -> (first_sample, time): K + 1 int32 bounds — slice k holds the samples first_sample[k] .. first_sample[k + 1] - 1
    of every pixel — and the K scene times the slices are posed at"""
    sh, k = D.TakeShutter(float(open), float(close), int(slices), 0), C.c_int32()
    _check(lib().take_hip_shutter_plan(int(spp), C.byref(sh), C.byref(k), None, None))
    first, time = np.zeros(k.value + 1, np.int32), np.zeros(k.value, np.float64)
    _check(lib().take_hip_shutter_plan(int(spp), C.byref(sh), C.byref(k), first.ctypes.data_as(C.POINTER(C.c_int32)),
                                       time.ctypes.data_as(C.POINTER(C.c_double))))
    return first, time


def _on_device(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def shutter_vertices(a, b, t, stream=None):
    """the vertices of a deforming mesh at scene time t in [0, 1] (take_hip_shutter_vertices): `a` the array at the marked
    frame, `b` at the current one — positions or normals, any shape, float64 — lerped entry by entry on the device as
    render_shutter_meshes lerps them -> (out, moved): the array at t, and 1 where any entry of it is not b's bit for bit.
    numpy arrays give a numpy array; contiguous float64 torch device tensors are read through their device pointers after
    `stream` (default: torch's current stream) and give a new device tensor."""
    moved = C.c_int32(-1)
    if _on_device(a) or _on_device(b):
        import torch

        if not (_on_device(a) and _on_device(b)) or a.shape != b.shape or a.device != b.device or not all(str(x.dtype) == "torch.float64" and x.is_contiguous() for x in (a, b)):
            raise ValueError("arrays on the device must be contiguous float64 tensors of one shape, both on one device")
        out = torch.empty_like(a)
        if stream is None:
            stream = torch.cuda.current_stream(a.device).cuda_stream
        with torch.cuda.device(a.device):
            _check(lib().take_hip_shutter_vertices_device(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.numel(), float(t), C.c_void_p(out.data_ptr()),
                                                          C.byref(moved), C.c_void_p(stream or 0)))
        return out, moved.value
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        raise ValueError("a and b must have one shape")
    out = np.zeros_like(a)
    _check(lib().take_hip_shutter_vertices(a.ctypes.data, b.ctypes.data, a.size, float(t), out.ctypes.data, C.byref(moved)))
    return out, moved.value


def ply_layout(data):
    """what the header of a binary PLY file says about its vertex / face elements (host only, no GPU)"""
    buf = bytes(data)
    out = D.TakePlyLayout()
    _check(lib().take_hip_ply_layout(buf, len(buf), C.byref(out)))
    return {k: getattr(out, k) for k, _ in D.TakePlyLayout._fields_ if k != "reserved"}


def compute_normals(positions, indices):
    """the reference's compute_normals (src/compute_normals.cpp:12-47) on the device, for host arrays: (nv, 3) positions,
    (nf, 3) vertex indices -> (nv, 3) angle-weighted unit vertex normals ((0, 0, 0) where the sum vanishes)"""
    pos = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.int32).reshape(-1, 3)
    out = np.zeros_like(pos)
    _check(lib().take_hip_compute_normals(pos.ctypes.data, pos.shape[0], idx.ctypes.data, idx.shape[0], out.ctypes.data))
    return out


def _pointer(a):
    """device pointer of a torch tensor, or the integer itself; None stays None"""
    return None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else int(a))


def _keyword_opts(make, opts, kw):
    """an options struct, keywords of `make` (cdefs.denoise_opts, cdefs.temporal_opts), or neither (None: the library's
    defaults, a NULL pointer)"""
    if kw and opts is not None:
        raise ValueError("give opts or keywords, not both")
    return make(**kw) if kw else opts


def _rgb_and_guides(rgb, albedo, normal, depth):
    """host arrays as denoise() takes them -> (contiguous rgb, its TAKE_PRECISION_*, a TakeFeatureBuffers over the guides that
    were given, the arrays it points into: empty = no guides)"""
    rgb = np.asarray(rgb)
    if rgb.dtype not in (np.float32, np.float64) or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("rgb must be a (H, W, 3) float32 or float64 array")
    h, w = rgb.shape[:2]
    rgb = np.ascontiguousarray(rgb)
    bufs, keep = D.TakeFeatureBuffers(), []
    for name, a, shape in (("albedo", albedo, (h, w, 3)), ("normal", normal, (h, w, 3)), ("depth", depth, (h, w))):
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        if a.dtype != rgb.dtype or a.shape != shape:
            raise ValueError(f"{name} must be a {shape} array of rgb's dtype")
        keep.append(a)
        setattr(bufs, name, a.ctypes.data)
    return rgb, D.TAKE_PRECISION_F32 if rgb.dtype == np.float32 else D.TAKE_PRECISION_F64, bufs, keep


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
    _check(lib().take_hip_denoise(rgb.ctypes.data, C.byref(bufs) if keep else None, precision, w, h,
                                  None if opts is None else C.byref(opts), out.ctypes.data))
    return out


def denoise_device(rgb, width, height, precision, out=None, albedo=None, normal=None, depth=None, opts=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_denoise_device): rgb, out and the guides are torch device tensors or
    integer device pointers of `precision`'s Real (TAKE_PRECISION_F32 / _F64); out = None filters in place; blocks until
    done.  Needs no scene: also for what render_accumulate or a scene group left on the device."""
    bufs = D.TakeFeatureBuffers(_pointer(albedo), _pointer(normal), _pointer(depth), None, None, None)
    opts = _keyword_opts(D.denoise_opts, opts, kw)
    _check(lib().take_hip_denoise_device(C.c_void_p(_pointer(rgb)), C.byref(bufs), int(precision), int(width), int(height),
                                         None if opts is None else C.byref(opts), C.c_void_p(_pointer(rgb if out is None else out)),
                                         C.c_void_p(stream or 0)))


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
    _check(lib().take_hip_denoise_variance(rgb.ctypes.data, C.byref(bufs) if keep else None, C.byref(stats), precision, w, h,
                                           None if opts is None else C.byref(opts), out.ctypes.data, None if var is None else var.ctypes.data))
    return (out, var) if variance else out


def denoise_variance_device(rgb, count, m1, m2, width, height, precision, out=None, albedo=None, normal=None, depth=None, variance=None, opts=None,
                            stream=None, **kw):
    """the same on planes in device memory (take_hip_denoise_variance_device): rgb, out, the guides and variance (the
    optional output plane) are torch device tensors or integer device pointers of `precision`'s Real, count int32, m1 and
    m2 float64; out = None filters in place; blocks until done.  Needs no scene."""
    bufs = D.TakeFeatureBuffers(_pointer(albedo), _pointer(normal), _pointer(depth), None, None, None)
    stats = D.TakeAdaptiveStats(_pointer(count), _pointer(m1), _pointer(m2))
    opts = _keyword_opts(D.denoise_opts, opts, kw)
    _check(lib().take_hip_denoise_variance_device(C.c_void_p(_pointer(rgb)), C.byref(bufs), C.byref(stats), int(precision), int(width), int(height),
                                                  None if opts is None else C.byref(opts), C.c_void_p(_pointer(rgb if out is None else out)),
                                                  C.c_void_p(_pointer(variance)), C.c_void_p(stream or 0)))


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
    return D.TakeAdaptiveStats(*[_pointer(stats.get(k)) for k in STATS_PLANES])


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
    rgb = np.asarray(cur.get("rgb") if isinstance(cur, dict) else None)
    if rgb.dtype not in (np.float32, np.float64) or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("cur['rgb'] must be a (H, W, 3) float32 or float64 array")
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
    precision = D.TAKE_PRECISION_F32 if rgb.dtype == np.float32 else D.TAKE_PRECISION_F64
    _check(lib().take_hip_temporal_accumulate(C.byref(c), None if hf is None else C.byref(hf), xy.ctypes.data, None if pd is None else pd.ctypes.data,
                                              precision, w, h, None if opts is None else C.byref(opts), C.byref(o)))
    return out


def temporal_accumulate_device(cur, hist, prev_xy, prev_depth, width, height, precision, out=None, opts=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_temporal_accumulate_device): cur, hist (or None) and out are
    {plane: torch device tensor or integer device pointer}, prev_xy and prev_depth (or None) tensors or pointers, of
    `precision`'s Real (count and shape_id int32, m1 and m2 float64); out = None accumulates into cur's planes (out must
    never be hist: the taps gather); blocks until done.  Needs no scene."""
    def frame(name, f):
        _known_temporal_planes(name, f)
        return D.TakeTemporalFrame(*[_pointer(f.get(k)) for k in TEMPORAL_PLANES])

    c = frame("cur", cur)
    hf = None if hist is None else frame("hist", hist)
    o = c if out is None else frame("out", out)
    opts = _keyword_opts(D.temporal_opts, opts, kw)
    _check(lib().take_hip_temporal_accumulate_device(C.byref(c), None if hf is None else C.byref(hf), C.c_void_p(_pointer(prev_xy)), C.c_void_p(_pointer(prev_depth)),
                                                     int(precision), int(width), int(height), None if opts is None else C.byref(opts), C.byref(o),
                                                     C.c_void_p(stream or 0)))


def _image(img):
    """a host image as the display calls take it -> (contiguous (H, W, 3) array, its TAKE_PRECISION_*)"""
    img = np.asarray(img)
    if img.dtype not in (np.float32, np.float64) or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("the image must be a (H, W, 3) float32 or float64 array")
    return np.ascontiguousarray(img), D.TAKE_PRECISION_F32 if img.dtype == np.float32 else D.TAKE_PRECISION_F64


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
    _check(lib().take_hip_luminance_histogram_device(C.c_void_p(_pointer(ptr)), int(precision), int(width), int(height),
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
    _check(lib().take_hip_auto_exposure(h.ctypes.data_as(C.POINTER(C.c_int64)), None if opts is None else C.byref(opts), C.byref(out)))
    return out.value


def _tonemap_opts(opts, exposure, op, transfer, format, kw):
    if opts is not None:
        if kw or exposure is not None:
            raise ValueError("give opts or keywords, not both")
        return opts
    return D.tonemap_opts(exposure, op, transfer, format, **kw)


def tonemap(img, exposure=None, op="aces", transfer="srgb", format="rgba", opts=None, **kw):
    """the display transform of a host image (take_hip_tonemap, include/take_hip.h): exposure, tone operator ("linear",
    "reinhard", "aces"), transfer ("srgb", "linear"), on the device -> (array, exposure_used): uint8 (H, W, 4) for
    format "rgba", (H, W, 3) of img's dtype for "real".  exposure None = automatic: the auto_exposure of the image's
    luminance_histogram, with the further keywords (white for "reinhard", and those of cdefs.exposure_opts); or opts = a
    TakeTonemapOpts instead of all keywords."""
    img, precision = _image(img)
    o = _tonemap_opts(opts, exposure, op, transfer, format, kw)
    h, w = img.shape[:2]
    out = np.zeros((h, w, 4), np.uint8) if o.format == D.TAKE_DISPLAY_RGBA else np.zeros_like(img)
    used = C.c_double(0.0)
    _check(lib().take_hip_tonemap(img.ctypes.data, precision, w, h, C.byref(o), out.ctypes.data, C.byref(used)))
    return out, used.value


def tonemap_device(rgb, width, height, precision, out=None, exposure=None, op="aces", transfer="srgb", format="rgba", opts=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_tonemap_device): rgb is a torch device tensor or an integer device
    pointer of `precision`'s Real, out one of height * width * 4 bytes ("rgba") or height * width * 3 Reals ("real":
    out = None transforms in place) -> exposure_used; blocks until done.  Needs no scene."""
    o = _tonemap_opts(opts, exposure, op, transfer, format, kw)
    if out is None and o.format == D.TAKE_DISPLAY_RGBA:
        raise ValueError("format 'rgba' needs an output plane")
    used = C.c_double(0.0)
    _check(lib().take_hip_tonemap_device(C.c_void_p(_pointer(rgb)), int(precision), int(width), int(height), C.byref(o),
                                         C.c_void_p(_pointer(rgb if out is None else out)), C.byref(used), C.c_void_p(stream or 0)))
    return used.value


class ImageWorkspace:
    """the workspace of the scene-free image-space calls (take_hip_image_workspace_create): it owns the histogram's block
    rows and the bloom pyramid, grows on demand and never shrinks, so that a sequence of frames allocates nothing after
    its first.  Bound to the device current at its creation; not thread-safe.  A context manager: `with ImageWorkspace()
    as ws: tonemap_bloom_device(..., workspace=ws)`."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(lib().take_hip_image_workspace_create(C.byref(self._h)))

    def close(self):
        if self._h:
            lib().take_hip_image_workspace_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # (interpreter shutdown: the library may be gone)
            pass


def _workspace(workspace):
    if workspace is None:
        return None
    if not isinstance(workspace, ImageWorkspace) or not workspace._h:
        raise ValueError("workspace must be an open ImageWorkspace")
    return workspace._h


def _bloom_opts(bloom, kw):
    """the bloom options of a call: a TakeBloomOpts, or the keywords of cdefs.bloom_opts taken out of `kw`, or neither
    (None: the library's defaults, a NULL pointer)"""
    names = [k for k in ("threshold", "knee", "intensity", "levels") if k in kw]
    if bloom is not None:
        if names:
            raise ValueError("give bloom or its keywords, not both")
        return bloom
    return D.bloom_opts(**{k: kw.pop(k) for k in names}) if names else None


def bloom_layer(img, exposure, bloom=None, **kw):
    """the bloom layer of a host image at that exposure (take_hip_bloom_layer, include/take_hip.h): what
    tonemap_bloom adds to the exposed image before the tone operator -> (H, W, 3) of img's dtype.  Options: threshold,
    knee, intensity, levels (cdefs.bloom_opts), or bloom = a TakeBloomOpts; neither = the library's defaults."""
    img, precision = _image(img)
    b = _bloom_opts(bloom, kw)
    if kw:
        raise ValueError(f"unknown keywords {sorted(kw)}")
    out = np.zeros_like(img)
    _check(lib().take_hip_bloom_layer(img.ctypes.data, precision, img.shape[1], img.shape[0], float(exposure), None if b is None else C.byref(b), out.ctypes.data))
    return out


def bloom_layer_device(rgb, width, height, precision, exposure, out, bloom=None, workspace=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_bloom_layer_device): rgb and out are torch device tensors or integer
    device pointers of height * width * 3 of `precision`'s Real (out may be rgb); workspace: an ImageWorkspace, or None =
    the pyramid is allocated per call; blocks until done.  Needs no scene."""
    b = _bloom_opts(bloom, kw)
    if kw:
        raise ValueError(f"unknown keywords {sorted(kw)}")
    _check(lib().take_hip_bloom_layer_device(C.c_void_p(_pointer(rgb)), int(precision), int(width), int(height), float(exposure), None if b is None else C.byref(b),
                                             C.c_void_p(_pointer(out)), _workspace(workspace), C.c_void_p(stream or 0)))


def tonemap_bloom(img, exposure=None, op="aces", transfer="srgb", format="rgba", opts=None, bloom=None, **kw):
    """tonemap with bloom (take_hip_tonemap_bloom, include/take_hip.h): the layer of what exceeds the threshold after
    exposure, blurred over a pyramid, added before the tone operator -> (array, exposure_used) as tonemap.  The further
    keywords: threshold, knee, intensity, levels (cdefs.bloom_opts; or bloom = a TakeBloomOpts), and tonemap's."""
    img, precision = _image(img)
    b = _bloom_opts(bloom, kw)
    o = _tonemap_opts(opts, exposure, op, transfer, format, kw)
    h, w = img.shape[:2]
    out = np.zeros((h, w, 4), np.uint8) if o.format == D.TAKE_DISPLAY_RGBA else np.zeros_like(img)
    used = C.c_double(0.0)
    _check(lib().take_hip_tonemap_bloom(img.ctypes.data, precision, w, h, C.byref(o), None if b is None else C.byref(b), out.ctypes.data, C.byref(used)))
    return out, used.value


def tonemap_bloom_device(rgb, width, height, precision, out=None, exposure=None, op="aces", transfer="srgb", format="rgba", opts=None, bloom=None,
                         workspace=None, stream=None, **kw):
    """the same on planes in device memory (take_hip_tonemap_bloom_device), as tonemap_device; workspace: an
    ImageWorkspace that keeps the histogram's rows and the pyramid between calls, or None = allocated per call
    -> exposure_used; blocks until done.  Needs no scene."""
    b = _bloom_opts(bloom, kw)
    o = _tonemap_opts(opts, exposure, op, transfer, format, kw)
    if out is None and o.format == D.TAKE_DISPLAY_RGBA:
        raise ValueError("format 'rgba' needs an output plane")
    used = C.c_double(0.0)
    _check(lib().take_hip_tonemap_bloom_device(C.c_void_p(_pointer(rgb)), int(precision), int(width), int(height), C.byref(o), None if b is None else C.byref(b),
                                               C.c_void_p(_pointer(rgb if out is None else out)), C.byref(used), _workspace(workspace), C.c_void_p(stream or 0)))
    return used.value


class DeviceMesh:
    """A triangle mesh decoded from a binary PLY file, a Mitsuba `.serialized` file or a Wavefront OBJ file ON the device
    (take_hip_mesh_from_ply / _from_serialized / _from_obj: replace the reference's parse_ply,
    src/parse/parse_ply.cpp:9-123, parse_serialized, src/parse/parse_serialized.cpp:174-256, and parse_obj,
    src/parse/parse_obj.cpp:118-203).  The arrays are device memory owned by the library; put the object into
    SceneData.meshes like a scene.Mesh.  `source`: a path or the file's bytes.  `format`: "ply", "serialized", "obj", or
    None = told from the source: a path ending in `.obj` (any case) is OBJ, otherwise the first bytes decide (`ply` /
    anything else = serialized, whose sub-mesh `shape_index` picks); bytes holding an OBJ file need format="obj".
    to_world: 4x4 (the reference's Matrix4x4); inv_to_world: the caller's inverse of it (the reference passes its own
    `inverse(to_world)`), default numpy's.  `normals`: None = the file's normals, or none; "scene" = what parse_scene
    does for a shape without faceNormals: the file's normals if it has any, else compute_normals' (computed on the
    device, compute_normals())."""

    FORMATS = (None, "ply", "serialized", "obj")
    NORMALS = (None, "scene")

    def __init__(self, source, material_id=0, to_world=None, inv_to_world=None, shape_index=0, format=None, normals=None):
        if format not in self.FORMATS:
            raise ValueError(f"format must be one of {self.FORMATS}, not {format!r}")
        if normals not in self.NORMALS:
            raise ValueError(f"normals must be one of {self.NORMALS}, not {normals!r}")
        self.c = D.TakeMesh()
        xw = xi = None
        if to_world is not None:
            xw = np.ascontiguousarray(to_world, np.float64).reshape(4, 4)
            xi = np.ascontiguousarray(np.linalg.inv(xw) if inv_to_world is None else inv_to_world, np.float64).reshape(4, 4)
        a = None if xw is None else xw.ctypes.data
        b = None if xi is None else xi.ctypes.data
        if isinstance(source, (bytes, bytearray, memoryview)):
            buf = bytes(source)
            fmt = format or ("ply" if buf[:3] == b"ply" else "serialized")
            if fmt == "ply":
                _check(lib().take_hip_mesh_from_ply(buf, len(buf), a, b, int(material_id), C.byref(self.c)))
            elif fmt == "obj":
                _check(lib().take_hip_mesh_from_obj(buf, len(buf), a, b, int(material_id), C.byref(self.c)))
            else:
                _check(lib().take_hip_mesh_from_serialized(buf, len(buf), int(shape_index), a, b, int(material_id), C.byref(self.c)))
        else:
            fmt = format
            if fmt is None and os.fsdecode(source).lower().endswith(".obj"):
                fmt = "obj"
            if fmt is None:
                with open(source, "rb") as f:
                    fmt = "ply" if f.read(3) == b"ply" else "serialized"
            path = os.fsencode(source)
            if fmt == "ply":
                _check(lib().take_hip_mesh_from_ply_file(path, a, b, int(material_id), C.byref(self.c)))
            elif fmt == "obj":
                _check(lib().take_hip_mesh_from_obj_file(path, a, b, int(material_id), C.byref(self.c)))
            else:
                _check(lib().take_hip_mesh_from_serialized_file(path, int(shape_index), a, b, int(material_id), C.byref(self.c)))
        self.material_id = int(material_id)
        if normals == "scene" and not self.c.normals:
            self.compute_normals()

    n_vertices = property(lambda self: int(self.c.n_vertices))
    n_faces = property(lambda self: int(self.c.n_faces))

    def compute_normals(self):
        """fill the mesh's missing normals in place: the reference's compute_normals on the device
        (take_hip_mesh_compute_normals); a mesh that has normals already is refused"""
        _check(lib().take_hip_mesh_compute_normals(C.byref(self.c)))
        return self

    def download(self):
        """-> scene.Mesh with host copies of the arrays (tests; the render path never needs it)"""
        from .scene import Mesh

        nv, nf = self.n_vertices, self.n_faces
        pos, idx = np.zeros((nv, 3), np.float64), np.zeros((nf, 3), np.int32)
        nrm = np.zeros((nv, 3), np.float64) if self.c.normals else None
        uv = np.zeros((nv, 2), np.float64) if self.c.uvs else None
        _check(lib().take_hip_mesh_download(C.byref(self.c), pos.ctypes.data, idx.ctypes.data,
                                            None if nrm is None else nrm.ctypes.data, None if uv is None else uv.ctypes.data))
        return Mesh(pos, idx, self.material_id, nrm, uv)

    def close(self):
        if self.c.flags:
            lib().take_hip_mesh_release(C.byref(self.c))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _on_device(a):
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def _rig_array(a, dtype, shape, name, device, keep):
    """one array of a rig or of a pose -> its pointer (None stays None): a contiguous torch tensor on the device when
    `device`, else host memory through numpy; `shape` with -1 for a free extent"""
    if a is None:
        return None
    if device:
        if not _on_device(a) or str(a.dtype) != "torch." + np.dtype(dtype).name or not a.is_contiguous():
            raise ValueError(f"{name}: arrays on the device must be contiguous {np.dtype(dtype).name} tensors, and all arrays of a call on the device")
        got = tuple(a.shape)
    else:
        if hasattr(a, "data_ptr"):  # a torch tensor in host memory
            a = a.numpy()
        a = np.ascontiguousarray(a, dtype)
        got = a.shape
    if len(got) != len(shape) or any(w >= 0 and g != w for g, w in zip(got, shape)):
        raise ValueError(f"{name} must have shape {tuple('n' if w < 0 else w for w in shape)}, not {tuple(got)}")
    keep.append(a)
    return a.data_ptr() if device else a.ctypes.data


class Rig:
    """A mesh's rest pose, joint influences and morph targets in device memory (take_hip_rig_create): what pose(),
    pose_device() and Scene.pose_meshes() skin and morph on the device — linear-blend skinning over a joint palette,
    normals by the cofactor matrix (include/take_hip.h has the arithmetic).  positions (n, 3) and the optional normals
    (n, 3) are the rest pose; joints (n, K) int32 and weights (n, K), K = 1..8, name each vertex's influences (weights are
    taken as they are, padding is a zero weight on any valid joint); inverse_bind (n_joints, 3, 4), None = identity —
    it fixes the joint count, which without it is max(joints) + 1 or `n_joints`; target_positions / target_normals
    (T, n, 3) are morph deltas.  Either numpy arrays (or anything numpy converts), or contiguous float64 / int32 torch
    tensors on the device — all of them then.  Bound to the device current at its creation; not thread-safe."""

    def __init__(self, positions, normals=None, joints=None, weights=None, inverse_bind=None, target_positions=None, target_normals=None, n_joints=None):
        self._h = C.c_void_p()
        device = _on_device(positions)
        keep = []
        d = D.TakeRigDesc()
        d.positions = _rig_array(positions, np.float64, (-1, 3), "positions", device, keep)
        nv = int(keep[0].shape[0])
        d.n_vertices, d.flags = nv, D.TAKE_RIG_DEVICE_ARRAYS if device else 0
        d.normals = _rig_array(normals, np.float64, (nv, 3), "normals", device, keep)
        if (joints is None) != (weights is None):
            raise ValueError("joints and weights go together")
        if joints is not None:
            d.joints = _rig_array(joints, np.int32, (nv, -1), "joints", device, keep)
            ja = keep[-1]
            k = int(ja.shape[1])
            d.weights = _rig_array(weights, np.float64, (nv, k), "weights", device, keep)
            d.inverse_bind = _rig_array(inverse_bind, np.float64, (-1, 3, 4), "inverse_bind", device, keep)
            if inverse_bind is not None:
                nj = int(keep[-1].shape[0])
            elif n_joints is not None:
                nj = int(n_joints)
            else:
                nj = int(ja.max()) + 1 if nv * k else 0
            d.n_joints, d.n_influences = nj, k
        if target_positions is not None:
            d.target_positions = _rig_array(target_positions, np.float64, (-1, nv, 3), "target_positions", device, keep)
            d.n_targets = int(keep[-1].shape[0])
            d.target_normals = _rig_array(target_normals, np.float64, (d.n_targets, nv, 3), "target_normals", device, keep)
        elif target_normals is not None:
            raise ValueError("target_normals without target_positions")
        _check(lib().take_hip_rig_create(C.byref(d), C.byref(self._h)))
        self.n_vertices, self.n_joints, self.n_influences, self.n_targets, self.has_normals = nv, int(d.n_joints), int(d.n_influences), int(d.n_targets), normals is not None

    def info(self):
        """-> {"n_vertices", "n_joints", "n_influences", "n_targets", "has_normals", "device_bytes"} (take_hip_rig_info)"""
        nv, bytes_ = C.c_int64(), C.c_int64()
        nj, k, t, hn = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().take_hip_rig_info(self._h, C.byref(nv), C.byref(nj), C.byref(k), C.byref(t), C.byref(hn), C.byref(bytes_)))
        return {"n_vertices": nv.value, "n_joints": nj.value, "n_influences": k.value, "n_targets": t.value, "has_normals": bool(hn.value),
                "device_bytes": bytes_.value}

    def _pose(self, joint_xforms, target_weights, keep):
        """a TakeRigPose over host arrays, or over device tensors (both then)"""
        device = _on_device(joint_xforms) or _on_device(target_weights)
        p = D.TakeRigPose()
        p.joint_xforms = _rig_array(joint_xforms, np.float64, (self.n_joints, 3, 4), "joint_xforms", device, keep)
        p.target_weights = _rig_array(target_weights, np.float64, (self.n_targets,), "target_weights", device, keep)
        p.flags = D.TAKE_RIG_POSE_DEVICE_ARRAYS if device else 0
        return p, device

    def pose(self, joint_xforms=None, target_weights=None):
        """the rig under a pose (take_hip_rig_pose): joint_xforms (n_joints, 3, 4) joint -> world, target_weights (T,)
        -> the posed positions (n, 3), or (positions, normals) when the rig has normals; numpy arrays"""
        keep = []
        p, device = self._pose(joint_xforms, target_weights, keep)
        if device:
            import torch

            torch.cuda.current_stream(keep[0].device).synchronize()
        pos = np.zeros((self.n_vertices, 3), np.float64)
        nrm = np.zeros((self.n_vertices, 3), np.float64) if self.has_normals else None
        _check(lib().take_hip_rig_pose(self._h, C.byref(p), pos.ctypes.data, None if nrm is None else nrm.ctypes.data))
        return pos if nrm is None else (pos, nrm)

    def pose_device(self, out_positions, out_normals=None, joint_xforms=None, target_weights=None, stream=None):
        """the same into device memory (take_hip_rig_pose_device): out_positions, out_normals are (n, 3) float64 torch
        device tensors or integer device pointers; runs on `stream` (default: torch's current stream when a pose array
        is a device tensor, else the default stream) and blocks until done"""
        keep = []
        p, device = self._pose(joint_xforms, target_weights, keep)
        if stream is None and device:
            import torch

            stream = torch.cuda.current_stream(keep[0].device).cuda_stream
        _check(lib().take_hip_rig_pose_device(self._h, C.byref(p), C.c_void_p(_pointer(out_positions)), C.c_void_p(_pointer(out_normals)), C.c_void_p(stream or 0)))

    def close(self):
        if self._h:
            lib().take_hip_rig_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # (interpreter shutdown: the library may be gone)
            pass


def _subdiv_desc(indices, n_vertices, levels, uvs, keep):
    d = D.TakeSubdivDesc()
    idx = np.ascontiguousarray(indices, np.int32)
    if idx.ndim != 2 or idx.shape[1] != 3:
        raise ValueError(f"indices must have shape ('n', 3), not {idx.shape}")
    keep.append(idx)
    d.n_vertices, d.n_faces, d.indices, d.levels, d.flags = int(n_vertices), idx.shape[0], idx.ctypes.data, int(levels), 0
    if uvs is not None:
        uv = np.ascontiguousarray(uvs, np.float64)
        if uv.shape != (int(n_vertices), 2):
            raise ValueError(f"uvs must have shape ({int(n_vertices)}, 2), not {uv.shape}")
        keep.append(uv)
        d.uvs = uv.ctypes.data
    return d


def subdiv_counts(indices, n_vertices, levels):
    """(refined vertices, refined faces) of a cage under `levels` levels of Loop subdivision (take_hip_subdiv_counts);
    needs no GPU"""
    keep = []
    d = _subdiv_desc(indices, n_vertices, levels, None, keep)
    nv, nf = C.c_int64(), C.c_int64()
    _check(lib().take_hip_subdiv_counts(C.byref(d), C.byref(nv), C.byref(nf)))
    return nv.value, nf.value


def subdiv_topology(indices, n_vertices, levels, uvs=None):
    """the refined faces (n, 3) int32 and — for a cage with uvs — the refined uvs (n, 2), else None
    (take_hip_subdiv_topology); needs no GPU"""
    keep = []
    d = _subdiv_desc(indices, n_vertices, levels, uvs, keep)
    nv, nf = C.c_int64(), C.c_int64()
    _check(lib().take_hip_subdiv_counts(C.byref(d), C.byref(nv), C.byref(nf)))
    idx = np.zeros((nf.value, 3), np.int32)
    uv = np.zeros((nv.value, 2), np.float64) if uvs is not None else None
    _check(lib().take_hip_subdiv_topology(C.byref(d), idx.ctypes.data, None if uv is None else uv.ctypes.data))
    return idx, uv


class Subdiv:
    """Loop subdivision of one triangle cage on the device (take_hip_subdiv_create; include/take_hip.h has the scheme):
    made once from the cage's topology — indices (n_faces, 3), the vertex count, optional uvs (n_vertices, 2), 1..6
    levels —, it keeps the stencil tables in device memory; refine(), refine_device() and Scene.subdivide_meshes() turn
    cage positions into refined positions and vertex normals there.  Bound to the device current at its creation; not
    thread-safe."""

    def __init__(self, indices, n_vertices, levels, uvs=None):
        self._h = C.c_void_p()
        self._keep = []
        self._desc = _subdiv_desc(indices, n_vertices, levels, uvs, self._keep)
        self._has_uvs = uvs is not None
        _check(lib().take_hip_subdiv_create(C.byref(self._desc), C.byref(self._h)))
        info = self.info()
        self.cage_vertices, self.n_vertices, self.n_faces, self.levels = info["cage_vertices"], info["n_vertices"], info["n_faces"], info["levels"]

    def info(self):
        """-> {"cage_vertices", "n_vertices", "n_faces", "levels", "device_bytes"} (take_hip_subdiv_info)"""
        cv, nv, nf, bytes_ = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        lv = C.c_int32()
        _check(lib().take_hip_subdiv_info(self._h, C.byref(cv), C.byref(nv), C.byref(nf), C.byref(lv), C.byref(bytes_)))
        return {"cage_vertices": cv.value, "n_vertices": nv.value, "n_faces": nf.value, "levels": lv.value, "device_bytes": bytes_.value}

    def topology(self):
        """-> (refined indices (n_faces, 3) int32, refined uvs (n_vertices, 2) or None).  Every call builds the refined
        topology again on the host (take_hip_subdiv_topology over the kept description: one sort of the face sides per
        level, millions of them at 6 levels) — call it once per cage, when the scene's mesh is made"""
        idx = np.zeros((self.n_faces, 3), np.int32)
        uv = np.zeros((self.n_vertices, 2), np.float64) if self._has_uvs else None
        _check(lib().take_hip_subdiv_topology(C.byref(self._desc), idx.ctypes.data, None if uv is None else uv.ctypes.data))
        return idx, uv

    def _cage(self, cage, keep):
        """-> (pointer, flags, on the device?) of cage positions: a numpy array, or a torch device tensor"""
        device = _on_device(cage)
        ptr = _rig_array(cage, np.float64, (self.cage_vertices, 3), "cage", device, keep)
        if ptr is None:
            raise ValueError("cage positions are required")
        return ptr, (D.TAKE_SUBDIV_DEVICE_ARRAYS if device else 0), device

    def refine_device(self, out_positions, out_normals=None, cage=None, stream=None):
        """the cage refined into device memory (take_hip_subdiv_refine_device): out_positions, out_normals are
        (n_vertices, 3) float64 torch device tensors or integer device pointers (out_normals None: no normals); runs on
        `stream` (default: torch's current stream when the cage is a device tensor, else the default stream) and blocks
        until done"""
        keep = []
        ptr, flags, device = self._cage(cage, keep)
        if stream is None and device:
            import torch

            stream = torch.cuda.current_stream(keep[0].device).cuda_stream
        _check(lib().take_hip_subdiv_refine_device(self._h, C.c_void_p(ptr), flags, C.c_void_p(_pointer(out_positions)), C.c_void_p(_pointer(out_normals)),
                                                   C.c_void_p(stream or 0)))

    def refine(self, cage, normals=True):
        """-> (positions, normals), or positions alone with normals=False: (n_vertices, 3) numpy arrays.  A numpy cage
        takes take_hip_subdiv_refine; a torch device tensor is refined on torch's current stream and downloaded"""
        if _on_device(cage):
            import torch

            out_p = torch.empty((self.n_vertices, 3), dtype=torch.float64, device=cage.device)
            out_n = torch.empty((self.n_vertices, 3), dtype=torch.float64, device=cage.device) if normals else None
            self.refine_device(out_p, out_n, cage)
            return (out_p.cpu().numpy(), out_n.cpu().numpy()) if normals else out_p.cpu().numpy()
        keep = []
        ptr, _, _ = self._cage(cage, keep)
        pos = np.zeros((self.n_vertices, 3), np.float64)
        nrm = np.zeros((self.n_vertices, 3), np.float64) if normals else None
        _check(lib().take_hip_subdiv_refine(self._h, C.c_void_p(ptr), pos.ctypes.data, None if nrm is None else nrm.ctypes.data))
        return (pos, nrm) if normals else pos

    def close(self):
        if self._h:
            lib().take_hip_subdiv_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # (interpreter shutdown: the library may be gone)
            pass


DEBUG_TABLES = {"material": (0, 27, 14), "light": (1, 30, 9), "texture": (2, 6, 3), "to_world": (3, 6, 3),
                "hemicos": (4, 1, 4), "burley": (5, 30, 14)}


def debug_table(name, inp, rnd, precision=D.TAKE_PRECISION_F64):
    """Device shading functions on golden-table rows (test hook).  rnd: (n, 8) random_real draws per row."""
    kind, cin, cout = DEBUG_TABLES[name]
    inp = np.ascontiguousarray(inp, np.float64).reshape(-1, cin)
    rnd = np.ascontiguousarray(rnd, np.float64).reshape(-1, 8)
    n = inp.shape[0]
    out = np.zeros((n, cout), np.float64)
    f = lib().take_hip_debug_table
    f.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    _check(f(kind, precision, inp.ctypes.data, n, cin, rnd.ctypes.data, out.ctypes.data, cout))
    return out


class Scene:
    """A scene resident on the current HIP device: flattened `Scene` + wide BVH in HBM."""

    def __init__(self, scene_data, precision=D.TAKE_PRECISION_F32, bvh_threads=0, max_leaf_size=0,
                 builder=D.TAKE_BUILDER_AUTO, burley_lobes=False, flatten_instances=False):
        """flatten_instances: placements (TakeInstance) are expanded to world-space triangles by scene_create instead of
        being traversed on two levels (TAKE_INSTANCES_FLATTEN).
        burley_lobes: the scene's Disney materials (tags 7..11: Lambert clones, as upstream) are rendered with the
        real lobes (tags 12..16, an extension — DESIGN.md §4d)"""
        self.sd = scene_data
        self.precision = precision
        self.dtype = np.float32 if precision == D.TAKE_PRECISION_F32 else np.float64
        desc, keep = scene_data.to_desc()
        opts = D.TakeBuildOpts(precision, bvh_threads, max_leaf_size, builder, 1 if burley_lobes else 0,
                               D.TAKE_INSTANCES_FLATTEN if flatten_instances else D.TAKE_INSTANCES_TWO_LEVEL)
        h = C.c_void_p()
        _check(lib().take_hip_scene_create(C.byref(desc), C.byref(opts), C.byref(h)))
        self.h = h
        del keep

    def close(self):
        if getattr(self, "h", None):
            lib().take_hip_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _opts(self, spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator=0):
        spp = self.sd.spp if spp is None else spp  # (None: the scene description's)
        max_depth = self.sd.max_depth if max_depth is None else max_depth
        o = D.TakeRenderOpts()
        o.exact_bounces = int(getattr(self, "exact_bounces", 0))  # TAKE_PRECISION_MIXED scenes (0 = the library's default)
        o.spp, o.max_depth, o.seed, o.ray_epsilon = int(spp), int(max_depth), int(seed), float(ray_epsilon)
        o.strip_first, o.strip_stride, o.samples_per_batch = int(strip_first), int(strip_stride), int(samples_per_batch)
        o.integrator = int(integrator)
        return o

    def rows(self, strip_first=0, strip_stride=1):
        n = _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, None))
        out = (C.c_int32 * max(n, 1))()
        _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, out))
        return np.array(out[:n], np.int32)

    def render(self, spp=None, max_depth=None, seed=0, ray_epsilon=0.0, strip_first=0, strip_stride=1,
               samples_per_batch=0, integrator=0):
        """-> (rows, W, 3) image rows owned by this strip set, top row first (host array)."""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        n = _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, None))
        out = np.zeros((n, self.sd.width, 3), self.dtype)
        _check(lib().take_hip_render(self.h, C.byref(o), out.ctypes.data))
        return out

    def render_device(self, d_ptr, spp, max_depth, seed=0, ray_epsilon=0.0, strip_first=0, strip_stride=1,
                      samples_per_batch=0, stream=None, integrator=0):
        """Render into device memory at `d_ptr` (e.g. a torch tensor's data_ptr()); blocks until done."""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        _check(lib().take_hip_render_device(self.h, C.byref(o), C.c_void_p(d_ptr), C.c_void_p(stream or 0)))

    def render_exr_scanlines(self, spp=None, max_depth=None, seed=0, samples_per_batch=0, integrator=0):
        """Render and convert on the device: -> uint16 (H, 3, W), per scanline the B, G, R halves of the reference's
        image.exr (take_amd.exr.write_exr_scanlines frames them into the file)."""
        o = self._opts(spp, max_depth, seed, 0.0, 0, 1, samples_per_batch, integrator)
        out = np.zeros((self.sd.height, 3, self.sd.width), np.uint16)
        _check(lib().take_hip_render_exr_scanlines(self.h, C.byref(o), out.ctypes.data))
        return out

    def render_accumulate(self, d_ptr, more_spp, max_depth, seed=0, restart=False, ray_epsilon=0.0, strip_first=0,
                          strip_stride=1, samples_per_batch=0, stream=None, integrator=0):
        """progressive rendering: `more_spp` further samples per pixel, mean over all samples so far -> device buffer"""
        o = self._opts(more_spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        _check(lib().take_hip_render_accumulate(self.h, C.byref(o), 1 if restart else 0, C.c_void_p(d_ptr), C.c_void_p(stream or 0)))
        return int(lib().take_hip_accumulated_samples(self.h))

    def render_features(self, spp, seed=0, ray_epsilon=0.0, strip_first=0, strip_stride=1, samples_per_batch=0,
                        want=tuple(D.FEATURE_PLANES)):
        """first-hit feature buffers (take_hip_render_features) -> {name: host array} for the names in `want`: albedo and
        normal (rows, W, 3), depth and alpha (rows, W) in the scene's Real, shape_id and material_id (rows, W) int32; the
        rows of this strip set, top row first; sums over the samples / spp (alpha-premultiplied), ids of sample 0"""
        o = self._opts(spp, 0, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch)
        n = _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, None))
        out, bufs = {}, D.TakeFeatureBuffers()
        for name in want:
            per_pixel, real = D.FEATURE_PLANES[name]
            out[name] = np.zeros((n, self.sd.width) + ((3,) if per_pixel == 3 else ()), self.dtype if real else np.int32)
            setattr(bufs, name, out[name].ctypes.data)
        _check(lib().take_hip_render_features(self.h, C.byref(o), C.byref(bufs)))
        return out

    def render_features_device(self, ptrs, spp, seed=0, ray_epsilon=0.0, strip_first=0, strip_stride=1, samples_per_batch=0,
                               stream=None):
        """the same into device memory (take_hip_render_features_device); ptrs: {name: torch device tensor or integer
        device pointer} for the planes wanted — contiguous, of the scene's Real (int32 for the ids), sized for the rows
        of the strip set; blocks until done"""
        o = self._opts(spp, 0, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch)
        bufs = D.TakeFeatureBuffers()
        for name, p in ptrs.items():
            if name not in D.FEATURE_PLANES:
                raise ValueError(f"unknown feature plane {name!r}: one of {tuple(D.FEATURE_PLANES)}")
            setattr(bufs, name, _pointer(p))
        _check(lib().take_hip_render_features_device(self.h, C.byref(o), C.byref(bufs), C.c_void_p(stream or 0)))

    def render_denoised(self, spp=None, max_depth=None, seed=0, ray_epsilon=0.0, samples_per_batch=0, integrator=0, opts=None, **kw):
        """render the whole image, make albedo, normal and depth with the same options and filter, all on the device
        (take_hip_render_denoised) -> (H, W, 3) host array.  Equal bit for bit to render + render_features + denoise made
        by hand.  Denoise options: keywords of cdefs.denoise_opts, or opts = a TakeDenoiseOpts; neither = the defaults."""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        out = np.zeros((self.sd.height, self.sd.width, 3), self.dtype)
        _check(lib().take_hip_render_denoised(self.h, C.byref(o), None if opts is None else C.byref(opts), out.ctypes.data))
        return out

    def render_denoised_device(self, d_ptr, spp, max_depth, seed=0, ray_epsilon=0.0, samples_per_batch=0, stream=None, integrator=0,
                               opts=None, **kw):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer; H * W * 3 of the
        scene's Real); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        _check(lib().take_hip_render_denoised_device(self.h, C.byref(o), None if opts is None else C.byref(opts),
                                                     C.c_void_p(_pointer(d_ptr)), C.c_void_p(stream or 0)))

    def render_adaptive(self, spp=None, max_depth=None, seed=0, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0, stats=False, opts="keywords",
                        ray_epsilon=0.0, strip_first=0, strip_stride=1, samples_per_batch=0, integrator=0):
        """adaptive sampling (take_hip_render_adaptive): at most `spp` samples per pixel, a pixel stops once the relative
        standard error of its mean is <= threshold -> (rows, W, 3) host image of this strip set, top row first; a pixel
        that received c samples equals render(spp=c) there bit for bit.  stats=True: -> (image, {"count": int32 (rows, W),
        "m1", "m2": float64 (rows, W)}), the samples each pixel received and the sums of its sample values (r + g + b)
        and of their squares.  What is left out of min_spp / step_spp / threshold / floor takes the library's default
        (16, 8, 0.05, 1e-3; threshold 0 is a value); opts: a TakeAdaptiveOpts instead of the keywords, or None = a NULL
        pointer (all defaults)."""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        a = _adaptive_opts(opts, min_spp, step_spp, threshold, floor)
        n = _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, None))
        out = np.zeros((n, self.sd.width, 3), self.dtype)
        planes, st = _host_stats((n, self.sd.width)) if stats else (None, None)
        _check(lib().take_hip_render_adaptive(self.h, C.byref(o), None if a is None else C.byref(a), out.ctypes.data,
                                              None if st is None else C.byref(st)))
        return (out, planes) if stats else out

    def render_adaptive_device(self, d_ptr, spp, max_depth, seed=0, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0, stats=None, opts="keywords",
                               ray_epsilon=0.0, strip_first=0, strip_stride=1, samples_per_batch=0, stream=None, integrator=0):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer; rows * W * 3 of the
        scene's Real); stats: {"count" / "m1" / "m2": device tensor or pointer} for the planes wanted (int32, float64,
        float64; rows * W each); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        a = _adaptive_opts(opts, min_spp, step_spp, threshold, floor)
        st = _device_stats(stats)
        _check(lib().take_hip_render_adaptive_device(self.h, C.byref(o), None if a is None else C.byref(a), C.c_void_p(_pointer(d_ptr)),
                                                     None if st is None else C.byref(st), C.c_void_p(stream or 0)))

    def render_adaptive_denoised(self, spp=None, max_depth=None, seed=0, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0, stats=False, variance=False,
                                 adaptive="keywords", ray_epsilon=0.0, samples_per_batch=0, integrator=0, opts=None, **kw):
        """render the whole image adaptively, make albedo, normal and depth from min_spp samples and filter with the
        sampler's own moments, all on the device (take_hip_render_adaptive_denoised) -> (H, W, 3) host array.  Equal bit
        for bit to render_adaptive(stats=True) + render_features(the effective min_spp) + denoise_variance made by hand.
        stats=True and / or variance=True: -> (image, the planes of render_adaptive) / (image, variance plane) / (image,
        planes, variance plane).  Sampler options as render_adaptive takes them (adaptive: a TakeAdaptiveOpts instead of
        the keywords, or None = all defaults); denoise options: keywords of cdefs.denoise_opts, or opts = a
        TakeDenoiseOpts; neither = the defaults (sigma_color 4.0 standard deviations)."""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        a = _adaptive_opts(adaptive, min_spp, step_spp, threshold, floor)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        h, w = self.sd.height, self.sd.width
        out = np.zeros((h, w, 3), self.dtype)
        planes, st = _host_stats((h, w)) if stats else (None, None)
        var = np.zeros((h, w), self.dtype) if variance else None
        _check(lib().take_hip_render_adaptive_denoised(self.h, C.byref(o), None if a is None else C.byref(a), None if opts is None else C.byref(opts),
                                                       out.ctypes.data, None if st is None else C.byref(st), None if var is None else var.ctypes.data))
        extra = ([planes] if stats else []) + ([var] if variance else [])
        return (out, *extra) if extra else out

    def render_adaptive_denoised_device(self, d_ptr, spp, max_depth, seed=0, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0, stats=None, variance=None,
                                        adaptive="keywords", ray_epsilon=0.0, samples_per_batch=0, stream=None, integrator=0, opts=None, **kw):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer; H * W * 3 of the
        scene's Real); stats: {"count" / "m1" / "m2": device tensor or pointer} for the planes wanted; variance: the
        optional (H * W of the scene's Real) output plane; blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        a = _adaptive_opts(adaptive, min_spp, step_spp, threshold, floor)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        st = _device_stats(stats)
        _check(lib().take_hip_render_adaptive_denoised_device(self.h, C.byref(o), None if a is None else C.byref(a), None if opts is None else C.byref(opts),
                                                              C.c_void_p(_pointer(d_ptr)), None if st is None else C.byref(st), C.c_void_p(_pointer(variance)),
                                                              C.c_void_p(stream or 0)))

    def mark_frame(self):
        """store "the previous frame" in the handle (take_hip_scene_mark_frame): the current camera and, in a two-level
        scene, the placements' current transforms — what render_motion takes surface points back to"""
        _check(lib().take_hip_scene_mark_frame(self.h))

    def track_vertices(self, on=True):
        """let the motion pass follow vertices that move after a mark (take_hip_scene_track_vertices): with tracking on,
        the first set_mesh_vertices / update_meshes after a mark keeps the marked frame's geometry; off (the default)
        drops it"""
        _check(lib().take_hip_scene_track_vertices(self.h, D.TAKE_TRACK_VERTICES if on else 0))

    def tracking_info(self):
        """-> {"flags", "marked_bytes"}: whether tracking is on, and the device bytes of marked geometry the handle holds
        (take_hip_scene_tracking_info)"""
        flags, held = C.c_int32(-1), C.c_int64(-1)
        _check(lib().take_hip_scene_tracking_info(self.h, C.byref(flags), C.byref(held)))
        return {"flags": flags.value, "marked_bytes": held.value}

    def render_motion(self, ray_epsilon=0.0, want=tuple(D.MOTION_PLANES)):
        """the motion pass against the marked frame (take_hip_render_motion) -> {name: host array} for the names in
        `want`: prev_xy (H, W, 2), prev_depth and depth (H, W) in the scene's Real, shape_id (H, W) int32; row 0 = top"""
        o = self._opts(1, 0, 0, ray_epsilon, 0, 1, 0)
        out, bufs = {}, D.TakeMotionBuffers()
        for name in want:
            if name not in D.MOTION_PLANES:
                raise ValueError(f"unknown motion plane {name!r}: one of {tuple(D.MOTION_PLANES)}")
            per_pixel, real = D.MOTION_PLANES[name]
            out[name] = np.zeros((self.sd.height, self.sd.width) + ((per_pixel,) if per_pixel > 1 else ()), self.dtype if real else np.int32)
            setattr(bufs, name, out[name].ctypes.data)
        _check(lib().take_hip_render_motion(self.h, C.byref(o), C.byref(bufs)))
        return out

    def render_motion_device(self, ptrs, ray_epsilon=0.0, stream=None):
        """the same into device memory (take_hip_render_motion_device); ptrs: {name: torch device tensor or integer device
        pointer} for the planes wanted — contiguous, of the scene's Real (int32 for shape_id); blocks until done"""
        o = self._opts(1, 0, 0, ray_epsilon, 0, 1, 0)
        bufs = D.TakeMotionBuffers()
        for name, p in ptrs.items():
            if name not in D.MOTION_PLANES:
                raise ValueError(f"unknown motion plane {name!r}: one of {tuple(D.MOTION_PLANES)}")
            setattr(bufs, name, _pointer(p))
        _check(lib().take_hip_render_motion_device(self.h, C.byref(o), C.byref(bufs), C.c_void_p(stream or 0)))

    def render_temporal(self, spp=None, max_depth=None, seed=0, restart=False, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0, adaptive="keywords",
                        temporal=None, ray_epsilon=0.0, samples_per_batch=0, integrator=0, opts=None, **kw):
        """one frame of an animation (take_hip_render_temporal): render adaptively, accumulate onto the handle's history
        through the motion pass, filter with the accumulated statistics, mark the frame -> (H, W, 3) host array.  Equal
        bit for bit to render_adaptive + render_motion + temporal_accumulate + render_features + denoise_variance +
        mark_frame made by hand.  Change `seed` from frame to frame.  restart=True: drop the history.  Sampler options as
        render_adaptive takes them; temporal: a TakeTemporalOpts or None = the defaults; denoise options as
        render_adaptive_denoised takes them."""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        a = _adaptive_opts(adaptive, min_spp, step_spp, threshold, floor)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        out = np.zeros((self.sd.height, self.sd.width, 3), self.dtype)
        _check(lib().take_hip_render_temporal(self.h, C.byref(o), None if a is None else C.byref(a), None if temporal is None else C.byref(temporal),
                                              None if opts is None else C.byref(opts), 1 if restart else 0, out.ctypes.data))
        return out

    def render_temporal_device(self, d_ptr, spp, max_depth, seed=0, restart=False, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0, adaptive="keywords",
                               temporal=None, ray_epsilon=0.0, samples_per_batch=0, stream=None, integrator=0, opts=None, **kw):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer; H * W * 3 of the
        scene's Real); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        a = _adaptive_opts(adaptive, min_spp, step_spp, threshold, floor)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        _check(lib().take_hip_render_temporal_device(self.h, C.byref(o), None if a is None else C.byref(a), None if temporal is None else C.byref(temporal),
                                                     None if opts is None else C.byref(opts), 1 if restart else 0, C.c_void_p(_pointer(d_ptr)),
                                                     C.c_void_p(stream or 0)))

    def set_instance_transforms(self, xforms, stream=None):
        """new object -> world transforms for ALL placements of a two-level scene, (n, 3, 4) float64 in the order of the
        description's instances; only the top level is rebuilt, on the device (take_hip_scene_set_instance_transforms).
        A numpy array (or anything numpy converts) goes through the host entry point; a torch device tensor or an
        integer device pointer — then `n` is the scene's placement count — through the device one."""
        if isinstance(xforms, int):
            n, ptr = len(self.sd.instance_mesh), xforms
        elif hasattr(xforms, "data_ptr") and getattr(xforms, "is_cuda", False):
            if str(xforms.dtype) != "torch.float64" or not xforms.is_contiguous() or xforms.numel() % 12:
                raise ValueError("transforms on the device must be a contiguous float64 tensor of shape (n, 3, 4)")
            n, ptr = xforms.numel() // 12, xforms.data_ptr()
        else:
            if hasattr(xforms, "data_ptr"):  # a torch tensor in host memory
                xforms = xforms.numpy()
            x = np.ascontiguousarray(xforms, np.float64)
            if x.size % 12:
                raise ValueError("transforms must have shape (n, 3, 4)")
            _check(lib().take_hip_scene_set_instance_transforms(self.h, x.ctypes.data, x.size // 12))
            return
        _check(lib().take_hip_scene_set_instance_transforms_device(self.h, C.c_void_p(ptr), n, C.c_void_p(stream or 0)))

    def set_envmap(self, image, scale=None, stream=None):
        """a new environment map for the resident scene (take_hip_scene_set_envmap): `image` is (h, w, 3), row 0 = zenith —
        a numpy float32 or float64 array (anything else numpy converts is taken as float64) read from host memory, or a
        contiguous float32 / float64 torch tensor on the device, read through its device pointer after `stream` (default:
        torch's current stream).  scale: the light's new (r, g, b) intensity, None = keep.  The tables are built on the
        device; afterwards the scene equals one newly created from its description with this image and scale."""
        sc = None if scale is None else D.c_double3(*map(float, scale))
        if hasattr(image, "data_ptr") and getattr(image, "is_cuda", False):
            reals = {"torch.float32": D.TAKE_PRECISION_F32, "torch.float64": D.TAKE_PRECISION_F64}
            if str(image.dtype) not in reals or not image.is_contiguous() or image.dim() != 3 or image.shape[2] != 3:
                raise ValueError("an environment map on the device must be a contiguous float32 or float64 tensor of shape (h, w, 3)")
            if stream is None:
                import torch

                stream = torch.cuda.current_stream(image.device).cuda_stream
            im = D.TakeEnvImage(int(image.shape[1]), int(image.shape[0]), image.data_ptr(), reals[str(image.dtype)], D.TAKE_MESH_DEVICE_ARRAYS)
            _check(lib().take_hip_scene_set_envmap_device(self.h, C.byref(im), sc, C.c_void_p(stream or 0)))
            return
        if hasattr(image, "data_ptr"):  # a torch tensor in host memory
            image = image.numpy()
        a = np.asarray(image)
        a = np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.float64)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("an environment map must have shape (h, w, 3)")
        im = D.TakeEnvImage(a.shape[1], a.shape[0], a.ctypes.data, D.TAKE_PRECISION_F32 if a.dtype == np.float32 else D.TAKE_PRECISION_F64, 0)
        _check(lib().take_hip_scene_set_envmap(self.h, C.byref(im), sc))

    def set_materials(self, materials, first=0):
        """new materials for the resident scene (take_hip_scene_set_materials): `materials` is a list of
        take_amd.scene.Material that replaces the scene's materials first, first + 1, ...; the table keeps its size and
        every shape, mesh and placement keeps its material id.  Afterwards the scene equals one newly created from its
        description with these materials."""
        materials = list(materials)
        mats = (D.TakeMaterial * max(len(materials), 1))()
        for c, m in zip(mats, materials):
            D.fill_material(c, m)
        _check(lib().take_hip_scene_set_materials(self.h, mats, int(first), len(materials)))

    def set_light_intensities(self, rgb, first=0, stream=None):
        """new (r, g, b) intensities for the lights first, first + 1, ... of the resident scene
        (take_hip_scene_set_light_intensities): a (count, 3) numpy array (or anything numpy converts) read from host
        memory, or a contiguous float64 torch tensor of that shape on the device, read through its device pointer after
        `stream` (default: torch's current stream).  Kinds and geometry stay; the power tables are made again."""
        if hasattr(rgb, "data_ptr") and getattr(rgb, "is_cuda", False):
            if str(rgb.dtype) != "torch.float64" or not rgb.is_contiguous() or rgb.dim() != 2 or rgb.shape[1] != 3:
                raise ValueError("intensities on the device must be a contiguous float64 tensor of shape (count, 3)")
            if stream is None:
                import torch

                stream = torch.cuda.current_stream(rgb.device).cuda_stream
            _check(lib().take_hip_scene_set_light_intensities_device(self.h, C.c_void_p(rgb.data_ptr()), int(first), int(rgb.shape[0]), C.c_void_p(stream or 0)))
            return
        if hasattr(rgb, "data_ptr"):  # a torch tensor in host memory
            rgb = rgb.numpy()
        a = np.ascontiguousarray(rgb, np.float64)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("intensities must have shape (count, 3)")
        _check(lib().take_hip_scene_set_light_intensities(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), int(first), a.shape[0]))

    def set_camera(self, lookfrom, lookat, up, vfov, width=None, height=None):
        """a new camera for the resident scene (take_hip_scene_set_camera); width and height stay the scene's"""
        cam = D.TakeCamera(self.sd.width if width is None else int(width), self.sd.height if height is None else int(height),
                           D.c_double3(*map(float, lookfrom)), D.c_double3(*map(float, lookat)), D.c_double3(*map(float, up)), float(vfov))
        _check(lib().take_hip_scene_set_camera(self.h, C.byref(cam)))

    def set_lens(self, aperture_radius, focus_distance=0.0):
        """a thin lens for the resident scene (take_hip_scene_set_lens): aperture radius in world units, 0 = back to the
        pinhole camera; focus_distance along the view axis, <= 0 = |lookat - lookfrom| of the current camera"""
        lens = D.TakeLens(float(aperture_radius), float(focus_distance), 0, 0)
        _check(lib().take_hip_scene_set_lens(self.h, C.byref(lens)))

    def get_lens(self):
        """-> {"aperture_radius", "focus_distance"}: the radius as given and the focus distance in effect (take_hip_scene_get_lens)"""
        lens = D.TakeLens()
        _check(lib().take_hip_scene_get_lens(self.h, C.byref(lens)))
        return {"aperture_radius": lens.aperture_radius, "focus_distance": lens.focus_distance}

    def focus_distance_at(self, column, row):
        """the distance along the view axis of the surface the centre ray of pixel (column, row; row 0 = top) sees, 0 for
        a miss (take_hip_scene_focus_distance_at): what set_lens takes as focus_distance to focus on it"""
        out = C.c_double(-1.0)
        _check(lib().take_hip_scene_focus_distance_at(self.h, int(column), int(row), C.byref(out)))
        return out.value

    def render_shutter(self, spp=None, max_depth=None, seed=0, open=0.0, close=1.0, slices=0, ray_epsilon=0.0, strip_first=0,
                       strip_stride=1, samples_per_batch=0, integrator=0):
        """motion blur (take_hip_render_shutter): a render whose exposure lasts from scene time `open` to `close`, 0 being
        the marked frame (mark_frame) and 1 the current one; the samples are cut into `slices` slices (<= 0: min(spp, 16)),
        each rendered with camera and placements lerped to its time; the scene is at its current pose again afterwards
        -> (rows, W, 3) host array, as render's"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        sh = D.TakeShutter(float(open), float(close), int(slices), 0)
        n = _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, None))
        out = np.zeros((n, self.sd.width, 3), self.dtype)
        _check(lib().take_hip_render_shutter(self.h, C.byref(o), C.byref(sh), out.ctypes.data))
        return out

    def render_shutter_device(self, d_ptr, spp, max_depth, seed=0, open=0.0, close=1.0, slices=0, ray_epsilon=0.0, strip_first=0,
                              strip_stride=1, samples_per_batch=0, stream=None, integrator=0):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        sh = D.TakeShutter(float(open), float(close), int(slices), 0)
        _check(lib().take_hip_render_shutter_device(self.h, C.byref(o), C.byref(sh), C.c_void_p(_pointer(d_ptr)), C.c_void_p(stream or 0)))

    def _motions(self, motions, stream):
        """[(mesh_id, positions0, positions1[, normals0, normals1]), ...] -> (TakeMeshMotion array, n, what keeps the
        arrays alive); device tensors are waited for on `stream` (default: torch's current stream)"""
        motions = list(motions)
        recs = (D.TakeMeshMotion * max(len(motions), 1))()
        keep, wait = [], None
        for k, m in enumerate(motions):
            if len(m) not in (3, 5):
                raise ValueError("a motion is (mesh_id, positions0, positions1) or (mesh_id, positions0, positions1, normals0, normals1)")
            arrays = list(m[1:]) + [None] * (5 - len(m))
            device = _on_device(arrays[0])
            ptrs = []
            for a in arrays:
                if a is None:
                    ptrs.append(None)
                elif device:
                    if not _on_device(a) or str(a.dtype) != "torch.float64" or not a.is_contiguous():
                        raise ValueError("arrays on the device must be contiguous float64 tensors, and all arrays of a mesh on the device")
                    keep.append(a)
                    ptrs.append(a.data_ptr())
                    wait = a.device if wait is None else wait
                else:
                    a = np.ascontiguousarray(a.numpy() if hasattr(a, "data_ptr") else a, np.float64)
                    keep.append(a)
                    ptrs.append(a.ctypes.data)
            recs[k].mesh, recs[k].flags = int(m[0]), D.TAKE_MESH_DEVICE_ARRAYS if device else 0
            recs[k].positions0, recs[k].positions1, recs[k].normals0, recs[k].normals1 = ptrs
        if wait is not None:
            import torch

            (torch.cuda.current_stream(wait) if stream is None else torch.cuda.ExternalStream(int(stream), device=wait)).synchronize()
        return recs, len(motions), keep

    def render_shutter_meshes(self, motions, spp=None, max_depth=None, seed=0, open=0.0, close=1.0, slices=0, ray_epsilon=0.0, strip_first=0,
                              strip_stride=1, samples_per_batch=0, integrator=0, stream=None):
        """motion blur for deforming meshes (take_hip_render_shutter_meshes): render_shutter, with the vertices of the
        named meshes lerped to every slice's time.  `motions` is [(mesh_id, positions0, positions1), ...] or, for a mesh
        with vertex normals, [(mesh_id, positions0, positions1, normals0, normals1), ...]: (n_vertices, 3) float64 arrays
        at the marked frame (0) and at the current one (1) — numpy arrays, or contiguous torch device tensors (all arrays
        of a mesh on the device), which are waited for on `stream` (default: torch's current stream) first.  The scene
        must BE at the ...1 arrays; it is again afterwards -> (rows, W, 3) host array, as render's.

        With a rig: pose it twice into two tensors, bring the scene to the current pose, pass both —
            p0, n0, p1, n1 = (torch.empty((rig.n_vertices, 3), dtype=torch.float64, device="cuda") for _ in range(4))
            rig.pose_device(p0, n0, joints_then)          # the pose at the marked frame
            rig.pose_device(p1, n1, joints_now)           # the current pose
            scene.update_meshes({mesh_id: (p1, n1)})      # or scene.pose_meshes([(mesh_id, rig, joints_now, None)])
            image = scene.render_shutter_meshes([(mesh_id, p0, p1, n0, n1)], spp=64)"""
        recs, n, keep = self._motions(motions, stream)
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        sh = D.TakeShutter(float(open), float(close), int(slices), 0)
        rows = _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, None))
        out = np.zeros((rows, self.sd.width, 3), self.dtype)
        _check(lib().take_hip_render_shutter_meshes(self.h, C.byref(o), C.byref(sh), recs, n, out.ctypes.data))
        del keep
        return out

    def render_shutter_meshes_device(self, d_ptr, motions, spp, max_depth, seed=0, open=0.0, close=1.0, slices=0, ray_epsilon=0.0, strip_first=0,
                                     strip_stride=1, samples_per_batch=0, stream=None, integrator=0):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer); blocks until done"""
        recs, n, keep = self._motions(motions, stream)
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        sh = D.TakeShutter(float(open), float(close), int(slices), 0)
        _check(lib().take_hip_render_shutter_meshes_device(self.h, C.byref(o), C.byref(sh), recs, n, C.c_void_p(_pointer(d_ptr)), C.c_void_p(stream or 0)))
        del keep

    def shutter_pose(self, t):
        """the pose render_shutter gives the scene at scene time t in [0, 1] (take_hip_shutter_pose) -> {"lookfrom", "lookat",
        "up" (3,), "vfov", "xforms" (n, 3, 4) float64 — n = 0 for a scene without placements}"""
        cam = D.TakeCamera()
        x = np.zeros((len(self.sd.instance_mesh), 3, 4), np.float64)
        _check(lib().take_hip_shutter_pose(self.h, float(t), C.byref(cam), x.ctypes.data if x.size else None))
        return {"lookfrom": np.array(cam.lookfrom[:]), "lookat": np.array(cam.lookat[:]), "up": np.array(cam.up[:]), "vfov": cam.vfov, "xforms": x}

    def update_meshes(self, updates):
        """new vertices for meshes of ANY scene, two-level ones included (take_hip_scene_update_meshes): the arguments of
        set_mesh_vertices.  In a two-level scene a named mesh moves in every role it has — its faces among the shapes,
        and as the prototype of placements, whose tree is rebuilt on the device — and the top level is rebuilt under the
        scene's current transforms; afterwards the scene traces and renders as one newly created from the description
        with these arrays and those transforms.  A scene without placements: the same as set_mesh_vertices."""
        self.set_mesh_vertices(updates, _entry="take_hip_scene_update_meshes")

    def pose_meshes(self, bindings, stream=None):
        """skin / morph meshes of the resident scene and update it in one step (take_hip_scene_pose_meshes): `bindings` is
        [(mesh_id, rig, joint_xforms, target_weights), ...] — a Rig of the mesh's vertex count and a pose as Rig.pose
        takes it (None for what the rig has none of).  Every rig is posed into its own device buffers and the scene takes
        update_meshes' path over them: afterwards it equals the scene after update_meshes({mesh_id: rig.pose(...)}).
        Pose arrays may be device tensors written on `stream` (default: torch's current stream), which the call waits
        for first."""
        bindings = list(bindings)
        recs = (D.TakeRigBinding * max(len(bindings), 1))()
        keep, wait = [], None
        for k, (mesh, rig, joint_xforms, target_weights) in enumerate(bindings):
            if not isinstance(rig, Rig) or not rig._h:
                raise ValueError("a binding's rig must be an open Rig")
            pose, device = rig._pose(joint_xforms, target_weights, keep)
            if device and wait is None:
                wait = keep[-1].device
            recs[k].mesh, recs[k].rig, recs[k].pose = int(mesh), rig._h, pose
        if wait is not None:
            import torch

            (torch.cuda.current_stream(wait) if stream is None else torch.cuda.ExternalStream(int(stream), device=wait)).synchronize()
        _check(lib().take_hip_scene_pose_meshes(self.h, recs, len(bindings)))
        del keep

    def subdivide_meshes(self, bindings, stream=None):
        """refine cages by Loop subdivision and update the resident scene in one step (take_hip_scene_subdivide_meshes):
        `bindings` is [(mesh_id, subdiv, cage), ...] — a Subdiv whose refined vertex count is the mesh's, and cage
        positions (cage_vertices, 3) as a numpy array or a torch device tensor — or [(mesh_id, subdiv, (rig,
        joint_xforms, target_weights)), ...]: the cage is then the rig's pose.  Afterwards the scene equals the one
        after update_meshes({mesh_id: subdiv.refine(cage)}); normals go to meshes that have vertex normals.  Device
        tensors may have been written on `stream` (default: torch's current stream), which the call waits for first."""
        bindings = list(bindings)
        recs = (D.TakeSubdivBinding * max(len(bindings), 1))()
        keep, wait = [], None
        for k, (mesh, subdiv, cage) in enumerate(bindings):
            if not isinstance(subdiv, Subdiv) or not subdiv._h:
                raise ValueError("a binding's subdiv must be an open Subdiv")
            recs[k].mesh, recs[k].subdiv = int(mesh), subdiv._h
            if isinstance(cage, tuple):
                rig, joint_xforms, target_weights = cage
                if not isinstance(rig, Rig) or not rig._h:
                    raise ValueError("a binding's rig must be an open Rig")
                pose, device = rig._pose(joint_xforms, target_weights, keep)
                recs[k].rig, recs[k].pose = rig._h, pose
            elif cage is not None:
                recs[k].cage_positions, recs[k].flags, device = subdiv._cage(cage, keep)
            else:
                device = False
            if device and wait is None:
                wait = keep[-1].device
        if wait is not None:
            import torch

            (torch.cuda.current_stream(wait) if stream is None else torch.cuda.ExternalStream(int(stream), device=wait)).synchronize()
        _check(lib().take_hip_scene_subdivide_meshes(self.h, recs, len(bindings)))
        del keep

    def set_mesh_vertices(self, updates, _entry="take_hip_scene_set_mesh_vertices"):
        """new vertices for meshes of a scene without placements (take_hip_scene_set_mesh_vertices): `updates` is
        {mesh_id: positions} or {mesh_id: (positions, normals)} (a tuple), every array (n_vertices, 3) float64 and complete, normals
        None = keep.  numpy arrays (or anything numpy converts) are read from host memory; torch device tensors —
        contiguous float64, all arrays of one mesh on the device — through their device pointers.  The tree is rebuilt
        on the device; afterwards the scene equals one newly created from the description with these arrays."""
        recs = (D.TakeMeshUpdate * max(len(updates), 1))()
        keep = []

        def on_device(a):
            return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)

        def pointer(a, device):
            if a is None:
                return None
            if device:
                if not on_device(a) or str(a.dtype) != "torch.float64" or not a.is_contiguous():
                    raise ValueError("arrays on the device must be contiguous float64 tensors, and all arrays of a mesh on the device")
                keep.append(a)
                return a.data_ptr()
            if hasattr(a, "data_ptr"):  # a torch tensor in host memory
                a = a.numpy()
            a = np.ascontiguousarray(a, np.float64)
            keep.append(a)
            return a.ctypes.data

        for k, (mesh, arrays) in enumerate(updates.items()):
            pos, nrm = arrays if isinstance(arrays, tuple) and len(arrays) == 2 else (arrays, None)
            device = on_device(pos)
            recs[k].mesh, recs[k].flags = int(mesh), D.TAKE_MESH_DEVICE_ARRAYS if device else 0
            recs[k].positions, recs[k].normals = pointer(pos, device), pointer(nrm, device)
        _check(getattr(lib(), _entry)(self.h, recs, len(updates)))
        del keep

    def trace_closest(self, rays_abi):
        """rays_abi: (n,8) array in TakeRayF/D layout (org3 tmin dir3 tmax) -> structured hits"""
        rays = np.ascontiguousarray(rays_abi, self.dtype)
        n = rays.shape[0]
        if self.precision != D.TAKE_PRECISION_F32:
            hits = np.zeros(n, dtype=[("shape_id", "<i4"), ("reserved", "<i4"), ("t", "<f8"), ("u", "<f8"), ("v", "<f8")])
        else:
            hits = np.zeros(n, dtype=[("shape_id", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4")])
        _check(lib().take_hip_trace_closest(self.h, rays.ctypes.data, n, hits.ctypes.data))
        return hits

    def trace_any(self, rays_abi):
        rays = np.ascontiguousarray(rays_abi, self.dtype)
        occ = np.zeros(rays.shape[0], np.int32)
        _check(lib().take_hip_trace_any(self.h, rays.ctypes.data, rays.shape[0],
                                        occ.ctypes.data_as(C.POINTER(C.c_int32))))
        return occ

    def trace_closest_device(self, d_rays, n, d_hits, count_mode=False, stream=None):
        _check(lib().take_hip_trace_closest_device(self.h, C.c_void_p(d_rays), int(n), C.c_void_p(d_hits),
                                                   int(count_mode), C.c_void_p(stream or 0)))

    def _ray_batch(self, ptr, n, ray_sets, first_sample, normalize):
        return D.TakeRayBatch(ptr, int(n), int(ray_sets), int(first_sample), D.TAKE_RAYS_NORMALIZE if normalize else 0, 0)

    def render_rays(self, rays, spp, max_depth=None, seed=0, ray_epsilon=0.0, samples_per_batch=0, integrator=0, ray_sets=1, first_sample=0,
                    normalize=False):
        """path tracing of the caller's rays (take_hip_render_rays): rays is (n, 8) — or (ray_sets, n, 8) — in TakeRayF/D
        layout (org3 tmin dir3 tmax; tmin and tmax are ignored, directions of unit length unless normalize=True) ->
        (n, 3) host array in the scene's Real, texel i the mean over spp samples of the radiance along ray i.  ray_sets:
        1 = ray i serves all samples, spp = sample s of texel i travels along rays[s, i].  The random stream of sample s
        of ray i is a render's for sample first_sample + s of pixel index i."""
        rays = np.ascontiguousarray(rays, self.dtype)
        if rays.shape[-1] != 8 or rays.size % (8 * int(ray_sets)):
            raise ValueError("rays must have shape (n, 8) or (ray_sets, n, 8)")
        n = rays.size // (8 * int(ray_sets))
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        b = self._ray_batch(rays.ctypes.data, n, ray_sets, first_sample, normalize)
        out = np.zeros((n, 3), self.dtype)
        _check(lib().take_hip_render_rays(self.h, C.byref(o), C.byref(b), out.ctypes.data))
        return out

    def render_rays_device(self, d_rays, n, d_out, spp, max_depth, seed=0, ray_epsilon=0.0, samples_per_batch=0, stream=None, integrator=0,
                           ray_sets=1, first_sample=0, normalize=False):
        """the same on device memory (take_hip_render_rays_device): d_rays and d_out are torch device tensors or integer
        device pointers (e.g. a tensor's data_ptr()) — ray_sets * n records of 8 Reals, 16-byte aligned, and n * 3 Reals
        of the scene's Real; the rays are taken as they are (unit directions, or normalize=True); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        b = self._ray_batch(_pointer(d_rays), n, ray_sets, first_sample, normalize)
        _check(lib().take_hip_render_rays_device(self.h, C.byref(o), C.byref(b), C.c_void_p(_pointer(d_out)), C.c_void_p(stream or 0)))

    def camera_rays(self, spp, seed=0, first_sample=0, ray_epsilon=0.0):
        """the scene's own camera rays (take_hip_camera_rays) -> (spp, H * W, 8) host array in TakeRayF/D layout: set s
        holds the rays a whole-image render with this seed traces for sample first_sample + s, ray i = y * W + x with
        y = 0 the BOTTOM image row; tmin = the effective ray epsilon, tmax = inf.  Goes into trace_closest as it is, and
        back into render_rays(ray_sets=spp), whose image — flipped vertically — is render()'s bit for bit."""
        o = self._opts(spp, 0, seed, ray_epsilon, 0, 1, 0)
        out = np.zeros((int(spp), self.sd.height * self.sd.width, 8), self.dtype)
        _check(lib().take_hip_camera_rays(self.h, C.byref(o), int(first_sample), out.ctypes.data))
        return out

    def camera_rays_device(self, d_rays_out, spp, seed=0, first_sample=0, ray_epsilon=0.0, stream=None):
        """the same into device memory (take_hip_camera_rays_device): d_rays_out is a torch device tensor or an integer
        device pointer of spp * H * W * 8 of the scene's Real, 16-byte aligned; blocks until done"""
        o = self._opts(spp, 0, seed, ray_epsilon, 0, 1, 0)
        _check(lib().take_hip_camera_rays_device(self.h, C.byref(o), int(first_sample), C.c_void_p(_pointer(d_rays_out)), C.c_void_p(stream or 0)))

    def set_instrumentation(self, timing=False, counting=False):
        _check(lib().take_hip_set_instrumentation(self.h, (1 if timing else 0) | (2 if counting else 0)))

    def counters(self):
        c = D.TakeCounters()
        _check(lib().take_hip_get_counters(self.h, C.byref(c)))
        return c.as_dict()

    def stats(self):
        nn, npr, dep, by = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
        _check(lib().take_hip_scene_stats(self.h, C.byref(nn), C.byref(npr), C.byref(dep), C.byref(by)))
        return {"n_nodes": nn.value, "n_prims": npr.value, "depth": dep.value, "device_bytes": by.value}

    def debug_env(self, kind, inp, side=None):
        """the shade kernel's environment-map functions on this scene's resident tables (take_hip_debug_env, a test hook).
        kind 0: (n, 2) draws (u1, u2) -> (n, 8) dir[3], radiance[3], pdf, texel y * width + x; kind 1: (n, 3) directions
        -> (n, 5) radiance[3], pdf, texel.  side: TAKE_PRECISION_F32 / _F64 (default: the scene's own, F64 for MIXED)"""
        if side is None:
            side = D.TAKE_PRECISION_F32 if self.precision == D.TAKE_PRECISION_F32 else D.TAKE_PRECISION_F64
        inp = np.ascontiguousarray(inp, np.float64).reshape(-1, 3 if kind else 2)
        out = np.zeros((inp.shape[0], 5 if kind else 8), np.float64)
        _check(lib().take_hip_debug_env(self.h, int(side), int(kind), inp.ctypes.data, inp.shape[0], out.ctypes.data))
        return out

    def debug_env_tables(self, side=None):
        """the environment map of one resident side, read back from device memory as the shade kernels read it
        (take_hip_debug_env_tables, a test hook) -> {"width", "height", "n_guide_m", "n_guide_c", "texel0", "scale",
        "intensity", "marginal" (h + 1,), "conditional" (h, w + 1), "guide_m" (n_guide_m + 1,), "guide_c" (h, n_guide_c + 1),
        "texels" (h, w, 3), "images" (n_images,) of cdefs.IMAGE_INFO_DTYPE}.  side: as debug_env's"""
        if side is None:
            side = D.TAKE_PRECISION_F32 if self.precision == D.TAKE_PRECISION_F32 else D.TAKE_PRECISION_F64
        info = D.TakeDebugEnvTablesInfo()
        _check(lib().take_hip_debug_env_tables_info(self.h, int(side), C.byref(info)))
        w, h, real = info.width, info.height, np.float32 if info.real_bytes == 4 else np.float64
        out = {"marginal": np.zeros(h + 1, real), "conditional": np.zeros((h, w + 1), real), "guide_m": np.zeros(info.n_guide_m + 1, np.int32),
               "guide_c": np.zeros((h, info.n_guide_c + 1), np.int32), "texels": np.zeros((h, w, 3), real),
               "images": np.zeros(max(info.n_images, 1), D.IMAGE_INFO_DTYPE)}
        _check(lib().take_hip_debug_env_tables(self.h, int(side), *(out[k].ctypes.data for k in ("marginal", "conditional", "guide_m", "guide_c", "texels", "images"))))
        out["images"] = out["images"][:info.n_images]
        out.update(width=w, height=h, n_guide_m=info.n_guide_m, n_guide_c=info.n_guide_c, texel0=info.texel0, scale=np.array(info.scale[:]),
                   intensity=np.array(info.intensity[:]))
        return out

    def debug_shading_tables(self, side=None):
        """the shading tables of one resident side, read back from device memory as the kernels read them
        (take_hip_debug_shading_tables, a test hook) -> {"materials", "lights", "inst_shade": numpy structured arrays
        (cdefs.shading_table_dtypes), "light_pmf", "light_cdf": arrays of the side's Real, "tag_mask", "n_material_tags",
        "single_tag": what the host holds of the tags in use, "real_bytes"}.  side: as debug_env's"""
        if side is None:
            side = D.TAKE_PRECISION_F32 if self.precision == D.TAKE_PRECISION_F32 else D.TAKE_PRECISION_F64
        info = D.TakeDebugShadingTablesInfo()
        _check(lib().take_hip_debug_shading_tables_info(self.h, int(side), C.byref(info)))
        material, light, inst = D.shading_table_dtypes(info.real_bytes)
        assert (material.itemsize, light.itemsize, inst.itemsize) == (info.material_bytes, info.light_bytes, info.inst_shade_bytes), "layout of the shading hook changed"
        real = np.float32 if info.real_bytes == 4 else np.float64
        counts = {"materials": (info.n_materials, material), "lights": (info.n_lights, light), "light_pmf": (info.n_pmf, real), "light_cdf": (info.n_cdf, real),
                  "inst_shade": (info.n_instances, inst)}
        out = {k: np.zeros(max(n, 1), t) for k, (n, t) in counts.items()}
        _check(lib().take_hip_debug_shading_tables(self.h, int(side), *(out[k].ctypes.data for k in ("materials", "lights", "light_pmf", "light_cdf", "inst_shade"))))
        out = {k: out[k][:n] for k, (n, _) in counts.items()}
        out.update(tag_mask=int(info.tag_mask), n_material_tags=int(info.n_material_tags), single_tag=int(info.single_tag), real_bytes=int(info.real_bytes))
        return out

    def debug_tree(self, side=None):
        """the resident tree of one side, read back from device memory as the trace kernels read it (take_hip_debug_tree,
        a test hook): a dict of the info's values (node_format, node_width, two_level, root_child, real_bytes, n_nodes,
        n_prims, n_instances, grid_lo, grid_step) and the numpy structured arrays "nodes", "prims", "inst_trace"
        (cdefs.debug_tree_dtypes).  side: TAKE_PRECISION_F32 / _F64 (default: the scene's own, F64 for MIXED)"""
        if side is None:
            side = D.TAKE_PRECISION_F32 if self.precision == D.TAKE_PRECISION_F32 else D.TAKE_PRECISION_F64
        info = D.TakeDebugTreeInfo()
        _check(lib().take_hip_debug_tree_info(self.h, int(side), C.byref(info)))
        node_t, prim_t, inst_t = D.debug_tree_dtypes(info)
        # (one spare element: a buffer is never NULL, an empty array is still an argument)
        nodes, prims, inst = np.zeros(info.n_nodes + 1, node_t), np.zeros(info.n_prims + 1, prim_t), np.zeros(info.n_instances + 1, inst_t)
        _check(lib().take_hip_debug_tree(self.h, int(side), nodes.ctypes.data, prims.ctypes.data, inst.ctypes.data))
        return D.debug_tree_result(info, nodes[:-1], prims[:-1], inst[:-1])

    def build_info(self):
        """who built the trees: {"f32": builder, "f64": builder}, each TAKE_BUILDER_DEVICE_LBVH, TAKE_BUILDER_HOST_SAH
        (asked for, or the fall-back of a device build) or -1 for a side a scene of this precision does not have"""
        f, d = C.c_int32(), C.c_int32()
        _check(lib().take_hip_scene_build_info(self.h, C.byref(f), C.byref(d)))
        return {"f32": f.value, "f64": d.value}


class SceneGroup:
    """The scene replicated on several GPUs of ONE process (take_hip_group_*): what the reference's single-process
    C++ host uses in place of its thread pool.  `devices`: HIP device per shard; a device may repeat (logical shards)."""

    def __init__(self, scene_data, devices, precision=D.TAKE_PRECISION_F32, bvh_threads=0, max_leaf_size=0,
                 builder=D.TAKE_BUILDER_AUTO, burley_lobes=False, flatten_instances=False):
        self.sd = scene_data
        self.precision = precision
        self.dtype = np.float32 if precision == D.TAKE_PRECISION_F32 else np.float64
        desc, keep = scene_data.to_desc()
        opts = D.TakeBuildOpts(precision, bvh_threads, max_leaf_size, builder, 1 if burley_lobes else 0,
                               D.TAKE_INSTANCES_FLATTEN if flatten_instances else D.TAKE_INSTANCES_TWO_LEVEL)
        devs = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        _check(lib().take_hip_group_create(C.byref(desc), C.byref(opts), len(devices), devs, C.byref(h)))
        self.h = h
        del keep

    def close(self):
        if getattr(self, "h", None):
            lib().take_hip_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return _check(lib().take_hip_group_size(self.h))

    def render(self, spp=None, max_depth=None, seed=0, samples_per_batch=0, integrator=0):
        """-> (H, W, 3) host image assembled on the group's first device"""
        o = D.TakeRenderOpts()
        o.spp = int(self.sd.spp if spp is None else spp)
        o.max_depth = int(self.sd.max_depth if max_depth is None else max_depth)
        o.seed, o.samples_per_batch, o.integrator = int(seed), int(samples_per_batch), int(integrator)
        out = np.zeros((self.sd.height, self.sd.width, 3), self.dtype)
        _check(lib().take_hip_group_render(self.h, C.byref(o), out.ctypes.data))
        return out

    def counters(self, k):
        c = D.TakeCounters()
        _check(lib().take_hip_group_get_counters(self.h, int(k), C.byref(c)))
        return c.as_dict()

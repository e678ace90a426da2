"""ctypes binding of libtake_hip.so (include/take_hip.h).

The library is the product; this package only marshals.  This module holds the resident scene and the scene group, and
hands on everything else the binding has: loading and errors (_lib), the image-space calls (image), meshes, rigs,
subdivision and displacement (meshes).  What the wrappers share — arrays to pointers, streams, handle lifetime — is in _marshal.
"""
import ctypes as C

import numpy as np

from . import _marshal as M
from . import cdefs as D
from ._lib import EXPORTS, LIB_PATH, TakeError, _check, build, device_count, lib  # noqa: F401
from .image import (STATS_PLANES, TEMPORAL_PLANES, ImageWorkspace, _adaptive_opts, _bloom_opts, _device_stats, _host_stats, _keyword_opts,  # noqa: F401
                    auto_exposure, bloom_layer, bloom_layer_device, denoise, denoise_device, denoise_variance, denoise_variance_device,
                    luminance_histogram, luminance_histogram_device, temporal_accumulate, temporal_accumulate_device, tonemap, tonemap_bloom,
                    tonemap_bloom_device, tonemap_device)
from .meshes import (DeviceMesh, Displace, Rig, Subdiv, _shutter, compute_normals, ply_layout, shutter_plan, shutter_vertices, subdiv_counts,  # noqa: F401
                     subdiv_topology)

DEBUG_TABLES = {"material": (0, 27, 14), "light": (1, 30, 9), "texture": (2, 6, 3), "to_world": (3, 6, 3),
                "hemicos": (4, 1, 4), "burley": (5, 30, 14)}


def debug_table(name, inp, rnd, precision=D.TAKE_PRECISION_F64):
    """Device shading functions on golden-table rows (test hook).  rnd: (n, 8) random_real draws per row."""
    kind, cin, cout = DEBUG_TABLES[name]
    inp = np.ascontiguousarray(inp, np.float64).reshape(-1, cin)
    rnd = np.ascontiguousarray(rnd, np.float64).reshape(-1, 8)
    n = inp.shape[0]
    out = np.zeros((n, cout), np.float64)
    _check(lib().take_hip_debug_table(kind, precision, inp.ctypes.data, n, cin, rnd.ctypes.data, out.ctypes.data, cout))
    return out


def _build_opts(precision, bvh_threads, max_leaf_size, builder, burley_lobes, flatten_instances):
    return D.TakeBuildOpts(precision, bvh_threads, max_leaf_size, builder, 1 if burley_lobes else 0,
                           D.TAKE_INSTANCES_FLATTEN if flatten_instances else D.TAKE_INSTANCES_TWO_LEVEL)


def _host_planes(known, what, want, shape, real):
    """zeroed host planes for the names in `want` -> ({name: array}, {name: its address}); known: cdefs.FEATURE_PLANES /
    MOTION_PLANES, shape: (rows, W), real: the scene's Real"""
    out = {}
    for name in want:
        if name not in known:
            raise ValueError(f"unknown {what} plane {name!r}: one of {tuple(known)}")
        per_pixel, is_real = known[name]
        out[name] = np.zeros(shape + ((per_pixel,) if per_pixel > 1 else ()), real if is_real else np.int32)
    return out, {name: a.ctypes.data for name, a in out.items()}


def _device_planes(known, what, ptrs):
    """{name: torch device tensor or integer device pointer} -> {name: its address}"""
    for name in ptrs:
        if name not in known:
            raise ValueError(f"unknown {what} plane {name!r}: one of {tuple(known)}")
    return {name: M.pointer(p) for name, p in ptrs.items()}


def _rig_pose(rec, rig, joint_xforms, target_weights, keep):
    """the rig and pose of one TakeRigBinding / TakeSubdivBinding -> whether the pose is in device memory"""
    rec.rig = M.handle_of(rig, Rig, "a binding's rig")
    rec.pose, device = rig._pose(joint_xforms, target_weights, keep)
    return device


def _pose_binding(rec, binding, keep):
    mesh, rig, joint_xforms, target_weights = binding
    rec.mesh = int(mesh)
    return _rig_pose(rec, rig, joint_xforms, target_weights, keep)


def _subdiv_binding(rec, binding, keep):
    mesh, subdiv, cage = binding
    rec.mesh, rec.subdiv = int(mesh), M.handle_of(subdiv, Subdiv, "a binding's subdiv")
    if isinstance(cage, tuple):
        return _rig_pose(rec, *cage, keep)
    if cage is None:
        return False
    rec.cage_positions, rec.flags, device = subdiv._cage(cage, keep)
    return device


def _displace_binding(rec, binding, keep):
    mesh, displace, base = binding[:3]
    rec.mesh, rec.displace = int(mesh), M.handle_of(displace, Displace, "a binding's displace")
    rec.scale, rec.bias = (float(x) for x in (tuple(binding[3:]) + (1.0, 0.0)[len(binding) - 3:]))
    if isinstance(base, tuple) and len(base) == 2 and isinstance(base[0], Subdiv):
        subdiv, cage = base
        rec.subdiv = M.handle_of(subdiv, Subdiv, "a binding's subdiv")
        if isinstance(cage, tuple):
            return _rig_pose(rec, *cage, keep)
        if cage is None:
            return False
        rec.cage_positions, rec.flags, device = subdiv._cage(cage, keep)
        return device
    if base is None:
        return False
    positions, normals = base if isinstance(base, tuple) else (base, None)
    rec.positions, rec.normals, rec.flags, device = displace._base(positions, normals, keep)
    return device


class Scene(M.Handle):
    """A scene resident on the current HIP device: flattened `Scene` + wide BVH in HBM."""
    _destroy = "take_hip_scene_destroy"
    h = property(lambda self: self._h)

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
        opts = _build_opts(precision, bvh_threads, max_leaf_size, builder, burley_lobes, flatten_instances)
        _check(lib().take_hip_scene_create(C.byref(desc), C.byref(opts), self._new()))
        del keep

    def _opts(self, spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator=0):
        spp = self.sd.spp if spp is None else spp  # (None: the scene description's)
        max_depth = self.sd.max_depth if max_depth is None else max_depth
        o = D.TakeRenderOpts()
        o.exact_bounces = int(getattr(self, "exact_bounces", 0))  # TAKE_PRECISION_MIXED scenes (0 = the library's default)
        o.spp, o.max_depth, o.seed, o.ray_epsilon = int(spp), int(max_depth), int(seed), float(ray_epsilon)
        o.strip_first, o.strip_stride, o.samples_per_batch = int(strip_first), int(strip_stride), int(samples_per_batch)
        o.integrator = int(integrator)
        return o

    def _strip_rows(self, strip_first, strip_stride):
        return _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, None))

    def _strip_image(self, strip_first, strip_stride):
        """the zeroed (rows, W, 3) host image of a strip set"""
        return np.zeros((self._strip_rows(strip_first, strip_stride), self.sd.width, 3), self.dtype)

    def _side(self, side):
        """a debug hook's side: TAKE_PRECISION_F32 / _F64 (None: the scene's own, F64 for MIXED)"""
        if side is None:
            side = D.TAKE_PRECISION_F32 if self.precision == D.TAKE_PRECISION_F32 else D.TAKE_PRECISION_F64
        return int(side)

    def rows(self, strip_first=0, strip_stride=1):
        n = self._strip_rows(strip_first, strip_stride)
        out = (C.c_int32 * max(n, 1))()
        _check(lib().take_hip_render_rows(self.h, strip_first, strip_stride, out))
        return np.array(out[:n], np.int32)

    def render(self, spp=None, max_depth=None, seed=0, ray_epsilon=0.0, strip_first=0, strip_stride=1,
               samples_per_batch=0, integrator=0):
        """-> (rows, W, 3) image rows owned by this strip set, top row first (host array)."""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        out = self._strip_image(strip_first, strip_stride)
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
        out, at = _host_planes(D.FEATURE_PLANES, "feature", want, (self._strip_rows(strip_first, strip_stride), self.sd.width), self.dtype)
        bufs = D.TakeFeatureBuffers(**at)
        _check(lib().take_hip_render_features(self.h, C.byref(o), C.byref(bufs)))
        return out

    def render_features_device(self, ptrs, spp, seed=0, ray_epsilon=0.0, strip_first=0, strip_stride=1, samples_per_batch=0,
                               stream=None):
        """the same into device memory (take_hip_render_features_device); ptrs: {name: torch device tensor or integer
        device pointer} for the planes wanted — contiguous, of the scene's Real (int32 for the ids), sized for the rows
        of the strip set; blocks until done"""
        o = self._opts(spp, 0, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch)
        bufs = D.TakeFeatureBuffers(**_device_planes(D.FEATURE_PLANES, "feature", ptrs))
        _check(lib().take_hip_render_features_device(self.h, C.byref(o), C.byref(bufs), C.c_void_p(stream or 0)))

    def render_denoised(self, spp=None, max_depth=None, seed=0, ray_epsilon=0.0, samples_per_batch=0, integrator=0, opts=None, **kw):
        """render the whole image, make albedo, normal and depth with the same options and filter, all on the device
        (take_hip_render_denoised) -> (H, W, 3) host array.  Equal bit for bit to render + render_features + denoise made
        by hand.  Denoise options: keywords of cdefs.denoise_opts, or opts = a TakeDenoiseOpts; neither = the defaults."""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        out = np.zeros((self.sd.height, self.sd.width, 3), self.dtype)
        _check(lib().take_hip_render_denoised(self.h, C.byref(o), M.ref(opts), out.ctypes.data))
        return out

    def render_denoised_device(self, d_ptr, spp, max_depth, seed=0, ray_epsilon=0.0, samples_per_batch=0, stream=None, integrator=0,
                               opts=None, **kw):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer; H * W * 3 of the
        scene's Real); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        _check(lib().take_hip_render_denoised_device(self.h, C.byref(o), M.ref(opts), C.c_void_p(M.pointer(d_ptr)), C.c_void_p(stream or 0)))

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
        out = self._strip_image(strip_first, strip_stride)
        planes, st = _host_stats(out.shape[:2]) if stats else (None, None)
        _check(lib().take_hip_render_adaptive(self.h, C.byref(o), M.ref(a), out.ctypes.data, M.ref(st)))
        return (out, planes) if stats else out

    def render_adaptive_device(self, d_ptr, spp, max_depth, seed=0, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0, stats=None, opts="keywords",
                               ray_epsilon=0.0, strip_first=0, strip_stride=1, samples_per_batch=0, stream=None, integrator=0):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer; rows * W * 3 of the
        scene's Real); stats: {"count" / "m1" / "m2": device tensor or pointer} for the planes wanted (int32, float64,
        float64; rows * W each); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        a = _adaptive_opts(opts, min_spp, step_spp, threshold, floor)
        st = _device_stats(stats)
        _check(lib().take_hip_render_adaptive_device(self.h, C.byref(o), M.ref(a), C.c_void_p(M.pointer(d_ptr)), M.ref(st), C.c_void_p(stream or 0)))

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
        _check(lib().take_hip_render_adaptive_denoised(self.h, C.byref(o), M.ref(a), M.ref(opts), out.ctypes.data, M.ref(st), None if var is None else var.ctypes.data))
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
        _check(lib().take_hip_render_adaptive_denoised_device(self.h, C.byref(o), M.ref(a), M.ref(opts), C.c_void_p(M.pointer(d_ptr)), M.ref(st),
                                                              C.c_void_p(M.pointer(variance)), C.c_void_p(stream or 0)))

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
        out, at = _host_planes(D.MOTION_PLANES, "motion", want, (self.sd.height, self.sd.width), self.dtype)
        bufs = D.TakeMotionBuffers(**at)
        _check(lib().take_hip_render_motion(self.h, C.byref(o), C.byref(bufs)))
        return out

    def render_motion_device(self, ptrs, ray_epsilon=0.0, stream=None):
        """the same into device memory (take_hip_render_motion_device); ptrs: {name: torch device tensor or integer device
        pointer} for the planes wanted — contiguous, of the scene's Real (int32 for shape_id); blocks until done"""
        o = self._opts(1, 0, 0, ray_epsilon, 0, 1, 0)
        bufs = D.TakeMotionBuffers(**_device_planes(D.MOTION_PLANES, "motion", ptrs))
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
        _check(lib().take_hip_render_temporal(self.h, C.byref(o), M.ref(a), M.ref(temporal), M.ref(opts), 1 if restart else 0, out.ctypes.data))
        return out

    def render_temporal_device(self, d_ptr, spp, max_depth, seed=0, restart=False, min_spp=0, step_spp=0, threshold=-1.0, floor=0.0, adaptive="keywords",
                               temporal=None, ray_epsilon=0.0, samples_per_batch=0, stream=None, integrator=0, opts=None, **kw):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer; H * W * 3 of the
        scene's Real); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, 0, 1, samples_per_batch, integrator)
        a = _adaptive_opts(adaptive, min_spp, step_spp, threshold, floor)
        opts = _keyword_opts(D.denoise_opts, opts, kw)
        _check(lib().take_hip_render_temporal_device(self.h, C.byref(o), M.ref(a), M.ref(temporal), M.ref(opts), 1 if restart else 0, C.c_void_p(M.pointer(d_ptr)),
                                                     C.c_void_p(stream or 0)))

    def set_instance_transforms(self, xforms, stream=None):
        """new object -> world transforms for ALL placements of a two-level scene, (n, 3, 4) float64 in the order of the
        description's instances; only the top level is rebuilt, on the device (take_hip_scene_set_instance_transforms).
        A numpy array (or anything numpy converts) goes through the host entry point; a torch device tensor or an
        integer device pointer — then `n` is the scene's placement count — through the device one."""
        if isinstance(xforms, int):
            n, ptr, device = len(self.sd.instance_mesh), xforms, True
        else:
            device, keep = M.on_device(xforms), []
            ptr = M.array(M.required(xforms, "transforms"), np.float64, None, "transforms", device, keep)
            n, rest = divmod(keep[0].numel() if device else keep[0].size, 12)
            if rest:
                raise ValueError("transforms must have shape (n, 3, 4)")
        if device:
            _check(lib().take_hip_scene_set_instance_transforms_device(self.h, C.c_void_p(ptr), n, C.c_void_p(stream or 0)))
        else:
            _check(lib().take_hip_scene_set_instance_transforms(self.h, ptr, n))

    def set_envmap(self, image, scale=None, stream=None):
        """a new environment map for the resident scene (take_hip_scene_set_envmap): `image` is (h, w, 3), row 0 = zenith —
        a numpy float32 or float64 array (anything else numpy converts is taken as float64) read from host memory, or a
        contiguous float32 / float64 torch tensor on the device, read through its device pointer after `stream` (default:
        torch's current stream).  scale: the light's new (r, g, b) intensity, None = keep.  The tables are built on the
        device; afterwards the scene equals one newly created from its description with this image and scale."""
        sc = None if scale is None else D.c_double3(*map(float, scale))
        device, keep = M.on_device(image), []
        ptr = M.array(M.required(image, "an environment map"), (np.float64, np.float32), (-1, -1, 3), "an environment map", device, keep)
        h, w = keep[0].shape[:2]
        real = D.TAKE_PRECISION_F32 if str(keep[0].dtype).endswith("float32") else D.TAKE_PRECISION_F64
        im = D.TakeEnvImage(int(w), int(h), ptr, real, D.TAKE_MESH_DEVICE_ARRAYS if device else 0)
        if device:
            _check(lib().take_hip_scene_set_envmap_device(self.h, C.byref(im), sc, C.c_void_p(M.stream_of(stream, image) or 0)))
        else:
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
        device, keep = M.on_device(rgb), []
        ptr = M.array(M.required(rgb, "intensities"), np.float64, (-1, 3), "intensities", device, keep)
        count = int(keep[0].shape[0])
        if device:
            _check(lib().take_hip_scene_set_light_intensities_device(self.h, C.c_void_p(ptr), int(first), count, C.c_void_p(M.stream_of(stream, rgb) or 0)))
        else:
            _check(lib().take_hip_scene_set_light_intensities(self.h, keep[0].ctypes.data_as(C.POINTER(C.c_double)), int(first), count))

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
        sh = _shutter(open, close, slices)
        out = self._strip_image(strip_first, strip_stride)
        _check(lib().take_hip_render_shutter(self.h, C.byref(o), C.byref(sh), out.ctypes.data))
        return out

    def render_shutter_device(self, d_ptr, spp, max_depth, seed=0, open=0.0, close=1.0, slices=0, ray_epsilon=0.0, strip_first=0,
                              strip_stride=1, samples_per_batch=0, stream=None, integrator=0):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer); blocks until done"""
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        sh = _shutter(open, close, slices)
        _check(lib().take_hip_render_shutter_device(self.h, C.byref(o), C.byref(sh), C.c_void_p(M.pointer(d_ptr)), C.c_void_p(stream or 0)))

    def _motions(self, motions, stream):
        """[(mesh_id, positions0, positions1[, normals0, normals1]), ...] -> (TakeMeshMotion array, n, what keeps the
        arrays alive); device tensors are waited for on `stream` (default: torch's current stream)"""
        motions = list(motions)
        recs = (D.TakeMeshMotion * max(len(motions), 1))()
        keep, wait = [], None
        for rec, m in zip(recs, motions):
            if len(m) not in (3, 5):
                raise ValueError("a motion is (mesh_id, positions0, positions1) or (mesh_id, positions0, positions1, normals0, normals1)")
            arrays = list(m[1:]) + [None] * (5 - len(m))
            device = M.on_device(arrays[0])
            rec.mesh, rec.flags = int(m[0]), D.TAKE_MESH_DEVICE_ARRAYS if device else 0
            rec.positions0, rec.positions1, rec.normals0, rec.normals1 = [M.array(a, np.float64, None, f"mesh {m[0]}", device, keep) for a in arrays]
            if device and wait is None:
                wait = arrays[0].device
        M.wait_for(stream, wait)
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
        sh = _shutter(open, close, slices)
        out = self._strip_image(strip_first, strip_stride)
        _check(lib().take_hip_render_shutter_meshes(self.h, C.byref(o), C.byref(sh), recs, n, out.ctypes.data))
        del keep
        return out

    def render_shutter_meshes_device(self, d_ptr, motions, spp, max_depth, seed=0, open=0.0, close=1.0, slices=0, ray_epsilon=0.0, strip_first=0,
                                     strip_stride=1, samples_per_batch=0, stream=None, integrator=0):
        """the same into device memory at `d_ptr` (a torch device tensor or an integer device pointer); blocks until done"""
        recs, n, keep = self._motions(motions, stream)
        o = self._opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator)
        sh = _shutter(open, close, slices)
        _check(lib().take_hip_render_shutter_meshes_device(self.h, C.byref(o), C.byref(sh), recs, n, C.c_void_p(M.pointer(d_ptr)), C.c_void_p(stream or 0)))
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

    def _bind(self, entry, record, fill, bindings, stream):
        """what pose_meshes, subdivide_meshes and displace_meshes share: one `record` per binding, filled by fill(record, binding, keep)
        -> whether the binding reads device tensors; those are waited for on `stream`, then the call is made"""
        bindings = list(bindings)
        recs = (record * max(len(bindings), 1))()
        keep, wait = [], None
        for rec, binding in zip(recs, bindings):
            if fill(rec, binding, keep) and wait is None:
                wait = keep[-1].device
        M.wait_for(stream, wait)
        _check(getattr(lib(), entry)(self.h, recs, len(bindings)))
        del keep

    def pose_meshes(self, bindings, stream=None):
        """skin / morph meshes of the resident scene and update it in one step (take_hip_scene_pose_meshes): `bindings` is
        [(mesh_id, rig, joint_xforms, target_weights), ...] — a Rig of the mesh's vertex count and a pose as Rig.pose
        takes it (None for what the rig has none of).  Every rig is posed into its own device buffers and the scene takes
        update_meshes' path over them: afterwards it equals the scene after update_meshes({mesh_id: rig.pose(...)}).
        Pose arrays may be device tensors written on `stream` (default: torch's current stream), which the call waits
        for first."""
        self._bind("take_hip_scene_pose_meshes", D.TakeRigBinding, _pose_binding, bindings, stream)

    def subdivide_meshes(self, bindings, stream=None):
        """refine cages by Loop subdivision and update the resident scene in one step (take_hip_scene_subdivide_meshes):
        `bindings` is [(mesh_id, subdiv, cage), ...] — a Subdiv whose refined vertex count is the mesh's, and cage
        positions (cage_vertices, 3) as a numpy array or a torch device tensor — or [(mesh_id, subdiv, (rig,
        joint_xforms, target_weights)), ...]: the cage is then the rig's pose.  Afterwards the scene equals the one
        after update_meshes({mesh_id: subdiv.refine(cage)}); normals go to meshes that have vertex normals.  Device
        tensors may have been written on `stream` (default: torch's current stream), which the call waits for first."""
        self._bind("take_hip_scene_subdivide_meshes", D.TakeSubdivBinding, _subdiv_binding, bindings, stream)

    def displace_meshes(self, bindings, stream=None):
        """displace surfaces by height maps and update the resident scene in one step (take_hip_scene_displace_meshes):
        `bindings` is [(mesh_id, displace, base, scale, bias), ...] (scale 1, bias 0 when left out) — a Displace of the
        mesh's vertex count, and the base surface: positions (n_vertices, 3), or (positions, normals) — numpy arrays or
        torch device tensors; normals None: the handle's own —, or (subdiv, cage) with cage as subdivide_meshes takes it
        (positions, or (rig, joint_xforms, target_weights)): the cage is refined first and moved along the refined
        normals.  Afterwards the scene equals the one after update_meshes({mesh_id: displace.apply(...)}); normals go to
        meshes that have vertex normals.  Device tensors may have been written on `stream` (default: torch's current
        stream), which the call waits for first."""
        self._bind("take_hip_scene_displace_meshes", D.TakeDisplaceBinding, _displace_binding, bindings, stream)

    def set_mesh_vertices(self, updates, _entry="take_hip_scene_set_mesh_vertices"):
        """new vertices for meshes of a scene without placements (take_hip_scene_set_mesh_vertices): `updates` is
        {mesh_id: positions} or {mesh_id: (positions, normals)} (a tuple), every array (n_vertices, 3) float64 and complete, normals
        None = keep.  numpy arrays (or anything numpy converts) are read from host memory; torch device tensors —
        contiguous float64, all arrays of one mesh on the device — through their device pointers.  The tree is rebuilt
        on the device; afterwards the scene equals one newly created from the description with these arrays."""
        recs = (D.TakeMeshUpdate * max(len(updates), 1))()
        keep = []
        for rec, (mesh, arrays) in zip(recs, updates.items()):
            pos, nrm = arrays if isinstance(arrays, tuple) and len(arrays) == 2 else (arrays, None)
            device = M.on_device(pos)
            rec.mesh, rec.flags = int(mesh), D.TAKE_MESH_DEVICE_ARRAYS if device else 0
            rec.positions, rec.normals = [M.array(a, np.float64, None, f"mesh {mesh}", device, keep) for a in (pos, nrm)]
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
        b = self._ray_batch(M.pointer(d_rays), n, ray_sets, first_sample, normalize)
        _check(lib().take_hip_render_rays_device(self.h, C.byref(o), C.byref(b), C.c_void_p(M.pointer(d_out)), C.c_void_p(stream or 0)))

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
        _check(lib().take_hip_camera_rays_device(self.h, C.byref(o), int(first_sample), C.c_void_p(M.pointer(d_rays_out)), C.c_void_p(stream or 0)))

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
        inp = np.ascontiguousarray(inp, np.float64).reshape(-1, 3 if kind else 2)
        out = np.zeros((inp.shape[0], 5 if kind else 8), np.float64)
        _check(lib().take_hip_debug_env(self.h, self._side(side), int(kind), inp.ctypes.data, inp.shape[0], out.ctypes.data))
        return out

    def debug_env_tables(self, side=None):
        """the environment map of one resident side, read back from device memory as the shade kernels read it
        (take_hip_debug_env_tables, a test hook) -> {"width", "height", "n_guide_m", "n_guide_c", "texel0", "scale",
        "intensity", "marginal" (h + 1,), "conditional" (h, w + 1), "guide_m" (n_guide_m + 1,), "guide_c" (h, n_guide_c + 1),
        "texels" (h, w, 3), "images" (n_images,) of cdefs.IMAGE_INFO_DTYPE}.  side: as debug_env's"""
        side = self._side(side)
        info = D.TakeDebugEnvTablesInfo()
        _check(lib().take_hip_debug_env_tables_info(self.h, side, C.byref(info)))
        w, h, real = info.width, info.height, np.float32 if info.real_bytes == 4 else np.float64
        out = {"marginal": np.zeros(h + 1, real), "conditional": np.zeros((h, w + 1), real), "guide_m": np.zeros(info.n_guide_m + 1, np.int32),
               "guide_c": np.zeros((h, info.n_guide_c + 1), np.int32), "texels": np.zeros((h, w, 3), real),
               "images": np.zeros(max(info.n_images, 1), D.IMAGE_INFO_DTYPE)}
        _check(lib().take_hip_debug_env_tables(self.h, side, *(out[k].ctypes.data for k in ("marginal", "conditional", "guide_m", "guide_c", "texels", "images"))))
        out["images"] = out["images"][:info.n_images]
        out.update(width=w, height=h, n_guide_m=info.n_guide_m, n_guide_c=info.n_guide_c, texel0=info.texel0, scale=np.array(info.scale[:]),
                   intensity=np.array(info.intensity[:]))
        return out

    def debug_shading_tables(self, side=None):
        """the shading tables of one resident side, read back from device memory as the kernels read them
        (take_hip_debug_shading_tables, a test hook) -> {"materials", "lights", "inst_shade": numpy structured arrays
        (cdefs.shading_table_dtypes), "light_pmf", "light_cdf": arrays of the side's Real, "tag_mask", "n_material_tags",
        "single_tag": what the host holds of the tags in use, "real_bytes"}.  side: as debug_env's"""
        side = self._side(side)
        info = D.TakeDebugShadingTablesInfo()
        _check(lib().take_hip_debug_shading_tables_info(self.h, side, C.byref(info)))
        material, light, inst = D.shading_table_dtypes(info.real_bytes)
        assert (material.itemsize, light.itemsize, inst.itemsize) == (info.material_bytes, info.light_bytes, info.inst_shade_bytes), "layout of the shading hook changed"
        real = np.float32 if info.real_bytes == 4 else np.float64
        counts = {"materials": (info.n_materials, material), "lights": (info.n_lights, light), "light_pmf": (info.n_pmf, real), "light_cdf": (info.n_cdf, real),
                  "inst_shade": (info.n_instances, inst)}
        out = {k: np.zeros(max(n, 1), t) for k, (n, t) in counts.items()}
        _check(lib().take_hip_debug_shading_tables(self.h, side, *(out[k].ctypes.data for k in ("materials", "lights", "light_pmf", "light_cdf", "inst_shade"))))
        out = {k: out[k][:n] for k, (n, _) in counts.items()}
        out.update(tag_mask=int(info.tag_mask), n_material_tags=int(info.n_material_tags), single_tag=int(info.single_tag), real_bytes=int(info.real_bytes))
        return out

    def debug_tree(self, side=None):
        """the resident tree of one side, read back from device memory as the trace kernels read it (take_hip_debug_tree,
        a test hook): a dict of the info's values (node_format, node_width, two_level, root_child, real_bytes, n_nodes,
        n_prims, n_instances, grid_lo, grid_step) and the numpy structured arrays "nodes", "prims", "inst_trace"
        (cdefs.debug_tree_dtypes).  side: TAKE_PRECISION_F32 / _F64 (default: the scene's own, F64 for MIXED)"""
        side = self._side(side)
        info = D.TakeDebugTreeInfo()
        _check(lib().take_hip_debug_tree_info(self.h, side, C.byref(info)))
        node_t, prim_t, inst_t = D.debug_tree_dtypes(info)
        # (one spare element: a buffer is never NULL, an empty array is still an argument)
        nodes, prims, inst = np.zeros(info.n_nodes + 1, node_t), np.zeros(info.n_prims + 1, prim_t), np.zeros(info.n_instances + 1, inst_t)
        _check(lib().take_hip_debug_tree(self.h, side, nodes.ctypes.data, prims.ctypes.data, inst.ctypes.data))
        return D.debug_tree_result(info, nodes[:-1], prims[:-1], inst[:-1])

    def build_info(self):
        """who built the trees: {"f32": builder, "f64": builder}, each TAKE_BUILDER_DEVICE_LBVH, TAKE_BUILDER_HOST_SAH
        (asked for, or the fall-back of a device build) or -1 for a side a scene of this precision does not have"""
        f, d = C.c_int32(), C.c_int32()
        _check(lib().take_hip_scene_build_info(self.h, C.byref(f), C.byref(d)))
        return {"f32": f.value, "f64": d.value}


class SceneGroup(M.Handle):
    """The scene replicated on several GPUs of ONE process (take_hip_group_*): what the reference's single-process
    C++ host uses in place of its thread pool.  `devices`: HIP device per shard; a device may repeat (logical shards)."""
    _destroy = "take_hip_group_destroy"
    h = property(lambda self: self._h)

    def __init__(self, scene_data, devices, precision=D.TAKE_PRECISION_F32, bvh_threads=0, max_leaf_size=0,
                 builder=D.TAKE_BUILDER_AUTO, burley_lobes=False, flatten_instances=False):
        self.sd = scene_data
        self.precision = precision
        self.dtype = np.float32 if precision == D.TAKE_PRECISION_F32 else np.float64
        desc, keep = scene_data.to_desc()
        opts = _build_opts(precision, bvh_threads, max_leaf_size, builder, burley_lobes, flatten_instances)
        devs = (C.c_int32 * len(devices))(*devices)
        _check(lib().take_hip_group_create(C.byref(desc), C.byref(opts), len(devices), devs, self._new()))
        del keep

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

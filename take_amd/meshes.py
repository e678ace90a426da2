"""Meshes on the device, apart from any scene (include/take_hip.h): decoding mesh files, vertex normals, rigs (skinning
and morph targets), Loop subdivision, displacement mapping, and the vertex lerp of the shutter."""
import ctypes as C
import os

import numpy as np

from . import cdefs as D
from ._lib import _check, lib
from ._marshal import Closing, Handle, array, on_device, pointer, required, stream_of, wait_for


def _shutter(open, close, slices):
    return D.TakeShutter(float(open), float(close), int(slices), 0)


def shutter_plan(spp, open=0.0, close=1.0, slices=0):
    """how a render over the shutter [open, close] cuts `spp` samples into slices (take_hip_shutter_plan; no scene, no
    GPU) -> (first_sample, time): K + 1 int32 bounds — slice k holds the samples first_sample[k] .. first_sample[k + 1] - 1
    of every pixel — and the K scene times the slices are posed at"""
    sh, k = _shutter(open, close, slices), C.c_int32()
    _check(lib().take_hip_shutter_plan(int(spp), C.byref(sh), C.byref(k), None, None))
    first, time = np.zeros(k.value + 1, np.int32), np.zeros(k.value, np.float64)
    _check(lib().take_hip_shutter_plan(int(spp), C.byref(sh), C.byref(k), first.ctypes.data_as(C.POINTER(C.c_int32)),
                                       time.ctypes.data_as(C.POINTER(C.c_double))))
    return first, time


def shutter_vertices(a, b, t, stream=None):
    """the vertices of a deforming mesh at scene time t in [0, 1] (take_hip_shutter_vertices): `a` the array at the marked
    frame, `b` at the current one — positions or normals, any shape, float64 — lerped entry by entry on the device as
    render_shutter_meshes lerps them -> (out, moved): the array at t, and 1 where any entry of it is not b's bit for bit.
    numpy arrays give a numpy array; contiguous float64 torch device tensors are read through their device pointers after
    `stream` (default: torch's current stream) and give a new device tensor."""
    moved, keep = C.c_int32(-1), []
    device = on_device(a) or on_device(b)
    pa, pb = array(required(a, "a"), np.float64, None, "a", device, keep), array(required(b, "b"), np.float64, None, "b", device, keep)
    if keep[0].shape != keep[1].shape or (device and a.device != b.device):
        raise ValueError("a and b must have one shape" + (", both on one device" if device else ""))
    if device:
        import torch

        out = torch.empty_like(a)
        with torch.cuda.device(a.device):
            _check(lib().take_hip_shutter_vertices_device(C.c_void_p(pa), C.c_void_p(pb), a.numel(), float(t), C.c_void_p(out.data_ptr()), C.byref(moved),
                                                          C.c_void_p(stream_of(stream, a) or 0)))
        return out, moved.value
    out = np.zeros_like(keep[0])
    _check(lib().take_hip_shutter_vertices(pa, pb, keep[0].size, float(t), out.ctypes.data, C.byref(moved)))
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


class DeviceMesh(Closing):
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
    # format -> (the entry point that decodes bytes, the one that reads a file, whether they take shape_index)
    _DECODERS = {"ply": ("take_hip_mesh_from_ply", "take_hip_mesh_from_ply_file", False),
                 "obj": ("take_hip_mesh_from_obj", "take_hip_mesh_from_obj_file", False),
                 "serialized": ("take_hip_mesh_from_serialized", "take_hip_mesh_from_serialized_file", True)}

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
        in_memory = isinstance(source, (bytes, bytearray, memoryview))
        fmt = format
        if in_memory:
            buf = bytes(source)
            fmt, what = fmt or ("ply" if buf[:3] == b"ply" else "serialized"), (buf, len(buf))
        else:
            if fmt is None and os.fsdecode(source).lower().endswith(".obj"):
                fmt = "obj"
            if fmt is None:
                with open(source, "rb") as f:
                    fmt = "ply" if f.read(3) == b"ply" else "serialized"
            what = (os.fsencode(source),)
        from_bytes, from_file, indexed = self._DECODERS[fmt]
        if indexed:
            what += (int(shape_index),)
        decode = getattr(lib(), from_bytes if in_memory else from_file)
        _check(decode(*what, None if xw is None else xw.ctypes.data, None if xi is None else xi.ctypes.data, int(material_id), C.byref(self.c)))
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


class Rig(Handle):
    """A mesh's rest pose, joint influences and morph targets in device memory (take_hip_rig_create): what pose(),
    pose_device() and Scene.pose_meshes() skin and morph on the device — linear-blend skinning over a joint palette,
    normals by the cofactor matrix (include/take_hip.h has the arithmetic).  positions (n, 3) and the optional normals
    (n, 3) are the rest pose; joints (n, K) int32 and weights (n, K), K = 1..8, name each vertex's influences (weights are
    taken as they are, padding is a zero weight on any valid joint); inverse_bind (n_joints, 3, 4), None = identity —
    it fixes the joint count, which without it is max(joints) + 1 or `n_joints`; target_positions / target_normals
    (T, n, 3) are morph deltas.  Either numpy arrays (or anything numpy converts), or contiguous float64 / int32 torch
    tensors on the device — all of them then.  Bound to the device current at its creation; not thread-safe."""
    _destroy = "take_hip_rig_destroy"

    def __init__(self, positions, normals=None, joints=None, weights=None, inverse_bind=None, target_positions=None, target_normals=None, n_joints=None):
        self._new()
        device = on_device(positions)
        keep = []
        d = D.TakeRigDesc()
        d.positions = array(required(positions, "positions"), np.float64, (-1, 3), "positions", device, keep)
        nv = int(keep[0].shape[0])
        d.n_vertices, d.flags = nv, D.TAKE_RIG_DEVICE_ARRAYS if device else 0
        d.normals = array(normals, np.float64, (nv, 3), "normals", device, keep)
        if (joints is None) != (weights is None):
            raise ValueError("joints and weights go together")
        if joints is not None:
            d.joints = array(joints, np.int32, (nv, -1), "joints", device, keep)
            ja = keep[-1]
            k = int(ja.shape[1])
            d.weights = array(weights, np.float64, (nv, k), "weights", device, keep)
            d.inverse_bind = array(inverse_bind, np.float64, (-1, 3, 4), "inverse_bind", device, keep)
            if inverse_bind is not None:
                nj = int(keep[-1].shape[0])
            elif n_joints is not None:
                nj = int(n_joints)
            else:
                nj = int(ja.max()) + 1 if nv * k else 0
            d.n_joints, d.n_influences = nj, k
        if target_positions is not None:
            d.target_positions = array(target_positions, np.float64, (-1, nv, 3), "target_positions", device, keep)
            d.n_targets = int(keep[-1].shape[0])
            d.target_normals = array(target_normals, np.float64, (d.n_targets, nv, 3), "target_normals", device, keep)
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
        device = on_device(joint_xforms) or on_device(target_weights)
        p = D.TakeRigPose()
        p.joint_xforms = array(joint_xforms, np.float64, (self.n_joints, 3, 4), "joint_xforms", device, keep)
        p.target_weights = array(target_weights, np.float64, (self.n_targets,), "target_weights", device, keep)
        p.flags = D.TAKE_RIG_POSE_DEVICE_ARRAYS if device else 0
        return p, device

    def pose(self, joint_xforms=None, target_weights=None):
        """the rig under a pose (take_hip_rig_pose): joint_xforms (n_joints, 3, 4) joint -> world, target_weights (T,)
        -> the posed positions (n, 3), or (positions, normals) when the rig has normals; numpy arrays"""
        keep = []
        p, device = self._pose(joint_xforms, target_weights, keep)
        wait_for(None, keep[0].device if device else None)
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
        if device:
            stream = stream_of(stream, keep[0])
        _check(lib().take_hip_rig_pose_device(self._h, C.byref(p), C.c_void_p(pointer(out_positions)), C.c_void_p(pointer(out_normals)), C.c_void_p(stream or 0)))


def _subdiv_desc(indices, n_vertices, levels, uvs, keep):
    d = D.TakeSubdivDesc()
    d.indices = array(required(indices, "indices"), np.int32, (-1, 3), "indices", False, keep)
    d.n_vertices, d.n_faces, d.levels, d.flags = int(n_vertices), keep[0].shape[0], int(levels), 0
    d.uvs = array(uvs, np.float64, (int(n_vertices), 2), "uvs", False, keep)
    return d


def _subdiv_sizes(d):
    nv, nf = C.c_int64(), C.c_int64()
    _check(lib().take_hip_subdiv_counts(C.byref(d), C.byref(nv), C.byref(nf)))
    return nv.value, nf.value


def _subdiv_topology(d, n_vertices, n_faces, has_uvs):
    idx = np.zeros((n_faces, 3), np.int32)
    uv = np.zeros((n_vertices, 2), np.float64) if has_uvs else None
    _check(lib().take_hip_subdiv_topology(C.byref(d), idx.ctypes.data, None if uv is None else uv.ctypes.data))
    return idx, uv


def subdiv_counts(indices, n_vertices, levels):
    """(refined vertices, refined faces) of a cage under `levels` levels of Loop subdivision (take_hip_subdiv_counts);
    needs no GPU"""
    keep = []
    return _subdiv_sizes(_subdiv_desc(indices, n_vertices, levels, None, keep))


def subdiv_topology(indices, n_vertices, levels, uvs=None):
    """the refined faces (n, 3) int32 and — for a cage with uvs — the refined uvs (n, 2), else None
    (take_hip_subdiv_topology); needs no GPU"""
    keep = []
    d = _subdiv_desc(indices, n_vertices, levels, uvs, keep)
    return _subdiv_topology(d, *_subdiv_sizes(d), uvs is not None)


class Subdiv(Handle):
    """Loop subdivision of one triangle cage on the device (take_hip_subdiv_create; include/take_hip.h has the scheme):
    made once from the cage's topology — indices (n_faces, 3), the vertex count, optional uvs (n_vertices, 2), 1..6
    levels —, it keeps the stencil tables in device memory; refine(), refine_device() and Scene.subdivide_meshes() turn
    cage positions into refined positions and vertex normals there.  Bound to the device current at its creation; not
    thread-safe."""
    _destroy = "take_hip_subdiv_destroy"

    def __init__(self, indices, n_vertices, levels, uvs=None):
        self._new()
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
        return _subdiv_topology(self._desc, self.n_vertices, self.n_faces, self._has_uvs)

    def _cage(self, cage, keep):
        """-> (pointer, flags, on the device?) of cage positions: a numpy array, or a torch device tensor"""
        device = on_device(cage)
        ptr = array(required(cage, "cage positions"), np.float64, (self.cage_vertices, 3), "cage", device, keep)
        return ptr, (D.TAKE_SUBDIV_DEVICE_ARRAYS if device else 0), device

    def refine_device(self, out_positions, out_normals=None, cage=None, stream=None):
        """the cage refined into device memory (take_hip_subdiv_refine_device): out_positions, out_normals are
        (n_vertices, 3) float64 torch device tensors or integer device pointers (out_normals None: no normals); runs on
        `stream` (default: torch's current stream when the cage is a device tensor, else the default stream) and blocks
        until done"""
        keep = []
        ptr, flags, device = self._cage(cage, keep)
        if device:
            stream = stream_of(stream, cage)
        _check(lib().take_hip_subdiv_refine_device(self._h, C.c_void_p(ptr), flags, C.c_void_p(pointer(out_positions)), C.c_void_p(pointer(out_normals)),
                                                   C.c_void_p(stream or 0)))

    def refine(self, cage, normals=True):
        """-> (positions, normals), or positions alone with normals=False: (n_vertices, 3) numpy arrays.  A numpy cage
        takes take_hip_subdiv_refine; a torch device tensor is refined on torch's current stream and downloaded"""
        if on_device(cage):
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


class Displace(Handle):
    """Displacement mapping of one triangle mesh on the device (take_hip_displace_create; include/take_hip.h has the
    arithmetic): made once from the mesh's topology — indices (n_faces, 3), the vertex count, uvs (n_vertices, 2) — and a
    height image (height, width), float32 or float64, a numpy array or a torch device tensor, with the lookup uvxf =
    (uscale, vscale, uoffset, voffset) of a texture; apply(), apply_device() and Scene.displace_meshes() move base
    positions along unit normals by scale * height + bias and compute the normals of the result.  Bound to the device
    current at its creation; not thread-safe."""
    _destroy = "take_hip_displace_destroy"

    def __init__(self, indices, n_vertices, uvs, image, uvxf=(1.0, 1.0, 0.0, 0.0), stream=None):
        self._new()
        keep = []
        d = D.TakeDisplaceDesc()
        d.indices = array(required(indices, "indices"), np.int32, (-1, 3), "indices", False, keep)
        d.n_vertices, d.n_faces = int(n_vertices), keep[0].shape[0]
        d.uvs = array(required(uvs, "uvs"), np.float64, (int(n_vertices), 2), "uvs", False, keep)
        device = on_device(image)
        d.texels = array(required(image, "image"), (np.float32, np.float64), (-1, -1), "image", device, keep)
        texels = keep[-1]
        d.height, d.width = int(texels.shape[0]), int(texels.shape[1])
        d.real = D.TAKE_PRECISION_F64 if str(texels.dtype).endswith("float64") else D.TAKE_PRECISION_F32
        d.flags = D.TAKE_DISPLACE_DEVICE_ARRAYS if device else 0
        d.uscale, d.vscale, d.uoffset, d.voffset = (float(x) for x in uvxf)
        wait_for(stream, texels.device if device else None)
        _check(lib().take_hip_displace_create(C.byref(d), C.byref(self._h)))
        info = self.info()
        self.n_vertices, self.n_faces, self.width, self.height = info["n_vertices"], info["n_faces"], info["width"], info["height"]

    @classmethod
    def of_subdiv(cls, subdiv, image, uvxf=(1.0, 1.0, 0.0, 0.0), stream=None):
        """the handle for the surface a Subdiv refines its cage to — a cage with uvs: indices and uvs are its topology()"""
        indices, uvs = subdiv.topology()
        return cls(indices, subdiv.n_vertices, required(uvs, "the cage's uvs"), image, uvxf, stream)

    def info(self):
        """-> {"n_vertices", "n_faces", "width", "height", "device_bytes"} (take_hip_displace_info)"""
        nv, nf, bytes_ = C.c_int64(), C.c_int64(), C.c_int64()
        w, h = C.c_int32(), C.c_int32()
        _check(lib().take_hip_displace_info(self._h, C.byref(nv), C.byref(nf), C.byref(w), C.byref(h), C.byref(bytes_)))
        return {"n_vertices": nv.value, "n_faces": nf.value, "width": w.value, "height": h.value, "device_bytes": bytes_.value}

    def _base(self, positions, normals, keep):
        """-> (positions pointer, normals pointer or None, flags, on the device?) of a base surface: numpy arrays, or
        torch device tensors (both then)"""
        device = on_device(positions) or on_device(normals)
        p = array(required(positions, "positions"), np.float64, (self.n_vertices, 3), "positions", device, keep)
        n = array(normals, np.float64, (self.n_vertices, 3), "normals", device, keep)
        return p, n, (D.TAKE_DISPLACE_DEVICE_ARRAYS if device else 0), device

    def apply_device(self, out_positions, out_normals=None, positions=None, normals=None, scale=1.0, bias=0.0, stream=None):
        """the base surface displaced into device memory (take_hip_displace_apply_device): out_positions, out_normals are
        (n_vertices, 3) float64 torch device tensors or integer device pointers (out_normals None: no normals); normals
        None: the direction is the handle's own vertex normals of `positions`; an output must not be (or overlap) an
        input: displacing in place is refused; runs on `stream` (default: torch's current
        stream when the base is a device tensor, else the default stream) and blocks until done"""
        keep = []
        p, n, flags, device = self._base(positions, normals, keep)
        if device:
            stream = stream_of(stream, keep[0])
        _check(lib().take_hip_displace_apply_device(self._h, C.c_void_p(p), C.c_void_p(n), flags, float(scale), float(bias), C.c_void_p(pointer(out_positions)),
                                                    C.c_void_p(pointer(out_normals)), C.c_void_p(stream or 0)))

    def apply(self, positions, normals=None, scale=1.0, bias=0.0, out_normals=True):
        """-> (positions, normals), or positions alone with out_normals=False: (n_vertices, 3) numpy arrays.  numpy base
        arrays take take_hip_displace_apply; torch device tensors are displaced on torch's current stream and downloaded"""
        if on_device(positions):
            import torch

            out_p = torch.empty((self.n_vertices, 3), dtype=torch.float64, device=positions.device)
            out_n = torch.empty((self.n_vertices, 3), dtype=torch.float64, device=positions.device) if out_normals else None
            self.apply_device(out_p, out_n, positions, normals, scale, bias)
            return (out_p.cpu().numpy(), out_n.cpu().numpy()) if out_normals else out_p.cpu().numpy()
        keep = []
        p, n, _, _ = self._base(positions, normals, keep)
        pos = np.zeros((self.n_vertices, 3), np.float64)
        nrm = np.zeros((self.n_vertices, 3), np.float64) if out_normals else None
        _check(lib().take_hip_displace_apply(self._h, C.c_void_p(p), C.c_void_p(n), float(scale), float(bias), pos.ctypes.data, None if nrm is None else nrm.ctypes.data))
        return (pos, nrm) if out_normals else pos

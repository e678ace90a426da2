"""Shared test helpers: golden scene loading, ray generators, the hostsim wrapper (tests/hostsim)."""
import ctypes as C
import os
import subprocess

import numpy as np

from take_amd import cdefs as D
from take_amd.scene import SceneData, load_tkscene

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GOLDEN_SCENES = ["cbox", "mats", "soup1k", "spherelight", "meshlight"]


def golden_scene(name):
    return load_tkscene(os.path.join(GOLD, "scenes", name + ".tkscene"))


_HOSTSIM = None


def hostsim():
    global _HOSTSIM
    if _HOSTSIM is None:
        d = os.path.join(HERE, "hostsim")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libhostsim.so"))
        L.hostsim_last_error.restype = C.c_char_p
        L.hostsim_render.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.hostsim_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
        L.hostsim_trace_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.POINTER(C.c_uint64)]
        L.hostsim_check_qnodes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.hostsim_env.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.hostsim_tree_prepare.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(D.TakeDebugTreeInfo), C.POINTER(C.c_int32)]
        L.hostsim_tree_copy.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _HOSTSIM = L
    return _HOSTSIM


def render_opts(spp, max_depth, seed=0, ray_epsilon=0.0, strip_first=0, strip_stride=1, samples_per_batch=0,
                integrator=0, exact_bounces=0):
    o = D.TakeRenderOpts()
    o.spp, o.max_depth, o.seed, o.ray_epsilon = spp, max_depth, seed, ray_epsilon
    o.strip_first, o.strip_stride, o.samples_per_batch = strip_first, strip_stride, samples_per_batch
    o.integrator, o.exact_bounces = integrator, exact_bounces
    return o


def n_local_rows(height, first, stride):
    from take_amd.dist import TILE_ROWS as T

    n_strips = (height + T - 1) // T
    return sum(min(height, (s + 1) * T) - s * T for s in range(first, n_strips, stride))


def hostsim_render(sd, precision, spp, max_depth, seed=0, ray_epsilon=0.0, strip_first=0, strip_stride=1,
                   samples_per_batch=0, integrator=0, exact_bounces=0):
    """precision 0 f32, 1 f64, 2 mixed (the first `exact_bounces` rounds in double, the rest in float; double image)"""
    desc, keep = sd.to_desc()
    o = render_opts(spp, max_depth, seed, ray_epsilon, strip_first, strip_stride, samples_per_batch, integrator,
                    exact_bounces)
    rows = n_local_rows(sd.height, strip_first, strip_stride)
    out = np.zeros((rows, sd.width, 3), np.float32 if precision == 0 else np.float64)
    stats = (C.c_uint64 * 7)()
    rc = hostsim().hostsim_render(C.addressof(desc), precision, C.addressof(o), out.ctypes.data, stats)
    if rc != 0:
        raise RuntimeError(hostsim().hostsim_last_error().decode())
    keys = ["closest", "shadow", "nodes", "prims", "max_stack", "bvh_nodes", "bvh_depth"]
    return out, dict(zip(keys, [int(x) for x in stats]))


def rays_to_abi(rays8, precision):
    """(n,8) org3 dir3 tmin tmax -> TakeRayF/D memory layout (org3 tmin dir3 tmax)"""
    r = np.asarray(rays8, np.float64)
    a = np.concatenate([r[:, 0:3], r[:, 6:7], r[:, 3:6], r[:, 7:8]], axis=1)
    return np.ascontiguousarray(a, np.float64 if precision == 1 else np.float32)


def hostsim_trace(sd, precision, rays8, any_hit=False):
    desc, keep = sd.to_desc()
    a = rays_to_abi(rays8, precision)
    hits = np.zeros((a.shape[0], 4), a.dtype)
    rc = hostsim().hostsim_trace(C.addressof(desc), precision, a.ctypes.data, a.shape[0], hits.ctypes.data, int(any_hit))
    if rc != 0:
        raise RuntimeError(hostsim().hostsim_last_error().decode())
    return hits


def hostsim_trace_stats(sd, precision, rays8, any_hit=False, lds_levels=15, drop_from=-1, hits=False):
    """Statistics of hostsim_trace on these rays: "max_stack" — the deepest traversal stack (entries, counted as the trace
    kernel's single stack holds them: a prototype's entries above the top level's and the return marker); "n_nodes",
    "depth" of the tree; "nodes", "prims", "leaves" — interior nodes visited, primitives tested, leaves visited, summed
    over the rays; "rays_deep" — rays whose own stack went beyond `lds_levels` entries; "marker_level" — the highest
    stack level a return marker was put at + 1 (0: no placement entered).
    drop_from >= 0 is a deliberate fault: every entry at that level or above is lost when it is popped, as a broken spill
    area would lose it.  hits=True: also the hit table, as a second value."""
    desc, keep = sd.to_desc()
    a = rays_to_abi(rays8, precision)
    out = (C.c_uint64 * 8)()
    table = np.zeros((a.shape[0], 4), a.dtype) if hits else None
    rc = hostsim().hostsim_trace_stats(C.addressof(desc), precision, a.ctypes.data, a.shape[0], int(any_hit), lds_levels,
                                       drop_from, table.ctypes.data if hits else None, out)
    if rc != 0:
        raise RuntimeError(hostsim().hostsim_last_error().decode())
    st = dict(zip(["max_stack", "n_nodes", "depth", "nodes", "prims", "leaves", "rays_deep", "marker_level"], [int(x) for x in out]))
    return (st, table) if hits else st


def hostsim_env(sd, precision, kind, inp):
    """the device's environment-map functions on the host, rows as take_hip_debug_env's (capi.Scene.debug_env):
    kind 0 (n, 2) draws -> (n, 8) dir[3], radiance[3], pdf, texel; kind 1 (n, 3) directions -> (n, 5) radiance[3], pdf,
    texel.  precision 0 f32, 1 f64"""
    desc, keep = sd.to_desc()
    inp = np.ascontiguousarray(inp, np.float64).reshape(-1, 3 if kind else 2)
    out = np.zeros((inp.shape[0], 5 if kind else 8), np.float64)
    rc = hostsim().hostsim_env(C.addressof(desc), precision, kind, inp.ctypes.data, inp.shape[0], out.ctypes.data)
    if rc != 0:
        raise RuntimeError(hostsim().hostsim_last_error().decode())
    return out


def hostsim_debug_tree(sd, precision, max_leaf_size=0):
    """the tree the HOST builder makes for `sd` (prepare_scene<R>, TAKE_HIP_NODES as the environment has it), in the
    layout of capi.Scene.debug_tree, plus "depth" (take_hip_scene_stats' figure).  precision 0 f32, 1 f64"""
    desc, keep = sd.to_desc()
    info, depth = D.TakeDebugTreeInfo(), C.c_int32()
    if hostsim().hostsim_tree_prepare(C.addressof(desc), precision, max_leaf_size, C.byref(info), C.byref(depth)) != 0:
        raise RuntimeError(hostsim().hostsim_last_error().decode())
    node_t, prim_t, inst_t = D.debug_tree_dtypes(info)
    nodes, prims, inst = np.zeros(info.n_nodes + 1, node_t), np.zeros(info.n_prims + 1, prim_t), np.zeros(info.n_instances + 1, inst_t)
    hostsim().hostsim_tree_copy(precision, nodes.ctypes.data, prims.ctypes.data, inst.ctypes.data)
    tree = D.debug_tree_result(info, nodes[:-1], prims[:-1], inst[:-1])
    tree["depth"] = depth.value
    return tree


def random_linear(rng, n, shear=0.4, scale=(0.4, 2.5)):
    """n linear maps: rotation x non-uniform scale x shear"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                    np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                    np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)
    out = []
    for k in range(n):
        sh = np.eye(3)
        sh[0, 1], sh[0, 2], sh[1, 2] = rng.uniform(-shear, shear, 3)
        out.append(rot[k] @ np.diag(rng.uniform(*scale, 3)) @ sh)
    return out


def sheared_placements():
    """rotated, sheared, non-uniformly scaled placements of three prototypes and nothing else"""
    from take_amd import scenes

    sd = SceneData(width=32, height=32, lookfrom=(0.0, 0.0, 4.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0,
                   background=(0.3, 0.3, 0.3), spp=1, max_depth=2)
    m = sd.add_material(D.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    rng = np.random.default_rng(12)
    protos = [sd.add_prototype(*scenes.soup_triangles(300, 5 + k, 0.15, 0.05), m) for k in range(3)]
    for k, lin in enumerate(random_linear(rng, 90, shear=0.8)):
        sd.add_instance(protos[k % 3], np.concatenate([lin, rng.uniform(-0.8, 0.8, (3, 1))], axis=1))
    return sd


def random_rays(n, seed, camera_fraction=0.25, bounded_fraction=0.3, tmin=1e-4):
    """rays inside the [-1,1]^3 box of the golden scenes, a share of them from the camera position"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.95, 0.95, (n, 3))
    d = rng.normal(size=(n, 3))
    k = int(n * camera_fraction)
    o[:k] = np.array([0, 0, 3.9])
    d[:k] = rng.uniform(-0.3, 0.3, (k, 3)) + np.array([0, 0, -1.0])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = np.where(rng.uniform(size=(n, 1)) < bounded_fraction, rng.uniform(0.05, 2, (n, 1)), np.inf)
    return np.hstack([o, d, np.full((n, 1), tmin), tmax])


def rmse(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)))


def mirror_box_scene(width=48, height=32, n_soup=12, seed=7):
    """A scene whose paths, on the device, need no transcendental function: triangles only (a sphere hit takes acos /
    atan2 for its uv), every surface a white Mirror (F0 = 1: the Schlick term's pow is multiplied by 0 — FG is exactly
    1), so NEE never runs (specular) and the quad light is reached by reflected rays alone.  What is left is +, -, x, /
    and sqrt: the GPU's image can equal the oracle's bit for bit.  The box is open at the front, so paths also end on
    the constant background, whose value (like the light's) is not a float: a path ending in a float round
    contributes float(value), one ending in a double round the value itself — which round a path ends in shows in
    the image."""
    from take_amd import scenes

    sd = SceneData(width=width, height=height, lookfrom=(0.0, 0.0, 3.9), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0),
                   vfov=scenes.vfov_from_xfov(39.0, width, height), background=(0.3, 0.2, 0.1), spp=2, max_depth=50)
    mirror = sd.add_material(D.MAT_MIRROR, (1.0, 1.0, 1.0))
    scenes.box_with_light(sd, mirror, mirror, mirror, light_half=0.35, radiance=(5.3, 4.1, 2.7))
    pos, idx = scenes.soup_triangles(n_soup, seed, half=0.6, jitter=0.35)
    sd.add_mesh(pos, idx, mirror)
    return sd

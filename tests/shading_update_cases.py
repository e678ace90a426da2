"""The scenes and edits of the shading-update tests (take_hip_scene_set_materials, take_hip_scene_set_light_intensities;
DESIGN.md §4p), shared by tests/test_shading_update_cpu.py — the kernels' bodies on the host — and
tests/test_gpu_shading_update.py: small scenes of at most a few hundred records, 16 x 16 pixels."""
import copy
import dataclasses

import numpy as np

from helpers import random_linear
from take_amd import cdefs as D
from take_amd import scenes as S
from take_amd.scene import Light, Material, SceneData

PARAMS = {D.MAT_MIRROR: (1.5,), D.MAT_PLASTIC: (1.5,), D.MAT_PHONG: (20.0,), D.MAT_BLINN_PHONG: (40.0,), D.MAT_BLINN_PHONG_MICROFACET: (50.0,),
          D.MAT_DISNEY_DIFFUSE: (0.5, 0.3), D.MAT_DISNEY_METAL: (0.4, 0.2), D.MAT_DISNEY_GLASS: (0.3, 0.1, 1.5), D.MAT_DISNEY_CLEARCOAT: (0.6,),
          D.MAT_DISNEY_SHEEN: (0.5,), D.MAT_DISNEY_BSDF: (0.5,) * 11 + (1.5,)}
COLOURS = [(0.7, 0.3, 0.2), (0.2, 0.6, 0.3), (0.3, 0.3, 0.8), (0.6, 0.6, 0.6)]
DIFFUSE = D.MAT_DIFFUSE


def mat(tag, colour=(0.5, 0.5, 0.5), tex_image=None, param=None):
    p = tuple(PARAMS.get(tag, ()) if param is None else param)
    return Material(int(tag), tuple(colour), 0 if tex_image is None else 1, 0 if tex_image is None else int(tex_image), (1.0, 1.0, 0.0, 0.0),
                    p + (0.0,) * (12 - len(p)))


def camera(background=(0.4, 0.5, 0.6)):
    return SceneData(width=16, height=16, lookfrom=(0.0, 0.0, 3.9), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0, background=background, spp=4,
                     max_depth=4)


def flat(n_tris, n_spheres=0, tags=(DIFFUSE, DIFFUSE, DIFFUSE), seed=3):
    """n_tris triangles in two meshes (materials 0 and 1) and n_spheres spheres (material 2), lit by the background; the
    table has its three materials whether they are used or not"""
    sd = camera()
    sd.materials = [mat(t, COLOURS[k]) for k, t in enumerate(tags)]
    tri = S.soup_triangles(n_tris, seed, 0.7, 0.3)[0].reshape(-1, 3, 3)
    for k, part in enumerate((tri[:(n_tris + 1) // 2], tri[(n_tris + 1) // 2:])):
        if len(part):
            sd.add_mesh(part.reshape(-1, 3), np.arange(3 * len(part), dtype=np.int32).reshape(-1, 3), k)
    rng = np.random.default_rng(seed + 100)
    for _ in range(n_spheres):
        sd.add_sphere(tuple(rng.uniform(-0.7, 0.7, 3)), 0.15, 2)
    return sd


def textured():
    """two images; two quads with uvs, the first textured with image 0"""
    rng = np.random.default_rng(31)
    sd = camera()
    sd.images = [rng.uniform(0.1, 0.9, (5, 7, 3)), rng.uniform(0.1, 0.9, (3, 2, 3))]
    sd.materials = [mat(DIFFUSE, tex_image=0), mat(DIFFUSE, COLOURS[1])]
    for k, centre in enumerate(((-0.8, 0.0, 0.0), (0.8, 0.0, 0.0))):
        pos, idx, nrm, uv = S._quad(centre, (0.7, 0.0, 0.0), (0.0, 0.7, 0.0), (0.0, 0.0, 1.0))
        sd.add_mesh(pos, idx, k, normals=nrm, uvs=uv)
    return sd


def two_level():
    """a floor of two plain triangles (material 3); prototypes of 20 and 33 triangles (materials 0 and 1); six placements,
    four with the prototype's material (material_id = -1), two with material 2"""
    sd = camera()
    sd.materials = [mat(DIFFUSE, COLOURS[0]), mat(DIFFUSE, COLOURS[1]), mat(D.MAT_PLASTIC, COLOURS[2]), mat(DIFFUSE, COLOURS[3])]
    pos, idx, nrm, uv = S._quad((0.0, -0.9, 0.0), (1.5, 0.0, 0.0), (0.0, 0.0, -1.5), (0.0, 1.0, 0.0))
    sd.add_mesh(pos, idx, 3, normals=nrm, uvs=uv)
    protos = [sd.add_prototype(*S.soup_triangles(n, 5 + k, 0.4, 0.25), k) for k, n in enumerate((20, 33))]
    rng = np.random.default_rng(12)
    for k, lin in enumerate(random_linear(rng, 6, shear=0.3, scale=(0.6, 1.2))):
        sd.add_instance(protos[k % 2], np.concatenate([0.8 * lin, rng.uniform(-0.6, 0.6, (3, 1))], axis=1), -1 if k < 4 else 2)
    return sd


def reposed(sd, seed=7):
    """other transforms for the placements of sd -> (n, 3, 4)"""
    rng = np.random.default_rng(seed)
    n = len(sd.instance_mesh)
    return np.stack([np.concatenate([0.7 * lin, rng.uniform(-0.5, 0.5, (3, 1))], axis=1) for lin in random_linear(rng, n, shear=0.3, scale=(0.6, 1.2))])


def with_transforms(sd, xforms):
    out = copy.copy(sd)
    out.instance_xform = [np.array(x, np.float64).reshape(3, 4) for x in xforms]
    return out


def with_positions(sd, mesh, positions):
    out = copy.copy(sd)
    out.meshes = list(sd.meshes)
    out.meshes[mesh] = dataclasses.replace(sd.meshes[mesh], positions=np.ascontiguousarray(positions, np.float64))
    return out


def bent(pos):
    return pos + 0.1 * np.sin(3.0 * pos[:, [1, 2, 0]] + 0.5)


def with_materials(sd, first, materials):
    """the description with materials first, first + 1, ... replaced"""
    out = copy.copy(sd)
    out.materials = list(sd.materials)
    out.materials[first:first + len(materials)] = list(materials)
    assert len(out.materials) == len(sd.materials)
    return out


def with_intensities(sd, first, rgb):
    """the description with the intensities of lights first, first + 1, ... replaced"""
    out = copy.copy(sd)
    out.lights = list(sd.lights)
    for k, v in enumerate(np.asarray(rgb, np.float64)):
        out.lights[first + k] = dataclasses.replace(sd.lights[first + k], intensity=tuple(float(x) for x in v))
    return out


# name -> (the scene, first, the new materials, keywords of capi.Scene, whether a tag changes)
def material_cases():
    grey = (0.45, 0.5, 0.55)
    cases = {
        "colours": (flat(65, 2), 0, [mat(DIFFUSE, (0.1, 0.8, 0.4)), mat(DIFFUSE, (0.9, 0.2, 0.2))], {}, False),
        "parameters": (flat(65, 2, (DIFFUSE, D.MAT_PHONG, D.MAT_PLASTIC)), 1, [mat(D.MAT_PHONG, grey, param=(7.0,)), mat(D.MAT_PLASTIC, grey, param=(1.3,))], {}, False),
        "mirror": (flat(65, 2, (DIFFUSE, D.MAT_PLASTIC, DIFFUSE)), 0, [mat(D.MAT_MIRROR, (0.9, 0.9, 0.9))], {}, True),
        "1to2": (flat(65, 2), 1, [mat(D.MAT_PHONG, grey)], {}, True),
        "2to1": (flat(65, 2, (DIFFUSE, D.MAT_PHONG, DIFFUSE)), 1, [mat(DIFFUSE, grey)], {}, True),
        "unused-material": (flat(30, 0), 2, [mat(D.MAT_BLINN_PHONG, grey)], {}, True),  # (no sphere uses material 2: the tags in use still count it)
        "burley": (flat(65, 2, (DIFFUSE, D.MAT_DISNEY_BSDF, DIFFUSE)), 0, [mat(D.MAT_DISNEY_METAL, grey), mat(D.MAT_DISNEY_GLASS, grey), mat(D.MAT_DISNEY_SHEEN, grey)],
                   {"burley_lobes": True}, True),
        "texture": (textured(), 0, [mat(DIFFUSE, tex_image=1)], {}, False),
        "first>0": (flat(65, 2), 2, [mat(D.MAT_PLASTIC, grey)], {}, True),
        "root-leaf": (flat(3, 0), 0, [mat(D.MAT_MIRROR, grey), mat(D.MAT_PHONG, grey)], {}, True),
        "spheres": (flat(40, 9), 1, [mat(D.MAT_MIRROR, grey), mat(D.MAT_BLINN_PHONG_MICROFACET, grey)], {}, True),
        "two-level": (two_level(), 0, [mat(D.MAT_MIRROR, grey), mat(DIFFUSE, COLOURS[1]), mat(D.MAT_PHONG, grey)], {}, True),
        "flattened": (two_level(), 0, [mat(D.MAT_MIRROR, grey), mat(DIFFUSE, COLOURS[1]), mat(D.MAT_PHONG, grey)], {"flatten_instances": True}, True),
    }
    for n in (1, 63, 64, 65, 257):
        cases[f"{n}-records"] = (flat(n, 0), 0, [mat(D.MAT_MIRROR, grey), mat(D.MAT_PHONG, grey)], {}, True)
    return cases


def lit(n_emissive, env=False, seed=9):
    """a floor, an emissive mesh of n_emissive triangles (lights 0 .. n - 1), a sphere light (n), a point light (n + 1)
    and, with env, an environment map (n + 2)"""
    sd = camera((0.0, 0.0, 0.0))
    sd.materials = [mat(DIFFUSE, COLOURS[3])]
    pos, idx, nrm, uv = S._quad((0.0, -0.9, 0.0), (1.5, 0.0, 0.0), (0.0, 0.0, -1.5), (0.0, 1.0, 0.0))
    sd.add_mesh(pos, idx, 0, normals=nrm, uvs=uv)
    pos, idx = S.soup_triangles(n_emissive, seed, 0.6, 0.2)
    sd.add_mesh(pos + (0.0, 0.3, 0.0), idx, 0, normals=np.tile((0.0, -1.0, 0.0), (pos.shape[0], 1)), emission=(3.0, 2.0, 1.0))
    sd.add_sphere((0.6, 0.6, 0.2), 0.2, 0, emission=(5.0, 5.0, 4.0))
    sd.lights.append(Light(0, -1, (9.0, 9.0, 9.0), (0.0, 2.0, 1.0)))
    if env:
        sd.add_envmap(np.random.default_rng(seed).uniform(0.05, 1.0, (4, 8, 3)), scale=(0.5, 0.6, 0.7))
    return sd


def intensities(n, seed=1):
    return np.random.default_rng(seed).uniform(0.5, 6.0, (n, 3))


# name -> (the scene, first, the new intensities)
def light_cases():
    cases = {}
    for n in (1, 2, 64, 65, 300):
        cases[f"{n}-triangles"] = (lit(n), 0, intensities(n + 2, n))  # (the sphere light and the point light are in the range)
    cases["sphere-light"] = (lit(5), 5, intensities(1))
    cases["point-light"] = (lit(5), 4, intensities(3))
    cases["sub-range"] = (lit(65), 10, intensities(40))
    cases["dark"] = (lit(5), 0, np.zeros((7, 3)))  # (total power 0: creation's NaN tables)
    cases["env"] = (lit(5, env=True), 3, intensities(5))
    return cases

"""TEST INFRASTRUCTURE: a numpy float64 restatement of displacement mapping as DESIGN.md §4t specifies it
(include/take_hip.h has the summary), written from the specification: every + - * / below is one elementwise IEEE
operation over all vertices at once, in the order the specification writes them.  The normals are subdiv_ref's
(§4s's rule, which §4t takes over).  Also the cases the CPU and the GPU tests share (cases())."""
import functools

import numpy as np

import subdiv_ref

BELOW_ONE = np.nextafter(1.0, 0.0)  # the largest double below 1


def modulo1(a):
    """modulo(a, 1) of the texture lookup: fmod, a negative remainder plus 1, and the largest double below 1 where that
    sum rounds to 1"""
    r = np.fmod(a, 1.0)
    up = r + 1.0
    up = np.where(up < 1.0, up, BELOW_ONE)
    return np.where(r < 0.0, up, r)


def sources(uvs, uvxf):
    """-> (a, b) of every vertex; uvxf = (uscale, vscale, uoffset, voffset)"""
    uv = np.asarray(uvs, np.float64)
    uscale, vscale, uoffset, voffset = (np.float64(x) for x in uvxf)
    s = uscale * uv[:, 0] + uoffset
    t = vscale * uv[:, 1] + voffset
    if not (np.isfinite(s).all() and np.isfinite(t).all()):
        raise ValueError("a lookup coordinate that is not finite")
    return modulo1(s), modulo1(t)


def cell(c, n):
    """-> (i1, i2, f) along an axis of n texels"""
    x = np.float64(n) * c
    x1 = np.floor(x)
    f = x - x1
    i1 = x1.astype(np.int64)
    i2 = np.where(i1 + 1 == n, 0, i1 + 1)
    return i1, i2, f


def heights(image, a, b):
    """bilinear with wrap over image (height, width), float32 or float64 -> (h, (x1, x2, y1, y2), (fx, fy))"""
    tex = np.asarray(image).astype(np.float64)  # (a float texel is widened, which is exact)
    height, width = tex.shape
    x1, x2, fx = cell(a, width)
    y1, y2, fy = cell(b, height)
    q11, q21, q12, q22 = tex[y1, x1], tex[y1, x2], tex[y2, x1], tex[y2, x2]
    with np.errstate(invalid="ignore"):
        h = (q11 * (1.0 - fx) + q21 * fx) * (1.0 - fy) + (q12 * (1.0 - fx) + q22 * fx) * fy
    return h, (x1, x2, y1, y2), (fx, fy)


def displace(positions, normals, indices, uvs, image, uvxf, scale, bias):
    """-> (displaced positions, the direction normals, the normals of the displaced positions); normals None: the
    direction is the vertex normals of `positions`"""
    p = np.asarray(positions, np.float64)
    n = subdiv_ref.vertex_normals(p, indices) if normals is None else np.asarray(normals, np.float64)
    a, b = sources(uvs, uvxf)
    h, _, _ = heights(image, a, b)
    with np.errstate(invalid="ignore"):
        d = np.float64(scale) * h + np.float64(bias)
        out = p + d[:, None] * n
        return out, n, subdiv_ref.vertex_normals(out, indices)


# ---------------------------------------------------------------------------------------------------- the cases
def image(width, height, dtype, nan=False):
    """a height image (height, width): smooth, signed, no two neighbours equal; values that a float holds exactly when
    dtype is float32"""
    y, x = np.mgrid[0:height, 0:width]
    img = (0.6 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y - 0.2) + 0.05 * ((3 * x + 5 * y) % 7) - 0.1).astype(dtype)
    if nan:
        img[height // 2, width // 3] = np.nan
    return np.ascontiguousarray(img)


# width x height
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (16, 16)]
# uvs of the first vertices of every mesh: exactly 0 and exactly 1, the BELOW_ONE case, the wrap cell in x and in y,
# above 1 and negative
CORNER_UVS = np.array([[0.0, 0.0], [1.0, 1.0], [-1e-20, 0.5], [0.999, -0.3], [1.6, 0.97], [-0.75, 2.25]])
IDENTITY, SKEWED = (1.0, 1.0, 0.0, 0.0), (1.7, -0.6, 0.25, 0.4)
AMPLITUDES = [(0.3, 0.0), (0.0, 0.25), (-0.2, 0.05)]  # (scale, bias): plain, scale 0 with a bias, a negative scale


def mesh_uvs(nv):
    i = np.arange(nv, dtype=np.float64)
    uv = np.stack([-1.5 + 4.0 * ((i * 0.61803) % 1.0), 2.5 - 4.0 * ((i * 0.41421) % 1.0)], axis=1)
    k = min(nv, len(CORNER_UVS))
    uv[:k] = CORNER_UVS[:k]
    return uv


@functools.lru_cache(maxsize=None)
def meshes():
    """[(name, positions, normals, indices, uvs)]: the octahedron with uvs at L = 2 (66 vertices), the bent strip of 23
    with uvs at L = 2 (215, with a boundary), a strip with a vertex no face uses, a single triangle"""
    out = []
    for name, (pos, idx) in (("octahedron-L2", subdiv_ref.octahedron()), ("strip23-L2", subdiv_ref.strip(23))):
        if name == "octahedron-L2":
            pos = pos * np.array([1.0, 0.8, 1.3]) + 0.1
        p, n, i = subdiv_ref.refine(pos, idx, 2)
        _, _, uv = subdiv_ref.topology(idx, pos.shape[0], 2, mesh_uvs(pos.shape[0]))
        out.append((name, p, n, i, uv))
    pos, idx = subdiv_ref.strip(9)
    pos = np.concatenate([pos, [[0.3, 2.0, -1.0]]])
    out.append(("strip9-unused-vertex", pos, subdiv_ref.vertex_normals(pos, idx), idx, mesh_uvs(10)))
    pos, idx = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.2], [0.2, 1.0, -0.1]]), np.array([[0, 1, 2]], np.int32)
    out.append(("triangle", pos, subdiv_ref.vertex_normals(pos, idx), idx, mesh_uvs(3)))
    for _, p, n, i, uv in out:
        for a in (p, n, i, uv):
            a.setflags(write=False)
    assert [m[1].shape[0] for m in out] == [66, 215, 10, 3]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[{name, positions, normals (None: the handle's own), indices, uvs, image, uvxf, scale, bias}]: every mesh under
    every image shape with float and with double texels and under the image with a NaN texel; the lookup, the amplitude
    and whose normals give the direction rotate through the list"""
    out = []
    k = 0
    for name, p, n, i, uv in meshes():
        images = [(f"{w}x{h}-{np.dtype(t).name}", image(w, h, t)) for (w, h) in SHAPES for t in (np.float32, np.float64)]
        images.append(("5x3-nan", image(5, 3, np.float64, nan=True)))
        for tag, img in images:
            img.setflags(write=False)
            scale, bias = AMPLITUDES[k % 3]
            out.append({"name": f"{name}/{tag}", "mesh": name, "positions": p, "normals": None if k % 2 else n, "indices": i, "uvs": uv, "image": img,
                        "uvxf": SKEWED if (k // 2) % 2 else IDENTITY, "scale": scale, "bias": bias, "nan": tag.endswith("nan")})
            k += 1
    return out

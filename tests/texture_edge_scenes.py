"""Scenes that take the edge-case texture coordinates of tests/texture_edge_cases.py through the real kernels
(tests/test_gpu_texture_edges.py), and what to expect of them from the oracle's hits and the exact reference of
tests/texture_ref.py alone.  No GPU is needed for anything in here (tests/test_texture_cpu.py checks the scenes).

quad_scene: the six images in one pool, a Diffuse material per image plus one with uscale = vscale = -1 (on the 8x4
image) and one with uoffset = voffset = -0.5 (on the 5x4 image); a 16 x 12 grid of quads in the plane z = 0 that fills a
128 x 96 pinhole image, each quad 8 x 8 pixels and a mesh of its own with vertex normals, all four vertices with the same
uv: c on u alone, on v alone and on both, c in C_VALUES.  Constant background, no lights.

What a sample looks up is not exactly c: the hit's uv is (1 - bu - bv) c + bu c + bv c, a few roundings away.  Where the
coordinate a = scale * c + offset sits on a wrap seam (a an integer: c = 1, c = 0.5 under the offset; in f32 also
pred32(1) and 0.5 - 2^-25, which the interpolation can round onto the integer) those roundings decide between the cell
W-1 and the cell 0, whose values differ.  Both are lookups of a valid coordinate.  So a quad has a set of candidate
values — the exact reference at a and at a -+ 4 ulp of the precision, where these fall in different cells — and a pixel,
the mean of four samples, has to be a mean of four candidates.  For every other quad (all those inside the window where
r + 1 rounds to 1 among them) there is one candidate: the exact reference at c."""
import itertools
import math
from fractions import Fraction

import numpy as np

import oracle
import texture_edge_cases as K
import texture_ref as T
from take_amd import cdefs as D
from take_amd.scene import SceneData

PRED32 = 1.0 - 2.0 ** -24
C_VALUES = (-2.0 ** -26, -0.0, 0.0, PRED32, 1.0, 0.5, 2.0 ** -26, 0.5 - 2.0 ** -25)
COLS, ROWS, CELL = 16, 12, 8
SPP, SEED = 4, 5
BACKGROUND = (0.7, 0.8, 0.9)
# (image, uvxf) of the eight materials
MATERIALS = [(k, (1.0, 1.0, 0.0, 0.0)) for k in range(6)] + [(5, (-1.0, -1.0, 0.0, 0.0)), (4, (1.0, 1.0, -0.5, -0.5))]


def quad_uvs():
    """the uv of each of the 24 quads of a material"""
    return [(c, K.OTHER) for c in C_VALUES] + [(K.OTHER, c) for c in C_VALUES] + [(c, c) for c in C_VALUES]


def quad_scene():
    """-> (SceneData, quads): quads[q] = (material, (cu, cv)); quad q is the shapes 2q and 2q + 1"""
    sd = SceneData(width=COLS * CELL, height=ROWS * CELL, lookfrom=(0.0, 0.0, 2.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0),
                   vfov=2.0 * math.degrees(math.atan(0.5)), background=BACKGROUND, spp=SPP, max_depth=5)
    sd.images = K.images()
    for image, uvxf in MATERIALS:
        sd.add_material(D.MAT_DIFFUSE, (0.5, 0.5, 0.5), tex_image=image, uvxf=uvxf)
    quads = [(m, uv) for m in range(len(MATERIALS)) for uv in quad_uvs()]
    assert len(quads) == COLS * ROWS
    s = 2.0 / ROWS  # the image is 2 high in the plane z = 0
    for q, (m, uv) in enumerate(quads):
        x0, y0 = -s * COLS / 2 + s * (q % COLS), 1.0 - s * (q // COLS + 1)
        pos = [(x0, y0, 0.0), (x0 + s, y0, 0.0), (x0 + s, y0 + s, 0.0), (x0, y0 + s, 0.0)]
        sd.add_mesh(pos, [(0, 1, 2), (0, 2, 3)], m, normals=[(0.0, 0.0, 1.0)] * 4, uvs=[uv] * 4)
    return sd, quads


def interior_pixels(sd, hit, n_quads):
    """hit: the oracle's record per camera sample -> per quad the (H, W) mask of the pixels whose samples all hit it and
    whose eight neighbours do too"""
    quad = np.where(hit[:, 0] != 0, hit[:, 16].astype(int) // 2, -1).reshape(sd.height, sd.width, -1)
    out = []
    for q in range(n_quads):
        m = (quad == q).all(-1)
        p = np.pad(m, 1)
        inner = m.copy()
        for dy, dx in itertools.product((0, 1, 2), (0, 1, 2)):
            inner &= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
        out.append(inner)
    return out


def axis_candidates(c, scale, offset, n, real):
    """the coordinates one axis of a quad can be looked up at: [a], or [a - d, a + d] where the interpolation's rounding
    (d = 4 ulp of the larger of |scale * c| and |a|) can put a sample in either of two cells"""
    p = Fraction(T.rounded(scale, real)) * Fraction(T.rounded(c, real))
    a = p + Fraction(T.rounded(offset, real))
    big = max(abs(p), abs(a))
    if big == 0:
        return [a]
    d = 4 * T.ulp(big, real)
    cells = {T.axis(a + k, n)[1] for k in (-d, 0, d)}
    return [a] if len(cells) == 1 else [a - d, a + d]


def quad_candidates(images, quad, real):
    """-> (k, 3): the values a sample of the quad can have (k = 1: the exact reference at its uv)"""
    m, (cu, cv) = quad
    image, (us, vs, uo, vo) = MATERIALS[m]
    img = images[image]
    t = T.texels(img, real)
    xs, ys = axis_candidates(cu, us, uo, img.shape[1], real), axis_candidates(cv, vs, vo, img.shape[0], real)
    return np.array([T.lookup_at(t, ax, ay) for ax in xs for ay in ys])


def pixel_errors(pix, cand):
    """pix (n, 3), cand (k, 3) -> (n,) the distance (largest channel) of each pixel to the nearest mean of SPP candidates"""
    pix = np.asarray(pix, np.float64)
    best = np.full(len(pix), np.inf)
    for combo in itertools.combinations_with_replacement(range(len(cand)), SPP):
        total = np.zeros(3)
        for k in combo:  # (the order of the sum is the device's business; the bar is far above its rounding)
            total = total + cand[k]
        best = np.minimum(best, np.abs(pix - total / SPP).max(-1))
    return best


def sphere_scene():
    """a sphere textured with the 8x4 image seen from straight above: the pole theta = pi (v = -1) at the image centre,
    the u seam (u = 0 | 1) a radius of the disc"""
    sd = SceneData(width=48, height=48, lookfrom=(0.0, 3.0, 0.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), vfov=40.0,
                   background=BACKGROUND, spp=SPP, max_depth=5)
    sd.images = [K.images()[5]]
    m = sd.add_material(D.MAT_DIFFUSE, (0.5, 0.5, 0.5), tex_image=0)
    sd.add_sphere((0.0, 0.0, 0.0), 1.0, m)
    return sd


def albedo_plane(sd, hit, real):
    """the albedo plane of the feature pass from the oracle's hits of the camera samples and the exact reference"""
    albedo = np.zeros((hit.shape[0], 3))
    for k, m in enumerate(sd.materials):
        sel = (hit[:, 0] != 0) & (hit[:, 13].astype(int) == k)
        rows = np.concatenate([hit[sel, 11:13], np.broadcast_to(np.asarray(m.uvxf, np.float64), (int(sel.sum()), 4))], 1)
        uniq, back = np.unique(rows, axis=0, return_inverse=True)  # (the samples of a quad share a handful of uvs)
        albedo[sel] = T.lookup_rows(sd.images[m.tex_image], uniq, real)[back.reshape(-1)]
    a = albedo.reshape(sd.height, sd.width, -1, 3)
    total = np.zeros_like(a[:, :, 0])
    for s in range(a.shape[2]):
        total = total + a[:, :, s]
    return total / a.shape[2]


def oracle_hits(sd, rays, precision=1):
    osc = oracle.OracleScene(sd, precision)
    try:
        return osc.isect(rays)
    finally:
        osc.close()

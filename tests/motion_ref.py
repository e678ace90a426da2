"""The motion pass that follows moved vertices (take_hip_scene_track_vertices; take_amd/csrc/tk_motion_pixel.h:
tracked_pixel; DESIGN.md par. 4i), restated in numpy, one array operation per operation of the specification, in the
dtype asked for; and what the tests of it share: synthetic hit records, deformations, the records' view of a mesh.

    a triangle hit (u along e1, v along e2, the MARKED words v0', e1', e2' of the hit record's identity):
        Q' = (v0' + e1' * u) + e2' * v  per component;  in a placement P' = M(marked) * Q', otherwise P' = Q'
    a sphere hit:  P = o + d * t;  in a placement P' = M(marked) * (inv(current) * P), otherwise P' = P
    a miss:  e = d;  otherwise e = P' - lookfrom'
    the projection with the marked camera, prev_depth: as temporal_ref.reproject

A 3 x 4 map is applied row by row as ((m0 * x + m1 * y) + m2 * z) + m3, a dot product is (a.x * b.x + a.y * b.y) + a.z * b.z,
M(marked) is 12 doubles each rounded to the dtype once."""
import numpy as np

MISS, POINT, TRIANGLE = 0, 1, 2


def _affine(m, p):
    """m (n, 12) row-major 3 x 4, p (n, 3), one dtype -> (n, 3)"""
    return np.stack([((m[:, 4 * r] * p[:, 0] + m[:, 4 * r + 1] * p[:, 1]) + m[:, 4 * r + 2] * p[:, 2]) + m[:, 4 * r + 3] for r in range(3)], -1)


def _dot(a, e):
    """a (3,), e (n, 3)"""
    return (a[0] * e[:, 0] + a[1] * e[:, 1]) + a[2] * e[:, 2]


def camera_words(cam, dtype):
    """a temporal_ref.camera -> its 14 Reals (u, v, w, lookfrom, viewport_width, viewport_height) rounded to dtype"""
    return np.concatenate([cam["u"], cam["v"], cam["w"], cam["from"], [cam["vw"], cam["vh"]]]).astype(dtype)


def tracked_pixels(cam, kind, ro, rd, t, u, v, words, inv, fwd, placed, dtype=np.float64):
    """cam: a temporal_ref.camera (the MARKED one); n records: kind (MISS / POINT / TRIANGLE), ro, rd (n, 3), t, u, v (n,),
    words (n, 9) = v0', e1', e2', inv (n, 12), fwd (n, 12) float64, placed (n,) bool -> prev_xy (n, 2), prev_depth (n,).
    Every array is rounded to dtype first (fwd too: once), every operation is one operation in dtype."""
    R = np.dtype(dtype).type
    c = camera_words(cam, dtype)
    cu, cv, cw, cf, vw, vh = c[0:3], c[3:6], c[6:9], c[9:12], c[12], c[13]
    W, H = R(cam["width"]), R(cam["height"])
    kind, placed = np.asarray(kind), np.asarray(placed, bool)
    ro, rd, t, u, v, words, inv, fwd = (np.asarray(a).astype(dtype) for a in (ro, rd, t, u, v, words, inv, fwd))
    with np.errstate(all="ignore"):
        q = np.stack([(words[:, a] + words[:, 3 + a] * u) + words[:, 6 + a] * v for a in range(3)], -1)
        p = ro + rd * t[:, None]
        p = np.where(placed[:, None], _affine(inv, p), p)
        P = np.where((kind == TRIANGLE)[:, None], q, p)
        P = np.where(placed[:, None], _affine(fwd, P), P)
        e = np.where((kind == MISS)[:, None], rd, P - cf)
        z = -_dot(cw, e)
        sx = (_dot(cu, e) / z / vw + R(0.5)) * W
        sy = (_dot(cv, e) / z / vh + R(0.5)) * H
        seen = z > 0
        xy = np.where(seen[:, None], np.stack([sx, H - sy], -1), R(-2))
        pd = np.where(seen & (kind != MISS), np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]), R(0))
    return xy.astype(dtype), pd.astype(dtype)


# ------------------------------------------------------------------ from a scene description to records
def triangle_words(positions, indices, dtype=np.float64):
    """PrimRec::a of every face of a mesh: v0, e1 = v1 - v0, e2 = v2 - v0 of the positions rounded to dtype -> (faces, 9)"""
    p = np.asarray(positions, np.float64).astype(dtype)[np.asarray(indices)]
    return np.concatenate([p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]], -1)


def affine12(m):
    """(..., 3, 4) -> (..., 12) row-major"""
    m = np.asarray(m, np.float64)
    return m.reshape(m.shape[:-2] + (12,))


def inverse12(m):
    """(n, 3, 4) -> the inverse maps (n, 12), float64"""
    m = np.asarray(m, np.float64)
    a = np.linalg.inv(m[..., :3])
    return affine12(np.concatenate([a, -np.einsum("...ij,...j->...i", a, m[..., 3])[..., None]], -1))


# ------------------------------------------------------------------ the synthetic records of the CPU test
def synthetic_records(seed=3, n=600):
    """Records for tracked_pixels in float64, made once per call: every kind, in and out of a placement; u, v on the
    corners (0, 0), (1, 0), (0, 1), on the edges and inside; points in front of the camera and behind it; and records
    with a NaN in each input in turn.  -> (cam, dict of arrays)"""
    import temporal_ref as T

    rng = np.random.default_rng(seed)
    cam = T.camera((0.3, 0.2, 4.0), (0.1, -0.1, 0.0), (0.0, 1.0, 0.0), 40.0, 48, 32)
    kind = rng.integers(0, 3, n).astype(np.int32)
    placed = (rng.random(n) < 0.5) & (kind != MISS)
    corners = np.array([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.5, 0.0), (0.0, 0.5)])
    uv = rng.dirichlet((1.0, 1.0, 1.0), n)[:, :2]
    special = rng.random(n) < 0.4
    uv[special] = corners[rng.integers(0, len(corners), int(special.sum()))]
    words = np.concatenate([rng.uniform(-1.0, 1.0, (n, 3)), rng.uniform(-0.7, 0.7, (n, 6))], -1)
    ro = np.broadcast_to(cam["from"], (n, 3)).copy()
    rd = rng.normal(size=(n, 3)) * 0.3 - cam["w"]
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    t = rng.uniform(1.0, 6.0, n)
    ang = rng.uniform(-0.6, 0.6, n)
    rot = np.zeros((n, 3, 4))
    rot[:, 0, 0], rot[:, 0, 2], rot[:, 2, 0], rot[:, 2, 2], rot[:, 1, 1] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang), 1.0
    rot[:, :, :3] *= rng.uniform(0.5, 1.5, (n, 1, 1))
    rot[:, :, 3] = rng.uniform(-0.5, 0.5, (n, 3))
    cur = rot.copy()
    cur[:, :, 3] += rng.uniform(-0.2, 0.2, (n, 3))
    fwd, inv = affine12(rot), inverse12(cur)
    # behind the camera: the geometry pushed past lookfrom along +w (triangles and points alike)
    behind = rng.random(n) < 0.1
    words[behind, :3] = cam["from"] + 3.0 * cam["w"] + rng.uniform(-0.1, 0.1, (int(behind.sum()), 3))
    placed &= ~behind
    uv[behind] = 0.0
    t[behind] = -t[behind]
    # not a number, in one input each
    nan = np.flatnonzero(rng.random(n) < 0.08)
    for k, i in enumerate(nan):
        (words[i], uv[i], fwd[i], rd[i], t[i:i + 1])[k % 5][0] = np.nan
    return cam, dict(kind=kind, ro=ro, rd=rd, t=t, u=uv[:, 0].copy(), v=uv[:, 1].copy(), words=words, inv=inv, fwd=fwd, placed=placed)

"""TEST INFRASTRUCTURE: a numpy float64 restatement of Loop subdivision as DESIGN.md §4s specifies it (include/take_hip.h
has the summary), written from the specification: every + - * / below is one elementwise IEEE operation over all
vertices at once, in the order the specification writes them; no sum(), no @, no np.cross.  Also the cages the CPU and
the GPU tests share (cases())."""
import numpy as np


# ---------------------------------------------------------------------------------------------------- topology
def edges(indices, n_vertices):
    """the edges of a mesh: the distinct unordered corner pairs in ascending (lo, hi) order -> (lo, hi, c, d, edge_of):
    c the opposite corner in the lower-numbered face, d in the higher (-1: one face only); edge_of (F, 3): the edge of
    every face's side k = corners (k, k + 1)"""
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    F = idx.shape[0]
    a, b, opp = idx[:, [0, 1, 2]].ravel(), idx[:, [1, 2, 0]].ravel(), idx[:, [2, 0, 1]].ravel()
    face = np.repeat(np.arange(F), 3)
    key = np.minimum(a, b) * int(n_vertices) + np.maximum(a, b)
    order = np.lexsort((face, key))  # by edge, the lower-numbered face first
    ks = key[order]
    new = np.concatenate([[True], ks[1:] != ks[:-1]])
    eid = np.cumsum(new) - 1
    first = np.flatnonzero(new)
    count = np.diff(np.concatenate([first, [len(ks)]]))
    if (count > 2).any():
        raise ValueError("an edge with more than two faces")
    lo, hi = ks[first] // int(n_vertices), ks[first] % int(n_vertices)
    c = opp[order][first]
    d = np.where(count == 2, opp[order][np.minimum(first + 1, len(ks) - 1)], -1)
    edge_of = np.zeros(3 * F, np.int64)
    edge_of[order] = eid
    return lo, hi, c, d, edge_of.reshape(F, 3)


def rows(owner, value, n):
    """the values of every owner 0 .. n-1, ascending, as a matrix padded with -1 -> (matrix, row lengths)"""
    order = np.lexsort((value, owner))
    owner, value = owner[order], value[order]
    count = np.bincount(owner, minlength=n)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    m = np.full((n, max(int(count.max()), 1) if n else 1), -1, np.int64)
    m[owner, np.arange(len(owner)) - start[owner]] = value
    return m, count


def refine_topology(indices, n_vertices, uvs=None):
    """one level -> (new indices (4F, 3), new vertex count, new uvs or None, the edges (lo, hi, c, d))"""
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    V = int(n_vertices)
    lo, hi, c, d, edge_of = edges(idx, V)
    a, b, cc = idx[:, 0], idx[:, 1], idx[:, 2]
    ab, bc, ca = V + edge_of[:, 0], V + edge_of[:, 1], V + edge_of[:, 2]
    new = np.stack([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, cc], 1), np.stack([ab, bc, ca], 1)], axis=1).reshape(-1, 3)
    new_uv = None
    if uvs is not None:
        uv = np.asarray(uvs, np.float64)
        new_uv = np.concatenate([uv, 0.5 * (uv[lo] + uv[hi])])
    return new.astype(np.int32), V + len(lo), new_uv, (lo, hi, c, d)


def topology(indices, n_vertices, levels, uvs=None):
    """-> (refined indices, refined vertex count, refined uvs or None)"""
    idx, V, uv = indices, n_vertices, uvs
    for _ in range(levels):
        idx, V, uv, _ = refine_topology(idx, V, uv)
    return idx, V, uv


# ---------------------------------------------------------------------------------------------------- positions
def refine_positions(positions, indices):
    """one level of positions over the mesh `indices` -> (V + E, 3)"""
    p = np.asarray(positions, np.float64)
    V = p.shape[0]
    lo, hi, c, d, _ = edges(indices, V)
    inner = d >= 0
    # odd vertices
    odd = np.where(inner[:, None], 0.375 * (p[lo] + p[hi]) + 0.125 * (p[c] + p[np.maximum(d, 0)]), 0.5 * (p[lo] + p[hi]))
    # even vertices
    nb, n = rows(np.concatenate([lo, hi]), np.concatenate([hi, lo]), V)
    bn, nbnd = rows(np.concatenate([lo[~inner], hi[~inner]]), np.concatenate([hi[~inner], lo[~inner]]), V)
    if ((nbnd != 0) & (nbnd != 2)).any():
        raise ValueError("a boundary vertex with other than two boundary edges")
    s = p[np.maximum(nb[:, 0], 0)].copy()
    for k in range(1, nb.shape[1]):
        m = k < n
        s[m] = s[m] + p[nb[m, k]]
    nf = np.maximum(n, 1).astype(np.float64)
    beta = np.where(n == 3, 3.0 / 16.0, 3.0 / (8.0 * nf))
    interior = (1.0 - nf * beta)[:, None] * p + beta[:, None] * s
    even = interior
    on_boundary = nbnd == 2
    if on_boundary.any():
        b0, b1 = bn[on_boundary, 0], bn[on_boundary, 1]
        even = even.copy()
        even[on_boundary] = 0.75 * p[on_boundary] + 0.125 * (p[b0] + p[b1])
    even = np.where((n == 0)[:, None], p, even)
    return np.concatenate([even, odd])


def vertex_normals(positions, indices):
    """N_f = cross(p1 - p0, p2 - p0); per vertex the sum over its faces in ascending face order, starting from the first;
    divided by its length when that is positive and finite"""
    p = np.asarray(positions, np.float64)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    u, v = p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]]
    N = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    fr, n = rows(idx.ravel(), np.repeat(np.arange(idx.shape[0]), 3), p.shape[0])
    s = np.where((n > 0)[:, None], N[np.maximum(fr[:, 0], 0)], 0.0)
    for k in range(1, fr.shape[1]):
        m = k < n
        s[m] = s[m] + N[fr[m, k]]
    with np.errstate(all="ignore"):
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (length > 0) & np.isfinite(length)
        return np.where(ok[:, None], s / np.where(ok, length, 1.0)[:, None], s)


def refine(positions, indices, levels, normals=True):
    """-> (refined positions, refined normals or None, refined indices)"""
    p, idx = np.asarray(positions, np.float64), np.asarray(indices, np.int32).reshape(-1, 3)
    for _ in range(levels):
        q = refine_positions(p, idx)
        idx, _, _, _ = refine_topology(idx, p.shape[0])
        p = q
    return p, (vertex_normals(p, idx) if normals else None), idx


# ---------------------------------------------------------------------------------------------------- the cages
def octahedron():
    pos = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    idx = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return pos, idx


def tetrahedron():
    pos = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * np.array([0.9, 1.0, 1.1])
    idx = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return pos, idx


def strip(nv, y0=-0.2):
    """a bent strip of triangles over nv vertices in two rows: nv - 2 faces (the shape of strip() in test_gpu_skin.py)"""
    i = np.arange(nv)
    x = -1.0 + 2.0 * (i // 2) / max((nv - 1) // 2, 1)
    pos = np.stack([x, y0 + 0.4 * (i % 2), 0.3 * np.sin(2.0 * x)], axis=1)
    idx = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(nv - 2)], np.int32)
    return pos, idx


def fan(n, closed):
    """vertex 0 in the middle, n rim vertices round it; open: n - 1 faces (the middle on the boundary), closed: n faces
    (the middle interior with n neighbours, the rim the boundary)"""
    t = 2.0 * np.pi * np.arange(n) / (n if closed else n + 3)
    rim = np.stack([np.cos(t), np.sin(t), 0.2 * np.sin(3.0 * t)], axis=1)
    pos = np.concatenate([[[0.0, 0.0, 0.5]], rim])
    idx = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n if closed else n - 1)], np.int32)
    return pos, idx


# the vertex counts after every level, verified by hand from V' = V + E, E' = 2 E + 3 F, F' = 4 F
COUNTS = {"octahedron": [18, 66, 258, 1026], "tetrahedron": [10, 34, 130, 514], "strip23": [66, 215, 765], "strip33": [96, 315, 1125],
          "open-fan7": [21, 65, 225], "closed-fan200": [601, 2001]}


def cases():
    """[(name, positions, indices, uvs or None, the levels to run)]"""
    out = []
    pos, idx = octahedron()
    out.append(("octahedron", pos * np.array([1.0, 0.8, 1.3]) + 0.1, idx, None, [1, 2, 3, 4]))
    pos, idx = tetrahedron()
    out.append(("tetrahedron", pos, idx, None, [1, 2, 3, 4]))
    for nv in (23, 33):
        pos, idx = strip(nv)
        out.append((f"strip{nv}", pos, idx, None, [1, 2, 3]))
    pos, idx = fan(7, False)
    out.append(("open-fan7", pos, idx, None, [1, 2, 3]))
    pos, idx = fan(200, True)
    out.append(("closed-fan200", pos, idx, None, [2]))
    pos, idx = strip(9)
    out.append(("strip9-unused-vertex", np.concatenate([pos, [[0.3, 2.0, -1.0]]]), idx, None, [2]))
    pos, idx = strip(23)
    flipped = idx.copy()
    flipped[7] = flipped[7][[1, 0, 2]]
    out.append(("strip23-flipped-face", pos, flipped, None, [1, 2]))
    pos, idx = strip(23)
    uv = np.stack([0.5 * (pos[:, 0] + 1.0), (np.arange(23) % 2) * 0.7 + 0.1], axis=1)
    out.append(("strip23-uvs", pos, idx, uv, [1, 2]))
    return out

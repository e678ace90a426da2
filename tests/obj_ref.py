"""obj_ref.py — TEST INFRASTRUCTURE: CPU restatement of the reference's OBJ loader, in numpy.

What it restates: `TriangleMesh parse_obj(filename, to_world)` (src/parse/parse_obj.cpp:118-203) for the scope of
take_hip_mesh_from_obj: lines split at '\\n' and trimmed with the "C" locale's isspace (bytes.strip / bytes.split use the
same six characters), `v x y z [w]` -> Vector3{x,y,z} / w (times 1 / w), `vt s t` -> (s, 1 - t), `vn x y z` ->
normalize(), `f` with 3 or 4 corners split as split_face_str splits them (pieces between '/', a trailing empty piece
dropped, "" -> 0, std::stoi on the rest), vertices deduplicated on the raw (v, vt, vn) triple in order of first use
(np.unique + first-index order), indices resolved against the pools as the face line finds them (negative vt: pool +
vt - 1, the reference's off-by-one), then xform_point(to_world) / xform_normal(inverse(to_world)).  numpy evaluates
a * b + c * d + ... left to right in IEEE double like the C++ does, so the arrays are bit-comparable.

Pinned by tests/golden/obj/* (the reference's own parser through oracle/_ref/ref_harness flatten,
tools/gen_obj_golden.py); the checker for files too large to commit.  The product decodes on the device
(take_amd/csrc/tk_obj.h).
"""
import re

import numpy as np

NUMBER = re.compile(rb"[+-]?(\d+(\.\d*)?|\.\d+)([eE][+-]?\d+)?")
STOI = re.compile(rb"[+-]?\d+")
TINY = 2.2250738585072014e-308

# error kinds, in the order the device reports two problems found on the same line
UNSUPPORTED, FEW, V0, RANGE, NGON = 1, 2, 3, 4, 5


class ObjError(ValueError):
    def __init__(self, code, line):
        super().__init__(f"line {line + 1}: code {code}")
        self.code, self.line = code, line

    @property
    def unsupported(self):
        return self.code == UNSUPPORTED


def real(tok):
    """`ss >> Real` on a whole token, or None where the device calls the file unsupported"""
    if not NUMBER.fullmatch(tok):
        return None
    x = float(tok)
    if x == float("inf") or x == -float("inf") or (abs(x) < TINY and re.search(rb"[1-9]", tok.split(b"e")[0].split(b"E")[0])):
        return None  # (strtod reports ERANGE: the stream fails on an overflow; underflow is refused too)
    return x


def stoi(piece):
    m = STOI.match(piece)
    if not m:
        return None
    v = int(m.group(0))
    return v if -2**31 <= v < 2**31 else None


def split_face(tok):
    """split_face_str -> [v, vt, vn] or None where std::stoi throws"""
    pieces = tok.split(b"/")
    if pieces[-1] == b"":
        pieces = pieces[:-1]
    out = []
    for p in pieces:
        v = 0 if p == b"" else stoi(p)
        if v is None:
            return None
        out.append(v)
    return (out + [0, 0, 0])[:3]


def line_kind(ln):
    """what parse_obj's loop makes of one line (without its '\\n') -> (kind, tokens): "v" / "vt" / "vn", "f3" / "f4" for a
    face of 3 / 4 corners, "fbad" for any other number of them, or None for a line it skips (blank, a comment, any other
    keyword)"""
    ln = ln.strip()
    if not ln or ln[:1] == b"#":
        return None, []
    tok = ln.split()
    kw = tok[0]
    if kw in (b"v", b"vt", b"vn"):
        return kw.decode(), tok
    if kw == b"f":
        return {3: "f3", 4: "f4"}.get(len(tok) - 1, "fbad"), tok
    return None, []


def xform_point(m, p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    tx = m[0, 0] * x + m[0, 1] * y + m[0, 2] * z + m[0, 3]
    ty = m[1, 0] * x + m[1, 1] * y + m[1, 2] * z + m[1, 3]
    tz = m[2, 0] * x + m[2, 1] * y + m[2, 2] * z + m[2, 3]
    tw = m[3, 0] * x + m[3, 1] * y + m[3, 2] * z + m[3, 3]
    inv_w = 1.0 / tw
    return np.stack([tx * inv_w, ty * inv_w, tz * inv_w], 1)


def normalize(n):
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        l = np.sqrt(x * x + y * y + z * z)
        inv = 1.0 / l
        out = np.stack([x * inv, y * inv, z * inv], 1)
    out[~(l > 0)] = 0.0
    return out


def xform_normal(mi, n):
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    return normalize(np.stack([mi[0, 0] * x + mi[1, 0] * y + mi[2, 0] * z, mi[0, 1] * x + mi[1, 1] * y + mi[2, 1] * z,
                               mi[0, 2] * x + mi[1, 2] * y + mi[2, 2] * z], 1))


def parse_obj(data, to_world=None, inv_to_world=None):
    """-> {"positions", "indices", "normals", "uvs"} (None for an empty normals / uvs array), or raises ObjError with
    the earliest line that has a problem (ObjError.unsupported: the caller keeps the host parser)"""
    X = np.eye(4) if to_world is None else np.asarray(to_world, np.float64).reshape(4, 4)
    Xi = np.eye(4) if inv_to_world is None else np.asarray(inv_to_world, np.float64).reshape(4, 4)
    vraw, traw, nraw = [], [], []
    keys, pools, lines, ncorner = [], [], [], []
    err = None  # (line, code)

    def bad(line, code):
        nonlocal err
        if err is None or (line, code) < err:
            err = (line, code)

    for i, ln in enumerate(bytes(data).split(b"\n")):
        kind, tok = line_kind(ln)
        if kind is None:
            continue
        kw = tok[0]
        if kw in (b"v", b"vt", b"vn"):
            need = 2 if kw == b"vt" else 3
            want = tok[1:5] if kw == b"v" else tok[1:1 + need]
            vals = [real(t) for t in want]
            if len(vals) < need or any(v is None for v in vals):
                bad(i, UNSUPPORTED)
                vals = [0.0] * need
            if kw == b"v":
                vraw.append(vals + [1.0] if len(vals) == 3 else vals)
            else:
                (traw if kw == b"vt" else nraw).append(vals[:need])
        elif kw == b"f":
            corners = [split_face(t) for t in tok[1:5]]
            if any(c is None for c in corners):
                bad(i, UNSUPPORTED)
            n = len(tok) - 1
            if n < 3 or n > 4:
                bad(i, FEW if n < 3 else NGON)
                continue
            keys += [c or [0, 0, 0] for c in corners]
            pools.append((len(vraw), len(traw), len(nraw)))
            lines.append(i)
            ncorner.append(n)
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    nc = np.asarray(ncorner, np.int64)
    face_of = np.repeat(np.arange(len(nc)), nc)
    pools = np.asarray(pools, np.int64).reshape(-1, 3)
    lines = np.asarray(lines, np.int64)
    # dedup on the raw triple, ids in order of first occurrence
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    vid = rank[inverse]
    fc = first[order]  # the first corner of each vertex, in id order
    k, f = keys[fc], face_of[fc]
    nv, nvt, nvn = pools[f, 0], pools[f, 1], pools[f, 2]
    iv = np.where(k[:, 0] > 0, k[:, 0] - 1, nv + k[:, 0])
    it = np.where(k[:, 1] > 0, k[:, 1] - 1, nvt + k[:, 1] - 1)
    inn = np.where(k[:, 2] > 0, k[:, 2] - 1, nvn + k[:, 2])
    v0 = k[:, 0] == 0
    rng = (iv < 0) | (iv >= nv) | ((k[:, 1] != 0) & ((it < 0) | (it >= nvt))) | ((k[:, 2] != 0) & ((inn < 0) | (inn >= nvn)))
    for sel, code in ((v0, V0), (rng & ~v0, RANGE)):
        if sel.any():
            bad(int(lines[f[sel]].min()), code)
    if err is not None:
        raise ObjError(err[1], err[0])
    vraw = np.asarray(vraw, np.float64).reshape(-1, 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_w = 1.0 / vraw[:, 3]
    pos_pool = vraw[:, :3] * inv_w[:, None]
    positions = xform_point(X, pos_pool[iv]) if len(iv) else np.zeros((0, 3))
    starts = np.concatenate([[0], np.cumsum(nc)[:-1]]) if len(nc) else np.zeros(0, np.int64)
    t1 = np.stack([vid[starts], vid[starts + 1], vid[starts + 2]], 1) if len(nc) else np.zeros((0, 3), np.int64)
    q = starts[nc == 4]
    t2 = np.stack([vid[q], vid[q + 2], vid[q + 3]], 1)
    # triangles in face order, a quad's second right behind its first
    tri = np.zeros((len(nc) + len(q), 3), np.int64)
    slot = np.arange(len(nc)) + np.concatenate([[0], np.cumsum(nc == 4)[:-1]]) if len(nc) else np.zeros(0, np.int64)
    tri[slot] = t1
    tri[slot[nc == 4] + 1] = t2
    has_t, has_n = k[:, 1] != 0, k[:, 2] != 0
    if has_t.any() and not has_t.all():
        raise ObjError(UNSUPPORTED, -1)
    if has_n.any() and not has_n.all():
        raise ObjError(UNSUPPORTED, -1)
    uvs = normals = None
    if has_t.any():
        traw = np.asarray(traw, np.float64).reshape(-1, 2)
        uvs = np.stack([traw[it, 0], 1.0 - traw[it, 1]], 1)
    if has_n.any():
        nraw = np.asarray(nraw, np.float64).reshape(-1, 3)
        normals = xform_normal(Xi, normalize(nraw)[inn])
    return {"positions": positions, "indices": tri.astype(np.int32), "normals": normals, "uvs": uvs}

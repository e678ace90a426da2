"""tests/golden/obj/: Wavefront OBJ files, their to_world matrices, and the TriangleMesh arrays the reference's own
parse_obj (src/parse/parse_obj.cpp:118-203) makes of them — what take_hip_mesh_from_obj must reproduce bit for bit.

    python tools/gen_obj_golden.py [--out DIR]      (needs oracle/_ref/ref_harness: __graft_entry__.build())

Per case: <case>.obj, <case>_xform.f64 (to_world, 16 doubles row-major) and <case>_mesh.f64 in the layout
tests/test_ply_cpu.py::load_case reads (nv nf has_normals has_uvs, inverse(to_world), positions, indices, normals,
uvs).  The arrays come from the reference through the existing harness commands:
  - `ref_harness flatten` on a one-shape XML (<shape type="obj">, to_world as a <matrix>, the OBJ by absolute path)
    -> the flattened scene's mesh.  Cases without `vn` set faceNormals=true, or parse_scene would put compute_normals
    in place of the (empty) normals parse_obj made.
  - `ref_harness ply` on a one-triangle PLY with the same to_world -> the reference's inverse(to_world) at out[4:20],
    the matrix parse_obj pushes the normals through.
Matrix entries are float-representable: parse_matrix4x4 reads them with std::stof.  Writes only under the output
directory (default tests/golden/obj/); tests/golden/manifest.json is not touched.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import obj_tokens  # noqa: E402  (the token lists of the number_grammar case)
from oracle.gen_golden import HARNESS, run, write_ply  # noqa: E402
from take_amd.scene import load_tkscene  # noqa: E402

I4 = np.eye(4)
AFFINE = np.array([[0.5, -0.75, 0.25, 1.5], [0.75, 0.5, 0.0, -2.0], [0.125, 0.25, 2.0, 0.375], [0.0, 0.0, 0.0, 1.0]])
PROJECTIVE = np.array([[1.25, 0.0, 0.5, 0.25], [0.0, 0.75, 0.0, -0.5], [0.25, 0.125, 1.0, 2.0], [0.0625, 0.125, 0.03125, 1.0]])


def grid(nx, ny, seed):
    rng = np.random.default_rng(seed)
    return [(x * 0.5 - 1 + rng.uniform(-0.1, 0.1), y * 0.5 - 1 + rng.uniform(-0.1, 0.1), rng.uniform(-0.3, 0.3))
            for y in range(ny) for x in range(nx)]


def cases():
    """name -> (obj text, to_world, has vn)"""
    out = {}
    # 1. triangles with full v/vt/vn corners, identity
    p = grid(4, 4, 1)
    lines = ["# triangles, v/vt/vn"] + [f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in p]
    lines += [f"vt {(k % 4) / 3:.6f} {(k // 4) / 3:.6f}" for k in range(16)]
    lines += [f"vn {0.1 * (k % 3):.6f} {0.2 - 0.05 * k:.6f} 1.000000" for k in range(16)]
    for y in range(3):
        for x in range(3):
            a, b, c, d = 4 * y + x + 1, 4 * y + x + 2, 4 * y + x + 6, 4 * y + x + 5
            lines += [f"f {a}/{a}/{a} {b}/{b}/{b} {c}/{c}/{c}", f"f {a}/{a}/{a} {c}/{c}/{c} {d}/{d}/{d}"]
    out["tri_full_identity"] = ("\n".join(lines) + "\n", I4, True)
    # 2. quads in v//vn form, affine
    p = grid(3, 3, 2)
    lines = [f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in p] + ["vn 0 0 1", "vn 0.000000 0.707107 0.707107", "vn 1 0 0"]
    for y in range(2):
        for x in range(2):
            a, b, c, d = 3 * y + x + 1, 3 * y + x + 2, 3 * y + x + 5, 3 * y + x + 4
            n = (x + y) % 3 + 1
            lines.append(f"f {a}//{n} {b}//{n} {c}//{n} {d}//{n}")
    out["quad_vn_affine"] = ("\n".join(lines) + "\n", AFFINE, True)
    # 3. negative indices between later v lines: (-1) read at two pool sizes is one vertex (its first data), 4 and -1
    #    naming the same position are two
    out["negative_interleaved"] = ("\n".join([
        "v 0 0 0", "v 1 0 0", "v 0 1 0",
        "f -3 -2 -1",
        "v 1 1 0", "v 2 1 0.5",
        "f -3 -2 -1",
        "f 4 5 -1",
        "v -1 2 0.25",
        "f 1 -1 -3 6",
        "f -4 4 -1",
    ]) + "\n", AFFINE, False)
    # 4. homogeneous v x y z w, v with six numbers (the fourth is w, the rest never read), projective to_world
    out["homogeneous_projective"] = ("\n".join([
        "v 0 0 0 1", "v 2 0 0 2", "v 0 3 0 0.5", "v 1 1 1 4",
        "v 0.5 0.25 0.125 0.75 0.1 0.2", "v -1 0.5 2 1.0 0.9 0.8",
        "f 1 2 3", "f 1 3 4 5", "f 6 5 4",
    ]) + "\n", PROJECTIVE, False)
    # 5. whitespace and number formats: CRLF, tabs, leading blanks, comments, ignored keywords, no final newline,
    #    1. / .5 / -0.0 / +2E+2, and 17-digit numbers (the host's strtod converts those)
    out["whitespace_formats"] = ("\r\n".join([
        "# comment line", "mtllib scene.mtl", "o object_1", "g group_a", "s 1", "usemtl white",
        "   v\t1.\t.5 -0.0", "\tv  +2E+2 0.1000000000000000055511151231257827 -3.0000000000000004  ",
        "v 0.30000000000000004 1e-3 2.5e1\t", "vp 0.5 0.5", "   ", "",
        "vt -0.0 1.", "vt .25 0.33333333333333331", "vt 1e0 +0.5",
        "vn 0 0 1.", "vn 0.57735026918962573 0.57735026918962573 0.57735026918962573", "vn -1 0 0",
        "l 1 2", "# f 9 9 9", "\tf 1/1/1\t2/2/2   3/3/3  ", "f\t3/3/3 2/2/2 1/1/3",
    ]), I4, True)
    # 6. negative vt (resolves to pool + vt - 1) and negative vn
    out["negative_vt_vn"] = ("\n".join([
        "v 0 0 0", "v 1 0 0", "v 0 1 0", "v 1 1 0",
        "vt 0.1 0.2", "vt 0.3 0.4", "vt 0.5 0.6", "vt 0.7 0.8",
        "vn 0 0 1", "vn 0 1 0", "vn 1 0 0",
        "f 1/-1/-1 2/-2/-2 3/-3/-3",
        "f 2/1/1 4/-1/-3 3/2/-1",
    ]) + "\n", AFFINE, True)
    # 7. vt only
    p = grid(3, 2, 3)
    lines = [f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in p] + [f"vt {k / 5:.6f} {1 - k / 7:.6f}" for k in range(6)]
    lines += ["f 1/1 2/2 5/5", "f 1/1 5/5 4/4", "f 2/2 3/3 6/6 5/5"]
    out["vt_only"] = ("\n".join(lines) + "\n", AFFINE, False)
    # 8. a zero-length vn (normalize() -> (0, 0, 0))
    out["zero_vn"] = ("\n".join([
        "v 0 0 0", "v 1 0 0", "v 0 1 0", "v 1 1 1",
        "vn 0 0 0", "vn 0 0 2", "vn 0.0 -0.0 0.0",
        "f 1//1 2//2 3//1", "f 2//3 4//2 3//2",
    ]) + "\n", AFFINE, True)
    # 9. `1/` and `1//` corners (split_face_str: a trailing empty piece dropped, "" -> 0), a piece std::stoi reads the
    #    leading integer of, and a fourth piece that is converted but not kept
    out["slash_forms"] = ("\n".join([
        "v 0 0 0", "v 1 0 0", "v 0 1 0", "v 1 1 0",
        "f 1/ 2// 3",
        "f 2 4x 3/",
        "f 1// 2/ 4",
        "f 4/// +3 2//",
    ]) + "\n", I4, False)
    # 10. the number grammar at the edges of the window in which the device converts a number itself (15 / 16
    #     significant digits, effective exponent 22 / 23, zero runs, signed zeros, the ends of the double range): the
    #     curated tokens and a fixed slice of the generated ones (oracle/obj_tokens.py), every one as a vt's first
    #     coordinate (the decode leaves it untouched: signed zeros are visible), as a v coordinate and as a vn coordinate;
    #     a few v lines carry a w.  Identity to_world; the faces use every vertex.
    toks = [t.decode() for t in obj_tokens.CURATED + obj_tokens.number_tokens(180 - len(obj_tokens.CURATED))]
    n = len(toks)
    mild = [t for t in toks if 1e-3 <= abs(float(t)) <= 1e3]
    v = [f"v {toks[i]} {toks[(i + 1) % n]} {toks[(i + 2) % n]}" for i in range(n)]
    v += [f"v {mild[i]} {mild[i + 1]} {mild[i + 2]} {mild[i + 3]}" for i in range(12)]
    m = len(v)
    vt = [f"vt {toks[i % n]} {toks[(i + 5) % n]}" for i in range(m)]
    vn = [f"vn {toks[(i + 3) % n]} {toks[(i + 4) % n]} {toks[(i + 7) % n]}" for i in range(m)]
    faces = ["f " + " ".join(f"{j % m + 1}/{j % m + 1}/{j % m + 1}" for j in (i, i + 1, i + 2)) for i in range(0, m, 3)]
    out["number_grammar"] = ("\n".join(["# number grammar"] + v + vt + vn + faces) + "\n", I4, True)
    return out


def flatten_mesh(obj_path, xf, face_normals, tmp):
    mat = " ".join(repr(float(np.float32(v))) for v in xf.reshape(-1))
    xml = os.path.join(tmp, "scene.xml")
    with open(xml, "w") as f:
        f.write('<scene version="0.5.0">\n'
                '  <sensor type="perspective"><float name="fov" value="39"/>\n'
                '    <transform name="toWorld"><lookat origin="0,0,5" target="0,0,0" up="0,1,0"/></transform>\n'
                '    <film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/></film></sensor>\n'
                '  <bsdf type="diffuse" id="white"><rgb name="reflectance" value="0.5 0.5 0.5"/></bsdf>\n'
                f'  <shape type="obj"><string name="filename" value="{os.path.abspath(obj_path)}"/>'
                f'<transform name="toWorld"><matrix value="{mat}"/></transform>'
                + ('<boolean name="faceNormals" value="true"/>' if face_normals else "")
                + '<ref id="white"/></shape>\n</scene>\n')
    out = os.path.join(tmp, "scene.tkscene")
    run("flatten", xml, out)
    sd = load_tkscene(out)
    assert len(sd.meshes) == 1
    return sd.meshes[0]


def reference_inverse(xf, tmp):
    ply = os.path.join(tmp, "tri.ply")
    write_ply(ply, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    xin, xout = os.path.join(tmp, "xf.f64"), os.path.join(tmp, "tri.f64")
    xf.astype("<f8").tofile(xin)
    run("ply", ply, xin, xout)
    return np.fromfile(xout, "<f8")[4:20]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "obj"))
    a = ap.parse_args()
    if not os.path.exists(HARNESS):
        raise SystemExit(f"{HARNESS} not built")
    os.makedirs(a.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, (text, xf, has_vn) in cases().items():
            xf = xf.astype(np.float32).astype(np.float64)
            path = os.path.join(a.out, name + ".obj")
            with open(path, "wb") as f:
                f.write(text.encode())
            m = flatten_mesh(path, xf, not has_vn, tmp)
            inv = reference_inverse(xf, tmp)
            nv, nf = len(m.positions), len(m.indices)
            hn, hu = int(m.normals is not None and len(m.normals) > 0), int(m.uvs is not None and len(m.uvs) > 0)
            parts = [np.array([nv, nf, hn, hu], np.float64), inv, m.positions.reshape(-1), m.indices.reshape(-1).astype(np.float64)]
            if hn:
                parts.append(m.normals.reshape(-1))
            if hu:
                parts.append(m.uvs.reshape(-1))
            xf.astype("<f8").tofile(os.path.join(a.out, name + "_xform.f64"))
            np.concatenate(parts).astype("<f8").tofile(os.path.join(a.out, name + "_mesh.f64"))
            print(f"obj/{name}: {nv} vertices, {nf} triangles, normals {hn}, uvs {hu}")


if __name__ == "__main__":
    main()

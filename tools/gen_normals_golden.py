"""tests/golden/normals/: meshes and the vertex normals the reference's own compute_normals
(src/compute_normals.cpp:12-47) gives them — what take_hip_compute_normals must reproduce.

    python tools/gen_normals_golden.py [--out DIR]      (needs oracle/_ref/ref_harness: __graft_entry__.build())

Per case one binary PLY without normals, in a one-shape XML scene without faceNormals, goes through
`ref_harness flatten`: parse_scene then calls compute_normals(mesh.positions, mesh.indices), and the flattened mesh's
normals are its output.  <case>_mesh.f64 holds nv, nf, then the reference's positions (the PLY's floats widened),
indices and normals, all as doubles.  Writes only under the output directory (default tests/golden/normals/);
tests/golden/manifest.json is not touched.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import HARNESS, run, write_ply  # noqa: E402
from take_amd.scene import load_tkscene  # noqa: E402


def icosphere(subdiv):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid = {}

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        f = [g for a, b, c in f for g in ((a, m(a, b), m(a, c)), (b, m(b, c), m(a, b)), (c, m(a, c), m(b, c)), (m(a, b), m(b, c), m(a, c)))]
    return np.array(v) * 0.8, np.array(f)


def grid(nx, ny, sx, sy, jitter, z, seed):
    rng = np.random.default_rng(seed)
    p = [(x * sx + rng.uniform(-jitter, jitter) * sx, y * sy + rng.uniform(-jitter, jitter) * sy, z(x, y, rng))
         for y in range(ny) for x in range(nx)]
    f = []
    for y in range(ny - 1):
        for x in range(nx - 1):
            a, b, c, d = y * nx + x, y * nx + x + 1, (y + 1) * nx + x + 1, (y + 1) * nx + x
            f += [(a, b, c), (a, c, d)] if (x + y) % 2 == 0 else [(a, b, d), (b, c, d)]
    return np.array(p), np.array(f)


def cases():
    """name -> (positions, faces)"""
    out = {}
    out["closed"] = icosphere(1)
    # long thin cells, strongly jittered: many corners over 90 degrees (the dot < 0 branch of unit_angle)
    out["obtuse"] = grid(7, 6, 1.0, 0.25, 0.35, lambda x, y, r: r.uniform(-0.2, 0.2), 2)
    # z = 0 with both windings: face normals (+-0, +-0, +-1), x / y sums of signed zeros
    p, f = grid(5, 5, 0.5, 0.5, 0.2, lambda x, y, r: 0.0, 3)
    f[::3] = f[::3, ::-1]
    out["planar"] = (p, f)
    # zero-area faces: collinear, coincident positions at distinct indices, a repeated index; next to ordinary faces
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 2, 1], [0.5, 0.5, 0.25], [1, 0, 0], [1, 0, 0],
                  [0.25, -1, 0.125], [-1, 0.5, 0.75]], float)
    f = np.array([[0, 1, 2], [1, 3, 2], [0, 3, 4],  # (0, 3, 4): (1, 1, 0.5) and (2, 2, 1) on one line through 0
                  [6, 7, 1],                         # three distinct indices, one position
                  [2, 2, 3],                         # a repeated index
                  [0, 8, 1], [9, 0, 2], [5, 3, 1]])
    out["degenerate"] = (p, f)
    p = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, 0.5], [3, 3, 3], [1, 1, -0.25]], float)
    out["unreferenced"] = (p, np.array([[0, 1, 2], [1, 4, 2]]))  # vertex 3: no face
    p = np.array([[0, 0, 0], [1, 0.25, 0], [0.25, 1, 0.5], [1.5, 1.25, -0.5]], float)
    out["cancelling"] = (p, np.array([[0, 1, 2], [0, 2, 1], [1, 3, 2]]))  # (0, 1, 2) both ways: vertex 0 sums to 0
    # a wavy fan: one centre shared by 2000 faces
    n = 2000
    a = np.arange(n) * (2 * np.pi / n)
    rim = np.stack([np.cos(a), np.sin(a), 0.3 * np.sin(7 * a)], axis=1) * (1 + 0.1 * np.cos(13 * a))[:, None]
    p = np.concatenate([[[0.0, 0.0, 0.4]], rim])
    out["fan"] = (p, np.array([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)]))
    return out


def flatten_mesh(ply_path, tmp):
    xml = os.path.join(tmp, "scene.xml")
    with open(xml, "w") as f:
        f.write('<scene version="0.5.0">\n'
                '  <sensor type="perspective"><float name="fov" value="39"/>\n'
                '    <transform name="toWorld"><lookat origin="0,0,5" target="0,0,0" up="0,1,0"/></transform>\n'
                '    <film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/></film></sensor>\n'
                '  <bsdf type="diffuse" id="white"><rgb name="reflectance" value="0.5 0.5 0.5"/></bsdf>\n'
                f'  <shape type="ply"><string name="filename" value="{os.path.abspath(ply_path)}"/><ref id="white"/></shape>\n'
                '</scene>\n')
    out = os.path.join(tmp, "scene.tkscene")
    run("flatten", xml, out)
    sd = load_tkscene(out)
    assert len(sd.meshes) == 1
    return sd.meshes[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "normals"))
    a = ap.parse_args()
    if not os.path.exists(HARNESS):
        raise SystemExit(f"{HARNESS} not built")
    os.makedirs(a.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for name, (p, f) in cases().items():
            ply = os.path.join(tmp, name + ".ply")
            write_ply(ply, p, f)
            m = flatten_mesh(ply, tmp)
            assert np.array_equal(m.positions, np.asarray(p, np.float32).astype(np.float64)) and np.array_equal(m.indices, f)
            assert m.normals is not None and m.normals.shape == m.positions.shape
            nv, nf = len(m.positions), len(m.indices)
            parts = [np.array([nv, nf], np.float64), m.positions.reshape(-1), m.indices.reshape(-1).astype(np.float64),
                     m.normals.reshape(-1)]
            np.concatenate(parts).astype("<f8").tofile(os.path.join(a.out, name + "_mesh.f64"))
            print(f"normals/{name}: {nv} vertices, {nf} triangles")


if __name__ == "__main__":
    main()

"""What displacement mapping costs on the device (take_hip_displace_apply_device, take_hip_scene_displace_meshes).

1. Kernel time, by the library's own events (TAKE_HIP_VERBOSE=1): tools/subdiv_time.py's bent grid of `--quads`^2 quads
   (88) at `--levels` levels (3: 497 025 vertices) under a `--texels`^2 float height map (1024); k_displace and the two
   normal launches behind it, the median over `--reps` calls after a warm-up, against the algorithmic bytes of each —
   every table entry, gathered record and written result counted once — as GB/s; beside each a device-to-device copy
   that moves the same number of bytes (read + written), timed in the same session: the ceiling.
2. The whole call: the median wall time of `--reps` Scene.displace_meshes calls with a subdivision binding after a
   warm-up on a scene of the refined grid, its split into refine, displace and update, and the only route there was
   before: Subdiv.refine to the host, the lookup and the normals in numpy (cells and fractions made once, as the handle
   makes them once), then update_meshes with host arrays.

`--baseline-only` runs that route alone; it uses nothing of the displacement API.

    python tools/displace_time.py [--reps 20] [--quads 88] [--levels 3] [--texels 1024] [--precisions f32,mixed] [--baseline-only | --kernel-only] [--out FILE]
"""
import argparse
import os
import re
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from subdiv_time import bent_grid, copy_ms, scatter, timed  # noqa: E402
from take_amd import capi  # noqa: E402
from take_amd import cdefs as D  # noqa: E402
from take_amd.scene import Light, SceneData  # noqa: E402

SCALE, BIAS = 0.03, 0.0


def verbose_lines(f):
    """the lines the library prints to stderr about a displacement for one call under TAKE_HIP_VERBOSE=1"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.environ["TAKE_HIP_VERBOSE"] = "1"
        try:
            os.dup2(tmp.fileno(), 2)
            f()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["TAKE_HIP_VERBOSE"]
        tmp.seek(0)
        return [line.strip() for line in tmp.read().decode(errors="replace").splitlines() if "displace_apply:" in line]


def height_map(n):
    """an n x n float32 height map in [-1, 1] that tiles"""
    g = 2.0 * np.pi * np.arange(n) / n
    y, x = np.meshgrid(g, g, indexing="ij")
    return (0.5 * np.sin(3.0 * x) * np.cos(5.0 * y) + 0.3 * np.sin(17.0 * x + 2.0 * y) + 0.2 * np.cos(41.0 * y - 7.0 * x)).astype(np.float32)


# ---- the host route: the lookup and the normals in vectorised numpy, as a user of update_meshes wrote them before
def numpy_cells(uv, width, height):
    """what depends on the uvs alone: made once per mesh, like the handle's lookup coordinates"""
    a, b = np.mod(uv[:, 0], 1.0), np.mod(uv[:, 1], 1.0)
    x, y = width * a, height * b
    x1, y1 = np.minimum(np.floor(x).astype(np.int64), width - 1), np.minimum(np.floor(y).astype(np.int64), height - 1)
    return x1, (x1 + 1) % width, y1, (y1 + 1) % height, x - x1, y - y1


def numpy_displace(p, n, faces, cells, image, scale, bias):
    x1, x2, y1, y2, fx, fy = cells
    h = (image[y1, x1] * (1.0 - fx) + image[y1, x2] * fx) * (1.0 - fy) + (image[y2, x1] * (1.0 - fx) + image[y2, x2] * fx) * fy
    q = p + (scale * h + bias)[:, None] * n
    fn = np.cross(q[faces[:, 1]] - q[faces[:, 0]], q[faces[:, 2]] - q[faces[:, 0]])
    m = scatter(faces[:, 0], fn, q.shape[0]) + scatter(faces[:, 1], fn, q.shape[0]) + scatter(faces[:, 2], fn, q.shape[0])
    return q, m / np.maximum(np.linalg.norm(m, axis=1, keepdims=True), 1e-300)


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quads", type=int, default=88)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--texels", type=int, default=1024)
    ap.add_argument("--precisions", default="f32,mixed")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="part 1 alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps, L = args.reps, args.levels
    rows = []

    def row(text):
        rows.append(text)
        print(text, flush=True)

    def wall(what, stats):
        row(f"{what:<92s} median {stats[0]:10.3f} ms   (min {stats[1]:.3f}, max {stats[2]:.3f}; {reps} calls)")

    cage, idx = bent_grid(args.quads)
    cage_uv = np.stack([2.0 * (cage[:, 0] + 1.0), 2.0 * (cage[:, 2] + 1.0)], axis=1)  # (the map tiles four times each way)
    image = height_map(args.texels)
    cages = [cage + 0.02 * np.sin(5.0 * cage[:, [2, 0, 1]] + k) for k in range(4)]
    sub = capi.Subdiv(idx, cage.shape[0], L, uvs=cage_uv)
    faces, uv = sub.topology()
    nv, nf = sub.n_vertices, sub.n_faces
    row(f"cage: {cage.shape[0]} vertices, {idx.shape[0]} faces; {L} levels: {nv} vertices, {nf} faces; height map {args.texels} x {args.texels} float32")
    base_p, base_n = (torch.zeros((nv, 3), dtype=torch.float64, device="cuda") for _ in range(2))
    out_p, out_n = (torch.zeros((nv, 3), dtype=torch.float64, device="cuda") for _ in range(2))
    sub.refine_device(base_p, base_n, cages[0])

    # ---- 1. the kernels
    if not args.baseline_only:
        with capi.Displace(faces, nv, uv, image) as dis:
            dis.apply_device(out_p, out_n, base_p, base_n, SCALE, BIAS)
            ms = {}
            for _ in range(reps):
                for line in verbose_lines(lambda: dis.apply_device(out_p, out_n, base_p, base_n, SCALE, BIAS)):
                    m = re.search(r"displace_apply: (\w+) (k_[\w<>]+) .* ([0-9.]+) ms$", line)
                    if m:
                        ms.setdefault((m.group(1), m.group(2)), []).append(float(m.group(3)))
            # algorithmic bytes: k_displace 16 (a, b) + 24 position + 24 normal + 4 texels of 4 bytes + 24 out; face normals
            # 12 + 72 + 24; vertex normals 4 row start + (4 index + 24 normal) per face of the row + 24 out
            passes = [("positions", "k_displace<float>", nv * (16 + 24 + 24 + 4 * 4 + 24)), ("normals", "k_subdiv_face_normals", nf * (12 + 72 + 24)),
                      ("normals", "k_subdiv_vertex_normals", nv * (4 + 24) + 3 * nf * (4 + 24))]
            total = 0.0
            for what, kernel, nbytes in passes:
                t = ms[(what, kernel)]
                med = statistics.median(t)
                total += med
                half = max(nbytes // 2 // 8, 1)
                src, dst = torch.zeros(half, dtype=torch.float64, device="cuda"), torch.zeros(half, dtype=torch.float64, device="cuda")
                copy = copy_ms(dst, src, reps)
                row(f"  {what} {kernel}: median {med:.4f} ms (min {min(t):.4f}, max {max(t):.4f}; {reps} calls), {nbytes / 1e6:.2f} MB, {nbytes / nv:.0f} B/vertex -> "
                    f"{nbytes / med / 1e6:.0f} GB/s; a device-to-device copy moving the same bytes (read + written; device events round 10 copies, a tenth of it): "
                    f"{copy[0]:.4f} ms -> {nbytes / copy[0] / 1e6:.0f} GB/s")
                del src, dst
            row(f"the three launches: {total:.4f} ms")
            wall(f"apply_device, {nv} vertices, device arrays, normals given, with normals out", timed(lambda: dis.apply_device(out_p, out_n, base_p, base_n, SCALE, BIAS), reps))
            wall(f"apply_device, {nv} vertices, device arrays, own normals, with normals out", timed(lambda: dis.apply_device(out_p, out_n, base_p, None, SCALE, BIAS), reps))
            wall(f"apply_device, {nv} vertices, device arrays, normals given, positions alone", timed(lambda: dis.apply_device(out_p, None, base_p, base_n, SCALE, BIAS), reps))
            row(f"the handle holds {dis.info()['device_bytes'] / 1e6:.1f} MB")

    # ---- 2. the whole call
    names = [] if args.kernel_only else args.precisions.split(",")
    if names:
        p0, n0 = sub.refine(cage)
        sd = SceneData(width=256, height=256, lookfrom=(0.0, 1.5, 3.0), lookat=(0.0, -0.3, 0.0), up=(0.0, 1.0, 0.0), vfov=45.0, background=(0.2, 0.3, 0.4), spp=4, max_depth=6)
        grey = sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7))
        sd.add_mesh(p0, faces, grey, normals=n0, uvs=uv)
        sd.add_sphere((0.0, 0.4, 0.0), 0.25, grey)
        sd.lights.append(Light(0, -1, (12.0, 12.0, 12.0), (0.3, 2.0, 1.5)))
        cells = numpy_cells(uv, args.texels, args.texels)
        faces64, image64 = faces.astype(np.int64), image.astype(np.float64)
    for name in names:
        precision = {"f32": D.TAKE_PRECISION_F32, "f64": D.TAKE_PRECISION_F64, "mixed": D.TAKE_PRECISION_MIXED}[name]
        tag = f"{nf}-face refined grid, {name}"
        sc = capi.Scene(sd, precision=precision)
        state = {"k": 0}

        def next_cage():
            state["k"] += 1
            return cages[state["k"] % len(cages)]

        try:
            made = {}

            def host_route():
                made["refined"] = sub.refine(next_cage())
                made["pn"] = numpy_displace(*made["refined"], faces64, cells, image64, SCALE, BIAS)
                sc.update_meshes({0: made["pn"]})

            wall(f"{tag}: refine to the host + numpy lookup and normals + update_meshes(host arrays)", timed(host_route, reps))
            wall(f"{tag}:   of it, Subdiv.refine to the host", timed(lambda: sub.refine(next_cage()), reps))
            wall(f"{tag}:   of it, numpy lookup and normals", timed(lambda: numpy_displace(*made["refined"], faces64, cells, image64, SCALE, BIAS), reps))
            wall(f"{tag}:   of it, update_meshes(host arrays)", timed(lambda: sc.update_meshes({0: made["pn"]}), reps))
            if not args.baseline_only:
                with capi.Displace(faces, nv, uv, image) as dis:
                    wall(f"{tag}: displace_meshes with a subdivision binding", timed(lambda: sc.displace_meshes([(0, dis, (sub, next_cage()), SCALE, BIAS)]), reps))
                    wall(f"{tag}:   refine alone (Subdiv.refine_device)", timed(lambda: sub.refine_device(base_p, base_n, next_cage()), reps))
                    wall(f"{tag}:   displace alone (Displace.apply_device over the refined device arrays)",
                         timed(lambda: dis.apply_device(out_p, out_n, base_p, base_n, SCALE, BIAS), reps))
                    wall(f"{tag}:   update alone (update_meshes over the displaced device arrays)", timed(lambda: sc.update_meshes({0: (out_p, out_n)}), reps))
        finally:
            sc.close()
    sub.close()
    text = "\n".join([f"displace_time.py --reps {reps} --quads {args.quads} --levels {L} --texels {args.texels} --precisions {args.precisions}"
                      f"{' --baseline-only' if args.baseline_only else ''}{' --kernel-only' if args.kernel_only else ''}   ({torch.cuda.get_device_name(0)})", ""] + rows) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

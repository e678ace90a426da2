"""What Loop subdivision costs on the device (take_hip_subdiv_refine_device, take_hip_scene_subdivide_meshes).

1. Kernel time, by the library's own events (TAKE_HIP_VERBOSE=1): a bent grid of `--quads`^2 quads (88: 15488 faces) at
   `--levels` levels (3: 991k refined faces); per level (even + odd launch) and for the normal pass (face + vertex launch)
   the median over `--reps` refines after a warm-up, against the algorithmic bytes of the pass — every table entry,
   gathered position and written result counted once — per output vertex and as GB/s; beside each a device-to-device
   copy that moves the same number of bytes (read + written), timed in the same session: the ceiling.
2. The whole call: the median wall time of `--reps` Scene.subdivide_meshes calls after a warm-up on a scene of the
   refined grid, its split into refine and update, and the only route there was before: the same refinement in numpy
   on the host (stencil tables made once, as the handle makes them once), then update_meshes with host arrays.

`--baseline-only` runs the numpy route alone; it needs nothing of the subdivision API — the topology below is the
tool's own numpy —, so a copy of this file in the tools/ of a checkout of an earlier commit measures that commit.

    python tools/subdiv_time.py [--reps 20] [--quads 88] [--levels 3] [--precisions f32,mixed] [--baseline-only | --kernel-only] [--out FILE]
"""
import argparse
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from take_amd import capi  # noqa: E402
from take_amd import cdefs as D  # noqa: E402
from take_amd.scene import Light, SceneData  # noqa: E402


def timed(f, reps):
    """one warm-up call, then the wall times of `reps` calls in ms -> (median, min, max)"""
    import torch

    f()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), max(ms)


def copy_ms(dst, src, reps):
    """a device-to-device copy between events on the stream it runs on, ten copies per window so that the window is the
    copies and not its ends: one warm-up, then `reps` windows -> ms per copy (median, min, max)"""
    import torch

    dst.copy_(src)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            dst.copy_(src)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / 10)
    return statistics.median(ms), min(ms), max(ms)


def verbose_lines(f):
    """the lines the library prints to stderr for one call under TAKE_HIP_VERBOSE=1"""
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
        return [line.strip() for line in tmp.read().decode(errors="replace").splitlines() if "subdiv_refine:" in line]


def bent_grid(n):
    """an n x n grid of quads, two faces each, bent out of its plane"""
    g = np.linspace(-1.0, 1.0, n + 1)
    x, z = np.meshgrid(g, g, indexing="ij")
    pos = np.stack([x.ravel(), 0.15 * np.sin(3.0 * x.ravel()) * np.cos(2.0 * z.ravel()) - 0.3, z.ravel()], axis=1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel()
    idx = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)]).astype(np.int32)
    return pos, idx


# ---- the host route: Loop subdivision in vectorised numpy, as a user of update_meshes wrote it before.  The topology
# below restates tests/subdiv_ref.py's on purpose: --baseline-only must run from a copy of this one file in a checkout of
# an earlier commit, which has no tests/subdiv_ref.py.
def level_tables(idx, V):
    """the stencil tables of one level and the refined faces: made once per cage, like the handle's"""
    idx = idx.astype(np.int64)
    F = idx.shape[0]
    a, b, opp = idx[:, [0, 1, 2]].ravel(), idx[:, [1, 2, 0]].ravel(), idx[:, [2, 0, 1]].ravel()
    key = np.minimum(a, b) * V + np.maximum(a, b)
    order = np.lexsort((np.repeat(np.arange(F), 3), key))
    ks = key[order]
    new = np.concatenate([[True], ks[1:] != ks[:-1]])
    first = np.flatnonzero(new)
    count = np.diff(np.concatenate([first, [len(ks)]]))
    lo, hi = ks[first] // V, ks[first] % V
    c, d = opp[order][first], np.where(count == 2, opp[order][np.minimum(first + 1, len(ks) - 1)], -1)
    edge_of = np.zeros(3 * F, np.int64)
    edge_of[order] = np.cumsum(new) - 1
    edge_of = edge_of.reshape(F, 3)
    inner = d >= 0
    valence = np.bincount(np.concatenate([lo, hi]), minlength=V)
    boundary = np.bincount(np.concatenate([lo[~inner], hi[~inner]]), minlength=V) > 0
    ab, bc, ca = V + edge_of[:, 0], V + edge_of[:, 1], V + edge_of[:, 2]
    faces = np.stack([np.stack([idx[:, 0], ab, ca], 1), np.stack([ab, idx[:, 1], bc], 1), np.stack([ca, bc, idx[:, 2]], 1), np.stack([ab, bc, ca], 1)], 1).reshape(-1, 3)
    return {"V": V, "lo": lo, "hi": hi, "c": c, "d": np.maximum(d, 0), "inner": inner, "valence": valence, "boundary": boundary, "faces": faces}


def scatter(index, values, n):
    """out[index[i]] += values[i] over (m, 3) values (np.bincount per axis: much faster than np.add.at)"""
    return np.stack([np.bincount(index, weights=values[:, a], minlength=n) for a in range(3)], axis=1)


def numpy_level(p, t):
    lo, hi, V = t["lo"], t["hi"], t["V"]
    ends = p[lo] + p[hi]
    odd = np.where(t["inner"][:, None], 0.375 * ends + 0.125 * (p[t["c"]] + p[t["d"]]), 0.5 * ends)
    s = scatter(lo, p[hi], V) + scatter(hi, p[lo], V)  # interior: the sum over all neighbours
    outer = ~t["inner"]
    sb = scatter(lo[outer], p[hi[outer]], V) + scatter(hi[outer], p[lo[outer]], V)  # boundary: over the boundary neighbours
    n = np.maximum(t["valence"], 1).astype(np.float64)
    beta = np.where(t["valence"] == 3, 3.0 / 16.0, 3.0 / (8.0 * n))
    even = np.where(t["boundary"][:, None], 0.75 * p + 0.125 * sb, (1.0 - n * beta)[:, None] * p + beta[:, None] * s)
    return np.concatenate([even, odd])


def numpy_refine(cage, tables):
    p = cage
    for t in tables:
        p = numpy_level(p, t)
    f = tables[-1]["faces"]
    fn = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    n = scatter(f[:, 0], fn, p.shape[0]) + scatter(f[:, 1], fn, p.shape[0]) + scatter(f[:, 2], fn, p.shape[0])
    return p, n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quads", type=int, default=88)
    ap.add_argument("--levels", type=int, default=3)
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
        row(f"{what:<88s} median {stats[0]:10.3f} ms   (min {stats[1]:.3f}, max {stats[2]:.3f}; {reps} calls)")

    cage, idx = bent_grid(args.quads)
    tables, faces, V = [], idx, cage.shape[0]
    for _ in range(L):
        tables.append(level_tables(faces, V))
        faces, V = tables[-1]["faces"], V + len(tables[-1]["lo"])
    nv, nf = V, faces.shape[0]
    cages = [cage + 0.02 * np.sin(5.0 * cage[:, [2, 0, 1]] + k) for k in range(4)]
    row(f"cage: {cage.shape[0]} vertices, {idx.shape[0]} faces; {L} levels: {nv} vertices, {nf} faces")

    # ---- 1. the kernels
    if not args.baseline_only:
        with capi.Subdiv(idx, cage.shape[0], L) as sub:
            assert (sub.n_vertices, sub.n_faces) == (nv, nf)
            out_p, out_n = (torch.zeros((nv, 3), dtype=torch.float64, device="cuda") for _ in range(2))
            d_cage = torch.from_numpy(cages[0]).cuda()
            sub.refine_device(out_p, out_n, d_cage)
            ms = {}
            for _ in range(reps):  # the two variants of the normal pass alternate (TAKE_HIP_SUBDIV_NORMALS: the library's switch)
                for variant in ("", "recompute"):
                    os.environ["TAKE_HIP_SUBDIV_NORMALS"] = variant
                    for line in verbose_lines(lambda: sub.refine_device(out_p, out_n, d_cage)):
                        m = re.search(r"subdiv_refine: (level \d+|normals) (k_subdiv_\w+) .* ([0-9.]+) ms$", line)
                        if m and (variant == "" or m.group(1) == "normals"):
                            ms.setdefault((m.group(1), m.group(2)), []).append(float(m.group(3)))
            del os.environ["TAKE_HIP_SUBDIV_NORMALS"]
            # algorithmic bytes: even 24 own + 4 row start + 8 boundary pair + (4 index + 24 position) per neighbour + 24 out;
            # odd 16 record + 24 per gathered end / wing + 24 out; face normals 12 + 72 + 24; vertex normals 4 row start +
            # (4 index + 24 normal) per face + 24 out
            passes = []
            for l, t in enumerate(tables):
                E, inner = len(t["lo"]), int(t["inner"].sum())
                even = t["V"] * (24 + 4 + 8 + 24) + 2 * E * (4 + 24)
                odd = E * (16 + 24) + (4 * inner + 2 * (E - inner)) * 24
                passes.append((f"level {l + 1}", [("k_subdiv_even", even), ("k_subdiv_odd", odd)], t["V"] + E))
            passes.append(("normals", [("k_subdiv_face_normals", nf * (12 + 72 + 24)), ("k_subdiv_vertex_normals", nv * (4 + 24) + 3 * nf * (4 + 24))], nv))
            # the variant that recomputes: 4 row start + (4 face + 12 indices + 72 positions) per face of the row + 24 out
            passes.append(("normals", [("k_subdiv_vertex_normals_recomputed", nv * (4 + 24) + 3 * nf * (4 + 12 + 72))], nv))
            for name, kernels, out_vertices in passes:
                total_ms, total_bytes = 0.0, 0
                for kernel, nbytes in kernels:
                    med = statistics.median(ms[(name, kernel)])
                    total_ms, total_bytes = total_ms + med, total_bytes + nbytes
                    row(f"  {name} {kernel}: median {med:.4f} ms (min {min(ms[(name, kernel)]):.4f}, max {max(ms[(name, kernel)]):.4f}; {reps} refines), "
                        f"{nbytes / 1e6:.2f} MB -> {nbytes / med / 1e6:.0f} GB/s")
                half = max(total_bytes // 2 // 8, 1)
                src, dst = torch.zeros(half, dtype=torch.float64, device="cuda"), torch.zeros(half, dtype=torch.float64, device="cuda")
                copy = copy_ms(dst, src, reps)
                row(f"{name}: {out_vertices} vertices out, {total_bytes / out_vertices:.0f} B/vertex, {total_ms:.4f} ms -> {total_bytes / total_ms / 1e6:.0f} GB/s; "
                    f"a device-to-device copy moving the same {total_bytes / 1e6:.2f} MB (read + written; device events round 10 copies, a tenth of it): {copy[0]:.4f} ms "
                    f"-> {total_bytes / copy[0] / 1e6:.0f} GB/s")
                del src, dst
            wall(f"refine_device, {nv} vertices, with normals", timed(lambda: sub.refine_device(out_p, out_n, d_cage), reps))
            wall(f"refine_device, {nv} vertices, positions alone", timed(lambda: sub.refine_device(out_p, None, d_cage), reps))
            row(f"the handle holds {sub.info()['device_bytes'] / 1e6:.1f} MB")
            del out_p, out_n

    # ---- 2. the whole call
    names = [] if args.kernel_only else args.precisions.split(",")
    if names:
        p0, n0 = numpy_refine(cage, tables)
        sd = SceneData(width=256, height=256, lookfrom=(0.0, 1.5, 3.0), lookat=(0.0, -0.3, 0.0), up=(0.0, 1.0, 0.0), vfov=45.0, background=(0.2, 0.3, 0.4), spp=4, max_depth=6)
        grey = sd.add_material(D.MAT_DIFFUSE, (0.7, 0.7, 0.7))
        sd.add_mesh(p0, faces.astype(np.int32), grey, normals=n0)
        sd.add_sphere((0.0, 0.4, 0.0), 0.25, grey)
        sd.lights.append(Light(0, -1, (12.0, 12.0, 12.0), (0.3, 2.0, 1.5)))
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
                made["pn"] = numpy_refine(next_cage(), tables)
                sc.update_meshes({0: made["pn"]})

            wall(f"{tag}: numpy refinement + update_meshes(host arrays)", timed(host_route, reps))
            wall(f"{tag}:   of it, numpy refinement", timed(lambda: numpy_refine(next_cage(), tables), reps))
            wall(f"{tag}:   of it, update_meshes(host arrays)", timed(lambda: sc.update_meshes({0: made["pn"]}), reps))
            if not args.baseline_only:
                with capi.Subdiv(idx, cage.shape[0], L) as sub:
                    out_p, out_n = (torch.zeros((nv, 3), dtype=torch.float64, device="cuda") for _ in range(2))
                    wall(f"{tag}: subdivide_meshes", timed(lambda: sc.subdivide_meshes([(0, sub, next_cage())]), reps))
                    wall(f"{tag}:   refine alone (Subdiv.refine_device)", timed(lambda: sub.refine_device(out_p, out_n, next_cage()), reps))
                    wall(f"{tag}:   update alone (update_meshes over the refined device arrays)", timed(lambda: sc.update_meshes({0: (out_p, out_n)}), reps))
                    del out_p, out_n
        finally:
            sc.close()
    text = "\n".join([f"subdiv_time.py --reps {reps} --quads {args.quads} --levels {L} --precisions {args.precisions}"
                      f"{' --baseline-only' if args.baseline_only else ''}{' --kernel-only' if args.kernel_only else ''}   ({torch.cuda.get_device_name(0)})", ""] + rows) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

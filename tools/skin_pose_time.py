"""What posing a rig costs on the device (take_hip_rig_pose_device, take_hip_scene_pose_meshes).

1. Kernel time, by the library's own events (TAKE_HIP_VERBOSE=1): a rig of `--vertices` vertices (1M), K = 4, 64 joints,
   with normals, T = 0 and T = 4 morph targets; the median over `--reps` poses after a warm-up, against the algorithmic
   bytes per vertex — 48 rest + 12 K influences + 48 T deltas + 48 out — as GB/s.
2. The whole call on the bench's scene (the 1M-triangle soup, its 3M soup vertices given 4 influences each over 64
   joints): the median wall time of `--reps` Scene.pose_meshes calls after a warm-up, its split into pose and update
   (pose: Rig.pose_device alone; update: update_meshes over the posed device arrays), and the only route there was
   before: the same skinning in numpy on the host, then update_meshes with host arrays.

`--baseline-only` runs the numpy route alone; it needs nothing of the rig API, so a copy of this file in the tools/ of a
checkout of an earlier commit measures that commit.

    python tools/skin_pose_time.py [--reps 10] [--vertices 1000000] [--joints 64] [--precisions f32,mixed] [--baseline-only | --kernel-only] [--out FILE]
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

from take_amd import capi, scenes  # noqa: E402
from take_amd import cdefs as D  # noqa: E402

N_JOINTS, K = 64, 4


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
        return [line.strip() for line in tmp.read().decode(errors="replace").splitlines() if "rig_pose:" in line]


def influences(pos, rng):
    """K joints and weights per vertex over N_JOINTS joints placed at random in the positions' box: the K nearest of 8
    drawn candidates, weights falling off with distance (a spatially coherent, but not sorted, gather)"""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    centres = rng.uniform(lo, hi, (N_JOINTS, 3))
    cand = rng.integers(0, N_JOINTS, (pos.shape[0], 8))
    d = np.linalg.norm(pos[:, None, :] - centres[cand], axis=2)
    order = np.argsort(d, axis=1)[:, :K]
    joints = np.take_along_axis(cand, order, axis=1).astype(np.int32)
    w = 1.0 / (0.05 + np.take_along_axis(d, order, axis=1))
    return joints, w / w.sum(axis=1, keepdims=True), centres


def joint_matrices(centres, rng, amount=0.05):
    """joint -> world: a small rotation about the joint's centre and a small translation; the inverse bind matrices"""
    n = centres.shape[0]
    bind = np.tile(np.eye(3, 4), (n, 1, 1))
    bind[:, :, 3] = -centres
    X = np.zeros((n, 3, 4))
    a = rng.uniform(-amount, amount, n)
    X[:, 0, 0], X[:, 0, 1], X[:, 1, 0], X[:, 1, 1], X[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1.0
    X[:, :, 3] = centres + rng.uniform(-amount, amount, (n, 3))
    return X, bind


def numpy_skin(pos, joints, weights, X, bind):
    """linear-blend skinning on the host, as a user of update_meshes wrote it before: vectorised numpy, float64"""
    J = np.zeros_like(X)
    J[:, :, :3] = X[:, :, :3] @ bind[:, :, :3]
    J[:, :, 3] = np.einsum("jrc,jc->jr", X[:, :, :3], bind[:, :, 3]) + X[:, :, 3]
    M = weights[:, 0, None, None] * J[joints[:, 0]]
    for k in range(1, joints.shape[1]):
        M += weights[:, k, None, None] * J[joints[:, k]]
    return np.einsum("vrc,vc->vr", M[:, :, :3], pos) + M[:, :, 3]


def main():
    global N_JOINTS
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vertices", type=int, default=1_000_000)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--joints", type=int, default=N_JOINTS, help="joints of both rigs (default 64)")
    ap.add_argument("--precisions", default="f32,mixed")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="part 1 alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(args.reps, 10)
    N_JOINTS = args.joints
    rng = np.random.default_rng(1)
    rows = []

    def row(text):
        rows.append(text)
        print(text, flush=True)

    def wall(what, stats):
        row(f"{what:<84s} median {stats[0]:10.3f} ms   (min {stats[1]:.3f}, max {stats[2]:.3f}; {reps} calls)")

    # ---- 1. the kernel
    if not args.baseline_only:
        nv = args.vertices
        pos = rng.uniform(-1, 1, (nv, 3))
        nrm = rng.standard_normal((nv, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        joints, weights, centres = influences(pos, rng)
        X, bind = joint_matrices(centres, rng)
        out_p, out_n = torch.zeros((nv, 3), dtype=torch.float64, device="cuda"), torch.zeros((nv, 3), dtype=torch.float64, device="cuda")
        d_X = torch.from_numpy(X).cuda()
        for T in (0, 4):
            tp = rng.uniform(-0.01, 0.01, (T, nv, 3)) if T else None
            tn = rng.uniform(-0.01, 0.01, (T, nv, 3)) if T else None
            d_w = torch.from_numpy(rng.uniform(0, 1, T)).cuda() if T else None
            with capi.Rig(pos, normals=nrm, joints=joints, weights=weights, inverse_bind=bind, target_positions=tp, target_normals=tn) as rig:
                rig.pose_device(out_p, out_n, d_X, d_w)
                ms, name = [], "k_skin_pose"
                for _ in range(reps):
                    for line in verbose_lines(lambda: rig.pose_device(out_p, out_n, d_X, d_w)):
                        m = re.search(r"(k_skin_pose\S*) .* ([0-9.]+) ms$", line)
                        if m:
                            name = m.group(1)
                            ms.append(float(m.group(2)))
                bytes_per_vertex = 48 + 12 * K + 48 * T + 48
                med = statistics.median(ms)
                row(f"{name}: {nv} vertices, K = {K}, {N_JOINTS} joints, T = {T}, normals: median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}; {len(ms)} poses), "
                    f"{bytes_per_vertex} B/vertex -> {nv * bytes_per_vertex / med / 1e6:.0f} GB/s")
        del out_p, out_n

    # ---- 2. the whole call, on the bench's scene
    names = [] if args.kernel_only else args.precisions.split(",")
    if names:
        sd = scenes.soup_scene(args.tris, 1920, 1080, spp=256)
        mesh = max(range(len(sd.meshes)), key=lambda m: sd.meshes[m].positions.shape[0])
        pos = sd.meshes[mesh].positions
        joints, weights, centres = influences(pos, rng)
        poses = [joint_matrices(centres, rng)[0] for _ in range(4)]
        bind = joint_matrices(centres, rng)[1]
    for name in names:
        precision = {"f32": D.TAKE_PRECISION_F32, "f64": D.TAKE_PRECISION_F64, "mixed": D.TAKE_PRECISION_MIXED}[name]
        tag = f"{args.tris}-triangle soup ({pos.shape[0]} vertices), {name}"
        sc = capi.Scene(sd, precision=precision)
        state = {"k": 0}

        def next_pose():
            state["k"] += 1
            return poses[state["k"] % len(poses)]

        try:
            skinned = {}

            def host_route():
                skinned["p"] = numpy_skin(pos, joints, weights, next_pose(), bind)
                sc.update_meshes({mesh: skinned["p"]})

            wall(f"{tag}: numpy skinning + update_meshes(host arrays)", timed(host_route, reps))
            wall(f"{tag}:   of it, numpy skinning", timed(lambda: numpy_skin(pos, joints, weights, next_pose(), bind), reps))
            wall(f"{tag}:   of it, update_meshes(host arrays)", timed(lambda: sc.update_meshes({mesh: skinned["p"]}), reps))
            if not args.baseline_only:
                with capi.Rig(pos, joints=joints, weights=weights, inverse_bind=bind) as rig:
                    out_p = torch.zeros(pos.shape, dtype=torch.float64, device="cuda")
                    wall(f"{tag}: pose_meshes", timed(lambda: sc.pose_meshes([(mesh, rig, next_pose(), None)]), reps))
                    wall(f"{tag}:   pose alone (Rig.pose_device)", timed(lambda: rig.pose_device(out_p, None, next_pose(), None), reps))
                    wall(f"{tag}:   update alone (update_meshes over the posed device array)", timed(lambda: sc.update_meshes({mesh: out_p}), reps))
                    del out_p
        finally:
            sc.close()
    text = "\n".join([f"skin_pose_time.py --reps {reps} --vertices {args.vertices} --tris {args.tris} --joints {args.joints} --precisions {args.precisions}"
                      f"{' --baseline-only' if args.baseline_only else ''}{' --kernel-only' if args.kernel_only else ''}   ({torch.cuda.get_device_name(0)})", ""] + rows) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""diagnostic: compute_normals on the device (take_hip_compute_normals / DeviceMesh.compute_normals, tk_normals.h).

    python tools/diag_normals.py [n_faces]        (default 10M; needs the GPU and tests/normals_shim)

Reports
  * the ulp distance of the device normals from the reference's (tests/golden/normals) and from the host build of the
    same kernels (tests/normals_shim) on a ~1M-face grid + soup and on a 1M-face fan: the measured value behind the
    bound in tests/test_gpu_normals.py;
  * on a jittered grid of n_faces faces written as a binary PLY without normals: the host build's serial loop (the
    reference's loop, the same arithmetic), the device step alone (DeviceMesh.compute_normals(): HIP events around
    the call and wall time), and file -> first pixel (decode with normals="scene", scene_create, a 1-spp frame);
  * the device step on a 1M-face fan (one vertex of valence 1M)."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import normals_ref  # noqa: E402
from oracle.gen_golden import write_ply  # noqa: E402
from take_amd import capi, scenes  # noqa: E402
from test_normals_cpu import CASES, fan, jittered_grid, load_case, shim_normals, soup  # noqa: E402


def ulp(got, want, p, f):
    """-> (max ulp in units of the row's largest component times the vertex's condition number, the same without the
    condition number, max ulp of the component itself, fraction of rows bit-identical, components whose sign or
    zero-ness differs)"""
    kappa = np.maximum(np.nan_to_num(normals_ref.condition(p, f), nan=1.0, posinf=1.0), 1.0)
    scale = np.spacing(np.abs(want).max(axis=1, initial=0))[:, None]
    own = np.abs(got.view(np.int64) - want.view(np.int64))
    same_sign = np.signbit(got) == np.signbit(want)
    return (float((np.abs(got - want) / (scale * kappa[:, None])).max(initial=0)), float((np.abs(got - want) / scale).max(initial=0)),
            int(own[same_sign].max(initial=0)), float(np.all(got.view(np.uint64) == want.view(np.uint64), axis=1).mean()),
            int(np.count_nonzero(~same_sign | ((got == 0) != (want == 0)))))


def timed_device_step(path, reps=3):
    """DeviceMesh.compute_normals() on a freshly decoded mesh: (HIP-event ms, wall ms) of the best rep"""
    best = None
    for _ in range(reps):
        dm = capi.DeviceMesh(path)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        dm.compute_normals()
        e1.record()
        torch.cuda.synchronize()
        r = (e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3)
        best = r if best is None or r[1] < best[1] else best
        dm.close()
    return best


def main():
    n_faces = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    capi.device_count()
    # 1. accuracy
    worst = {name: ulp(capi.compute_normals(*load_case(name)[:2]), load_case(name)[2], *load_case(name)[:2]) for name in CASES}
    print("ulp vs the reference per fixture:", worst, flush=True)
    g, s = jittered_grid(801, 401, 21), soup(360_000, 120_000, 22)
    p = np.concatenate([g[0], s[0]])
    f = np.concatenate([g[1], s[1] + len(g[0])]).astype(np.int32)
    d = capi.compute_normals(p, f)
    print(f"ulp vs the host build, {len(f)}-face grid + soup: {ulp(d, shim_normals(p, f), p, f)}; "
          f"identical over two runs: {np.array_equal(d.view(np.uint64), capi.compute_normals(p, f).view(np.uint64))}", flush=True)
    fp, ff = fan(1_000_000, 23)
    print(f"ulp vs the host build, 1M-face fan: {ulp(capi.compute_normals(fp, ff), shim_normals(fp, ff), fp, ff)}", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        # 2. the 1M fan, device step alone
        fan_ply = os.path.join(tmp, "fan.ply")
        write_ply(fan_ply, fp, ff)
        ev, wall = timed_device_step(fan_ply)
        print(f"1M-face fan, device step: {ev:.2f} ms (events), {wall:.2f} ms wall", flush=True)
        # 3. a grid of n_faces faces in the soup scene's box
        nx = int(round((n_faces / 2) ** 0.5)) + 1
        gp, gf = jittered_grid(nx, nx, 31)
        gp = gp - gp.min(axis=0)
        gp = gp / gp.max(axis=0).max()
        sd = scenes.soup_scene(8, 64, 64, spp=1)
        k = max(range(len(sd.meshes)), key=lambda i: sd.meshes[i].indices.shape[0])
        lo, hi = sd.meshes[k].positions.min(axis=0), sd.meshes[k].positions.max(axis=0)
        gp = lo + gp * (hi - lo)
        path = os.path.join(tmp, "grid.ply")
        write_ply(path, gp, gf)
        print(f"grid: {len(gp)} vertices, {len(gf)} faces, {os.path.getsize(path) / 1e6:.0f} MB", flush=True)
        hp = gp.astype(np.float32).astype(np.float64)
        t0 = time.perf_counter()
        shim_normals(hp, gf)
        print(f"host serial loop (the reference's, tk_normals.h built with g++ -O2): {time.perf_counter() - t0:.3f} s", flush=True)
        del hp
        ev, wall = timed_device_step(path)
        print(f"device step alone: {ev:.2f} ms (events), {wall:.2f} ms wall", flush=True)
        for rep in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dm = capi.DeviceMesh(path, material_id=sd.meshes[k].material_id, normals="scene")
            t1 = time.perf_counter()
            sdx = scenes.soup_scene(8, 64, 64, spp=1)
            sdx.meshes[k] = dm
            sc = capi.Scene(sdx)
            t2 = time.perf_counter()
            img = sc.render(spp=1, max_depth=4)
            t3 = time.perf_counter()
            print(f"file -> first pixel: {t3 - t0:.3f} s (decode + normals {t1 - t0:.3f}, scene_create {t2 - t1:.3f}, "
                  f"frame {t3 - t2:.3f}; mean {img.mean():.4f})", flush=True)
            sc.close()
            dm.close()


if __name__ == "__main__":
    main()

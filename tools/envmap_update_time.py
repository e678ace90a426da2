"""What a new environment map costs on a resident scene (take_hip_scene_set_envmap) against the only route
there was before it — creating the scene again.  On the bench's scene (1M-triangle soup, env-lit, F32), after one warm-up
call each, the median wall time of `--reps` calls (at least 10) of

  * Scene.set_envmap at 2048 x 1024 (scenes.sky_envmap) and at 8192 x 4096, from a host float64 array and from a float32
    tensor on the device;
  * Scene(...) of that scene again (what changing the map took before);
  * Scene(env_scene(map)) — an empty scene, so in effect the host's table build plus the upload — at both sizes;

and, from one more call of each set_envmap under TAKE_HIP_VERBOSE=1, the library's own event times per kernel.

    python tools/envmap_update_time.py [--reps 10] [--tris 1000000] [--large 8192x4096] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from take_amd import capi, scenes  # noqa: E402


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


def kernel_times(f):
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
        return [line.strip() for line in tmp.read().decode(errors="replace").splitlines() if "set_envmap:" in line]


def main():
    import torch

    import env_maps

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--large", default="8192x4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(args.reps, 10)
    lw, lh = (int(v) for v in args.large.split("x"))
    small, large = scenes.sky_envmap(2048, 1024), scenes.sky_envmap(lw, lh)
    large32 = torch.from_numpy(large.astype(np.float32)).cuda()
    sd = scenes.soup_scene(args.tris, 1920, 1080, spp=256, envmap=(2048, 1024))
    rows, kernels = [], []

    def row(what, stats):
        rows.append(f"{what:<64s} median {stats[0]:10.3f} ms   (min {stats[1]:.3f}, max {stats[2]:.3f}; {reps} calls)")
        print(rows[-1], flush=True)

    sc = capi.Scene(sd)
    try:
        for what, img in ((f"set_envmap 2048x1024, host float64", small), (f"set_envmap {lw}x{lh}, host float64", large),
                          (f"set_envmap {lw}x{lh}, float32 device tensor", large32)):
            row(what, timed(lambda: sc.set_envmap(img), reps))
            kernels += [f"{what}:"] + ["    " + line for line in kernel_times(lambda: sc.set_envmap(img))]
    finally:
        sc.close()
    row(f"Scene(...) of the {args.tris}-triangle scene again", timed(lambda: capi.Scene(sd).close(), reps))
    for what, img in (("Scene(env_scene(map)) 2048x1024 (empty scene: host tables + upload)", small),
                      (f"Scene(env_scene(map)) {lw}x{lh} (empty scene: host tables + upload)", large)):
        esd = env_maps.env_scene(img)
        row(what, timed(lambda: capi.Scene(esd).close(), reps))
    text = "\n".join([f"envmap_update_time.py --reps {reps} --tris {args.tris} --large {args.large}   ({torch.cuda.get_device_name(0)})", ""] + rows +
                     ["", "per kernel, the library's own event times of one call (TAKE_HIP_VERBOSE=1):"] + kernels) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    else:
        print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

"""What new materials and new light intensities cost on a resident scene (take_hip_scene_set_materials,
take_hip_scene_set_light_intensities) against the only route there was before them — creating the scene
again.  On the bench's scene (1M-triangle soup, F32) and on a 10M-triangle scene built by the device builder, each with
an emissive mesh of `--emissive` triangles (one area light per triangle) added, after one warm-up call each, the median
wall time of `--reps` calls (at least 10) of

  * Scene.set_materials with a tag change (the soup's material Lambert <-> Phong, alternating: every call rewrites the
    tag byte of every soup record) and without one (a new colour: the table alone);
  * Scene.set_light_intensities over the emissive mesh's lights, from a host array and from a float64 device tensor;
  * Scene(...) of that scene again (what either change took before);

and, from one more call of the tag change under TAKE_HIP_VERBOSE=1, the library's own event time of the retag kernels.

    python tools/shading_update_time.py [--reps 10] [--sizes 1000000,10000000] [--emissive 100000] [--out FILE]
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

from take_amd import capi, scenes  # noqa: E402
from take_amd import cdefs as D  # noqa: E402
from take_amd.scene import Material  # noqa: E402


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
        return [line.strip() for line in tmp.read().decode(errors="replace").splitlines() if "set_materials:" in line]


def scene(tris, emissive):
    """the bench's soup scene plus an emissive soup of `emissive` triangles under the ceiling -> (scene, first light of the mesh)"""
    sd = scenes.soup_scene(tris, 1920, 1080, spp=256)
    first = len(sd.lights)
    pos, idx = scenes.soup_triangles(emissive, 99, 0.5, 0.004)
    sd.add_mesh(pos * (1.0, 0.1, 1.0) + (0.0, 0.8, 0.0), idx, 0, normals=np.tile((0.0, -1.0, 0.0), (pos.shape[0], 1)), emission=(2.0, 2.0, 2.0))
    return sd, first


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--emissive", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps = max(args.reps, 10)
    rows, kernels = [], []

    def row(what, stats):
        rows.append(f"{what:<72s} median {stats[0]:10.3f} ms   (min {stats[1]:.3f}, max {stats[2]:.3f}; {reps} calls)")
        print(rows[-1], flush=True)

    for tris in (int(v) for v in args.sizes.split(",")):
        builder = D.TAKE_BUILDER_DEVICE_LBVH if tris > 4_000_000 else D.TAKE_BUILDER_AUTO
        sd, first = scene(tris, args.emissive)
        white = sd.materials[0]
        phong = Material(D.MAT_PHONG, white.color, param=(20.0,) + (0.0,) * 11)
        state = {"k": 0}

        def retag():
            state["k"] ^= 1
            sc.set_materials([phong if state["k"] else white])

        def recolour():
            state["k"] ^= 1
            sc.set_materials([Material(sd.materials[1].tag, (0.65, 0.05 + 0.1 * state["k"], 0.05))], first=1)

        rgb = np.random.default_rng(1).uniform(0.5, 4.0, (args.emissive, 3))
        d_rgb = torch.from_numpy(rgb).cuda()
        tag = f"{tris} triangles"
        sc = capi.Scene(sd, builder=builder)
        try:
            n_prims = sc.stats()["n_prims"]
            row(f"{tag}: set_materials, a tag change ({n_prims} records)", timed(retag, reps))
            kernels += [f"{tag}, a tag change:"] + ["    " + line for line in kernel_times(retag)]
            row(f"{tag}: set_materials, a colour (no tag changes)", timed(recolour, reps))
            row(f"{tag}: set_light_intensities, {args.emissive} lights, host array", timed(lambda: sc.set_light_intensities(rgb, first), reps))
            row(f"{tag}: set_light_intensities, {args.emissive} lights, device tensor", timed(lambda: sc.set_light_intensities(d_rgb, first), reps))
        finally:
            sc.close()
        row(f"{tag}: Scene(...) of the scene again", timed(lambda: capi.Scene(sd, builder=builder).close(), reps))
        del sd, d_rgb
    text = "\n".join([f"shading_update_time.py --reps {reps} --sizes {args.sizes} --emissive {args.emissive}   ({torch.cuda.get_device_name(0)})", ""] + rows +
                     ["", "the retag kernels, the library's own event times of one call (TAKE_HIP_VERBOSE=1):"] + kernels) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    else:
        print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

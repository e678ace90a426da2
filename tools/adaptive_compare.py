"""measurement: adaptive sampling (Scene.render_adaptive_device) against uniform renders on the bench scene — time,
samples taken and RMSE to a high-spp uniform render (the figures of DESIGN.md par. 4g; needs an MI355X).

  python tools/adaptive_compare.py [--tris N] [--width W --height H] [--precision mixed|f32|f64] [--truth-spp 4096]
      [--uniform 64,128,256] [--max-spp 256,1024] [--thresholds 0.02,0.05,0.1] [--min-spp 16 --step-spp 8] [--reps 3]
      [--out FILE.json]

Every image stays in device memory; a time is a host clock around a call that ends in a stream synchronisation, the
median of --reps calls after one warm-up call of the same shape.  The overhead block runs the machinery with
threshold 0 (only pixels of zero sample variance stop) against the uniform render of the same spp at
samples_per_batch = step_spp (like against like) and at the automatic batch size (what a user gets)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library is loaded)

from take_amd import capi, scenes  # noqa: E402
from take_amd import cdefs as D  # noqa: E402


def timed(call, reps):
    call()  # warm-up of this shape
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--max-depth", type=int, default=50)
    ap.add_argument("--precision", default="mixed", choices=["f32", "f64", "mixed"])
    ap.add_argument("--no-envmap", dest="envmap", action="store_false")
    ap.add_argument("--truth-spp", type=int, default=4096)
    ap.add_argument("--uniform", default="64,128,256")
    ap.add_argument("--max-spp", default="256,1024")
    ap.add_argument("--thresholds", default="0.02,0.05,0.1")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--step-spp", type=int, default=8)
    ap.add_argument("--overhead-spp", type=int, default=256, help="0: skip the overhead block")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    precision = {"f32": D.TAKE_PRECISION_F32, "f64": D.TAKE_PRECISION_F64, "mixed": D.TAKE_PRECISION_MIXED}[a.precision]
    dtype = torch.float32 if a.precision == "f32" else torch.float64
    sd = scenes.soup_scene(a.tris, a.width, a.height, spp=1, max_depth=a.max_depth, envmap=(2048, 1024) if a.envmap else None)
    sc = capi.Scene(sd, precision=precision)
    npix = a.width * a.height
    truth = torch.zeros((a.height, a.width, 3), dtype=dtype, device="cuda")
    img = torch.zeros_like(truth)
    count = torch.zeros((a.height, a.width), dtype=torch.int32, device="cuda")
    result = {"scene": f"{a.tris}-triangle soup" + (" + env-map" if a.envmap else ""), "size": [a.width, a.height], "precision": a.precision,
              "max_depth": a.max_depth, "min_spp": a.min_spp, "step_spp": a.step_spp, "reps": a.reps, "rows": []}

    def rmse():
        return float(torch.sqrt(torch.mean((img.double() - truth.double()) ** 2)))

    def row(**kw):
        result["rows"].append(kw)
        print(json.dumps(kw), flush=True)

    # (another seed than the compared renders: the ground truth shares no sample with them)
    t0 = time.perf_counter()
    sc.render_device(truth.data_ptr(), a.truth_spp, a.max_depth, seed=a.seed + 1)
    row(kind="truth", spp=a.truth_spp, seconds=time.perf_counter() - t0)
    for spp in [int(x) for x in a.uniform.split(",") if x]:
        med, lo, hi = timed(lambda: sc.render_device(img.data_ptr(), spp, a.max_depth, seed=a.seed), a.reps)
        row(kind="uniform", spp=spp, seconds=med, seconds_min=lo, seconds_max=hi, samples=npix * spp, rmse=rmse())
    for max_spp in [int(x) for x in a.max_spp.split(",") if x]:
        for thr in [float(x) for x in a.thresholds.split(",") if x]:
            call = lambda: sc.render_adaptive_device(img, max_spp, a.max_depth, seed=a.seed, min_spp=a.min_spp, step_spp=a.step_spp, threshold=thr,  # noqa: E731
                                                     stats={"count": count})
            med, lo, hi = timed(call, a.reps)
            c = count.cpu().numpy()
            row(kind="adaptive", max_spp=max_spp, threshold=thr, seconds=med, seconds_min=lo, seconds_max=hi, samples=int(c.sum(dtype="int64")),
                mean_spp=float(c.mean()), at_min=float((c == min(a.min_spp, max_spp)).mean()), at_max=float((c == max_spp).mean()), rmse=rmse())
    if a.overhead_spp > 0:
        spp = a.overhead_spp
        calls = {"adaptive, threshold 0": lambda: sc.render_adaptive_device(img, spp, a.max_depth, seed=a.seed, min_spp=a.min_spp, step_spp=a.step_spp, threshold=0.0,
                                                                            stats={"count": count}),
                 f"uniform, samples_per_batch {a.step_spp}": lambda: sc.render_device(img.data_ptr(), spp, a.max_depth, seed=a.seed, samples_per_batch=a.step_spp),
                 "uniform, automatic batch": lambda: sc.render_device(img.data_ptr(), spp, a.max_depth, seed=a.seed)}
        for name, call in calls.items():
            med, lo, hi = timed(call, a.reps)
            extra = {"samples": int(count.cpu().numpy().sum(dtype="int64"))} if name.startswith("adaptive") else {"samples": npix * spp}
            row(kind="overhead", what=name, spp=spp, seconds=med, seconds_min=lo, seconds_max=hi, **extra)
    sc.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

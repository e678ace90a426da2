"""measurement: the variance-guided denoiser (take_hip_denoise_variance*, take_hip_render_adaptive_denoised*) against the
fixed-sigma one (the figures of DESIGN.md par. 4h; needs an MI355X).  Three commands:

  python tools/denoise_var_compare.py levels [--width 1920 --height 1080] [--reps 5]
      runs both filters (default options, all three guides) on synthetic planes in device memory, f32 and f64, `reps`
      times after a warm-up each, and prints the host-clock time of a whole call.  Meant to run under
      `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/denoise_var_compare.py levels`;
  python tools/denoise_var_compare.py trace DIR
      reads the *kernel_trace.csv under DIR and prints, per precision, the median duration of the level launches of
      k_denoise_level and k_denoise_var_level (warm-up launches left out) and their ratio;
  python tools/denoise_var_compare.py table [--tris N] [--width W --height H] [--precision mixed|f32|f64] [--truth-spp 4096]
      [--max-spp 256,1024] [--thresholds 0.02,0.05,0.1] [--min-spp 16 --step-spp 8] [--out FILE.json]
      the adaptive rows of tools/adaptive_compare.py on the bench scene with one more column: the RMSE to the truth of
      the variance-guided result (Scene.render_adaptive_denoised_device) beside that of the adaptive image itself."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def levels(a):
    import torch  # (before the library is loaded)

    from take_amd import capi
    from take_amd import cdefs as D

    w, h = a.width, a.height
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rand(*shape):
        return torch.rand(*shape, generator=gen, device="cuda", dtype=torch.float64)

    albedo = 0.2 + 0.6 * rand(h, w, 3)
    normal = torch.nn.functional.normalize(rand(h, w, 3) - 0.5, dim=-1)
    depth = 2.0 + rand(h, w)
    n = 8  # samples per pixel: rgb their mean, m1 / m2 their moments, 30 % noise
    samples = (albedo * 0.8)[None] * (1.0 + 0.3 * (2.0 * rand(n, h, w, 3) - 1.0))
    L = samples.sum(-1)
    planes64 = {"rgb": samples.mean(0), "albedo": albedo, "normal": normal, "depth": depth}
    count = torch.full((h, w), n, dtype=torch.int32, device="cuda")
    m1, m2 = L.sum(0).contiguous(), (L * L).sum(0).contiguous()
    for name, dtype, precision in (("f32", torch.float32, D.TAKE_PRECISION_F32), ("f64", torch.float64, D.TAKE_PRECISION_F64)):
        p = {k: v.to(dtype).contiguous() for k, v in planes64.items()}
        out = torch.zeros_like(p["rgb"])
        guides = {k: p[k] for k in ("albedo", "normal", "depth")}
        calls = {"fixed sigma": lambda: capi.denoise_device(p["rgb"], w, h, precision, out=out, **guides),
                 "variance-guided": lambda: capi.denoise_variance_device(p["rgb"], count, m1, m2, w, h, precision, out=out, **guides)}
        for what, call in calls.items():
            call()  # warm-up of this shape
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()  # (returns after the stream has completed)
                times.append(time.perf_counter() - t0)
            print(json.dumps({"kind": "call", "precision": name, "filter": what, "size": [w, h], "ms_median": 1e3 * statistics.median(times),
                              "ms_min": 1e3 * min(times), "ms_max": 1e3 * max(times), "finite": bool(torch.isfinite(out).all())}), flush=True)
    return 0


def trace(a):
    files = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        print(f"no *kernel_trace.csv under {a.dir}")
        return 1
    launches = {}
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        for kernel in ("k_denoise_level", "k_denoise_var_level"):
            if kernel + "<" in name or kernel + "I" in name:  # (demangled, or the mangled name)
                precision = "f32" if kernel + "<float" in name or kernel + "If" in name else "f64"
                launches.setdefault((precision, kernel), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for precision in ("f32", "f64"):
        med = {}
        for kernel in ("k_denoise_level", "k_denoise_var_level"):
            d = [ns for _, ns in sorted(launches.get((precision, kernel), []))]
            d = d[a.levels:]  # (the first call of the shape is the warm-up)
            if d:
                med[kernel] = statistics.median(d)
                print(json.dumps({"kind": "level", "precision": precision, "kernel": kernel, "launches": len(d), "us_median": med[kernel] / 1e3, "us_min": min(d) / 1e3,
                                  "us_max": max(d) / 1e3}))
        if len(med) == 2:
            print(json.dumps({"kind": "ratio", "precision": precision, "var_over_fixed": med["k_denoise_var_level"] / med["k_denoise_level"]}))
    return 0


def table(a):
    import torch  # (before the library is loaded)

    from take_amd import capi, scenes
    from take_amd import cdefs as D

    precision = {"f32": D.TAKE_PRECISION_F32, "f64": D.TAKE_PRECISION_F64, "mixed": D.TAKE_PRECISION_MIXED}[a.precision]
    dtype = torch.float32 if a.precision == "f32" else torch.float64
    sd = scenes.soup_scene(a.tris, a.width, a.height, spp=1, max_depth=a.max_depth, envmap=(2048, 1024) if a.envmap else None)
    sc = capi.Scene(sd, precision=precision)
    truth = torch.zeros((a.height, a.width, 3), dtype=dtype, device="cuda")
    img = torch.zeros_like(truth)
    count = torch.zeros((a.height, a.width), dtype=torch.int32, device="cuda")
    result = {"scene": f"{a.tris}-triangle soup" + (" + env-map" if a.envmap else ""), "size": [a.width, a.height], "precision": a.precision,
              "max_depth": a.max_depth, "min_spp": a.min_spp, "step_spp": a.step_spp, "rows": []}

    def rmse():
        return float(torch.sqrt(torch.mean((img.double() - truth.double()) ** 2)))

    def row(**kw):
        result["rows"].append(kw)
        print(json.dumps(kw), flush=True)

    t0 = time.perf_counter()
    sc.render_device(truth.data_ptr(), a.truth_spp, a.max_depth, seed=a.seed + 1)  # (another seed than the compared renders)
    row(kind="truth", spp=a.truth_spp, seconds=time.perf_counter() - t0)
    for max_spp in [int(x) for x in a.max_spp.split(",") if x]:
        for thr in [float(x) for x in a.thresholds.split(",") if x]:
            kw = dict(seed=a.seed, min_spp=a.min_spp, step_spp=a.step_spp, threshold=thr, stats={"count": count})
            t0 = time.perf_counter()
            sc.render_adaptive_device(img, max_spp, a.max_depth, **kw)
            seconds, plain = time.perf_counter() - t0, rmse()
            t0 = time.perf_counter()
            sc.render_adaptive_denoised_device(img, max_spp, a.max_depth, **kw)
            seconds_denoised, guided = time.perf_counter() - t0, rmse()
            row(kind="adaptive", max_spp=max_spp, threshold=thr, mean_spp=float(count.float().mean()), seconds=seconds, rmse=plain,
                seconds_denoised=seconds_denoised, rmse_variance_guided=guided)
    sc.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="command", required=True)
    lv = sub.add_parser("levels")
    lv.add_argument("--width", type=int, default=1920)
    lv.add_argument("--height", type=int, default=1080)
    lv.add_argument("--reps", type=int, default=5)
    tr = sub.add_parser("trace")
    tr.add_argument("dir")
    tr.add_argument("--levels", type=int, default=5, help="level launches of the warm-up call to leave out")
    tb = sub.add_parser("table")
    tb.add_argument("--tris", type=int, default=1_000_000)
    tb.add_argument("--width", type=int, default=1920)
    tb.add_argument("--height", type=int, default=1080)
    tb.add_argument("--max-depth", type=int, default=50)
    tb.add_argument("--precision", default="mixed", choices=["f32", "f64", "mixed"])
    tb.add_argument("--no-envmap", dest="envmap", action="store_false")
    tb.add_argument("--truth-spp", type=int, default=4096)
    tb.add_argument("--max-spp", default="256,1024")
    tb.add_argument("--thresholds", default="0.02,0.05,0.1")
    tb.add_argument("--min-spp", type=int, default=16)
    tb.add_argument("--step-spp", type=int, default=8)
    tb.add_argument("--seed", type=int, default=0)
    tb.add_argument("--out", default=None)
    a = ap.parse_args()
    return {"levels": levels, "trace": trace, "table": table}[a.command](a)


if __name__ == "__main__":
    raise SystemExit(main())

"""The bytes every path-traced call returns, as one SHA-256 per call: what a change of the host side of rendering
(take_amd/csrc/tk_render.hip, tk_api.hip, tk_scene_update.hip) must leave as it is.  Two runs — two builds (TAKE_HIP_LIB),
or the two settings of TAKE_HIP_CAMERA_FUSED — are compared line by line; tests/test_gpu_camera_routes.py does the latter.

Scenes, each built once per precision: the golden cbox at 9 x 7 and at 65 x 3 (at 1 spp 63 and 195 paths: a queue that
ends inside a wave, one that crosses a block), the golden mats at its own size (sorted material tags) and
scenes.instanced_scene(5, 300, 45, 27) (two levels).  Calls, in f32, f64 and mixed precision where the call exists: see
image_calls.  One line per call, "<scene>/<precision>/<call> <sha256 of the returned bytes>".

Then a shorter list of calls under set_instrumentation(timing=True, counting=True), one line each that starts with
"counters": the integer fields of TakeCounters (never the times).  Counting keeps round 0 on the generate route under
either setting of TAKE_HIP_CAMERA_FUSED, so these lines say nothing about the two routes; between two builds they are
equal too.

    python tools/render_digests.py > digests.txt

With --resident the tool prints another list instead: the bytes a resident scene holds in device memory after each change
of it (take_amd/csrc/tk_scene_update.hip, and the drivers of tk_build.hip behind it), which a change of those must leave as
they are.  One line per item, "resident/<scene>/<precision>/<step>/<array> <sha256>": per side of the scene the arrays
Scene.debug_tree returns (<side>.nodes, .prims, .inst_trace) and its scalars (<side>.info), and one 9 x 7, 2 spp render,
which covers the placements' shading records, lights, tables and normals.  Scenes and steps: see resident_steps.

    python tools/render_digests.py --resident > resident.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch  # (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import golden_scene  # noqa: E402
from take_amd import capi, scenes  # noqa: E402
from take_amd import cdefs as D  # noqa: E402

PRECISIONS = {"f32": D.TAKE_PRECISION_F32, "f64": D.TAKE_PRECISION_F64, "mixed": D.TAKE_PRECISION_MIXED}
DEPTH, SEED = 4, 7
LENS_RADIUS = 0.05
ADAPTIVE = dict(spp=16, min_spp=4, step_spp=4, threshold=0.05, samples_per_batch=3, stats=True)
MOVED_CAMERA = dict(lookfrom=(0.3, 0.2, 3.7), lookat=(0.05, 0.0, 0.0), up=(0.02, 1.0, 0.0))
COUNTED_SCENES = ("cbox65x3", "instanced")
COUNTER_FIELDS = ("samples", "rays_closest", "rays_closest_f32", "rays_shadow", "bounces", "node_visits", "prim_tests",
                  "launches_trace_closest", "launches_trace_closest_f32", "launches_trace_shadow")


def scene_set():
    """name -> SceneData"""
    def cbox(w, h):
        sd = golden_scene("cbox")
        sd.width, sd.height = w, h
        return sd

    return {"cbox9x7": cbox(9, 7), "cbox65x3": cbox(65, 3), "mats": golden_scene("mats"),
            "instanced": scenes.instanced_scene(5, 300, 45, 27, 1)}


def digest(result):
    """SHA-256 of an array, of a dict's arrays in the order of their names, or of a tuple's members in turn"""
    h = hashlib.sha256()

    def feed(r):
        if isinstance(r, dict):
            for k in sorted(r):
                feed(r[k])
        elif isinstance(r, (tuple, list)):
            for m in r:
                feed(m)
        else:
            h.update(np.ascontiguousarray(r).tobytes())

    feed(result)
    return h.hexdigest()


def moved_transforms(sd):
    """the placements of `sd` pushed along x and y: the current frame of the motion pass and the shutter"""
    x = np.stack([np.asarray(t, np.float64).reshape(3, 4) for t in sd.instance_xform]).copy()
    x[:, 0, 3] += 0.07
    x[:, 1, 3] -= 0.04
    return x


def accumulate_twice(sc):
    img = torch.zeros((sc.sd.height, sc.sd.width, 3), dtype=torch.float32 if sc.dtype == np.float32 else torch.float64, device="cuda")
    first = None
    for restart in (True, False):
        sc.render_accumulate(img.data_ptr(), 2, DEPTH, seed=SEED, restart=restart)
        torch.cuda.synchronize()
        first = img.cpu().numpy() if restart else first
    return first, img.cpu().numpy()


def adaptive(sc, name):
    img, planes = sc.render_adaptive(max_depth=DEPTH, seed=SEED, **ADAPTIVE)
    count = planes["count"]
    assert (count > ADAPTIVE["min_spp"]).any(), f"{name}: no pixel stays active after pass 0: the listed passes do not run"
    return img, planes


def with_lens(sc, call):
    sc.set_lens(LENS_RADIUS)
    try:
        return call()
    finally:
        sc.set_lens(0.0)


def image_calls(sc, name, precision):
    """[(label, f() -> what the call returns)] in the order they run; the scene ends as it began but for its mark"""
    rays = {}

    def camera_rays():
        rays["all"] = sc.camera_rays(3, seed=SEED, first_sample=2)
        return rays["all"]

    def motion():
        sc.mark_frame()
        sc.set_camera(**MOVED_CAMERA, vfov=sc.sd.vfov)
        try:
            return sc.render_motion()
        finally:
            sc.set_camera(sc.sd.lookfrom, sc.sd.lookat, sc.sd.up, sc.sd.vfov)

    def shutter():
        sc.mark_frame()
        sc.set_instance_transforms(moved_transforms(sc.sd))
        sc.set_camera(**MOVED_CAMERA, vfov=sc.sd.vfov)
        try:
            return sc.render_shutter(spp=4, max_depth=DEPTH, seed=SEED, slices=2)
        finally:
            sc.set_instance_transforms(np.stack([np.asarray(t, np.float64).reshape(3, 4) for t in sc.sd.instance_xform]))
            sc.set_camera(sc.sd.lookfrom, sc.sd.lookat, sc.sd.up, sc.sd.vfov)

    calls = [("render", lambda: sc.render(spp=3, max_depth=DEPTH, seed=SEED, samples_per_batch=2))]
    if precision != "mixed":  # (mixed precision renders integrator 0 only)
        calls.append(("render_integrator1", lambda: sc.render(spp=3, max_depth=DEPTH, seed=SEED, samples_per_batch=2, integrator=1)))
    calls += [
        ("render_lens", lambda: with_lens(sc, lambda: sc.render(spp=3, max_depth=DEPTH, seed=SEED, samples_per_batch=2))),
        ("render_accumulate", lambda: accumulate_twice(sc)),
        ("render_adaptive", lambda: adaptive(sc, name)),
        ("render_adaptive_lens", lambda: with_lens(sc, lambda: adaptive(sc, name))),
        ("render_features", lambda: sc.render_features(3, seed=SEED, samples_per_batch=2)),
        ("camera_rays", camera_rays),
        ("render_rays_sets", lambda: sc.render_rays(rays["all"], 3, DEPTH, seed=SEED, samples_per_batch=2, ray_sets=3, first_sample=2)),
        ("render_rays_normalize", lambda: sc.render_rays(rays["all"][0] * np.array([1, 1, 1, 1, 2.5, 2.5, 2.5, 1], sc.dtype), 3, DEPTH, seed=SEED,
                                                         samples_per_batch=2, normalize=True)),
        ("render_motion", motion),
    ]
    if name == "instanced":
        calls.append(("render_shutter", shutter))
    return calls


def counted_calls(sc, name, precision):
    """the shorter list, run with timing and counting on"""
    keep = ("render", "render_adaptive", "render_features", "camera_rays", "render_rays_sets", "render_motion")
    return [(label, f) for label, f in image_calls(sc, name, precision) if label in keep]


def resident_steps():
    """[(scene name, SceneData, [(step, f(sc))])]: what each step does to the resident scene `sc`.  The scenes and the
    deformations are those of tests/test_gpu_proto_update.py and tests/test_gpu_mesh_update.py, at 9 x 7 pixels."""
    import test_gpu_mesh_update as M
    import test_gpu_proto_update as P

    def small(sd):
        sd.width, sd.height = 9, 7
        return sd

    two = small(P.scene())
    first, second, _, last = P.proto_meshes(two)
    pos = {m: two.meshes[m].positions for m in (first, second, last)}
    at_rest = np.array(two.instance_xform, np.float64)

    def current_frame(sc):
        # the mark under the moved transforms, the current frame under the description's
        sc.mark_frame()
        sc.set_instance_transforms(at_rest)

    def shutter_meshes(sc):
        # every slice's pose differs from the transforms the placements' records were made from, and the first prototype
        # deforms: the update makes the records again (new_records).  Afterwards the scene is at the current frame again:
        # every line of this step equals the step before's
        sc.render_shutter_meshes([(first, pos[first], M.smooth(pos[first]))], spp=4, max_depth=DEPTH, seed=SEED, slices=2)

    flat, lamp = M.emissive_scene()
    old = flat.meshes[lamp].positions
    return [
        ("protos", two, [
            ("created", lambda sc: None),
            ("set_instance_transforms", lambda sc: sc.set_instance_transforms(moved_transforms(two))),
            # (a run of two untouched prototypes between moved ones)
            ("update_first_and_last", lambda sc: sc.update_meshes({first: M.smooth(pos[first]), last: M.smooth(pos[last])})),
            # (untouched runs on both sides, with different shifts: half_shrunk changes the tree's node count)
            ("update_second", lambda sc: sc.update_meshes({second: P.half_shrunk(pos[second])})),
            ("mark_and_current_frame", current_frame),
            ("render_shutter_meshes", shutter_meshes),
        ]),
        ("emissive", small(flat), [
            ("created", lambda sc: None),
            ("set_mesh_vertices", lambda sc: sc.set_mesh_vertices({lamp: (M.smooth(old) - (0.0, 0.15, 0.0), -M.bent_grid(6)[2][::-1].copy())})),
        ]),
    ]


def resident():
    arrays = ("nodes", "prims", "inst_trace")
    sides = {D.TAKE_PRECISION_F32: "f32", D.TAKE_PRECISION_F64: "f64"}
    for name, sd, steps in resident_steps():
        for precision, code in PRECISIONS.items():
            sc = capi.Scene(sd, precision=code, builder=D.TAKE_BUILDER_DEVICE_LBVH)
            try:
                for step, change in steps:
                    change(sc)
                    where = f"resident/{name}/{precision}/{step}"
                    for side, side_name in sides.items():
                        if precision != "mixed" and side_name != precision:
                            continue
                        tree = sc.debug_tree(side)
                        for a in arrays:
                            print(f"{where}/{side_name}.{a} {digest(tree[a])}", flush=True)
                        print(f"{where}/{side_name}.info {digest({k: np.asarray(v) for k, v in tree.items() if k not in arrays})}", flush=True)
                    print(f"{where}/render {digest(sc.render(spp=2, max_depth=DEPTH, seed=SEED))}", flush=True)
            finally:
                sc.close()


def main():
    assert capi.device_count() >= 1
    if "--resident" in sys.argv[1:]:
        return resident()
    compressed = []  # the scenes on 64-byte 4-wide nodes: the only ones whose round 0 has the fused route
    for name, sd in scene_set().items():
        for precision, code in PRECISIONS.items():
            sc = capi.Scene(sd, precision=code)
            try:
                if sc.debug_tree()["node_format"] == D.NODE_FORMAT_Q4:
                    compressed.append(f"{name}/{precision}")
                for label, call in image_calls(sc, name, precision):
                    print(f"{name}/{precision}/{label} {digest(call())}", flush=True)
                if name in COUNTED_SCENES:
                    sc.set_instrumentation(timing=True, counting=True)
                    for label, call in counted_calls(sc, name, precision):
                        call()
                        c = sc.counters()
                        print(f"counters {name}/{precision}/{label} " + " ".join(f"{k}={int(c[k])}" for k in COUNTER_FIELDS), flush=True)
            finally:
                sc.close()
    print(f"scenes on compressed 4-wide nodes: {' '.join(compressed)}", file=sys.stderr)
    assert compressed, "no scene of the set takes the fused route by default: the two settings of TAKE_HIP_CAMERA_FUSED would run the same launches"


if __name__ == "__main__":
    main()

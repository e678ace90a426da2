"""scene_create phases at 10M triangles (TAKE_HIP_VERBOSE): where the setup time goes, host SAH vs device LBVH.
usage: tools/diag_setup.py [n_triangles] [f32|f64|mixed] [repetitions] [device|host|both]
       tools/diag_setup.py instanced PxTxN [f32|f64|mixed] [repetitions] [device|host|both]
           a two-level scene: P prototypes of T triangles each, N placements in all (round-robin over the prototypes)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["TAKE_HIP_VERBOSE"] = "1"
from take_amd import capi, scenes
from take_amd import cdefs as D
instanced = len(sys.argv) > 1 and sys.argv[1] == "instanced"
if instanced:
    n_protos, n_tris, n_placed = (int(x) for x in sys.argv[2].split("x"))
    del sys.argv[1]
n = int(sys.argv[1]) if len(sys.argv) > 1 and not instanced else 10_000_000
pname = sys.argv[2] if len(sys.argv) > 2 else "f32"
precision = {"f32": D.TAKE_PRECISION_F32, "f64": D.TAKE_PRECISION_F64, "mixed": D.TAKE_PRECISION_MIXED}[pname]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
which = sys.argv[4] if len(sys.argv) > 4 else "both"
t = time.time()
if instanced:
    sd = scenes.instanced_scene(n_placed, n_tris, 640, 360, spp=1)
    protos = [sd.instance_mesh[0]] + [sd.add_prototype(*scenes.soup_triangles(n_tris, 5000 + k, 0.07, 0.012), 0) for k in range(1, n_protos)]
    sd.instance_mesh = [protos[i % n_protos] for i in range(n_placed)]
else:
    sd = scenes.soup_scene(n, 640, 360, spp=1)
print(f"scene generation {time.time()-t:.2f} s", flush=True)
for b, name in ((D.TAKE_BUILDER_DEVICE_LBVH, "device"), (D.TAKE_BUILDER_HOST_SAH, "host")):
    if which not in ("both", name):
        continue
    for rep in range(reps):
        t = time.time(); sc = capi.Scene(sd, precision=precision, builder=b); dt = time.time() - t
        print(f"{pname} builder {name} rep {rep}: scene_create {dt:.3f} s  {sc.stats()}", flush=True)
        sc.close()

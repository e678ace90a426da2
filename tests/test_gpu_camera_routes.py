"""Round 0's two routes to the camera rays give the same images (take_amd/csrc/tk_render.hip: start_batch; DESIGN.md
par. 4e).  By default the trace launch of round 0 makes the camera rays itself where it can (CameraIo); under
TAKE_HIP_CAMERA_FUSED=0 k_generate always writes them first.  The variable is read once per process, so
tools/render_digests.py runs twice, each time as a fresh child process, and every image digest of the two runs is
compared line by line: np.array_equal through a hash.

Why equality is the bar: tests/test_gpu_rays.py pins render == k_generate's exported rays through render_rays bit for
bit, and shade_path treats k == 0 the same on both routes.  The "counters" lines are left out: counting keeps the
generate route under either setting.  No image label is left out: measured on the commit before the routes got one
place to be decided in, all labels — the feature planes, the camera-ray export, the motion pass and the shutter among
them — were equal under the two settings.

What this does not show: that the default child took the fused route at all.  The library has no observable for the
route short of counting, and counting is what forces the generate route; the tool only asserts that its scenes are on
the node format the fused route needs, which holds under either setting.  A change that made start_batch never leave
the rays to the trace launch would pass here — it shows in the launch lists of a kernel trace, and in the time of small
renders (DESIGN.md par. 4n), not in this test."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 240
MUST_COMPARE = ("render", "render_accumulate", "render_adaptive", "render_rays_sets", "render_rays_normalize")


def run_tool(fused):
    """the tool's image lines {label: digest} from a fresh child process; a child that ends on a signal, a non-zero status
    or the timeout fails the test here"""
    env = dict(os.environ)
    env.pop("TAKE_HIP_CAMERA_FUSED", None)
    if not fused:
        env["TAKE_HIP_CAMERA_FUSED"] = "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_digests.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, (fused, r.returncode, r.stderr[-2000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln and not ln.startswith("counters ")]
    assert lines and all(len(ln) == 2 and len(ln[1]) == 64 for ln in lines), r.stdout[-2000:]
    return dict(lines), [ln[0] for ln in lines]


def test_the_fused_and_the_generate_route_give_the_same_bytes():
    fused, order = run_tool(True)  # (a failure here ends the test: the second child is not started)
    unfused, order_unfused = run_tool(False)
    assert order == order_unfused
    calls = {label.rsplit("/", 1)[1] for label in order}
    assert calls.issuperset(MUST_COMPARE)
    differ = [label for label in order if fused[label] != unfused[label]]
    assert not differ, differ

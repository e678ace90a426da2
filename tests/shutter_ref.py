"""numpy float64 restatement of the shutter (include/take_hip.h: take_hip_shutter_plan, take_hip_shutter_pose; DESIGN.md
par. 4l; the device text is take_amd/csrc/tk_shutter.h): the plan of a render over a shutter, and the pose of camera and
placements at a scene time.  Every operation is one IEEE double operation in the order written, as the library's."""
import copy

import numpy as np


def plan(spp, open=0.0, close=1.0, slices=0):
    """-> (first_sample: K + 1 ints, time: K floats); K = slices capped at spp, <= 0: min(spp, 16)"""
    spp = int(spp)
    K = min(spp, 16) if slices <= 0 else min(int(slices), spp)
    first = [k * spp // K for k in range(K + 1)]
    o, c = np.float64(open), np.float64(close)
    time = [o + (c - o) * ((np.float64(k) + np.float64(0.5)) / np.float64(K)) for k in range(K)]
    return np.array(first, np.int32), np.array(time, np.float64)


def lerp(t, a, b):
    """(1 - t) a + t b: `1 - t` rounded once, two products, one sum; where the ends are equal, the end itself (b)"""
    t, a, b = np.float64(t), np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.float64(1.0) - t
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(a == b, b, s * a + t * b)


def pose_camera(t, marked, current):
    """marked, current: anything with lookfrom, lookat, up, vfov -> the same four, lerped component by component"""
    return {"lookfrom": lerp(t, marked.lookfrom, current.lookfrom), "lookat": lerp(t, marked.lookat, current.lookat),
            "up": lerp(t, marked.up, current.up), "vfov": float(lerp(t, marked.vfov, current.vfov))}


def pose_xforms(t, marked, current):
    """(n, 3, 4) object -> world transforms, lerped entry by entry (a rotation moves along its chord)"""
    return lerp(t, np.asarray(marked, np.float64).reshape(-1, 3, 4), np.asarray(current, np.float64).reshape(-1, 3, 4))


def singular(x):
    """the re-pose's rule for one 3x4 transform: an entry that is not finite, or |det| of the linear part <= 1e-300 (the
    determinant in the library's expression)"""
    m = np.asarray(x, np.float64).reshape(3, 4)
    det = m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])
    return bool(not np.isfinite(m).all() or not abs(det) > 1e-300)


def posed_scene(sd, t, marked_camera, marked_xforms):
    """a copy of the scene description `sd` (the current frame) at scene time t: marked_camera — anything with lookfrom,
    lookat, up, vfov; marked_xforms — (n, 3, 4) or None for a scene without placements"""
    out = copy.copy(sd)
    cam = pose_camera(t, marked_camera, sd)
    out.lookfrom, out.lookat, out.up, out.vfov = tuple(cam["lookfrom"]), tuple(cam["lookat"]), tuple(cam["up"]), cam["vfov"]
    if marked_xforms is not None:
        out.instance_xform = list(pose_xforms(t, marked_xforms, np.stack(sd.instance_xform)))
    return out

"""numpy restatement of the temporal accumulation (include/take_hip.h: take_hip_temporal_accumulate*;
take_amd/csrc/tk_temporal.h), templated on the dtype, with the operation order of the specification (DESIGN.md par. 4i):
the bilinear footprint, its weights, their sum and the colour in the dtype, the moments and the history length in double;
taps in the order (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).  And of the motion pass's projection
(take_hip_render_motion*; take_amd/csrc/tk_motion.h) in float64.  Also the planes and motion fields the CPU and GPU tests
share."""
import numpy as np

import denoise_var_ref as V

DEFAULTS = dict(max_history=64, depth_tol=0.05)
PLANES = ("rgb", "count", "m1", "m2", "depth", "shape_id")


def accumulate(cur, hist, prev_xy, prev_depth=None, dtype=None, max_history=0, depth_tol=0.0, debug=False):
    """cur / hist: dicts of rgb (H, W, 3), count int32, m1 / m2 float64 (H, W) and optionally depth (H, W), shape_id int32
    (H, W); hist None = no history; prev_xy (H, W, 2), prev_depth (H, W) or None -> the accumulated frame, a dict of the
    same planes in `dtype` (default: cur's rgb's).  Options <= 0 take the default, as in TakeTemporalOpts.  debug: also
    "_nr", n_r + 0.5 before the floor (NaN where the output is the current frame)."""
    T = np.dtype(dtype or np.asarray(cur["rgb"]).dtype).type
    mh = int(max_history) if max_history > 0 else DEFAULTS["max_history"]
    tol = T(depth_tol if depth_tol > 0 else DEFAULTS["depth_tol"])
    rgb = np.array(cur["rgb"], T)
    c = np.array(cur["count"], np.int32)
    m1c, m2c = np.array(cur["m1"], np.float64), np.array(cur["m2"], np.float64)
    h, w = c.shape
    out = {"rgb": rgb.copy(), "count": c.copy(), "m1": m1c.copy(), "m2": m2c.copy()}
    if cur.get("depth") is not None:
        out["depth"] = np.array(cur["depth"], T)
    if cur.get("shape_id") is not None:
        out["shape_id"] = np.array(cur["shape_id"], np.int32)
    if debug:
        out["_nr"] = np.full((h, w), np.nan)
    if hist is None:
        return out
    hrgb, hn = np.array(hist["rgb"], T), np.array(hist["count"], np.int32)
    hm1, hm2 = np.array(hist["m1"], np.float64), np.array(hist["m2"], np.float64)
    ids = cur.get("shape_id") is not None and hist.get("shape_id") is not None
    depths = hist.get("depth") is not None and prev_depth is not None
    pxy = np.array(prev_xy, T)
    with np.errstate(all="ignore"):
        fx, fy = pxy[..., 0] - T(0.5), pxy[..., 1] - T(0.5)
        ok = (fx >= T(-1)) & (fx < T(w)) & (fy >= T(-1)) & (fy < T(h))  # (false for a NaN)
        fx, fy = np.where(ok, fx, T(0)), np.where(ok, fy, T(0))
        flx, fly = np.floor(fx), np.floor(fy)
        tx, ty = fx - flx, fy - fly
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        wx, wy = (T(1) - tx, tx), (T(1) - ty, ty)
        W = np.zeros((h, w), T)
        hc = np.zeros((h, w, 3), T)
        a, b, nr = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        if depths:
            pd, hd = np.array(prev_depth, T), np.array(hist["depth"], T)
        for j in range(2):
            for i in range(2):
                wgt = wx[i] * wy[j]
                qx, qy = x0 + i, y0 + j
                valid = ok & (wgt > 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                nq = hn[qy, qx]
                valid &= nq > 0
                if ids:
                    valid &= np.asarray(hist["shape_id"])[qy, qx] == np.asarray(cur["shape_id"])
                if depths:
                    valid &= np.abs(hd[qy, qx] - pd) <= tol * pd
                wd, nd = wgt.astype(np.float64), nq.astype(np.float64)
                hc = np.where(valid[..., None], hc + wgt[..., None] * hrgb[qy, qx], hc)
                a = np.where(valid, a + wd * (hm1[qy, qx] / nd), a)
                b = np.where(valid, b + wd * (hm2[qy, qx] / nd), b)
                nr = np.where(valid, nr + wd * nd, nr)
                W = np.where(valid, W + wgt, W)
        has = W > 0
        Wd = W.astype(np.float64)
        hc = hc / W[..., None]
        a, b, nr = a / Wd, b / Wd, nr / Wd
        half = nr + 0.5
        rounded = np.floor(half)
        nh = np.where(rounded < mh, rounded, mh)
        nh = np.where(has, nh, 0).astype(np.int32)
        n = nh + c
        Rh, Rc, Rn = nh.astype(T), c.astype(T), n.astype(T)
        acc = (hc * Rh[..., None] + rgb * Rc[..., None]) / Rn[..., None]
        out["rgb"] = np.where(has[..., None], acc, rgb)
        out["count"] = np.where(has, n, c).astype(np.int32)
        out["m1"] = np.where(has, a * nh.astype(np.float64) + m1c, m1c)
        out["m2"] = np.where(has, b * nh.astype(np.float64) + m2c, m2c)
        if debug:
            out["_nr"] = np.where(has, half, np.nan)
    assert out["rgb"].dtype == T
    return out


# ------------------------------------------------------------------ the motion pass's projection, float64
def camera(lookfrom, lookat, up, vfov, width, height):
    """the camera record of the library (make_camera) in float64"""
    f, at, up = (np.asarray(v, np.float64) for v in (lookfrom, lookat, up))
    vh = 2.0 * np.tan(vfov / 180.0 * np.pi / 2.0)
    w = (f - at) / np.linalg.norm(f - at)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    return {"u": u, "v": v, "w": w, "from": f, "vw": vh / height * width, "vh": vh, "width": int(width), "height": int(height)}


def centre_rays(cam):
    """-> (H, W, 3) unit directions of the rays through the pixel centres, row 0 = top (origin: cam["from"])"""
    W, H = cam["width"], cam["height"]
    row, x = np.mgrid[0:H, 0:W]
    y = H - 1 - row  # the render loop's y: 0 = bottom
    d = (cam["u"] * (((x + 0.5) / W - 0.5) * cam["vw"])[..., None] + cam["v"] * (((y + 0.5) / H - 0.5) * cam["vh"])[..., None]) - cam["w"]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def affine(m, p):
    """(..., 3, 4) maps on (..., 3) points"""
    return np.einsum("...ij,...j->...i", m[..., :3], p) + m[..., 3]


def inverse_affine(m):
    m = np.asarray(m, np.float64)
    a = np.linalg.inv(m[..., :3])
    return np.concatenate([a, -np.einsum("...ij,...j->...i", a, m[..., 3])[..., None]], axis=-1)


def reproject(depth, shape_id, cam_cur, cam_mark, shape_base=None, xf_cur=None, xf_mark=None):
    """The motion pass in float64 on the centre rays of cam_cur: depth (H, W) = t of the hit (0 for a miss), shape_id
    (H, W) (-1 = miss) -> prev_xy (H, W, 2), prev_depth (H, W).  Placements: shape_base = the first shape id of every
    placement and one past the last (n + 1 ascending values), xf_cur / xf_mark (n, 3, 4) their transforms now / at the mark."""
    depth, shape_id = np.asarray(depth, np.float64), np.asarray(shape_id)
    d = centre_rays(cam_cur)
    hit = shape_id >= 0
    P = cam_cur["from"] + d * depth[..., None]
    if shape_base is not None:
        shape_base = np.asarray(shape_base)
        inst = np.searchsorted(shape_base, shape_id, side="right") - 1
        placed = hit & (shape_id >= shape_base[0]) & (shape_id < shape_base[-1])
        k = np.clip(inst, 0, len(shape_base) - 2)
        moved = affine(np.asarray(xf_mark, np.float64)[k], affine(inverse_affine(xf_cur)[k], P))
        P = np.where(placed[..., None], moved, P)
    e = np.where(hit[..., None], P - cam_mark["from"], d)
    with np.errstate(all="ignore"):
        z = -(e @ cam_mark["w"])
        sx = ((e @ cam_mark["u"]) / z / cam_mark["vw"] + 0.5) * cam_mark["width"]
        sy = ((e @ cam_mark["v"]) / z / cam_mark["vh"] + 0.5) * cam_mark["height"]
    seen = z > 0
    xy = np.where(seen[..., None], np.stack([sx, cam_mark["height"] - sy], -1), -2.0)
    pd = np.where(seen & hit, np.linalg.norm(e, axis=-1), 0.0)
    return xy, pd


# ------------------------------------------------------------------ the planes and motion fields of the tests
MOTIONS = ("identity", "integer", "fraction", "leaving", "random", "nowhere")


def motion(name, width, height):
    """-> prev_xy (H, W, 2) float64: the pixel centres moved by the named field"""
    y, x = np.mgrid[0:height, 0:width]
    c = np.stack([x + 0.5, y + 0.5], -1).astype(np.float64)
    if name == "identity":
        return c
    if name == "integer":
        return c + (3.0, -2.0)
    if name == "fraction":
        return c + (0.25, -0.6)
    if name == "leaving":  # off the right and the top edge for the far half of the image
        return c + (width / 2 + 0.3, -(height / 2 + 0.3))
    if name == "random":
        return c + np.random.default_rng(11).uniform(-3.0, 3.0, c.shape)
    if name == "nowhere":  # identity, with a block of (-2, -2)
        c[height // 3:height // 3 + max(1, height // 4), width // 5:width // 5 + max(1, width // 3)] = -2.0
        return c
    raise KeyError(name)


_FRAMES = {}


def frames(width, height):
    """The two frames the tests share, made once per size and never written to: cur = denoise_var_ref.sampled_planes, hist
    = its variant (other counts, a block without variance) with a patch of count == 0; shape ids in stripes (5 columns
    wide in cur, the history's shifted by one column, so some taps fail); a depth plane with a step at mid-width (2 | 3,
    with a gentle slope), the history's the same, prev_depth 1 % off it — inside the default tolerance except across the
    step.  -> (cur, hist, prev_depth), float64 planes."""
    if (width, height) not in _FRAMES:
        a, b = V.sampled_planes(width, height), V.sampled_planes(width, height, variant=True)
        y, x = np.mgrid[0:height, 0:width]
        depth = np.where(x < width // 2, 2.0, 3.0) + 0.01 * y
        cur = {"rgb": a["rgb"], "count": a["count"], "m1": a["m1"], "m2": a["m2"], "depth": depth, "shape_id": ((x // 5) % 3).astype(np.int32)}
        hist = {"rgb": b["rgb"] * 0.9, "count": b["count"].copy(), "m1": b["m1"] * 0.9, "m2": b["m2"] * 0.81, "depth": depth.copy(),
                "shape_id": (((x + 1) // 5) % 3).astype(np.int32)}
        patch = (slice(height // 4, height // 2), slice(width // 4, width // 2))
        hist["count"][patch] = 0
        hist["m1"][patch] = 0.0
        hist["m2"][patch] = 0.0
        _FRAMES[width, height] = (cur, hist, depth * 1.01)
    return _FRAMES[width, height]


def cast(f, dtype, tests=("depth", "shape_id")):
    """a frame's planes, contiguous: rgb and depth in `dtype`, count and shape_id int32, the moments float64; tests: which
    of depth / shape_id to keep"""
    out = {"rgb": np.ascontiguousarray(f["rgb"], dtype), "count": np.ascontiguousarray(f["count"], np.int32),
           "m1": np.ascontiguousarray(f["m1"], np.float64), "m2": np.ascontiguousarray(f["m2"], np.float64)}
    if "depth" in tests and f.get("depth") is not None:
        out["depth"] = np.ascontiguousarray(f["depth"], dtype)
    if "shape_id" in tests and f.get("shape_id") is not None:
        out["shape_id"] = np.ascontiguousarray(f["shape_id"], np.int32)
    return out

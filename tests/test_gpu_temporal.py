"""Temporal reprojection and accumulation on the device (take_hip_scene_mark_frame, take_hip_render_motion*,
take_hip_temporal_accumulate*, take_hip_render_temporal*: include/take_hip.h; kernels: take_amd/csrc/tk_motion.h,
tk_temporal.h) against the numpy restatement of its specification (tests/temporal_ref.py).

Accumulate: the cases of tests/test_temporal_cpu.py (1x1, 7x1, 1x7, 37x23, 130x70 — more than one wave per row, no
multiple of the 64 x 4 block; every motion field, the id and depth tests on and off, max_history 1 and 64, no history).
Bars, those of tests/test_gpu_denoise_var.py: f64 planes 1e-9 * max(1, max|ref|), f32 planes 1e-5 * max(1, max|ref|)
against the f64 restatement of the float-rounded inputs; count equal to the restatement's in the planes' own dtype (the
same operations), except that a pixel where n_r + 0.5 lies within 1e-9 of an integer may differ by one, on at most 0.1 %
of the pixels.  In f32 the values are held to the f64 restatement on the pixels where the f32 and the f64 restatement give
the same count (tests/test_temporal_cpu.py holds the others to the same 0.1 %), to the f32 restatement on all.

Motion: shape_id and depth against take_hip_trace_closest of centre rays made in numpy (ids equal on >= 99.5 % of the
pixels: last-bit differences of the ray direction move a ray across an edge); prev_xy and prev_depth against the float64
restatement applied to the device's own depth and shape_id, the caller's cameras and the caller's transforms.  F64 bars:
1e-9 * width pixels, 1e-9 relative.  F32 bars: F32_XY_BAR pixels and F32_REL_BAR relative — the next power of ten above
8 x the largest difference measured on these scenes on an MI355X (DESIGN.md par. 4i has both numbers); the pixel bar has
to stay below 0.01 pixel, where a bilinear weight visibly changes.

Everything the library is compared with itself on is np.array_equal."""
import copy

import numpy as np
import pytest
import torch  # (before the library is loaded: the two share one HIP runtime only in this order)

import temporal_ref as T
from helpers import golden_scene, rays_to_abi, rmse
from take_amd import capi, scenes
from take_amd import cdefs as D
from test_temporal_cpu import CAP, CASES, SIZES, case_id, check, inputs, widen

pytestmark = pytest.mark.gpu
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
GUIDES = ("albedo", "normal", "depth")
STATS = ("count", "m1", "m2")
DEPTH = 6
# measured on an MI355X over the motion scenes below: prev_xy 1.03e-5 pixel at most (8 x = 8.2e-5); depth against the
# trace hook's t 4.54e-6 relative at most (8 x = 3.6e-5), prev_depth 2.7e-7
F32_XY_BAR, F32_REL_BAR = 1e-4, 1e-4
assert F32_XY_BAR < 0.01


# ------------------------------------------------------------------ accumulate against the restatement
def check_count(got, ref_debug, label):
    """count equal; a pixel where n_r + 0.5 is within 1e-9 of an integer may differ by one, on at most 0.1 % of the pixels"""
    diff = got["count"] != ref_debug["count"]
    if diff.any():
        half = ref_debug["_nr"]
        near = np.abs(half - np.round(half)) <= 1e-9
        print(f"{label}: {int(diff.sum())} pixels differ in count")
        assert (near[diff]).all() and (np.abs(got["count"].astype(np.int64) - ref_debug["count"])[diff] == 1).all(), label
        assert diff.sum() <= CAP * diff.size, label
    return ~diff


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_f64_against_the_restatement(c):
    cur, hist, xy, pd, mh = inputs(c, np.float64)
    got = capi.temporal_accumulate(cur, hist, xy, pd, max_history=mh)
    ref = T.accumulate(cur, hist, xy, pd, max_history=mh, debug=True)
    assert got["rgb"].dtype == np.float64 and set(got) == set(cur)
    same = check_count(got, ref, case_id(c))
    check(got, ref, 1e-9, "device f64 " + case_id(c), where=same)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_f32_against_the_restatements(c):
    cur, hist, xy, pd, mh = inputs(c, np.float32)
    got = capi.temporal_accumulate(cur, hist, xy, pd, max_history=mh)
    ref32 = T.accumulate(cur, hist, xy, pd, max_history=mh, debug=True)
    ref64 = T.accumulate(widen(cur), widen(hist), xy.astype(np.float64), None if pd is None else pd.astype(np.float64), max_history=mh)
    assert got["rgb"].dtype == np.float32
    same = check_count(got, ref32, case_id(c))
    check(got, ref64, 1e-5, "device f32 against f64 " + case_id(c), where=same & (ref32["count"] == ref64["count"]))
    check(got, widen({k: v for k, v in ref32.items() if k != "_nr"}), 1e-5, "device f32 against the f32 restatement " + case_id(c), where=same)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_without_a_history_the_frame_comes_back(size, dtype):
    cur, _, _ = T.frames(*size)
    c = T.cast(cur, dtype)
    out = capi.temporal_accumulate(c, None, T.motion("identity", *size).astype(dtype))
    assert all(np.array_equal(out[k], c[k]) for k in c)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_repeats_twins_in_place_and_null_options_are_the_same_bits(dtype):
    w, h = 130, 70
    cur, hist, pd = T.frames(w, h)
    c, hh, xy, pd = T.cast(cur, dtype), T.cast(hist, dtype), T.motion("random", w, h).astype(dtype), pd.astype(dtype)
    first = capi.temporal_accumulate(c, hh, xy, pd)
    again = capi.temporal_accumulate(c, hh, xy, pd)
    assert all(np.array_equal(first[k], again[k]) for k in first), "a repeated call"
    for label, kw in (("opts = NULL against the explicit defaults", D.TEMPORAL_DEFAULTS), ("opts = NULL against all fields 0", dict(opts=D.TakeTemporalOpts()))):
        a = capi.temporal_accumulate(c, hh, xy, pd, **kw)
        assert all(np.array_equal(first[k], a[k]) for k in first), label
    assert not np.array_equal(first["count"], capi.temporal_accumulate(c, hh, xy, pd, max_history=3)["count"])
    precision = F32 if dtype == np.float32 else F64
    tc, th = ({k: torch.from_numpy(v).cuda() for k, v in f.items()} for f in (c, hh))
    txy, tpd = torch.from_numpy(xy).cuda(), torch.from_numpy(pd).cuda()
    out = {k: torch.full_like(v, -7) for k, v in tc.items()}
    capi.temporal_accumulate_device(tc, th, txy, tpd, w, h, precision, out=out)
    torch.cuda.synchronize()
    assert all(np.array_equal(first[k], out[k].cpu().numpy()) for k in first), "host twin against device twin"
    assert all(np.array_equal(tc[k].cpu().numpy(), c[k]) for k in c) and all(np.array_equal(th[k].cpu().numpy(), hh[k]) for k in hh), "out of place leaves the inputs alone"
    capi.temporal_accumulate_device(tc, th, txy, tpd, w, h, precision)  # out = None: d_out == d_cur
    torch.cuda.synchronize()
    assert all(np.array_equal(first[k], tc[k].cpu().numpy()) for k in first), "in place against out of place"


# ------------------------------------------------------------------ the motion pass
def two_level_scene():
    return scenes.instanced_scene(12, 300, 48, 32, spp=2, max_depth=DEPTH)


def small(name):
    if name == "two-level":
        return two_level_scene()
    sd = copy.copy(golden_scene(name))
    sd.width, sd.height = 48, 32
    return sd


def camera_of(sd):
    return dict(lookfrom=tuple(sd.lookfrom), lookat=tuple(sd.lookat), up=tuple(sd.up), vfov=float(sd.vfov))


def moved_camera(sd, k=1):
    """a small translation plus rotation, k times over"""
    f, a = np.asarray(sd.lookfrom, np.float64), np.asarray(sd.lookat, np.float64)
    d = float(np.linalg.norm(a - f))
    return dict(lookfrom=tuple(f + k * d * np.array([0.02, 0.01, -0.015])), lookat=tuple(a + k * d * np.array([-0.01, 0.015, 0.0])), up=tuple(sd.up), vfov=float(sd.vfov))


def moved_transforms(sd, k=1):
    """every placement turned a little about z and pushed a little, k times over"""
    a = 0.05 * k
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    out = []
    for i, x in enumerate(sd.instance_xform):
        t = x[:, 3] + k * np.array([0.01, -0.008, 0.005]) * (1 + i % 3)
        out.append(np.concatenate([rz @ x[:, :3], t[:, None]], axis=1))
    return np.stack(out)


def shape_base(sd):
    faces = [sd.meshes[m].indices.shape[0] for m in sd.instance_mesh]
    return sd.n_shapes + np.concatenate([[0], np.cumsum(faces)]) if faces else None


def numpy_camera(sd, cam):
    return T.camera(cam["lookfrom"], cam["lookat"], cam["up"], cam["vfov"], sd.width, sd.height)


def traced(sc, sd, cam, precision):
    """take_hip_trace_closest of the centre rays of `cam`, made in numpy -> shape_id, t (H, W)"""
    c = numpy_camera(sd, cam)
    d = T.centre_rays(c).reshape(-1, 3)
    n = d.shape[0]
    eps = 1e-4 if precision == F32 else 1e-7
    rays = np.concatenate([np.broadcast_to(c["from"], (n, 3)), d, np.full((n, 1), eps), np.full((n, 1), np.inf)], axis=1)
    hits = sc.trace_closest(rays_to_abi(rays, 0 if precision == F32 else 1))
    return hits["shape_id"].reshape(sd.height, sd.width), hits["t"].reshape(sd.height, sd.width).astype(np.float64)


MOTION_SCENES = [("cbox", F32), ("cbox", F64), ("cbox", MIXED), ("two-level", F32), ("two-level", F64)]


@pytest.mark.parametrize("name,precision", MOTION_SCENES, ids=[f"{n}-{p}" for n, p in MOTION_SCENES])
def test_motion_against_the_trace_hook_and_the_restatement(name, precision):
    sd = small(name)
    W, H = sd.width, sd.height
    dtype = np.float32 if precision == F32 else np.float64
    xy_bar, rel_bar = (F32_XY_BAR, F32_REL_BAR) if precision == F32 else (1e-9 * W, 1e-9)
    cam0, cam1 = camera_of(sd), moved_camera(sd)
    base = shape_base(sd)
    xf0 = np.stack(sd.instance_xform) if base is not None else None
    xf1 = moved_transforms(sd) if base is not None else None
    sc = capi.Scene(sd, precision=precision)
    try:
        with pytest.raises(capi.TakeError) as e:
            sc.render_motion()
        assert e.value.code == D.TAKE_E_INVALID and "no marked frame" in str(e.value)
        # what must be the same bits afterwards
        plain = sc.render(spp=3, max_depth=DEPTH, seed=5)
        feats = sc.render_features(2, seed=5)
        sc.mark_frame()
        # nothing changed since the mark: prev_xy is the pixel centres, prev_depth the depth
        still = sc.render_motion()
        assert still["prev_xy"].dtype == dtype and still["prev_xy"].shape == (H, W, 2) and still["shape_id"].dtype == np.int32
        hit = still["shape_id"] >= 0
        assert hit.mean() > 0.3 and ((still["depth"] > 0) == hit).all()
        d_xy = float(np.abs(still["prev_xy"].astype(np.float64) - T.motion("identity", W, H)).max())
        d_pd = float(np.abs(still["prev_depth"][hit].astype(np.float64) / still["depth"][hit] - 1).max())
        print(f"{name}-{precision} nothing moved: prev_xy off the centres by {d_xy:.3e} pixel (bar {xy_bar:.1e}), prev_depth off depth by {d_pd:.3e} relative (bar {rel_bar:.1e})")
        assert d_xy <= xy_bar and d_pd <= rel_bar and (still["prev_depth"][~hit] == 0).all()
        if base is not None:
            assert (still["shape_id"] >= sd.n_shapes).mean() > 0.02, "placements are seen"
        # a progressive sequence goes on across the pass
        tdtype = torch.float32 if precision == F32 else torch.float64
        buf = torch.zeros(plain.shape, dtype=tdtype, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=5, restart=True) == 2
        assert all(np.array_equal(still[k], v) for k, v in sc.render_motion().items()), "a repeated call"
        assert sc.render_accumulate(buf.data_ptr(), 1, DEPTH, seed=5) == 3
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), plain), "a progressive sequence across the motion pass"
        assert np.array_equal(sc.render(spp=3, max_depth=DEPTH, seed=5), plain), "a render afterwards"
        after = sc.render_features(2, seed=5)
        assert all(np.array_equal(after[k], feats[k]) for k in feats), "the feature planes afterwards"
        # the scene moves; the mark stays
        sc.set_camera(**cam1)
        if base is not None:
            sc.set_instance_transforms(xf1)
        got = sc.render_motion()
        ids, t = traced(sc, sd, cam1, precision)
        agree = got["shape_id"] == ids
        print(f"{name}-{precision}: ids equal to the trace hook's on {100 * agree.mean():.3f} % of the pixels")
        assert agree.mean() >= 0.995
        both = agree & (ids >= 0)
        d_t = float(np.abs(got["depth"][both].astype(np.float64) / t[both] - 1).max())
        print(f"{name}-{precision}: depth off the trace hook's t by {d_t:.3e} relative (bar {rel_bar:.1e})")
        assert d_t <= rel_bar and (got["depth"][got["shape_id"] < 0] == 0).all()
        want_xy, want_pd = T.reproject(got["depth"], got["shape_id"], numpy_camera(sd, cam1), numpy_camera(sd, cam0), base, xf1, xf0)
        d_xy = float(np.abs(got["prev_xy"].astype(np.float64) - want_xy).max())
        hit = got["shape_id"] >= 0
        d_pd = float(np.abs(got["prev_depth"][hit].astype(np.float64) / want_pd[hit] - 1).max())
        print(f"{name}-{precision} moved: prev_xy off the restatement by {d_xy:.3e} pixel (bar {xy_bar:.1e}), prev_depth by {d_pd:.3e} relative (bar {rel_bar:.1e})")
        assert d_xy <= xy_bar and d_pd <= rel_bar and (got["prev_depth"][~hit] == 0).all()
        assert float(np.abs(want_xy - T.motion("identity", W, H)).max()) > 0.5, "the move is seen"
        # a subset of the planes, and the device twin
        some = sc.render_motion(want=("prev_xy", "shape_id"))
        assert set(some) == {"prev_xy", "shape_id"} and all(np.array_equal(some[k], got[k]) for k in some)
        d = {"prev_depth": torch.zeros((H, W), dtype=tdtype, device="cuda"), "depth": torch.zeros((H, W), dtype=tdtype, device="cuda")}
        sc.render_motion_device(d)
        torch.cuda.synchronize()
        assert all(np.array_equal(d[k].cpu().numpy(), got[k]) for k in d), "device twin"
        # a camera turned by 180 degrees sees nothing of the marked frame
        f, a = np.asarray(cam0["lookfrom"]), np.asarray(cam0["lookat"])
        sc.set_camera(**dict(cam0, lookat=tuple(2 * f - a)))
        if base is not None:
            sc.set_instance_transforms(xf0)
        away = sc.render_motion()
        assert (away["prev_xy"] == -2).all() and (away["prev_depth"] == 0).all()
    finally:
        sc.close()


def moved_motion(sd, monkeypatch, fmt, move_placements):
    """the f32 motion planes after the camera (and the placements) moved, of a scene built under TAKE_HIP_NODES=fmt (None:
    unset) -> (planes, the node format the scene traverses)"""
    if fmt is None:
        monkeypatch.delenv("TAKE_HIP_NODES", raising=False)
    else:
        monkeypatch.setenv("TAKE_HIP_NODES", fmt)
    sc = capi.Scene(sd, precision=F32)
    try:
        sc.mark_frame()
        sc.set_camera(**moved_camera(sd))
        if move_placements:
            sc.set_instance_transforms(moved_transforms(sd))
        return sc.render_motion(), sc.debug_tree()["node_format"]
    finally:
        sc.close()


@pytest.mark.parametrize("name", ["cbox", "two-level"])
def test_motion_on_the_other_node_formats(name, monkeypatch):
    """the centre-ray launch has an instance of its own for every node format (the render's fused camera launch only for
    the default one): full-width and 8-wide nodes give the planes of the default format"""
    sd = small(name)
    for fmt, code in (("wide", D.NODE_FORMAT_WIDE), ("q8", D.NODE_FORMAT_Q8)):
        move_placements = bool(sd.instance_mesh) and fmt != "q8"  # (a scene of 8-wide nodes takes no new transforms)
        want, _ = moved_motion(sd, monkeypatch, None, move_placements)
        got, node_format = moved_motion(sd, monkeypatch, fmt, move_placements)
        assert node_format == code
        same = got["shape_id"] == want["shape_id"]
        hit = same & (want["shape_id"] >= 0)
        d_t = float(np.abs(got["depth"][hit].astype(np.float64) / want["depth"][hit] - 1).max())
        d_xy = float(np.abs(got["prev_xy"].astype(np.float64) - want["prev_xy"])[same].max())
        print(f"{name} {fmt}: ids equal on {100 * same.mean():.3f} % of the pixels, depth within {d_t:.3e} relative, prev_xy within {d_xy:.3e} pixel")
        assert same.mean() >= 0.995 and d_t <= F32_REL_BAR and d_xy <= F32_XY_BAR


# ------------------------------------------------------------------ the sequence
RULE = dict(spp=9, min_spp=4, step_spp=3, threshold=0.2, max_depth=DEPTH)
FILTER = dict(iterations=4, sigma_color=3.0)


def frame_by_hand(sc, history, seed, temporal=None):
    """one frame of take_hip_render_temporal through the public calls -> (the filtered image, the accumulated frame)"""
    img, st = sc.render_adaptive(seed=seed, stats=True, **RULE)
    if history is None:
        sc.mark_frame()
        m = sc.render_motion(want=("depth", "shape_id"))
        acc = dict(rgb=img, **st, **m)
    else:
        m = sc.render_motion()
        acc = capi.temporal_accumulate(dict(rgb=img, **st, depth=m["depth"], shape_id=m["shape_id"]), history, m["prev_xy"], m["prev_depth"], opts=temporal)
    planes = sc.render_features(RULE["min_spp"], seed=seed, want=GUIDES)
    out = capi.denoise_variance(acc["rgb"], acc["count"], acc["m1"], acc["m2"], **planes, **FILTER)
    sc.mark_frame()
    return out, acc


SEQUENCE_SCENES = [("cbox", F32), ("cbox", F64), ("mats", MIXED), ("two-level", F32)]


@pytest.mark.parametrize("name,precision", SEQUENCE_SCENES, ids=[f"{n}-{p}" for n, p in SEQUENCE_SCENES])
def test_render_temporal_is_the_calls_made_by_hand(name, precision):
    sd = small(name)
    base = shape_base(sd)
    temporal = D.temporal_opts(max_history=12, depth_tol=0.1)
    a, b = capi.Scene(sd, precision=precision), capi.Scene(sd, precision=precision)
    try:
        history, frames = None, []
        for k, seed in enumerate((5, 6, 7)):
            if k:
                for sc in (a, b):
                    sc.set_camera(**moved_camera(sd, k))
                    if base is not None:
                        sc.set_instance_transforms(moved_transforms(sd, k))
            if k == 1:  # a failing call in the middle leaves the next frame as it would have been
                with pytest.raises(capi.TakeError) as e:
                    a.render_temporal(seed=seed, temporal=temporal, **dict(RULE, spp=0), **FILTER)
                assert e.value.code == D.TAKE_E_INVALID
            got = a.render_temporal(seed=seed, temporal=temporal, **RULE, **FILTER)
            want, history = frame_by_hand(b, history, seed, temporal)
            assert got.dtype == want.dtype and np.array_equal(got, want), f"frame {k + 1}"
            if k == 0:
                assert np.array_equal(got, b.render_adaptive_denoised(seed=seed, **RULE, **FILTER)), "frame 1 is render_adaptive_denoised"
            else:
                _, st = b.render_adaptive(seed=seed, stats=True, **RULE)
                found = (history["count"] > st["count"]).mean()
                print(f"{name}-{precision} frame {k + 1}: {100 * found:.1f} % of the pixels found a history")
                assert found > 0.5, "most pixels found their history"
                assert not np.array_equal(got, b.render_adaptive_denoised(seed=seed, **RULE, **FILTER))
            frames.append(got)
        # restart: the third frame again, as a first frame; then the device twin goes on from it
        again = a.render_temporal(seed=7, restart=True, temporal=temporal, **RULE, **FILTER)
        first, history = frame_by_hand(b, None, 7)
        assert np.array_equal(again, first) and np.array_equal(again, b.render_adaptive_denoised(seed=7, **RULE, **FILTER)) and not np.array_equal(again, frames[2])
        buf = torch.zeros(again.shape, dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        rule = {k: v for k, v in RULE.items() if k not in ("spp", "max_depth")}
        a.render_temporal_device(buf, RULE["spp"], RULE["max_depth"], seed=8, temporal=temporal, **rule, **FILTER)
        torch.cuda.synchronize()
        want, history = frame_by_hand(b, history, 8, temporal)
        assert np.array_equal(buf.cpu().numpy(), want), "device twin"
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ end to end
def big_cbox():
    sd = copy.copy(golden_scene("cbox"))
    sd.width, sd.height = 128, 96
    return sd


def accumulated(sc, history, seed):
    """a 4-spp frame (every count 4) accumulated onto `history` through the scene-free calls, before any filter"""
    img, st = sc.render_adaptive(spp=4, min_spp=4, max_depth=8, seed=seed, stats=True)
    if history is None:
        sc.mark_frame()
        return img, dict(rgb=img, **st, **sc.render_motion(want=("depth", "shape_id")))
    m = sc.render_motion()
    return img, capi.temporal_accumulate(dict(rgb=img, **st, depth=m["depth"], shape_id=m["shape_id"]), history, m["prev_xy"], m["prev_depth"])


def test_four_static_frames_of_4_spp_are_closer_to_the_1024_spp_render():
    """a condition, not a measurement (the RMSEs are in DESIGN.md par. 4i): pooling 16 samples against 4 predicts a
    factor of 2; 1.5 leaves room for the pixels whose history is capped or rejected"""
    sc = capi.Scene(big_cbox(), precision=F32)
    try:
        truth = sc.render(spp=1024, max_depth=8, seed=11)
        history = None
        for seed in (1, 2, 3, 4):
            alone, history = accumulated(sc, history, seed)
            sc.mark_frame()
    finally:
        sc.close()
    assert (history["count"] == 16).mean() > 0.95
    single, pooled = rmse(alone, truth), rmse(history["rgb"], truth)
    print(f"cbox 128x96, static camera: RMSE to 1024 spp: frame 4 alone {single:.4f}, four frames accumulated {pooled:.4f} (alone / {single / pooled:.2f})")
    assert np.isfinite(history["rgb"]).all() and pooled < single / 1.5


def test_a_frame_after_a_two_pixel_move_is_closer_with_its_history():
    sd = big_cbox()
    f, a = np.asarray(sd.lookfrom, np.float64), np.asarray(sd.lookat, np.float64)
    cam = T.camera(f, a, sd.up, sd.vfov, sd.width, sd.height)
    step = cam["u"] * (2.0 * cam["vw"] / sd.width * float(np.linalg.norm(a - f)))  # about two pixels at the distance of lookat
    sc = capi.Scene(sd, precision=F32)
    try:
        _, history = accumulated(sc, None, 1)
        sc.mark_frame()
        sc.set_camera(lookfrom=tuple(f + step), lookat=tuple(a + step), up=tuple(sd.up), vfov=float(sd.vfov))
        truth = sc.render(spp=1024, max_depth=8, seed=11)
        alone, acc = accumulated(sc, history, 2)
        m = sc.render_motion(want=("prev_xy",))
    finally:
        sc.close()
    shift = np.abs(m["prev_xy"][..., 0].astype(np.float64) - T.motion("identity", sd.width, sd.height)[..., 0])
    single, pooled = rmse(alone, truth), rmse(acc["rgb"], truth)
    print(f"cbox 128x96, camera moved (median |dx| {np.median(shift):.2f} px): RMSE to 1024 spp of the new camera: frame 2 alone {single:.4f}, "
          f"accumulated {pooled:.4f} (alone / {single / pooled:.2f}); {100 * (acc['count'] > 4).mean():.1f} % of the pixels found a history")
    assert 1.0 < np.median(shift) < 3.0 and np.isfinite(acc["rgb"]).all() and pooled < single

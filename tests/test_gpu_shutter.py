"""Motion blur on the device (take_hip_render_shutter*, take_hip_shutter_pose: include/take_hip.h; the pose kernel:
take_amd/csrc/tk_shutter.h; DESIGN.md par. 4l) against the numpy restatement (tests/shutter_ref.py) and against renders
of scenes newly created at the restatement's poses.

Bars.  The pose: bit for bit.  No motion, one slice, before/after, batches, strips, the lens: np.array_equal.  K slices:
with N = spp, slice k = samples [a_k, b_k) and R_k(n) = render(spp = n) of a fresh scene at the pose of t_k,
    want = sum_k (b_k R_k(b_k) - a_k R_k(a_k)),   mag = sum_k (b_k |R_k(b_k)| + a_k |R_k(a_k)|)    (float64)
    |N got - want| <= 4 (N + 2) eps mag    per component, eps = 2^-53 (f64) or 2^-24 (f32):
every sample value is non-negative, so each of the at most N additions into a pixel's accumulator, the one multiplication
by 1 / n of a resolve and the subtraction above each err by at most eps times a partial sum that mag bounds; N + 2 such
terms, and the bar is twice that.  Measured: the largest |N got - want| / (eps mag) is printed (DESIGN.md par. 4l)."""
import copy
import types

import numpy as np
import pytest

import shutter_ref as S
from helpers import golden_scene, random_rays, rays_to_abi
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import SceneData
from test_gpu_features import placed_scene, placement_transforms

pytestmark = pytest.mark.gpu
DEV, HOST, AUTO = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH, D.TAKE_BUILDER_AUTO
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
DEPTH, SEED = 4, 5
MOVED = dict(lookfrom=(0.9, 0.5, 3.4), lookat=(0.0, -0.1, 0.0), up=(0.05, 1.0, 0.0), vfov=33.0)
DOLLY = dict(lookfrom=(0.25, 0.1, 3.6), lookat=(0.05, 0.0, 0.0), up=(0.0, 1.0, 0.0))
NO_MARK = "no marked frame: take_hip_scene_mark_frame has not been called on this scene"


def camera_of(sd):
    return types.SimpleNamespace(lookfrom=sd.lookfrom, lookat=sd.lookat, up=sd.up, vfov=sd.vfov)


def moved_scene(sd, camera=None, xforms=None):
    """the description of the current frame: `sd` with another camera and other transforms"""
    cur = copy.copy(sd)
    for k, v in (camera or {}).items():
        setattr(cur, k, v)
    if xforms is not None:
        cur.instance_xform = list(xforms)
    return cur


def marked_then_moved(sd, cur, precision, builder=AUTO):
    """a scene created from `sd`, marked, then brought to `cur` through the calls that change a resident scene"""
    sc = capi.Scene(sd, precision=precision, builder=builder)
    sc.mark_frame()
    if cur.instance_xform is not sd.instance_xform:  # (placements that stay are not re-posed either)
        sc.set_instance_transforms(np.stack(cur.instance_xform))
    sc.set_camera(cur.lookfrom, cur.lookat, cur.up, cur.vfov)
    return sc


def fresh_render(sd, precision, spp, builder=DEV, lens=None, **kw):
    sc = capi.Scene(sd, precision=precision, builder=builder)
    try:
        if lens is not None:
            sc.set_lens(*lens)
        return sc.render(spp=spp, max_depth=DEPTH, seed=SEED, **kw)
    finally:
        sc.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def many_placements(n=300):
    """n placements of a two-triangle prototype and nothing else"""
    sd = SceneData(width=32, height=24, lookfrom=(0.0, 0.0, 4.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0,
                   background=(0.3, 0.3, 0.3), spp=1, max_depth=2)
    m = sd.add_material(D.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    quad = sd.add_prototype(np.array([[-0.1, -0.1, 0.0], [0.1, -0.1, 0.0], [0.1, 0.1, 0.0], [-0.1, 0.1, 0.02]]), np.array([[0, 1, 2], [0, 2, 3]]), m)
    for x in many_transforms(n, 3):
        sd.add_instance(quad, x)
    return sd


def many_transforms(n, seed):
    rng = np.random.default_rng(seed)
    lin = rng.uniform(-0.3, 0.3, (n, 3, 3)) + np.eye(3)
    return np.concatenate([lin, rng.uniform(-1.0, 1.0, (n, 3, 1))], axis=2)


# ------------------------------------------------------------------ 1. the pose
def test_the_pose_is_the_restatement_s():
    sd = placed_scene()
    cur = moved_scene(sd, MOVED, placement_transforms(2))
    sc = marked_then_moved(sd, cur, F64)
    try:
        for t in (0.0, 0.3, 1.0):
            got, cam = sc.shutter_pose(t), S.pose_camera(t, camera_of(sd), camera_of(cur))
            assert got["xforms"].shape == (5, 3, 4)
            assert same_bits(got["xforms"], S.pose_xforms(t, placement_transforms(1), placement_transforms(2))), t
            for n in ("lookfrom", "lookat", "up", "vfov"):
                assert same_bits(got[n], cam[n]), (t, n)
        assert same_bits(sc.shutter_pose(0.0)["xforms"], placement_transforms(1)) and same_bits(sc.shutter_pose(1.0)["xforms"], placement_transforms(2))
    finally:
        sc.close()
    sc = capi.Scene(golden_scene("cbox"), precision=F32)
    try:
        sc.mark_frame()
        sc.set_camera(**DOLLY, vfov=sc.sd.vfov)
        got = sc.shutter_pose(0.3)
        assert got["xforms"].shape == (0, 3, 4) and same_bits(got["lookfrom"], S.lerp(0.3, sc.sd.lookfrom, DOLLY["lookfrom"]))
    finally:
        sc.close()


def test_the_pose_of_many_placements_in_every_slice():
    """300 placements: two blocks for one time; with 3 slices 900 lanes — four blocks, the last one partly filled, no
    multiple of the wave.  All three slices at t = 0.3 (open = close) is the scene posed at 0.3, whatever the slice; and
    the first offender among the 900 lanes is named by slice and placement."""
    sd = many_placements()
    a, b = np.stack(sd.instance_xform), many_transforms(300, 4)
    cur = moved_scene(sd, None, b)
    sc = marked_then_moved(sd, cur, F64, DEV)
    try:
        for t in (0.0, 0.3, 1.0):
            assert same_bits(sc.shutter_pose(t)["xforms"], S.pose_xforms(t, a, b)), t
        got = sc.render_shutter(spp=3, max_depth=DEPTH, seed=SEED, open=0.3, close=0.3, slices=3)
        want = fresh_render(S.posed_scene(cur, 0.3, camera_of(sd), a), F64, 3)
        assert np.array_equal(got, want) and not np.array_equal(got, fresh_render(cur, F64, 3))
        # placements 299 and 7 make a half turn: singular at t = 0.5, which is slice 1 of 3 — lanes 307 and 599 of 900
        turned = b.copy()
        for i in (7, 299):
            turned[i, :, :3] = a[i, :, :3] @ np.diag([-1.0, -1.0, 1.0])
        sc.set_instance_transforms(turned)
        before = sc.render(spp=2, max_depth=DEPTH, seed=SEED)
        with pytest.raises(capi.TakeError, match="slice 1: instance 7: singular or non-finite transform") as e:
            sc.render_shutter(spp=3, max_depth=DEPTH, seed=SEED, slices=3)
        assert e.value.code == D.TAKE_E_INVALID
        with pytest.raises(capi.TakeError, match="slice 0: instance 7: singular"):
            sc.shutter_pose(0.5)
        assert np.array_equal(sc.render(spp=2, max_depth=DEPTH, seed=SEED), before)
        sc.render_shutter(spp=3, max_depth=DEPTH, seed=SEED, slices=2)  # t = 0.25, 0.75: no slice at the singular time
        assert np.array_equal(sc.render(spp=2, max_depth=DEPTH, seed=SEED), before)
    finally:
        sc.close()


# ------------------------------------------------------------------ 2. no motion is no change
@pytest.mark.parametrize("levels", ["one-level", "two-level"])
@pytest.mark.parametrize("precision", [F32, F64, MIXED])
def test_no_motion_is_no_change(precision, levels):
    sd = golden_scene("cbox") if levels == "one-level" else placed_scene()
    sc = capi.Scene(sd, precision=precision)
    try:
        want = sc.render(spp=7, max_depth=DEPTH, seed=SEED)
        sc.mark_frame()
        assert np.array_equal(sc.render_shutter(spp=7, max_depth=DEPTH, seed=SEED, slices=3), want)
        assert np.array_equal(sc.render(spp=7, max_depth=DEPTH, seed=SEED), want)
    finally:
        sc.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_placements_that_did_not_move_are_not_reposed(precision):
    """camera blur in a two-level scene: every slice's pose is the current transforms bit for bit, so the host-built top
    level is neither rebuilt nor replaced, and one slice is the host-built scene at the posed camera"""
    sd = placed_scene()
    cur = moved_scene(sd, MOVED)
    sc = marked_then_moved(sd, cur, precision, HOST)
    try:
        stats, built = sc.stats(), sc.build_info()
        got = sc.render_shutter(spp=4, max_depth=DEPTH, seed=SEED, slices=1)
        several = sc.render_shutter(spp=4, max_depth=DEPTH, seed=SEED, slices=4)
        assert sc.stats() == stats and sc.build_info() == built
        after = sc.render(spp=4, max_depth=DEPTH, seed=SEED)
    finally:
        sc.close()
    mid = S.posed_scene(cur, 0.5, camera_of(sd), None)
    assert np.array_equal(got, fresh_render(mid, precision, 4, builder=HOST))
    assert np.array_equal(after, fresh_render(cur, precision, 4, builder=HOST))
    assert not np.array_equal(several, got) and not np.array_equal(several, after)


# ------------------------------------------------------------------ 3. one slice is the posed scene
@pytest.mark.parametrize("precision,builder", [(F32, DEV), (F64, HOST), (MIXED, DEV)])
def test_one_slice_is_the_posed_scene(precision, builder):
    sd = placed_scene()
    cur = moved_scene(sd, MOVED, placement_transforms(2))
    sc = marked_then_moved(sd, cur, precision, builder)
    try:
        first, time = capi.shutter_plan(4, slices=1)
        assert list(first) == [0, 4] and list(time) == [0.5]
        got = sc.render_shutter(spp=4, max_depth=DEPTH, seed=SEED, slices=1)
        after = sc.render(spp=4, max_depth=DEPTH, seed=SEED)
    finally:
        sc.close()
    mid = S.posed_scene(cur, 0.5, camera_of(sd), placement_transforms(1))
    assert np.array_equal(got, fresh_render(mid, precision, 4))
    at_mark, at_now = fresh_render(sd, precision, 4), fresh_render(cur, precision, 4)
    assert not np.array_equal(got, at_mark) and not np.array_equal(got, at_now)
    assert np.array_equal(after, at_now)  # the scene is at its current pose again


# ------------------------------------------------------------------ 4. K slices are the sample-weighted mean
@pytest.mark.parametrize("name", ["placed", "cbox"])
@pytest.mark.parametrize("precision", [F64, F32])
def test_slices_are_the_sample_weighted_mean_of_the_posed_renders(precision, name):
    N, K = 7, 3
    if name == "placed":
        sd, builder = placed_scene(), DEV
        cur = moved_scene(sd, MOVED, placement_transforms(2))
        marked_x = placement_transforms(1)
    else:
        sd, builder = golden_scene("cbox"), AUTO
        cur, marked_x = moved_scene(sd, DOLLY), None
    sc = marked_then_moved(sd, cur, precision, builder)
    try:
        got = sc.render_shutter(spp=N, max_depth=DEPTH, seed=SEED, slices=K).astype(np.float64)
    finally:
        sc.close()
    first, time = S.plan(N, 0.0, 1.0, K)
    assert list(first) == [0, 2, 4, 7]
    want, mag = np.zeros_like(got), np.zeros_like(got)
    for k in range(K):
        posed = S.posed_scene(cur, time[k], camera_of(sd), marked_x)
        psc = capi.Scene(posed, precision=precision, builder=builder)
        try:
            for n, sign in ((int(first[k + 1]), 1.0), (int(first[k]), -1.0)):
                if n == 0:
                    continue
                r = psc.render(spp=n, max_depth=DEPTH, seed=SEED).astype(np.float64)
                want += sign * n * r
                mag += n * np.abs(r)
        finally:
            psc.close()
    eps = 2.0 ** -53 if precision == F64 else 2.0 ** -24
    err = np.abs(N * got - want)
    ratio = float((err[mag > 0] / (eps * mag[mag > 0])).max())
    print(f"{name}, {'f64' if precision == F64 else 'f32'}: max |N got - want| / (eps mag) = {ratio:.3f} (bar {4 * (N + 2)})")
    assert (mag > 0).mean() > 0.9
    assert (err <= 4 * (N + 2) * eps * mag).all(), ratio


# ------------------------------------------------------------------ 5. before = after
@pytest.mark.parametrize("precision,builder", [(F32, HOST), (F64, DEV), (MIXED, HOST)])
def test_the_scene_is_as_before_after_a_render_and_after_a_refusal(precision, builder):
    sd = placed_scene()
    cur = moved_scene(sd, MOVED, placement_transforms(2))
    sc = marked_then_moved(sd, cur, precision, builder)
    rays = rays_to_abi(random_rays(4096, 3), 0 if precision == F32 else 1)
    try:
        def state():
            return sc.trace_closest(rays).tobytes(), sc.trace_any(rays).tobytes(), sc.render(spp=3, max_depth=DEPTH, seed=SEED).tobytes()

        before, motion = state(), sc.render_motion()
        pose = sc.shutter_pose(1.0)
        sc.render_shutter(spp=5, max_depth=DEPTH, seed=SEED, slices=3)
        assert state() == before
        # a progressive sequence ends as a one-shot render ends it: the next accumulate call is fresh, restart or not
        import torch

        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED, restart=True) == 2
        sc.render(spp=1, max_depth=DEPTH, seed=SEED)
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED) == 2
        after_render = buf.cpu().numpy().copy()
        sc.render_shutter(spp=5, max_depth=DEPTH, seed=SEED, slices=3)
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED) == 2
        assert np.array_equal(buf.cpu().numpy(), after_render)
        # a refused call: placement 3 makes a half turn between the mark and now
        turned = placement_transforms(2)
        turned[3, :, :3] = placement_transforms(1)[3, :, :3] @ np.diag([-1.0, -1.0, 1.0])
        sc.set_instance_transforms(turned)
        before = state()
        with pytest.raises(capi.TakeError, match="slice 1: instance 3: singular or non-finite transform"):
            sc.render_shutter(spp=5, max_depth=DEPTH, seed=SEED, slices=3)
        assert state() == before
        # ... and where a one-shot render leaves the accumulate call refused (the scene changed), so does this one
        with pytest.raises(capi.TakeError, match="pass restart = 1"):
            sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED)
        sc.render_shutter(spp=2, max_depth=DEPTH, seed=SEED, slices=1, close=0.2)
        with pytest.raises(capi.TakeError, match="pass restart = 1"):
            sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED)
        sc.set_instance_transforms(placement_transforms(2))
        # the mark, the current transforms and the current camera are untouched
        again = sc.render_motion()
        for n in motion:
            assert np.array_equal(again[n], motion[n]), n
        assert same_bits(sc.shutter_pose(1.0)["xforms"], pose["xforms"]) and same_bits(sc.shutter_pose(1.0)["lookfrom"], pose["lookfrom"])
    finally:
        sc.close()


# ------------------------------------------------------------------ 6. the library against itself
@pytest.mark.parametrize("precision", [F32, MIXED])
def test_batches_and_strips_change_nothing(precision):
    sd = placed_scene()
    cur = moved_scene(sd, MOVED, placement_transforms(2))
    sc = marked_then_moved(sd, cur, precision)
    try:
        kw = dict(spp=7, max_depth=DEPTH, seed=SEED, slices=3)
        whole = sc.render_shutter(**kw)
        for spb in (1, 2, 5):
            assert np.array_equal(sc.render_shutter(samples_per_batch=spb, **kw), whole), spb
        for stride in (2, 3):
            out = np.zeros_like(whole)
            for first in range(stride):
                out[sc.rows(first, stride)] = sc.render_shutter(strip_first=first, strip_stride=stride, **kw)
            assert np.array_equal(out, whole), stride
        import torch

        buf = torch.zeros(whole.shape, dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        sc.render_shutter_device(buf, **kw)
        assert np.array_equal(buf.cpu().numpy(), whole)
    finally:
        sc.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_a_lens_composes(precision):
    sd = placed_scene()
    cur = moved_scene(sd, MOVED, placement_transforms(2))
    sc = marked_then_moved(sd, cur, precision, DEV)
    try:
        sc.set_lens(0.05, 3.5)
        got = sc.render_shutter(spp=4, max_depth=DEPTH, seed=SEED, slices=1)
        sc.set_lens(0.0)
        without = sc.render_shutter(spp=4, max_depth=DEPTH, seed=SEED, slices=1)
    finally:
        sc.close()
    mid = S.posed_scene(cur, 0.5, camera_of(sd), placement_transforms(1))
    assert np.array_equal(got, fresh_render(mid, precision, 4, lens=(0.05, 3.5)))
    assert np.array_equal(without, fresh_render(mid, precision, 4)) and not np.array_equal(got, without)


def test_the_command_line_writes_shutter_exr(tmp_path):
    """-shutter: shutter.exr is render_shutter of the scene file's camera against the marked -from_camera; image.exr is
    the same bytes with or without the flag"""
    from take_amd import exr
    from test_gpu_display import run_cli

    for d in ("without", "with"):
        (tmp_path / d).mkdir()
    run_cli(tmp_path / "without")
    run_cli(tmp_path / "with", "-shutter", "0.25,1", "-slices", "3", "-from_camera", ",".join(repr(float(v)) for v in DOLLY["lookfrom"] + DOLLY["lookat"]))
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == ["image.exr", "shutter.exr"]
    assert (tmp_path / "with" / "image.exr").read_bytes() == (tmp_path / "without" / "image.exr").read_bytes()
    sd = golden_scene("cbox")
    sc = capi.Scene(sd)
    try:
        sc.set_camera(DOLLY["lookfrom"], DOLLY["lookat"], sd.up, sd.vfov)
        sc.mark_frame()
        sc.set_camera(sd.lookfrom, sd.lookat, sd.up, sd.vfov)
        want = sc.render_shutter(spp=sd.spp, max_depth=5, seed=0, open=0.25, close=1.0, slices=3)
        still = sc.render(spp=sd.spp, max_depth=5, seed=0)
    finally:
        sc.close()
    exr.write_exr(str(tmp_path / "want.exr"), want)
    exr.write_exr(str(tmp_path / "still.exr"), still)
    assert (tmp_path / "with" / "shutter.exr").read_bytes() == (tmp_path / "want.exr").read_bytes()
    assert (tmp_path / "with" / "shutter.exr").read_bytes() != (tmp_path / "still.exr").read_bytes()


# ------------------------------------------------------------------ 7. no mark, and the other refusals that need a scene
def test_refusals():
    sc = capi.Scene(placed_scene(), precision=F32)
    try:
        for call in (lambda: sc.render_shutter(spp=2, max_depth=DEPTH), lambda: sc.shutter_pose(0.5)):
            with pytest.raises(capi.TakeError) as e:
                call()
            assert e.value.code == D.TAKE_E_INVALID and NO_MARK in str(e.value)
        with pytest.raises(capi.TakeError, match="no marked frame"):
            sc.render_motion()  # the motion pass's message
        sc.mark_frame()
        # the camera turns round its lookfrom's mirror image: at t = 0.5 lookat and lookfrom coincide
        sc.set_camera((0.0, 0.0, -3.9), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), sc.sd.vfov)
        before = sc.render(spp=2, max_depth=DEPTH, seed=SEED)
        with pytest.raises(capi.TakeError, match="slice 1: the interpolated camera") as e:
            sc.render_shutter(spp=3, max_depth=DEPTH, slices=3)
        assert e.value.code == D.TAKE_E_INVALID
        assert np.array_equal(sc.render(spp=2, max_depth=DEPTH, seed=SEED), before)
        sc.render_shutter(spp=2, max_depth=DEPTH, slices=2)
    finally:
        sc.close()

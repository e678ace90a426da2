"""Motion vectors that follow deforming meshes (take_hip_scene_track_vertices, take_hip_scene_tracking_info:
include/take_hip.h; kernels: take_amd/csrc/tk_motion.h k_motion<R, true>, tk_motion_pixel.h, tk_build_gpu.h
k_copy_marked) against the float64 restatement of the specification (tests/motion_ref.py; DESIGN.md par. 4i) applied to
take_hip_trace_closest's own (id, t, u, v) of centre rays made in numpy, with the vertex arrays the test supplied.

Scenes, 48 x 32.  Flat: two meshes of 8 x 8 quads (128 triangles each: the rebuild really reorders the records), a third
mesh that is never updated, one sphere.  Two-level: two prototypes of that size with two placements each, only one of
them updated, its faces also among the head shapes.

Bars.  F64 (and MIXED, whose motion pass runs on the f64 side): 1e-9 pixel, 1e-9 relative on prev_depth.  F32:
F32_XY_BAR pixel and F32_REL_BAR relative, the next power of ten above 8 x the largest difference measured on these
scenes on an MI355X (prev_xy 7.63e-6 pixel: 8 x = 6.1e-5; prev_depth 1.90e-6 relative: 8 x = 1.5e-5; DESIGN.md par. 4i);
the pixel bar has to stay at or below 0.01 pixel, where a bilinear weight visibly changes.  Ids equal to the trace
hook's on >= 99.5 % of the pixels (last-bit differences of the ray direction move a ray across an edge).

Everything the library is compared with itself on is np.array_equal."""

import numpy as np
import pytest
import torch  # (before the library is loaded: the two share one HIP runtime only in this order)

import motion_ref as M
import temporal_ref as T
from helpers import rays_to_abi, rmse
from take_amd import capi
from take_amd import cdefs as D
from take_amd.scene import Light, SceneData

pytestmark = pytest.mark.gpu
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
DEPTH = 6
F32_XY_BAR, F32_REL_BAR = 1e-4, 1e-4
assert F32_XY_BAR <= 0.01
LEFT, RIGHT, BACK = 0, 1, 2  # the meshes of flat_scene
OFFSET = np.array([0.15, 0.1, 0.05])  # the translation of LEFT: about 1.7 x 1.1 pixels


# ------------------------------------------------------------------ scenes
def grid_mesh(n, x0, x1, y0, y1, z=0.0, bend=0.05):
    """n x n quads over [x0, x1] x [y0, y1], gently bent out of the plane z -> positions ((n + 1)^2, 3), indices (2 n^2, 3)"""
    x, y = np.meshgrid(np.linspace(x0, x1, n + 1), np.linspace(y0, y1, n + 1))
    pos = np.stack([x, y, z + bend * np.sin(3.0 * x) * np.cos(2.0 * y)], -1).reshape(-1, 3)
    j, i = np.mgrid[0:n, 0:n]
    a = (j * (n + 1) + i).reshape(-1)
    idx = np.stack([np.stack([a, a + 1, a + n + 2], -1), np.stack([a, a + n + 2, a + n + 1], -1)], 1).reshape(-1, 3)
    return pos, idx.astype(np.int32)


def empty_scene(width=48, height=32):
    sd = SceneData(width=width, height=height, lookfrom=(0.0, 0.0, 4.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0, background=(0.2, 0.3, 0.4),
                   spp=4, max_depth=DEPTH)
    mats = [sd.add_material(D.MAT_DIFFUSE, c) for c in ((0.73, 0.73, 0.73), (0.65, 0.05, 0.05), (0.12, 0.45, 0.15))]
    sd.lights.append(Light(0, -1, (12.0, 12.0, 12.0), (0.3, 2.0, 3.0)))
    return sd, mats


def flat_scene():
    sd, (white, red, green) = empty_scene()
    assert sd.add_mesh(*grid_mesh(8, -1.6, -0.15, -1.0, 1.0), red) == LEFT
    assert sd.add_mesh(*grid_mesh(8, 0.15, 1.6, -1.0, 1.0), green) == RIGHT
    assert sd.add_mesh(*grid_mesh(2, -3.0, 3.0, -2.0, 2.0, z=-0.8, bend=0.0), white) == BACK
    sd.add_sphere((0.0, 0.1, 0.4), 0.3, white)
    assert sd.n_shapes == 128 + 128 + 8 + 1
    return sd


def placement(angle, scale, t):
    c, s = np.cos(angle), np.sin(angle)
    return np.concatenate([scale * np.array([[c, -s, 0.0], [s, c, 0.1], [0.0, 0.05, 1.0]]), np.asarray(t, np.float64)[:, None]], axis=1)


def two_level_scene():
    """mesh 0: faces among the head shapes AND the prototype of placements 0 and 1 (the one that is updated); mesh 1:
    the prototype of placements 2 and 3; mesh 2: a backdrop among the head shapes; a sphere"""
    sd, (white, red, green) = empty_scene()
    assert sd.add_mesh(*grid_mesh(8, -0.45, 0.45, -0.45, 0.45), red) == 0
    assert sd.add_prototype(*grid_mesh(8, -0.5, 0.5, -0.4, 0.4, bend=0.08), green) == 1
    assert sd.add_mesh(*grid_mesh(2, -3.0, 3.0, -2.0, 2.0, z=-0.8, bend=0.0), white) == 2
    sd.add_sphere((0.0, 0.9, 0.3), 0.25, white)
    sd.add_instance(0, placement(0.3, 0.9, (-1.3, 0.55, 0.1)))
    sd.add_instance(0, placement(-0.5, 1.1, (1.3, 0.5, -0.1)), material_id=white)
    sd.add_instance(1, placement(0.8, 1.0, (-1.2, -0.7, 0.2)))
    sd.add_instance(1, placement(-0.2, 0.8, (1.2, -0.75, 0.0)))
    assert sd.n_shapes == 128 + 8 + 1
    return sd


def smooth(pos, k=1.0):
    """a smooth displacement that is no rigid motion, about a pixel at k = 1"""
    return pos + k * 0.1 * np.sin(3.0 * pos[:, [1, 2, 0]] + 0.5)


def shape_base(sd):
    faces = [sd.meshes[m].indices.shape[0] for m in sd.instance_mesh]
    return sd.n_shapes + np.concatenate([[0], np.cumsum(faces)]).astype(np.int64)


def camera_of(sd):
    return T.camera(sd.lookfrom, sd.lookat, sd.up, sd.vfov, sd.width, sd.height)


def centres(sd):
    return T.motion("identity", sd.width, sd.height)


def traced(sc, sd, precision):
    """take_hip_trace_closest of the centre rays of the scene's camera, made in numpy -> (cam, directions (n, 3), hits)"""
    cam = camera_of(sd)
    d = T.centre_rays(cam).reshape(-1, 3)
    n = d.shape[0]
    eps = 1e-4 if precision == F32 else 1e-7
    rays = np.concatenate([np.broadcast_to(cam["from"], (n, 3)), d, np.full((n, 1), eps), np.full((n, 1), np.inf)], axis=1)
    return cam, d, sc.trace_closest(rays_to_abi(rays, 0 if precision == F32 else 1))


def restated(sd, sc, precision, marked_positions, xf_mark=None):
    """the float64 restatement on the trace hook's (id, t, u, v): the geometry of the marked frame is `marked_positions`
    ({mesh: positions}; every other mesh: the description's), the marked camera the scene's, the marked transforms xf_mark
    -> ids (H, W), prev_xy (H, W, 2), prev_depth (H, W)"""
    cam, d, hits = traced(sc, sd, precision)
    ids = hits["shape_id"].astype(np.int64)
    n = ids.shape[0]
    words_of = [M.triangle_words(marked_positions.get(m, mesh.positions), mesh.indices) for m, mesh in enumerate(sd.meshes)]
    kind, placed = np.full(n, M.MISS, np.int32), np.zeros(n, bool)
    words, fwd = np.zeros((n, 9)), np.zeros((n, 12))
    head = (ids >= 0) & (ids < sd.n_shapes)
    tri = head & (sd.shape_kind[np.clip(ids, 0, sd.n_shapes - 1)] == 1)
    kind[head] = M.POINT
    kind[tri] = M.TRIANGLE
    for i in np.flatnonzero(tri):
        words[i] = words_of[sd.shape_ref[ids[i]]][sd.shape_face[ids[i]]]
    if sd.instance_mesh:
        base = shape_base(sd)
        inst = np.searchsorted(base, ids, side="right") - 1
        for i in np.flatnonzero(ids >= sd.n_shapes):
            kind[i], placed[i] = M.TRIANGLE, True
            words[i] = words_of[sd.instance_mesh[inst[i]]][ids[i] - base[inst[i]]]
            fwd[i] = M.affine12(xf_mark[inst[i]])
    ro = np.broadcast_to(cam["from"], (n, 3))
    xy, pd = M.tracked_pixels(cam, kind, ro, d, hits["t"], hits["u"], hits["v"], words, np.zeros((n, 12)), fwd, placed, dtype=np.float64)
    H, W = sd.height, sd.width
    return ids.reshape(H, W), xy.reshape(H, W, 2), pd.reshape(H, W)


def bars(precision):
    return (F32_XY_BAR, F32_REL_BAR) if precision == F32 else (1e-9, 1e-9)


def held_to(got, want, precision, label, min_hit=0.3):
    """motion planes against restated(): ids on >= 99.5 % of the pixels, prev_xy and prev_depth within the bars where the
    ids agree -> the mask of agreeing pixels"""
    ids, want_xy, want_pd = want
    xy_bar, rel_bar = bars(precision)
    agree = got["shape_id"] == ids
    hit = agree & (ids >= 0)
    d_xy = float(np.abs(got["prev_xy"].astype(np.float64) - want_xy)[agree].max())
    d_pd = float(np.abs(got["prev_depth"][hit].astype(np.float64) / want_pd[hit] - 1).max())
    print(f"{label}: ids equal on {100 * agree.mean():.3f} % of the pixels; prev_xy off the restatement by {d_xy:.3e} pixel (bar {xy_bar:.0e}), "
          f"prev_depth by {d_pd:.3e} relative (bar {rel_bar:.0e})")
    assert agree.mean() >= 0.995 and hit.mean() > min_hit, label
    assert d_xy <= xy_bar and d_pd <= rel_bar and (got["prev_depth"][got["shape_id"] < 0] == 0).all(), label
    return agree


def same_planes(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ 1. the test that fails without the feature
@pytest.mark.parametrize("precision", [F32, F64, MIXED])
def test_flat_scene_a_translation_and_a_deformation_are_followed(precision):
    sd = flat_scene()
    moved = {LEFT: sd.meshes[LEFT].positions + OFFSET, RIGHT: smooth(sd.meshes[RIGHT].positions)}
    sc = capi.Scene(sd, precision=precision)
    try:
        sc.track_vertices()
        assert sc.tracking_info() == {"flags": D.TAKE_TRACK_VERTICES, "marked_bytes": 0}
        sc.mark_frame()
        sc.set_mesh_vertices(moved)
        real = 4 if precision == F32 else 8
        assert sc.tracking_info()["marked_bytes"] == sd.n_shapes * 12 * real, "one entry of 12 Real per record, of the primary side only"
        got = sc.render_motion()
        want = restated(sd, sc, precision, {})
        agree = held_to(got, want, precision, f"flat-{precision}")
        ids = want[0]
        # the translated mesh: the marked point is the hit point less the offset — without tracking it is the pixel's centre
        cam, d, hits = traced(sc, sd, precision)
        on_left = (agree & (ids >= 0) & (ids < 128)).reshape(-1)
        assert on_left.mean() > 0.1
        P = cam["from"] + d * hits["t"].astype(np.float64)[:, None] - OFFSET
        n = P.shape[0]
        xy, _ = M.tracked_pixels(cam, np.full(n, M.POINT, np.int32), P, np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, 9)), np.zeros((n, 12)),
                                 np.zeros((n, 12)), np.zeros(n, bool))
        off = got["prev_xy"].astype(np.float64).reshape(-1, 2) - centres(sd).reshape(-1, 2)
        d_off = float(np.abs(got["prev_xy"].astype(np.float64).reshape(-1, 2) - xy)[on_left].max())
        xy_bar = bars(precision)[0] if precision == F32 else 1e-9 * sd.width  # (o + d * t is off the surface by a rounding of t)
        print(f"flat-{precision} translated mesh: prev_xy - centre = {off[on_left].mean(0)} pixel on average, off the projected offset by {d_off:.3e} pixel (bar {xy_bar:.0e})")
        assert d_off <= xy_bar and (np.abs(off[on_left]).max(-1) > 0.5).all(), "the pixel's own centre is what an untracked pass gives"
        on_right = agree & (ids >= 128) & (ids < 256)
        assert (np.abs(got["prev_xy"].astype(np.float64) - centres(sd))[on_right].max(-1) > 0.05).mean() > 0.9, "the deformation is seen"
        still = (ids >= 256) & agree  # the third mesh and the sphere did not move
        assert float(np.abs(got["prev_xy"].astype(np.float64) - centres(sd))[still].max()) <= (F32_XY_BAR if precision == F32 else 1e-9 * sd.width)
        # the device twin, and a subset of the planes
        tdtype = torch.float32 if precision == F32 else torch.float64
        dev = {"prev_xy": torch.zeros((sd.height, sd.width, 2), dtype=tdtype, device="cuda"), "shape_id": torch.zeros((sd.height, sd.width), dtype=torch.int32, device="cuda")}
        sc.render_motion_device(dev)
        torch.cuda.synchronize()
        assert all(np.array_equal(dev[k].cpu().numpy(), got[k]) for k in dev), "device twin"
        assert same_planes(sc.render_motion(want=("prev_depth",)), {"prev_depth": got["prev_depth"]})
    finally:
        sc.close()


def two_level_moved(sd):
    return {0: smooth(sd.meshes[0].positions, 0.6)}


@pytest.mark.parametrize("precision", [F32, F64])
def test_two_level_scene_a_deformed_prototype_is_followed_in_every_role(precision):
    sd = two_level_scene()
    xf = np.stack(sd.instance_xform)
    sc = capi.Scene(sd, precision=precision)
    try:
        sc.track_vertices()
        sc.mark_frame()
        sc.update_meshes(two_level_moved(sd))
        n_records = sd.n_shapes + sum(sd.meshes[m].indices.shape[0] for m in (0, 1))  # the shapes' and one set per prototype
        assert sc.tracking_info()["marked_bytes"] == n_records * 12 * (4 if precision == F32 else 8) + 4 * len(sd.instance_mesh)
        got = sc.render_motion()
        want = restated(sd, sc, precision, {}, xf)
        agree = held_to(got, want, precision, f"two-level-{precision}")
        ids, base = want[0], shape_base(sd)
        shift = np.abs(got["prev_xy"].astype(np.float64) - centres(sd)).max(-1)
        for label, where, moves in (("head faces of the updated mesh", (ids >= 0) & (ids < 128), True), ("placements of the updated prototype", (ids >= base[0]) & (ids < base[2]), True),
                                    ("placements of the other prototype", ids >= base[2], False), ("backdrop and sphere", (ids >= 128) & (ids < sd.n_shapes), False)):
            where = where & agree
            assert where.mean() > 0.02, label
            print(f"two-level-{precision} {label}: {100 * where.mean():.1f} % of the pixels, |prev_xy - centre| median {np.median(shift[where]):.3e} max {shift[where].max():.3e}")
            if moves:
                assert np.median(shift[where]) > 0.05, label
            else:
                assert shift[where].max() <= (F32_XY_BAR if precision == F32 else 1e-9 * sd.width), label
    finally:
        sc.close()


# ------------------------------------------------------------------ 2. off is what it was
def sequence(sc, sd, moved, update):
    """mark, move, motion"""
    sc.mark_frame()
    getattr(sc, update)(moved)
    return sc.render_motion()


@pytest.mark.parametrize("name,precision", [("flat", F32), ("flat", MIXED), ("two-level", F32)])
def test_tracking_off_and_tracking_without_an_update_are_the_untracked_bits(name, precision):
    sd = flat_scene() if name == "flat" else two_level_scene()
    update = "set_mesh_vertices" if name == "flat" else "update_meshes"
    moved = {LEFT: sd.meshes[LEFT].positions + OFFSET, RIGHT: smooth(sd.meshes[RIGHT].positions)} if name == "flat" else two_level_moved(sd)
    plain, off, on = (capi.Scene(sd, precision=precision) for _ in range(3))
    try:
        off.track_vertices(True)
        off.track_vertices(False)
        on.track_vertices()
        assert plain.tracking_info() == off.tracking_info() == {"flags": 0, "marked_bytes": 0}
        for sc in (plain, off, on):
            sc.mark_frame()
        still = plain.render_motion()
        assert same_planes(on.render_motion(), still) and on.tracking_info()["marked_bytes"] == 0, "tracking on, no update since the mark"
        want = sequence(plain, sd, moved, update)
        assert same_planes(sequence(off, sd, moved, update), want) and off.tracking_info() == {"flags": 0, "marked_bytes": 0}, "tracking off"
        hit = want["shape_id"] >= 0
        assert float(np.abs(want["prev_xy"].astype(np.float64) - centres(sd))[hit].max()) <= 1e-4, "an untracked pass: the pixel centres"
        tracked = sequence(on, sd, moved, update)
        assert on.tracking_info()["marked_bytes"] > 0 and not np.array_equal(tracked["prev_xy"], want["prev_xy"])
        assert np.array_equal(tracked["shape_id"], want["shape_id"]) and np.array_equal(tracked["depth"], want["depth"]), "depth and shape_id are as without tracking"
    finally:
        for sc in (plain, off, on):
            sc.close()


# ------------------------------------------------------------------ 3. the lifetime of the copy
@pytest.mark.parametrize("precision", [F32, F64])
def test_the_copy_is_of_the_frame_at_the_mark_and_lives_until_the_next_mark(precision):
    sd = flat_scene()
    p0 = {m: sd.meshes[m].positions for m in (LEFT, RIGHT)}
    p1 = {LEFT: p0[LEFT] + OFFSET, RIGHT: smooth(p0[RIGHT], 0.5)}
    p2 = {LEFT: p0[LEFT] + 2 * OFFSET, RIGHT: smooth(p0[RIGHT])}
    sc, plain = capi.Scene(sd, precision=precision), capi.Scene(sd, precision=precision)
    try:
        sc.track_vertices()
        sc.mark_frame()
        sc.set_mesh_vertices(p1)
        held = sc.tracking_info()["marked_bytes"]
        first = sc.render_motion()
        # a failing update leaves the planes and the copy as they were
        bad = p2[RIGHT].copy()
        bad[17, 1] = np.nan
        with pytest.raises(capi.TakeError) as e:
            sc.set_mesh_vertices({LEFT: p2[LEFT], RIGHT: bad})
        assert e.value.code == D.TAKE_E_INVALID and "vertex 17" in str(e.value)
        assert sc.tracking_info()["marked_bytes"] == held and same_planes(sc.render_motion(), first), "after a failed update"
        # update, update, motion: against the geometry at the mark, not the intermediate one
        sc.set_mesh_vertices(p2)
        assert sc.tracking_info()["marked_bytes"] == held
        got = sc.render_motion()
        agree = held_to(got, restated(sd, sc, precision, p0), precision, f"update-update-{precision}")
        ids, wrong_xy, _ = restated(sd, sc, precision, p1)
        on_left = agree & (ids >= 0) & (ids < 128)
        assert (np.abs(got["prev_xy"].astype(np.float64) - wrong_xy)[on_left].max(-1) > 0.5).all(), "the intermediate geometry is a pixel away"
        # update, mark, motion: the pixel centres, nothing held
        sc.mark_frame()
        assert sc.tracking_info() == {"flags": 1, "marked_bytes": 0}
        after = sc.render_motion()
        hit = after["shape_id"] >= 0
        assert float(np.abs(after["prev_xy"].astype(np.float64) - centres(sd))[hit].max()) <= (F32_XY_BAR if precision == F32 else 1e-9 * sd.width)
        # off and on again drops the copy: the pass is the untracked one until the next mark
        for s in (sc, plain):
            s.set_mesh_vertices(p2)
            s.mark_frame()
            s.set_mesh_vertices(p1)
        assert sc.tracking_info()["marked_bytes"] == held
        sc.track_vertices(False)
        assert sc.tracking_info() == {"flags": 0, "marked_bytes": 0}
        sc.track_vertices(True)
        sc.set_mesh_vertices(p0)
        plain.set_mesh_vertices(p0)
        assert sc.tracking_info() == {"flags": 1, "marked_bytes": 0}, "tracking turned on after an update holds nothing until the next mark"
        assert same_planes(sc.render_motion(), plain.render_motion())
    finally:
        sc.close()
        plain.close()


@pytest.mark.parametrize("name", ["flat", "two-level"])
def test_an_update_that_cannot_allocate_the_copy_fails_as_a_whole(name, monkeypatch):
    """fault injection (TAKE_HIP_FAIL_ALLOC: the n-th device allocation after it is set fails; a real out-of-memory cannot
    be provoked reliably): whichever allocation of the update call fails, the call fails, holds nothing and leaves the
    planes as they were; the table's allocations — one, and the placements' array in a two-level scene — fail with
    TAKE_E_NOMEM and their own message; the same call without the injection then succeeds as if nothing had happened"""
    sd = flat_scene() if name == "flat" else two_level_scene()
    update = "set_mesh_vertices" if name == "flat" else "update_meshes"
    moved = {LEFT: sd.meshes[LEFT].positions + OFFSET} if name == "flat" else two_level_moved(sd)
    sc, ref = capi.Scene(sd, precision=F32), capi.Scene(sd, precision=F32)
    try:
        for s in (sc, ref):
            s.track_vertices()
            s.mark_frame()
        before = sc.render_motion()
        own = []
        for nth in range(1, 9):
            monkeypatch.setenv("TAKE_HIP_FAIL_ALLOC", str(nth))
            with pytest.raises(capi.TakeError) as e:
                getattr(sc, update)(moved)
            monkeypatch.delenv("TAKE_HIP_FAIL_ALLOC")
            if "out of device memory for the marked frame's geometry" in str(e.value):
                assert e.value.code == D.TAKE_E_NOMEM
                own.append(nth)
            assert sc.tracking_info() == {"flags": 1, "marked_bytes": 0}, nth
            assert same_planes(sc.render_motion(), before), nth
        assert len(own) == (1 if name == "flat" else 2) and own == list(range(own[0], own[0] + len(own))), own
        for s in (sc, ref):
            getattr(s, update)(moved)
        assert sc.tracking_info() == ref.tracking_info() and sc.tracking_info()["marked_bytes"] > 0
        assert same_planes(sc.render_motion(), ref.render_motion())
    finally:
        sc.close()
        ref.close()


# ------------------------------------------------------------------ 4. a rigid motion of the vertices is a motion of the placements
@pytest.mark.parametrize("precision", [F32, F64])
def test_rigid_vertices_against_rigid_placements(precision):
    """case A multiplies prototype 0's vertices by a rigid T; case B gives its placements M * T.  The same surface, the
    same marked frame: the same prev_xy, A through the marked words, B through the placements' inverses"""
    sd = two_level_scene()
    a, t = 0.1, np.array([0.05, -0.03, 0.02])
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    xf = np.stack(sd.instance_xform)
    xf_b = xf.copy()
    for i in (0, 1):
        xf_b[i, :, :3], xf_b[i, :, 3] = xf[i, :, :3] @ rot, xf[i, :, :3] @ t + xf[i, :, 3]
    A, B = capi.Scene(sd, precision=precision), capi.Scene(sd, precision=precision)
    try:
        for sc in (A, B):
            sc.track_vertices()
            sc.mark_frame()
        A.update_meshes({0: sd.meshes[0].positions @ rot.T + t})
        B.set_instance_transforms(xf_b)
        assert A.tracking_info()["marked_bytes"] > 0 and B.tracking_info()["marked_bytes"] == 0
        pa, pb = A.render_motion(), B.render_motion()
        base = shape_base(sd)
        placed = (pa["shape_id"] >= base[0]) & (pa["shape_id"] < base[2])
        where = placed & (pa["shape_id"] == pb["shape_id"])
        assert where.mean() > 0.05 and where.sum() >= 0.98 * placed.sum()
        # B's transforms are M * T rounded to double and inverted by the library: in f64 the bar is that of the untracked pass
        xy_bar, rel_bar = (F32_XY_BAR, F32_REL_BAR) if precision == F32 else (1e-9 * sd.width, 1e-9)
        d_xy = float(np.abs(pa["prev_xy"].astype(np.float64) - pb["prev_xy"])[where].max())
        d_pd = float(np.abs(pa["prev_depth"][where].astype(np.float64) / pb["prev_depth"][where] - 1).max())
        moved = float(np.median(np.abs(pa["prev_xy"].astype(np.float64) - centres(sd))[where].max(-1)))
        print(f"rigid-{precision}: {100 * where.mean():.1f} % of the pixels, median motion {moved:.2f} pixel; A against B: prev_xy {d_xy:.3e} pixel (bar {xy_bar:.0e}), "
              f"prev_depth {d_pd:.3e} relative (bar {rel_bar:.0e})")
        assert moved > 0.2 and d_xy <= xy_bar and d_pd <= rel_bar
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------ 5. node formats
def tracked_motion(sd, monkeypatch, fmt, update, moved):
    if fmt is None:
        monkeypatch.delenv("TAKE_HIP_NODES", raising=False)
    else:
        monkeypatch.setenv("TAKE_HIP_NODES", fmt)
    sc = capi.Scene(sd, precision=F32)
    try:
        sc.track_vertices()
        sc.mark_frame()
        getattr(sc, update)(moved)
        assert sc.tracking_info()["marked_bytes"] > 0
        return sc.render_motion(), sc.debug_tree()["node_format"]
    finally:
        sc.close()


@pytest.mark.parametrize("name", ["flat", "two-level"])
def test_full_width_and_compressed_nodes_give_the_same_planes(name, monkeypatch):
    sd = flat_scene() if name == "flat" else two_level_scene()
    update = "set_mesh_vertices" if name == "flat" else "update_meshes"
    moved = {LEFT: sd.meshes[LEFT].positions + OFFSET, RIGHT: smooth(sd.meshes[RIGHT].positions)} if name == "flat" else two_level_moved(sd)
    want, default_format = tracked_motion(sd, monkeypatch, None, update, moved)
    got, node_format = tracked_motion(sd, monkeypatch, "wide", update, moved)
    assert (default_format, node_format) == (D.NODE_FORMAT_Q4, D.NODE_FORMAT_WIDE)
    # the same records hit by the same rays: the trees differ, the hits do not (conservative box tests)
    assert same_planes(got, want)


# ------------------------------------------------------------------ 6. a render and a progressive sequence across the pass
@pytest.mark.parametrize("name,precision", [("flat", F32), ("flat", MIXED), ("two-level", F64)])
def test_a_render_and_a_progressive_sequence_keep_their_bits(name, precision):
    sd = flat_scene() if name == "flat" else two_level_scene()
    update = "set_mesh_vertices" if name == "flat" else "update_meshes"
    moved = {LEFT: sd.meshes[LEFT].positions + OFFSET, RIGHT: smooth(sd.meshes[RIGHT].positions)} if name == "flat" else two_level_moved(sd)
    sc = capi.Scene(sd, precision=precision)
    try:
        sc.track_vertices()
        sc.mark_frame()
        getattr(sc, update)(moved)
        plain = sc.render(spp=3, max_depth=DEPTH, seed=5)
        feats = sc.render_features(2, seed=5)
        first = sc.render_motion()
        buf = torch.zeros(plain.shape, dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=5, restart=True) == 2
        assert same_planes(sc.render_motion(), first), "a repeated call"
        assert sc.render_accumulate(buf.data_ptr(), 1, DEPTH, seed=5) == 3
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), plain), "a progressive sequence across the tracked motion pass"
        assert np.array_equal(sc.render(spp=3, max_depth=DEPTH, seed=5), plain), "a render afterwards"
        assert same_planes(sc.render_features(2, seed=5), feats), "the feature planes afterwards"
    finally:
        sc.close()


# ------------------------------------------------------------------ 7. the sequence
N_STRIPES, STRIPE, SLIDE = 56, 0.15, 0.06  # a stripe is about 5 pixels wide at 128 x 96; the surface slides about two pixels per frame
RULE = dict(spp=4, min_spp=4, max_depth=DEPTH)
FILTER = dict(iterations=4, sigma_color=3.0)
GUIDES = ("albedo", "normal", "depth")


def striped_scene():
    """a surface of 56 stripes in the plane z = 0, far wider than the view: the even ones are mesh 0, the odd ones mesh 1,
    of different albedo; a quad light above it and out of the camera's sight, which does not move (a visible one
    would leave its own edge pixels, of mixed content, in the history that the sliding surface then fetches)"""
    sd, (white, red, green) = empty_scene(128, 96)
    sd.lights.clear()
    for parity, mat in ((0, red), (1, green)):
        pos, idx = [], []
        for k in range(parity, N_STRIPES, 2):
            x0 = -4.2 + STRIPE * k
            idx += [[len(pos), len(pos) + 1, len(pos) + 2], [len(pos), len(pos) + 2, len(pos) + 3]]
            pos += [(x0, -2.0, 0.0), (x0 + STRIPE, -2.0, 0.0), (x0 + STRIPE, 2.0, 0.0), (x0, 2.0, 0.0)]
        sd.add_mesh(np.array(pos), np.array(idx, np.int32), mat)
    # the light: above the surface and beside the view (at its height the view is 1.17 wide to either side), facing down
    h, cx = 0.35, 1.9
    sd.add_mesh(np.array([(cx - h, 0.5 + h, 1.6), (cx + h, 0.5 + h, 1.6), (cx + h, 0.5 - h, 1.6), (cx - h, 0.5 - h, 1.6)]), np.array([[0, 1, 2], [0, 2, 3]], np.int32), white,
                normals=np.tile([0.0, 0.0, -1.0], (4, 1)), emission=(17.0, 12.0, 4.0))
    return sd


def slid(sd, k):
    return {m: sd.meshes[m].positions + k * np.array([SLIDE, 0.0, 0.0]) for m in (0, 1)}


def frame_by_hand(sc, history, seed):
    """one frame of take_hip_render_temporal through the public calls -> (the filtered image, the accumulated frame)"""
    img, st = sc.render_adaptive(seed=seed, stats=True, **RULE)
    if history is None:
        sc.mark_frame()
        acc = dict(rgb=img, **st, **sc.render_motion(want=("depth", "shape_id")))
    else:
        m = sc.render_motion()
        acc = capi.temporal_accumulate(dict(rgb=img, **st, depth=m["depth"], shape_id=m["shape_id"]), history, m["prev_xy"], m["prev_depth"])
    planes = sc.render_features(RULE["min_spp"], seed=seed, want=GUIDES)
    out = capi.denoise_variance(acc["rgb"], acc["count"], acc["m1"], acc["m2"], **planes, **FILTER)
    sc.mark_frame()
    return out, acc


def test_four_frames_of_a_sliding_surface_are_closer_with_tracking():
    """a condition, not a measurement (the RMSEs are in DESIGN.md par. 4i): with tracking every pixel of the surface finds
    its history where the surface was; without, a pixel finds it only where the same triangle still covers it, and
    what it finds there belongs to a point two pixels away"""
    sd = striped_scene()
    tracked, untracked, hand = (capi.Scene(sd, precision=F32) for _ in range(3))
    try:
        tracked.track_vertices()
        hand.track_vertices()
        history = None
        for k, seed in enumerate((1, 2, 3, 4)):
            if k:
                for sc in (tracked, untracked, hand):
                    sc.set_mesh_vertices(slid(sd, k))
            with_t = tracked.render_temporal(seed=seed, **RULE, **FILTER)
            without = untracked.render_temporal(seed=seed, **RULE, **FILTER)
            want, history = frame_by_hand(hand, history, seed)
            assert np.array_equal(with_t, want), f"frame {k + 1}: render_temporal with tracking is the calls made by hand"
            if k:
                assert tracked.tracking_info()["marked_bytes"] == 0, "the frame's own mark dropped the copy"
                assert not np.array_equal(with_t, without)
        alone = untracked.render_temporal(seed=4, restart=True, **RULE, **FILTER)
        truth = untracked.render(spp=1024, max_depth=DEPTH, seed=11)
    finally:
        for sc in (tracked, untracked, hand):
            sc.close()
    found = (history["count"] > 4).mean()
    e_alone, e_without, e_with = rmse(alone, truth), rmse(without, truth), rmse(with_t, truth)
    print(f"striped surface 128x96, {SLIDE * 96 / (2 * np.tan(np.radians(20.0)) * 4.0):.1f} pixels per frame: RMSE of frame 4 to 1024 spp: alone {e_alone:.4f}, four frames without tracking {e_without:.4f}, "
          f"with tracking {e_with:.4f}; {100 * found:.1f} % of the pixels found a history with tracking")
    assert np.isfinite(with_t).all() and e_with < e_alone and e_with < e_without

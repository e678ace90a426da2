"""Motion blur for deforming meshes on the device (take_hip_shutter_vertices*, take_hip_render_shutter_meshes*:
include/take_hip.h; the kernel: k_shutter_vertices in take_amd/csrc/tk_shutter.h; DESIGN.md par. 4r) against the numpy
restatement (tests/shutter_deform_ref.py, tests/shutter_ref.py) and against renders of scenes NEWLY CREATED by the device
LBVH builder from the restatement's arrays at the restatement's poses.

Bars.  The kernel: bit for bit.  No motion, one slice, before/after, inputs, batches, strips, the lens: np.array_equal.
K slices: the bar of tests/test_gpu_shutter.py, its formula and its reasoning unchanged — with N = spp, slice k = samples
[a_k, b_k) and R_k(n) = render(spp = n) of a fresh scene at the vertices and the pose of t_k,
    want = sum_k (b_k R_k(b_k) - a_k R_k(a_k)),   mag = sum_k (b_k |R_k(b_k)| + a_k |R_k(a_k)|)    (float64)
    |N got - want| <= 4 (N + 2) eps mag    per component, eps = 2^-53 (f64) or 2^-24 (f32).
Measured: the largest |N got - want| / (eps mag) is printed (DESIGN.md par. 4r)."""
import numpy as np
import pytest

import shutter_deform_ref as V
import shutter_ref as S
from take_amd import capi
from take_amd import cdefs as D
from test_gpu_device_build_instanced import abi, same_hits, scene_rays
from test_gpu_mesh_update import base_scene, emissive_scene, smooth, with_arrays
from test_gpu_proto_update import BOTH, GRID as PROTO_GRID, half_shrunk, original, proto_meshes, scene
from test_gpu_repose import tmin_of
from test_gpu_shutter import camera_of, fresh_render, moved_scene

pytestmark = pytest.mark.gpu
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]
DEPTH, SEED = 4, 5
GRID = 0  # the mesh of base_scene that has vertex normals


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def turned(nrm):
    """other vertex normals: tilted, and not of unit length"""
    return nrm * [-1.0, 1.0, 1.0] + [0.0, 0.0, 0.4]


def moved_camera(sd):
    """the description's camera, dollied and turned a little (relative to the scene: far-from-origin scenes too)"""
    f, a = np.asarray(sd.lookfrom, np.float64), np.asarray(sd.lookat, np.float64)
    return dict(lookfrom=tuple(f + (0.3, 0.1, -0.2)), lookat=tuple(a + (0.05, -0.05, 0.0)), up=(0.03, 1.0, 0.0), vfov=sd.vfov - 3.0)


def moved_placements(sd):
    """every placement sheared and shifted a little: no transform is bit for bit the marked one"""
    x = original(sd).copy()
    k = np.arange(len(x), dtype=np.float64)
    x[:, :, :3] = x[:, :, :3] @ np.array([[1.0, 0.05, 0.0], [0.0, 0.95, 0.02], [0.03, 0.0, 1.02]])
    x[:, :, 3] += np.stack([0.04 + 0.01 * k, -0.03 * np.ones_like(k), 0.02 * np.cos(k)], axis=1)
    return x


class Case:
    """a marked description, the current one, and the scene brought from the first to the second through the calls
    that change a resident scene; `ends` is {mesh: (positions0, positions1)} or {mesh: (p0, p1, normals0, normals1)}"""

    def __init__(self, sd, ends, camera=None, xforms=None):
        self.sd, self.ends, self.marked_x = sd, ends, (original(sd) if sd.instance_mesh else None)
        cur = moved_scene(sd, camera, xforms)
        self.cur = with_arrays(cur, {m: (e[1], e[3] if len(e) == 4 else None) for m, e in ends.items()})
        self.motions = [(m,) + tuple(np.ascontiguousarray(a, np.float64) for a in e) for m, e in ends.items()]
        self.camera, self.xforms = camera, xforms

    def open(self, precision, builder=DEV, track=False):
        sc = capi.Scene(self.sd, precision=precision, builder=builder)
        if track:
            sc.track_vertices(True)
        sc.mark_frame()
        if self.xforms is not None:
            sc.set_instance_transforms(np.asarray(self.xforms))
        if self.camera is not None:
            sc.set_camera(self.cur.lookfrom, self.cur.lookat, self.cur.up, self.cur.vfov)
        sc.update_meshes({m: (e[1], e[3] if len(e) == 4 else None) for m, e in self.ends.items()})
        return sc

    def at(self, t):
        """the description at scene time t: the restatement's vertices, camera and transforms"""
        arrays = {m: (V.vertices(t, e[0], e[1])[0], V.vertices(t, e[2], e[3])[0] if len(e) == 4 else None) for m, e in self.ends.items()}
        return with_arrays(S.posed_scene(self.cur, t, camera_of(self.sd), self.marked_x), arrays)


def one_level(camera=True):
    """the emissive scene: its lamp — 20 of its 72 faces are area lights — deforms, and its vertex normals with it"""
    sd, lamp = emissive_scene()
    p0, n0 = sd.meshes[lamp].positions, sd.meshes[lamp].normals
    return Case(sd, {lamp: (p0, smooth(p0) - (0.0, 0.15, 0.0), n0, turned(n0))}, moved_camera(sd) if camera else None)


def two_level(camera=True, placements=True):
    """test_gpu_proto_update's scene: `both` — a mesh of the shape arrays AND a prototype — and prototype 0, the bent grid
    with vertex normals, deform; camera and placements move"""
    sd = scene()
    assert BOTH in proto_meshes(sd) and proto_meshes(sd)[0] == PROTO_GRID
    b, g = sd.meshes[BOTH], sd.meshes[PROTO_GRID]
    ends = {BOTH: (b.positions, smooth(b.positions)), PROTO_GRID: (g.positions, half_shrunk(g.positions, 0.5), g.normals, turned(g.normals))}
    return Case(sd, ends, moved_camera(sd) if camera else None, moved_placements(sd) if placements else None)


CASES = {"one-level": one_level, "two-level": two_level}


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 3 * 4099, 2 * 256 * 8 * 512 + 771])
def test_the_kernel_is_the_restatement_s(n):
    """odd tails, one element, a block edge, and — the last size: more pairs than 8 blocks of 256 lanes on each of 512
    CUs — more than one step of the grid-stride loop on any device.  Host entry and device entry (torch tensors); then
    arrays that start 8 bytes past a 16-byte boundary (one scalar element in front), and ends that do not agree mod 16
    (the scalar loop throughout)."""
    import torch

    a, b = V.edge_arrays(n, n)
    da, db = torch.from_numpy(a).to("cuda"), torch.from_numpy(b).to("cuda")
    for t in (0.0, 1.0 / 3.0, 0.5, 1.0):
        want, want_moved = V.vertices(t, a, b)
        got, moved = capi.shutter_vertices(da, db, t)
        assert got.is_cuda and same_bits(got.cpu().numpy(), want) and moved == want_moved, t
    got, moved = capi.shutter_vertices(a, b, 1.0 / 3.0)
    assert same_bits(got, V.vertices(1.0 / 3.0, a, b)[0]) and moved == V.vertices(1.0 / 3.0, a, b)[1]
    # moved: 0 when a is b's copy, at every t; 0 at t = 1 (finite ends); 1 when one element's last bit differs
    fa, fb = np.where(np.isfinite(a), a, 1.0) + 0.0, np.where(np.isfinite(b), b, 2.0) + 0.0  # (+ 0.0: no -0 either)
    assert capi.shutter_vertices(torch.from_numpy(fb).to("cuda"), torch.from_numpy(fb.copy()).to("cuda"), 0.3)[1] == 0
    got, moved = capi.shutter_vertices(torch.from_numpy(fa).to("cuda"), torch.from_numpy(fb).to("cuda"), 1.0)
    assert moved == 0 and same_bits(got.cpu().numpy(), fb)
    c = fb.copy()
    c[n // 2] = np.nextafter(c[n // 2], np.inf)
    got, moved = capi.shutter_vertices(torch.from_numpy(c).to("cuda"), torch.from_numpy(fb).to("cuda"), 0.0)  # (t = 0: the output IS c)
    assert moved == 1 and same_bits(got.cpu().numpy(), c)
    # other alignments, through the C entry: (a, b, out) all 8 mod 16; then out alone 8 mod 16
    if n <= 3 * 4099:
        C = capi.C
        pa, pb, po = (torch.zeros(n + 3, dtype=torch.float64, device="cuda") for _ in range(3))
        pa[1:n + 1], pb[1:n + 1] = da, db
        want = V.vertices(0.5, a, b)
        for oa, ob, oo in ((1, 1, 1), (0, 0, 1)):
            pa[oa:n + oa], pb[ob:n + ob] = da, db
            po.fill_(7.0)
            moved = C.c_int32(-1)
            assert pa.data_ptr() % 16 == 0 and capi.lib().take_hip_shutter_vertices_device(pa.data_ptr() + 8 * oa, pb.data_ptr() + 8 * ob, n, 0.5, po.data_ptr() + 8 * oo,
                                                                                          C.byref(moved), None) == 0
            out = po.cpu().numpy()
            assert same_bits(out[oo:n + oo], want[0]) and moved.value == want[1], (oa, ob, oo)
            assert (out[:oo] == 7.0).all() and (out[n + oo:] == 7.0).all(), (oa, ob, oo)  # nothing outside the n doubles is written


# ------------------------------------------------------------------ 2. no motion is render_shutter, and no rebuild
@pytest.mark.parametrize("levels", ["one-level", "two-level"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_motion_is_no_change_and_no_rebuild(precision, levels):
    sd = base_scene() if levels == "one-level" else scene()
    meshes = (GRID, 1) if levels == "one-level" else (BOTH, PROTO_GRID)
    motions = [(m, sd.meshes[m].positions, sd.meshes[m].positions.copy()) for m in meshes]
    motions[0] += (sd.meshes[meshes[0]].normals, sd.meshes[meshes[0]].normals.copy()) if sd.meshes[meshes[0]].normals is not None else ()
    sc = capi.Scene(sd, precision=precision, builder=HOST)
    try:
        want = sc.render(spp=7, max_depth=DEPTH, seed=SEED)
        sc.mark_frame()
        stats, built = sc.stats(), sc.build_info()
        assert np.array_equal(sc.render_shutter(spp=7, max_depth=DEPTH, seed=SEED, slices=3), want)
        assert np.array_equal(sc.render_shutter_meshes(motions, spp=7, max_depth=DEPTH, seed=SEED, slices=3), want)
        assert np.array_equal(sc.render_shutter_meshes([], spp=7, max_depth=DEPTH, seed=SEED, slices=3), want)
        assert sc.stats() == stats and sc.build_info() == built  # the host's trees are still there: nothing was rebuilt
        assert np.array_equal(sc.render(spp=7, max_depth=DEPTH, seed=SEED), want)
    finally:
        sc.close()


# ------------------------------------------------------------------ 3. one slice is the posed scene
@pytest.mark.parametrize("t", [0.25, 0.5])
@pytest.mark.parametrize("levels", ["one-level", "two-level"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_slice_is_the_scene_newly_created_at_that_time(precision, levels, t):
    case = CASES[levels]()
    sc = case.open(precision)
    try:
        got = sc.render_shutter_meshes(case.motions, spp=4, max_depth=DEPTH, seed=SEED, open=t, close=t, slices=1)
        after = sc.render(spp=4, max_depth=DEPTH, seed=SEED)
    finally:
        sc.close()
    assert list(capi.shutter_plan(4, t, t, 1)[1]) == [t]
    assert np.array_equal(got, fresh_render(case.at(t), precision, 4))
    at_mark, at_now = fresh_render(case.sd, precision, 4), fresh_render(case.cur, precision, 4)
    assert not np.array_equal(got, at_mark) and not np.array_equal(got, at_now)
    assert np.array_equal(after, at_now)  # the scene is at its current vertices and pose again


# ------------------------------------------------------------------ 4. K slices are the sample-weighted mean
@pytest.mark.parametrize("levels", ["one-level", "two-level"])
@pytest.mark.parametrize("precision", [F64, F32])
def test_slices_are_the_sample_weighted_mean_of_the_posed_renders(precision, levels):
    N, K = 7, 3
    case = CASES[levels]()
    sc = case.open(precision)
    try:
        got = sc.render_shutter_meshes(case.motions, spp=N, max_depth=DEPTH, seed=SEED, slices=K).astype(np.float64)
    finally:
        sc.close()
    first, time = S.plan(N, 0.0, 1.0, K)
    assert list(first) == [0, 2, 4, 7]
    want, mag = np.zeros_like(got), np.zeros_like(got)
    for k in range(K):
        psc = capi.Scene(case.at(time[k]), precision=precision, builder=DEV)
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
    print(f"{levels}, {'f64' if precision == F64 else 'f32'}: max |N got - want| / (eps mag) = {ratio:.3f} (bar {4 * (N + 2)})")
    assert (mag > 0).mean() > 0.9
    assert (err <= 4 * (N + 2) * eps * mag).all(), ratio


# ------------------------------------------------------------------ 5. before = after
@pytest.mark.parametrize("levels", ["one-level", "two-level"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_scene_is_as_before_after_a_render_and_after_a_refusal(precision, levels):
    import torch

    case = CASES[levels]()
    sc = case.open(precision, track=True)
    rays = abi(scene_rays(4096, 3, tmin=tmin_of(precision)), precision)
    try:
        def state():
            return sc.trace_closest(rays).tobytes(), sc.trace_any(rays).tobytes(), sc.render(spp=3, max_depth=DEPTH, seed=SEED).tobytes()

        before, motion, tracking = state(), sc.render_motion(), sc.tracking_info()
        assert tracking["flags"] == D.TAKE_TRACK_VERTICES and tracking["marked_bytes"] > 0  # (case.open's update made the copy)
        sc.render_shutter_meshes(case.motions, spp=5, max_depth=DEPTH, seed=SEED, slices=3)
        assert state() == before and sc.tracking_info() == tracking
        # ... and as a scene newly created at the current frame
        fresh = capi.Scene(case.cur, precision=precision, builder=DEV)
        try:
            same_hits(sc, fresh, rays)
            assert np.array_equal(sc.render(spp=3, max_depth=DEPTH, seed=SEED), fresh.render(spp=3, max_depth=DEPTH, seed=SEED))
        finally:
            fresh.close()
        # a progressive sequence ends as render_shutter ends it
        buf = torch.zeros((case.sd.height, case.sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED, restart=True) == 2
        sc.render_shutter(spp=5, max_depth=DEPTH, seed=SEED, slices=3)
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED) == 2
        after_shutter = buf.cpu().numpy().copy()
        sc.render_shutter_meshes(case.motions, spp=5, max_depth=DEPTH, seed=SEED, slices=3)
        assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED) == 2
        assert np.array_equal(buf.cpu().numpy(), after_shutter)
        # a refused call: a NaN in positions0 of the last motion shows at slice 0, in the loop
        bad = [tuple(m) for m in case.motions]
        p0 = bad[-1][1].copy()
        face = case.sd.meshes[bad[-1][0]].indices
        p0[int(np.asarray(face).reshape(-1)[0]), 1] = np.nan
        bad[-1] = (bad[-1][0], p0) + bad[-1][2:]
        with pytest.raises(capi.TakeError, match=r"slice 0: mesh \d+: vertex \d+: a new position is not finite") as e:
            sc.render_shutter_meshes(bad, spp=5, max_depth=DEPTH, seed=SEED, slices=3)
        assert e.value.code == D.TAKE_E_INVALID
        assert state() == before and sc.tracking_info() == tracking
        # the mark and vertex tracking are untouched: the motion pass sees what it saw
        again = sc.render_motion()
        for n in motion:
            assert np.array_equal(again[n], motion[n]), n
    finally:
        sc.close()


# ------------------------------------------------------------------ 6. inputs; the library against itself
@pytest.mark.parametrize("levels", ["one-level", "two-level"])
@pytest.mark.parametrize("precision", [F32, MIXED])
def test_device_tensors_batches_and_strips_change_nothing(precision, levels):
    import torch

    case = CASES[levels]()
    sc = case.open(precision)
    try:
        kw = dict(spp=7, max_depth=DEPTH, seed=SEED, slices=3)
        whole = sc.render_shutter_meshes(case.motions, **kw)
        assert not np.array_equal(whole, sc.render_shutter(**kw))  # the vertices do blur
        on_device = [(m[0],) + tuple(torch.from_numpy(a).to("cuda") for a in m[1:]) for m in case.motions]
        assert np.array_equal(sc.render_shutter_meshes(on_device, **kw), whole)
        mixed = [on_device[0]] + list(case.motions[1:])  # device arrays for one mesh, host arrays for the other
        assert np.array_equal(sc.render_shutter_meshes(mixed, **kw), whole)
        for spb in (1, 2, 5):
            assert np.array_equal(sc.render_shutter_meshes(case.motions, samples_per_batch=spb, **kw), whole), spb
        for stride in (2, 3):
            out = np.zeros_like(whole)
            for first in range(stride):
                out[sc.rows(first, stride)] = sc.render_shutter_meshes(on_device, strip_first=first, strip_stride=stride, **kw)
            assert np.array_equal(out, whole), stride
        buf = torch.zeros(whole.shape, dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        sc.render_shutter_meshes_device(buf, on_device, **kw)
        assert np.array_equal(buf.cpu().numpy(), whole)
    finally:
        sc.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_a_lens_composes(precision):
    case = two_level()
    sc = case.open(precision)
    try:
        sc.set_lens(0.05, 3.5)
        got = sc.render_shutter_meshes(case.motions, spp=4, max_depth=DEPTH, seed=SEED, slices=1)
        sc.set_lens(0.0)
        without = sc.render_shutter_meshes(case.motions, spp=4, max_depth=DEPTH, seed=SEED, slices=1)
    finally:
        sc.close()
    assert np.array_equal(got, fresh_render(case.at(0.5), precision, 4, lens=(0.05, 3.5)))
    assert np.array_equal(without, fresh_render(case.at(0.5), precision, 4)) and not np.array_equal(got, without)


def test_vertices_blur_alone_under_the_current_transforms():
    """camera and placements unmoved, the meshes alone deform: every slice updates under the current transforms, and the
    placements' records are never made again.  A shutter that stays at t = 0 renders the marked vertices."""
    case = two_level(camera=False, placements=False)
    sc = case.open(F32)
    try:
        got = sc.render_shutter_meshes(case.motions, spp=4, max_depth=DEPTH, seed=SEED, open=0.5, close=0.5, slices=1)
        assert np.array_equal(got, fresh_render(case.at(0.5), F32, 4))
        before = sc.render(spp=3, max_depth=DEPTH, seed=SEED)
        at_mark = sc.render_shutter_meshes(case.motions, spp=4, max_depth=DEPTH, seed=SEED, open=0.0, close=0.0, slices=1)
        assert np.array_equal(at_mark, fresh_render(case.sd, F32, 4))
        assert np.array_equal(sc.render(spp=3, max_depth=DEPTH, seed=SEED), before)
    finally:
        sc.close()


# ------------------------------------------------------------------ 7. refusals that need a scene
def test_refusals_against_the_scene():
    sd = scene()
    g, b = sd.meshes[PROTO_GRID], sd.meshes[BOTH]
    sc = capi.Scene(sd, precision=F32, builder=DEV)
    try:
        good = [(PROTO_GRID, g.positions, smooth(g.positions))]
        with pytest.raises(capi.TakeError, match="no marked frame") as e:
            sc.render_shutter_meshes(good, spp=2, max_depth=DEPTH)
        assert e.value.code == D.TAKE_E_INVALID
        sc.mark_frame()
        before = sc.render(spp=2, max_depth=DEPTH, seed=SEED)
        for motions, msg in (([(len(sd.meshes), g.positions, g.positions)], "motion 0: mesh index out of range"),
                             (good + [(BOTH, b.positions, b.positions, b.positions, b.positions)], "motion 1: normals given for a mesh without vertex normals")):
            with pytest.raises(capi.TakeError, match=msg) as e:
                sc.render_shutter_meshes(motions, spp=2, max_depth=DEPTH)
            assert e.value.code == D.TAKE_E_INVALID
        # the update's own refusal, found in the loop: a NaN in positions0 reaches every slice with t < 1; the first is named
        p0 = g.positions.copy()
        p0[int(np.asarray(g.indices).reshape(-1)[5]), 2] = np.nan
        with pytest.raises(capi.TakeError, match=rf"slice 0: mesh {PROTO_GRID}: vertex \d+: a new position is not finite"):
            sc.render_shutter_meshes([(PROTO_GRID, p0, g.positions)], spp=3, max_depth=DEPTH, slices=3)
        assert np.array_equal(sc.render(spp=2, max_depth=DEPTH, seed=SEED), before)
    finally:
        sc.close()
    # "unsupported", in the update's words: a scene flattened from instances
    from test_instancing import small

    flat = capi.Scene(small(4, 20, 4), precision=F32, flatten_instances=True)
    try:
        flat.mark_frame()
        m = flat.sd.meshes[0]
        with pytest.raises(capi.TakeError, match="unsupported: the scene was flattened from instances"):
            flat.render_shutter_meshes([(0, m.positions, m.positions)], spp=2, max_depth=DEPTH)
    finally:
        flat.close()

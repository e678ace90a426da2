"""Re-posing a resident scene: take_hip_scene_set_instance_transforms (new transforms for all placements of a two-level
scene: k_placement_records, k_placement_boxes_resident, k_widen_tight, a new top-level LBVH, the prototypes' trees
copied behind it — take_amd/csrc/tk_build_gpu.h, tk_build.hip: repose_two_level_device), its _device twin and
take_hip_scene_set_camera.  The yardstick is always a FRESH capi.Scene built from the description with the new
transforms (camera): hits and images bit for bit (np.array_equal) — results do not depend on the tree, and the records
are the ones a fresh scene_create computes."""
import copy
import time

import numpy as np
import pytest

from helpers import random_rays
from take_amd import capi
from take_amd import cdefs as D
from test_gpu_device_build_instanced import (ALL_EXACT, OFFSET, abi, built_by, everything_scene, random_linear, render, same_hits,
                                             scene_rays, scene_with_node_format, sheared_placements, two_big_prototypes)
from test_instancing import small

pytestmark = pytest.mark.gpu
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]


def posed(sd, xforms):
    """the description with other transforms (the arrays are shared, the placement lists are not)"""
    out = copy.copy(sd)
    out.instance_xform = [np.array(x, np.float64).reshape(3, 4) for x in xforms]
    assert len(out.instance_xform) == len(sd.instance_mesh)
    return out


def original(sd):
    return np.array(sd.instance_xform, np.float64)


def drawn(sd, seed, spread, scale=0.6, offset=(0.0, 0.0, 0.0)):
    """new transforms for every placement: random_linear (rotation x non-uniform scale x shear) plus new translations in
    [-spread, spread]^3 — spread out (1.0) or clustered (0.05)"""
    rng = np.random.default_rng(seed)
    n = len(sd.instance_mesh)
    lin = random_linear(rng, n)
    t = rng.uniform(-spread, spread, (n, 3)) + np.asarray(offset)
    return np.stack([np.concatenate([scale * lin[k], t[k][:, None]], axis=1) for k in range(n)])


def tmin_of(precision):
    return 1e-7 if precision == F64 else 1e-4


def same_everything(a, b, precision, rays8, spp=4, max_depth=6, seed=5):
    """hit tables and occlusion (F32 / F64: a mixed scene's hooks are its f64 side's, compared through the images at all-exact
    bounces) and images, bit for bit"""
    if precision != MIXED:
        hits = same_hits(a, b, abi(rays8, precision))
        assert (hits["shape_id"] >= 0).mean() > 0.01
    for eb in ((0, ALL_EXACT) if precision == MIXED else (0,)):
        ia, ib = render(a, eb, spp=spp, max_depth=max_depth, seed=seed), render(b, eb, spp=spp, max_depth=max_depth, seed=seed)
        assert np.array_equal(ia, ib), eb
        assert np.isfinite(ia).all() and ia.mean() > 0


# ------------------------------------------------------------------ 1. equals a fresh scene
@pytest.mark.parametrize("builder", [DEV, HOST])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_updated_scene_equals_a_fresh_scene(precision, builder):
    """spread out, then clustered: the top-level tree's node count changes (the prototypes' nodes move, their child words
    and the placements' roots with them).  A is built by the device in one run and by the host SAH in the other."""
    sd = everything_scene()
    rays = scene_rays(8192, 3, tmin=tmin_of(precision))
    a = capi.Scene(sd, precision=precision, builder=builder)
    try:
        assert a.build_info() == built_by(precision, builder)
        n_nodes = [a.stats()["n_nodes"]]
        for seed, spread in ((1, 1.0), (2, 0.05)):
            x = drawn(sd, seed, spread)
            a.set_instance_transforms(x)
            n_nodes.append(a.stats()["n_nodes"])
            b = capi.Scene(posed(sd, x), precision=precision, builder=DEV)
            try:
                assert a.stats()["n_prims"] == b.stats()["n_prims"]
                same_everything(a, b, precision, rays)
            finally:
                b.close()
        print(f"\nnodes: created {n_nodes[0]}, spread out {n_nodes[1]}, clustered {n_nodes[2]}")
        assert len(set(n_nodes)) > 1, n_nodes
    finally:
        a.close()


# ------------------------------------------------------------------ 2. round trip and repetition
@pytest.mark.parametrize("precision", PRECISIONS)
def test_round_trip_and_repetition(precision):
    sd = everything_scene()
    rays = abi(scene_rays(8192, 3, tmin=tmin_of(precision)), precision)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        h0 = a.trace_closest(rays) if precision != MIXED else None
        i0 = a.render(spp=4, max_depth=6, seed=5)
        x = drawn(sd, 7, 0.7)
        a.set_instance_transforms(x)
        i1 = a.render(spp=4, max_depth=6, seed=5)
        assert not np.array_equal(i0, i1)
        a.set_instance_transforms(x)  # the same again: nothing changes
        assert np.array_equal(i1, a.render(spp=4, max_depth=6, seed=5))
        a.set_instance_transforms(original(sd))
        assert np.array_equal(i0, a.render(spp=4, max_depth=6, seed=5))
        if h0 is not None:
            h2 = a.trace_closest(rays)
            for f in ("shape_id", "t", "u", "v"):
                assert np.array_equal(h0[f], h2[f]), f
    finally:
        a.close()


# ------------------------------------------------------------------ 3. the transforms in device memory
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_entry_point(precision):
    import torch

    sd = small(20, 100, 16)
    x = drawn(sd, 3, 0.8, scale=1.0)
    a, b = capi.Scene(sd, precision=precision, builder=DEV), capi.Scene(sd, precision=precision, builder=DEV)
    try:
        a.set_instance_transforms(x)
        t = torch.from_numpy(x).to("cuda")
        b.set_instance_transforms(t)
        ia = a.render(spp=4, max_depth=6, seed=1)
        assert np.array_equal(ia, b.render(spp=4, max_depth=6, seed=1))
        b.set_instance_transforms(original(sd))
        b.set_instance_transforms(int(t.data_ptr()))  # an integer device pointer
        assert np.array_equal(ia, b.render(spp=4, max_depth=6, seed=1))
        b.set_instance_transforms(original(sd))
        assert not np.array_equal(ia, b.render(spp=4, max_depth=6, seed=1))
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 4. placement boxes, through hits
@pytest.mark.parametrize("precision", [F32, F64])
def test_sheared_placements_no_shapes(precision):
    """placements only (no shape records: an empty head), both pads of k_placement_pad on boxes made from the records:
    60 000 rays bit-identical to a fresh build; in double also the containment assertions of
    test_placement_boxes_contain_the_placed_geometry against the flattened fresh scene"""
    sd = sheared_placements()
    rng = np.random.default_rng(5)
    x = np.stack([np.concatenate([lin, rng.uniform(-0.8, 0.8, (3, 1))], axis=1) for lin in random_linear(rng, 90, shear=0.8)])
    rays = abi(random_rays(60000, 17, tmin=tmin_of(precision)), precision)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(posed(sd, x), precision=precision, builder=DEV)
    try:
        a.set_instance_transforms(x)
        ha = same_hits(a, b, rays)
        assert (ha["shape_id"] >= 0).mean() > 0.5
        assert np.array_equal(a.render(spp=1, max_depth=2, seed=5), b.render(spp=1, max_depth=2, seed=5))
        if precision == F64:
            c = capi.Scene(posed(sd, x).flattened(), precision=F64, builder=HOST)
            try:
                ha, hc = a.trace_closest(rays), c.trace_closest(rays)
                hit = hc["shape_id"] >= 0
                assert hit.sum() > 10000
                assert (ha["shape_id"][hit] >= 0).all()
                assert (ha["t"][hit] <= hc["t"][hit] + 1e-13 * np.maximum(1.0, hc["t"][hit])).all()
                assert np.array_equal(a.trace_any(rays).astype(bool)[hit], hit[hit])
            finally:
                c.close()
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 5. coincident placements
@pytest.mark.parametrize("precision", [F32, F64])
def test_placements_moved_onto_one_transform_tie_on_the_instance_id(precision):
    """placements 0 and 3 (one prototype) moved onto ONE transform in front of the camera: every hit inside them carries
    the larger instance id, as in test_coincident_placements_tie_on_the_instance_id"""
    sd = everything_scene()
    assert sd.instance_mesh[0] == sd.instance_mesh[3]
    faces = [sd.meshes[m].indices.shape[0] for m in sd.instance_mesh]
    base = sd.n_shapes + np.concatenate([[0], np.cumsum(faces)])
    x = original(sd)
    lin = random_linear(np.random.default_rng(8), 1)[0]
    x[0] = x[3] = np.concatenate([2.0 * lin, np.array([[0.0], [0.1], [1.6]])], axis=1)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    b = capi.Scene(posed(sd, x), precision=precision, builder=DEV)
    try:
        a.set_instance_transforms(x)
        ids = same_hits(a, b, abi(scene_rays(20000, 9), precision))["shape_id"]
        assert ((ids >= base[3]) & (ids < base[4])).sum() > 20
        assert not ((ids >= base[0]) & (ids < base[1])).any()
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 6. far from the origin
@pytest.mark.parametrize("precision", PRECISIONS)
def test_translated_far_from_the_origin_through_the_update(precision):
    """the scene is created far from the origin, its placements around the origin; the update takes them there"""
    sd = everything_scene(OFFSET)
    near = original(sd)
    near[:, :, 3] -= OFFSET
    x = drawn(sd, 4, 0.8, offset=OFFSET)
    a = capi.Scene(posed(sd, near), precision=precision, builder=DEV)
    b = capi.Scene(posed(sd, x), precision=precision, builder=DEV)
    try:
        a.set_instance_transforms(x)
        same_everything(a, b, precision, scene_rays(8192, 4, OFFSET, tmin=1e-7 if precision == F64 else 1e-3))
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 7. full-width nodes
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_wide_scene_stays_wide(precision):
    import os

    if os.environ.get("TAKE_HIP_NODES"):
        pytest.skip("experiment knobs select the node format")
    sd = everything_scene()
    x = drawn(sd, 6, 0.3)
    a = scene_with_node_format("wide", sd, precision=precision, builder=DEV)
    b = capi.Scene(posed(sd, x), precision=precision, builder=DEV)
    try:
        a.render(spp=1, max_depth=2, seed=1)
        wide = a.counters()["node_bytes"]
        assert wide in {F32: (128,), F64: (256,), MIXED: (128, 256)}[precision]  # sizeof(Node4<float>), sizeof(Node4<double>)
        a.set_instance_transforms(x)
        assert np.array_equal(a.render(spp=4, max_depth=6, seed=2), b.render(spp=4, max_depth=6, seed=2))
        assert a.counters()["node_bytes"] == wide and b.counters()["node_bytes"] == 64
        if precision != MIXED:
            same_hits(a, b, abi(scene_rays(8192, 6, tmin=tmin_of(precision)), precision))
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------ 8. refusals leave the scene unchanged
def refused(sc, x, starts=None):
    with pytest.raises(capi.TakeError) as e:
        sc.set_instance_transforms(x)
    assert e.value.code == D.TAKE_E_INVALID
    msg = str(e.value).split(": ", 1)[1]
    if starts:
        assert msg.startswith(starts), msg
    return msg


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_leave_the_scene_unchanged(precision, monkeypatch):
    sd = small(20, 100, 16)
    good = drawn(sd, 3, 0.8, scale=1.0)

    def images(sc):
        return [render(sc, eb, spp=2, max_depth=6, seed=1) for eb in ((0, ALL_EXACT) if precision == MIXED else (0,))]

    def unchanged(sc, before):
        return all(np.array_equal(p, q) for p, q in zip(before, images(sc)))

    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        before = images(a)
        refused(a, good[:-1])  # a wrong n
        assert unchanged(a, before)
        zero = good.copy()
        zero[7] = 0.0
        zero[12] = 0.0
        assert "instance 7" in refused(a, zero)  # the first bad placement
        assert unchanged(a, before)
        nan = good.copy()
        nan[5, 1, 1] = np.nan
        assert "instance 5" in refused(a, nan)
        assert unchanged(a, before)
        inf = good.copy()
        inf[19, 2, 3] = np.inf  # a translation: the determinant does not see it
        assert "instance 19" in refused(a, inf)
        assert unchanged(a, before)
        a.set_instance_transforms(good)  # ... and the scene still takes an update
        assert not unchanged(a, before)
    finally:
        a.close()
    plain = copy.copy(sd)
    plain.instance_mesh, plain.instance_material, plain.instance_xform = [], [], []
    for sc in (capi.Scene(plain, precision=precision), capi.Scene(sd, precision=precision, flatten_instances=True)):
        try:
            before = images(sc)
            refused(sc, good)
            refused(sc, good[:0].reshape(0, 3, 4))
            assert unchanged(sc, before)
        finally:
            sc.close()
    monkeypatch.setenv("TAKE_HIP_BRAID", "4")
    sc = capi.Scene(small(20, 300, 16), precision=precision, builder=HOST)
    monkeypatch.delenv("TAKE_HIP_BRAID")
    try:
        before = images(sc)
        refused(sc, good, starts="unsupported")
        assert unchanged(sc, before)
    finally:
        sc.close()


# ------------------------------------------------------------------ 9. progressive rendering
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_update_ends_a_progressive_sequence(precision):
    import torch

    sd = small(20, 100, 16)
    x = drawn(sd, 3, 0.8, scale=1.0)
    a = capi.Scene(sd, precision=precision, builder=DEV)
    try:
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4, restart=True) == 2
        assert a.render_accumulate(buf.data_ptr(), 2, 6, seed=4) == 4
        a.set_instance_transforms(x)
        assert capi.lib().take_hip_accumulated_samples(a.h) == 0
        with pytest.raises(capi.TakeError) as e:
            a.render_accumulate(buf.data_ptr(), 3, 6, seed=4)
        assert e.value.code == D.TAKE_E_INVALID and "restart" in str(e.value)
        assert a.render_accumulate(buf.data_ptr(), 3, 6, seed=4, restart=True) == 3
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), a.render(spp=3, max_depth=6, seed=4))
        # the camera ends a sequence in the same way
        assert a.render_accumulate(buf.data_ptr(), 3, 6, seed=4, restart=True) == 3
        a.set_camera((0.5, 0.2, 3.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0)
        with pytest.raises(capi.TakeError) as e:
            a.render_accumulate(buf.data_ptr(), 1, 6, seed=4)
        assert e.value.code == D.TAKE_E_INVALID
        assert a.render_accumulate(buf.data_ptr(), 1, 6, seed=4, restart=True) == 1
    finally:
        a.close()


# ------------------------------------------------------------------ 10. camera
@pytest.mark.parametrize("precision", PRECISIONS)
def test_set_camera(precision):
    cam = dict(lookfrom=(1.0, 0.6, 3.2), lookat=(0.1, -0.1, 0.0), up=(0.1, 1.0, 0.0), vfov=47.0)
    with_placements = everything_scene()
    without = copy.copy(with_placements)
    without.instance_mesh, without.instance_material, without.instance_xform = [], [], []
    for sd in (with_placements, without):
        moved = copy.copy(sd)
        for k, v in cam.items():
            setattr(moved, k, v)
        a, b = capi.Scene(sd, precision=precision), capi.Scene(moved, precision=precision)
        try:
            before = a.render(spp=2, max_depth=6, seed=3)
            with pytest.raises(capi.TakeError) as e:
                a.set_camera(width=sd.width + 1, **cam)
            assert e.value.code == D.TAKE_E_INVALID
            with pytest.raises(capi.TakeError):
                a.set_camera(height=sd.height // 2, **cam)
            assert np.array_equal(before, a.render(spp=2, max_depth=6, seed=3))
            a.set_camera(**cam)
            for eb in ((0, ALL_EXACT) if precision == MIXED else (0,)):
                ia = render(a, eb, spp=2, max_depth=6, seed=3)
                assert np.array_equal(ia, render(b, eb, spp=2, max_depth=6, seed=3))
                assert not np.array_equal(ia, before)
        finally:
            a.close(), b.close()


# ------------------------------------------------------------------ 11. size and time
def test_two_500k_triangle_prototypes_update_is_faster_than_create():
    """an update does a strict subset of a fresh device build's work — no uploads, no prototype trees — so it must be
    faster; no ratio is fixed"""
    sd = two_big_prototypes(500_000, 64, 96)
    x = drawn(sd, 11, 0.8, scale=1.0)
    a = capi.Scene(sd, precision=F32, builder=DEV)
    try:
        assert a.build_info() == built_by(F32, DEV)
        t0 = time.perf_counter()
        a.set_instance_transforms(x)
        t_update = time.perf_counter() - t0
        fresh = posed(sd, x)
        t0 = time.perf_counter()
        b = capi.Scene(fresh, precision=F32, builder=DEV)
        t_create = time.perf_counter() - t0
        try:
            print(f"\n2 x 500k triangles x 64 placements, f32: set_instance_transforms {1e3 * t_update:.2f} ms, "
                  f"fresh device-built scene_create {1e3 * t_create:.1f} ms")
            assert np.array_equal(a.render(spp=1, max_depth=50, seed=4), b.render(spp=1, max_depth=50, seed=4))
            assert t_update < t_create, (t_update, t_create)
        finally:
            b.close()
    finally:
        a.close()

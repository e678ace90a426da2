"""The trace kernels (tk_trace_quad.h: k_trace_group through the C-ABI hooks, and the render loop's instance of it) on
the rays and the scene the rest of the suite never sends them: tests/trace_edge_rays.py — axis-parallel and
tiny-component directions, far origins, unnormalised directions, a tmin per ray, tmin / tmax exactly at a hit distance,
and the hairball, whose traversal stack leaves the 15 LDS levels for the global spill area (tq_spill_store /
tq_spill_load, StackSpill's stride over the persistent grid; hairball_deep_marker puts the instance return marker up there).

Only a few primitive tests of a hairball ray hang under entries beyond level 15 (under 1 %), so hit tables alone see a
broken spill area on tens of rays (the CPU file measures it with hostsim's drop_from).  The visit counters of the
counting kernel are the sharp check: on rays that hit nothing and have no tmax the limit never shrinks, the visited set
is exactly the nodes whose box test passes, whatever the order — the kernel's node, leaf and primitive counts must EQUAL
hostsim's, and one lost or repeated entry on any ray moves them.

Bars: against the oracle's exhaustive search those of tests/test_trace_edges_cpu.py (trace_edge_rays.check_against_brute:
hit / miss, t bit for bit; u, v bit for bit on the same shape; another shape only on an exact tie, towards the larger
(u, v), on at most 10 % of a batch); against hostsim_trace — the per-lane traversal of tk_traverse.h on the same host SAH
4-wide tree — (shape_id, t, u, v) bit for bit on every ray, no exclusions; trace_any == (shape_id >= 0)."""
import numpy as np
import pytest
import torch  # (before the library is loaded, as tests/test_gpu_mixed.py does: one HIP runtime in the process)

import oracle
import trace_edge_rays as E
from helpers import golden_scene, hostsim_trace, hostsim_trace_stats, rays_to_abi, rmse
from take_amd import capi
from take_amd import cdefs as D

pytestmark = pytest.mark.gpu
F32, F64 = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64
HOST, DEV = D.TAKE_BUILDER_HOST_SAH, D.TAKE_BUILDER_DEVICE_LBVH
# configuration -> (TAKE_HIP_NODES, builder, the tree is hostsim's: host SAH, 4-wide)
CONFIGS = {"default": ("", D.TAKE_BUILDER_AUTO, True), "wide": ("wide", HOST, True), "lbvh": ("", DEV, False), "q8": ("q8", HOST, False)}
# The persistent grid holds 5 blocks x 256 rays per CU: about 330 k ray slots on this part.  80 tiles of the 5000 rays
# put 400 k rays in flight, so every block of the grid has rays deep in the spill area at the same time.
TILES = 80


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert capi.device_count() >= 1


def built_by(precision, builder):
    return {"f32": -1 if precision == F64 else builder, "f64": -1 if precision == F32 else builder}


def make_scene(sd, precision, config, monkeypatch):
    fmt, builder, _ = CONFIGS[config]
    monkeypatch.setenv("TAKE_HIP_NODES", fmt)  # read when a scene is built — by capi.Scene and by hostsim alike
    sc = capi.Scene(sd, precision=precision, builder=builder)
    assert sc.build_info() == built_by(precision, HOST if builder == D.TAKE_BUILDER_AUTO else builder), sc.build_info()
    return sc


def trace(sc, rays8, precision):
    a = rays_to_abi(rays8, precision)
    return E.hits_table(sc.trace_closest(a)), sc.trace_any(a).astype(bool)


def same_table(got, want, what):
    for k, col in enumerate(("shape_id", "t", "u", "v")):
        assert np.array_equal(got[:, k], want[:, k]), f"{what}: {col} differs on {np.sum(got[:, k] != want[:, k])} rays"


# ------------------------------------------------------------------ 1. the ray families
@pytest.mark.parametrize("precision", [F32, F64])
@pytest.mark.parametrize("name,config", [(n, "default") for n in E.SCENES] + [(n, c) for n in ("cbox", "hairball") for c in ("wide", "lbvh", "q8")])
def test_edge_rays(name, config, precision, monkeypatch):
    sd, cases = E.scene(name), E.cases(name, precision)
    rays = np.concatenate([r for _, r, _ in cases])  # one call: tmin and tmax differ from ray to ray across the batches
    sc = make_scene(sd, precision, config, monkeypatch)
    try:
        got, occ = trace(sc, rays, precision)
        if name == "hairball" and CONFIGS[config][2]:
            st = sc.stats()
            assert (st["n_nodes"], st["depth"]) == (E.HAIRBALL_NODES, E.HAIRBALL_DEPTH), st  # the tree of the CPU test's max_stack
    finally:
        sc.close()
    at = 0
    for label, r, want in cases:
        g = got[at:at + len(r)]
        n_hit, n_tie = E.check_against_brute(g, want, f"{name} {config} {label}")
        assert np.array_equal(occ[at:at + len(r)], g[:, 0] >= 0), f"{name} {config} {label}: trace_any"
        at += len(r)
    if CONFIGS[config][2]:  # "bit-identical to the per-lane traversal" (tk_trace_quad.h): ties and keys included
        same_table(got, hostsim_trace(sd, precision, rays).astype(np.float64), f"{name} {config} against hostsim")


# ------------------------------------------------------------------ 2. the spilled stack
def tiled(sc, rays8, precision):
    """TILES copies of the rays in one call -> (first tile's table, first tile's occlusion); all tiles must agree"""
    got, occ = trace(sc, np.tile(rays8, (TILES, 1)), precision)
    assert got.shape[0] >= 400_000
    got, occ = got.reshape(TILES, -1, 4), occ.reshape(TILES, -1)
    for k, col in enumerate(("shape_id", "t", "u", "v")):
        assert (got[:, :, k] == got[0, :, k]).all(), f"{col}: tiles differ on {np.sum((got[:, :, k] != got[0, :, k]).any(axis=0))} rays"
    assert (occ == occ[0]).all(), f"trace_any: tiles differ on {np.sum((occ != occ[0]).any(axis=0))} rays"
    return got[0], occ[0]


@pytest.fixture(scope="module")
def spill_reference():
    """(kind, precision) -> (rays, exhaustive search): the issue's 5000 random rays, and 5000 aimed at needles"""
    out = {}
    for precision in (F32, F64):
        osc = oracle.OracleScene(E.scene("hairball"), precision=precision)
        for kind, rays in (("random", E.spill_rays(precision)), ("needles", E.needle_rays(precision))):
            out[kind, precision] = (rays, osc.isect_brute(rays))
        osc.close()
    return out


def spilled_stack(precision, config, kind, spill_reference, monkeypatch):
    rays, want = spill_reference[kind, precision]
    sd = E.scene("hairball")
    sc = make_scene(sd, precision, config, monkeypatch)
    try:
        got, occ = tiled(sc, rays, precision)
    finally:
        sc.close()
    n_hit, _ = E.check_against_brute(got, want, f"hairball {config} {kind}")
    assert n_hit >= (20 if kind == "random" else 4900)
    assert np.array_equal(occ, want[:, 0] >= 0)
    if CONFIGS[config][2]:
        st = hostsim_trace_stats(sd, precision, rays)
        assert st["max_stack"] >= E.LDS_LEVELS + 1 and st["rays_deep"] >= 1000, st
        same_table(got, hostsim_trace(sd, precision, rays).astype(np.float64), "hairball against hostsim")


@pytest.mark.parametrize("config", ["default", "lbvh"])
@pytest.mark.parametrize("precision", [F32, F64])
def test_spilled_stack(precision, config, spill_reference, monkeypatch):
    """400 k hairball rays in flight, a fifth of them with stack levels beyond LDS (test_trace_edges_cpu.py asserts 16+
    entries on this tree), in every block of the persistent grid at once.  All tiles agree; the first equals the
    exhaustive search and, on the host tree, the per-lane traversal."""
    spilled_stack(precision, config, "random", spill_reference, monkeypatch)


@pytest.mark.parametrize("config", ["default", "lbvh"])
@pytest.mark.parametrize("precision", [F32, F64])
def test_spilled_stack_on_rays_that_hit(precision, config, spill_reference, monkeypatch):
    """the same with the needle rays: two fifths beyond LDS, and all of them hit, so a lost subtree takes winners along"""
    spilled_stack(precision, config, "needles", spill_reference, monkeypatch)


def count_on_device(sc, rays8, precision, tiles):
    """`tiles` copies of the rays, device-resident, through take_hip_trace_closest_device with count_mode 0 and 1 ->
    the counters of the counting call.  The two hit tables and all tiles must be the same bytes."""
    flat = np.tile(rays_to_abi(rays8, precision), (tiles, 1))
    assert flat.shape[0] >= 400_000
    d_rays = torch.from_numpy(flat).cuda()
    tables = []
    for mode in (0, 1):
        d_hits = torch.zeros((flat.shape[0], 4), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")  # HitAoS: four words of the scene's Real
        sc.trace_closest_device(d_rays.data_ptr(), flat.shape[0], d_hits.data_ptr(), count_mode=mode)
        torch.cuda.synchronize()
        tables.append(d_hits.cpu().numpy().view(np.uint8).copy())
    counters = sc.counters()
    assert np.array_equal(tables[0], tables[1])
    first = tables[0].reshape(tiles, -1)
    assert (first == first[0]).all()
    return counters


def check_counts(sc, sd, precision, rays8, deep_at_least):
    """The rays without a tmax that hit nothing (by hostsim): their limit never shrinks, so nothing is culled and the
    order of the visits cannot matter — the visit counts are a property of the tree and the box test alone, and the
    kernel's must equal the per-lane traversal's."""
    quiet = rays8[(hostsim_trace(sd, precision, rays8)[:, 0] < 0) & np.isinf(rays8[:, 7])]
    tiles = -(-400_000 // len(quiet))
    st = hostsim_trace_stats(sd, precision, quiet)
    assert st["rays_deep"] >= deep_at_least, st
    c = count_on_device(sc, quiet, precision, tiles)
    got = (c["node_visits"], c["leaf_visits"], c["prim_tests"])
    print(f"visits of {tiles} x {len(quiet)} rays: kernel {got}, per-lane traversal x tiles {tuple(tiles * st[k] for k in ('nodes', 'leaves', 'prims'))}")
    assert got == (tiles * st["nodes"], tiles * st["leaves"], tiles * st["prims"])
    return st


@pytest.mark.parametrize("precision", [F32, F64])
def test_spilled_stack_counting_kernel_gives_the_same_hits(precision, monkeypatch):
    """The counting instance of the kernel (count_mode = 1) writes the hit table of the plain one, and on the quiet
    random rays (about 3400 of the 5000, 700 of them beyond the LDS levels; tiled to 400 k) visits exactly the nodes,
    leaves and primitives hostsim's traverse() visits: an entry lost, repeated or read from another ray's column
    changes a count."""
    sd = E.scene("hairball")
    sc = make_scene(sd, precision, "default", monkeypatch)
    try:
        count_on_device(sc, E.needle_rays(precision), precision, TILES)  # hit tables only: these rays shrink their limit
        check_counts(sc, sd, precision, E.spill_rays(precision), deep_at_least=500)
    finally:
        sc.close()


# ------------------------------------------------------------------ 3. two levels on one stack
@pytest.mark.parametrize("precision", [F32, F64])
def test_two_levels_on_one_stack(precision, monkeypatch):
    """8 overlapping placements of the hairball: the kernel keeps the top level's entries, the return marker and the
    prototype's entries on ONE stack; hostsim nests a second stack.  The top-level tree is small here — the marker stays
    within the LDS levels (level <= 6) and only the prototype's entries above it spill;
    test_return_marker_in_the_spill_area covers the other case.  The results are specified to be equal — and equal for
    the host-built and the device-built trees."""
    monkeypatch.setenv("TAKE_HIP_NODES", "")
    sd = E.hairball_two_level()
    spill = E.spill_rays(precision)
    more = np.concatenate([r for _, r in E.axis_parallel(n=60)] + [E.per_ray_tmin(n=500)])
    more = E.working(more, precision)
    st = hostsim_trace_stats(sd, precision, spill)
    assert st["max_stack"] >= E.LDS_LEVELS + 1 and 1 <= st["marker_level"] <= E.LDS_LEVELS, st
    tables = {}
    for builder in (HOST, DEV):
        sc = capi.Scene(sd, precision=precision, builder=builder)
        try:
            assert sc.build_info() == built_by(precision, builder), sc.build_info()
            got, occ = tiled(sc, spill, precision)
            got2, occ2 = trace(sc, more, precision)
        finally:
            sc.close()
        tables[builder] = np.concatenate([got, got2])
        assert np.array_equal(np.concatenate([occ, occ2]), tables[builder][:, 0] >= 0)
    same_table(tables[DEV], tables[HOST], "device-built against host-built")
    assert (tables[HOST][:len(spill), 0] >= sd.n_shapes).sum() >= 50  # hits inside placements
    want = hostsim_trace(sd, precision, np.concatenate([spill, more])).astype(np.float64)
    same_table(tables[HOST], want, "two-level hairball against hostsim")


@pytest.mark.parametrize("precision", [F32, F64])
def test_return_marker_in_the_spill_area(precision, monkeypatch):
    """hairball_deep_marker: 256 small placements among the 1024 needles of the top level.  hostsim_trace_stats shows
    placements entered with more than 15 top-level entries live, so the return marker and every entry of the prototype
    above it are in global memory.  Hit tables (closest, any; all tiles) equal hostsim's; the visit counts of the quiet
    rays equal its counts, which holds only if every marker brings its ray back to the right top-level entry."""
    monkeypatch.setenv("TAKE_HIP_NODES", "")
    sd = E.hairball_deep_marker()
    rays = np.concatenate([E.spill_rays(precision)[:1000], E.needle_rays(precision)[:1000]])
    st, want = hostsim_trace_stats(sd, precision, rays, hits=True)
    want = want.astype(np.float64)
    assert st["marker_level"] >= E.LDS_LEVELS + 1 and st["max_stack"] > st["marker_level"], st  # (marker_level = its level + 1)
    sc = capi.Scene(sd, precision=precision, builder=HOST)
    try:
        assert sc.build_info() == built_by(precision, HOST), sc.build_info()
        got, occ = tiled(sc, np.tile(rays, (3, 1)), precision)
        got, occ = got[:len(rays)], occ[:len(rays)]
        quiet_st = check_counts(sc, sd, precision, rays, deep_at_least=200)
        assert quiet_st["marker_level"] >= E.LDS_LEVELS + 1, quiet_st
    finally:
        sc.close()
    same_table(got, want, "deep-marker scene against hostsim")
    assert np.array_equal(occ, want[:, 0] >= 0)
    assert (want[:, 0] >= sd.n_shapes).sum() >= 50 and (want[:, 0] >= 0).sum() >= 800  # hits inside placements, and outside


# ------------------------------------------------------------------ 4. rendering
def test_render_over_the_spilled_stack():
    """the render loop's instance of the kernel (PathIo: uniform tmin, rays from the path state) over the spill path:
    the image does not depend on the batch size (other rays share a block) nor on the builder"""
    sd = E.hairball_lit()
    images = []
    for builder in (HOST, DEV):
        sc = capi.Scene(sd, precision=F32, builder=builder)
        try:
            assert sc.build_info() == built_by(F32, builder)
            images.append(sc.render(spp=4, max_depth=6, seed=3, samples_per_batch=4))
            assert np.array_equal(images[-1], sc.render(spp=4, max_depth=6, seed=3, samples_per_batch=1))
        finally:
            sc.close()
    assert np.array_equal(images[0], images[1])
    assert np.isfinite(images[0]).all() and images[0].mean() > 0


def test_render_with_the_camera_on_an_axis():
    """the camera exactly on the z axis, an odd-sized image: the rays through the image centre are the axis-parallel
    ones, straight onto axis-aligned walls — against the oracle's render, at the bar of test_render_f64_matches_oracle"""
    sd = golden_scene("cbox")
    sd.width = sd.height = 33
    sd.lookfrom, sd.lookat, sd.up = (0.0, 0.0, 3.9), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    osc = oracle.OracleScene(sd, precision=1)
    want = osc.render(4, 5, rng_mode=oracle.RNG_COUNTER, seed=11)
    osc.close()
    sc = capi.Scene(sd, precision=F64)
    try:
        got = sc.render(spp=4, max_depth=5, seed=11)
    finally:
        sc.close()
    assert rmse(got, want) < 1e-9, rmse(got, want)

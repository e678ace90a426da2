"""The traversal header on the rays the random generators never draw (tests/trace_edge_rays.py), executed on the host
(tests/hostsim: tk_traverse.h and the host tree builder, serially) against the exhaustive search of the oracle — no GPU.

Bars (trace_edge_rays.check_against_brute), per batch of a family: hit / miss and t bit for bit on every ray; u, v bit
for bit where the shape id is the same; where it differs the distance is an exact tie and the product holds the
lexicographically larger (u, v) (the rule test_exact_ties_vs_reference_visiting_order pins; the exhaustive search keeps
the lowest id), on at most 10 % of the batch; any hit == closest hit's boolean.

The hairball's preconditions live here too: its rays reach a stack deeper than the trace kernel's LDS levels on the tree
whose size tests/test_gpu_trace_edges.py compares the device scene's with."""
import numpy as np
import pytest

import oracle
import trace_edge_rays as E
from helpers import hostsim_trace, hostsim_trace_stats


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", E.SCENES)
def test_edge_rays_equal_exhaustive_search(name, precision):
    sd = E.scene(name)
    labels = []
    for label, rays, want in E.cases(name, precision):
        got = hostsim_trace(sd, precision, rays).astype(np.float64)
        E.check_against_brute(got, want, f"{name} {label}")
        occ = hostsim_trace(sd, precision, rays, any_hit=True)[:, 0] >= 0
        assert np.array_equal(occ, want[:, 0] >= 0), f"{name} {label}: any hit"
        labels.append(label)
    # every family ran: 12 axis-parallel batches, the two component families, far origins, scales, per-ray tmin, 5 boundaries
    n_far, n_scale = (len(E.FAR_F32), len(E.UNNORM_F32)) if precision == 0 else (len(E.FAR_F64), len(E.UNNORM_F64))
    assert len(labels) == 12 + 2 + n_far + n_scale + 1 + 5


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("fmt", ["wide", "q8"])
@pytest.mark.parametrize("name", ["cbox", "hairball"])
def test_edge_rays_through_the_other_node_formats(name, fmt, precision, monkeypatch):
    """full-width nodes (box_test) and the 8-wide tree.  The full-width slab test lost axis-parallel rays whose origin
    lies exactly on a plane of a box (76 to 85 of 666 per batch on cbox: rays along the edge of a wall): 0 x 1e30 = 0
    put the far plane at the origin."""
    monkeypatch.setenv("TAKE_HIP_NODES", fmt)
    sd = E.scene(name)
    for label, rays, want in E.cases(name, precision):
        E.check_against_brute(hostsim_trace(sd, precision, rays).astype(np.float64), want, f"{name} {fmt} {label}")
        occ = hostsim_trace(sd, precision, rays, any_hit=True)[:, 0] >= 0
        assert np.array_equal(occ, want[:, 0] >= 0), f"{name} {fmt} {label}: any hit"


def test_generators_draw_what_they_promise():
    """signed zeros, components at / below safe_inv's clamp (a float32 denormal and a zero among them), origins on the
    lattice, a tmin per ray, lengths far from 1 — and the same rays from the same seed"""
    batches = E.axis_parallel()
    assert len(batches) == 12 and len({label for label, _ in batches}) == 12
    for label, r in batches:
        d = r[:, 3:6]
        axis = "xyz".index(label[4])
        others = [a for a in range(3) if a != axis]
        assert (np.abs(d[:, axis]) == 1.0).all() and (d[:, others] == 0.0).all()
        assert (np.signbit(d[:, others]) == label.endswith("zero-")).all()
        assert (r[:, axis] == -3.0 * d[:, axis]).all() and (r[:, 6] == 0).all() and np.isinf(r[:, 7]).all()
        assert np.isin(r[: len(r) // 2, others], E.LATTICE).all() and not np.isin(r[len(r) // 2:, others], E.LATTICE).any()
    z = E.one_zero_component()[:, 3:6]
    assert ((z == 0).sum(axis=1) == 1).all() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    t64, t32 = E.working(E.tiny_component(), 1)[:, 3:6], E.working(E.tiny_component(), 0)[:, 3:6]
    for v in E.TINY:
        assert (t64 == v).any() and (t64 == -v).any()
    assert ((np.abs(t64) <= 1e-30).sum(axis=1) == 1).all()
    tiny32 = np.abs(t32[np.abs(t32) <= 1e-30])
    assert (tiny32 == 0).any() and ((tiny32 > 0) & (tiny32 < np.finfo(np.float32).tiny)).any()
    tm = E.per_ray_tmin()[:, 6]
    assert len(np.unique(tm)) == len(tm) and tm.min() >= 0 and tm.max() <= 1.5 and np.isfinite(E.per_ray_tmin()[:, 7]).any()
    for k in E.UNNORM_F64:
        assert np.allclose(np.linalg.norm(E.unnormalised(k)[:, 3:6], axis=1), k, rtol=1e-12)
    for s in E.FAR_F64:
        r = E.far_origin(s)
        assert np.allclose(np.linalg.norm(r[:, 0:3], axis=1), s, rtol=0.02) and (np.abs(r[:, 0:3] + s * r[:, 3:6]) <= 0.9 + 1e-9 * s).all()
    assert np.array_equal(E.far_origin(100.0), E.far_origin(100.0)) and np.array_equal(E.tiny_component(), E.tiny_component())
    a, b = E.hairball(), E.hairball()
    assert np.array_equal(a.meshes[0].positions, b.meshes[0].positions) and a.n_shapes == 1024


@pytest.mark.parametrize("precision", [0, 1])
def test_hairball_rays_go_deeper_than_the_lds_stack(precision):
    """the precondition of the GPU's spilled-stack tests: on the host SAH tree (472 nodes, depth 8) the rays of those
    tests need more stack entries than the kernel keeps in LDS — closest hit and any hit, one level and two — and the
    traversal still equals the exhaustive search on them"""
    rays = E.spill_rays(precision)
    sd = E.scene("hairball")
    for any_hit in (False, True):
        st = hostsim_trace_stats(sd, precision, rays, any_hit=any_hit)
        assert st["max_stack"] >= E.LDS_LEVELS + 1, st
        assert (st["n_nodes"], st["depth"]) == (E.HAIRBALL_NODES, E.HAIRBALL_DEPTH), st
        two = hostsim_trace_stats(E.hairball_two_level(), precision, rays, any_hit=any_hit)
        assert two["max_stack"] >= E.LDS_LEVELS + 1 and two["n_nodes"] > E.HAIRBALL_NODES and two["depth"] > E.HAIRBALL_DEPTH, two
    osc = oracle.OracleScene(sd, precision=precision)
    want = osc.isect_brute(rays)
    osc.close()
    n_hit, _ = E.check_against_brute(hostsim_trace(sd, precision, rays).astype(np.float64), want, "hairball random_rays")
    assert n_hit >= 20
    assert np.array_equal(hostsim_trace(sd, precision, rays, any_hit=True)[:, 0] >= 0, want[:, 0] >= 0)


def test_trace_stats_count_the_kernels_single_stack():
    """hostsim_trace_stats on a two-level scene: the prototype's entries are counted above the top level's and the
    return marker.  One placement beside the floor: the top level holds at most 2 entries below the marker, and the
    figure is the one-level hairball's + 1 at least (21 against 20 today: the marker alone)."""
    rays = E.spill_rays(1)[:500]
    one = hostsim_trace_stats(E.scene("hairball"), 1, rays)
    two = hostsim_trace_stats(E.hairball_two_level(placements=1), 1, rays)
    assert one["max_stack"] >= E.LDS_LEVELS + 1 and one["marker_level"] == 0
    assert one["max_stack"] + 1 <= two["max_stack"] <= one["max_stack"] + 3 and 1 <= two["marker_level"] <= 3, (one, two)
    # a cbox ray never needs more than 3 entries per level + 1
    st = hostsim_trace_stats(E.scene("cbox"), 1, rays)
    assert 1 <= st["max_stack"] <= 3 * st["depth"] + 1


@pytest.mark.parametrize("precision", [0, 1])
def test_a_lost_spill_area_would_show(precision):
    """Non-vacuity of the GPU's spilled-stack tests, on the host twin: with every stack entry at level >= 15 (the part
    the kernel keeps in global memory) lost, the needle rays change on tens of closest hits and any hits, and the visit
    counts of the quiet rays (no tmax, no hit) fall; losing levels nobody reaches changes nothing.  Under 1 % of a
    ray's primitive tests hang under such entries, which is why the random rays' 53 hits alone see nothing."""
    sd = E.scene("hairball")
    needles = E.needle_rays(precision)
    for any_hit, at_least in ((False, 25), (True, 50)):
        st, whole = hostsim_trace_stats(sd, precision, needles, any_hit=any_hit, hits=True)
        assert st["rays_deep"] >= 1000 and np.array_equal(whole, hostsim_trace(sd, precision, needles, any_hit=any_hit))
        _, lost = hostsim_trace_stats(sd, precision, needles, any_hit=any_hit, drop_from=E.LDS_LEVELS, hits=True)
        assert ((lost[:, 0] >= 0) != (whole[:, 0] >= 0)).sum() >= at_least
        _, kept = hostsim_trace_stats(sd, precision, needles, any_hit=any_hit, drop_from=st["max_stack"], hits=True)
        assert np.array_equal(kept, whole)
    rays = E.spill_rays(precision)
    quiet = rays[(hostsim_trace(sd, precision, rays)[:, 0] < 0) & np.isinf(rays[:, 7])]
    whole, lost = hostsim_trace_stats(sd, precision, quiet), hostsim_trace_stats(sd, precision, quiet, drop_from=E.LDS_LEVELS)
    assert len(quiet) >= 3000 and whole["rays_deep"] >= 500
    assert whole["nodes"] - lost["nodes"] >= whole["rays_deep"] and whole["prims"] - lost["prims"] >= whole["rays_deep"]


@pytest.mark.parametrize("precision", [0, 1])
def test_deep_marker_scene_puts_the_return_marker_beyond_lds(precision):
    """hairball_deep_marker: some placement is entered with more than 15 top-level entries live (marker_level is the
    marker's level + 1), and losing the levels from the marker's on changes hits inside placements"""
    sd = E.hairball_deep_marker()
    rays = np.concatenate([E.spill_rays(precision)[:1000], E.needle_rays(precision)[:1000]])
    st, whole = hostsim_trace_stats(sd, precision, rays, hits=True)
    assert st["marker_level"] >= E.LDS_LEVELS + 1 and st["max_stack"] > st["marker_level"], st
    assert np.array_equal(whole, hostsim_trace(sd, precision, rays))
    assert (whole[:, 0] >= sd.n_shapes).sum() >= 50
    _, lost = hostsim_trace_stats(sd, precision, rays, drop_from=E.LDS_LEVELS, hits=True)
    assert not np.array_equal(lost, whole)

"""Mixed precision (TAKE_PRECISION_MIXED): the first `exact_bounces` rounds of every path in the reference's arithmetic
(double, on the f64 scene), the surviving paths' records converted to float and finished on the f32 scene.

Pinned, per sample, to the oracle's restatement of exactly that split (oracle/take_oracle.hpp path_tracing_mixed, which
the device code re-executed on the host equals bit for bit: tests/test_mixed_cpu.py), at matched counter seeds:
  * on a scene whose paths need no transcendental function (tests/helpers.py mirror_box_scene) the GPU image IS the
    oracle's, bit for bit, at every handover tried — and is not the oracle's at the neighbouring handovers;
  * on the golden scenes and an env-map soup (ocml's libm against the host's) within bars measured on the MI355X, with
    a statistic that tells the right handover from its neighbours; and at the bench's workload shape;
  * with exact_bounces >= the number of rounds the render IS the f64 render: bit-identical images;
  * the error against the f64 image falls with every exact bounce, and with the default three it is well inside the
    f32 path's;
  * the usual invariances hold (determinism, batch size, strip sharding, progressive accumulation, scene groups,
    counting mode)."""
import numpy as np
import pytest
import torch

import oracle
from helpers import GOLDEN_SCENES, golden_scene, mirror_box_scene, rmse
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.dist import strip_rows

pytestmark = pytest.mark.gpu


def _render(sd, precision, spp, depth, seed, exact=0, **kw):
    sc = capi.Scene(sd, precision=precision)
    sc.exact_bounces = exact
    try:
        return sc.render(spp=spp, max_depth=depth, seed=seed, **kw)
    finally:
        sc.close()


@pytest.mark.parametrize("name", ["cbox", "mats", "meshlight"])
def test_all_rounds_exact_is_the_f64_render(name):
    sd = golden_scene(name)
    want = _render(sd, D.TAKE_PRECISION_F64, 4, 6, 3)
    got = _render(sd, D.TAKE_PRECISION_MIXED, 4, 6, 3, exact=8)  # max_depth 6 -> 8 rounds
    assert got.dtype == np.float64 and np.array_equal(got, want)


def test_error_falls_with_the_exact_bounces_on_a_soup():
    sd = scenes.soup_scene(100_000, 640, 360, spp=16, envmap=(512, 256))
    ref = _render(sd, D.TAKE_PRECISION_F64, 16, 50, 1)
    e32 = rmse(_render(sd, D.TAKE_PRECISION_F32, 16, 50, 1), ref)
    errs = [rmse(_render(sd, D.TAKE_PRECISION_MIXED, 16, 50, 1, exact=k), ref) for k in (1, 3, 6)]
    print("f32", e32, "mixed", errs)
    assert errs[0] < e32 and errs[1] < 0.6 * e32 and errs[2] < 0.35 * e32, (e32, errs)
    assert errs[0] > errs[1] > errs[2] > 0
    # the default is three exact bounces
    assert np.array_equal(_render(sd, D.TAKE_PRECISION_MIXED, 16, 50, 1), _render(sd, D.TAKE_PRECISION_MIXED, 16, 50, 1, exact=3))


def test_mixed_invariances():
    sd = golden_scene("mats")  # 64 x 48, every reference material tag: the material sort runs in both halves
    sc = capi.Scene(sd, precision=D.TAKE_PRECISION_MIXED)
    try:
        a = sc.render(spp=6, max_depth=10, seed=4)
        assert np.isfinite(a).all() and a.mean() > 0.01
        assert np.array_equal(a, sc.render(spp=6, max_depth=10, seed=4))
        assert np.array_equal(a, sc.render(spp=6, max_depth=10, seed=4, samples_per_batch=1))
        img = np.zeros_like(a)
        for r in range(3):
            img[strip_rows(sd.height, r, 3)] = sc.render(spp=6, max_depth=10, seed=4, strip_first=r, strip_stride=3)
        assert np.array_equal(img, a)
        out = torch.zeros((sd.height, sd.width, 3), dtype=torch.float64, device="cuda")
        sc.render_accumulate(out.data_ptr(), 4, 10, seed=4, restart=True)
        assert sc.render_accumulate(out.data_ptr(), 2, 10, seed=4) == 6
        assert np.array_equal(out.cpu().numpy(), a)
        # integrators 1..3 are refused (the mixed path is the reference's path_tracing)
        with pytest.raises(capi.TakeError):
            sc.render(spp=1, max_depth=3, seed=1, integrator=2)
        # the trace hooks of a mixed scene are the f64 scene's
        rays = np.zeros((4, 8))
        rays[:, 2], rays[:, 5], rays[:, 7] = 3.0, -1.0, np.inf
        assert sc.trace_closest(np.concatenate([rays[:, 0:3], rays[:, 6:7], rays[:, 3:6], rays[:, 7:8]], axis=1))["t"].dtype == np.float64
    finally:
        sc.close()
    f64 = _render(sd, D.TAKE_PRECISION_F64, 6, 10, 4)
    assert rmse(a, f64) < 5e-3  # (bounded radiance, 6 spp: f32 alone is at 4.5e-3 on this scene, tests/test_gpu_precision.py)


def test_mixed_scene_group_equals_single_scene():
    sd = golden_scene("cbox")
    want = _render(sd, D.TAKE_PRECISION_MIXED, 4, 8, 2)
    g = capi.SceneGroup(sd, [0, 0, 0], precision=D.TAKE_PRECISION_MIXED)
    try:
        got = g.render(spp=4, max_depth=8, seed=2)
    finally:
        g.close()
    assert np.array_equal(got, want)


def test_mixed_on_an_instanced_scene():
    """two-level scenes (TakeInstance): the conversion hands over rays, not hits, so the f32 rounds traverse the f32
    twin of the same two-level tree.  All rounds exact = the f64 render; the default = closer to it than the f32 path."""
    sd = scenes.instanced_scene(60, 400, 160, 96, spp=8)
    ref = _render(sd, D.TAKE_PRECISION_F64, 8, 12, 5)
    assert np.array_equal(_render(sd, D.TAKE_PRECISION_MIXED, 8, 12, 5, exact=14), ref)
    e32 = rmse(_render(sd, D.TAKE_PRECISION_F32, 8, 12, 5), ref)
    emx = rmse(_render(sd, D.TAKE_PRECISION_MIXED, 8, 12, 5), ref)
    print("instanced: f32", e32, "mixed", emx)
    assert 0 < emx < 0.7 * e32


# ------------------------------------------------------------------ against the oracle's mixed restatement
def _oracle(sd, precision, spp, depth, seed, exact=0):
    osc = oracle.OracleScene(sd, precision=precision)
    try:
        return osc.render(spp, depth, rng_mode=oracle.RNG_COUNTER, seed=seed, threads=16, exact_bounces=exact)
    finally:
        osc.close()


def _lower_neighbour(sd, spp, depth, seed, E):
    """the oracle one handover earlier; below E = 1 is the all-float render (E = 0 means the default, 3)"""
    return _oracle(sd, 0, spp, depth, seed) if E == 1 else _oracle(sd, oracle.PRECISION_MIXED, spp, depth, seed, E - 1)


def test_transcendental_free_scene_is_bit_identical_to_the_oracle():
    """Measured on the MI355X: the f64 and f32 paths and the mixed path at E = 1, 2, 3, 7 all bit-identical to the
    oracle on this scene (the neighbouring handovers differ from it in 1-50 % of the pixels)"""
    sd = mirror_box_scene()
    for precision in (D.TAKE_PRECISION_F64, D.TAKE_PRECISION_F32):
        got = _render(sd, precision, 2, 50, 1).astype(np.float64)
        assert np.array_equal(got, _oracle(sd, precision, 2, 50, 1)), precision
    for E in (1, 2, 3, 7):
        got = _render(sd, D.TAKE_PRECISION_MIXED, 2, 50, 1, exact=E)
        assert np.array_equal(got, _oracle(sd, oracle.PRECISION_MIXED, 2, 50, 1, E)), E
        assert not np.array_equal(got, _oracle(sd, oracle.PRECISION_MIXED, 2, 50, 1, E + 1)), E
        assert not np.array_equal(got, _lower_neighbour(sd, 2, 50, 1, E)), E


def test_mixed_edges_are_bit_identical_to_the_oracle():
    """the handover just before the final (trace + C2 only) round, max_depth -1 and 0, a ragged image size"""
    sd = mirror_box_scene()
    for depth, E in ((5, 6), (50, 51), (-1, 1), (0, 1), (0, 2)):
        got = _render(sd, D.TAKE_PRECISION_MIXED, 2, depth, 3, exact=E)
        assert np.array_equal(got, _oracle(sd, oracle.PRECISION_MIXED, 2, depth, 3, E)), (depth, E)
    ragged = mirror_box_scene(37, 21)
    for E in (1, 3):
        got = _render(ragged, D.TAKE_PRECISION_MIXED, 2, 50, 2, exact=E)
        assert got.shape == (21, 37, 3)
        assert np.array_equal(got, _oracle(ragged, oracle.PRECISION_MIXED, 2, 50, 2, E)), E


def _stats(a, b):
    d = np.abs(np.asarray(a, np.float64) - b)
    return dict(rmse=float(np.sqrt(np.mean(d ** 2))), median=float(np.median(d)),
                outside=float(np.mean(d.max(axis=2) > 1e-5)),       # share of pixels off by more than 1e-5
                differ=float(np.mean((a != b).any(axis=2))))         # share of pixels not bit-identical


def _env_soup():
    return scenes.soup_scene(1000, 64, 64, spp=2, envmap=(128, 64))


# Worst value over depth {5, 50} x E {1, 3} x seeds {1, 2, 3} measured on the MI355X (GPU mixed at 2 spp against
# oracle mixed; `differ` at 1 spp); each bar is twice that.  The median |diff| was 0 in every case.
MIXED_BARS = {  # scene: (rmse, outside, differ at 1 spp) bars        measured worst
    "cbox": (2.2e-6, 2.0e-3, 0.34),         # 1.06e-6, 9.8e-4, 0.168
    "mats": (3.8e-7, 6.6e-4, 0.46),         # 1.88e-7, 3.3e-4, 0.229
    "soup1k": (6.7e-6, 4.9e-4, 0.28),       # 3.34e-6, 2.4e-4, 0.139
    "spherelight": (1.5e-3, 7.9e-3, 0.40),  # 7.51e-4, 3.9e-3, 0.196 (sphere uv: acos / atan2)
    "meshlight": (7.0e-6, 4.9e-4, 0.39),    # 3.47e-6, 2.4e-4, 0.192
    "envsoup": (3.9e-6, 4.9e-4, 0.29),      # 1.93e-6, 2.4e-4, 0.145
}
# The statistic that separates the right handover from its neighbours: at 1 spp the share of pixels that are not
# bit-identical to the oracle at E +- 1 was at least 3.54x (worst case, spherelight E = 3) the share at E itself.
# (RMSE does not separate them: it is dominated by the libm-driven flips, which every handover has.)
NEIGHBOUR_RATIO = 1.75


@pytest.mark.parametrize("name", list(MIXED_BARS))
def test_mixed_matches_the_oracle_mixed_within_measured_bars(name):
    sd = _env_soup() if name == "envsoup" else golden_scene(name)
    b_rmse, b_out, b_differ = MIXED_BARS[name]
    for depth in (5, 50):
        for E in (1, 3):
            for seed in (1, 2, 3):
                s = _stats(_render(sd, D.TAKE_PRECISION_MIXED, 2, depth, seed, exact=E),
                           _oracle(sd, oracle.PRECISION_MIXED, 2, depth, seed, E))
                assert s["rmse"] <= b_rmse and s["outside"] <= b_out and s["median"] == 0.0, (depth, E, seed, s)
                g1 = _render(sd, D.TAKE_PRECISION_MIXED, 1, depth, seed, exact=E)
                own = _stats(g1, _oracle(sd, oracle.PRECISION_MIXED, 1, depth, seed, E))["differ"]
                up = _stats(g1, _oracle(sd, oracle.PRECISION_MIXED, 1, depth, seed, E + 1))["differ"]
                down = _stats(g1, _lower_neighbour(sd, 1, depth, seed, E))["differ"]
                assert own <= b_differ, (depth, E, seed, own)
                assert min(up, down) >= NEIGHBOUR_RATIO * own, (depth, E, seed, own, up, down)


def test_bench_workload_shape_matches_the_oracle_mixed():
    """bench.py's scene and camera (1M-triangle soup, 2048 x 1024 env map) at 128 x 72, 2 spp, depth 50, the default
    exact bounces.  Measured: RMSE 1.04e-4, median |diff| 0, 0.34 % of the pixels off by more than 1e-5 against the
    oracle's mixed image — and RMSE 2.3e-3 against the oracle's f64 image (what the mixed path is not)"""
    sd = scenes.soup_scene(1_000_000, 128, 72, spp=2, envmap=(2048, 1024))
    got = _render(sd, D.TAKE_PRECISION_MIXED, 2, 50, 1)
    s = _stats(got, _oracle(sd, oracle.PRECISION_MIXED, 2, 50, 1))
    assert s["rmse"] <= 2.1e-4 and s["median"] == 0.0 and s["outside"] <= 6.8e-3, s
    assert s["rmse"] < 0.1 * rmse(got, _oracle(sd, 1, 2, 50, 1)), s


def test_accumulate_refuses_a_change_of_exact_bounces():
    """take_hip_render_accumulate: on a mixed scene the effective exact_bounces (<= 0: the default, 3) is part of what
    a sequence must keep; f32 / f64 scenes ignore the field"""
    sd = golden_scene("cbox")
    sc = capi.Scene(sd, precision=D.TAKE_PRECISION_MIXED)
    try:
        out = torch.zeros((sd.height, sd.width, 3), dtype=torch.float64, device="cuda")
        sc.exact_bounces = 3
        assert sc.render_accumulate(out.data_ptr(), 2, 6, seed=4, restart=True) == 2
        sc.exact_bounces = 5
        with pytest.raises(capi.TakeError) as e:
            sc.render_accumulate(out.data_ptr(), 2, 6, seed=4)
        assert e.value.code == D.TAKE_E_INVALID
        sc.exact_bounces = 0  # the default: the same three rounds
        assert sc.render_accumulate(out.data_ptr(), 2, 6, seed=4) == 4
        three = out.cpu().numpy().copy()
        sc.exact_bounces = 5
        assert sc.render_accumulate(out.data_ptr(), 4, 6, seed=4, restart=True) == 4
        five = out.cpu().numpy().copy()
    finally:
        sc.close()
    assert np.array_equal(three, _render(sd, D.TAKE_PRECISION_MIXED, 4, 6, 4, exact=3))
    assert np.array_equal(five, _render(sd, D.TAKE_PRECISION_MIXED, 4, 6, 4, exact=5))
    assert not np.array_equal(three, five)
    for precision, dtype in ((D.TAKE_PRECISION_F32, torch.float32), (D.TAKE_PRECISION_F64, torch.float64)):
        sc = capi.Scene(sd, precision=precision)
        try:
            out = torch.zeros((sd.height, sd.width, 3), dtype=dtype, device="cuda")
            sc.exact_bounces = 3
            sc.render_accumulate(out.data_ptr(), 2, 6, seed=4, restart=True)
            sc.exact_bounces = 5
            assert sc.render_accumulate(out.data_ptr(), 2, 6, seed=4) == 4
            assert np.array_equal(out.cpu().numpy(), sc.render(spp=4, max_depth=6, seed=4))
        finally:
            sc.close()


@pytest.mark.parametrize("name", ["mats", "soup"])
def test_counting_mode_does_not_change_the_mixed_image(name):
    """the instrumented (counting) kernels probe the previous occluder of a slot (S_OCC); the conversion writes -1
    there, so the f32 rounds start without one — and the image is the uninstrumented one, bit for bit"""
    sd = golden_scene("mats") if name == "mats" else scenes.soup_scene(20_000, 64, 48, spp=2)
    for E in (1, 3):
        want = _render(sd, D.TAKE_PRECISION_MIXED, 2, 20, 1, exact=E)
        sc = capi.Scene(sd, precision=D.TAKE_PRECISION_MIXED)
        sc.exact_bounces = E
        try:
            sc.set_instrumentation(counting=True)
            got = sc.render(spp=2, max_depth=20, seed=1)
        finally:
            sc.close()
        assert np.array_equal(got, want), E

"""The shade kernels' cooperative record moves (tk_record_io.h: a wave loads and stores the path records of its 64 lanes
as whole lines, transposed through a wave-private LDS stage) against the row-per-lane form they replace
(TAKE_HIP_SHADE_COOP=0, read per render call): only who moves which 16 bytes differs, so every image must be the same
bit for bit.  Each test renders both ways from ONE scene handle.

The shapes are the smallest at which the cooperative move can go wrong: queues that end inside a wave (lanes that own
no record still move their neighbours' pieces, and the last record of the allocation belongs to such a wave), queues of
exactly one wave and one block, one more and one fewer; sparse later rounds; sorted queues whose per-tag segments start
at offsets that are no multiple of 8 or 64; the handover round of a mixed-precision render, where only the paths that
go on write an f32 record; the other integrators' instances; two-level scenes; env-map lights; an adaptive render."""
import numpy as np
import pytest

from helpers import golden_scene
from take_amd import capi, scenes
from take_amd import cdefs as D

pytestmark = pytest.mark.gpu

PRECISIONS = {"f32": D.TAKE_PRECISION_F32, "f64": D.TAKE_PRECISION_F64, "mixed": D.TAKE_PRECISION_MIXED}
# width x height at 1 spp = the paths of the first round: 1, 7, 8, 9, 63, 64, 65, 255, 256, 257
SIZES = [(1, 1), (7, 1), (8, 1), (3, 3), (9, 7), (8, 8), (13, 5), (51, 5), (16, 16), (257, 1)]


def _both_ways(monkeypatch, call):
    """call() with the row-per-lane records and with the cooperative ones -> the (identical) result"""
    monkeypatch.setenv("TAKE_HIP_SHADE_COOP", "0")
    row = call()
    monkeypatch.setenv("TAKE_HIP_SHADE_COOP", "1")
    coop = call()
    monkeypatch.delenv("TAKE_HIP_SHADE_COOP")
    default = call()
    assert np.isfinite(row).all()
    assert np.array_equal(coop, row), f"{np.count_nonzero(coop != row)} of {row.size} values differ"
    assert np.array_equal(default, coop)
    return row


def _cbox(width=None, height=None):
    sd = golden_scene("cbox")
    if width is not None:
        sd.width, sd.height = width, height
    return sd


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_first_round_path_counts(monkeypatch, size, precision):
    sc = capi.Scene(_cbox(*size), precision=PRECISIONS[precision])
    try:
        img = _both_ways(monkeypatch, lambda: sc.render(spp=1, max_depth=6, seed=5))
        assert img.shape == (size[1], size[0], 3)
    finally:
        sc.close()


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_sparse_later_rounds(monkeypatch, precision):
    sc = capi.Scene(_cbox(), precision=PRECISIONS[precision])
    try:
        img = _both_ways(monkeypatch, lambda: sc.render(spp=4, max_depth=10, seed=2))
        assert img.mean() > 0.01
        one = _both_ways(monkeypatch, lambda: sc.render(spp=4, max_depth=10, seed=2, samples_per_batch=1))
        assert np.array_equal(one, img)
    finally:
        sc.close()


@pytest.mark.parametrize("exact", [1, 3])
def test_sorted_segments_and_partial_handover(monkeypatch, exact):
    sc = capi.Scene(golden_scene("mats"), precision=D.TAKE_PRECISION_MIXED)  # 64 x 48, every material tag
    sc.exact_bounces = exact
    try:
        img = _both_ways(monkeypatch, lambda: sc.render(spp=4, max_depth=10, seed=4))
        assert img.mean() > 0.01
    finally:
        sc.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_sorted_segments(monkeypatch, precision):
    sc = capi.Scene(golden_scene("mats"), precision=PRECISIONS[precision])
    try:
        _both_ways(monkeypatch, lambda: sc.render(spp=4, max_depth=10, seed=4))
    finally:
        sc.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("integrator", [1, 2, 3])
def test_other_integrators(monkeypatch, integrator, precision):
    sc = capi.Scene(_cbox(), precision=PRECISIONS[precision])
    try:
        _both_ways(monkeypatch, lambda: sc.render(spp=2, max_depth=6, seed=7, integrator=integrator))
    finally:
        sc.close()


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_two_level_scene(monkeypatch, precision):
    sd = scenes.instanced_scene(5, 300, 45, 27, spp=2)
    sc = capi.Scene(sd, precision=PRECISIONS[precision])
    try:
        img = _both_ways(monkeypatch, lambda: sc.render(spp=2, max_depth=8, seed=9))
        assert img.mean() > 0.0
    finally:
        sc.close()


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_env_map_soup(monkeypatch, precision):
    sd = scenes.soup_scene(20_000, 64, 36, spp=2, envmap=(64, 32))
    sc = capi.Scene(sd, precision=PRECISIONS[precision])
    try:
        img = _both_ways(monkeypatch, lambda: sc.render(spp=2, max_depth=12, seed=11))
        assert img.mean() > 0.0
    finally:
        sc.close()


def test_adaptive_render(monkeypatch):
    sc = capi.Scene(_cbox(), precision=D.TAKE_PRECISION_F32)
    try:
        # its listed passes (pixels still above the threshold) run the same shade kernels on queues of any length
        _both_ways(monkeypatch, lambda: sc.render_adaptive(spp=32, max_depth=6, seed=3, min_spp=8, step_spp=8, threshold=0.05))
    finally:
        sc.close()

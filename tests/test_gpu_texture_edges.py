"""The texture lookup on the device (take_amd/csrc/tk_shade.h: modulo1, eval_texture) at wrap edges and odd image shapes,
against the exact rational reference of tests/texture_ref.py (rows and images: tests/texture_edge_cases.py, scenes:
tests/texture_edge_scenes.py; the same rows on the host build of the header: tests/test_texture_cpu.py).

a. take_hip_debug_table "texture" (the fixed 5x4 image) on every exact and generic row, f32 and f64.
b. take_hip_debug_table "material": a Diffuse and a Mirror row per exact texture row, columns 10..12 (eval_bsdf at the given
   direction) = the exact texel * max(n . dir_out, 0) / pi, and F0 + (1 - F0) (1 - n . dir_out)^5.
c. The albedo plane of render_features on the quad scene — a pool of six images, eight materials, 192 quads whose uv is an
   edge value — every interior pixel of every quad, f32 and f64.
d. render() of that scene against the oracle (f64) and the oracle's float twin (f32).
e. The albedo plane of a textured sphere seen from above its pole, against the oracle's hits + the exact reference.

Bars.  Rows: f64 rtol 1e-11, atol 1e-13 (tests/test_gpu_golden_tables.py), f32 rtol 5e-4, atol 2e-5 (test_small_tables);
no exact row is left out, a generic row only where its cell is not the same over the rounding of its coordinate.  Planes:
f64 1e-9, f32 1e-3 (tests/test_gpu_features.py); in (c) on every interior pixel, in (e) on that file's shares (99.5 % and
99 %: a sample within rounding of the seam radius or of a texel boundary under the pole may sit in another cell than the
oracle's; on the CPU the oracle's float twin is within 1e-3 of the exact f64 plane on 100 % of this scene's pixels:
tests/test_texture_cpu.py::test_the_sphere_scene_leaves_room_for_f32).  Renders: RMSE < 1e-9 (f64), < 1e-3 against the
float twin (f32) (tests/test_gpu_parity.py)."""
import numpy as np
import pytest

import oracle
import texture_edge_cases as K
import texture_edge_scenes as S
import texture_ref as T
from helpers import rmse
from take_amd import capi
from take_amd import cdefs as D
from test_gpu_features import camera_rays, share_within
from test_texture_cpu import close, rows_of, want_of

pytestmark = pytest.mark.gpu
PRECISIONS = [D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64]  # (= texture_ref's F32, F64)
IDS = ["f32", "f64"]
PLANE_BAR = {T.F32: 1e-3, T.F64: 1e-9}


# ------------------------------------------------------------------ a. the texture table
@pytest.mark.parametrize("real", PRECISIONS, ids=IDS)
def test_debug_table_texture(real):
    rows, n_exact = rows_of(real)
    want, stable = want_of(real, -1)
    got = capi.debug_table("texture", rows, np.zeros((len(rows), 8)), real)
    ok = close(got, want, real).all(axis=1)
    print(f"largest error on the exact rows {np.abs(got - want)[:n_exact].max():.3e}; generic rows left out {100 * (~stable[n_exact:]).mean():.2f} %")
    assert stable[:n_exact].all()
    assert ok[:n_exact].all(), (rows[:n_exact][~ok[:n_exact]][:5], got[:n_exact][~ok[:n_exact]][:5], want[:n_exact][~ok[:n_exact]][:5])
    bad = ~ok[n_exact:] & stable[n_exact:]
    assert not bad.any(), (rows[n_exact:][bad][:5], got[n_exact:][bad][:5], want[n_exact:][bad][:5])


# ------------------------------------------------------------------ b. the material table
@pytest.mark.parametrize("real", PRECISIONS, ids=IDS)
def test_debug_table_material(real):
    rows = K.exact_rows(real)
    texel = want_of(real, -1)[0][:len(rows)]
    dt = np.float32 if real == T.F32 else np.float64
    unit = lambda v: np.asarray(v, np.float64) / np.linalg.norm(v)
    normal = np.array([0.0, 0.0, 1.0])
    dir_in, dir_out = unit((0.3, 0.2, 0.9)).astype(dt).astype(np.float64), unit((-0.4, 0.1, 0.8)).astype(dt).astype(np.float64)
    cos = float(dir_out @ normal)
    for tag in (D.MAT_DIFFUSE, D.MAT_MIRROR):
        a = np.zeros((len(rows), 27))
        a[:, 0] = tag
        a[:, 6:9], a[:, 9:12] = normal, normal
        a[:, 12:14] = rows[:, 0:2]
        a[:, 14:17], a[:, 17:20] = dir_in, dir_out
        a[:, 20], a[:, 21], a[:, 22] = 0.5, 1.0, 1.0
        a[:, 23:27] = rows[:, 2:6]
        got = capi.debug_table("material", a, np.full((len(rows), 8), 0.37), real)[:, 10:13]
        want = texel * cos / np.pi if tag == D.MAT_DIFFUSE else texel + (1.0 - texel) * (1.0 - cos) ** 5
        ok = close(got, want, real)
        assert ok.all(), (tag, rows[~ok.all(axis=1)][:5], got[~ok.all(axis=1)][:5], want[~ok.all(axis=1)][:5])


# ------------------------------------------------------------------ c, d. the quad scene
@pytest.fixture(scope="module")
def quads():
    """the scene, its quads, the interior pixels of each from the oracle's hits: computed once, never written to"""
    sd, q = S.quad_scene()
    hit = S.oracle_hits(sd, camera_rays(sd, S.SPP, S.SEED, 1e-7))
    interior = S.interior_pixels(sd, hit, len(q))
    assert min(int(m.sum()) for m in interior) >= 16
    return sd, q, interior


@pytest.mark.parametrize("real", PRECISIONS, ids=IDS)
def test_albedo_of_every_quad(quads, real):
    sd, q, interior = quads
    sc = capi.Scene(sd, precision=real)
    try:
        got = sc.render_features(S.SPP, seed=S.SEED)["albedo"]
    finally:
        sc.close()
    worst, one_valued = 0.0, 0
    for k, quad in enumerate(q):
        cand = S.quad_candidates(sd.images, quad, real)
        one_valued += len(cand) == 1
        err = S.pixel_errors(got[interior[k]], cand)
        worst = max(worst, float(err.max()))
        assert (err <= PLANE_BAR[real]).all(), (k, quad, len(cand), float(err.max()), got[interior[k]][int(err.argmax())], cand)
    print(f"{len(q)} quads, {one_valued} with one candidate value; largest error {worst:.3e}")


def test_render_of_the_quad_scene_f64(quads):
    sd = quads[0]
    osc = oracle.OracleScene(sd, precision=1)
    want = osc.render(S.SPP, 5, rng_mode=oracle.RNG_COUNTER, seed=11)
    osc.close()
    sc = capi.Scene(sd, precision=D.TAKE_PRECISION_F64)
    try:
        got = sc.render(spp=S.SPP, max_depth=5, seed=11)
    finally:
        sc.close()
    assert want.max() > 0.3 and rmse(got, want) < 1e-9, rmse(got, want)


def test_render_of_the_quad_scene_f32(quads):
    sd = quads[0]
    osc = oracle.OracleScene(sd, precision=0)
    want = osc.render(S.SPP, 5, seed=11)
    osc.close()
    sc = capi.Scene(sd, precision=D.TAKE_PRECISION_F32)
    try:
        got = sc.render(spp=S.SPP, max_depth=5, seed=11)
    finally:
        sc.close()
    assert rmse(got, want) < 1e-3, rmse(got, want)


# ------------------------------------------------------------------ e. the textured sphere
@pytest.mark.parametrize("real", PRECISIONS, ids=IDS)
def test_albedo_of_a_sphere_seen_from_above_its_pole(real):
    sd = S.sphere_scene()
    want = S.albedo_plane(sd, S.oracle_hits(sd, camera_rays(sd, S.SPP, S.SEED, 1e-7)), T.F64)
    sc = capi.Scene(sd, precision=real)
    try:
        got = sc.render_features(S.SPP, seed=S.SEED)["albedo"]
    finally:
        sc.close()
    share = share_within(got, want, PLANE_BAR[real])
    print(f"albedo within {PLANE_BAR[real]} on {100 * share:.3f} % of the pixels")
    assert share >= (0.99 if real == T.F32 else 0.995), share

"""The texture lookup (take_amd/csrc/tk_shade.h: modulo1, eval_texture) without a GPU, held to the exact rational
reference of tests/texture_ref.py on the rows and image shapes of tests/texture_edge_cases.py.

1. The exact reference is accepted on the reference's own golden table (tests/golden/tables/texture_*, 512 rows of the
   compiled reference in double) at the f64 bar, and on values worked out by hand.
2. eval_texture<float|double>, built for the host by tests/texture_host, on all six image shapes — each alone and inside
   the pool of all six — on every exact and generic row.  f64: rtol 1e-11, atol 1e-13 (tests/test_gpu_golden_tables.py);
   f32: rtol 5e-4, atol 2e-5 (test_small_tables).  No exact row is left out; a generic row only where its cell is not the
   same over the rounding of its coordinate (texture_ref.is_stable), and those are at most 5 %.
3. oracle.table("texture") (double, the fixed 5x4 image) on the f64 rows.

4. The scenes of tests/test_gpu_texture_edges.py: every quad has its interior pixels, the oracle's own hits satisfy what
   that file asks of the device, the device headers run on the host render the quad scene bit for bit as the oracle does,
   and the sphere scene leaves the f32 share room.

Measured here: generic rows left out 0 of 640 in f32 and in f64, on every shape (no drawn coordinate lies within an ulp of
a cell boundary); largest f32 error on the exact rows 1.8e-7 (2x2 image), f64 4.4e-16."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle
import texture_edge_cases as K
import texture_ref as T
from helpers import HERE

TAB = os.path.join(HERE, "golden", "tables")
BARS = {T.F32: (5e-4, 2e-5), T.F64: (1e-11, 1e-13)}
IMAGES = K.images()
_LIB = None
_WANT = {}


def close(got, want, real):
    rtol, atol = BARS[real]
    return np.abs(got - want) <= atol + rtol * np.abs(want)


def rows_of(real):
    """(rows, n_exact): the exact rows first"""
    e, g = K.exact_rows(real), K.generic_rows(real)
    return np.concatenate([e, g]), len(e)


def want_of(real, k):
    """the exact reference on image k (-1: the table image) for every row of the precision: computed once, never written to"""
    if (real, k) not in _WANT:
        img = K.table_image() if k < 0 else IMAGES[k]
        rows, _ = rows_of(real)
        stable = np.array([T.is_stable(img.shape[:2], r, real) for r in rows])
        _WANT[real, k] = (T.lookup_rows(img, rows, real), stable)
    return _WANT[real, k]


def host():
    global _LIB
    if _LIB is None:
        d = os.path.join(HERE, "texture_host")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        L = C.CDLL(os.path.join(d, "libtexture_host.so"))
        L.texture_host_eval.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        _LIB = L
    return _LIB


def host_eval(images, k, rows, real):
    """eval_texture of the host build through image k of a pool made of `images`, laid out back to back"""
    dt = np.float32 if real == T.F32 else np.float64
    dims = np.array([(im.shape[1], im.shape[0]) for im in images], np.int32)
    pool = np.concatenate([np.asarray(im, np.float64).reshape(-1) for im in images]).astype(dt)
    rows = np.ascontiguousarray(rows, np.float64)
    out = np.zeros((len(rows), 3))
    assert host().texture_host_eval(real, len(images), dims.ctypes.data, k, pool.ctypes.data, rows.ctypes.data, len(rows), out.ctypes.data) == 0
    return out


# ------------------------------------------------------------------ 1. the reference is the reference's
def test_the_exact_reference_reproduces_the_reference_s_table():
    rows = np.fromfile(os.path.join(TAB, "texture_in.f64"), "<f8").reshape(-1, 6)
    want = np.fromfile(os.path.join(TAB, "texture_out.f64"), "<f8").reshape(-1, 3)
    assert rows.shape[0] == 512
    got = T.lookup_rows(K.table_image(), rows, T.F64)
    ok = close(got, want, T.F64)
    assert ok.all(), np.argwhere(~ok)[:5]


def test_values_worked_out_by_hand():
    img = IMAGES[5]  # 4 x 8
    assert img.shape == (4, 8, 3)
    assert np.array_equal(T.lookup(img, (0.25, 0.5, 1, 1, 0, 0), T.F64), img[2, 2])  # on a texel: its value
    assert np.allclose(T.lookup(img, (0.3125, 0.625, 1, 1, 0, 0), T.F64), (img[2, 2] + img[2, 3] + img[3, 2] + img[3, 3]) / 4, rtol=0, atol=1e-15)
    # just below the seam the filter, as written, extrapolates: (W q[W-1] - q[0]) / (W - 1) in the limit
    for a in (-2.0 ** -26, -2.0 ** -100):
        assert T.cell((4, 8), (a, a, 1, 1, 0, 0), T.F32) == (7, 3)
        got = T.lookup(img, (a, 0.5, 1, 1, 0, 0), T.F64)
        assert np.allclose(got, (8 * img[2, 7] - img[2, 0]) / 7, rtol=0, atol=1e-6)
    assert T.cell((4, 8), (0.0, -0.0, 1, 1, 0, 0), T.F32) == (0, 0) and T.cell((4, 8), (1.0, -1.0, 1, 1, 0, 0), T.F32) == (0, 0)
    assert np.array_equal(T.lookup(IMAGES[0], (-2.0 ** -26, 0.7, 1, 1, 0, 0), T.F64), IMAGES[0][0, 0])  # 1 x 1: its texel


def test_the_images_cannot_hide_a_wrong_texel():
    flat = np.concatenate([im.reshape(-1) for im in IMAGES])
    assert [im.shape[:2] for im in IMAGES] == K.SHAPES and flat.min() > 0 and flat.max() < 1
    assert len(np.unique(flat.astype(np.float32))) == flat.size == 207
    for im in IMAGES:  # not affine in (x, y): the least-squares plane leaves a residual
        h, w = im.shape[:2]
        if h * w < 4:
            continue
        yy, xx = np.mgrid[0:h, 0:w]
        A = np.stack([xx.ravel(), yy.ravel(), np.ones(h * w)], 1).astype(np.float64)
        for c in range(3):
            res = im[..., c].ravel() - A @ np.linalg.lstsq(A, im[..., c].ravel(), rcond=None)[0]
            assert np.abs(res).max() > 0.02, (im.shape, c)


@pytest.mark.parametrize("real", [T.F32, T.F64], ids=["f32", "f64"])
def test_the_rows_are_values_of_the_precision_and_the_exact_ones_exact(real):
    rows, n_exact = rows_of(real)
    dt = np.float32 if real == T.F32 else np.float64
    assert np.isfinite(rows).all() and np.array_equal(rows.astype(dt).astype(np.float64), rows)
    tiny = float(np.finfo(dt).tiny)
    window = 0
    for u, v, us, vs, uo, vo in rows[:n_exact].tolist():
        for x, s, o in ((u, us, uo), (v, vs, vo)):
            p, a = Fraction(s) * Fraction(x), T.coordinate(x, s, o, real)
            assert T.representable(p, real) and T.representable(a, real) and (a == 0 or abs(a) >= tiny)
            window += -Fraction(1, 2 ** (25 if real == T.F32 else 54)) <= a < 0
    assert window >= 20  # axes of rows inside the window where r + 1 rounds to 1
    assert len(rows) - n_exact == 640 and np.abs(rows[n_exact + 512:, 0:2]).max() > 2.0 ** 16


# ------------------------------------------------------------------ 2. the host build of eval_texture
@pytest.mark.parametrize("real", [T.F32, T.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", range(6), ids=[f"{w}x{h}" for h, w in K.SHAPES])
def test_the_host_build_against_the_exact_reference(k, real):
    rows, n_exact = rows_of(real)
    want, stable = want_of(real, k)
    assert stable[:n_exact].all()  # no exact row is ever left out
    alone = host_eval([IMAGES[k]], 0, rows, real)
    pooled = host_eval(IMAGES, k, rows, real)
    assert np.array_equal(alone, pooled)
    ok = close(alone, want, real).all(axis=1)
    print(f"{K.SHAPES[k]}: largest error on the exact rows {np.abs(alone - want)[:n_exact].max():.3e}, generic rows left out {100 * (~stable[n_exact:]).mean():.2f} %")
    assert ok[:n_exact].all(), (rows[:n_exact][~ok[:n_exact]][:5], alone[:n_exact][~ok[:n_exact]][:5], want[:n_exact][~ok[:n_exact]][:5])
    bad = ~ok[n_exact:] & stable[n_exact:]
    assert not bad.any(), (rows[n_exact:][bad][:5], alone[n_exact:][bad][:5], want[n_exact:][bad][:5])


@pytest.mark.parametrize("real", [T.F32, T.F64], ids=["f32", "f64"])
def test_at_most_5_percent_of_the_generic_rows_are_left_out(real):
    _, n_exact = rows_of(real)
    for k in range(-1, 6):
        stable = want_of(real, k)[1]
        assert stable[:n_exact].all()
        share = float((~stable[n_exact:]).mean())
        print(f"image {k}: {100 * share:.2f} % of the generic rows left out")
        assert share <= 0.05, (k, share)


# ------------------------------------------------------------------ 3. the oracle's restatement
def test_the_oracle_s_table_on_the_f64_rows():
    rows, n_exact = rows_of(T.F64)
    want, stable = want_of(T.F64, -1)
    got = oracle.table("texture", rows)
    ok = close(got, want, T.F64).all(axis=1)
    assert ok[:n_exact].all(), (rows[:n_exact][~ok[:n_exact]][:5], got[:n_exact][~ok[:n_exact]][:5], want[:n_exact][~ok[:n_exact]][:5])
    assert not (~ok[n_exact:] & stable[n_exact:]).any()


# ------------------------------------------------------------------ 4. the scenes of tests/test_gpu_texture_edges.py
@pytest.fixture(scope="module")
def quad_scene():
    import texture_edge_scenes as S
    from test_gpu_features import camera_rays

    sd, quads = S.quad_scene()
    rays = camera_rays(sd, S.SPP, S.SEED, 1e-7)
    hit = S.oracle_hits(sd, rays)
    return S, sd, quads, rays, hit, S.interior_pixels(sd, hit, len(quads))


def test_every_quad_has_interior_pixels_and_the_window_quads_one_value(quad_scene):
    S, sd, quads, rays, hit, interior = quad_scene
    assert len(quads) == 192 and min(int(m.sum()) for m in interior) >= 16
    assert (hit[:, 0] != 0).all()  # the grid fills the image
    for real in (T.F32, T.F64):
        n = [len(S.quad_candidates(sd.images, q, real)) for q in quads]
        print(f"real {real}: {n.count(1)} quads with one candidate value, {n.count(2)} with two, {n.count(4)} with four")
        for (m, (cu, cv)), k in zip(quads, n):
            if m < 6 and cu in (-2.0 ** -26, 0.0, 2.0 ** -26, K.OTHER) and cv in (-2.0 ** -26, 0.0, 2.0 ** -26, K.OTHER):  # (0.0 == -0.0)
                assert k == 1, (m, cu, cv)
        assert n.count(1) >= 96


@pytest.mark.parametrize("real", [T.F32, T.F64], ids=["f32", "f64"])
def test_the_oracle_s_own_uvs_give_a_mean_of_candidates_on_every_interior_pixel(quad_scene, real):
    """what tests/test_gpu_texture_edges.py asks of the device, asked of the oracle's hits in the same precision"""
    S, sd, quads, rays, hit, interior = quad_scene
    if real == T.F32:
        hit = S.oracle_hits(sd, rays.astype(np.float32).astype(np.float64), 0)
    plane = S.albedo_plane(sd, hit, real)
    for k, quad in enumerate(quads):
        err = S.pixel_errors(plane[interior[k]], S.quad_candidates(sd.images, quad, real))
        assert (err <= (1e-3 if real == T.F32 else 1e-9)).all(), (k, quad, float(err.max()))


def test_the_sphere_scene_leaves_room_for_f32():
    """the oracle's float twin against the exact f64 plane: within 1e-3 on >= 99 % of the pixels (measured: 100 %)"""
    import texture_edge_scenes as S
    from test_gpu_features import camera_rays, share_within

    sd = S.sphere_scene()
    rays = camera_rays(sd, S.SPP, S.SEED, 1e-7)
    hit = S.oracle_hits(sd, rays)
    want = S.albedo_plane(sd, hit, T.F64)
    twin = S.albedo_plane(sd, S.oracle_hits(sd, rays.astype(np.float32).astype(np.float64), 0), T.F32)
    covered = (hit[:, 0] != 0).reshape(sd.height, sd.width, -1)
    assert 0.3 < covered.mean() < 0.9 and covered[sd.height // 2 - 1:sd.height // 2 + 1, sd.width // 2 - 1:sd.width // 2 + 1].all()
    assert hit[hit[:, 0] != 0, 12].min() < -0.99 and hit[hit[:, 0] != 0, 11].min() < 0.01 and hit[hit[:, 0] != 0, 11].max() > 0.99
    share = share_within(twin, want, 1e-3)
    print(f"f32 twin within 1e-3 of the exact f64 plane on {100 * share:.3f} % of the pixels")
    assert share >= 0.99, share


@pytest.mark.parametrize("precision", [1, 0], ids=["f64", "f32"])
def test_the_device_headers_on_the_host_render_the_quad_scene_as_the_oracle_does(quad_scene, precision):
    """tk_shade.h and oracle/take_oracle.hpp wrap alike at every seam of the scene: on the host, with one libm, the two
    renders are equal bit for bit (tests/test_hostsim_parity.py's bar) — and neither reads outside an image on the way"""
    from helpers import hostsim_render

    sd = quad_scene[1]
    osc = oracle.OracleScene(sd, precision=precision)
    want = osc.render(2, 5, rng_mode=oracle.RNG_COUNTER, seed=11)
    osc.close()
    got, _ = hostsim_render(sd, precision, 2, 5, seed=11)
    assert want.max() > 0.3 and np.array_equal(got.astype(np.float64), want)

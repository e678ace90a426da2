"""Path tracing of caller-supplied rays and the export of a scene's camera rays on the device (take_hip_render_rays*,
take_hip_camera_rays*: include/take_hip.h; DESIGN.md par. 4n; kernels: take_amd/csrc/tk_rays.h, driver: tk_render.hip
rays_impl / camera_rays_impl).

The pin: the exported camera rays, path-traced by the new call, are take_hip_render's image bit for bit — which holds
only if key, slot order, batch split and the mixed hand-over are the render's.  The export itself is held to the device
text built for the host (tests/lens_host: generate_path) with tests/test_lens_cpu.py's bars, 1e-12 in f64 and 1e-5 in
f32 (one libm against another on values of order 1).  Everything the library is compared with itself on is
np.array_equal.  The furnace expectation and its 2 % are tests/test_gpu_parity.py::test_white_furnace's.

Scenes: the golden ones and test_gpu_features.placed_scene (two-level), with the camera set to 24 x 16 in this file's own
copy of the scene data."""
import ctypes as C

import numpy as np
import pytest

import lens_ref as L
from helpers import golden_scene
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import SceneData
from test_gpu_features import placed_scene
from test_lens_cpu import host_records

pytestmark = pytest.mark.gpu
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]
W, H, N = 24, 16, 24 * 16
SPP, DEPTH, SEED = 5, 4, 5
LENS_RADIUS = 0.05


def scene_data(name):
    sd = placed_scene() if name == "placed" else golden_scene(name)
    sd.width, sd.height = W, H
    return sd


@pytest.fixture(scope="module")
def resident():
    """scenes by (name, precision), created once for the module; the tests leave them as they found them (no lens)"""
    made = {}

    def get(name, precision):
        if (name, precision) not in made:
            made[(name, precision)] = capi.Scene(scene_data(name), precision=precision)
        return made[(name, precision)]

    yield get
    for sc in made.values():
        sc.close()


def image(texels):
    """(H * W, 3) texels in ray order (row y = 0 the bottom) -> the (H, W, 3) image, top row first"""
    return texels.reshape(H, W, 3)[::-1]


def dtype_of(precision):
    return np.float32 if precision == F32 else np.float64


# ------------------------------------------------------------------ 1. the pin
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["cbox", "mats", "spherelight", "placed"])
def test_the_exported_camera_rays_render_the_render_s_image(resident, name, precision):
    sc = resident(name, precision)

    def pin(label, **kw):
        rays = sc.camera_rays(SPP, seed=SEED)
        assert rays.shape == (SPP, N, 8) and rays.dtype == sc.dtype
        got = sc.render_rays(rays, SPP, DEPTH, seed=SEED, ray_sets=SPP, **kw)
        want = sc.render(spp=SPP, max_depth=DEPTH, seed=SEED, **kw)
        assert got.shape == (N, 3) and got.dtype == want.dtype and want.shape == (H, W, 3)
        assert np.isfinite(want).all() and want.max() > 0
        assert np.array_equal(image(got), want), (name, precision, label, int((image(got) != want).any(-1).sum()))
        return want

    plain = pin("pinhole")
    assert np.array_equal(pin("two samples per batch", samples_per_batch=2), plain)
    sc.set_lens(LENS_RADIUS)
    try:
        assert not np.array_equal(pin("lens"), plain)
    finally:
        sc.set_lens(0.0)


@pytest.mark.parametrize("integrator", [1, 2, 3])
def test_the_pin_holds_for_the_other_integrators(resident, integrator):
    sc = resident("cbox", F64)
    rays = sc.camera_rays(SPP, seed=SEED)
    got = sc.render_rays(rays, SPP, DEPTH, seed=SEED, ray_sets=SPP, integrator=integrator)
    want = sc.render(spp=SPP, max_depth=DEPTH, seed=SEED, integrator=integrator)
    assert want.max() > 0 and np.array_equal(image(got), want)
    assert not np.array_equal(want, sc.render(spp=SPP, max_depth=DEPTH, seed=SEED))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_environment_map_behaves_as_in_a_render(precision):
    """the pin with an importance-sampled sky over an open scene, and a render's refusal of the map for integrators 1..3"""
    sd = SceneData(width=W, height=H, lookfrom=(0.0, 0.3, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0,
                   background=(0.3, 0.2, 0.1), spp=4, max_depth=4)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    sd.add_sphere((-0.4, 0.0, 0.0), 0.45, grey)
    sd.add_sphere((0.5, -0.2, 0.2), 0.3, sd.add_material(D.MAT_MIRROR, (0.9, 0.9, 0.9)))
    sd.add_envmap(scenes.sky_envmap(32, 16))
    sc = capi.Scene(sd, precision=precision)
    try:
        rays = sc.camera_rays(SPP, seed=SEED)
        want = sc.render(spp=SPP, max_depth=DEPTH, seed=SEED)
        assert np.isfinite(want).all() and want.max() > 0
        assert np.array_equal(image(sc.render_rays(rays, SPP, DEPTH, seed=SEED, ray_sets=SPP)), want)
        for call in (lambda: sc.render_rays(rays, SPP, DEPTH, seed=SEED, ray_sets=SPP, integrator=2), lambda: sc.render(spp=SPP, max_depth=DEPTH, seed=SEED, integrator=2)):
            with pytest.raises(capi.TakeError, match="do not know the environment-map extension") as e:
                call()
            assert e.value.code == D.TAKE_E_INVALID
        assert np.array_equal(sc.render(spp=SPP, max_depth=DEPTH, seed=SEED), want)
    finally:
        sc.close()


# ------------------------------------------------------------------ 2. the export against the device text on the host
def as_records(rays):
    """(spp, H * W, 8) exported rays -> (H, W, spp, 8), image row 0 = top: the order of test_lens_cpu.host_records"""
    spp = rays.shape[0]
    return np.ascontiguousarray(rays.reshape(spp, H, W, 8)[:, ::-1].transpose(1, 2, 0, 3))


@pytest.mark.parametrize("precision,bar", [(F64, 1e-12), (F32, 1e-5), (MIXED, 1e-12)])
@pytest.mark.parametrize("radius", [0.0, LENS_RADIUS])
def test_the_exported_rays_are_the_host_build_s(resident, precision, bar, radius):
    sc = resident("cbox", precision)
    dtype = dtype_of(precision)
    cam = L.camera(sc.sd, dtype, radius, 0.0)
    want = host_records(cam, SPP, SEED, dtype, with_lens=radius > 0)
    sc.set_lens(radius)
    try:
        got = as_records(sc.camera_rays(SPP, seed=SEED))
    finally:
        sc.set_lens(0.0)
    eo = float(np.abs(got[..., 0:3].astype(np.float64) - want[..., 0:3]).max())
    ed = float(np.abs(got[..., 4:7].astype(np.float64) - want[..., 3:6]).max())
    print(f"{np.dtype(dtype).name}, radius {radius}: origins within {eo:.3e}, directions within {ed:.3e}")
    assert eo <= bar and ed <= bar
    if radius == 0:
        assert (got[..., 0:3] == cam["lookfrom"]).all()
    assert (got[..., 3] == dtype(1e-4 if precision == F32 else 1e-7)).all() and np.isposinf(got[..., 7]).all()
    assert float(np.abs((got[..., 4:7].astype(np.float64) ** 2).sum(-1) - 1.0).max()) <= (1e-12 if dtype == np.float64 else 1e-5)


@pytest.mark.parametrize("precision", [F32, F64])
def test_first_sample_numbers_the_exported_sets(resident, precision):
    sc = resident("cbox", precision)
    long = sc.camera_rays(SPP, seed=SEED)
    assert np.array_equal(sc.camera_rays(2, seed=SEED, first_sample=3), long[3:5])
    assert not np.array_equal(long[3], long[4]) and not np.array_equal(long, sc.camera_rays(SPP, seed=SEED + 1))
    assert (sc.camera_rays(1, seed=SEED, ray_epsilon=0.015625)[..., 3] == 0.015625).all()
    sc.set_lens(LENS_RADIUS)
    try:
        lens = sc.camera_rays(SPP, seed=SEED)
        assert np.array_equal(sc.camera_rays(2, seed=SEED, first_sample=3), lens[3:5]) and not np.array_equal(lens, long)
    finally:
        sc.set_lens(0.0)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["cbox", "placed"])
def test_the_exported_rays_go_into_the_trace_hook(resident, name, precision):
    sc = resident(name, precision)
    rays = sc.camera_rays(2, seed=SEED)
    hits = sc.trace_closest(rays[0])
    want = sc.render_features(2, seed=SEED, want=("shape_id",))["shape_id"]
    assert (want >= 0).mean() > 0.5
    assert np.array_equal(hits["shape_id"].reshape(H, W)[::-1], want)


# ------------------------------------------------------------------ 3. sample numbering
@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_sample_calls_are_the_samples_of_one_call(resident, precision):
    sc = resident("cbox", precision)
    T = sc.dtype
    rays = sc.camera_rays(SPP, seed=SEED)
    total = np.zeros((N, 3), T)
    for s in range(SPP):
        one = sc.render_rays(rays[s], 1, DEPTH, seed=SEED, first_sample=s)
        assert one.dtype == T
        total = total + one
    want = sc.render_rays(rays, SPP, DEPTH, seed=SEED, ray_sets=SPP)
    assert np.array_equal(total * (T(1) / T(SPP)), want)
    # a shifted numbering is another set of streams
    assert not np.array_equal(sc.render_rays(rays, SPP, DEPTH, seed=SEED, ray_sets=SPP, first_sample=1), want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_ray_set_is_the_ray_repeated(resident, precision):
    sc = resident("mats", precision)
    rays = sc.camera_rays(1, seed=SEED)[0]
    one = sc.render_rays(rays, SPP, DEPTH, seed=SEED, samples_per_batch=2)
    rep = sc.render_rays(np.repeat(rays[None], SPP, 0), SPP, DEPTH, seed=SEED, ray_sets=SPP)
    assert one.max() > 0 and np.array_equal(one, rep)


# ------------------------------------------------------------------ 4. rays that are no camera rays
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rays_that_see_nothing_return_the_background(precision):
    """every sample's radiance is the background itself; with values and a sample count that are powers of two the sum
    and the multiplication by 1 / spp are exact"""
    sd = scene_data("cbox")
    sd.background = (0.25, 0.5, 0.125)
    sc = capi.Scene(sd, precision=precision)
    try:
        rng = np.random.default_rng(2)
        n = 100
        d = rng.normal(size=(n, 3))
        d[:, 1] = np.abs(d[:, 1]) + 0.1  # upwards, from far above everything
        d /= np.sqrt((d * d).sum(-1, keepdims=True))
        rays = np.zeros((n, 8), sc.dtype)
        rays[:, 0:3], rays[:, 4:7], rays[:, 7] = (0.0, 1000.0, 0.0), d, np.inf
        got = sc.render_rays(rays, 4, DEPTH, seed=SEED)
        assert got.shape == (n, 3) and (got == np.array(sd.background, sc.dtype)).all()
    finally:
        sc.close()


def test_rays_inside_the_white_furnace():
    """tests/test_gpu_parity.py::test_white_furnace's box, expectation and tolerance, seen by rays that start at random
    points inside it in random directions instead of by its camera (as many samples: 1024 rays x 256)"""
    rho, Le = 0.5, 1.0
    sd = SceneData(width=W, height=H, lookfrom=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), vfov=60.0,
                   background=(0.0, 0.0, 0.0), spp=64, max_depth=20)
    m = sd.add_material(D.MAT_DIFFUSE, (rho, rho, rho))
    faces = [((0, 0, -1), (1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, 0, 1), (-1, 0, 0), (0, 1, 0), (0, 0, -1)),
             ((0, -1, 0), (1, 0, 0), (0, 0, -1), (0, 1, 0)), ((0, 1, 0), (1, 0, 0), (0, 0, 1), (0, -1, 0)),
             ((-1, 0, 0), (0, 0, -1), (0, 1, 0), (1, 0, 0)), ((1, 0, 0), (0, 0, 1), (0, 1, 0), (-1, 0, 0))]
    for c, ux, uy, nrm_ in faces:
        pos, idx, nrm, uv = scenes._quad(c, ux, uy, nrm_)
        sd.add_mesh(pos, idx, m, normals=nrm, uvs=uv, emission=(Le, Le, Le))
    rng = np.random.default_rng(4)
    n = 1024
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = rng.uniform(-0.5, 0.5, (n, 3)), d, np.inf
    sc = capi.Scene(sd, precision=F32)
    try:
        got = sc.render_rays(rays, 256, 20, seed=2)
    finally:
        sc.close()
    want = Le * sum(rho ** k for k in range(0, 22))
    print(f"furnace: mean {got.mean():.5f}, expected {want:.5f}")
    assert abs(got.mean() - want) / want < 0.02


@pytest.mark.parametrize("precision", [F32, F64])
def test_the_normalise_flag_on_the_device_is_the_restated_normalize(resident, precision):
    sc = resident("cbox", precision)
    T = sc.dtype
    rays = sc.camera_rays(1, seed=SEED)[0]
    scaled = rays.copy()
    scaled[:, 4:7] = rays[:, 4:7] * T(3.7)
    before = scaled.copy()
    before[:, 4:7] = L._norm(np.ascontiguousarray(scaled[:, 4:7]), T)
    assert before.dtype == T and not np.array_equal(before[:, 4:7], rays[:, 4:7])
    got = sc.render_rays(scaled, 3, DEPTH, seed=SEED, normalize=True)
    want = sc.render_rays(before, 3, DEPTH, seed=SEED)
    assert want.max() > 0 and np.array_equal(got, want)
    with pytest.raises(capi.TakeError, match="ray 0: the direction is not of unit length") as e:
        sc.render_rays(scaled, 3, DEPTH, seed=SEED)
    assert e.value.code == D.TAKE_E_INVALID


# ------------------------------------------------------------------ 5. shapes where the launches can go wrong
@pytest.mark.parametrize("precision", [F32, F64])
def test_small_and_odd_ray_counts(resident, precision):
    """a texel's stream depends on its index alone: the first n texels of a longer call are the call on the first n rays
    (n = 1, one wave less one, one wave, one wave and one, a block and one)"""
    sc = resident("cbox", precision)
    rays = sc.camera_rays(1, seed=SEED)[0][::-1].copy()  # (top row first: most of these see the box)
    full = sc.render_rays(rays[:257], 3, 2, seed=SEED)
    assert full.shape == (257, 3) and full.max() > 0
    for n in (1, 63, 64, 65):
        got = sc.render_rays(rays[:n], 3, 2, seed=SEED)
        assert got.shape == (n, 3) and np.array_equal(got, full[:n]), n
    assert sc.render_rays(rays[:0], 3, 2, seed=SEED).shape == (0, 3)


@pytest.mark.parametrize("precision", [F32, F64])
def test_more_slots_than_the_grid_has_threads(resident, precision):
    """n = 70001 rays x 8 samples in one batch = 560008 slots, more than num_cus * 8 * BLOCK = 524288 threads: the
    grid-stride loops of the generate, accumulate and resolve kernels wrap.  Against the same call in batches of one
    sample (70001 slots: no loop wraps); texels 0 and 1 against a call of those two rays, texel n - 1 against a call
    in which it is alone at its index (the rays before it see nothing)"""
    sc = resident("cbox", precision)
    base = sc.camera_rays(1, seed=SEED)[0]
    n = 70001
    rays = np.ascontiguousarray(np.tile(base, (n // N + 1, 1))[:n])
    got = sc.render_rays(rays, 8, 1, seed=SEED, samples_per_batch=8)
    assert sc.counters()["samples"] == n * 8
    want = sc.render_rays(rays, 8, 1, seed=SEED, samples_per_batch=1)
    assert got.max() > 0 and np.array_equal(got, want)
    assert np.array_equal(sc.render_rays(rays[:2], 8, 1, seed=SEED), got[:2])
    # texel n - 1 alone at its index: the rays before it replaced by rays that see nothing
    alone = rays.copy()
    alone[:n - 1, 0:3], alone[:n - 1, 4:7] = (0.0, 1000.0, 0.0), (0.0, 1.0, 0.0)
    assert np.array_equal(sc.render_rays(alone, 8, 1, seed=SEED, samples_per_batch=8)[n - 1], got[n - 1])


# ------------------------------------------------------------------ 6. lifecycle
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_scene_renders_as_before(resident, precision):
    sc = resident("mats", precision)
    before = sc.render(spp=3, max_depth=DEPTH, seed=SEED)
    rays = sc.camera_rays(2, seed=9)
    texels = sc.render_rays(rays[0, :100], 2, DEPTH, seed=9)
    c = sc.counters()
    assert c["samples"] == 100 * 2 and c["rays_closest"] >= c["samples"]
    assert np.array_equal(sc.render(spp=3, max_depth=DEPTH, seed=SEED), before)
    # a refused call leaves the next render unchanged
    with pytest.raises(capi.TakeError, match="ray_sets must be 1 or spp") as e:
        sc.render_rays(rays, SPP, DEPTH, seed=9, ray_sets=2)
    assert e.value.code == D.TAKE_E_INVALID
    assert np.array_equal(sc.render(spp=3, max_depth=DEPTH, seed=SEED), before)
    assert np.array_equal(sc.render_rays(rays[0, :100], 2, DEPTH, seed=9), texels)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_progressive_sequences(resident, precision):
    import torch

    sc = resident("cbox", precision)
    buf = torch.zeros((H, W, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
    assert sc.render_accumulate(buf.data_ptr(), 2, DEPTH, seed=SEED, restart=True) == 2
    rays = sc.camera_rays(3, seed=11)  # path records only: the sequence goes on
    assert capi.lib().take_hip_accumulated_samples(sc.h) == 2
    assert sc.render_accumulate(buf.data_ptr(), 3, DEPTH, seed=SEED) == 5
    torch.cuda.synchronize()
    acc = buf.cpu().numpy()
    sc.render_rays(rays[0], 1, DEPTH, seed=11)  # the accumulator is the render workspace's: the sequence ends
    assert capi.lib().take_hip_accumulated_samples(sc.h) == 0
    assert np.array_equal(acc, sc.render(spp=5, max_depth=DEPTH, seed=SEED))


def test_the_device_entries_take_torch_tensors(resident):
    import torch

    sc = resident("cbox", F32)
    d_rays = torch.zeros((SPP, N, 8), dtype=torch.float32, device="cuda")
    sc.camera_rays_device(d_rays, SPP, seed=SEED)
    torch.cuda.synchronize()
    assert np.array_equal(d_rays.cpu().numpy(), sc.camera_rays(SPP, seed=SEED))
    d_out = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    sc.render_rays_device(d_rays, N, d_out, SPP, DEPTH, seed=SEED, ray_sets=SPP)
    torch.cuda.synchronize()
    assert np.array_equal(image(d_out.cpu().numpy()), sc.render(spp=SPP, max_depth=DEPTH, seed=SEED))


def test_a_scene_group_has_no_such_call():
    """the entry points take a TakeScene; a group's handle is another type, and the binding offers it no such method"""
    assert not any(hasattr(capi.SceneGroup, n) for n in ("render_rays", "render_rays_device", "camera_rays", "camera_rays_device"))
    handle = C.c_void_p()
    assert capi.lib().take_hip_render_rays(handle, None, None, None) == D.TAKE_E_INVALID

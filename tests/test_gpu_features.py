"""First-hit feature buffers on the device (take_hip_render_features: the camera + closest-hit launch of a render's
round 0, then k_features / k_features_resolve — take_amd/csrc/tk_features.h, tk_render.hip: features_impl) against planes
made from the oracle alone: the camera basis as make_camera computes it, the jitter from oracle.counter_words, the hits
from OracleScene.isect, the albedo from the scene's material table (a constant colour, or a numpy restatement of the
bilinear wrap lookup of src/texture.cpp:3-25).

Bars.  f64: ids equal on every pixel, every Real plane within 1e-9 on >= 99.5 % of the pixels (tests/test_gpu_parity.py's
bar and share for rounding-level agreement; the expected number of excluded pixels is 0, the cap is there for a one-ulp
ray difference at a silhouette).  f32 against the f64 oracle: >= 99 % of the pixels within 1e-3 in every plane, ids equal
on >= 99 % (the oracle's f32 twin against its f64 self, 4 spp, seed 5: at most 1 pixel of 3072 beyond 1e-4, none flipped).
Everything the library is compared with itself on is np.array_equal."""
import copy

import numpy as np
import pytest

import oracle
from helpers import golden_scene
from take_amd import capi, scenes
from take_amd import cdefs as D
from take_amd.scene import SceneData
from test_gpu_device_build_instanced import bent_grid, scene_with_node_format

pytestmark = pytest.mark.gpu
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
REAL = ("albedo", "normal", "depth", "alpha")
IDS = ("shape_id", "material_id")
SPP, SEED = 4, 5


# ------------------------------------------------------------------ the expected planes, from the oracle alone
def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def camera_rays(sd, spp, seed, tmin):
    """(H * W * spp, 8) rays org3 dir3 tmin tmax, image row major (row 0 = top), the samples of a pixel adjacent"""
    W, H = sd.width, sd.height
    h = np.tan(sd.vfov / 180.0 * np.pi / 2.0)
    vh = 2.0 * h
    vw = vh / H * W
    origin, at, up = (np.asarray(v, np.float64) for v in (sd.lookfrom, sd.lookat, sd.up))
    w = _unit(origin - at)
    u = _unit(np.cross(up, w))
    v = np.cross(w, u)
    jit = np.zeros((H, W, spp, 2))
    for r in range(H):
        y = H - 1 - r  # the render loop's y: 0 = the bottom row
        for x in range(W):
            for s in range(spp):
                jit[r, x, s] = (oracle.counter_words(seed, y * W + x, s, 2) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    ry, rx = jit[..., 0], jit[..., 1]  # y is drawn first
    xs = np.arange(W, dtype=np.float64)[None, :, None]
    ys = (H - 1 - np.arange(H, dtype=np.float64))[:, None, None]
    d = _unit(u * (((xs + rx) / W - 0.5) * vw)[..., None] + v * (((ys + ry) / H - 0.5) * vh)[..., None] - w)
    n = H * W * spp
    return np.concatenate([np.broadcast_to(origin, (n, 3)), d.reshape(n, 3), np.full((n, 1), tmin), np.full((n, 1), np.inf)], 1)


def texture_lookup(sd, m, uv):
    """src/texture.cpp:3-25 for an image texture: wrap, bilinear, the seam arithmetic kept"""
    img = np.asarray(sd.images[m.tex_image], np.float64)
    ih, iw = img.shape[:2]
    us, vs, uo, vo = m.uvxf

    def mod1(a):
        r = np.fmod(a, 1.0)
        return np.where(r < 0, np.minimum(r + 1.0, np.nextafter(1.0, 0.0)), r)  # below 1 where r + 1 rounds to 1

    x, y = iw * mod1(us * uv[:, 0] + uo), ih * mod1(vs * uv[:, 1] + vo)
    x1, y1 = np.floor(x).astype(int), np.floor(y).astype(int)
    x2, y2 = np.where(x1 + 1 == iw, 0, x1 + 1), np.where(y1 + 1 == ih, 0, y1 + 1)
    q11, q12, q21, q22 = img[y1, x1], img[y2, x1], img[y1, x2], img[y2, x2]
    x2, y2 = np.where(x1 == x2, x2 + 1, x2), np.where(y1 == y2, y2 + 1, y2)
    fx2, fx1, fy2, fy1 = (x2 - x)[:, None], (x - x1)[:, None], (y2 - y)[:, None], (y - y1)[:, None]
    return (q11 * fx2 * fy2 + q21 * fx1 * fy2 + q12 * fx2 * fy1 + q22 * fx1 * fy1) / ((x2 - x1) * (y2 - y1))[:, None]


def expected_planes(sd, spp=SPP, seed=SEED, tmin=1e-7):
    """the contract of include/take_hip.h computed by the f64 oracle (sd: no placements — flatten first)"""
    W, H = sd.width, sd.height
    osc = oracle.OracleScene(sd, 1)
    try:
        hit = osc.isect(camera_rays(sd, spp, seed, tmin))
    finally:
        osc.close()
    is_hit = hit[:, 0] != 0
    mat = hit[:, 13].astype(int)
    albedo = np.zeros((hit.shape[0], 3))
    for k, m in enumerate(sd.materials):
        sel = is_hit & (mat == k)
        if sel.any():
            albedo[sel] = texture_lookup(sd, m, hit[sel, 11:13]) if m.tex_kind else np.asarray(m.color, np.float64)
    per_sample = {"albedo": albedo, "normal": np.where(is_hit[:, None], hit[:, 8:11], 0.0),
                  "depth": np.where(is_hit, hit[:, 1], 0.0)[:, None], "alpha": is_hit.astype(np.float64)[:, None]}
    out = {}
    for name, a in per_sample.items():
        a = a.reshape(H, W, spp, -1)
        total = np.zeros_like(a[:, :, 0])
        for s in range(spp):  # in sample order
            total = total + a[:, :, s]
        out[name] = (total / spp).reshape((H, W, 3) if a.shape[-1] == 3 else (H, W))
    first = hit.reshape(H, W, spp, -1)[:, :, 0]
    out["shape_id"] = np.where(first[..., 0] != 0, first[..., 16], -1).astype(np.int32)
    out["material_id"] = np.where(first[..., 0] != 0, first[..., 13], -1).astype(np.int32)
    return out


_EXPECTED = {}


def expected_golden(name):
    """computed once per scene, shared by the f64 and f32 tests (the camera starts outside every scene: the two
    precisions' tmin does not matter to it), never written to"""
    if name not in _EXPECTED:
        _EXPECTED[name] = expected_planes(golden_scene(name))
    return _EXPECTED[name]


def share_within(got, want, bar):
    """share of the pixels whose every component of the plane is within `bar`"""
    d = np.abs(np.asarray(got, np.float64) - want)
    return float((d.reshape(d.shape[0], d.shape[1], -1).max(-1) <= bar).mean())


def rounding_level(got, want, label):
    """the f64 bar"""
    for n in IDS:
        assert np.array_equal(got[n], want[n]), (label, n, int((got[n] != want[n]).sum()))
    for n in REAL:
        share = share_within(got[n], want[n], 1e-9)
        print(f"{label}: {n} within 1e-9 on {100 * share:.3f} % of the pixels")
        assert got[n].dtype == np.float64 and share >= 0.995, (label, n, share)


def same_planes(a, b, label=""):
    assert set(a) == set(b)
    for n in a:
        assert a[n].dtype == b[n].dtype and np.array_equal(a[n], b[n]), (label, n)


def features(sd, precision, spp=SPP, seed=SEED, **kw):
    sc = capi.Scene(sd, precision=precision)
    try:
        return sc.render_features(spp, seed=seed, **kw)
    finally:
        sc.close()


# ------------------------------------------------------------------ 1. f64 against the oracle
@pytest.mark.parametrize("name", ["cbox", "mats", "meshlight"])
def test_f64_against_the_oracle(name):
    sd = golden_scene(name)
    got = features(sd, F64)
    want = expected_golden(name)
    assert got["albedo"].shape == (sd.height, sd.width, 3) and got["depth"].shape == (sd.height, sd.width)
    assert (want["shape_id"] >= 0).mean() > 0.5 and len(np.unique(want["material_id"])) > 2
    rounding_level(got, want, name)


# ------------------------------------------------------------------ 2. f32 against the f64 oracle
@pytest.mark.parametrize("name", ["cbox", "mats", "meshlight", "spherelight"])
def test_f32_against_the_f64_oracle(name):
    got = features(golden_scene(name), F32)
    want = expected_golden(name)
    for n in REAL:
        share = share_within(got[n], want[n], 1e-3)
        print(f"{name}: {n} within 1e-3 on {100 * share:.3f} % of the pixels")
        assert got[n].dtype == np.float32 and share >= 0.99, (name, n, share)
    for n in IDS:
        share = float((got[n] == want[n]).mean())
        print(f"{name}: {n} equal on {100 * share:.3f} % of the pixels")
        assert got[n].dtype == np.int32 and share >= 0.99, (name, n, share)


# ------------------------------------------------------------------ 3. placements
def placed_scene():
    """3 prototypes with vertex normals and uvs (one textured), 5 placements under rotation x non-uniform scale +
    translation, one of them with a material of its own; walls, a light and a sphere beside them"""
    sd = SceneData(width=48, height=32, lookfrom=(0.0, 0.0, 3.9), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0),
                   vfov=scenes.vfov_from_xfov(39.0, 48, 32), background=(0.1, 0.1, 0.1), spp=4, max_depth=4)
    rng = np.random.default_rng(11)
    sd.images.append(rng.uniform(0.05, 0.95, (6, 8, 3)))
    white = sd.add_material(D.MAT_DIFFUSE, (0.73, 0.73, 0.73))
    red = sd.add_material(D.MAT_DIFFUSE, (0.65, 0.05, 0.05))
    green = sd.add_material(D.MAT_PLASTIC, (0.12, 0.45, 0.15), (1.5,))
    checker = sd.add_material(D.MAT_DIFFUSE, (0.5, 0.5, 0.5), tex_image=0, uvxf=(3.0, 2.0, 0.25, 0.4))
    blue = sd.add_material(D.MAT_PHONG, (0.2, 0.3, 0.8), (20.0,))
    scenes.box_with_light(sd, white, red, green)
    sd.add_sphere((0.6, -0.7, 0.4), 0.25, checker)
    protos = []
    for n, mat in ((3, checker), (4, white), (5, checker)):
        pos, idx, nrm, uv = bent_grid(n)
        protos.append(sd.add_prototype(pos, idx, mat, normals=nrm, uvs=uv))
    for k, x in enumerate(placement_transforms(1)):
        sd.add_instance(protos[k % 3], x, blue if k == 3 else -1)
    return sd


def placement_transforms(seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(5):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        t = np.array([-0.6 + 0.3 * k, rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.6)])
        out.append(np.concatenate([rot @ np.diag(rng.uniform(0.5, 1.3, 3)), t[:, None]], axis=1))
    return np.stack(out)


def test_placements_equal_the_flattened_scene_and_the_oracle():
    sd = placed_scene()
    moved = dict(lookfrom=(0.9, 0.5, 3.4), lookat=(0.0, -0.1, 0.0), up=(0.05, 1.0, 0.0), vfov=33.0)
    per_builder = []
    for builder in (DEV, HOST):
        a = capi.Scene(sd, precision=F64, builder=builder)
        try:
            assert a.build_info()["f64"] == builder
            steps, cur = [], sd
            for step in ("created", "re-posed", "camera"):
                if step == "re-posed":
                    cur = copy.copy(cur)
                    cur.instance_xform = list(placement_transforms(2))
                    a.set_instance_transforms(np.stack(cur.instance_xform))
                elif step == "camera":
                    cur = copy.copy(cur)
                    for k, v in moved.items():
                        setattr(cur, k, v)
                    a.set_camera(**moved)
                got = a.render_features(SPP, seed=SEED)
                steps.append(got)
                if builder == HOST:
                    continue  # (its planes are compared with the device build's below: the yardsticks are the same)
                flat = cur.flattened()
                instanced = got["shape_id"] >= sd.n_shapes
                assert 0.03 < instanced.mean() < 0.9, (step, instanced.mean())
                assert (got["material_id"][instanced] == 4).any() and (got["material_id"][instanced] == 3).any()
                through_the_same_call = features(flat, F64)
                for n in IDS:
                    assert np.array_equal(got[n], through_the_same_call[n]), (step, n)
                for n in REAL:
                    share = share_within(got[n], through_the_same_call[n], 1e-9)
                    print(f"{step}: {n} within 1e-9 of the flattened scene's on {100 * share:.3f} % of the pixels")
                    assert share >= 0.995, (step, n, share)
                rounding_level(got, expected_planes(flat), step + " against the oracle")
            assert not np.array_equal(steps[0]["depth"], steps[1]["depth"]) and not np.array_equal(steps[1]["depth"], steps[2]["depth"])
            per_builder.append(steps)
        finally:
            a.close()
    for dev, host in zip(*per_builder):
        same_planes(dev, host, "device LBVH against host SAH")


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("precision", [F32, F64])
def test_batches_strips_and_subsets_change_nothing(precision):
    sd = golden_scene("mats")
    sc = capi.Scene(sd, precision=precision)
    try:
        full = sc.render_features(6, seed=SEED)
        assert ((full["alpha"] > 0) & (full["alpha"] < 1)).any()  # partly covered pixels exist
        for spb in (1, 4):
            same_planes(full, sc.render_features(6, seed=SEED, samples_per_batch=spb), f"samples_per_batch {spb}")
        for first, stride in ((1, 3), (0, 2)):
            rows = sc.rows(first, stride)
            assert 0 < len(rows) < sd.height
            part = sc.render_features(6, seed=SEED, strip_first=first, strip_stride=stride, samples_per_batch=4)
            same_planes({n: a[rows] for n, a in full.items()}, part, f"strips {first} of {stride}")
        two = sc.render_features(6, seed=SEED, want=("depth", "shape_id"))
        same_planes({n: full[n] for n in ("depth", "shape_id")}, two, "two planes only")
    finally:
        sc.close()


def test_device_buffers_equal_the_host_call():
    import torch

    sd = golden_scene("mats")
    sc = capi.Scene(sd, precision=F32)
    try:
        host = sc.render_features(SPP, seed=SEED)
        t = {n: torch.full(host[n].shape, -7, dtype=torch.int32 if n in IDS else torch.float32, device="cuda") for n in host}
        sc.render_features_device(t, SPP, seed=SEED)
        torch.cuda.synchronize()
        same_planes(host, {n: v.cpu().numpy() for n, v in t.items()})
    finally:
        sc.close()


# ------------------------------------------------------------------ every trace kernel instance behind the pass
@pytest.mark.parametrize("precision", [F32, F64])
def test_node_formats_and_counting_instances_change_nothing(precision, monkeypatch):
    """compressed 4-wide nodes with the fused camera launch (the default), full-width and 8-wide nodes and the counting
    instances (k_generate + the queue): the planes are the same bit for bit, and the counters are a render's"""
    monkeypatch.delenv("TAKE_HIP_NODES", raising=False)
    sd = golden_scene("mats")
    want = features(sd, precision)
    for fmt in ("wide", "q8"):
        sc = scene_with_node_format(fmt, sd, precision=precision)
        try:
            same_planes(want, sc.render_features(SPP, seed=SEED), fmt)
        finally:
            sc.close()
    sc = capi.Scene(sd, precision=precision)
    try:
        sc.set_instrumentation(timing=True, counting=True)
        same_planes(want, sc.render_features(SPP, seed=SEED, samples_per_batch=3), "counting")
        c = sc.counters()
        n = sd.width * sd.height * SPP
        assert c["samples"] == n and c["rays_closest"] == n and c["rays_shadow"] == 0 and c["bounces"] == 0
        assert c["node_visits"] > n and c["launches_trace_closest"] == 2
        assert c["ms_total"] > 0 and c["ms_trace_closest"] > 0 and c["ms_shade"] > 0 and c["ms_trace_shadow"] == 0
        sc.set_instrumentation()
        same_planes(want, sc.render_features(SPP, seed=SEED), "plain again")
        c = sc.counters()
        assert c["samples"] == n and c["rays_closest"] == n
    finally:
        sc.close()


# ------------------------------------------------------------------ 5. mixed precision
def test_a_mixed_scene_gives_its_f64_side_s_planes():
    sd = golden_scene("mats")
    want = features(sd, F64)
    got = features(sd, MIXED)
    assert all(got[n].dtype == np.float64 for n in REAL)
    same_planes(want, got)


# ------------------------------------------------------------------ 6. a progressive sequence goes on
@pytest.mark.parametrize("precision", [F32, F64, MIXED])
def test_a_progressive_sequence_survives(precision):
    import torch

    sd = golden_scene("cbox")
    sc = capi.Scene(sd, precision=precision)
    try:
        buf = torch.zeros((sd.height, sd.width, 3), dtype=torch.float32 if precision == F32 else torch.float64, device="cuda")
        assert sc.render_accumulate(buf.data_ptr(), 3, 6, seed=SEED, restart=True) == 3
        planes = sc.render_features(SPP, seed=SEED)
        assert capi.lib().take_hip_accumulated_samples(sc.h) == 3
        sc.render_features(2, seed=9, strip_first=1, strip_stride=2)  # other options, another strip set
        assert sc.render_accumulate(buf.data_ptr(), 4, 6, seed=SEED) == 7
        torch.cuda.synchronize()
        assert capi.lib().take_hip_accumulated_samples(sc.h) == 7
        assert np.array_equal(buf.cpu().numpy(), sc.render(spp=7, max_depth=6, seed=SEED))
        same_planes(planes, sc.render_features(SPP, seed=SEED))
    finally:
        sc.close()


# ------------------------------------------------------------------ 7. environment map
@pytest.mark.parametrize("precision", [F32, F64])
def test_a_miss_is_zero_with_an_environment_map(precision):
    sd = SceneData(width=40, height=28, lookfrom=(0.0, 0.3, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0,
                   background=(0.3, 0.2, 0.1), spp=4, max_depth=4)
    grey = sd.add_material(D.MAT_DIFFUSE, (0.6, 0.6, 0.6))
    gold = sd.add_material(D.MAT_BLINN_PHONG_MICROFACET, (0.8, 0.7, 0.3), (30.0,))
    sd.add_sphere((-0.4, 0.0, 0.0), 0.45, gold)
    pos, idx, nrm, uv = bent_grid(3)
    sd.add_mesh(pos + (0.5, -0.2, 0.2), idx, grey, normals=nrm, uvs=uv)
    without = features(sd, precision)
    lit = copy.copy(sd)
    lit.images, lit.lights = list(sd.images), list(sd.lights)
    lit.add_envmap(scenes.sky_envmap(32, 16))
    got = features(lit, precision)
    miss = got["shape_id"] < 0
    assert 0.2 < miss.mean() < 0.95
    assert np.array_equal(miss, got["material_id"] < 0)
    for n in REAL:
        assert not got[n][miss & (got["alpha"] == 0)].any(), n
    assert ((got["alpha"] > 0) & (got["alpha"] < 1)).any() and (got["alpha"][~miss] > 0).all()
    assert (got["alpha"][miss] < 1).all()  # (sample 0 missed; later samples of the pixel may hit)
    same_planes(without, got, "the map changes nothing")


# ------------------------------------------------------------------ 8. errors
@pytest.mark.parametrize("precision", [F32, MIXED])
def test_refusals_leave_the_scene_as_it_was(precision):
    sd = golden_scene("cbox")
    sc = capi.Scene(sd, precision=precision)
    try:
        image = sc.render(spp=2, max_depth=6, seed=3)
        planes = sc.render_features(SPP, seed=SEED)
        for kw in (dict(spp=SPP, want=()), dict(spp=0), dict(spp=-3), dict(spp=SPP, strip_first=2, strip_stride=2),
                   dict(spp=SPP, strip_first=-1, strip_stride=1)):
            with pytest.raises(capi.TakeError) as e:
                sc.render_features(seed=SEED, **kw)
            assert e.value.code == D.TAKE_E_INVALID, kw
        assert np.array_equal(image, sc.render(spp=2, max_depth=6, seed=3))
        same_planes(planes, sc.render_features(SPP, seed=SEED))
    finally:
        sc.close()

"""take_hip_scene_set_envmap* on the GPU (include/take_hip.h): after the call a resident scene is, byte for
byte, the scene take_hip_scene_create makes from its description with the image (and the light's intensity) replaced.
What is compared: the dump of take_hip_debug_env_tables — the EnvMap record, marginal and conditional CDFs, both guide
tables, the map's texels, the whole image table, the light record's intensity — and renders, all bit for bit; and, so
that not everything leans on the host's tables, the independent float64 reference of tests/env_ref.py on the updated
scene (tests/env_checks.py: its bars, unchanged).  No tolerance of this file's own anywhere.  The maps: tests/envmap_cases.py."""
import numpy as np
import pytest

import env_checks as K
import env_maps
import envmap_cases as M
from take_amd import capi
from take_amd import cdefs as D
from take_amd import scenes as S
from take_amd.scene import SceneData

pytestmark = pytest.mark.gpu

F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PRECISIONS = [F32, F64, MIXED]
PID = {F32: "f32", F64: "f64", MIXED: "mixed"}
SIDES = {F32: [F32], F64: [F64], MIXED: [F64, F32]}
ARRAYS = ("marginal", "conditional", "guide_m", "guide_c", "texels", "images")
HEADER = ("width", "height", "n_guide_m", "n_guide_c", "texel0")


def scale_of(name):
    return env_maps.SCALES.get(name, M.SCALE)


def dumps(sc):
    """the dump of every resident side"""
    return [sc.debug_env_tables(side) for side in SIDES[sc.precision]]


def assert_same_dumps(got, want, what=""):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in HEADER:
            assert g[k] == w[k], (what, k, g[k], w[k])
        for k in ("scale", "intensity"):
            assert g[k].tobytes() == w[k].tobytes(), (what, k, g[k], w[k])
        for k in ARRAYS:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and g[k].tobytes() == w[k].tobytes(), (what, k)


def fresh_dumps(img, scale, precision):
    sc = capi.Scene(env_maps.env_scene(img, scale), precision=precision)
    try:
        return dumps(sc)
    finally:
        sc.close()


_FRESH = {}


def fresh(name, precision):
    """the dumps of a scene freshly created with map `name` and its scale, made once"""
    if (name, precision) not in _FRESH:
        _FRESH[name, precision] = fresh_dumps(M.image(name), scale_of(name), precision)
    return _FRESH[name, precision]


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own, which found no device when it was first initialised behind this module's two
    hundred scenes (run alone, the tensor cases passed): the cases that pass device tensors need it up before them"""
    import torch

    torch.cuda.init()


@pytest.fixture(scope="module")
def resident():
    """precision -> ONE scene created with `colours`, which every table case updates in turn: each case also shows that an
    update leaves nothing of the map before it"""
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = capi.Scene(env_maps.env_scene(env_maps.colours(), env_maps.COLOURS_SCALE), precision=precision)
        return made[precision]

    yield get
    for sc in made.values():
        sc.close()


# ------------------------------------------------------------------ the tables
TABLE_CASES = [(n, p) for n in M.CASES for p in (F32, F64)] + [(n, MIXED) for n in ("sun", "halves", "ragged", "65x63")]


@pytest.mark.parametrize("name,precision", TABLE_CASES, ids=[f"{n}-{PID[p]}" for n, p in TABLE_CASES])
def test_the_dump_is_the_fresh_scene_s(resident, name, precision):
    sc = resident(precision)
    sc.set_envmap(M.image(name), scale=scale_of(name))
    assert_same_dumps(dumps(sc), fresh(name, precision), name)


def test_the_sky_at_its_default_size():
    """2048 x 1024: 64 blocks of 16 rows, 32 tiles each, guide tables of 4096 and 2048 entries"""
    sky = S.sky_envmap()
    sc = capi.Scene(env_maps.env_scene(env_maps.colours(), env_maps.COLOURS_SCALE), precision=F32)
    try:
        sc.set_envmap(sky, scale=(1.0, 1.0, 1.0))
        got = dumps(sc)
    finally:
        sc.close()
    assert (got[0]["n_guide_m"], got[0]["n_guide_c"]) == (4096, 2048)
    assert_same_dumps(got, fresh_dumps(sky, (1.0, 1.0, 1.0), F32), "sky")


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["ragged", "range", "wide", "tall"])
def test_the_updated_scene_against_the_independent_reference(resident, name, precision):
    """tests/env_ref.py never sees the host's tables: samples, round trip, random directions and the normalisation of the
    shade kernel's own functions on the updated scene's resident tables, inside env_checks' bars"""
    sc = resident(precision)
    sc.set_envmap(env_maps.image(name), scale=env_maps.SCALES[name])
    c = K.case(name, precision)

    def run(kind, rows):
        return sc.debug_env(kind, rows, side=precision)

    sampled, _, _ = K.check_samples(c, run)
    K.check_round_trip(c, run, sampled)
    K.check_directions(c, run)
    K.check_normalisation(c, run)


@pytest.mark.parametrize("precision", PRECISIONS, ids=[PID[p] for p in PRECISIONS])
def test_a_round_trip_gives_the_original_dump(precision):
    a, b = M.image("ragged"), M.image("65x63")
    sc = capi.Scene(env_maps.env_scene(a, M.SCALE), precision=precision)
    try:
        first = dumps(sc)
        sc.set_envmap(b, scale=(0.25, 4.0, 1.0))
        assert dumps(sc)[0]["width"] == 65
        sc.set_envmap(a, scale=M.SCALE)
        assert_same_dumps(dumps(sc), first)
    finally:
        sc.close()


# ------------------------------------------------------------------ relocation: images before and behind the map
def textured_scene(env, scale, map_is_a_texture):
    """images [texture A, the map, texture B]; two textured quads in view, lit by the map alone — and, with
    map_is_a_texture, a third one that shows the map's own image"""
    rng = np.random.default_rng(31)
    sd = SceneData(width=16, height=16, lookfrom=(0.0, 0.0, 4.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), vfov=40.0, background=(0.0, 0.0, 0.0),
                   spp=4, max_depth=4)
    sd.images.append(rng.uniform(0.1, 0.9, (5, 7, 3)))
    sd.add_envmap(np.array(env), scale=scale)
    sd.images.append(rng.uniform(0.1, 0.9, (3, 2, 3)))
    quads = [((-1.0, 0.5, 0.0), 0), ((1.0, 0.5, 0.0), 2)] + ([((0.0, -1.0, 0.0), 1)] if map_is_a_texture else [])
    for centre, image in quads:
        mat = sd.add_material(D.MAT_DIFFUSE, (0.5, 0.5, 0.5), tex_image=image)
        pos, idx, nrm, uv = S._quad(centre, (0.8, 0.0, 0.0), (0.0, 0.6, 0.0), (0.0, 0.0, 1.0))
        sd.add_mesh(pos, idx, mat, normals=nrm, uvs=uv)
    return sd


@pytest.mark.parametrize("map_is_a_texture", [False, True], ids=["plain", "map-as-texture"])
@pytest.mark.parametrize("precision", PRECISIONS, ids=[PID[p] for p in PRECISIONS])
def test_images_behind_the_map_move_and_renders_follow(precision, map_is_a_texture):
    first, other_size = M.image("halves"), M.image("ragged")
    same_size = np.ascontiguousarray(np.resize(M.image("65x63"), (19, 37, 3)))  # (other texels at the size of `ragged`)

    def fresh_scene(env, scale):
        sc = capi.Scene(textured_scene(env, scale, map_is_a_texture), precision=precision)
        try:
            return dumps(sc), sc.render(spp=4, max_depth=4, seed=5)
        finally:
            sc.close()

    sc = capi.Scene(textured_scene(first, (1.0, 1.0, 1.0), map_is_a_texture), precision=precision)
    try:
        before = dumps(sc)[0]["images"]
        for env, scale in ((other_size, M.SCALE), (same_size, (2.0, 2.0, 0.5))):
            sc.set_envmap(env, scale=scale)
            want_dumps, want_img = fresh_scene(env, scale)
            got = dumps(sc)
            assert_same_dumps(got, want_dumps)
            assert np.array_equal(sc.render(spp=4, max_depth=4, seed=5), want_img)
            assert want_img.max() > 0
        after = got[0]["images"]
        assert list(after["offset"]) == [0, 35, 35 + 37 * 19] and list(before["offset"]) == [0, 35, 35 + 16 * 8]
        assert (after["width"][1], after["height"][1]) == (37, 19) and list(after["width"][[0, 2]]) == [7, 2]
    finally:
        sc.close()


@pytest.mark.parametrize("precision", PRECISIONS, ids=[PID[p] for p in PRECISIONS])
def test_the_render_of_a_lit_soup_is_the_fresh_scene_s(precision):
    sd = S.soup_scene(50, 16, 16, spp=4, envmap=(64, 32))
    want_sd = S.soup_scene(50, 16, 16, spp=4)
    want_sd.add_envmap(M.image("130x67"), scale=M.SCALE)
    sc, want = capi.Scene(sd, precision=precision), capi.Scene(want_sd, precision=precision)
    try:
        assert not np.array_equal(sc.render(spp=4, max_depth=6, seed=3), want.render(spp=4, max_depth=6, seed=3))
        sc.set_envmap(M.image("130x67"), scale=M.SCALE)
        assert np.array_equal(sc.render(spp=4, max_depth=6, seed=3), want.render(spp=4, max_depth=6, seed=3))
        assert_same_dumps(dumps(sc), dumps(want))
    finally:
        sc.close()
        want.close()


# ------------------------------------------------------------------ input kinds
@pytest.mark.parametrize("precision", PRECISIONS, ids=[PID[p] for p in PRECISIONS])
def test_device_tensors_and_float_texels(precision):
    import torch

    img = M.image("130x67")
    img32 = img.astype(np.float32)
    sc = capi.Scene(env_maps.env_scene(env_maps.colours(), env_maps.COLOURS_SCALE), precision=precision)
    try:
        # float64 on the device = float64 on the host; scale None keeps the scale
        sc.set_envmap(torch.from_numpy(np.array(img)).cuda())
        assert_same_dumps(dumps(sc), fresh_dumps(img, env_maps.COLOURS_SCALE, precision), "f64 tensor")
        # float32, from the host and from the device: the fresh scene of those values widened to double
        want = fresh_dumps(img32.astype(np.float64), M.SCALE, precision)
        sc.set_envmap(img32, scale=M.SCALE)
        assert_same_dumps(dumps(sc), want, "f32 host")
        sc.set_envmap(env_maps.colours())
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # (the texels are still being written on another stream when the call is made)
            t = torch.from_numpy(img32).cuda(non_blocking=True) * 1.0
            sc.set_envmap(t)
        assert_same_dumps(dumps(sc), want, "f32 tensor")
        with pytest.raises(ValueError):
            sc.set_envmap(t[:, ::2])  # (not contiguous)
    finally:
        sc.close()


# ------------------------------------------------------------------ the contract
@pytest.mark.parametrize("precision", PRECISIONS, ids=[PID[p] for p in PRECISIONS])
def test_a_refused_map_leaves_the_scene_as_it_was(precision):
    sd = S.soup_scene(50, 16, 16, spp=4, envmap=(64, 32))
    sc = capi.Scene(sd, precision=precision)
    try:
        img, tables = sc.render(spp=4, max_depth=6, seed=3), dumps(sc)
        for bad in (M.black(64, 32), M.one_nan(64, 32), M.black(), M.one_nan()):  # (of the map's own size: nothing may be overwritten in place)
            with pytest.raises(capi.TakeError, match="environment map: no positive luminance") as e:
                sc.set_envmap(bad, scale=(3.0, 3.0, 3.0))
            assert e.value.code == D.TAKE_E_INVALID
            assert_same_dumps(dumps(sc), tables)
            assert np.array_equal(sc.render(spp=4, max_depth=6, seed=3), img)
        # creation refuses the same maps with the same message
        for bad in (M.black(), M.one_nan()):
            with pytest.raises(capi.TakeError, match="environment map: no positive luminance"):
                capi.Scene(env_maps.env_scene(bad), precision=precision)
    finally:
        sc.close()


def test_a_scene_without_a_map_is_refused():
    sc = capi.Scene(S.soup_scene(50, 8, 8, spp=1))
    try:
        with pytest.raises(capi.TakeError, match="no environment map") as e:
            sc.set_envmap(env_maps.colours())
        assert e.value.code == D.TAKE_E_INVALID
        with pytest.raises(capi.TakeError, match="no environment map"):
            sc.debug_env_tables()
    finally:
        sc.close()


def test_a_successful_call_ends_a_progressive_sequence():
    import torch

    sc = capi.Scene(S.soup_scene(50, 16, 16, spp=4, envmap=(64, 32)))
    try:
        out = torch.zeros((16, 16, 3), dtype=torch.float32, device="cuda")
        assert sc.render_accumulate(out.data_ptr(), 2, 6, seed=1, restart=True) == 2
        with pytest.raises(capi.TakeError):
            sc.set_envmap(M.black())
        assert capi.lib().take_hip_accumulated_samples(sc.h) == 2  # (a refused call changes nothing)
        assert sc.render_accumulate(out.data_ptr(), 2, 6, seed=1) == 4
        sc.set_envmap(env_maps.colours())
        assert capi.lib().take_hip_accumulated_samples(sc.h) == 0
        with pytest.raises(capi.TakeError, match="restart"):
            sc.render_accumulate(out.data_ptr(), 2, 6, seed=1)
        assert sc.render_accumulate(out.data_ptr(), 2, 6, seed=1, restart=True) == 2
    finally:
        sc.close()


@pytest.mark.parametrize("precision", [F32, MIXED], ids=["f32", "mixed"])
def test_the_guide_override_is_honoured_as_creation_honours_it(precision, monkeypatch):
    img = M.image("65x63")
    sc = capi.Scene(env_maps.env_scene(env_maps.colours(), env_maps.COLOURS_SCALE), precision=precision)
    try:
        monkeypatch.setenv("TAKE_HIP_ENV_GUIDE", "4,2")
        sc.set_envmap(img, scale=M.SCALE)
        want = fresh_dumps(img, M.SCALE, precision)
        monkeypatch.delenv("TAKE_HIP_ENV_GUIDE")
        got = dumps(sc)
        assert (got[0]["n_guide_m"], got[0]["n_guide_c"]) == (4, 2)
        assert_same_dumps(got, want)
    finally:
        sc.close()


@pytest.mark.parametrize("precision", [F32, MIXED], ids=["f32", "mixed"])
def test_a_failed_allocation_leaves_the_scene_as_it_was(precision, monkeypatch):
    """every device allocation of the call fails in turn (fault injection, TAKE_HIP_FAIL_ALLOC): TAKE_E_NOMEM, and the
    dump and the render are what they were; then the call succeeds"""
    sc = capi.Scene(textured_scene(M.image("halves"), (1.0, 1.0, 1.0), True), precision=precision)
    try:
        img, tables = sc.render(spp=4, max_depth=4, seed=5), dumps(sc)
        failed = 0
        for nth in range(1, 40):
            monkeypatch.setenv("TAKE_HIP_FAIL_ALLOC", str(nth))
            try:
                sc.set_envmap(M.image("ragged"), scale=M.SCALE)
                monkeypatch.delenv("TAKE_HIP_FAIL_ALLOC")
                break
            except capi.TakeError as e:
                monkeypatch.delenv("TAKE_HIP_FAIL_ALLOC")
                assert e.code == D.TAKE_E_NOMEM, str(e)
                failed += 1
                assert_same_dumps(dumps(sc), tables)
                assert np.array_equal(sc.render(spp=4, max_depth=4, seed=5), img)
        # per side 3 in prepare (texels, image table, lights) and 4 tables; 4 shared (the image, row weights, prefixes, row sums)
        assert failed >= (18 if precision == MIXED else 11)
        assert dumps(sc)[0]["width"] == 37
    finally:
        sc.close()

"""take_hip_scene_set_materials and take_hip_scene_set_light_intensities* on the GPU (include/take_hip.h):
after the call a resident scene is, byte for byte, the scene take_hip_scene_create makes from its description with the
materials / intensities replaced.  What is compared, on every resident side: the dump of take_hip_debug_shading_tables —
material table, light records, both power tables, the placements' shade records, the host's tags in use —, the primitive
records of take_hip_debug_tree, and renders.  Every comparison is byte equality against a freshly created scene; no
tolerance anywhere.  The scenes and edits: tests/shading_update_cases.py (at most a few hundred records, 16 x 16, 4 spp)."""
import numpy as np
import pytest

import shading_update_cases as K
from take_amd import capi
from take_amd import cdefs as D

pytestmark = pytest.mark.gpu

F32, F64, MIXED = D.TAKE_PRECISION_F32, D.TAKE_PRECISION_F64, D.TAKE_PRECISION_MIXED
PID = {F32: "f32", F64: "f64", MIXED: "mixed"}
SIDES = {F32: [F32], F64: [F64], MIXED: [F64, F32]}
DEV, HOST = D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_BUILDER_HOST_SAH
TABLES = ("materials", "lights", "light_pmf", "light_cdf", "inst_shade")
TAGS_IN_USE = ("tag_mask", "n_material_tags", "single_tag", "real_bytes")
MATERIAL_CASES, LIGHT_CASES = K.material_cases(), K.light_cases()


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """the cases that pass device tensors need torch's HIP runtime up before this module's scenes (as
    tests/test_gpu_envmap_update.py found)"""
    import torch

    torch.cuda.init()


def create(sd, precision, **kw):
    sc = capi.Scene(sd, precision=precision, **kw)
    if precision == MIXED:
        sc.exact_bounces = 1  # the first round on the f64 side, the rest on the f32 side: a render reads both
    return sc


def same_bytes(a, b):
    """byte equality of every value of two arrays (of a structured array: of every field, not of its padding)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in a.dtype.names)
    return a.tobytes() == b.tobytes()


def tables(sc):
    return [sc.debug_shading_tables(side) for side in SIDES[sc.precision]]


def records(sc):
    return [sc.debug_tree(side)["prims"] for side in SIDES[sc.precision]]


def image(sc, integrator=0):
    return sc.render(spp=4, max_depth=4, seed=5, integrator=integrator)


def assert_same_tables(got, want, what=""):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in TAGS_IN_USE:
            assert g[k] == w[k], (what, k, g[k], w[k])
        for k in TABLES:
            assert same_bytes(g[k], w[k]), (what, k)


def assert_same_records(got, want, what="", n_shapes=None):
    """n_shapes: a two-level scene whose top level was rebuilt on the device — the shapes' records (the head) stand in
    the new tree's leaf order, which need not be a fresh build's: they are compared as a set, the prototypes' in place"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if n_shapes is not None:
            assert same_bytes(g[n_shapes:], w[n_shapes:]), what
            g, w = g[:n_shapes], w[:n_shapes]
            g, w = g[np.argsort(g["shape_id"], kind="stable")], w[np.argsort(w["shape_id"], kind="stable")]
        assert same_bytes(g, w), what


def assert_same_scene(a, b, what="", n_shapes=None, integrators=(0,)):
    assert_same_tables(tables(a), tables(b), what)
    assert_same_records(records(a), records(b), what, n_shapes)
    for i in integrators:
        assert np.array_equal(image(a, i), image(b, i)), (what, i)


def snapshot(sc):
    return tables(sc), records(sc), image(sc)


def assert_unchanged(sc, snap, what=""):
    assert_same_tables(tables(sc), snap[0], what)
    assert_same_records(records(sc), snap[1], what)
    assert np.array_equal(image(sc), snap[2]), what


def tags_of(recs):
    return [(r["meta"] >> 8) & 0xff for r in recs]


# ------------------------------------------------------------------ materials
SHOWS = ("colours", "mirror", "texture", "two-level", "spheres", "65-records", "257-records")  # edits of surfaces that fill the view
MIXED_TOO = ("colours", "mirror", "burley", "texture", "two-level", "flattened", "65-records", "257-records")
MATERIAL_RUNS = [(n, p) for n in MATERIAL_CASES for p in (F32, F64)] + [(n, MIXED) for n in MIXED_TOO]


@pytest.mark.parametrize("name,precision", MATERIAL_RUNS, ids=[f"{n}-{PID[p]}" for n, p in MATERIAL_RUNS])
def test_new_materials_leave_the_fresh_scene(name, precision):
    sd, first, new, kw, retag = MATERIAL_CASES[name]
    a, b = create(sd, precision, **kw), create(K.with_materials(sd, first, new), precision, **kw)
    try:
        before_tables, before_records, before_image = snapshot(a)
        a.set_materials(new, first)
        assert_same_scene(a, b, name)
        after_tables, after_records = tables(a), records(a)
        if name in SHOWS:
            assert not np.array_equal(image(a), before_image)  # (the edit shows)
        for side in range(len(after_records)):
            changed = not same_bytes(after_records[side], before_records[side]) or not same_bytes(after_tables[side]["inst_shade"], before_tables[side]["inst_shade"])
            # colours, textures, parameters: no record changes; a new tag: the records that use the material do
            assert changed == (retag and name != "unused-material"), name
            t = after_tables[side]["materials"]
            assert same_bytes(t[:first], before_tables[side]["materials"][:first]) and same_bytes(t[first + len(new):], before_tables[side]["materials"][first + len(new):])
        if name.endswith("-records"):
            assert len(after_records[0]) == int(name.split("-")[0])
        if name == "burley":
            assert list(after_tables[0]["materials"]["tag"]) == [D.MAT_BURLEY_METAL, D.MAT_BURLEY_GLASS, D.MAT_BURLEY_SHEEN]
            assert set(np.unique(tags_of(after_records[0]))) == {D.MAT_BURLEY_METAL, D.MAT_BURLEY_GLASS, D.MAT_BURLEY_SHEEN}
        if name in ("1to2", "2to1"):
            assert (before_tables[0]["n_material_tags"], after_tables[0]["n_material_tags"]) == ((1, 2) if name == "1to2" else (2, 1))
        if name == "2to1":
            assert after_tables[0]["single_tag"] == D.MAT_DIFFUSE and after_tables[0]["tag_mask"] == 1
        if name == "unused-material":
            assert after_tables[0]["n_material_tags"] == 2 and set(np.unique(tags_of(after_records[0]))) == {D.MAT_DIFFUSE}
        if name == "two-level":
            inst = after_tables[0]["inst_shade"]
            assert list(inst["material"]) == [0, 1, 0, 1, 2, 2] and list(inst["tag"]) == [D.MAT_MIRROR, D.MAT_DIFFUSE, D.MAT_MIRROR, D.MAT_DIFFUSE, D.MAT_PHONG, D.MAT_PHONG]
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("builder", [DEV, HOST], ids=["device-built", "host-built"])
def test_device_built_and_host_built_trees(builder):
    sd, first, new, kw, _ = MATERIAL_CASES["spheres"]
    a, b = create(sd, MIXED, builder=builder), create(K.with_materials(sd, first, new), MIXED, builder=builder)
    try:
        want = {"f32": builder, "f64": builder}
        assert a.build_info() == want and b.build_info() == want
        a.set_materials(new, first)
        assert_same_scene(a, b, builder)
    finally:
        a.close()
        b.close()


def test_a_q8_scene(monkeypatch):
    sd, first, new, kw, _ = MATERIAL_CASES["257-records"]
    monkeypatch.setenv("TAKE_HIP_NODES", "q8")
    a, b = create(sd, F32, builder=HOST), create(K.with_materials(sd, first, new), F32, builder=HOST)
    monkeypatch.delenv("TAKE_HIP_NODES")
    try:
        assert a.debug_tree()["node_width"] == 8
        a.set_materials(new, first)
        assert_same_scene(a, b, "q8")
    finally:
        a.close()
        b.close()


def test_the_albedo_follows_a_colour_change():
    sd, first, new, kw, _ = MATERIAL_CASES["colours"]
    a, b = create(sd, F32), create(K.with_materials(sd, first, new), F32)
    try:
        before = a.render_features(4, seed=2, want=("albedo",))["albedo"]
        a.set_materials(new, first)
        got, want = a.render_features(4, seed=2, want=("albedo",))["albedo"], b.render_features(4, seed=2, want=("albedo",))["albedo"]
        assert np.array_equal(got, want) and not np.array_equal(got, before)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ ... and the updates that build on the tags
@pytest.mark.parametrize("materials_first", [True, False], ids=["materials-then-transforms", "transforms-then-materials"])
@pytest.mark.parametrize("precision", [F32, F64, MIXED], ids=["f32", "f64", "mixed"])
def test_new_materials_and_a_re_pose_in_either_order(precision, materials_first):
    sd, first, new, kw, _ = MATERIAL_CASES["two-level"]
    x = K.reposed(sd)
    a, b = create(sd, precision), create(K.with_transforms(K.with_materials(sd, first, new), x), precision)
    try:
        for step in ((0, 1) if materials_first else (1, 0)):
            if step == 0:
                a.set_materials(new, first)
            else:
                a.set_instance_transforms(x)
        assert_same_scene(a, b, n_shapes=sd.n_shapes)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("materials_first", [True, False], ids=["materials-then-vertices", "vertices-then-materials"])
@pytest.mark.parametrize("precision", [F32, F64, MIXED], ids=["f32", "f64", "mixed"])
def test_new_materials_and_moved_vertices_in_either_order(precision, materials_first):
    """set_mesh_vertices makes the records again from the host's material tags: they must be the new ones"""
    sd, first, new, kw, _ = MATERIAL_CASES["spheres"]
    pos = K.bent(sd.meshes[1].positions)
    a, b = create(sd, precision, builder=DEV), create(K.with_positions(K.with_materials(sd, first, new), 1, pos), precision, builder=DEV)
    try:
        for step in ((0, 1) if materials_first else (1, 0)):
            if step == 0:
                a.set_materials(new, first)
            else:
                a.set_mesh_vertices({1: pos})
        assert_same_scene(a, b)
        assert D.MAT_MIRROR in tags_of(records(a)[0])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("materials_first", [True, False], ids=["materials-then-vertices", "vertices-then-materials"])
@pytest.mark.parametrize("precision", [F32, MIXED], ids=["f32", "mixed"])
def test_new_materials_and_a_moved_prototype_in_either_order(precision, materials_first):
    sd, first, new, kw, _ = MATERIAL_CASES["two-level"]
    pos = K.bent(sd.meshes[1].positions)  # (mesh 1: the prototype whose material becomes a mirror)
    a, b = create(sd, precision, builder=DEV), create(K.with_positions(K.with_materials(sd, first, new), 1, pos), precision, builder=DEV)
    try:
        for step in ((0, 1) if materials_first else (1, 0)):
            if step == 0:
                a.set_materials(new, first)
            else:
                a.update_meshes({1: pos})
        assert_same_scene(a, b, n_shapes=sd.n_shapes)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ lights
LIGHT_RUNS = [(n, p) for n in LIGHT_CASES for p in (F32, F64)] + [(n, MIXED) for n in ("65-triangles", "env", "dark")]


@pytest.mark.parametrize("name,precision", LIGHT_RUNS, ids=[f"{n}-{PID[p]}" for n, p in LIGHT_RUNS])
def test_new_intensities_leave_the_fresh_scene(name, precision):
    sd, first, rgb = LIGHT_CASES[name]
    a, b = create(sd, precision), create(K.with_intensities(sd, first, rgb), precision)
    try:
        before = tables(a)
        a.set_light_intensities(rgb, first)
        # integrator 3 picks lights by the power tables (it renders neither mixed-precision scenes nor environment maps);
        # NaN tables (a total power of 0) are dumped, not rendered with
        assert_same_scene(a, b, name, integrators=(0,) if name in ("dark", "env") or precision == MIXED else (0, 3))
        for got, old in zip(tables(a), before):
            lights = got["lights"]
            assert same_bytes(lights[:first], old["lights"][:first]) and same_bytes(lights[first + len(rgb):], old["lights"][first + len(rgb):])
            for f in ("kind", "shape_id", "is_sphere", "v", "n"):
                assert np.array_equal(lights[f], old["lights"][f]), f
            point = lights["kind"] == 0
            assert point.sum() == 1 and np.all(got["light_pmf"][point] == 0) or name == "dark"
            if name == "dark":
                assert np.isnan(got["light_pmf"]).all() and np.isnan(got["light_cdf"][1:]).all() and got["light_cdf"][0] == 0
            else:
                assert not same_bytes(got["light_pmf"], old["light_pmf"]) and got["light_cdf"][-1] > 0.999
        if name == "env":
            for side in SIDES[precision]:
                ea, eb = a.debug_env_tables(side), b.debug_env_tables(side)
                assert ea["scale"].tobytes() == eb["scale"].tobytes() and ea["intensity"].tobytes() == eb["intensity"].tobytes()
                assert np.array_equal(ea["scale"], np.asarray(rgb[-1], np.float32 if side == F32 else np.float64).astype(np.float64))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("precision", [F32, MIXED], ids=["f32", "mixed"])
def test_a_device_tensor_written_on_another_stream(precision):
    import torch

    sd, first, rgb = LIGHT_CASES["sub-range"]
    a, b = create(sd, precision), create(K.with_intensities(sd, first, rgb), precision)
    try:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # (the values are still being written on another stream when the call is made)
            t = torch.from_numpy(np.ascontiguousarray(rgb * 0.5)).cuda(non_blocking=True) * 2.0
            a.set_light_intensities(t, first)
        assert_same_scene(a, b, integrators=(0,) if precision == MIXED else (0, 3))
        with pytest.raises(ValueError):
            a.set_light_intensities(t.float(), first)
        with pytest.raises(ValueError):
            a.set_light_intensities(t[:, :2], first)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("precision", [F32, F64, MIXED], ids=["f32", "f64", "mixed"])
def test_there_and_back_gives_the_original_scene(precision):
    sd, first, rgb = LIGHT_CASES["env"]
    msd, mfirst, mnew, _, _ = MATERIAL_CASES["mirror"]
    a, m = create(sd, precision), create(msd, precision)
    try:
        original = snapshot(a)
        a.set_light_intensities(rgb, first)
        assert not np.array_equal(image(a), original[2])
        a.set_light_intensities([sd.lights[first + k].intensity for k in range(len(rgb))], first)
        assert_unchanged(a, original)
        original = snapshot(m)
        m.set_materials(mnew, mfirst)
        m.set_materials(msd.materials[mfirst:mfirst + len(mnew)], mfirst)
        assert_unchanged(m, original)
    finally:
        a.close()
        m.close()


# ------------------------------------------------------------------ the contract
def refused(call, match, code=D.TAKE_E_INVALID):
    with pytest.raises(capi.TakeError, match=match) as e:
        call()
    assert e.value.code == code


@pytest.mark.parametrize("precision", [F32, MIXED], ids=["f32", "mixed"])
def test_a_refused_call_leaves_the_scene_as_it_was(precision):
    sd = K.lit(5, env=True)
    sd.materials = [K.mat(D.MAT_DIFFUSE, K.COLOURS[3]), K.mat(D.MAT_DISNEY_METAL)]
    a = create(sd, precision, burley_lobes=True)
    try:
        snap = snapshot(a)
        good = K.mat(D.MAT_MIRROR)
        n_lights, n_images = len(sd.lights), len(sd.images)
        for call, match in ((lambda: a.set_materials([good, K.mat(99)]), "material 1: unknown tag"),
                            (lambda: a.set_materials([good, K.mat(-1)]), "material 1: unknown tag"),
                            (lambda: a.set_materials([K.mat(D.MAT_DIFFUSE, tex_image=n_images)], 1), "material 1: bad texture image id"),
                            (lambda: a.set_materials([good, K.mat(D.MAT_DISNEY_METAL, param=(1.5, 0.0))]), "material 1: Burley parameter"),
                            (lambda: a.set_materials([good, K.mat(D.MAT_DISNEY_GLASS, param=(0.5, 0.5, 0.0))]), "material 1: Burley parameter"),
                            (lambda: a.set_materials([good, good, good]), "outside the table"),
                            (lambda: a.set_materials([good], 2), "outside the table"),
                            (lambda: a.set_light_intensities(np.ones((n_lights + 1, 3))), "outside the table"),
                            (lambda: a.set_light_intensities(np.ones((1, 3)), n_lights), "outside the table"),
                            (lambda: a.set_light_intensities(np.array([[1.0, np.nan, 1.0]]), 2), "light 2: the intensity must be finite")):
            refused(call, match)
            assert_unchanged(a, snap, match)
        # creation refuses the same materials with the same messages
        bad = K.with_materials(sd, 1, [K.mat(D.MAT_DISNEY_METAL, param=(1.5, 0.0))])
        refused(lambda: create(bad, precision, burley_lobes=True), "material 1: Burley parameter")
    finally:
        a.close()
    plain = create(sd, F32)  # the same material in a scene created without burley_lobes: no Burley lobe, no range
    try:
        plain.set_materials([K.mat(D.MAT_DISNEY_METAL, param=(1.5, 0.0))], 1)
        assert list(plain.debug_shading_tables()["materials"]["tag"]) == [D.MAT_DIFFUSE, D.MAT_DISNEY_METAL]
    finally:
        plain.close()


@pytest.mark.parametrize("precision", [F32, MIXED], ids=["f32", "mixed"])
@pytest.mark.parametrize("what", ["materials", "intensities", "intensities-device"])
def test_a_failed_allocation_leaves_the_scene_as_it_was(precision, what, monkeypatch):
    """every device allocation of the call fails in turn (fault injection, TAKE_HIP_FAIL_ALLOC): TAKE_E_NOMEM, and the
    dumps and the render are what they were; then the call succeeds"""
    import torch

    if what == "materials":
        sd, first, new, kw, _ = MATERIAL_CASES["two-level"]
        call = lambda sc: sc.set_materials(new, first)
        edited, expected = K.with_materials(sd, first, new), 2  # per side: the table, the tags
    else:
        sd, first, rgb = LIGHT_CASES["env"]
        values = torch.from_numpy(np.ascontiguousarray(rgb)).cuda() if what.endswith("device") else rgb
        call = lambda sc: sc.set_light_intensities(values, first)
        edited, expected = K.with_intensities(sd, first, rgb), 4  # per side: the records, the powers, both tables
    shared = 1 if what == "intensities" else 0  # (the uploaded values)
    a, b = create(sd, precision), create(edited, precision)
    try:
        snap = snapshot(a)
        failed = 0
        for nth in range(1, 40):
            monkeypatch.setenv("TAKE_HIP_FAIL_ALLOC", str(nth))
            try:
                call(a)
                monkeypatch.delenv("TAKE_HIP_FAIL_ALLOC")
                break
            except capi.TakeError as e:
                monkeypatch.delenv("TAKE_HIP_FAIL_ALLOC")
                assert e.code == D.TAKE_E_NOMEM, str(e)
                failed += 1
                assert_unchanged(a, snap, nth)
        assert failed == shared + expected * len(SIDES[precision])
        assert_same_scene(a, b)
    finally:
        a.close()
        b.close()


def test_a_successful_call_ends_a_progressive_sequence():
    import torch

    sd, first, rgb = LIGHT_CASES["sub-range"]
    sc = create(sd, F32)
    try:
        out = torch.zeros((16, 16, 3), dtype=torch.float32, device="cuda")
        for good, bad in ((lambda: sc.set_light_intensities(rgb, first), lambda: sc.set_light_intensities(rgb, 1000)),
                          (lambda: sc.set_materials([K.mat(D.MAT_MIRROR)]), lambda: sc.set_materials([K.mat(99)]))):
            assert sc.render_accumulate(out.data_ptr(), 2, 4, seed=1, restart=True) == 2
            with pytest.raises(capi.TakeError):
                bad()
            assert capi.lib().take_hip_accumulated_samples(sc.h) == 2  # (a refused call changes nothing)
            assert sc.render_accumulate(out.data_ptr(), 2, 4, seed=1) == 4
            good()
            assert capi.lib().take_hip_accumulated_samples(sc.h) == 0
            with pytest.raises(capi.TakeError, match="restart"):
                sc.render_accumulate(out.data_ptr(), 2, 4, seed=1)
            assert sc.render_accumulate(out.data_ptr(), 2, 4, seed=1, restart=True) == 2
    finally:
        sc.close()

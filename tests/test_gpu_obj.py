"""Wavefront OBJ -> device mesh arrays on the GPU (take_hip_mesh_from_obj): the arrays the kernels write are
bit-identical to the `TriangleMesh` the reference's own parse_obj fills (tests/golden/obj), to the numpy restatement
(tests/obj_ref.py) on a generated file of about a million faces (quads, negative indices, repr() numbers that take the
host fix-up path), and a scene built from a device-decoded mesh renders the same image, bit for bit, as the scene built
from host arrays — on the host SAH builder and on the device LBVH builder.  Files the reference rejects, or would run
into undefined behaviour or std::terminate on, are refused."""
import copy
import os

import numpy as np
import pytest

import obj_ref
from take_amd import capi, scenes
from take_amd import cdefs as D
from test_obj_cpu import CASES, OBJ, load_case
from test_ply_cpu import assert_same_mesh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CASES)
def test_device_decode_is_bit_identical_to_the_reference_parser(name):
    data, xf, inv, ref = load_case(name)
    m = capi.DeviceMesh(data, material_id=2, to_world=xf, inv_to_world=inv, format="obj")
    try:
        assert (m.n_vertices, m.n_faces) == (ref["positions"].shape[0], ref["indices"].shape[0])
        got = m.download()
        assert got.material_id == 2
        assert_same_mesh(got, ref)
    finally:
        m.close()
    f = capi.DeviceMesh(os.path.join(OBJ, name + ".obj"), to_world=xf, inv_to_world=inv)  # (path: told by its suffix)
    try:
        assert_same_mesh(f.download(), ref)
    finally:
        f.close()


def big_obj(n_chunks, per_chunk, seed, fmt=repr):
    """~n_chunks * per_chunk * 2 faces: each chunk adds per_chunk v / vt / vn lines, then faces (a third of them quads)
    whose corners name any vertex so far, by a positive or a negative index"""
    rng = np.random.default_rng(seed)
    out = ["# generated"]
    nv = 0
    for _ in range(n_chunks):
        p = rng.uniform(-1, 1, (per_chunk, 3))
        t = rng.uniform(0, 1, (per_chunk, 2))
        n = rng.normal(size=(per_chunk, 3))
        out += [f"v {fmt(a)} {fmt(b)} {fmt(c)}" for a, b, c in p.tolist()]
        out += [f"vt {fmt(a)} {fmt(b)}" for a, b in t.tolist()]
        out += [f"vn {fmt(a)} {fmt(b)} {fmt(c)}" for a, b, c in n.tolist()]
        nv += per_chunk
        nf = 2 * per_chunk
        quad = rng.random(nf) < 1 / 3
        j = rng.integers(0, nv, (nf, 4))
        neg = rng.random((nf, 4)) < 0.3
        # v and vn: j + 1 or j - nv; vt: j + 1 or j + 1 - nv (pool + vt - 1 = j), only where that is negative
        vi = np.where(neg, j - nv, j + 1)
        ti = np.where(neg & (j < nv - 1), j + 1 - nv, j + 1)
        for f in range(nf):
            k = 4 if quad[f] else 3
            out.append("f " + " ".join(f"{vi[f, c]}/{ti[f, c]}/{vi[f, c]}" for c in range(k)))
    return ("\n".join(out) + "\n").encode()


@pytest.fixture(scope="module")
def million():
    data = big_obj(100, 3_400, 11)  # ~680k faces + ~227k quads -> ~907k triangles, ~1.02M face lines incl. pools
    xf = np.array([[0.6, -0.8, 0.0, 1.0], [0.8, 0.6, 0.0, -2.0], [0.0, 0.0, 1.7, 0.5], [0.0, 0.0, 0.0, 1.0]])
    inv = np.linalg.inv(xf)
    return data, xf, inv, obj_ref.parse_obj(data, xf, inv)


def test_million_face_file_matches_the_restatement_bit_for_bit(million):
    data, xf, inv, want = million
    assert want["indices"].shape[0] > 800_000
    for _ in range(2):  # (and a second decode of the same file: the dedup is deterministic)
        m = capi.DeviceMesh(data, to_world=xf, inv_to_world=inv, format="obj")
        try:
            assert_same_mesh(m.download(), want)
        finally:
            m.close()


def test_fixed_point_file_from_disk_matches(tmp_path):
    data = big_obj(20, 2_000, 12, fmt=lambda x: f"{x:.6f}")
    path = tmp_path / "mesh.OBJ"
    path.write_bytes(data)
    m = capi.DeviceMesh(str(path))
    try:
        assert_same_mesh(m.download(), obj_ref.parse_obj(data))
    finally:
        m.close()


def soup_obj(positions, indices):
    """the mesh as OBJ text: repr() positions (exact round trip), 1-based triangles"""
    lines = [f"v {x!r} {y!r} {z!r}" for x, y, z in positions.tolist()]
    lines += [f"f {a + 1} {b + 1} {c + 1}" for a, b, c in indices.tolist()]
    return ("\n".join(lines) + "\n").encode()


@pytest.mark.parametrize("builder,precision", [(D.TAKE_BUILDER_HOST_SAH, D.TAKE_PRECISION_F32), (D.TAKE_BUILDER_DEVICE_LBVH, D.TAKE_PRECISION_F32),
                                               (D.TAKE_BUILDER_HOST_SAH, D.TAKE_PRECISION_F64), (D.TAKE_BUILDER_AUTO, D.TAKE_PRECISION_MIXED)])
def test_scene_from_a_device_decoded_mesh_renders_the_same_image(builder, precision, tmp_path):
    """configs[1]'s soup written as an OBJ file, decoded on the device and rendered, against the same scene from the
    host arrays the restatement of parse_obj makes of that file"""
    sd = scenes.soup_scene(20_000, 96, 64, spp=4)
    soup = max(range(len(sd.meshes)), key=lambda i: sd.meshes[i].indices.shape[0])
    host = sd.meshes[soup]
    data = soup_obj(host.positions, host.indices)
    path = tmp_path / "soup.obj"
    path.write_bytes(data)
    ref = obj_ref.parse_obj(data)
    sd_host = copy.copy(sd)
    sd_host.meshes = list(sd.meshes)
    sd_host.meshes[soup] = type(host)(ref["positions"], ref["indices"], host.material_id, None, None)
    dm = capi.DeviceMesh(str(path), material_id=host.material_id)
    assert_same_mesh(dm.download(), ref)
    sd_dev = copy.copy(sd)
    sd_dev.meshes = list(sd.meshes)
    sd_dev.meshes[soup] = dm
    a = capi.Scene(sd_host, precision=precision, builder=builder)
    b = capi.Scene(sd_dev, precision=precision, builder=builder)
    try:
        assert a.stats() == b.stats()
        ia, ib = a.render(spp=4, max_depth=8, seed=3), b.render(spp=4, max_depth=8, seed=3)
        assert np.array_equal(ia, ib) and ia.mean() > 0.01
    finally:
        a.close(), b.close(), dm.close()


V3 = b"v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nv 2 2 2\n"


@pytest.mark.parametrize("text,msg", [
    (V3 + b"f 1 2 3 4 5\n", "n-gon (n>4)"),
    (V3 + b"f 1 0 2\n", "vertex index 0"),
    (b"v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n", "outside its pool"),  # (3 exists only after the face line)
    (V3 + b"f -6 1 2\n", "outside its pool"),
    (V3 + b"vt 0 0\nf 1/2 2/1 3/1\n", "outside its pool"),
    (V3 + b"vt 0 0\nf 1/-1 2/-1 3/-1\n", "outside its pool"),  # (negative vt: pool + vt - 1 = -1)
    (V3 + b"f 1 2\n", "fewer than 3 corners"),
    (V3 + b"f\n", "fewer than 3 corners"),
])
def test_invalid_files_are_refused(text, msg):
    with pytest.raises(capi.TakeError) as e:
        capi.DeviceMesh(text, format="obj")
    assert e.value.code == D.TAKE_E_INVALID and msg in str(e.value) and not str(e.value).split(": ", 1)[1].startswith("unsupported")


@pytest.mark.parametrize("text", [
    V3 + b"f 1 2 3 # c\n",  # std::stoi("#") throws
    V3 + b"f 1 2 x\n",
    V3 + b"f 1/2/3/q 2 3\n",  # (a fourth piece is converted too)
    V3 + b"f 1 2 99999999999\n",  # std::stoi out of range
    V3 + b"vt 0 0\nf 1/1 2 3\n",  # only some vertices have a uv
    V3 + b"vn 0 0 1\nf 1//1 2//1 3\n",
    b"v 0 0 0\nv 1 0 nan\nv 0 1 0\nf 1 2 3\n",
    b"v 0 0 0\nv 1 0 1e999\nv 0 1 0\nf 1 2 3\n",  # (host fix-up path: out of range)
    b"v 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
    b"v 0 0 0 w\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
])
def test_unsupported_files_say_so(text):
    with pytest.raises(capi.TakeError) as e:
        capi.DeviceMesh(text, format="obj")
    assert e.value.code == D.TAKE_E_INVALID and str(e.value).split(": ", 1)[1].startswith("unsupported"), str(e.value)


def test_errors_in_a_large_file_report_the_earliest_line():
    base = big_obj(4, 2_000, 13, fmt=lambda x: f"{x:.6f}").split(b"\n")
    for bad, msg in ((b"f 1 2 3 4 5", "n-gon"), (b"f 1 2 3 #", "unsupported"), (b"f 1 2 999999", "outside its pool")):
        lines = list(base)
        at = len(lines) // 2
        lines.insert(at, bad)
        lines.insert(at + 10, b"f 1 2 0")  # (a later error does not win)
        with pytest.raises(capi.TakeError) as e:
            capi.DeviceMesh(b"\n".join(lines), format="obj")
        assert msg in str(e.value) and f"line {at + 1}:" in str(e.value), str(e.value)


def test_empty_and_face_free_files():
    for text in (b"", b"# nothing\n", b"v 1 2 3\nv 4 5 6\n"):
        m = capi.DeviceMesh(text, format="obj")
        assert (m.n_vertices, m.n_faces) == (0, 0)
        got = m.download()
        assert got.positions.shape == (0, 3) and got.indices.shape == (0, 3) and got.normals is None and got.uvs is None
        m.close()

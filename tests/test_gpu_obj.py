"""Wavefront OBJ -> device mesh arrays on the GPU (take_hip_mesh_from_obj): the arrays the kernels write are
bit-identical to the `TriangleMesh` the reference's own parse_obj fills (tests/golden/obj), to the numpy restatement
(tests/obj_ref.py) on a generated file of about a million faces (quads, negative indices, repr() numbers that take the
host fix-up path), and a scene built from a device-decoded mesh renders the same image, bit for bit, as the scene built
from host arrays — on the host SAH builder and on the device LBVH builder.  Files the reference rejects, or would run
into undefined behaviour or std::terminate on, are refused.  The second half aims at the decode's edges
(tests/obj_numbers.py): the boundary of the window in which the device converts a number itself, files of exactly k * 4096
bytes, lines and corners (the scans' tiles), the dedup table's smallest sizes and heaviest contention, and two problems
found by different stages of the decode (the earliest line wins)."""
import copy
import os

import numpy as np
import pytest

import obj_numbers
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


# ---- the decode at its edges: the number window, the 4096-element scan tiles, the dedup table, the status word -------
AFFINE = np.array([[0.6, -0.8, 0.0, 1.0], [0.8, 0.6, 0.0, -2.0], [0.0, 0.0, 1.7, 0.5], [0.0, 0.0, 0.0, 1.0]])
TRI = [b"v 0 0 0", b"v 1 0 0", b"v 0 1 0", b"f 1 2 3"]
KIND = {obj_ref.FEW: "fewer than 3 corners", obj_ref.V0: "vertex index 0", obj_ref.RANGE: "outside its pool", obj_ref.NGON: "n-gon (n>4)"}


def decode(data, xf=None, inv=None):
    m = capi.DeviceMesh(data, to_world=xf, inv_to_world=inv, format="obj")
    try:
        return m.download()
    finally:
        m.close()


def assert_decodes_like_the_restatement(data, xf=None, inv=None):
    """two decodes of the file, both bit-identical to obj_ref.parse_obj's arrays -> those arrays"""
    want = obj_ref.parse_obj(data, xf, inv)
    for _ in range(2):
        assert_same_mesh(decode(data, xf, inv), want)
    return want


def assert_refused_like_the_restatement(data):
    """the decode refuses the file with the line and the kind of message of the restatement's ObjError -> that error"""
    with pytest.raises(obj_ref.ObjError) as want:
        obj_ref.parse_obj(data)
    with pytest.raises(capi.TakeError) as e:
        capi.DeviceMesh(data, format="obj")
    msg = str(e.value).split(": ", 1)[1]
    assert e.value.code == D.TAKE_E_INVALID, msg
    assert f"OBJ line {want.value.line + 1}:" in msg, (msg, want.value.line + 1)
    assert msg.startswith("unsupported") == want.value.unsupported, (msg, want.value.code)
    if not want.value.unsupported:
        assert KIND[want.value.code] in msg, (msg, want.value.code)
    return want.value


@pytest.fixture(scope="module")
def grammar_tokens():
    return obj_numbers.number_tokens(30_000) + obj_numbers.CURATED


def test_number_grammar_through_vt_keeps_every_bit(grammar_tokens):
    """every token as a vt's first coordinate, which the decode copies: uv[k, 0] is float(token k), signed zeros included"""
    toks = grammar_tokens
    n = len(toks)
    lines = list(TRI[:3]) + [b"vt " + toks[k] + b" " + toks[(k + 1) % n] for k in range(n)]
    lines += [b"f " + b" ".join(b"%d/%d" % (j % n % 3 + 1, j % n + 1) for j in (k, k + 1, k + 2)) for k in range(0, n, 3)]
    data = b"\n".join(lines) + b"\n"
    want = assert_decodes_like_the_restatement(data, AFFINE, np.linalg.inv(AFFINE))
    assert want["uvs"].shape == (n, 2)
    assert np.array_equal(want["uvs"][:, 0].view(np.uint64), np.array([float(t) for t in toks]).view(np.uint64))
    uv = decode(data).uvs
    at = {t: k for k, t in enumerate(toks)}
    for t in obj_numbers.NEGATIVE_ZEROS:
        assert uv[at[t], 0] == 0 and np.signbit(uv[at[t], 0]), t
    for t in obj_numbers.POSITIVE_ZEROS:
        assert uv[at[t], 0] == 0 and not np.signbit(uv[at[t], 0]), t


def test_number_grammar_through_v_w_and_vn(grammar_tokens):
    """every token as a coordinate of a v (every other one with a w) and of a vn, under an affine to_world.  Left out:
    magnitudes whose squares or quotients leave the range of a double (the two ends of the range in the curated list), a
    zero as w — they make NaNs, whose bits the arrays are not compared on"""
    vals = [float(t) for t in grammar_tokens]
    safe = [t for t, x in zip(grammar_tokens, vals) if x == 0 or 1e-150 < abs(x) < 1e150]
    w = [t for t in safe if float(t) != 0]
    assert len(safe) > len(grammar_tokens) - 10 and len(w) > len(safe) - 40
    n = len(safe) // 3
    lines = [b"v " + b" ".join(safe[3 * i:3 * i + 3]) + (b" " + w[i] if i % 2 else b"") for i in range(n)]
    lines += [b"vn " + b" ".join(safe[3 * i:3 * i + 3]) for i in range(n)]
    lines += [b"f " + b" ".join(b"%d//%d" % (j % n + 1, j % n + 1) for j in (i, i + 1, i + 2)) for i in range(0, n, 3)]
    want = assert_decodes_like_the_restatement(b"\n".join(lines) + b"\n", AFFINE, np.linalg.inv(AFFINE))
    assert want["positions"].shape == (n, 3) and np.isfinite(want["positions"]).all() and np.isfinite(want["normals"]).all()


@pytest.mark.parametrize("where", ["first_line", "last_line_without_newline", "line_4097"])
def test_refused_number_tokens_are_unsupported_on_their_line(where):
    for tok in obj_numbers.REFUSED:
        if where == "first_line":
            data, line = b"\n".join([b"v " + tok + b" 0 0"] + TRI) + b"\n", 0
        elif where == "last_line_without_newline":
            data, line = b"\n".join(TRI + [b"vn 0 0 " + tok]), len(TRI)
        else:  # just behind the first 256-line block of the second 4096-line tile
            data, line = obj_numbers.place_lines({0: TRI[0], 1: TRI[1], 2: TRI[2], 3: TRI[3], 4097: b"vt 1 " + tok, 4300: TRI[3]}, 4400), 4097
        err = assert_refused_like_the_restatement(data)
        assert err.unsupported and err.line == line, (tok, err.line)


def tile_face_lines(start, tag):
    """a v, a vt and a face whose negative indices name them, at lines start, start + 1, start + 2"""
    return {start: b"v %d.5 %d 1" % (tag, start), start + 1: b"vt 0.%d 0.25" % tag, start + 2: b"f -1/-1 -2/-1 -3/-2"}


@pytest.mark.parametrize("total", [4095, 4096, 4097, 8192, 8193])
@pytest.mark.parametrize("newline", [True, False])
def test_files_of_a_whole_number_of_byte_tiles(total, newline):
    lines = TRI[:3] + [b"vt 0 0", b"vt 1 0", b"vt 0.5 1", b"f 1/1 2/2 3/3", b"v 2 2 2", b"f -1/-1 -2/-2 4/3"]
    data = obj_numbers.pad_to_bytes(lines, total, newline, at=7)
    assert len(data) == total and data.endswith(b"\n") == newline
    want = assert_decodes_like_the_restatement(data)
    assert want["indices"].shape == (2, 3)


def test_newlines_on_both_sides_of_a_byte_tile_edge():
    head = obj_numbers.pad_to_bytes([b"v 0 0 0", b"v 1 0 0"], 4095, trailing_newline=False)
    data = head + b"\n\n" + b"\n".join([b"v 0 1 0", b"f 1 2 3", b"f -1 -2 -3"]) + b"\n"
    assert data[4095:4097] == b"\n\n" and data[4088:4095] == b"v 1 0 0" and data[4097:4098] == b"v"
    assert_decodes_like_the_restatement(data)
    # and the edge inside a number, inside a keyword, between a '\r' and its '\n'
    for cut in (b"v 0.12345678901234567 1 0", b"vt 0.5 0.5", b"v 1 1 1\r"):
        for k in range(1, len(cut)):
            head = obj_numbers.pad_to_bytes([b"v 0 0 0", b"v 1 0 0", b"v 2 0 0", b"vt 0 0", b"vt 1 1", b"vt 1 0", cut], 4096 + len(cut) - k, trailing_newline=False)
            data = head + b"\n" + b"\n".join([b"v 0 1 0", b"vt 0 1", b"f 1/1 2/2 3/3", b"f -1/-1 -2/-2 -3/-3"]) + b"\n"
            assert data[4096 - k:4096 - k + len(cut)] == cut
            assert_same_mesh(decode(data), obj_ref.parse_obj(data))


@pytest.mark.parametrize("nlines", [4095, 4096, 4097, 8192, 8193])
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_files_of_a_whole_number_of_line_tiles(nlines, shift):
    """a face at, just in front of and just behind a line-tile edge: its pool sizes are the scan's carry"""
    placed = {0: TRI[0], 1: TRI[1], 2: TRI[2], 3: b"vt 0 0", 4: b"vt 1 0", 5: b"vt 0 1"}
    starts = [s for s in (4095 - shift, 8191 - shift, nlines - 3) if s + 2 < nlines]
    for tag, s in enumerate(sorted(set(starts))):
        if not any(abs(s - o) < 3 for o in starts if o < s):
            placed.update(tile_face_lines(s, tag + 1))
    data = obj_numbers.place_lines(placed, nlines)
    assert data.count(b"\n") == nlines - 1 and data.count(b"\nf ") >= 1
    want = assert_decodes_like_the_restatement(data)
    assert want["indices"].shape[0] == data.count(b"\nf ")
    assert_decodes_like_the_restatement(data + b"\n")  # (one more, empty, line)


def corner_file(ncorners, nverts, same_at=None):
    """exactly ncorners face corners, triangles and as many quads as it takes; corner i names vertex 19 i mod nverts, except
    that corner same_at + 1 repeats corner same_at's key"""
    v = [(19 * i) % nverts + 1 for i in range(ncorners)]
    if same_at is not None:
        v[same_at + 1] = v[same_at]
    nquad = ncorners % 3
    sizes = [4] * nquad + [3] * ((ncorners - 4 * nquad) // 3)
    assert sum(sizes) == ncorners and min(sizes) >= 3
    lines = [b"v %d %d.25 -%d" % (i, i % 7, i % 3) for i in range(nverts)] + [b"vt 0.5 0.5", b"vn 0 0 1"]
    c = 0
    for s in sizes:
        lines.append(b"f " + b" ".join(b"%d/1/1" % v[c + j] for j in range(s)))
        c += s
    return b"\n".join(lines) + b"\n", v


@pytest.mark.parametrize("ncorners", [4095, 4096, 4097, 8192, 8193])
@pytest.mark.parametrize("same", [True, False])
def test_files_of_a_whole_number_of_corner_tiles(ncorners, same):
    at = min(4095, ncorners - 2)
    data, v = corner_file(ncorners, 1000, at if same else None)
    assert (v[at] == v[at + 1]) == same
    want = assert_decodes_like_the_restatement(data)
    assert want["positions"].shape[0] == 1000
    data, v = corner_file(ncorners, ncorners, at if same else None)  # every corner its own vertex (but the repeated one)
    want = assert_decodes_like_the_restatement(data)
    assert want["positions"].shape[0] == ncorners - same


@pytest.mark.parametrize("ncorners", [32, 33, 64, 65])
def test_dedup_table_at_its_smallest_sizes(ncorners):
    """64 slots up to 32 corners, 128 from 33, 256 from 65"""
    for nverts in (ncorners, 5, 1):
        want = assert_decodes_like_the_restatement(corner_file(ncorners, nverts)[0])
        assert want["positions"].shape[0] == nverts


def test_dedup_of_one_key_and_of_all_distinct_keys():
    n = 2000
    head = [b"v 1 2 3", b"vt 0.25 0.75", b"vn 0 1 0"]
    want = assert_decodes_like_the_restatement(b"\n".join(head + [b"f 1/1/1 1/1/1 1/1/1"] * n) + b"\n")
    assert want["positions"].shape == (1, 3) and np.all(want["indices"] == 0) and want["indices"].shape == (n, 3)
    # one position, 3 n keys: the same corners told apart by their vt alone
    lines = head[:1] + [b"vt 0.%04d 0.5" % k for k in range(3 * n)] + head[2:]
    lines += [b"f 1/%d/1 1/%d/1 1/%d/1" % (3 * k + 1, 3 * k + 2, 3 * k + 3) for k in range(n)]
    want = assert_decodes_like_the_restatement(b"\n".join(lines) + b"\n")
    assert want["positions"].shape == (3 * n, 3) and np.array_equal(want["indices"].reshape(-1), np.arange(3 * n))
    # 3 n positions
    lines = [b"v %d 0.5 %d" % (k, k % 11) for k in range(3 * n)] + [b"f %d %d %d" % (3 * k + 1, 3 * k + 2, 3 * k + 3) for k in range(n)]
    want = assert_decodes_like_the_restatement(b"\n".join(lines) + b"\n")
    assert want["positions"].shape == (3 * n, 3)


def test_dedup_keys_that_differ_in_one_index_only():
    pools = [b"v %d 0 0" % k for k in range(5)] + [b"vt 0.1 0.2", b"vt 0.3 0.4", b"vn 0 0 1", b"vn 0 1 0"]
    for faces, nvert in (([b"f 1/1/1 2/1/1 1/1/1", b"f 2/1/1 1/1/1 2/1/1"], 2), ([b"f 1/1/1 1/2/1 1/1/1", b"f 1/2/1 1/1/1 1/2/1"], 2),
                         ([b"f 1/1/1 1/1/2 1/1/1", b"f 1/1/2 1/1/1 1/1/2"], 2), ([b"f 1/1/1 2/1/1 1/2/1 1/1/2", b"f 1/1/2 1/2/1 2/1/1"], 4),
                         # the same pool entries under two names are two vertices: the key is the raw triple
                         ([b"f 5/2/2 -1/2/2 1/2/2", b"f -1/2/2 5/2/2 -5/2/2"], 4), ([b"f 1/2/2 1/-1/2 1/2/-1"], 3)):
        want = assert_decodes_like_the_restatement(b"\n".join(pools + faces) + b"\n")
        assert want["positions"].shape[0] == nvert, faces
    want = obj_ref.parse_obj(b"\n".join(pools + [b"f 5/2/2 -1/2/2 1/2/2"]) + b"\n")
    assert np.array_equal(want["positions"][0], want["positions"][1]) and not np.array_equal(want["indices"][0, 0], want["indices"][0, 1])


FEW, THROW, NGON, HOST_RANGE, INDEX0, POOL, BAD_V = (b"f 1 2", b"f 1 2 x", b"f 1 2 3 1 2", b"v 1e999 0 0", b"f 1 0 2", b"f 1 2 99", b"v 1 x 0")


@pytest.mark.parametrize("a,b", [(FEW, THROW), (THROW, NGON), (HOST_RANGE, INDEX0), (POOL, BAD_V)])
@pytest.mark.parametrize("i,j", [(10, 11), (10, 200), (100, 300), (255, 256), (100, 5000), (4095, 4096)])
def test_the_earliest_problem_line_wins(a, b, i, j):
    """two problems found by different stages (the parse kernel, the host's strtod, the emit kernel), within one 256-line
    block, in two blocks, in two 4096-line tiles, in both orders"""
    for first, second in ((a, b), (b, a)):
        data = obj_numbers.place_lines({0: TRI[0], 1: TRI[1], 2: TRI[2], i: first, j: second}, 5200)
        err = assert_refused_like_the_restatement(data)
        assert err.line == i, (first, second, err.line)


@pytest.mark.parametrize("line,code", [(b"f 1 x", obj_ref.UNSUPPORTED), (b"f x", obj_ref.UNSUPPORTED), (b"f 1 2 x 4 5", obj_ref.UNSUPPORTED),
                                       (b"f 1 2 3 4 x", obj_ref.NGON), (b"f 1 0", obj_ref.FEW), (b"f 1 0 99", obj_ref.V0),
                                       (b"f 1 0 3 4 5", obj_ref.NGON), (b"f 1 2 99 0", obj_ref.V0), (b"f 1 2 x 0", obj_ref.UNSUPPORTED)])
def test_two_problems_on_one_line(line, code):
    """std::stoi runs on the first four corners before the corner count is looked at; index 0 is found before a pool's end"""
    for at in (3, 4096):
        err = assert_refused_like_the_restatement(obj_numbers.place_lines({0: TRI[0], 1: TRI[1], 2: TRI[2], at: line}, at + 2))
        assert (err.line, err.code) == (at, code)


def test_a_host_found_number_next_to_a_device_found_problem():
    """the host's strtod finds `1e999`, the parse kernel `x`: the same line is unsupported once, neighbours in file order"""
    for lines, line in (([b"v 1e999 x 0"], 3), ([b"v x 1e999 0"], 3), ([b"v 1e999 0 0", b"v 0 x 0"], 3), ([b"v 0 x 0", b"v 1e999 0 0"], 3),
                        ([b"f 1 0 2", b"v 1e999 0 0"], 3), ([b"v 1e999 0 0", b"f 1 0 2"], 3), ([b"f 1 2 3 4 5", b"v 0 0 1e-999"], 3),
                        ([b"v 0 0 1e-999", b"f 1 2 3 4 5"], 3)):
        err = assert_refused_like_the_restatement(b"\n".join(TRI[:3] + lines + [TRI[3]]) + b"\n")
        assert err.line == line, lines

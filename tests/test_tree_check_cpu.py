"""The structural validator (tests/tree_check.py) on trees the HOST builder makes (tests/hostsim: prepare_scene<R>, the
layout of take_hip_debug_tree), and the controls that prove it bites: seven deliberate faults, each applied to a copy
of a passing tree, each reported in its category with the count an independent rational-arithmetic walk predicts.
tests/test_gpu_tree_check.py runs the same validator on what the device builder leaves in device memory."""
import time
from fractions import Fraction as Fr
from functools import lru_cache

import numpy as np
import pytest

import tree_check as T
from helpers import GOLDEN_SCENES, golden_scene, hostsim_debug_tree, sheared_placements
from take_amd import scenes

F32, F64 = 0, 1


@lru_cache(maxsize=None)
def scene(name):
    if name in GOLDEN_SCENES:
        return golden_scene(name)
    return {"soup20k": lambda: scenes.soup_scene(20_000, 32, 32, 1),
            "soup100k": lambda: scenes.soup_scene(100_000, 32, 32, 1),
            "instanced": lambda: scenes.instanced_scene(12, 300, 32, 32, 1),
            "sheared": sheared_placements}[name]()


def host_tree(name, precision, leaf, fmt, monkeypatch):
    if fmt:
        monkeypatch.setenv("TAKE_HIP_NODES", fmt)
    else:
        monkeypatch.delenv("TAKE_HIP_NODES", raising=False)
    monkeypatch.delenv("TAKE_HIP_BRAID", raising=False)
    return hostsim_debug_tree(scene(name), precision, leaf)


def check(tree, name, leaf, xforms=None, **kw):
    sd = scene(name)
    if xforms is None and sd.instance_mesh:
        xforms = np.array(sd.instance_xform)
    return T.check_tree(tree, leaf, n_shapes=sd.n_shapes, xforms=xforms, **kw)


def mutable(tree):
    out = dict(tree)
    for k in ("nodes", "prims", "inst_trace"):
        out[k] = tree[k].copy()
    return out


def only(result, **want):
    """every error count is 0 but the named ones, which are as given"""
    expect = {k: 0 for k in T.ERROR_CATEGORIES}
    expect.update(want)
    assert result["errors"] == expect, (result["errors"], result["where"])


# ------------------------------------------------------------------ host-built trees pass
@pytest.mark.parametrize("fmt", ["", "wide", "q8"])
@pytest.mark.parametrize("leaf", [1, 2, 4])
@pytest.mark.parametrize("precision", [F32, F64])
@pytest.mark.parametrize("name", GOLDEN_SCENES + ["soup20k", "instanced", "sheared"])
def test_host_built_trees_pass(name, precision, leaf, fmt, monkeypatch):
    """every category 0, and the measured depth is the one the scene reports, for compressed 4-wide nodes, full-width
    nodes (where no delta hides a sliver) and the 8-wide tree (same slot layout, node_width 8)"""
    tree = host_tree(name, precision, leaf, fmt, monkeypatch)
    assert tree["node_format"] == {"": 1, "wide": 0, "q8": 2}[fmt] and tree["node_width"] == (8 if fmt == "q8" else 4)
    r = check(tree, name, leaf, expected_depth=tree["depth"])
    only(r)
    assert r["diag"]["slots"] > 0 and r["diag"]["min_margin_lo"] >= 0 and r["diag"]["min_margin_hi"] >= 0


def test_100k_primitives_in_a_few_seconds(monkeypatch):
    """the numpy walk over a 100 000-triangle tree (95 249 child boxes, 11 levels): 0.44 s measured on one
    CPU core, f32 and f64 alike; held to 5 s"""
    tree = host_tree("soup100k", F32, 2, "", monkeypatch)
    t0 = time.perf_counter()
    r = check(tree, "soup100k", 2, expected_depth=tree["depth"])
    dt = time.perf_counter() - t0
    print(f"\nvalidator on {tree['n_prims']} primitives, {tree['n_nodes']} nodes: {dt:.2f} s")
    only(r)
    assert dt < 5.0, dt


# ------------------------------------------------------------------ an independent, scalar, rational walk for the controls
def path_slots(tree, prim):
    """the (node, slot) chain from the leaf slot that holds record `prim` up to the root"""
    child = tree["nodes"]["c"]["child"].astype(np.int64)
    leaf = (child < 0) & (child >= -(1 << 30))
    first, count = (-child - 1) // 4, (-child - 1) % 4 + 1
    hit = np.argwhere(leaf & (first <= prim) & (prim < first + count))
    assert hit.shape[0] == 1
    chain = [tuple(int(x) for x in hit[0])]
    while chain[-1][0] != tree["root_child"]:
        up = np.argwhere(child == chain[-1][0])
        assert up.shape[0] == 1
        chain.append(tuple(int(x) for x in up[0]))
    return chain


def exact_extent(rec):
    a = [Fr(float(x)) for x in rec["a"]]
    if (int(rec["meta"]) & 0xff) == 1:
        return [a[k] - a[3] for k in range(3)], [a[k] + a[3] for k in range(3)]
    pts = [[a[k], a[k] + a[3 + k], a[k] + a[6 + k]] for k in range(3)]
    return [min(p) for p in pts], [max(p) for p in pts]


def slot_contains(tree, node, slot, lo, hi):
    c = tree["nodes"]["c"][node][slot]
    if tree["node_format"] == 0:
        return all(Fr(float(c["bmin"][k])) <= lo[k] and hi[k] <= Fr(float(c["bmax"][k])) for k in range(3))
    ok = True
    for k in range(3):
        g, st = Fr(float(np.float32(tree["grid_lo"][k]))), Fr(float(np.float32(tree["grid_step"][k])))
        d = T.Q_MAX * st / (1 << 20)
        ql, qh = int(c["q"][k]) & 0xffff, int(c["q"][k]) >> 16
        ok = ok and g + (T.Q_BIAS + ql) * st + d <= lo[k] and hi[k] <= g + (T.Q_BIAS + qh) * st - d
    return ok


# ------------------------------------------------------------------ the seven controls
def test_control_1_a_compressed_plane_one_cell_too_high(monkeypatch):
    tree = mutable(host_tree("soup20k", F32, 2, "", monkeypatch))
    base = check(tree, "soup20k", 2)
    only(base)
    node, slot, axis = base["diag"]["min_margin_lo_at"]
    assert 0 <= base["diag"]["min_margin_lo"] < 1  # the content is within a cell of this plane
    q = tree["nodes"]["c"]["q"]
    assert (int(q[node, slot, axis]) & 0xffff) + 1 < int(q[node, slot, axis]) >> 16
    q[node, slot, axis] += 1  # lo is the low half
    only(check(tree, "soup20k", 2), containment=1)


def test_control_2_a_full_width_plane_one_ulp_too_high(monkeypatch):
    """on the slot with the smallest margin: for the host builder that is 0 float ulps (a plane that is a vertex), so the
    next float up leaves the vertex outside"""
    tree = mutable(host_tree("soup20k", F32, 2, "wide", monkeypatch))
    base = check(tree, "soup20k", 2)
    only(base)
    node, slot, axis = base["diag"]["min_margin_lo_at"]
    assert 0 <= base["diag"]["min_margin_lo"] < 1
    b = tree["nodes"]["c"]["bmin"]
    b[node, slot, axis] = np.nextafter(b[node, slot, axis], np.float32(np.inf))
    only(check(tree, "soup20k", 2), containment=1)


@pytest.mark.parametrize("fmt", ["", "wide"])
def test_control_3_two_primitives_exchanged_between_distant_leaves(fmt, monkeypatch):
    tree = mutable(host_tree("soup20k", F32, 2, fmt, monkeypatch))
    i, j = 17, tree["n_prims"] - 23  # leaf order: the two ends of the tree
    want = 0
    for p, other in ((i, j), (j, i)):
        lo, hi = exact_extent(tree["prims"][other])
        want += sum(not slot_contains(tree, n, s, lo, hi) for n, s in path_slots(tree, p))
    assert want >= 2
    tree["prims"][[i, j]] = tree["prims"][[j, i]]
    only(check(tree, "soup20k", 2), containment=want)


def test_control_4_a_leaf_one_primitive_short(monkeypatch):
    tree = mutable(host_tree("soup20k", F32, 4, "", monkeypatch))
    child = tree["nodes"]["c"]["child"]
    leaf = (child < 0) & (child >= -(1 << 30))
    count = (-child.astype(np.int64) - 1) % 4 + 1
    node, slot = np.argwhere(leaf & (count >= 2))[5]
    child[node, slot] += 1  # make_leaf(first, count - 1)
    only(check(tree, "soup20k", 4), partition=1)


def test_control_5_a_child_word_redirected_to_a_visited_node(monkeypatch):
    tree = mutable(host_tree("soup20k", F32, 2, "", monkeypatch))
    child = tree["nodes"]["c"]["child"]
    leaf = (child < 0) & (child >= -(1 << 30))
    interior = child >= 0
    leaves_only = ~interior.any(1)                      # nodes with no interior child
    target = np.where(interior, leaves_only[np.where(interior, child, 0)], False)
    node, slot = np.argwhere(target)[3]
    lost = int(child[node, slot])
    n_lost = int(((-child[lost].astype(np.int64) - 1) % 4 + 1)[leaf[lost]].sum())
    child[node, slot] = 0  # the root: visited first
    only(check(tree, "soup20k", 2), reached_twice=1, unreached=1, partition=n_lost)


def test_control_6_an_f64_sphere_one_ulp_larger(monkeypatch):
    """a double record: c +- r is not a double, the comparison with the plane is decided by the residual of TwoSum"""
    tree = mutable(host_tree("mats", F64, 1, "wide", monkeypatch))
    only(check(tree, "mats", 1))
    prims = tree["prims"]
    spheres = np.nonzero((prims["meta"] & 0xff) == 1)[0]
    assert spheres.size
    for p in spheres:
        grown = prims[p].copy()
        grown["a"][3] = np.nextafter(grown["a"][3], np.inf)
        lo, hi = exact_extent(grown)
        want = sum(not slot_contains(tree, n, s, lo, hi) for n, s in path_slots(tree, int(p)))
        if want:
            break
    assert want >= 1  # (some sphere's box is tight to the ulp)
    prims[p] = grown
    only(check(tree, "mats", 1), containment=want)


@pytest.mark.parametrize("precision", [F32, F64])
def test_control_7_a_placement_moved_by_1e_5_of_its_extent(precision, monkeypatch):
    """full-width nodes: the float box of a placement is its tight box + the builder's pad (4e-6 / 1e-13 of the
    magnitude) + at most a float; on the compressed grid a cell of the whole scene would hide the move"""
    tree = host_tree("sheared", precision, 2, "wide", monkeypatch)
    sd = scene("sheared")
    x = np.array(sd.instance_xform)
    only(check(tree, "sheared", 2, xforms=x))
    # the placement whose box is largest against its distance from the origin, so that the move beats the pad
    best, ratio = None, 0.0
    for i, (m, mesh) in enumerate(zip(x, sd.instance_mesh)):
        w = sd.meshes[mesh].positions @ m[:, :3].T + m[:, 3]
        ext, mag = (w.max(0) - w.min(0)).max(), np.abs(w).max()
        if ext / mag > ratio:
            best, ratio, extent = i, ext / mag, ext
    assert 1e-5 * ratio > 2 * 4e-6
    x[best, 0, 3] += 1e-5 * extent
    only(check(tree, "sheared", 2, xforms=x), placement_box=1)


def test_records_of_two_trees_of_one_scene_are_the_same_records(monkeypatch):
    """record_mismatches pairs records by shape id (prototypes: mesh, face): two host trees with different leaf orders
    agree, and one changed word is one mismatch"""
    a = host_tree("instanced", F32, 1, "", monkeypatch)
    b = mutable(host_tree("instanced", F32, 4, "wide", monkeypatch))
    n = scene("instanced").n_shapes
    assert not np.array_equal(a["prims"]["shape_id"], b["prims"]["shape_id"])
    assert T.record_mismatches(a, b, n) == 0
    b["prims"]["material"][5] += 1
    assert T.record_mismatches(a, b, n) == 1

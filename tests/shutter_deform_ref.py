"""numpy float64 restatement of the vertices of a deforming mesh at a time of the shutter (include/take_hip.h:
take_hip_shutter_vertices, take_hip_render_shutter_meshes; DESIGN.md par. 4r; the device text is k_shutter_vertices in
take_amd/csrc/tk_shutter.h): the shutter's lerp (tests/shutter_ref.py) applied to whole arrays, and the `moved` flag.
Every operation is one IEEE double operation in the order written, as the library's."""
import numpy as np

import shutter_ref as S


def vertices(t, a, b):
    """a (the marked frame) -> b (the current one) at scene time t, entry by entry; positions and normals alike: nothing
    is renormalised, nothing is looked at -> (out, moved): moved = 1 where any entry of out is not b's bit for bit"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    out = np.ascontiguousarray(S.lerp(t, a, b))
    return out, int(not np.array_equal(out.view(np.uint64), b.view(np.uint64)))


def edge_values():
    """(a, b) pairs of the cases that matter to the lerp: equal ends, zeros of either sign at either end, subnormals,
    huge values of opposite sign (their sum stays finite, each product too), a NaN and an infinity at either end"""
    tiny, sub = np.finfo(np.float64).tiny, 5e-324
    nan, inf = np.nan, np.inf
    pairs = [(1.5, 1.5), (-2.25, -2.25), (0.1, 0.1), (1e300, 1e300), (sub, sub),
             (0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (0.0, 3.0), (-0.0, 3.0), (3.0, 0.0), (3.0, -0.0), (-0.0, -3.0),
             (sub, 3 * sub), (-sub, sub), (tiny, tiny / 2), (tiny / 4, -tiny), (sub, 1.0), (0.0, sub),
             (1e300, -1e300), (-1e300, 1e300), (1e300, -3e299), (-1.7e308, 1.7e308),
             (nan, 1.0), (1.0, nan), (nan, nan), (inf, 1.0), (1.0, -inf), (inf, inf), (inf, -inf),
             (0.1, 0.7), (1.0 / 3.0, -2.0 / 3.0), (1e-9, 1e9)]
    a, b = np.array(pairs, np.float64).T
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def edge_arrays(n, seed):
    """n doubles per end: the edge values, repeated in a shuffled order, among ordinary values — a third of which did
    not move"""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=n), rng.normal(size=n)
    still = rng.random(n) < 1.0 / 3.0
    b[still] = a[still]
    ea, eb = edge_values()
    at = rng.permutation(n)[:min(n, 4 * len(ea))]
    pick = rng.integers(0, len(ea), len(at))
    a[at], b[at] = ea[pick], eb[pick]
    return a, b

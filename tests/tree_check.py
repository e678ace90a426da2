"""Structural validation of an acceleration structure against the exact extents of its primitives.

Input: a tree in the raw layout of take_hip_debug_tree (capi.Scene.debug_tree: what the trace kernels read from device
memory) or of its host twin (helpers.hostsim_debug_tree).  Nothing here is shared with the builders: the checker knows
the struct layouts, the child-word encoding and the constants of take_amd/csrc/tk_scene.h, restated below, and never
looks at a box a builder computed as if it were true — every box is compared with the primitives below it.

Exactness.  A coordinate of a primitive's extent is a sum of two stored numbers, v0 + e or c +- r.  It is carried as
the pair (s, err) of TwoSum: s = fl(a + b) in double and err the exact residual, a + b = s + err as real numbers
(|err| <= ulp(s) / 2, so the order of the reals is the lexicographic order of the pairs).  For float records err is 0
unless the exponents differ by more than 29; for double records it decides the comparison when s ties with a plane.
A full-width plane is one stored number: the comparison is exact.  A compressed plane is
plane(q) = grid_lo + (Q_BIAS + q) * grid_step, moved inwards by delta = Q_MAX * grid_step * 2^-20 (the allowance
tk_traverse.h's qray_make spends on the grid-space slab test): the product and delta are exact doubles, the sums are
evaluated in double with a bound on their rounding, and a slot whose margin is inside that bound is decided in
rational arithmetic (fractions.Fraction).  No tolerance anywhere.

check_tree returns a dict: "errors" = counts per category (all must be 0), "diag" = figures that are reported and not
judged, "where" = the first few offenders in words.
"""
from fractions import Fraction

import numpy as np

CHILD_EMPTY = -(1 << 31)
INSTANCE_WORD_END = -(1 << 30)  # instance words: CHILD_EMPTY < w < this
MAX_LEAF = 4
Q_MAX, Q_BIAS = 32767, 32768
MAX_STACK_ENTRIES, MAX_STACK_ENTRIES_W8 = 96, 192
U = 2.0 ** -53  # unit roundoff of a double
NODE_FORMAT_WIDE = 0

ERROR_CATEGORIES = ("bad_child", "unreached", "reached_twice", "leaf_size", "partition", "shape_ids", "instance_ids",
                    "empty_slot", "q_range", "containment", "placement_box", "placement_nesting", "depth", "stack")


def two_sum(a, b):
    """(s, err) with a + b = s + err exactly (Knuth; a, b finite doubles)"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _less(s1, e1, s2, e2):
    return (s1 < s2) | ((s1 == s2) & (e1 < e2))


def _lex_min(a, b):
    m = _less(b[0], b[1], a[0], a[1])
    return np.where(m, b[0], a[0]), np.where(m, b[1], a[1])


def _lex_max(a, b):
    m = _less(a[0], a[1], b[0], b[1])
    return np.where(m, b[0], a[0]), np.where(m, b[1], a[1])


def prim_extents(prims):
    """exact extent of every record per axis: (lo_s, lo_e, hi_s, hi_e), each (n, 3) — triangles: the real numbers v0,
    v0 + e1, v0 + e2 of the stored record, spheres: c -+ r (the geometry the intersection tests see)"""
    a = prims["a"].astype(np.float64)
    sphere = ((prims["meta"] & 0xff) == 1)[:, None]
    v0 = (a[:, 0:3], np.zeros_like(a[:, 0:3]))
    v1, v2 = two_sum(a[:, 0:3], a[:, 3:6]), two_sum(a[:, 0:3], a[:, 6:9])
    tlo, thi = _lex_min(v0, _lex_min(v1, v2)), _lex_max(v0, _lex_max(v1, v2))
    r = a[:, 3:4] * np.ones((1, 3))
    slo, shi = two_sum(a[:, 0:3], -r), two_sum(a[:, 0:3], r)
    return (np.where(sphere, slo[0], tlo[0]), np.where(sphere, slo[1], tlo[1]),
            np.where(sphere, shi[0], thi[0]), np.where(sphere, shi[1], thi[1]))


def prim_vertices(prims):
    """the records' vertices as doubles, (n, 3 vertices, 3): triangles only (prototype records); each sum is within
    2^-53 of the real vertex"""
    a = prims["a"].astype(np.float64)
    return np.stack([a[:, 0:3], a[:, 0:3] + a[:, 3:6], a[:, 0:3] + a[:, 6:9]], 1)


def _half_area(lo, hi):
    e = np.maximum(hi - lo, 0.0)
    return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]


class _Check:
    def __init__(self, tree, max_leaf_size, n_shapes, xforms):
        self.t = tree
        self.fmt, self.W = tree["node_format"], tree["node_width"]
        self.wide = self.fmt == NODE_FORMAT_WIDE
        self.n_nodes, self.n_prims, self.n_inst = tree["n_nodes"], tree["n_prims"], tree["n_instances"]
        self.two_level = bool(tree["two_level"])
        self.max_leaf = max_leaf_size
        self.n_top = self.n_prims if not self.two_level else n_shapes
        if self.two_level and (n_shapes is None or xforms is None):
            raise ValueError("a two-level scene needs n_shapes and the placements' transforms")
        self.xforms = None if xforms is None else np.ascontiguousarray(xforms, np.float64).reshape(-1, 3, 4)
        self.err = {k: 0 for k in ERROR_CATEGORIES}
        self.where = []
        self.child = tree["nodes"]["c"]["child"].reshape(self.n_nodes, self.W).astype(np.int64)
        self.refs = np.zeros(self.n_nodes, np.int64)
        self.expanded = np.zeros(self.n_nodes, bool)
        self.cover = np.zeros(self.n_prims + 1, np.int64)  # difference array of the leaf ranges, all trees
        self.ext = prim_extents(tree["prims"]) if self.n_prims else tuple(np.zeros((0, 3)) for _ in range(4))
        inf = np.inf
        # per node: the exact extent of everything below it (pairs), and the native box of the placements below it
        self.node_ext = [np.full((self.n_nodes, 3), v) for v in (inf, 0.0, -inf, 0.0)]
        self.node_ibox = [np.full((self.n_nodes, 3), inf), np.full((self.n_nodes, 3), -inf)]
        self.inst_seen = np.zeros(max(self.n_inst, 1), np.int64)
        self.inst_slot = {}  # placement -> (node, slot) of its instance word
        self.margin = {"lo": (np.inf, None), "hi": (np.inf, None)}  # smallest box margin and where (node, slot, axis)
        self.infl_sum, self.infl_n = 0.0, 0

    def fail(self, cat, n, text):
        n = int(n)
        if n:
            self.err[cat] += n
            if len(self.where) < 12:
                self.where.append(f"{cat}: {text}")

    # ---- the planes of the slots of `nodes` (k, W, 3): native (float planes / grid coordinates) and, for compressed
    # nodes, the exact product (Q_BIAS + q) * step
    def native_planes(self, nodes):
        c = self.t["nodes"]["c"][nodes]
        if self.wide:
            return c["bmin"].astype(np.float64), c["bmax"].astype(np.float64)
        q = c["q"]
        return (q & 0xffff).astype(np.float64), (q >> 16).astype(np.float64)

    def walk(self, root, grid, top):
        """one tree from the child word `root`: reachability, leaf ranges, then bottom-up containment; -> (levels of
        wide nodes, [first, end) hull of its leaf ranges)"""
        own = np.zeros(self.n_prims + 1, np.int64)
        levels = []
        if root == CHILD_EMPTY:
            return 0, (0, 0), own
        if root < 0:  # the whole tree is one leaf
            first, count = (-root - 1) // MAX_LEAF, (-root - 1) % MAX_LEAF + 1
            if first + count > self.n_prims:
                self.fail("bad_child", 1, f"root leaf [{first}, {first + count}) outside the {self.n_prims} records")
                return 0, (0, 0), own
            own[first] += 1
            own[first + count] -= 1
            return 0, (first, first + count), own
        if root >= self.n_nodes:
            self.fail("bad_child", 1, f"root {root} outside the {self.n_nodes} nodes")
            return 0, (0, 0), own
        self.refs[root] += 1
        frontier = np.array([root], np.int64)
        frontier = frontier[~self.expanded[frontier]]
        while frontier.size and len(levels) < 128:
            self.expanded[frontier] = True
            levels.append(frontier)
            w = self.child[frontier]
            interior = w >= 0
            bad = interior & (w >= self.n_nodes)
            self.fail("bad_child", bad.sum(), f"node {frontier[bad.any(1)][:1]}: a child index outside the {self.n_nodes} nodes")
            nxt = w[interior & ~bad]
            np.add.at(self.refs, nxt, 1)
            nxt = np.unique(nxt)
            frontier = nxt[~self.expanded[nxt]]
        self.bottom_up(levels, grid, top, own)
        cs = np.cumsum(own[:-1])
        idx = np.nonzero(cs)[0]
        hull = (int(idx[0]), int(idx[-1]) + 1) if idx.size else (0, 0)
        return len(levels), hull, own

    def bottom_up(self, levels, grid, top, own):
        g_lo, g_step = (np.asarray(grid[0], np.float64), np.asarray(grid[1], np.float64)) if grid is not None else (None, None)
        for nodes in reversed(levels):
            w = self.child[nodes]  # (k, W)
            k = nodes.size
            empty = w == CHILD_EMPTY
            interior = (w >= 0) & (w < self.n_nodes)
            inst = (w < INSTANCE_WORD_END) & ~empty
            leaf = (w < 0) & ~inst & ~empty
            nat_lo, nat_hi = self.native_planes(nodes)
            # -- the slot's content
            shape = (k, self.W, 3)
            c = [np.full(shape, v) for v in (np.inf, 0.0, -np.inf, 0.0)]
            ib = [np.full(shape, np.inf), np.full(shape, -np.inf)]
            first, count = (-w - 1) // MAX_LEAF, (-w - 1) % MAX_LEAF + 1
            bad_leaf = leaf & (first + count > self.n_prims)
            self.fail("bad_child", bad_leaf.sum(), f"node {nodes[bad_leaf.any(1)][:1]}: a leaf range outside the {self.n_prims} records")
            leaf &= ~bad_leaf
            big = leaf & (count > self.max_leaf)
            self.fail("leaf_size", big.sum(), f"node {nodes[big.any(1)][:1]}: a leaf of more than {self.max_leaf} primitives")
            np.add.at(own, first[leaf], 1)
            np.add.at(own, (first + count)[leaf], -1)
            for j in range(MAX_LEAF):
                m = leaf & (j < count)
                p = np.where(m, first + j, 0)
                mm = m[..., None]
                lo = _lex_min((c[0], c[1]), (np.where(mm, self.ext[0][p], np.inf), np.where(mm, self.ext[1][p], 0.0)))
                hi = _lex_max((c[2], c[3]), (np.where(mm, self.ext[2][p], -np.inf), np.where(mm, self.ext[3][p], 0.0)))
                c = [lo[0], lo[1], hi[0], hi[1]]
            ch = np.where(interior, w, 0)
            mi = interior[..., None]
            for i in range(4):
                c[i] = np.where(mi, self.node_ext[i][ch], c[i])
            for i in range(2):
                ib[i] = np.where(mi, self.node_ibox[i][ch], ib[i])
            if inst.any():
                ids = (w - (CHILD_EMPTY + 1))
                if not top:
                    self.fail("bad_child", inst.sum(), f"node {nodes[inst.any(1)][:1]}: an instance word inside a prototype's tree")
                else:
                    bad = inst & (ids >= self.n_inst)
                    self.fail("bad_child", bad.sum(), f"node {nodes[bad.any(1)][:1]}: an instance word beyond the {self.n_inst} placements")
                    ok = inst & ~bad
                    np.add.at(self.inst_seen, ids[ok], 1)
                    for a, s in zip(*np.nonzero(ok)):
                        self.inst_slot[int(ids[a, s])] = (int(nodes[a]), int(s))
                    mo = ok[..., None]
                    ib[0], ib[1] = np.where(mo, nat_lo, ib[0]), np.where(mo, nat_hi, ib[1])
            # -- the slot's box against its content
            has = ~empty & np.isfinite(c[0]).all(-1)
            self.check_slots(nodes, has, nat_lo, nat_hi, c, g_lo, g_step)
            nest = ~empty & ((nat_lo > ib[0]) | (nat_hi < ib[1])).any(-1)
            self.fail("placement_nesting", nest.sum(), f"node {nodes[nest.any(1)][:1]}: a box that does not contain a placement's box below it")
            # -- empty slots, plane ranges
            if self.wide:
                inverted = (nat_lo > nat_hi).all(-1)
                wrong = empty != inverted
            else:
                wrong = empty & ((nat_lo != Q_MAX) | (nat_hi != 0)).any(-1)
                rng = ~empty & ((nat_lo > nat_hi) | (nat_hi > Q_MAX)).any(-1)
                self.fail("q_range", rng.sum(), f"node {nodes[rng.any(1)][:1]}: planes outside 0 <= lo <= hi <= Q_MAX")
            self.fail("empty_slot", wrong.sum(), f"node {nodes[wrong.any(1)][:1]}: an empty slot without the inverted box (or the reverse)")
            # -- the node's own content: union over its slots
            lo, hi = (c[0][:, 0], c[1][:, 0]), (c[2][:, 0], c[3][:, 0])
            ilo, ihi = ib[0][:, 0], ib[1][:, 0]
            for s in range(1, self.W):
                lo, hi = _lex_min(lo, (c[0][:, s], c[1][:, s])), _lex_max(hi, (c[2][:, s], c[3][:, s]))
                ilo, ihi = np.minimum(ilo, ib[0][:, s]), np.maximum(ihi, ib[1][:, s])
            for i, v in enumerate((lo[0], lo[1], hi[0], hi[1])):
                self.node_ext[i][nodes] = v
            self.node_ibox[0][nodes], self.node_ibox[1][nodes] = ilo, ihi

    def check_slots(self, nodes, has, nat_lo, nat_hi, c, g_lo, g_step):
        if not has.any():
            return
        h3 = has[..., None] & np.ones(3, bool)
        if self.wide:
            bad_lo = h3 & _less(c[0], c[1], nat_lo, 0.0)  # content below bmin
            bad_hi = h3 & _less(nat_hi, 0.0, c[2], c[3])
            with np.errstate(invalid="ignore", over="ignore"):
                m_lo = (c[0] - nat_lo) / np.spacing(np.abs(nat_lo).astype(np.float32)).astype(np.float64)
                m_hi = (nat_hi - c[2]) / np.spacing(np.abs(nat_hi).astype(np.float32)).astype(np.float64)
            box_lo, box_hi = nat_lo, nat_hi
        else:
            step = g_step[None, None, :]
            g = g_lo[None, None, :]
            d = Q_MAX * step * 2.0 ** -20                      # exact: 15 bits x 24 bits
            p_lo, p_hi = (Q_BIAS + nat_lo) * step, (Q_BIAS + nat_hi) * step  # exact: 16 bits x 24 bits
            # content - (inward plane), in double, and a bound on the roundings of the four operations
            a_lo = (((c[0] - g) - p_lo) - d) + c[1]
            a_hi = (((g - c[2]) + p_hi) - d) - c[3]
            t_lo = 8 * U * (np.abs(c[0]) + np.abs(g) + p_lo + d)
            t_hi = 8 * U * (np.abs(c[2]) + np.abs(g) + p_hi + d)
            bad_lo, bad_hi = h3 & (a_lo < -t_lo), h3 & (a_hi < -t_hi)
            for a, t, bad, side in ((a_lo, t_lo, bad_lo, 0), (a_hi, t_hi, bad_hi, 1)):
                for i, s, ax in zip(*np.nonzero(h3 & (np.abs(a) <= t))):  # too close for doubles: rationals
                    plane = Fraction(float(g_lo[ax])) + Fraction(int(Q_BIAS + (nat_hi if side else nat_lo)[i, s, ax])) * Fraction(float(g_step[ax]))
                    delta = Fraction(Q_MAX) * Fraction(float(g_step[ax])) / (1 << 20)
                    x = Fraction(float(c[2 * side][i, s, ax])) + Fraction(float(c[2 * side + 1][i, s, ax]))
                    bad[i, s, ax] = (x > plane - delta) if side else (x < plane + delta)
            m_lo, m_hi = a_lo / step, a_hi / step
            box_lo, box_hi = g + p_lo + d, g + p_hi - d
        bad = (bad_lo | bad_hi).any(-1)
        if bad.any():
            i, s = [int(v[0]) for v in np.nonzero(bad)]
            ax = int(np.nonzero((bad_lo | bad_hi)[i, s])[0][0])
            self.fail("containment", bad.sum(), f"node {int(nodes[i])} slot {s} axis {ax}: box [{box_lo[i, s, ax]!r}, {box_hi[i, s, ax]!r}] "
                      f"content [{c[0][i, s, ax]!r}, {c[2][i, s, ax]!r}]")
        for key, m in (("lo", m_lo), ("hi", m_hi)):
            mm = np.where(h3 & np.isfinite(m), m, np.inf)
            j = np.unravel_index(np.argmin(mm), mm.shape)
            if mm[j] < self.margin[key][0]:
                self.margin[key] = (float(mm[j]), (int(nodes[j[0]]), int(j[1]), int(j[2])))
        at, ab = _half_area(c[0], c[2])[has], _half_area(box_lo, box_hi)[has]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(at > 0, np.minimum(ab / at, 100.0), np.where(ab > 0, 100.0, 1.0))
        self.infl_sum += float(r.sum())
        self.infl_n += int(r.size)

    def placements(self, proto_range):
        """the box of the slot that holds placement i's instance word against the image, under xforms[i], of every vertex
        of its prototype's resident records"""
        if self.xforms.shape[0] != self.n_inst:
            raise ValueError(f"{self.xforms.shape[0]} transforms for {self.n_inst} placements")
        inst = self.t["inst_trace"]
        g_lo, g_step = np.asarray(self.t["grid_lo"], np.float64), np.asarray(self.t["grid_step"], np.float64)
        verts = {}
        worst = np.inf
        for i in range(self.n_inst):
            if i not in self.inst_slot:
                continue  # (counted under instance_ids)
            root = int(inst["root_child"][i])
            if root not in verts:
                p0, p1 = proto_range[root]
                verts[root] = prim_vertices(self.t["prims"][p0:p1]).reshape(-1, 3)
            v, m = verts[root], self.xforms[i]
            w = m[:, 0] * v[:, 0:1] + m[:, 1] * v[:, 1:2] + m[:, 2] * v[:, 2:3] + m[:, 3]
            # The checker's own rounding.  A coordinate of the image is m0 x + m1 y + m2 z + t evaluated in double: three
            # products and three sums, each within 2^-53 relative, on a vertex that is itself within 2^-53 of the real
            # v0 + e — together at most 6 * 2^-53 * (|m0 x| + |m1 y| + |m2 z| + |t|) = 6.7e-16 of the magnitude (first
            # order; the factor is 5 for the operations + 1 for the vertex).  k_placement_pad pads by 4e-6 (float sides)
            # and 1e-13 (double sides) of the magnitude: 6e9 and 150 times this bound.
            b = 6 * U * (np.abs(m[:, 0] * v[:, 0:1]) + np.abs(m[:, 1] * v[:, 1:2]) + np.abs(m[:, 2] * v[:, 2:3]) + np.abs(m[:, 3]))
            w_lo, w_hi = (w - b).min(0), (w + b).max(0)
            node, slot = self.inst_slot[i]
            nat_lo, nat_hi = self.native_planes(np.array([node]))
            nat_lo, nat_hi = nat_lo[0, slot], nat_hi[0, slot]
            if self.wide:
                box_lo, box_hi = nat_lo, nat_hi  # exact
            else:  # the inward planes, evaluated in double: moved further inwards by the bound on those roundings
                d = Q_MAX * g_step * 2.0 ** -20
                p_lo, p_hi = (Q_BIAS + nat_lo) * g_step, (Q_BIAS + nat_hi) * g_step
                box_lo = (g_lo + p_lo + d) + 4 * U * (np.abs(g_lo) + p_lo + d)
                box_hi = (g_lo + p_hi - d) - 4 * U * (np.abs(g_lo) + p_hi + d)
            bad = (box_lo > w_lo) | (box_hi < w_hi)
            if bad.any():
                ax = int(np.nonzero(bad)[0][0])
                self.fail("placement_box", 1, f"placement {i} (node {node} slot {slot}) axis {ax}: box [{box_lo[ax]!r}, {box_hi[ax]!r}] "
                          f"image [{w_lo[ax]!r}, {w_hi[ax]!r}]")
            mag = max(np.abs(w_lo).max(), np.abs(w_hi).max(), 1e-300)
            worst = min(worst, float(min((w_lo - box_lo).min(), (box_hi - w_hi).min()) / mag))
        return worst

    def run(self, expected_depth):
        t = self.t
        top_levels, top_hull, own = self.walk(t["root_child"], (t["grid_lo"], t["grid_step"]), True)
        cs = np.cumsum(own[:-1])
        n_top = self.n_top
        self.fail("partition", (cs[:n_top] != 1).sum() + (cs[n_top:] != 0).sum(),
                  f"the top-level tree's leaves do not cover its records [0, {n_top}) once each")
        self.cover += own
        ids = t["prims"]["shape_id"][:n_top].astype(np.int64)
        inside = (ids >= 0) & (ids < n_top)
        cnt = np.bincount(ids[inside], minlength=n_top)
        self.fail("shape_ids", (~inside).sum() + (cnt != 1).sum(), "the top level's shape ids are not 0..n_shapes-1 once each")
        proto_levels, proto_range = 0, {}
        if self.two_level:
            inst = t["inst_trace"]
            for root in np.unique(inst["root_child"]):
                first = int(np.nonzero(inst["root_child"] == root)[0][0])
                same = inst[inst["root_child"] == root]
                if (same["grid_lo"] != same["grid_lo"][0]).any() or (same["grid_step"] != same["grid_step"][0]).any():
                    self.fail("bad_child", 1, f"placements of the prototype at {root} disagree about its grid")
                levels, hull, own = self.walk(int(root), (inst["grid_lo"][first], inst["grid_step"][first]), False)
                cs = np.cumsum(own[:-1])
                self.fail("partition", (cs[hull[0]:hull[1]] != 1).sum(), f"the leaves of the prototype at {root} do not cover [{hull[0]}, {hull[1]}) once each")
                self.cover += own
                ids = t["prims"]["shape_id"][hull[0]:hull[1]].astype(np.int64)
                n = hull[1] - hull[0]
                inside = (ids >= 0) & (ids < n)
                self.fail("shape_ids", (~inside).sum() + (np.bincount(ids[inside], minlength=n) != 1).sum(),
                          f"the face ids of the prototype at {root} are not 0..{n - 1} once each")
                proto_levels = max(proto_levels, levels)
                proto_range[int(root)] = hull
            self.fail("instance_ids", (self.inst_seen[:self.n_inst] != 1).sum(), "a placement without exactly one instance word")
        total = np.cumsum(self.cover[:-1])
        if self.two_level:  # (records no tree owns, or two trees own; the per-tree counts above cover the rest)
            orphan = (total == 0) & (np.arange(self.n_prims) >= n_top)
            self.fail("partition", orphan.sum(), "records behind the shapes' that no prototype's tree owns")
        self.fail("unreached", (self.refs == 0).sum(), f"first: node {np.nonzero(self.refs == 0)[0][:1]}")
        self.fail("reached_twice", np.maximum(self.refs - 1, 0).sum(), f"first: node {np.nonzero(self.refs > 1)[0][:1]}")
        depth = top_levels + proto_levels
        if expected_depth is not None and depth != expected_depth:
            self.fail("depth", 1, f"measured {depth} levels ({top_levels} + {proto_levels}), the scene's stats say {expected_depth}")
        # the trace kernel's one stack: W - 1 entries per level of both trees, + 1, + the return marker of a placement
        entries = (self.W - 1) * depth + 1 + (1 if self.two_level else 0)
        if entries > (MAX_STACK_ENTRIES_W8 if self.W == 8 else MAX_STACK_ENTRIES):
            self.fail("stack", 1, f"{entries} stack entries for {depth} levels")
        diag = {"depth": depth, "top_levels": top_levels, "proto_levels": proto_levels,
                "min_margin_lo": self.margin["lo"][0], "min_margin_lo_at": self.margin["lo"][1],
                "min_margin_hi": self.margin["hi"][0], "min_margin_hi_at": self.margin["hi"][1],
                "margin_unit": "float ulps" if self.wide else "grid cells",
                "inflation": self.infl_sum / self.infl_n if self.infl_n else 1.0, "slots": self.infl_n}
        if self.two_level:
            diag["min_placement_margin_rel"] = self.placements(proto_range)
        return {"errors": dict(self.err), "diag": diag, "where": list(self.where)}


def check_tree(tree, max_leaf_size=MAX_LEAF, n_shapes=None, xforms=None, expected_depth=None):
    """Validate `tree` (capi.Scene.debug_tree / helpers.hostsim_debug_tree).  max_leaf_size: the largest leaf the
    builder was allowed; n_shapes and xforms ((n, 3, 4) object -> world, the CURRENT transforms): two-level scenes;
    expected_depth: take_hip_scene_stats' depth, compared with the measured one when given."""
    return _Check(tree, max_leaf_size, n_shapes, xforms).run(expected_depth)


def total_errors(result):
    return sum(result["errors"].values())


def record_mismatches(a, b, n_shapes):
    """records of two trees of one scene that differ, whatever their leaf orders: the shapes' records paired by shape
    id, a prototype's by (mesh, face).  Compared: the geometry words (bits), shape_id, meta, material, area_light, nidx, mesh."""
    pa, pb = a["prims"], b["prims"]
    if pa.shape != pb.shape or pa.dtype != pb.dtype:
        return max(pa.shape[0], pb.shape[0])

    def ordered(p):
        proto = np.arange(p.shape[0]) >= n_shapes
        return p[np.lexsort((p["shape_id"], np.where(proto, p["mesh"], -1), proto))]

    pa, pb = ordered(pa), ordered(pb)
    bits = "<u4" if pa["a"].dtype.itemsize == 4 else "<u8"
    diff = (pa["a"].view(bits) != pb["a"].view(bits)).any(1)
    for f in ("shape_id", "meta", "material", "area_light", "nidx", "mesh"):
        diff |= pa[f] != pb[f]
    return int(diff.sum())

"""A structural audit of the wide BVHs the product builds and re-fits, in numpy alone: what MsneReadBvh returns (Node8 nodes, TriRec records, the TLAS root and the
TLAS items) held against the scene's own vertex arrays.  Nothing of csrc/bvh_build.hip is restated here but the byte layout of Node8 / TriRec
(csrc/msne_device.h); a child plane is origin + q * 2^(e - 127), evaluated in float64, which is exact.

Bounds come bottom-up from the MESHES, never from the builder's boxes.  For a slot, B is the per-axis min / max over the finite corner coordinates (|x| < 3.4e38)
of every triangle under it ("Garbage in"); ext is B's largest extent, g = 1e-4 * ext, Q_k the node's quantum on axis k, M the largest absolute
coordinate among B and the node's origin, tau = 2 * ulp_f32(M): the builder's floor((lo - grow - origin) * 2^-e - 1e-3) rounds twice before the exact scaling, each
time by at most half an ulp of M.  Per used slot of every node reachable from a root:

  I1 containment   lower plane <= B.lo, upper plane >= B.hi                                           (always)
  I2 margin        B.lo - lower plane >= max(0, g + 1e-3 * Q_k - tau), likewise above                 (builds; identity-only slots of a TLAS)
  I3 tightness     B.lo - lower plane <= g + 2 * Q_k + tau, likewise above                            (fresh builds)
  I4 grid          with U the union under the node and Qmax its coarsest quantum: Q_k >= ext_k(U) / 252, Q_k >= Qmax / 4,
                   Q_k <= max(2 * ext_k(U) / 252 * (1 + 2^-22), Qmax / 4), |(U.lo_k - origin_k) - Q_k| <= tau; every exponent 1 where U has no extent   (fresh builds)
  I5 topology      imask & lmask == 0; child ranges disjoint and inside the pool (a cyclic child_base is reported, the walk ends); every item referenced once; every
                   record bit for bit a triangle of its tree's meshes, every triangle of them once; the TLAS items are the instances the scene says

Child planes are NOT held against the parent's planes: a child's quantum can exceed the parent's 1e-3-quantum push.  I2 at every level, with B the union under the
slot, is what the traversal needs.  The only slots passed over are those whose subtree has no finite corner on some axis; they are counted, the tests hold the count.
"""
from collections import namedtuple

import numpy as np

GROWTH = 1e-4          # every child box grown by 1e-4 of its own largest extent ...
PUSH = 1e-3            # ... and rounded outward by at least 1e-3 quantum
FINITE = 3.4e38

Violation = namedtuple("Violation", "invariant tree node slot axis amount what")


def boxes(node):
    """one 80-byte node -> (lo (3, 8), hi (3, 8), imask, lmask, child_base, item_base): the child planes as the traversal sees them, in float64"""
    node = np.ascontiguousarray(node, np.uint8).reshape(80)
    o = node[0:12].view(np.float32).astype(np.float64); e = node[12:15].astype(np.int32)
    sc = np.ldexp(1.0, e - 127)
    lo = o[:, None] + node[32:56].reshape(3, 8).astype(np.float64) * sc[:, None]
    hi = o[:, None] + node[56:80].reshape(3, 8).astype(np.float64) * sc[:, None]
    return lo, hi, int(node[15]), int(node[24]), int(node[16:20].view(np.uint32)[0]), int(node[20:24].view(np.uint32)[0])


class Decoded:
    """every node of the pool at once"""
    def __init__(self, nodes):
        N = np.ascontiguousarray(nodes, np.uint8).reshape(-1, 80)
        self.n = len(N)
        self.origin = N[:, 0:12].copy().view(np.float32).astype(np.float64)
        self.e = N[:, 12:15].astype(np.int32)
        self.imask = N[:, 15].astype(np.int64); self.lmask = N[:, 24].astype(np.int64)
        self.child_base = N[:, 16:20].copy().view(np.uint32)[:, 0].astype(np.int64)
        self.item_base = N[:, 20:24].copy().view(np.uint32)[:, 0].astype(np.int64)
        self.quantum = np.ldexp(1.0, self.e - 127)
        self.lo = self.origin[:, :, None] + N[:, 32:56].reshape(-1, 3, 8).astype(np.float64) * self.quantum[:, :, None]
        self.hi = self.origin[:, :, None] + N[:, 56:80].reshape(-1, 3, 8).astype(np.float64) * self.quantum[:, :, None]


_POP = np.array([bin(i).count("1") for i in range(256)])


def ulp32(x):
    return np.spacing(np.minimum(np.abs(np.asarray(x, np.float64)), 3.0e38).astype(np.float32)).astype(np.float64)


def finite_bounds(V):
    """(..., corners, 3) coordinates -> per-axis min and max over the finite ones; NaN where an axis has none"""
    V = np.asarray(V, np.float64)
    V = np.where(np.abs(V) < FINITE, V, np.nan)
    return np.fmin.reduce(V, axis=-2), np.fmax.reduce(V, axis=-2)


class Report:
    def __init__(self):
        self.violations = []; self.skipped_leaf_slots = 0; self.skipped_internal_slots = 0
        self.slots = {"I1": 0, "I2": 0, "I3": 0}; self.nodes_i4 = 0; self.nodes = 0; self.trees = 0

    def add(self, inv, tree, node, slot, axis, amount, what):
        self.violations.append(Violation(inv, tree, int(node), int(slot), int(axis), float(amount), what))

    def invariants(self):
        return sorted({v.invariant for v in self.violations})

    def __str__(self):
        head = "%d violations %s over %d nodes of %d trees (slots held: %s, grids held: %d, slots passed over: %d leaves, %d internal)" % (
            len(self.violations), self.invariants(), self.nodes, self.trees, self.slots, self.nodes_i4, self.skipped_leaf_slots, self.skipped_internal_slots)
        return "\n".join([head] + ["  %s %s node %d slot %d axis %d by %g: %s" % v for v in self.violations[:20]])


def walk(dec, root, claimed, rep, tree):
    """the nodes of the tree under `root`, parents before children.  claimed[n] = the node n was reached from (-2 for a root, -1: not reached).  A child range that
    leaves the pool, or holds a node that was reached before (overlapping ranges; a child_base that points at an ancestor), is reported and not entered: the walk ends."""
    order = []
    if not 0 <= root < dec.n:
        rep.add("I5", tree, root, -1, -1, 0, "root outside the pool of %d nodes" % dec.n); return order
    if claimed[root] != -1:
        rep.add("I5", tree, root, -1, -1, 0, "root was reached from node %d" % claimed[root]); return order
    claimed[root] = -2
    stack = [root]
    while stack:
        n = stack.pop(); order.append(n)
        if dec.imask[n] & dec.lmask[n]:
            rep.add("I5", tree, n, -1, -1, dec.imask[n] & dec.lmask[n], "imask & lmask != 0")
        k = int(_POP[dec.imask[n]]); cb = int(dec.child_base[n])
        if k and cb + k > dec.n:
            rep.add("I5", tree, n, -1, -1, cb + k - dec.n, "child range [%d, %d) leaves the pool" % (cb, cb + k)); continue
        for c in range(cb, cb + k):
            if claimed[c] != -1:
                rep.add("I5", tree, n, -1, -1, c, "child %d was reached before (from %d): overlapping child ranges or a cycle" % (c, claimed[c])); continue
            claimed[c] = n; stack.append(c)
    return order


def check_tree(dec, order, claimed, leaf_lo, leaf_hi, item_refs, rep, tree, margin=True, fresh=True, strict_items=None, widen=False):
    """I1 (always), I2 (`margin`), I3 and I4 (`fresh`) for the nodes of `order` (walk()), children before parents.  leaf_lo / leaf_hi: (items, 3) bounds of every
    leaf item from the scene's own arrays, NaN where an axis has no finite corner.  strict_items (TLAS): the items I2-I4 apply to — a slot is held to them when every
    item under it is; `widen`: tau grows by k_instance_boxes' documented 1.2e-7 |x| + 1e-30.  Returns the items in slot order."""
    n_items = len(leaf_lo)
    node_lo = {}; node_hi = {}; node_strict = {}
    for n in reversed(order):
        Bl = np.full((8, 3), np.nan); Bh = np.full((8, 3), np.nan)
        used = np.zeros(8, bool); leaf = np.zeros(8, bool); strict = np.ones(8, bool)
        ci = li = 0
        for s in range(8):
            if (dec.imask[n] >> s) & 1:
                c = int(dec.child_base[n]) + ci; ci += 1; used[s] = True
                if c < dec.n and claimed[c] == n and c in node_lo:
                    Bl[s] = node_lo[c]; Bh[s] = node_hi[c]; strict[s] = node_strict[c]
            elif (dec.lmask[n] >> s) & 1:
                it = int(dec.item_base[n]) + li; li += 1; used[s] = True; leaf[s] = True
                if it >= n_items:
                    rep.add("I5", tree, n, s, -1, it, "leaf item %d outside the %d items" % (it, n_items)); continue
                item_refs[it] += 1
                Bl[s] = leaf_lo[it]; Bh[s] = leaf_hi[it]
                if strict_items is not None:
                    strict[s] = bool(strict_items[it])
        rep.nodes += 1
        U_lo = np.fmin.reduce(Bl[used], axis=0) if used.any() else np.full(3, np.nan)
        U_hi = np.fmax.reduce(Bh[used], axis=0) if used.any() else np.full(3, np.nan)
        node_lo[n] = U_lo; node_hi[n] = U_hi; node_strict[n] = bool(strict[used].all())
        ok = used & ~(np.isnan(Bl).any(1) | np.isnan(Bh).any(1))
        rep.skipped_leaf_slots += int((used & ~ok & leaf).sum()); rep.skipped_internal_slots += int((used & ~ok & ~leaf).sum())
        Q = dec.quantum[n]; o = dec.origin[n]
        Pl = dec.lo[n].T; Ph = dec.hi[n].T                                              # (8, 3)
        with np.errstate(invalid="ignore"):
            ext = (Bh - Bl).max(1); g = GROWTH * ext
            M = np.maximum(np.maximum(np.abs(Bl).max(1), np.abs(Bh).max(1)), np.abs(o).max())
            tau = 2.0 * ulp32(np.where(ok, M, 0.0))
            for side, d, B in (("lower", Bl - Pl, Bl), ("upper", Ph - Bh, Bh)):           # d: how far the plane lies outside B
                t = tau[:, None] + ((1.2e-7 * np.abs(B) + 1e-30) if widen else 0.0)
                need = np.maximum(0.0, g[:, None] + PUSH * Q[None, :] - t)
                most = g[:, None] + 2.0 * Q[None, :] + t
                held = ok & strict
                for s, k in np.argwhere(ok[:, None] & (d < 0.0)):
                    rep.add("I1", tree, n, s, k, -d[s, k], "%s plane inside the bounds of what lies under the slot" % side)
                if margin:
                    for s, k in np.argwhere(held[:, None] & (d < need)):
                        rep.add("I2", tree, n, s, k, need[s, k] - d[s, k], "%s margin %g below g + 1e-3 Q - tau = %g" % (side, d[s, k], need[s, k]))
                if fresh:
                    for s, k in np.argwhere(held[:, None] & (d > most)):
                        rep.add("I3", tree, n, s, k, d[s, k] - most[s, k], "%s plane %g outside, more than g + 2 Q + tau = %g" % (side, d[s, k], most[s, k]))
        rep.slots["I1"] += int(ok.sum()); rep.slots["I2"] += int((ok & strict).sum()) if margin else 0; rep.slots["I3"] += int((ok & strict).sum()) if fresh else 0
        if fresh and node_strict[n] and not (np.isnan(U_lo).any() or np.isnan(U_hi).any()):
            rep.nodes_i4 += 1
            eu = U_hi - U_lo; Qmax = Q.max()
            t = 2.0 * float(ulp32(max(np.abs(U_lo).max(), np.abs(U_hi).max(), np.abs(o).max())))
            tk = t + ((1.2e-7 * np.abs(U_lo) + 1e-30) if widen else 0.0)
            if not (eu > 0.0).any():
                for k in np.flatnonzero(dec.e[n] != 1):
                    rep.add("I4", tree, n, -1, k, dec.e[n][k], "a node without extent has exponent %d, not 1" % dec.e[n][k])
            else:
                top = np.maximum(np.maximum(2.0 * eu / 252.0 * (1.0 + 2.0 ** -22), Qmax / 4.0), 2.0 ** -126)   # (2^-126: the smallest exponent a node can hold)
                for k in np.flatnonzero(Q < eu / 252.0):
                    rep.add("I4", tree, n, -1, k, eu[k] / 252.0 / Q[k], "quantum %g below extent / 252 = %g" % (Q[k], eu[k] / 252.0))
                for k in np.flatnonzero(Q < Qmax / 4.0):
                    rep.add("I4", tree, n, -1, k, Qmax / 4.0 / Q[k], "quantum %g finer than a quarter of the coarsest %g" % (Q[k], Qmax))
                for k in np.flatnonzero(Q > top):
                    rep.add("I4", tree, n, -1, k, Q[k] / top[k], "quantum %g coarser than max(2 extent / 252, Qmax / 4) = %g" % (Q[k], top[k]))
            off = np.abs((U_lo - o) - Q)
            for k in np.flatnonzero(off > tk):
                rep.add("I4", tree, n, -1, k, off[k], "origin %g is not one quantum %g below the lower face %g" % (o[k], Q[k], U_lo[k]))


# ---------------- the scene as the test made it ----------------

class SceneRecorder:
    """stands in front of a context (the product's, or any with the same calls) and keeps what the audit needs of the scene: every mesh's arrays, every instance's
    mesh list, transform and visibility.  Everything else goes through untouched."""
    def __init__(self, ctx):
        self._ctx = ctx; self.meshes = {}; self.instances = []

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def create_mesh(self, positions, indices, normals=None, texcoords=None):
        h = self._ctx.create_mesh(positions, indices, normals, texcoords)
        self.meshes[h] = (np.array(positions, np.float32).reshape(-1, 3), np.array(indices, np.uint32).reshape(-1, 3))
        return h

    def create_instance(self, geometries, transform=None, visible=True):
        h = self._ctx.create_instance(geometries, transform=transform, visible=visible)
        T = np.eye(3, 4, dtype=np.float32) if transform is None else np.array(transform, np.float32).reshape(3, 4)
        assert h == len(self.instances)
        self.instances.append({"meshes": [g[0] for g in geometries], "T": T, "visible": bool(visible)})
        return h

    def set_instance_transform(self, h, transform):
        self._ctx.set_instance_transform(h, transform)
        self.instances[h]["T"] = np.array(transform, np.float32).reshape(3, 4)

    def set_instance_visibility(self, h, v):
        self._ctx.set_instance_visibility(h, v)
        self.instances[h]["visible"] = bool(v)

    # what the scene says the acceleration structure holds (DESIGN.md sections 2-4: visible identity instances share ONE world BLAS, every other mesh list has one BLAS;
    # the TLAS holds the visible instances with finite transforms that are not in the world BLAS, and the world BLAS as instance number len(instances))
    def triangles(self, i):
        return sum(len(self.meshes[m][1]) for m in self.instances[i]["meshes"])

    def identity(self, i):
        return bool(np.array_equal(self.instances[i]["T"], np.eye(3, 4, dtype=np.float32)))

    def in_world(self, i):
        return self.instances[i]["visible"] and self.triangles(i) > 0 and self.identity(i)

    def expected_trees(self):
        """every BLAS as {(owner, geometry): mesh}: `owner` is TriRec::pad (the instance, in the world BLAS; 0 elsewhere)"""
        trees = {}; world = {}
        for i, inst in enumerate(self.instances):
            if self.in_world(i):
                world.update({(i, g): m for g, m in enumerate(inst["meshes"])})
            elif self.triangles(i) > 0:
                trees.setdefault(tuple(inst["meshes"]), {(0, g): m for g, m in enumerate(inst["meshes"])})
        out = list(trees.values())
        if world:
            out.append(world)
        return out

    def expected_items(self):
        """the TLAS items: instance numbers; empty when the world BLAS is all there is (the traversal then starts inside it)"""
        out = [i for i, inst in enumerate(self.instances)
               if not self.in_world(i) and inst["visible"] and self.triangles(i) > 0 and bool((np.abs(inst["T"]) < 3.0e38).all())]
        world = any(self.in_world(i) for i in range(len(self.instances)))
        if world and out:
            out.append(len(self.instances))
        return out

    def world_vertices(self, i):
        """float64 image of instance i's vertices under its f32 transform; i == len(instances): everything in the world BLAS"""
        if i == len(self.instances):
            return np.concatenate([self.world_vertices(j) for j in range(i) if self.in_world(j)])
        T = self.instances[i]["T"].astype(np.float64)
        return np.concatenate([self.meshes[m][0].astype(np.float64) @ T[:, :3].T + T[:, 3] for m in self.instances[i]["meshes"]])


def _tree_records(tree, meshes):
    """the TriRec records a BLAS over `tree` must hold, as (pad, geo, prim) rows and (n, 9) vertex words, sorted by (pad, geo, prim)"""
    keys = []; words = []
    for (owner, g), m in sorted(tree.items()):
        P, I = meshes[m]
        keys.append(np.stack([np.full(len(I), owner, np.uint32), np.full(len(I), g, np.uint32), np.arange(len(I), dtype=np.uint32)], 1))
        words.append(np.ascontiguousarray(P[I.astype(np.int64)].reshape(len(I), 9)).view(np.uint32))
    return np.concatenate(keys), np.concatenate(words)


def audit(bvh, scene, fresh=True, refit=False, world=None):
    """bvh: what Context.read_bvh() returns; scene: a SceneRecorder (or anything with its meshes / expected_trees / expected_items / world_vertices).
    fresh: a context that has built once — every TriRec of the pool belongs to a tree.  refit: the TLAS was re-fitted in place — I1 and I5 alone hold for it (a
    re-fitted grid may stay coarse).  world: per-instance world-space vertices to hold the TLAS against, instead of scene.world_vertices."""
    nodes, tris, root, items = bvh
    dec = Decoded(nodes); rep = Report()
    tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 12); items = np.asarray(items, np.int64)
    claimed = np.full(dec.n, -1, np.int64)
    want_items = scene.expected_items()
    has_tlas = len(items) > 0
    tlas_order = walk(dec, int(root), claimed, rep, "TLAS") if has_tlas else []
    # BLAS roots: nobody's child, not the TLAS root
    is_child = np.zeros(dec.n, bool)
    for n in range(dec.n):
        k = int(_POP[dec.imask[n]])
        if k:
            is_child[dec.child_base[n]:dec.child_base[n] + k] = True
    roots = [int(n) for n in np.flatnonzero(~is_child) if not (has_tlas and n == root)]
    if not has_tlas and dec.n and int(root) not in roots:                             # (the traversal starts there whatever points at it: walked first)
        rep.add("I5", "BLAS", root, -1, -1, 0, "the traversal's root is some node's child"); roots.insert(0, int(root))
    # ---- every BLAS against the meshes ----
    want = [(_tree_records(t, scene.meshes), t) for t in scene.expected_trees()]
    taken = [False] * len(want)
    tri_refs = np.zeros(len(tris), np.int64)
    for r in roots:
        name = "BLAS@%d" % r; rep.trees += 1
        order = walk(dec, r, claimed, rep, name)
        got = []                                                                       # the tree's items, in any order: which records does it hold?
        for n in order:
            k = int(_POP[dec.lmask[n]]); got += range(int(dec.item_base[n]), int(dec.item_base[n]) + k)
        got = np.array([i for i in got if i < len(tris)], np.int64)
        rec = tris[got]
        key = rec[:, [11, 9, 10]]                                                      # pad (owner), geo, prim
        srt = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))
        match = None
        for j, ((wk, ww), t) in enumerate(want):
            if not taken[j] and len(wk) == len(key) and np.array_equal(wk, key[srt]) and np.array_equal(ww, rec[srt][:, :9]):
                match = j; break
        if match is None:
            rep.add("I5", name, r, -1, -1, len(key), "its %d records are not, bit for bit and once each, the triangles of any mesh list of the scene" % len(key))
            np.add.at(tri_refs, got, 1)
            continue
        taken[match] = True
        # leaf bounds from the MESH arrays (the records equal them bit for bit)
        leaf_lo = np.full((len(tris), 3), np.nan); leaf_hi = np.full((len(tris), 3), np.nan)
        (wk, ww), t = want[match]
        lo, hi = finite_bounds(ww.view(np.float32).reshape(-1, 3, 3))
        leaf_lo[got[srt]] = lo; leaf_hi[got[srt]] = hi
        check_tree(dec, order, claimed, leaf_lo, leaf_hi, tri_refs, rep, name, margin=True, fresh=True)
    for j, ((wk, ww), t) in enumerate(want):
        if not taken[j]:
            rep.add("I5", "BLAS", -1, -1, -1, len(wk), "no tree holds the %d triangles of mesh list %s" % (len(wk), sorted(t.items())))
    if fresh:
        for i in np.flatnonzero(tri_refs != 1)[:8]:
            rep.add("I5", "BLAS", -1, -1, -1, tri_refs[i], "TriRec %d is referenced by %d leaf slots" % (i, tri_refs[i]))
    else:
        for i in np.flatnonzero(tri_refs > 1)[:8]:
            rep.add("I5", "BLAS", -1, -1, -1, tri_refs[i], "TriRec %d is referenced by %d leaf slots" % (i, tri_refs[i]))
    # ---- the TLAS against the instances' world-space vertices ----
    if sorted(items.tolist()) != sorted(want_items):
        rep.add("I5", "TLAS", root, -1, -1, len(items), "TLAS items %s, the scene's visible instances with finite transforms are %s" % (sorted(items.tolist())[:12], sorted(want_items)[:12]))
    if has_tlas:
        rep.trees += 1
        n_inst = len(scene.instances)
        leaf_lo = np.full((len(items), 3), np.nan); leaf_hi = np.full((len(items), 3), np.nan); strict = np.zeros(len(items), bool)
        for it, inst in enumerate(items.tolist()):
            if inst > n_inst or (inst < n_inst and inst not in want_items):
                continue
            W = world[inst] if (world is not None and inst < len(world)) else scene.world_vertices(inst)
            leaf_lo[it], leaf_hi[it] = finite_bounds(W)
            strict[it] = inst == n_inst or scene.identity(inst)
        item_refs = np.zeros(len(items), np.int64)
        check_tree(dec, tlas_order, claimed, leaf_lo, leaf_hi, item_refs, rep, "TLAS", margin=not refit, fresh=fresh and not refit, strict_items=strict, widen=True)
        for i in np.flatnonzero(item_refs != 1)[:8]:
            rep.add("I5", "TLAS", -1, -1, -1, item_refs[i], "TLAS item %d (instance %d) is referenced by %d leaf slots" % (i, items[i], item_refs[i]))
    return rep


def assert_clean(rep, planted, what):
    """no violation, and nothing passed over but the `planted` all-non-finite triangles"""
    print(what, str(rep).split("\n")[0])
    assert not rep.violations, "%s: %s" % (what, rep)
    assert rep.skipped_leaf_slots == planted and planted <= 1 and rep.skipped_internal_slots == 0, "%s: %d leaf slots passed over, %d planted: %s" % (what, rep.skipped_leaf_slots, planted, rep)
    assert rep.slots["I1"] > 0

"""The acceleration structure held as a STRUCTURE, not through rays (tests/bvh_audit.py: containment, the grown-box margin, tightness, the grid rules, coverage).

Every other GPU test sees the tree through the planes its rays happen to graze; a plane too tight where no ray passes, or a builder that stops culling, renders
the same film.  Here every used slot of every reachable node of what MsneReadBvh returns is held against bounds computed from the test's own vertex arrays.

The first half runs without a GPU: a small reference builder (median splits into <= 8 children, one triangle per leaf, quantised in numpy float32 from the words
of DESIGN.md section 3) emits Node8 / TriRec bytes the auditor must pass, and single mutations of them it must report under the right invariant.  The second half
audits what the product builds and re-fits on the GPU.  Both halves and the builder-variant worker draw their soups from tests/parity_scenes.py."""
import numpy as np
import pytest

import bvh_audit
from bvh_audit import SceneRecorder, assert_clean, audit
from parity_common import run_worker
from parity_scenes import build_case, grey, soup

f32 = np.float32


# ---------------- the reference builder (CPU) ----------------

def _tri_boxes(T):
    V = np.where(np.abs(T) < f32(3.4e38), T, f32(np.nan)).astype(f32)
    return np.fmin.reduce(V, axis=1), np.fmax.reduce(V, axis=1)


def ref_build(T, growth=1e-4, origin_on_face=False):
    """median splits into <= 8 children, one triangle per leaf; children and items numbered contiguously in slot order; the grid and the planes in float32 as
    DESIGN.md section 3 words them: per axis the smallest power-of-two quantum greater than extent / 252, no axis finer than a quarter of the coarsest, the origin
    one quantum below the lower face, every child box grown by 1e-4 of its largest extent, then rounded outward by at least 1e-3 quantum.  -> (nodes (m, 80) uint8,
    tris (n, 12) uint32)"""
    T = np.asarray(T, f32); n = len(T)
    lo, hi = _tri_boxes(T)
    cen = (lo + hi) * f32(0.5)

    def split(idx, parts):
        if parts == 1 or len(idx) == 1:
            return [idx]
        c = cen[idx]
        with np.errstate(invalid="ignore"):
            span = np.fmax.reduce(c, axis=0) - np.fmin.reduce(c, axis=0)
        ax = int(np.argmax(np.nan_to_num(span, nan=-1.0)))
        order = idx[np.argsort(c[:, ax], kind="stable")]                               # (NaN centres sort last)
        h = len(order) // 2
        return split(order[:h], parts // 2) + split(order[h:], parts // 2)

    nodes = [None]; items = []
    queue = [(0, np.arange(n))]
    while queue:
        at, idx = queue.pop(0)
        groups = split(idx, 8)
        nd = np.zeros(80, np.uint8)
        qlo = np.full((3, 8), 255, np.uint8); qhi = np.zeros((3, 8), np.uint8)
        cl = np.stack([np.fmin.reduce(lo[g], axis=0) for g in groups]); ch = np.stack([np.fmax.reduce(hi[g], axis=0) for g in groups])
        nl = np.fmin.reduce(cl, axis=0); nh = np.fmax.reduce(ch, axis=0)
        e = np.ones(3, np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            ext = (nh - nl).astype(f32)
            for k in range(3):
                if ext[k] > 0:
                    q = f32(ext[k] / f32(252.0))
                    e[k] = min(max(int((np.array(q, f32).view(np.uint32) >> 23) & 0xff) + 1, 1), 254)
            e = np.maximum(e, e.max() - 2)
            Q = np.ldexp(f32(1.0), e - 127).astype(f32)
            origin = nl.copy() if origin_on_face else (nl - Q).astype(f32)
            inv = np.ldexp(f32(1.0), 127 - e).astype(f32)
            imask = lmask = 0
            child_base = len(nodes); item_base = len(items)
            for s, g in enumerate(groups):
                gext = (ch[s] - cl[s]).astype(f32).max()
                grow = f32(growth) * gext if (gext > 0 and gext < 3.0e38) else f32(0.0)
                a = np.floor((((cl[s] - grow).astype(f32) - origin).astype(f32) * inv).astype(f32) - f32(1e-3))
                b = np.ceil((((ch[s] + grow).astype(f32) - origin).astype(f32) * inv).astype(f32) + f32(1e-3))
                qlo[:, s] = np.nan_to_num(np.clip(a, 0, 255), nan=0.0).astype(np.uint8); qhi[:, s] = np.nan_to_num(np.clip(b, 0, 255), nan=0.0).astype(np.uint8)
                if len(g) == 1:
                    lmask |= 1 << s; items.append(int(g[0]))
                else:
                    imask |= 1 << s; nodes.append(None); queue.append((len(nodes) - 1, g))
        nd[0:12] = origin.astype(f32).view(np.uint8); nd[12:15] = e.astype(np.uint8); nd[15] = imask
        nd[16:20] = np.array([child_base if imask else 0], np.uint32).view(np.uint8); nd[20:24] = np.array([item_base], np.uint32).view(np.uint8)
        nd[24] = lmask; nd[32:56] = qlo.reshape(-1); nd[56:80] = qhi.reshape(-1)
        nodes[at] = nd
    tris = np.zeros((n, 12), np.uint32)
    for j, t in enumerate(items):
        tris[j, :9] = T[t].reshape(9).view(np.uint32); tris[j, 10] = t
    return np.stack(nodes), tris


class _NoContext:
    """hands out handles and nothing else"""
    def __init__(self):
        self.n = {}

    def _next(self, what):
        self.n[what] = self.n.get(what, -1) + 1; return self.n[what]

    def create_mesh(self, *a, **k):
        return self._next("mesh")

    def create_instance(self, *a, **k):
        return self._next("instance")


def cpu_scene(T):
    sc = SceneRecorder(_NoContext())
    sc.create_instance([(sc.create_mesh(T.reshape(-1, 3), np.arange(3 * len(T), dtype=np.uint32).reshape(-1, 3)), 0, False)])
    return sc


def cpu_audit(nodes, tris, T):
    return audit((nodes, tris, 0, np.zeros(0, np.uint32)), cpu_scene(T))


CPU_SOUPS = ["1", "8", "9", "257", "4097", "257-flat", "257-far"]
_built = {}


def cpu_tree(name):
    """the reference builder's tree of a named soup, built once and handed out as copies"""
    if name not in _built:
        T, planted = soup(int(name.partition("-")[0]), name.partition("-")[2])
        _built[name] = (T, planted) + ref_build(T)
    T, planted, nodes, tris = _built[name]
    return T, planted, nodes.copy(), tris.copy()


@pytest.mark.parametrize("name", CPU_SOUPS)
def test_auditor_passes_the_reference_builder(name):
    T, planted, nodes, tris = cpu_tree(name)
    rep = cpu_audit(nodes, tris, T)
    assert_clean(rep, planted, "reference tree " + name)
    assert rep.nodes == len(nodes) and rep.nodes_i4 == len(nodes) and rep.slots["I2"] == rep.slots["I1"] == rep.slots["I3"]
    assert rep.slots["I1"] == len(T) - planted + len(nodes) - 1                       # every triangle's slot and every internal slot was held, but the NaN triangle's


def _leaf_slot(nodes, tris, want=lambda node, s: True):
    """(node, slot, item) of a leaf slot that `want`s and whose triangle is finite, deepest nodes first"""
    for n in range(len(nodes) - 1, -1, -1):
        lo, hi, imask, lmask, cb, ib = bvh_audit.boxes(nodes[n])
        li = 0
        for s in range(8):
            if (lmask >> s) & 1:
                if want(nodes[n], s) and np.isfinite(tris[ib + li, :9].view(f32)).all():
                    return n, s, ib + li
                li += 1
    raise AssertionError("no such slot")


def _at(rep, inv, node):
    return [v for v in rep.violations if v.invariant == inv and v.node == node]


def test_mutation_lower_plane_raised_across_the_bounds_is_I1():
    T, _, nodes, tris = cpu_tree("257")
    n, s, item = _leaf_slot(nodes, tris, lambda nd, s: nd[32 + s] < 250)
    blo = _tri_boxes(tris[item, :9].view(f32).reshape(1, 3, 3))[0][0]
    while bvh_audit.boxes(nodes[n])[0][0, s] <= blo[0]:
        nodes[n][32 + s] += 1                                                          # qlo[x][s]
    rep = cpu_audit(nodes, tris, T)
    hit = _at(rep, "I1", n)
    assert hit and all((v.slot, v.axis) == (s, 0) for v in hit), str(rep)
    assert set(rep.invariants()) <= {"I1", "I2"}, str(rep)   # (a plane inside the bounds has no margin either)


def needle_scene():
    """three triangles in z = 0 on a 200 x 200 node (quantum 1, origin -1): a 2000 : 1 needle whose lower y face lies 2e-3 quantum above a grid plane.  Grown by
    g = 1e-4 * 200 = 0.02 it rounds down a whole quantum; ungrown, its plane stays 2e-3 quantum below it — less than g"""
    return np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]],
                     [[199, 200, 0], [200, 200, 0], [200, 199, 0]],
                     [[0, 50.002, 0], [200, 50.102, 0], [200, 50.05, 0]]], f32)


def test_mutation_growth_zero_is_I2():
    T = needle_scene()
    nodes, tris = ref_build(T)
    assert_clean(cpu_audit(nodes, tris, T), 0, "needle scene")
    nodes0, tris0 = ref_build(T, growth=0.0)
    rep = cpu_audit(nodes0, tris0, T)
    assert rep.invariants() == ["I2"], str(rep)
    v = [v for v in rep.violations if v.axis == 1 and "lower" in v.what]
    assert len(v) == 1 and abs(v[0].amount - (0.02 + 1e-3 - 0.002)) < 1e-4, str(rep)   # the needle's lower y plane: 0.002 outside, g + 1e-3 Q wanted
    # and in a soup, where nothing was constructed: some slot's margin is below its g
    T, _, nodes, tris = cpu_tree("4097")
    rep = cpu_audit(*ref_build(T, growth=0.0), T)
    assert rep.invariants() == ["I2"] and len(rep.violations) > 10, str(rep)


def test_mutation_plane_lowered_by_three_is_I3():
    T, _, nodes, tris = cpu_tree("257")
    n, s, item = _leaf_slot(nodes, tris, lambda nd, s: nd[32 + 8 + s] >= 3)
    nodes[n][32 + 8 + s] -= 3                                                          # qlo[y][s]
    rep = cpu_audit(nodes, tris, T)
    assert rep.invariants() == ["I3"] and [(v.node, v.slot, v.axis) for v in rep.violations] == [(n, s, 1)], str(rep)


def test_mutation_exponent_plus_one_is_I4():
    T, _, nodes, tris = cpu_tree("257")
    n = len(nodes) // 2
    k = int(np.argmax(nodes[n][12:15]))
    nodes[n][12 + k] += 1
    rep = cpu_audit(nodes, tris, T)
    hit = _at(rep, "I4", n)
    assert hit and any(v.axis == k and "coarser" in v.what for v in hit), str(rep)
    assert all(v.node == n for v in rep.violations), str(rep)


def test_mutation_origin_on_the_lower_face_is_I4():
    T, _, nodes, tris = cpu_tree("257")
    rep = cpu_audit(*ref_build(T, origin_on_face=True), T)
    hit = [v for v in rep.violations if v.invariant == "I4"]
    assert len(hit) >= 3 * len(nodes) - 3 and all("origin" in v.what for v in hit), str(rep)
    assert "I1" not in rep.invariants() and "I3" not in rep.invariants(), str(rep)      # (the planes on the face still contain; they have lost their margin: I2)


def test_mutation_leaf_bit_cleared_is_I5():
    T, _, nodes, tris = cpu_tree("257")
    n, s, item = _leaf_slot(nodes, tris)
    lmask = int(nodes[n][24])
    top = max(b for b in range(8) if (lmask >> b) & 1)                                   # the node's last leaf: nobody's numbering moves
    nodes[n][24] = lmask & ~(1 << top)
    last = int(nodes[n][20:24].view(np.uint32)[0]) + bin(lmask).count("1") - 1
    rep = cpu_audit(nodes, tris, T)
    assert rep.invariants() == ["I5"], str(rep)
    assert any("matches" in v.what or "not, bit for bit" in v.what for v in rep.violations), str(rep)   # the tree no longer covers its mesh
    assert any(("TriRec %d is referenced by 0" % last) in v.what for v in rep.violations), str(rep)


def test_mutation_two_slots_with_the_same_item_is_I5():
    T, _, nodes, tris = cpu_tree("257")
    n, s, item = _leaf_slot(nodes, tris)
    m, s2, item2 = _leaf_slot(nodes, tris, lambda nd, s_: int(nd[20:24].view(np.uint32)[0]) != int(nodes[n][20:24].view(np.uint32)[0]))
    nodes[m][20:24] = nodes[n][20:24]                                                  # node m's leaves now name node n's items
    rep = cpu_audit(nodes, tris, T)
    assert "I5" in rep.invariants() and any("not, bit for bit" in v.what for v in rep.violations), str(rep)


def test_mutation_overlapping_child_ranges_is_I5():
    T, _, nodes, tris = cpu_tree("4097")
    inner = [n for n in range(1, len(nodes)) if nodes[n][15]]
    a, b = inner[0], inner[-1]
    nodes[b][16:20] = nodes[a][16:20]
    rep = cpu_audit(nodes, tris, T)
    assert any(v.invariant == "I5" and "reached before" in v.what for v in rep.violations), str(rep)


def test_mutation_imask_and_lmask_overlap_is_I5():
    T, _, nodes, tris = cpu_tree("257")
    n = next(n for n in range(len(nodes)) if nodes[n][15])
    bit = int(nodes[n][15]) & -int(nodes[n][15])
    nodes[n][24] |= bit
    rep = cpu_audit(nodes, tris, T)
    assert any(v.invariant == "I5" and v.node == n and "imask & lmask" in v.what for v in rep.violations), str(rep)


def test_mutation_child_base_at_an_ancestor_is_I5_and_terminates():
    T, _, nodes, tris = cpu_tree("257")
    n = max(n for n in range(len(nodes)) if nodes[n][15])                              # the last node with children: its child_base now names the root
    nodes[n][16:20] = np.array([0], np.uint32).view(np.uint8)
    rep = cpu_audit(nodes, tris, T)
    assert any(v.invariant == "I5" and v.node == n and "cycle" in v.what for v in rep.violations), str(rep)


# ---------------- the product's trees (GPU) ----------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 64, 65, 255, 256, 257, 513, 4097, 16385])
def test_gpu_soup_trees(gpu_api, n):
    """one mesh, one identity instance: the world BLAS is the whole structure.  4097 is the smallest n at which the default build hands 4096 clusters to the top
    stage, 16385 one past the sweep's super-tile.  I1-I5."""
    rec = SceneRecorder(gpu_api.Context())
    planted = build_case(rec, str(n))
    rep = audit(rec.read_bvh(), rec)
    assert_clean(rep, planted, "soup %d" % n)
    assert rep.slots["I2"] == rep.slots["I1"] == rep.slots["I3"] and rep.nodes_i4 == rep.nodes


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["flat", "far", "tiny", "huge", "point", "needle"])
def test_gpu_degenerate_and_edge_trees(gpu_api, family):
    """257 triangles: all in z = 0 (the quarter-of-the-coarsest rule on every node), translated by 1e4 times the soup's size (where tau decides), times 1e-20 and
    1e20, with a point triangle (g = 0), with a 2000 : 1 needle.  I1-I5."""
    rec = SceneRecorder(gpu_api.Context())
    planted = build_case(rec, "257-" + family)
    rep = audit(rec.read_bvh(), rec)
    assert_clean(rep, planted, "soup 257 " + family)
    assert rep.slots["I2"] == rep.slots["I1"] == rep.slots["I3"] and rep.nodes_i4 == rep.nodes


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["MSNE_SAH_TOP=48", "MSNE_SAH_TOP=0", "MSNE_TOPDOWN=host", "MSNE_MORTON_BITS=21"])
def test_gpu_builder_variants(env):
    """the builder's other routes (read from the environment when a context is made, hence a process of their own: tests/workers/bvh_audit_variants.py): PLOC, cluster
    rebuilds and a top tree in every mesh and in the TLAS; PLOC alone; the top-down stages on the host; 63-bit Morton keys.  Soups of 257 and 4097 triangles and the
    instanced S2, I1-I5 each."""
    k, _, v = env.partition("=")
    run_worker("bvh_audit_variants", env={"MSNE_DEBUG_POISON": "1", k: v}, timeout=300, token="AUDIT_OK")


@pytest.mark.gpu
def test_gpu_instanced_s2(gpu_api):
    """18 rotated and scaled instances of one icosphere, a ground quad and a lamp as identity instances (the world BLAS, one item of the TLAS): every BLAS I1-I5,
    the TLAS I1 and I5 — and I2-I4 where everything under a slot is untransformed"""
    rec = SceneRecorder(gpu_api.Context())
    build_case(rec, "s2")
    rep = audit(rec.read_bvh(), rec)
    assert_clean(rep, 0, "s2")
    assert rep.trees == 3 and rep.slots["I2"] >= 1


@pytest.mark.gpu
def test_gpu_identity_instances_share_one_world_tree(gpu_api):
    """27 untransformed instances of an icosphere set out on a 3 x 3 x 3 grid: ONE world BLAS, every record's owner in TriRec::pad"""
    from moonshine_amd import scenes
    rec = SceneRecorder(gpu_api.Context())
    P, I = scenes.icosphere(1)
    mat = grey(rec)
    for k in range(27):
        rec.create_instance([(rec.create_mesh((P + f32(2.5) * np.array([k % 3, (k // 3) % 3, k // 9], f32)).astype(f32), I), mat, False)])
    rec.set_background(np.ones((1, 1, 4), f32), 1, 1)
    bvh = rec.read_bvh()
    rep = audit(bvh, rec)
    assert_clean(rep, 0, "27 identity instances")
    assert rep.trees == 1 and len(bvh[3]) == 0
    assert sorted(set(bvh[1][:, 11].tolist())) == list(range(27))


HULL_SEEDS = [0, 1, 2, 14, 501, 707, 910, 6709891, 6711985]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,baked", [(s, False) for s in HULL_SEEDS] + [(2, True), (14, True)])
def test_gpu_hull_scenes_built_and_refitted(gpu_api, seed, baked):
    """tests/hull_rays.py's instances (scaled 1e-3 ... 1e3 per axis, sheared, carried up to 3e4 away): every BLAS I1-I5 and the TLAS I1 and I5 after the build,
    and again after each of the two batches of transform edits (tools/tlas_check.py by hand, once)"""
    import hull_rays
    rec = SceneRecorder(gpu_api.Context())
    parts = []
    world = hull_rays.hull_scene(rec, seed, seed % 2 == 1, parts, baked)
    assert_clean(audit(rec.read_bvh(), rec, world=world), 0, "hull scene %d built" % seed)
    if baked:
        return
    for step in (0, 5):
        hull_rays.hull_move((rec,), seed + step, parts, world)
        assert_clean(audit(rec.read_bvh(), rec, refit=True, world=world), 0, "hull scene %d moved (%d)" % (seed, step))


@pytest.mark.gpu
def test_gpu_refits_of_three_hundred_instances(gpu_api):
    """300 small instances on a jittered grid, ten batches of 1, 65 or 256 transform edits (256 is the most a scene of 300 re-fits in place): jitters, moves to 8
    times the scene's radius (a child leaves its node's grid: the grid is re-made) and moves back (the child fits a grid that stays coarse).  Every batch must take
    the refit route, and the TLAS must hold I1 and I5 after it."""
    from moonshine_amd import scenes
    rs = np.random.default_rng(300)
    rec = SceneRecorder(gpu_api.Context())
    P, I = scenes.icosphere(0)
    mesh = rec.create_mesh(P, I); mat = grey(rec)

    def place(t):
        T = np.zeros((3, 4), f32)
        T[:, :3] = scenes._rot(rs.normal(size=3), rs.uniform(0, 6.28))[:3, :3] * rs.uniform(0.05, 0.2); T[:, 3] = t
        return T
    home = np.array([[x, y, z] for z in range(3) for y in range(10) for x in range(10)], np.float64) + rs.uniform(-0.3, 0.3, (300, 3))
    for k in range(300):
        rec.create_instance([(mesh, mat, False)], transform=place(home[k]))
    rec.set_background(np.ones((1, 1, 4), f32), 1, 1)
    assert_clean(audit(rec.read_bvh(), rec), 0, "300 instances built")
    radius = float(max(np.abs(rec.world_vertices(k)).max() for k in range(300)))
    away = set()
    for r in range(10):
        count = (1, 65, 256)[(r + r // 3) % 3]; kind = ("jitter", "far", "back")[r % 3]
        st0 = rec.accel_stats()
        if kind == "far":
            batch = rs.choice(sorted(set(range(300)) - away), count, replace=False); away |= set(batch.tolist())
        elif kind == "back":
            back = sorted(away)[:count]; away -= set(back)
            batch = np.array(back + rs.choice(sorted(set(range(300)) - away - set(back)), count - len(back), replace=False).tolist())
        else:
            batch = rs.choice(300, count, replace=False)
        for k in batch.tolist():
            if k in away:
                t = rs.choice([-1.0, 1.0], 3) * rs.uniform(0.5, 1.0, 3) * 8.0 * radius
                t[int(rs.integers(3))] = 8.0 * radius * float(rs.choice([-1.0, 1.0]))
            else:
                t = home[k] + rs.uniform(-0.3, 0.3, 3)
            rec.set_instance_transform(k, place(t))
        rep = audit(rec.read_bvh(), rec, refit=True)
        st1 = rec.accel_stats()
        assert (st1["tlas_updates"] - st0["tlas_updates"], st1["rebuilds"] - st0["rebuilds"]) == (1, 0), "round %d (%s, %d edits): %s -> %s" % (r, kind, count, st0, st1)
        assert_clean(rep, 0, "300 instances, round %d (%s, %d edits)" % (r, kind, count))

"""usage: sweep_vs_host.py ORDER — every scene built twice by the shipped library, with the builder's top-down stages on the host ($MSNE_TOPDOWN=host) and on the
GPU: the same wide nodes (compared by a hash of each node's whole subtree) and the same films.  S1 at icosphere order ORDER, the instanced S2, a batch of 40
meshes, the pile and the chain; with ORDER 4 the triangle soups as well.  Prints SWEEP_OK."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from moonshine_amd import api, scenes
from parity_scenes import many_meshes, pile, soup_scene


def tree_hashes(c):
    # every wide node as a hash of what the traversal sees of it — grid, masks, child planes, its leaf items' records and, in slot order, its children's hashes — i.e.
    # of its whole subtree whatever the node numbering (k_collapse hands node indices out with atomics).  Children are allocated after their parents: descending order.
    nodes, tris, root, items = c.read_bvh()
    h = [None] * len(nodes)
    pc = lambda x: bin(int(x)).count("1")
    tlas = np.zeros(len(nodes), bool)               # nodes of the TLAS (their leaves index the instance list): reachable from the root when there is an instance list
    if len(items) and root < len(nodes):
        stack = [root]
        while stack:
            i = stack.pop(); tlas[i] = True
            cb = int(nodes[i][16:20].view(np.uint32)[0])
            stack += [cb + k for k in range(pc(nodes[i][15]))]
    for i in range(len(nodes) - 1, -1, -1):
        nd = nodes[i]
        cb, ib = int(nd[16:20].view(np.uint32)[0]), int(nd[20:24].view(np.uint32)[0])
        m = hashlib.sha1(nd[0:16].tobytes() + nd[24:25].tobytes() + nd[32:80].tobytes())
        for k in range(pc(nd[15])):
            m.update(h[cb + k])
        for k in range(pc(nd[24])):
            m.update(items[ib + k].tobytes() if tlas[i] else tris[ib + k].tobytes())
        h[i] = m.digest()
    return sorted(h), len(nodes)


order = int(sys.argv[1])
cases = [("soup%d" % n, soup_scene(n), dict(extent=(32, 32))) for n in ((1, 2, 3, 7, 255, 256, 257, 513, 16383, 16385, 33000) if order == 4 else ())] + [
         ("s1", scenes.s1, dict(extent=(48, 27), grid=2, order=order)), ("s2", scenes.s2, dict(extent=(48, 27), dims=(4, 4, 3), order=3)),
         ("meshes", many_meshes, dict(extent=(48, 27))), ("pile", pile, dict(extent=(16, 16)))]
for name, builder, kw in cases:
    got = {}
    for where in ("host", "gpu"):
        os.environ["MSNE_TOPDOWN"] = where
        c = api.Context()
        s, l = builder(c, **kw)
        c.set_pipeline(samples_per_run=1, max_bounces=4, env_samples_per_bounce=1, mesh_samples_per_bounce=1)
        c.render(s, l, launches=2)
        got[where] = (tree_hashes(c), c.sensor_data(s).copy())
    (hh, nh), (hg, ng) = got["host"][0], got["gpu"][0]
    assert nh == ng, "%s: %d nodes from the host stages, %d from the GPU's" % (name, nh, ng)
    assert hh == hg, "%s: %d of %d subtrees differ" % (name, sum(a != b for a, b in zip(hh, hg)), nh)
    assert np.array_equal(got["host"][1].view(np.uint32), got["gpu"][1].view(np.uint32)), name + ": films differ"
    print(name, nh, "nodes equal")
print("SWEEP_OK")

"""usage (GPU box): python tools/tlas_check.py SEED — the acceleration structure of tests/hull_rays.py's scene as the product holds it (MsneReadBvh), after the build and
after each re-fit of tests/test_gpu_parity.py::test_rays_at_the_hulls_...: every slot of every node held against the vertices under it by tests/bvh_audit.py (the TLAS
against the instances' world-space vertices, every BLAS against its meshes).  Prints every violation (invariant, tree, node, slot, axis, by how much)."""
import sys; sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import numpy as np
np.set_printoptions(precision=6, linewidth=200)
import moonshine_amd.api as api
import hull_rays
from bvh_audit import SceneRecorder, audit


def check(gc, world, tag, refit):
    nodes, tris, root, items = bvh = gc.read_bvh()
    rep = audit(bvh, gc, refit=refit, world=world)
    for v in rep.violations:
        print(tag, "%s %s node %d slot %d axis %d by %g: %s" % v)
    print(tag, "TLAS root", root, "instances reached", sorted(items.tolist()), "violations", len(rep.violations), str(rep).split("\n")[0], "accel", gc.accel_stats(), flush=True)


seed = int(sys.argv[1])
gc = SceneRecorder(api.Context())   # keeps the meshes and the transforms the audit holds the trees against
harsh = seed % 2 == 1; baked = seed % 3 == 2
parts = []
world = hull_rays.hull_scene(gc, seed, harsh, parts, baked)
gc.create_sensor(8, 8)
gc.trace_rays(hull_rays.hull_rays(world, seed)); check(gc, world, "built", False)
hull_rays.hull_move((gc,), seed, parts, world)
gc.trace_rays(hull_rays.hull_rays(world, seed + 1)[::2]); check(gc, world, "moved", True)
hull_rays.hull_move((gc,), seed + 5, parts, world)
gc.trace_rays(hull_rays.hull_rays(world, seed + 2, far=1.0)[::3]); check(gc, world, "moved2", True)

"""What the parity tests, the tools that explain their failures and the worker processes (tests/workers/) share: a scene built on both sides, the film and ray-count
comparisons, probe rays against the oracle's hit records, and the start of a worker process."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAY_COUNTERS = ("closest_rays", "shadow_rays", "samples")


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


def assert_film_equal(gpu_img, orc_img, what):
    g, o = gpu_img[..., :3], orc_img[..., :3]
    l2 = rel_l2(g, o)
    nbad = int((g.view(np.uint32) != o.view(np.uint32)).any(axis=-1).sum())
    assert l2 < 1e-4, "%s: relative L2 %g" % (what, l2)
    assert nbad == 0, "%s: %d pixels differ bitwise (rel L2 %g, max abs %g)" % (what, nbad, l2, float(np.abs(g - o).max()))
    assert np.array_equal(gpu_img[..., 3], orc_img[..., 3]), "%s: alpha (launch count) differs" % what


def assert_same_bits(go, oo, what):
    """every value of the two films equal as uint32, or NaN in both (all four channels; no bound on a norm: that is assert_film_equal)"""
    same = (go.view(np.uint32) == oo.view(np.uint32)) | (np.isnan(go) & np.isnan(oo))
    assert same.all(), "%s: %d values differ (%d pixels)" % (what, int((~same).sum()), int((~same).any(-1).sum()))


def assert_same_ray_counts(gc, oc, what=""):
    """the product counts closest-hit rays, shadow rays and samples; the oracle counts more, and those three must be the product's"""
    g, o = gc.counters(), {k: v for k, v in oc.counters().items() if k in RAY_COUNTERS}
    assert g == o, "%sray counts differ: %s, the oracle's %s" % (what and what + ": ", g, o)


def both(orc, gpu_api, builder, **kw):
    oc = orc.Context(threads=8)
    gc = gpu_api.Context()
    so, lo = builder(oc, **kw)
    sg, lg = builder(gc, **kw)
    return oc, so, lo, gc, sg, lg


def random_rays(n, seed, radius=4.0):
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * radius
    tgt = rng.normal(size=(n, 3)) * 0.7
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 7), np.float32)
    rays[:, :3] = o; rays[:, 3:6] = d; rays[:, 6] = 1e12
    return rays


def check_rays(oc, gc, rays):
    ids, tuv = gc.trace_rays(rays, any_hit=False)
    occ, _ = gc.trace_rays(rays, any_hit=True)
    for k in range(len(rays)):
        hit, oid, otuv = oc.trace_closest(rays[k, :3], rays[k, 3:6], float(rays[k, 6]))
        assert bool(ids[k, 0]) == hit, "ray %d hit flag" % k
        if hit:
            assert tuple(ids[k, 1:4]) == tuple(oid), "ray %d ids %s vs %s" % (k, ids[k, 1:4], oid)
            assert np.array_equal(tuv[k].view(np.uint32), otuv.view(np.uint32)), "ray %d tuv %s vs %s" % (k, tuv[k], otuv)
        assert bool(occ[k, 0]) == oc.trace_shadow(rays[k, :3], rays[k, 3:6], float(rays[k, 6])), "ray %d occlusion" % k


def run_worker(name, *args, token, timeout, env=None):
    """tests/workers/<name>.py in a process of its own (a second library, or a builder route that is read from the environment when a context is made): it must
    exit with 0 and print `token`.  -> the completed process"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "workers", name + ".py")] + [str(a) for a in args],
                         capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    assert out.returncode == 0 and token in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return out

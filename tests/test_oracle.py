"""CPU tests (-m "not gpu"): the oracle against the reference's own pins and the committed golden vectors.

Pins available for this path: the reference's furnace tests (engine/tests.zig:257-455), run here
at the reference's exact parameters and tolerances, and the integer-exact PCG answers.  Everything else the
reference leaves untested; for those the golden files freeze the oracle's restatement of Appendix A.
"""
import json
import math
import os

import numpy as np
import pytest

from moonshine_amd import scenes
from moonshine_amd.hostinfo import usable_cores
from parity_common import random_rays
from parity_scenes import random_scene
from seeds import seeds

G = os.path.join(os.path.dirname(__file__), "golden")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_pcg_known_answers(orc):
    d = json.load(open(os.path.join(G, "rng.json")))
    # SURVEY.md Appendix A.1 (random.hlsl:8-46, integer-exact)
    assert orc.pcg(0) == 0x07bb2fe2 and orc.pcg(1) == 0xa8beea3c and orc.pcg(0xFFFFFFFF) == 0xe62a4902
    st, f = orc.rng_floats(0, 0, 0, 4)
    assert st == 0x7fddb461 and [int(x * 2 ** 24) for x in f] == [9253448, 10386727, 5161806, 1356166]
    st, f = orc.rng_floats(5, 1919, 1079, 4)
    assert st == 0xa704cf68 and [int(x * 2 ** 24) for x in f] == [9975394, 12244545, 12969628, 11018050]
    for s in d["streams"]:
        st, f = orc.rng_floats(*s["seed"], 16)
        assert st == s["state0"] and [int(x * 2 ** 24) for x in f] == s["h_shr8"]
        assert np.all((f >= 0) & (f < 1))


def test_math_golden_and_accuracy(orc):
    m = np.load(os.path.join(G, "math.npz"))
    assert np.array_equal(bits(orc.math_probe("sin", m["xs"])), bits(m["sin"]))
    assert np.array_equal(bits(orc.math_probe("cos", m["xs"])), bits(m["cos"]))
    assert np.array_equal(bits(orc.math_probe("log", m["x01"])), bits(m["log"]))
    assert np.array_equal(bits(orc.math_probe("atan2", m["atan2_in"])), bits(m["atan2"]))
    # the from-scratch transcendentals are as accurate as a libm: <= 2 ulp-ish absolute error on the ranges the path uses
    x = np.linspace(-1, 7, 20001).astype(np.float32)
    assert np.abs(orc.math_probe("sin", x) - np.sin(x.astype(np.float64))).max() < 2.5e-7
    assert np.abs(orc.math_probe("cos", x) - np.cos(x.astype(np.float64))).max() < 2.5e-7
    u = np.linspace(1e-7, 0.99, 20001).astype(np.float32)
    assert np.abs(orc.math_probe("log", u) / np.log(u.astype(np.float64)) - 1).max() < 3e-7
    a = np.linspace(-1, 1, 20001).astype(np.float32)
    assert np.abs(orc.math_probe("acos", a) - np.arccos(a.astype(np.float64))).max() < 6e-7
    assert orc.math_probe("log", np.float32([1.0]))[0] == 0.0


def test_equal_area_sphere_roundtrip(orc):
    m = np.load(os.path.join(G, "math.npz"))
    sph = orc.square_to_equal_area_sphere(m["grid"])
    assert np.array_equal(bits(sph), bits(m["sphere"]))
    assert np.array_equal(bits(orc.square_to_equal_area_sphere_inverse(sph)), bits(m["sphere_inv"]))
    rs = np.random.default_rng(3)
    uv = rs.random((4000, 2)).astype(np.float32)
    d = orc.square_to_equal_area_sphere(uv)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6            # on the unit sphere (mappings.hlsl:67-83)
    assert np.abs(orc.square_to_equal_area_sphere_inverse(d) - uv).max() < 2e-6   # inverse (mappings.hlsl:85-99)
    assert abs(d[:, 2].mean()) < 0.03                                     # equal-area: z uniform in [-1,1]


def test_offset_along_normal(orc):
    m = np.load(os.path.join(G, "math.npz"))
    out = orc.offset_along_normal(m["off_p"], m["off_n"])
    assert np.array_equal(bits(out), bits(m["off_out"]))
    # math.hlsl:32-42: near the origin the offset is n/65536, elsewhere an integer ulp step away from the surface
    assert np.allclose(orc.offset_along_normal([(0, 0, 0)], [(1, 0, 0)]), [[1 / 65536, 0, 0]])
    p = orc.offset_along_normal([(1, 1, 1)], [(0, 0, 1)])[0]
    assert bits(p)[2] - bits(np.float32(1.0)) == 256 and p[0] == 1 and p[1] == 1
    q = orc.offset_along_normal([(-1, -1, -1)], [(0, 0, 1)])[0]
    assert bits(np.float32(-1.0)) - bits(q)[2] == 256      # moves towards +z also for negative coordinates


def test_alias_table_golden_and_invariants(orc):
    d = json.load(open(os.path.join(G, "alias.json")))
    for name, g in d.items():
        a, s, tot = orc.build_alias_table(g["weights"])
        assert a.tolist() == g["alias"], name
        assert [bytes(b).hex() for b in s.astype(">f4").view(np.uint8).reshape(-1, 4)] == g["select_hex"], name
        w = np.array(g["weights"], np.float64); n = len(w)
        # Vose invariant (alias_table.zig:25-92): the table reproduces the input distribution
        p = np.zeros(n)
        for i in range(n):
            sel = min(float(s[i]), 1.0)
            p[i] += sel / n
            if sel < 1.0:
                p[a[i]] += (1.0 - sel) / n
        assert np.abs(p - w / w.sum()).max() < 1e-5, name
    a, s, tot = orc.build_alias_table([1, 2, 3, 4])
    assert tot == 10.0


def test_camera_rays(orc):
    c = np.load(os.path.join(G, "camera.npz"))
    for key, lens in (("lens0", orc.make_lens((-3, 0, 0), (1, 0, 0), (0, 0, 1), math.pi / 4)), ("lens1", orc.make_lens((0, 0, 0), (1, 0, 0), (0, 0, 1), math.pi / 3))):
        rows = np.array([orc.generate_ray(lens, 32, 32, u, v) for u in (0.0, 0.5, 1.0) for v in (0.0, 0.5, 1.0)], np.float32)
        assert np.array_equal(bits(rows), bits(c[key]))
    centre = orc.generate_ray(orc.make_lens((-3, 0, 0), (1, 0, 0), (0, 0, 1), math.pi / 4), 32, 32, 0.5, 0.5)
    assert np.allclose(centre, [-3, 0, 0, 1, 0, 0], atol=1e-7)           # camera.hlsl:14-42
    corner = orc.generate_ray(orc.make_lens((-3, 0, 0), (1, 0, 0), (0, 0, 1), math.pi / 4), 32, 32, 1.0, 1.0)
    assert abs(math.atan2(corner[5], corner[3]) - math.pi / 8) < 1e-6    # top edge at vfov/2


def test_bsdf_golden_and_properties(orc):
    rows = np.load(os.path.join(G, "bsdf.npy"))
    for r in rows:
        t, met, rough = int(r[0]), float(r[1]), float(r[2])
        out = orc.bsdf_probe(t, (0.9, 0.6, 0.2), met, rough, 1.5, r[3:6], r[6:9], r[9:11])
        got = np.concatenate([[out["pdf"]], out["eval"], out["dir"], [out["sample_pdf"]]]).astype(np.float32)
        assert np.array_equal(bits(got), bits(r[11:19]))
    # Lambert: pdf integrates to 1 over the hemisphere; eval*cos/pdf == albedo (material.hlsl:137-175)
    wo = np.float32([0.3, -0.2, math.sqrt(1 - 0.13)])
    n, acc = 200, 0.0
    for i in range(n):
        for j in range(4 * n):
            th, ph = (i + 0.5) / n * math.pi / 2, (j + 0.5) / (4 * n) * 2 * math.pi
            wi = (math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th))
            acc += orc.bsdf_probe(orc.LAMBERT, (1, 1, 1), 0, 0, 1.5, wi, wo, (0.5, 0.5))["pdf"] * math.sin(th)
    assert abs(acc * (math.pi / 2 / n) * (2 * math.pi / (4 * n)) - 1.0) < 1e-3
    rs = np.random.default_rng(5)
    for _ in range(200):
        sq = rs.random(2)
        s = orc.bsdf_probe(orc.LAMBERT, (0.5, 0.25, 1.0), 0, 0, 1.5, (0, 0, 1), wo, sq)
        e = orc.bsdf_probe(orc.LAMBERT, (0.5, 0.25, 1.0), 0, 0, 1.5, s["dir"], wo, sq)["eval"]
        assert np.allclose(e * abs(s["dir"][2]) / s["sample_pdf"], [0.5, 0.25, 1.0], rtol=2e-6)
        # mirror / glass: f*|cos|/pdf == 1 (material.hlsl:313-393)
        m = orc.bsdf_probe(orc.PERFECT_MIRROR, (1, 1, 1), 0, 0, 1.5, (0, 0, 1), wo, sq)
        assert np.allclose(m["dir"], [-wo[0], -wo[1], wo[2]]) and m["sample_pdf"] == 1.0
        g = orc.bsdf_probe(orc.GLASS, (1, 1, 1), 0, 0, 1.5, (0, 0, 1), wo, sq)
        ge = orc.bsdf_probe(orc.GLASS, (1, 1, 1), 0, 0, 1.5, g["dir"], wo, sq)["eval"]
        assert np.allclose(ge * abs(g["dir"][2]) / g["sample_pdf"], 1.0, rtol=3e-6)
        # GGX/StandardPBR: sampled direction has positive pdf equal to pdf(); energy bounded
        p = orc.bsdf_probe(orc.STANDARD_PBR, (0.9, 0.6, 0.2), 0.7, 0.4, 1.5, (0, 0, 1), wo, sq)
        pp = orc.bsdf_probe(orc.STANDARD_PBR, (0.9, 0.6, 0.2), 0.7, 0.4, 1.5, p["dir"], wo, sq)
        if p["dir"][2] > 0:
            assert abs(pp["pdf"] - p["sample_pdf"]) <= 2e-5 * max(1.0, p["sample_pdf"])   # h is re-derived from wi+wo in pdf()
            assert np.all(pp["eval"] * abs(p["dir"][2]) / p["sample_pdf"] < 2.5)


# ---- the reference's furnace tests on the oracle, at the reference's parameters and tolerances ----
def test_reference_furnace_white_sphere(orc):
    c = orc.Context(threads=usable_cores())
    s, l = scenes.furnace_white_sphere(c)
    c.set_pipeline(samples_per_run=512, max_bounces=1024, env_samples_per_bounce=0, mesh_samples_per_bounce=0)   # tests.zig:330-335
    c.render(s, l)
    img = c.sensor_data(s)
    assert np.all(np.abs(img[..., :3] - 1.0) <= 0.00001)        # tests.zig:339-343
    c.set_pipeline(samples_per_run=512, max_bounces=1024, env_samples_per_bounce=1, mesh_samples_per_bounce=0)   # tests.zig:347-352
    c.render(s, l)
    assert np.all(np.abs(c.sensor_data(s)[..., :3] - 1.0) <= 0.1)   # tests.zig:358-362


def test_reference_furnace_inside_sphere(orc):
    c = orc.Context(threads=usable_cores())
    s, l = scenes.furnace_inside_sphere(c)
    c.set_pipeline(samples_per_run=1024, max_bounces=1024, env_samples_per_bounce=0, mesh_samples_per_bounce=0)  # tests.zig:440-445
    c.render(s, l)
    assert np.all(np.abs(c.sensor_data(s)[..., :3] - 1.0) <= 0.02)  # tests.zig:449-454


def test_reference_furnace_inside_sphere_with_mesh_sampling(orc):
    """the reference's fourth furnace test (tests.zig:457-487), disabled there for want of an instance upload path for sampled
    meshes: the emissive sphere is a mesh light, one light sample per bounce with MIS; its stated tolerance is 0.1"""
    c = orc.Context(threads=usable_cores())
    s, l = scenes.furnace_inside_sphere(c, sampled=True)
    c.set_pipeline(samples_per_run=512, max_bounces=1024, env_samples_per_bounce=0, mesh_samples_per_bounce=1)   # tests.zig:470-475
    c.render(s, l)
    img = c.sensor_data(s)[..., :3]
    assert np.all(np.abs(img - 1.0) <= 0.1)                         # tests.zig:483
    assert abs(float(img.mean()) - 1.0) < 0.005                     # unbiased: the mean over 1024 pixels x 512 samples


def test_icosphere_fixture():
    P, I = scenes.icosphere(5)
    assert P.shape == (10242, 3) and I.shape == (20480, 3)       # tests.zig:115-247 at order 5
    assert np.abs(np.linalg.norm(P, axis=1) - 1).max() < 1e-6
    n = np.cross(P[I[:, 1]] - P[I[:, 0]], P[I[:, 2]] - P[I[:, 0]])
    assert np.all((n * P[I].mean(1)).sum(1) > 0)                 # outward winding
    _, Ir = scenes.icosphere(2, True)
    assert np.array_equal(Ir, scenes.icosphere(2)[1][:, ::-1])


def test_golden_films(orc):
    for name, builder, kw, pipe, launches in (
            ("furnace_white_16spp", scenes.furnace_white_sphere, {}, dict(samples_per_run=16, max_bounces=1024, env_samples_per_bounce=0, mesh_samples_per_bounce=0), 1),
            ("furnace_inside_16spp", scenes.furnace_inside_sphere, {}, dict(samples_per_run=16, max_bounces=1024, env_samples_per_bounce=0, mesh_samples_per_bounce=0), 1),
            ("s1_mini_64x36_4spp", scenes.s1, dict(extent=(64, 36), grid=2, order=2), dict(samples_per_run=1, max_bounces=8, env_samples_per_bounce=1, mesh_samples_per_bounce=1), 4),
            ("cornell_48_4spp", scenes.cornell, dict(extent=(48, 48)), dict(samples_per_run=2, max_bounces=8, env_samples_per_bounce=0, mesh_samples_per_bounce=1), 2)):
        c = orc.Context(threads=usable_cores())
        s, l = builder(c, **kw)
        c.set_pipeline(**pipe)
        c.render(s, l, launches=launches)
        assert np.array_equal(bits(c.sensor_data(s)), bits(np.load(os.path.join(G, name + ".npy")))), name


def test_env_preprocessing(orc):
    e = np.load(os.path.join(G, "env_32x16.npz"))
    c = orc.Context()
    c.set_background(e["src"], 32, 16)
    rgb, lum = c.env()
    assert rgb.shape == (16, 16, 4)                               # S = min(floorPow2(height), 1024), BackgroundManager.zig:154
    assert np.array_equal(bits(rgb), bits(e["rgb"]))
    for i, l in enumerate(lum):
        assert np.array_equal(bits(l), bits(e["lum%d" % i]))
    # fold.hlsl:6-17 is a 2x2 SUM: the top level is the integral of level 0
    assert abs(float(lum[-1][0, 0]) - float(lum[0].astype(np.float64).sum())) < 1e-3 * float(lum[-1][0, 0])
    # luminance.hlsl:7-15
    assert np.allclose(lum[0], 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2], rtol=1e-6)
    # 1x1 constant environment stays exact (tests.zig:313-321)
    c.set_background(np.float32([0.25, 0.5, 1.0, 1.0]), 1, 1)
    rgb, lum = c.env()
    assert rgb.shape == (1, 1, 4) and np.array_equal(rgb[0, 0, :3], np.float32([0.25, 0.5, 1.0]))


def test_nee_and_plain_estimators_agree(orc):
    """light sampling must not change the expectation (integrator.hlsl:108-181): Cornell with and without mesh NEE."""
    means = []
    for mesh in (0, 1):
        c = orc.Context(threads=usable_cores())
        s, l = scenes.cornell(c, extent=(24, 24))
        c.set_pipeline(samples_per_run=1, max_bounces=6, env_samples_per_bounce=0, mesh_samples_per_bounce=mesh)
        c.render(s, l, launches=600 if mesh == 0 else 150)
        means.append(c.sensor_data(s)[..., :3].astype(np.float64).mean())
    assert abs(means[0] - means[1]) / means[1] < 0.06


def test_sample_count_and_clear_rules(orc):
    c = orc.Context()
    s, l = scenes.single_triangle(c, extent=(8, 8))
    c.set_pipeline(samples_per_run=3, max_bounces=1, env_samples_per_bounce=1, mesh_samples_per_bounce=0)
    c.render(s, l, launches=2)
    assert c.sample_count(s) == 6 and np.all(c.sensor_data(s)[..., 3] == 2.0)     # alpha counts launches (main.hlsl:46,49)
    c.set_lens(l, c.make_lens((0, -3, 0), (0, 1, 0), (0, 0, 1), 0.7))             # SetLens clears sensors (hydra.zig:530-540)
    assert c.sample_count(s) == 0
    c.render(s, l)
    assert np.all(c.sensor_data(s)[..., 3] == 1.0)


def test_geometry_material_reassignment(orc):
    """Accel.recordUpdateSingleMaterial (Accel.zig:609-628) on the oracle: one field of the flat geometry table — the film changes from the next render on, the alias table
    (areas only, Accel.zig:503-519) and the sample count do not, an edit back restores the first film bit for bit, unknown handles are refused"""
    c = orc.Context(threads=usable_cores())
    black = c.solid_texture(0.0, 0.0, 0.0); flat = c.solid_texture(0.5, 0.5)
    red = c.create_material(scenes.LAMBERT, flat, black, color=c.solid_texture(0.8, 0.1, 0.1))
    mirror = c.create_material(scenes.PERFECT_MIRROR, flat, black)
    glow = c.create_material(scenes.LAMBERT, flat, c.solid_texture(4.0, 4.0, 4.0), color=black)
    P, I = scenes.icosphere(2); sphere = c.create_mesh(P, I)
    Pq, Iq = scenes.quad((-1, -1, 2.5), (1, -1, 2.5), (1, 1, 2.5), (-1, 1, 2.5)); lamp = c.create_mesh(Pq, Iq)
    inst = c.create_instance([(sphere, red, False)], transform=np.eye(3, 4, dtype=np.float32))
    c.create_instance([(lamp, glow, True)], transform=np.eye(3, 4, dtype=np.float32))
    c.set_background(np.array([0.2, 0.2, 0.3, 1.0], np.float32), 1, 1)
    s = c.create_sensor(24, 16); l = c.create_lens(c.make_lens((0.0, -5.0, 0.5), (0.0, 1.0, 0.0), (0, 0, 1), 0.7))
    c.set_pipeline(samples_per_run=4, max_bounces=4, env_samples_per_bounce=1, mesh_samples_per_bounce=1)
    c.render(s, l, launches=2); first = c.sensor_data(s).copy(); alias = np.asarray(c.alias_table()).copy()
    c.set_geometry_material(inst, 0, mirror)
    assert c.sample_count(s) == 8                                  # the caller clears (online/main.zig:231), the call does not
    c.clear_sensor(s); c.render(s, l, launches=2); second = c.sensor_data(s).copy()
    assert not np.array_equal(first[..., :3], second[..., :3])
    assert np.array_equal(np.asarray(c.alias_table()).view(np.uint8), alias.view(np.uint8))
    c.set_geometry_material(inst, 0, red); c.clear_sensor(s); c.render(s, l, launches=2)
    assert np.array_equal(c.sensor_data(s).view(np.uint32), first.view(np.uint32))
    for bad in ((7, 0, red), (inst, 1, red), (inst, 0, 99)):
        with pytest.raises(RuntimeError):
            c.set_geometry_material(*bad)


def _same_hits(c, rays, level=1):
    """every ray through the culled search and through the search without instance boxes (OrcSetExhaustiveSearch 1; 2: without any box): the same hit record, the same occlusion"""
    bad = []
    for k, r in enumerate(rays):
        c.set_exhaustive_search(0); a = c.trace_closest(r[:3], r[3:6], float(r[6])); sa = c.trace_shadow(r[:3], r[3:6], float(r[6]))
        c.set_exhaustive_search(level); b = c.trace_closest(r[:3], r[3:6], float(r[6])); sb = c.trace_shadow(r[:3], r[3:6], float(r[6]))
        if a[0] != b[0] or sa != sb or (a[0] and (tuple(a[1]) != tuple(b[1]) or not np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))):
            bad.append((k, a, b, sa, sb))
    c.set_exhaustive_search(0)
    return bad


@pytest.mark.parametrize("seed", seeds(list(range(24)) + [14, 501, 593, 707, 910, 1115, 1199, 1228, 2166, 2846, 3277, 3369], 60))
def test_instance_boxes_never_change_a_hit(orc, seed):
    """The contract (orc_bvh.c:1-10) is the search over every triangle of every visible instance in ITS space; the TLAS boxes only cut it short.  They live in world space,
    and the two spaces agree up to the rounding of the inverse transform and of the transformed ray: orc_bvh.c instance_cull_slack bounds that and grows the boxes by it.
    Held here against the search that enters every instance (OrcSetExhaustiveSearch): rays at the hulls' outermost vertices, tangent to them, from inside, from 1e5 away
    (tests/hull_rays.py), with one transform that loses six digits in its inverse.  (The seeds named are the ones on which the boxes of round 5's oracle — the transformed
    corners grown by 1e-6 of their size — lost or invented a hit.)"""
    import hull_rays
    c = orc.Context(threads=1)
    parts = []
    world = hull_rays.hull_scene(c, seed, harsh=True, parts=parts, baked=seed % 3 == 2)
    c.create_sensor(8, 8)
    bad = _same_hits(c, hull_rays.hull_rays(world, seed), 2 if seed % 3 == 2 else 1)   # (one world BLAS: against the search that tests every triangle)
    assert not bad, bad[:3]
    if seed % 3 == 2:
        return
    hull_rays.hull_move((c,), seed, parts, world)
    bad = _same_hits(c, hull_rays.hull_rays(world, seed + 1)[::2])
    assert not bad, bad[:3]


@pytest.mark.parametrize("far", [1e2, 1e4, 1e6])
@pytest.mark.parametrize("seed", seeds(list(range(6)), 6))
def test_far_origins_with_and_without_boxes(orc, seed, far):
    """intersection.hlsl:20: any origin.  The oracle's instance slack takes the ray's origin per ray (orc_bvh.c instance_cull_slack); held here from 1e2 ... 1e6 scene
    sizes out against the search without boxes — the product's far-camera test (tests/test_gpu_parity.py::test_camera_far_outside_the_baked_reach) leans on it"""
    import hull_rays
    c = orc.Context(threads=1)
    world = hull_rays.hull_scene(c, seed, harsh=seed % 2 == 1, baked=seed % 3 == 2)
    c.create_sensor(8, 8)
    bad = _same_hits(c, hull_rays.far_rays(world, seed, far), 2 if seed % 2 == 0 else 1)
    assert not bad, bad[:3]


def test_triangle_boxes_never_change_a_hit(orc):
    """the same for the boxes inside a BLAS: the search that tests every triangle of every instance (level 2) against the one that only enters every instance (level 1)"""
    import hull_rays
    for seed in range(6):
        c = orc.Context(threads=1)
        world = hull_rays.hull_scene(c, seed, harsh=True)
        c.create_sensor(8, 8)
        for r in hull_rays.hull_rays(world, seed):
            c.set_exhaustive_search(1); a = c.trace_closest(r[:3], r[3:6], float(r[6])); sa = c.trace_shadow(r[:3], r[3:6], float(r[6]))
            c.set_exhaustive_search(2); b = c.trace_closest(r[:3], r[3:6], float(r[6])); sb = c.trace_shadow(r[:3], r[3:6], float(r[6]))
            assert a[0] == b[0] and sa == sb and (not a[0] or (tuple(a[1]) == tuple(b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))), (seed, r, a, b)


@pytest.mark.parametrize("seed", seeds(list(range(12)), 20))
def test_no_box_changes_a_pixel(orc, seed):
    """the randomized scenes of tests/parity_scenes.py rendered twice by the oracle — with its two-level BVH, and testing every triangle of every visible instance for
    every ray (OrcSetExhaustiveSearch 2, the contract with nothing in the way): the same film bit for bit, the same ray counts, the same probe rays"""
    rs = np.random.default_rng(1000 + seed)
    films, counts, hits = [], [], []
    rays = random_rays(200, seed, radius=8.0)
    bounces = int(rs.integers(1, 5))
    for level in (0, 2):
        c = orc.Context(threads=usable_cores())
        s, l = random_scene(c, seed=seed)
        c.set_pipeline(samples_per_run=1, max_bounces=bounces, env_samples_per_bounce=1, mesh_samples_per_bounce=1)
        c.set_exhaustive_search(level)
        c.render(s, l, launches=1)
        films.append(c.sensor_data(s).copy())
        k = c.counters(); counts.append((k["closest_rays"], k["shadow_rays"], k["samples"]))
        hits.append([(c.trace_closest(r[:3], r[3:6], float(r[6])), c.trace_shadow(r[:3], r[3:6], float(r[6]))) for r in rays])
    same = (films[0].view(np.uint32) == films[1].view(np.uint32)) | (np.isnan(films[0]) & np.isnan(films[1]))
    assert same.all(), "%d values differ" % int((~same).sum())
    assert counts[0] == counts[1]
    for (a, sa), (b, sb) in zip(*hits):
        assert a[0] == b[0] and sa == sb and (not a[0] or (tuple(a[1]) == tuple(b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))))


@pytest.mark.parametrize("seed", seeds(list(range(8)), 24))
def test_lattice_rays_with_and_without_boxes(orc, seed):
    """exact arithmetic everywhere (tests/hull_rays.py lattice_*): rays in face planes, along edges, through corners, starting and ending on faces — box distances of
    +-0, ties between up to six triangles of several instances; the culled search against the exhaustive one"""
    import hull_rays
    c = orc.Context(threads=1)
    hull_rays.lattice_scene(c, seed, baked=seed % 3 == 2)
    c.create_sensor(8, 8)
    rays = hull_rays.lattice_rays(seed)
    bad = _same_hits(c, rays, 2)
    assert not bad, bad[:3]
    c.set_exhaustive_search(0)
    assert sum(1 for r in rays[:300] if c.trace_closest(r[:3], r[3:6], float(r[6]))[0]) >= 1       # (the rays do hit things; at a scale of 2^-62 as few as two of 300: seed 24871 of a 140 000-case sweep)


@pytest.mark.parametrize("seed", seeds(list(range(6)) + [6100112, 6100853], 16))
def test_lattice_films_with_and_without_boxes(orc, seed):
    """the lattice scenes RENDERED from a camera on a lattice point, with the BVH and testing every triangle: the same film.  A camera on a face plane starts every ray
    exactly in that face's triangles' planes; the test's t for them is +-2e-8 around 0, some are taken, and the flat box of such a triangle lies exactly behind the
    origin — round 5's box test held the exit distance against 0 without the slack the other end of the range had (the two seeds named; the PRODUCT agreed with the
    exhaustive search there and this file's BVH did not).  And rays leaving faces from a few denormals off them (tests/hull_rays.py face_rays)"""
    import hull_rays
    rs = np.random.default_rng(seed + 9)
    eye = rs.integers(-6, 7, 3) * 0.5; fwd = rs.integers(-2, 3, 3) * 1.0
    if not fwd.any():
        fwd = np.array([1.0, 0, 0])
    up = np.array([0, 0, 1.0]) if abs(fwd[2]) < 0.9 * np.linalg.norm(fwd) else np.array([0, 1.0, 0])
    films = []
    for level in (0, 2):
        c = orc.Context(threads=usable_cores())
        hull_rays.lattice_scene(c, seed, baked=seed % 3 == 2, scale=1.0)
        lens = c.create_lens(c.make_lens(tuple(eye), tuple(fwd / np.linalg.norm(fwd)), tuple(up), 0.9, 0.0, 1.0)); sn = c.create_sensor(24, 16)
        c.set_pipeline(samples_per_run=2, max_bounces=5, env_samples_per_bounce=1, mesh_samples_per_bounce=0)
        c.set_exhaustive_search(level)
        c.render(sn, lens, launches=2); films.append(c.sensor_data(sn).copy())
    same = (films[0].view(np.uint32) == films[1].view(np.uint32)) | (np.isnan(films[0]) & np.isnan(films[1]))
    assert same.all(), "%d pixels differ" % int((~same).any(-1).sum())
    bad = _same_hits(c, hull_rays.face_rays(seed), 2)
    assert not bad, bad[:3]


_GRAZING_SEEDS = [6204351, 6226272, 6240180]   # round 6: a shadow ray leaving a large flat quad 1.4 degrees off its plane; the triangle test's t is +6.8e-4 around a true -2.4e-3 (box_hit8: slack per axis)


@pytest.mark.parametrize("seed", seeds(list(range(6)) + [6200851, 6201195, 6201640] + _GRAZING_SEEDS, 16))
def test_hull_films_with_and_without_boxes(orc, seed):
    """tests/test_gpu_parity.py::test_films_of_hull_and_lattice_scenes' hull family rendered by the oracle with its BVH and by its search over every triangle: the same film
    and ray counts.  Round 6's sweep of the GPU test found seed 6204351 where THIS FILE's BVH dropped an occluder the search takes (and the product too): a shadow ray that
    leaves a 19 x 0.1 flat quad at 1.4 degrees.  The watertight t is a weighted mean of the vertices' plane distances with weights that are differences of products — a
    computed hit point can sit anywhere inside the triangle's range ALONG THE DOMINANT AXIS, off its true place by eps x size / sin(grazing angle); a box may therefore
    only cull against the ray's range after it has been grown IN POSITION, per axis (orc_bvh.c box_hit8)."""
    import hull_rays
    films, counts = [], []
    for level in (0, 2):
        c = orc.Context(threads=usable_cores())
        rs = np.random.default_rng(seed + 9)
        world = hull_rays.hull_scene(c, seed, seed % 2 == 1, baked=seed % 3 == 2)
        W = world[int(rs.integers(len(world)))]; ctr = 0.5 * (W.min(0) + W.max(0)); r = max(np.linalg.norm(W - ctr, axis=1).max(), 1e-20)
        eye = ctr + rs.normal(size=3) * r * rs.choice([0.3, 1.5, 4.0]); fwd = ctr - eye + rs.normal(size=3) * r * 0.1
        up = np.array([0, 0, 1.0]) if abs(fwd[2]) < 0.9 * np.linalg.norm(fwd) else np.array([0, 1.0, 0])
        lens = c.create_lens(c.make_lens(tuple(eye), tuple(fwd / np.linalg.norm(fwd)), tuple(up), 0.9, 0.0, 1.0)); sn = c.create_sensor(24, 16)
        c.set_pipeline(samples_per_run=2, max_bounces=5, env_samples_per_bounce=1, mesh_samples_per_bounce=0)
        c.set_exhaustive_search(level)
        c.render(sn, lens, launches=2); films.append(c.sensor_data(sn).copy())
        k = c.counters(); counts.append((k["closest_rays"], k["shadow_rays"], k["samples"]))
    same = (films[0].view(np.uint32) == films[1].view(np.uint32)) | (np.isnan(films[0]) & np.isnan(films[1]))
    assert same.all(), "%d pixels differ" % int((~same).any(-1).sum())
    assert counts[0] == counts[1]

"""The scenes the parity tests, the structural audit and their worker processes (tests/workers/) draw: every generator once, each a function of a context — the
product's, the oracle's or a recorder — and its parameters.  A generator's calls on the context and the draws from its random stream keep their order: handle numbers
and the regression seeds of tests/test_gpu_parity.py mean what they mean only through it.  (tests/hull_rays.py holds the hull and lattice scenes.)"""
import numpy as np

from moonshine_amd import scenes

f32 = np.float32


def grey(ctx, albedo=0.7):
    """a Lambert material of one albedo under a flat normal map, no emission (its three constant textures in the order the calls are written)"""
    return ctx.create_material(scenes.LAMBERT, ctx.solid_texture(0.5, 0.5), ctx.solid_texture(0.0, 0.0, 0.0), color=ctx.solid_texture(albedo, albedo, albedo))


# ---------------- triangle soups, piles and batches of meshes: the builder's scenes ----------------

def soup(n, family=""):
    """(n, 3, 3) float32 corners and the number of all-non-finite triangles planted: n random triangles of very different sizes (spread e^N(-1.5, 1.5)), from 8 on
    with one copy pair, one triangle flat in z and one all-NaN triangle.  `family`: flat (every triangle in z = 0), far (translated by 1e4 times its size), tiny / huge
    (times 1e-20 / 1e20), point (a triangle of three equal corners), needle (2000 : 1)."""
    rs = np.random.default_rng(n)
    centre = rs.normal(size=(n, 1, 3)) * 4.0
    size = np.exp(rs.normal(size=(n, 1, 1)) * 1.5 - 1.5)
    P = (centre + rs.normal(size=(n, 3, 3)) * size).astype(f32)
    planted = 0
    if family == "point":
        P[7] = P[7, 0]
    if family == "needle":
        u = np.array([0.6, 0.64, 0.48]); v = np.array([-0.8, 0.48, 0.36])             # orthonormal
        a = P[11, 0].astype(np.float64)
        P[11, 1] = (a + 6.0 * u).astype(f32); P[11, 2] = (a + 6.0 * u + 6.0 / 2000.0 * v).astype(f32)
    if n >= 8:
        P[n // 2] = P[0]; P[n // 3, :, 2] = P[n // 3, 0, 2]; P[n // 5] = np.nan; planted = 1
    if family == "flat":
        P[..., 2] *= f32(0.0)                                                          # (NaN stays NaN)
    if family == "far":
        with np.errstate(invalid="ignore"):
            size_ = float(np.nanmax(P) - np.nanmin(P))
        P = (P.astype(np.float64) + 1.0e4 * size_ * np.array([1.0, -0.7, 0.4])).astype(f32)
    if family == "tiny":
        P = P * f32(1e-20)
    if family == "huge":
        P = P * f32(1e20)
    return P, planted


def soup_scene(n):
    """soup(n) as one mesh under a camera: sizes around the sweep's tile (256 positions) and super-tile (64 tiles) boundaries exercise every carry of its
    segmented scans"""
    def build(c, extent):
        P, _ = soup(n)
        mat = grey(c)
        c.create_instance([(c.create_mesh(P.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)), mat, False)])
        c.set_background(np.ones((1, 1, 4), np.float32), 1, 1)
        return c.create_sensor(*extent), c.create_lens(c.make_lens((0, 0, 14), (0, 0, -1), (0, 1, 0), 0.9))
    return build


def one_mesh_scene(ctx, P):
    ctx.create_instance([(ctx.create_mesh(P.reshape(-1, 3), np.arange(3 * len(P), dtype=np.uint32).reshape(-1, 3)), grey(ctx), False)])
    ctx.set_background(np.ones((1, 1, 4), f32), 1, 1)


def build_case(ctx, name):
    """a named scene into the (recording) context -> how many all-non-finite triangles it holds"""
    if name == "s2":
        scenes.s2(ctx, extent=(16, 9), dims=(3, 3, 2), order=3)
        return 0
    n, _, family = name.partition("-")
    P, planted = soup(int(n), family)
    one_mesh_scene(ctx, P)
    return planted


def pile_and_chain():
    """what a surface-area sweep cannot split -> (tri, pile_idx, chain, chain_idx, pos): one triangle indexed 6000 times, and 3000 triangles along a line with
    geometrically shrinking sizes (the chain's k-th triangle sits at x = pos[k] + 3)"""
    tri = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], np.float32)
    pile_idx = np.tile(np.array([[0, 1, 2]], np.uint32), (6000, 1))
    k = np.arange(3000)
    size = (0.97 ** k).astype(np.float32)[:, None, None]
    pos = np.cumsum(np.concatenate([[0.0], (0.97 ** k[:-1]) * 1.2])).astype(np.float32)
    chain = (tri[None] * size * 0.5 + np.stack([pos + 3.0, np.zeros(3000, np.float32), np.zeros(3000, np.float32)], 1)[:, None, :]).reshape(-1, 3).astype(np.float32)
    chain_idx = np.arange(9000, dtype=np.uint32).reshape(-1, 3)
    return tri, pile_idx, chain, chain_idx, pos


def pile(c, extent):
    tri, pile_idx, chain, chain_idx, _ = pile_and_chain()
    mat = grey(c)
    c.create_instance([(c.create_mesh(tri, pile_idx), mat, False)])
    c.create_instance([(c.create_mesh(chain, chain_idx), mat, False)])
    c.set_background(np.ones((1, 1, 4), np.float32), 1, 1)
    return c.create_sensor(*extent), c.create_lens(c.make_lens((0, 0, 5), (0, 0, -1), (0, 1, 0), 0.5))


def many_meshes(c, extent):
    """40 distinct icospheres in one batch, some with a NaN vertex, two in three under a rotation and a scale"""
    rs = np.random.default_rng(4)
    mat = grey(c)
    for k in range(40):
        P, I = scenes.icosphere(k % 4 + 1); P = (P * rs.uniform(0.3, 0.6, (1, 3))).astype(np.float32)
        if k % 9 == 4: P[5] = np.nan                                                                                  # NaN vertices: empty boxes in the sweep
        T = np.zeros((3, 4), np.float32); T[:, :3] = np.eye(3) if k % 3 == 0 else scenes._rot((rs.normal(), rs.normal(), rs.normal() + 1e-3), rs.uniform(0, 6.28)) * rs.uniform(0.6, 1.2)
        T[:, 3] = (1.5 * (k % 5), 1.5 * ((k // 5) % 5), 1.5 * (k // 25))
        c.create_instance([(c.create_mesh(P, I), mat, False)], transform=T)
    c.set_background(np.ones((1, 1, 4), np.float32), 1, 1)
    return c.create_sensor(*extent), c.create_lens(c.make_lens((3, 3, 12), (0, 0, -1), (0, 1, 0), 0.8))


# ---------------- lit scenes for the integrator ----------------

def edge_scene(ctx, scale, extent=(64, 48)):
    """a small lit scene with what real assets contain: zero-area triangles (repeated vertex, collinear vertices) inside
    ordinary meshes AND inside the sampled emitter (alias-table weight 0), a mirrored (negative-determinant) and a
    non-uniformly scaled instance, everything multiplied by `scale`"""
    S = np.float32(scale)
    normal = ctx.solid_texture(0.5, 0.5); black = ctx.solid_texture(0.0, 0.0, 0.0)
    grey = ctx.create_material(scenes.LAMBERT, normal, black, color=ctx.solid_texture(0.7, 0.7, 0.7))
    gold = ctx.create_material(scenes.STANDARD_PBR, normal, black, color=ctx.solid_texture(0.9, 0.7, 0.3), metalness=ctx.solid_texture(1.0), roughness=ctx.solid_texture(0.3))
    glass = ctx.create_material(scenes.GLASS, normal, black, ior=1.5)
    light = ctx.create_material(scenes.LAMBERT, normal, ctx.solid_texture(20.0, 18.0, 15.0), color=black)
    P, I = scenes.icosphere(2)
    # degenerate triangles appended to the sphere: a repeated vertex, three collinear vertices, three identical vertices
    Pd = np.concatenate([P, np.array([[0, 0, 2], [0, 0, 3], [0, 0, 4]], np.float32)])
    n0 = len(P)
    Id = np.concatenate([I, np.array([[0, 0, 1], [n0, n0 + 1, n0 + 2], [5, 5, 5]], np.uint32)])
    sphere = ctx.create_mesh(Pd * S, Id)
    fp, fi = scenes.quad((-6, -6, -1), (6, -6, -1), (6, 6, -1), (-6, 6, -1))
    floor = ctx.create_mesh(fp * S, fi)
    lp, li = scenes.quad((-1, -1, 4), (-1, 1, 4), (1, 1, 4), (1, -1, 4))
    lp = np.concatenate([lp, np.array([[0.5, 0.5, 4], [0.5, 0.5, 4], [2, 2, 4]], np.float32)])      # + a zero-area emissive triangle
    li = np.concatenate([li, np.array([[4, 5, 6]], np.uint32)])
    lamp = ctx.create_mesh(lp * S, li)
    def T(m3, t):
        out = np.zeros((3, 4), np.float32); out[:, :3] = m3; out[:, 3] = np.asarray(t, np.float32) * S
        return out
    ctx.create_instance([(floor, grey, False)])
    ctx.create_instance([(lamp, light, True)])
    ctx.create_instance([(sphere, gold, False)], transform=T(np.eye(3), (-2.2, 0, 0)))
    ctx.create_instance([(sphere, glass, False)], transform=T(np.diag([-1.0, 1.0, 1.0]), (0, 0.3, 0)))                 # mirrored
    ctx.create_instance([(sphere, grey, False)], transform=T(np.diag([0.5, 1.5, 0.75]) @ scenes._rot((0, 0, 1), 0.6)[:3, :3], (2.3, -0.2, 0)))
    ctx.set_background(np.array([0.3, 0.35, 0.5, 1], np.float32), 1, 1)
    lens = ctx.create_lens(ctx.make_lens((0, -9 * S, 2.5 * S), (0, 1, -0.2), (0, 0, 1), 0.7, 0.0, 1.0))
    return ctx.create_sensor(*extent), lens


def odd_transform_scene(c, M):
    normal = c.solid_texture(0.5, 0.5); black = c.solid_texture(0.0, 0.0, 0.0)
    grey = c.create_material(scenes.LAMBERT, normal, black, color=c.solid_texture(0.7, 0.7, 0.7))
    P, I = scenes.icosphere(2); m = c.create_mesh(P, I)
    def T(M, t):
        o = np.zeros((3, 4), np.float32); o[:, :3] = M; o[:, 3] = t
        return o
    c.create_instance([(m, grey, False)], transform=T(np.eye(3), (0, 0, 0)))
    c.create_instance([(m, grey, False)], transform=T(np.diag([1, 1, 0.5]), (2.5, 0, 0)))
    c.create_instance([(m, grey, False)], transform=T(M, (-2.5, 0, 0)))
    c.set_background(np.array([0.5, 0.5, 0.5, 1], np.float32), 1, 1)
    lens = c.create_lens(c.make_lens((0, -9, 1.0), (0, 1, -0.1), (0, 0, 1), 0.7, 0.0, 1.0))
    return c.create_sensor(48, 27), lens, T


def odd_scene(c, extent, ior, aperture):
    """texture coordinates far outside [0, 1] (negative, > 1, 1e4: the sampler's wrap rule), non-square and 1-texel-wide textures,
    an emissive texture on a sampled mesh, glass with the given ior, a thin lens with a large aperture"""
    rs = np.random.default_rng(21)
    gp, gi = scenes.quad((-5, -5, -1), (5, -5, -1), (5, 5, -1), (-5, 5, -1))
    uv = np.array([[-2.3, -1.7], [3.9, -1.7], [3.9, 10001.25], [-2.3, 10001.25]], np.float32)
    col = c.create_texture(rs.integers(0, 256, size=(5, 13, 4), dtype=np.uint8), 13, 5, "r8g8b8a8_srgb")      # 13 x 5
    strip = c.create_texture(rs.integers(40, 220, size=(7, 1), dtype=np.uint8), 1, 7, "r8_unorm")             # 1 x 7
    nrm = c.create_texture((128 + rs.integers(-50, 50, size=(3, 9, 2))).astype(np.uint8), 9, 3, "r8g8_unorm")
    black = c.solid_texture(0.0, 0.0, 0.0)
    floor = c.create_material(scenes.STANDARD_PBR, nrm, black, color=col, metalness=c.solid_texture(0.5), roughness=strip, ior=1.5)
    c.create_instance([(c.create_mesh(gp, gi, normals=np.tile(np.array([[0, 0, 1]], np.float32), (4, 1)), texcoords=uv), floor, False)])
    P, I = scenes.icosphere(3)
    glass = c.create_material(scenes.GLASS, c.solid_texture(0.5, 0.5), black, ior=ior)
    c.create_instance([(c.create_mesh(P, I), glass, False)])
    mirror = c.create_material(scenes.PERFECT_MIRROR, c.solid_texture(0.5, 0.5), black)
    T = np.eye(3, 4, dtype=np.float32); T[:, 3] = [2.4, 0.5, 0.0]
    c.create_instance([(c.create_mesh(P, I), mirror, False)], transform=T)
    lp, li = scenes.quad((-1, -1, 3.5), (-1, 1, 3.5), (1, 1, 3.5), (1, -1, 3.5))
    luv = np.array([[0, 0], [0, 2.5], [2.5, 2.5], [2.5, 0]], np.float32)
    etex = c.create_texture((rs.random((4, 4, 4)) * 30).astype(np.float32), 4, 4, "r32g32b32a32_sfloat")
    lamp = c.create_material(scenes.LAMBERT, c.solid_texture(0.5, 0.5), etex, color=black)
    c.create_instance([(c.create_mesh(lp, li, texcoords=luv), lamp, True)])
    c.set_background(np.array([0.2, 0.25, 0.3, 1], np.float32), 1, 1)
    lens = c.create_lens(c.make_lens((0.5, -7, 2.0), (0, 1, -0.25), (0, 0, 1), 0.9, aperture=aperture, focus_distance=6.5))
    return c.create_sensor(*extent), lens


def textured_scene(c, extent=(96, 64)):
    """a sphere with vertex normals and texcoords under an sRGB colour map, a two-component normal map and a roughness map, over a grey floor, lit by the sky, seen
    through a thin lens"""
    rs = np.random.default_rng(7)
    P, I = scenes.icosphere(3)
    N = P.copy()
    T = np.stack([np.arctan2(P[:, 1], P[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(P[:, 2], -1, 1)) / np.pi], -1).astype(np.float32)
    mesh = c.create_mesh(P, I, normals=N, texcoords=T)
    col = rs.integers(0, 256, size=(16, 32, 4), dtype=np.uint8)
    nrm = (128 + rs.integers(-40, 40, size=(8, 8, 2))).astype(np.uint8)
    rough = rs.integers(30, 200, size=(4, 4), dtype=np.uint8)
    tcol = c.create_texture(col, 32, 16, "r8g8b8a8_srgb")
    tn = c.create_texture(nrm, 8, 8, "r8g8_unorm")
    tr = c.create_texture(rough, 4, 4, "r8_unorm")
    m = c.create_material(scenes.STANDARD_PBR, tn, c.solid_texture(0.0, 0.0, 0.0), color=tcol, metalness=c.solid_texture(0.3), roughness=tr, ior=1.45)
    c.create_instance([(mesh, m, False)])
    gp, gi = scenes.quad((-4, -4, -1), (4, -4, -1), (4, 4, -1), (-4, 4, -1))
    gm = grey(c, 0.6)
    c.create_instance([(c.create_mesh(gp, gi), gm, False)])
    img = scenes.sky_sun_equirect(64, 32)
    c.set_background(img, 64, 32)
    lens = c.create_lens(c.make_lens((-3, -1, 1.5), (0.8, 0.3, -0.4), (0, 0, 1), 0.7, aperture=0.05, focus_distance=3.0))
    return c.create_sensor(*extent), lens


def material_edit_scene(c):
    """three instances around the origin over a ground quad: [0] a transformed two-geometry instance (sphere + quad), [1] a sampled emissive quad, [2] an identity-transform
    sphere (part of the merged world BLAS, like the ground [3])"""
    black = c.solid_texture(0.0, 0.0, 0.0); flat = c.solid_texture(0.5, 0.5)
    lam = [c.create_material(scenes.LAMBERT, flat, black, color=c.solid_texture(*rgb)) for rgb in ((0.8, 0.2, 0.2), (0.2, 0.8, 0.3), (0.7, 0.7, 0.7))]
    pbr = c.create_material(scenes.STANDARD_PBR, flat, black, color=c.solid_texture(0.9, 0.8, 0.3), metalness=c.solid_texture(1.0), roughness=c.solid_texture(0.3), ior=1.5)
    glass = c.create_material(scenes.GLASS, flat, black, ior=1.5)
    rs = np.random.default_rng(7)
    glow_a = c.create_material(scenes.LAMBERT, flat, c.solid_texture(6.0, 5.0, 4.0), color=black)
    glow_b = c.create_material(scenes.LAMBERT, flat, c.create_texture((rs.random((4, 4, 4)) * 9).astype(np.float16), 4, 4, "r16g16b16a16_sfloat"), color=black)
    P, I = scenes.icosphere(2); sphere = c.create_mesh(P, I, normals=(P / np.linalg.norm(P, axis=1, keepdims=True)).astype(np.float32))
    Pq, Iq = scenes.quad((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)); uvq = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    quad = c.create_mesh(Pq, Iq, texcoords=uvq)
    Pg, Ig = scenes.quad((-6, -6, -1.2), (6, -6, -1.2), (6, 6, -1.2), (-6, 6, -1.2)); ground = c.create_mesh(Pg, Ig)
    T0 = np.zeros((3, 4), np.float32); T0[:, :3] = scenes._rot((0.3, 1.0, 0.2), 0.7) * 0.8; T0[:, 3] = (-1.6, 0.2, 0.1)
    T1 = np.zeros((3, 4), np.float32); T1[:, :3] = scenes._rot((1.0, 0.0, 0.0), 3.14159265) * 0.9; T1[:, 3] = (0.2, 0.0, 2.4)
    c.create_instance([(sphere, lam[0], False), (quad, lam[1], False)], transform=T0)
    c.create_instance([(quad, glow_a, True)], transform=T1)
    c.create_instance([(sphere, lam[2], False)], transform=np.eye(3, 4, dtype=np.float32))
    c.create_instance([(ground, lam[2], False)], transform=np.eye(3, 4, dtype=np.float32))
    c.set_background(np.array([0.15, 0.18, 0.25, 1.0], np.float32), 1, 1)
    c.mats = dict(lam=lam, pbr=pbr, glass=glass, glow_a=glow_a, glow_b=glow_b)
    lens = c.create_lens(c.make_lens((0.0, -7.0, 1.5), (0.0, 1.0, -0.15), (0, 0, 1), 0.8))
    return c.create_sensor(72, 48), lens


def env_image(kind):
    rs = np.random.default_rng(33)
    if kind == "odd_size":        # 37 x 19: neither a power of two nor 2:1
        img = rs.random((19, 37, 4)).astype(np.float32) * 2.0
    elif kind == "two_by_one":    # the smallest equirect that is not constant
        img = np.array([[[3.0, 0.5, 0.1, 1.0], [0.1, 0.5, 3.0, 1.0]]], np.float32)
    elif kind == "hot_pixel":     # one texel 1e6 times brighter than the rest: importance sampling puts nearly every sample there
        img = np.full((64, 128, 4), 0.01, np.float32); img[20, 90, :3] = [1.0e4, 0.8e4, 0.5e4]
    elif kind == "black":         # nothing to sample: every env light sample has pdf 0
        img = np.zeros((8, 16, 4), np.float32)
    elif kind == "tall":          # higher than wide
        img = rs.random((64, 8, 4)).astype(np.float32)
    img[..., 3] = 1.0
    return np.ascontiguousarray(img)


# ---------------- the randomized scene ----------------

def random_scene(c, seed, big=False, hydra=False):
    """a scene drawn from a seed: 3-9 meshes (icospheres, quads, triangle soups; with and without normals / texcoords), materials of every type with constant or
    small image textures of every format, 4-14 instances under random affine transforms (rotations, non-uniform and NEGATIVE scales, identities, two-geometry
    instances, hidden ones), zero to two sampled emitters, a constant or an image environment, a thin-lens or pinhole camera, an odd-sized sensor"""
    rs = np.random.default_rng(seed)
    black = c.solid_texture(0.0, 0.0, 0.0)
    # hydra: the scene as Hydra's pipeline reads it (hydra.zig:97-105) — normal textures hold raw three-component normals, attributes come per face corner
    flat = c.solid_texture(0.0, 0.0, 1.0) if hydra else c.solid_texture(0.5, 0.5)

    def tex(kind):
        w, h = int(rs.integers(1, 9)), int(rs.integers(1, 9))
        if kind == "normal" and hydra:
            n = np.concatenate([rs.normal(size=(h, w, 2)) * 0.15, np.ones((h, w, 1)), np.zeros((h, w, 1))], -1)
            return c.create_texture(n.astype(np.float16), w, h, "r16g16b16a16_sfloat") if rs.random() < 0.4 else flat
        if kind == "rgb":
            return c.create_texture(rs.integers(0, 256, size=(h, w, 4), dtype=np.uint8), w, h, "r8g8b8a8_srgb") if rs.random() < 0.5 else c.solid_texture(*rs.random(3))
        if kind in ("scalar", "rough"):   # (a roughness below ~0.01 overflows GGX's D to inf and the BSDF to inf - inf = NaN, in the reference too: NaN pixels compare equal and test nothing)
            return c.create_texture(rs.integers(10, 250, size=(h, w), dtype=np.uint8), w, h, "r8_unorm") if rs.random() < 0.5 else c.solid_texture(float(rs.random()) * (0.97 if kind == "rough" else 1.0) + (0.03 if kind == "rough" else 0.0))
        if kind == "normal":
            return c.create_texture((128 + rs.integers(-40, 40, size=(h, w, 2))).astype(np.uint8), w, h, "r8g8_unorm") if rs.random() < 0.4 else flat
        return c.create_texture((rs.random((h, w, 4)) * 8).astype(np.float16), w, h, "r16g16b16a16_sfloat") if rs.random() < 0.5 else c.solid_texture(*(rs.random(3) * 6))
    mats = []
    for _ in range(int(rs.integers(3, 7))):
        kind = int(rs.integers(0, 4))
        if kind == scenes.GLASS:
            mats.append(c.create_material(scenes.GLASS, tex("normal"), black, ior=float(rs.uniform(1.05, 2.2))))
        elif kind == scenes.PERFECT_MIRROR:
            mats.append(c.create_material(scenes.PERFECT_MIRROR, tex("normal"), black))
        elif kind == scenes.LAMBERT:
            mats.append(c.create_material(scenes.LAMBERT, tex("normal"), black, color=tex("rgb")))
        else:
            mats.append(c.create_material(scenes.STANDARD_PBR, tex("normal"), black, color=tex("rgb"), metalness=tex("scalar"), roughness=tex("rough"), ior=float(rs.uniform(1.2, 1.8))))
    glow = [c.create_material(scenes.LAMBERT, flat, tex("emissive"), color=black) for _ in range(2)]
    meshes, not_finite = [], []
    for _ in range(int(rs.integers(3, 10))):
        kind = int(rs.integers(0, 3))
        if kind == 0:
            P, I = scenes.icosphere(int(rs.integers(2, 5) if big else rs.integers(0, 3))); P = (P * rs.uniform(0.3, 1.2, (1, 3))).astype(np.float32)
        elif kind == 1:
            e = float(rs.uniform(0.5, 3.0)); P, I = scenes.quad((-e, -e, 0), (e, -e, 0), (e, e, 0), (-e, e, 0))
        else:
            n = int(rs.integers(200, 3000) if big else rs.integers(1, 40)); P = (rs.normal(size=(3 * n, 3)) * rs.uniform(0.1, 1.0)).astype(np.float32); I = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
            if big:   # small triangles scattered in a cloud instead of a ball of long slivers, some of them degenerate (two equal corners) or not finite
                c0 = rs.normal(size=(n, 1, 3)) * 1.5; P = (c0 + rs.normal(size=(n, 3, 3)) * 0.08).reshape(-1, 3).astype(np.float32)
                P[3 * int(rs.integers(n)) + 1] = P[3 * int(rs.integers(n))]
                if rs.random() < 0.3: P[int(rs.integers(3 * n))] = np.nan; not_finite.append(len(meshes))
        nrm = uv = None
        if rs.random() < 0.5:   # shading normals: the surface's own direction, bent by up to ~30 degrees (arbitrary directions make frames whose tangent is parallel to the
            #                     normal: NaN in the reference too, and NaN pixels compare equal and test nothing)
            nrm = rs.normal(size=P.shape).astype(np.float32); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            if kind == 0:
                base = P / np.linalg.norm(P, axis=1, keepdims=True)
            elif kind == 1:
                base = np.tile(np.array([[0, 0, 1]], np.float32), (len(P), 1))
            else:
                t = np.nan_to_num(P.reshape(-1, 3, 3)); g = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); g /= np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-20)
                base = np.repeat(g, 3, axis=0)
            nrm = (0.5 * nrm + base).astype(np.float32); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        if rs.random() < 0.5:
            uv = (rs.random((len(P), 2)) * rs.uniform(0.5, 4.0) - 0.7).astype(np.float32)
        if hydra:   # world.hlsl:127-135: corner 3 * triangle + k
            nrm = None if nrm is None else np.ascontiguousarray(nrm[np.asarray(I).reshape(-1)])
            uv = None if uv is None else np.ascontiguousarray(uv[np.asarray(I).reshape(-1)])
        meshes.append(c.create_mesh(P, I, normals=nrm, texcoords=uv))
    n_emit = int(rs.integers(0, 3))
    for k in range(int(rs.integers(20, 60) if big else rs.integers(4, 15))):
        A = rs.normal(size=(3, 3)) * rs.uniform(0.4, 1.3)
        if rs.random() < 0.3:
            A = scenes._rot(tuple(rs.normal(size=3) + 1e-3), rs.random() * 6.0) * np.array([1.0, 1.0, -1.0 if rs.random() < 0.5 else 1.0])[None, :] * rs.uniform(0.5, 1.5)
        T = np.zeros((3, 4), np.float32); T[:, :3] = A; T[:, 3] = rs.normal(size=3) * 2.5
        if rs.random() < 0.25:
            T = np.eye(3, 4, dtype=np.float32)
        geos = [(meshes[int(rs.integers(len(meshes)))], mats[int(rs.integers(len(mats)))], False)]
        if rs.random() < 0.3:
            geos.append((meshes[int(rs.integers(len(meshes)))], mats[int(rs.integers(len(mats)))], False))
        if k < n_emit:   # (a sampled triangle with a NaN corner has a NaN area: every light sample of the scene would be NaN, in the reference too)
            geos = [(meshes[[m for m in range(len(meshes)) if m not in not_finite][int(rs.integers(len(meshes) - len(not_finite)))]], glow[k % 2], True)]
        c.create_instance(geos, transform=T, visible=bool(rs.random() > 0.1))
        geo_counts = (geo_counts if k else []) + [len(geos)]
    c.fuzz_instances, c.fuzz_emitters = k + 1, n_emit
    c.fuzz_geo_counts, c.fuzz_materials = geo_counts, mats + glow
    if rs.random() < 0.5:
        c.set_background(np.array([*(rs.random(3) * 0.8), 1.0], np.float32), 1, 1)
    else:
        w, h = int(rs.integers(2, 40)), int(rs.integers(2, 24))
        img = np.ones((h, w, 4), np.float32); img[..., :3] = rs.random((h, w, 3)) ** 4 * 5.0
        c.set_background(img, w, h)
    o = rs.normal(size=3); o = o / np.linalg.norm(o) * rs.uniform(5.0, 9.0)
    lens = c.create_lens(c.make_lens(tuple(o), tuple(-o / np.linalg.norm(o)), (0, 0, 1), float(rs.uniform(0.4, 1.2)), aperture=float(rs.choice([0.0, 0.05, 0.3])), focus_distance=float(rs.uniform(3.0, 9.0))))
    if big:
        return c.create_sensor(int(rs.integers(100, 300)), int(rs.integers(60, 200))), lens
    return c.create_sensor(int(rs.integers(5, 70)), int(rs.integers(5, 50))), lens

"""Second source for the texture lookups: every texel format and the sampler's edges, on the oracle (CPU) and on the HIP path (-m gpu), through the batch
probes "texture" (dTextures[i].SampleLevel, linear / repeat) and "env_incoming" (the equal-area environment map, linear / mirrored repeat).

The HIP path equals the oracle bit for bit and both decode a texel "with the same expressions" (csrc/msne_device.h texel_decode, oracle/orc_core.c): a wrong
divisor, a swapped channel or a wrong row pitch would be the same on both sides.  The judge here shares no text with either: second_source.decode_texels is
written from the Vulkan format definitions, second_source.vk_sample_linear from the Vulkan texel-filtering rules.

(1) exact decode.  At the texel centres ((i + 1/2) / w, (j + 1/2) / h) of a power-of-two-sized texture u * w - 1/2 is exact in f32, the blend weight is exactly 0
    and the lookup returns the decoded texel itself: all 256 bytes of every 8-bit channel, all 63 488 finite half patterns, random finite float patterns must come
    back EQUAL BY VALUE to float32(decode_texels) (a texel of -0 comes back as +0 through a * 1 + b * 0, hence values and not bits; the sRGB colour channels may be one
    f32 ulp off, libm's and numpy's pow).  Non-finite halves and one non-trivial texel per format go through 1x1 textures (the host-decoded TexDesc::first).
(2) sampler edges.  All seven formats x eight awkward shapes (strips, odd widths: uint16 and byte rows at odd addresses, a 15-byte texture before the next one's
    offset), 2000 coordinates each: random in [-3, 4]^2, every texel border and centre, signed zeros, +-1e4, 2^24, 1e-30 — judged by test_second_source.check_values
    as the three textures of probe_textures are, with its rule and constants unchanged.  Then the texel pool GROWS (the textures of (1), 512 KB of halves, into the
    same context): the first set must read the same bits from the moved pool.
(3) the environment lookup at its seams: axes, coordinate planes, the equal-area square's texel borders and centres, one-ulp neighbours; map sizes 1 ... 16.
(4) the checkers of (1) and (2) report every one of thirteen deliberately wrong decoders / samplers (CPU only, no library).

Texture coordinates that are not finite or reach 2^31 texels are deliberately not sent to either side: (int)floor(x) is outside C's defined range there."""
import functools
import itertools
import types

import numpy as np
import pytest

from tests import second_source as ss
from tests.test_second_source import check_values, env_of

FORMATS = list(ss.TEXEL_FORMATS)
SHAPES = [(2, 1), (1, 2), (1, 7), (3, 5), (5, 3), (13, 7), (16, 16), (17, 1)]      # (w, h)
COORDS = 2000


# ----------------------------------------------------------------------------------------------------------------------
# the two sides: (make a context, probe(ctx, name, records))
def oracle_side(orc):
    return (lambda: orc.Context()), (lambda ctx, name, x: orc.probe(name, x, ctx))


def hip_side(api):
    return (lambda: api.Context()), (lambda ctx, name, x: ctx.shade_probe(*ss.PROBES[name], x))


def create(ctx, textures):
    return [ctx.create_texture(raw, w, h, fmt) for raw, w, h, fmt in textures]


def lookup(probe, ctx, handles, coords):
    """coords: one (n, 2) float32 array per texture -> one (n, 4) float32 array per texture, from ONE probe call"""
    x = np.concatenate([np.concatenate([np.full((len(uv), 1), t, np.float32), uv], 1) for t, uv in zip(handles, coords)])
    return np.split(probe(ctx, "texture", x), np.cumsum([len(uv) for uv in coords])[:-1])


def centres(w, h):
    j, i = np.mgrid[0:h, 0:w]
    return np.stack([(i + 0.5) / w, (j + 0.5) / h], -1).reshape(-1, 2).astype(np.float32)


def pool_bytes(textures):
    return sum((np.asarray(raw).nbytes + 15) // 16 * 16 for raw, _, _, _ in textures)


# ----------------------------------------------------------------------------------------------------------------------
# (1) the textures whose every texel is looked up exactly
@functools.lru_cache(None)
def exact_textures():
    """-> [(raw, w, h, format)]: power-of-two sizes holding every value of the 8- and 16-bit channels, then the 1x1 textures"""
    rs = np.random.default_rng(2024)
    every = lambda values, count, channels: np.stack([np.resize(rs.permutation(values), count) for _ in range(channels)], 1)      # each channel its own permutation of all values
    byte = np.arange(256, dtype=np.uint8)
    half = np.arange(65536, dtype=np.uint32).astype(np.uint16); half = half[((half >> 10) & 31) != 31]                             # the 63 488 finite patterns: both zeros, all subnormals
    assert len(half) == 63488

    def floats(*shape):   # random bit patterns of finite floats: any sign, any exponent but 255, subnormals included
        b = rs.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
        return np.where((b >> 23) & 255 == 255, b & np.uint32(0xBFFFFFFF), b).astype(np.uint32).view(np.float32)
    out = [(every(byte, 256, 4).reshape(16, 16, 4), 16, 16, "r8g8b8a8_srgb"), (every(byte, 256, 2).reshape(16, 16, 2), 16, 16, "r8g8_unorm"),
           (every(byte, 256, 1).reshape(16, 16), 16, 16, "r8_unorm"), (every(half, 65536, 4).reshape(256, 256, 4), 256, 256, "r16g16b16a16_sfloat"),
           (floats(8, 8, 4), 8, 8, "r32g32b32a32_sfloat"), (floats(8, 8, 2), 8, 8, "r32g32_sfloat"), (floats(8, 8), 8, 8, "r32_sfloat")]
    # 1x1: the host-decoded `first` texel of every format ...
    out += [(np.uint8([201, 7, 94, 130]), 1, 1, "r8g8b8a8_srgb"), (np.uint8([77, 250]), 1, 1, "r8g8_unorm"), (np.uint8([3]), 1, 1, "r8_unorm"),
            (np.float16([0.3331, -5.5, 6.1e-5, 3e-7]).view(np.uint16), 1, 1, "r16g16b16a16_sfloat"), (np.float32([-1.7, 3e-41, 2.5e30, 0.1]), 1, 1, "r32g32b32a32_sfloat"),
            (np.float32([0.3, -0.0]), 1, 1, "r32g32_sfloat"), (np.float32([-123.456]), 1, 1, "r32_sfloat")]
    # ... and the halves that are not finite (a blend would multiply them by a zero weight): +inf, -inf, a quiet and a signalling NaN, in every channel in turn
    for k, bits in enumerate((0x7c00, 0xfc00, 0x7e00, 0x7c01)):
        t = np.roll(np.uint16([bits, 0x3c00, 0xbc00, 0x0000]), k)
        out.append((t, 1, 1, "r16g16b16a16_sfloat"))
    return out


@functools.lru_cache(None)
def exact_reference():
    with np.errstate(invalid="ignore"):      # (the signalling NaN, narrowed to f32)
        return [ss.decode_texels(raw, w, h, fmt).reshape(-1, 4).astype(np.float32) for raw, w, h, fmt in exact_textures()]


def check_exact(got, textures=None, reference=None):
    """got[t]: the lookups at the texel centres of texture t, row after row.  Every texel and channel equals float32(decode_texels) by value
    (NaN where that is NaN); the sRGB colour channels may be one f32 ulp off."""
    textures = exact_textures() if textures is None else textures
    reference = exact_reference() if reference is None else reference
    assert len(got) == len(textures)
    for g, ref, (raw, w, h, fmt) in zip(got, reference, textures):
        assert g.shape == ref.shape and g.dtype == np.float32, (fmt, w, h, g.shape, g.dtype)
        same = (g == ref) | (np.isnan(g) & np.isnan(ref))
        if fmt == "r8g8b8a8_srgb":      # positive finite floats: neighbouring values have neighbouring bit patterns
            ulps = np.abs(g.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
            same[:, :3] |= (ulps[:, :3] <= 1) & (g[:, :3] >= 0)
        if not same.all():
            i, c = np.argwhere(~same)[0]
            raise AssertionError("%s %dx%d: %d of %d texel channels differ from the decoded texel; first: texel (%d, %d) channel %d got %r, decode_texels gives %r"
                                 % (fmt, w, h, int((~same).sum()), same.size, i % w, i // w, c, g[i, c], ref[i, c]))


def run_exact_decode(side):
    make, probe = side
    ctx = make()
    tex = exact_textures()
    got = lookup(probe, ctx, create(ctx, tex), [centres(w, h) for _, w, h, _ in tex])
    check_exact(got)
    return ctx


def test_oracle_decodes_every_texel_value_exactly(orc):
    run_exact_decode(oracle_side(orc))


@pytest.mark.gpu
def test_hip_decodes_every_texel_value_exactly(gpu_api):
    ctx = run_exact_decode(hip_side(gpu_api))
    assert ctx.texel_pool_bytes() == pool_bytes(exact_textures())


# ----------------------------------------------------------------------------------------------------------------------
# (2) sampler edges
def random_texels(rs, fmt, w, h):
    """bytes over the full range; floats and halves in -2 ... 6"""
    n, dt = ss.TEXEL_FORMATS[fmt]
    if dt == np.uint8:
        return rs.integers(0, 256, (h, w, n), dtype=np.uint8)
    v = rs.uniform(-2.0, 6.0, (h, w, n))
    return v.astype(np.float32) if dt == np.float32 else v.astype(np.float16).view(np.uint16)


def edge_coordinates(rs, w, h, n=COORDS):
    uv = rs.uniform(-3.0, 4.0, (n, 2))
    bw, cw = np.arange(-2 * w, 3 * w + 1) / w, (np.arange(-2 * w, 3 * w) + 0.5) / w          # every texel border and centre, two periods to the left, three to the right
    bh, ch = np.arange(-2 * h, 3 * h + 1) / h, (np.arange(-2 * h, 3 * h) + 0.5) / h
    assert max(len(bw), len(bh)) <= 100
    uv[0:len(bw), 0] = bw; uv[100:100 + len(cw), 0] = cw
    uv[200:200 + len(bh), 1] = bh; uv[300:300 + len(ch), 1] = ch
    k = min(len(bw), len(bh)); uv[400:400 + k] = np.stack([bw[:k], bh[-k:]], 1)             # texel corners
    uv[500:564] = rs.choice([0.0, -0.0, 1.0, 0.5, -1.0, 2.0, 1e4, -1e4, 2.0 ** 24, 1e-30], (64, 2))
    return uv.astype(np.float32)


@functools.lru_cache(None)
def edge_textures(formats=tuple(FORMATS), shapes=tuple(SHAPES)):
    """-> ([(raw, w, h, format)], [decoded (h, w, 4) float64], [coordinates (COORDS, 2) float32])"""
    rs = np.random.default_rng(77)
    tex = [(random_texels(rs, fmt, w, h), w, h, fmt) for fmt in formats for (w, h) in shapes]
    return tex, [ss.decode_texels(*t) for t in tex], [edge_coordinates(rs, w, h) for _, w, h, _ in tex]


def check_edges(got, images, coords):
    """the lookups of all textures in one check_values call (texture index = position in `images`), rule and constants as for probe_textures"""
    x = np.concatenate([np.concatenate([np.full((len(uv), 1), t, np.float32), uv], 1) for t, uv in enumerate(coords)])
    rep = check_values("texture", np.concatenate(got), x, rel=1e-4, images=images)
    assert rep["skipped"] == 0 and rep["records"] == len(x), rep
    return rep


def run_sampler_edges(side):
    make, probe = side
    ctx = make()
    tex, images, coords = edge_textures()
    assert len(tex) == 56
    rep = check_edges(lookup(probe, ctx, create(ctx, tex), coords), images, coords)
    print("sampler edges:", rep)
    return rep


def test_oracle_sampler_edges_in_every_format_and_shape(orc):
    run_sampler_edges(oracle_side(orc))


@pytest.mark.gpu
def test_hip_sampler_edges_in_every_format_and_shape(gpu_api):
    run_sampler_edges(hip_side(gpu_api))


def run_pool_growth(side):
    make, probe = side
    ctx = make()
    tex, images, coords = edge_textures()
    first = create(ctx, tex)
    before = lookup(probe, ctx, first, coords)                     # (the probe puts what has been created so far on the device)
    big = exact_textures()
    second = create(ctx, big)                                      # 512 KB of halves: far beyond the pool's slack, it is reallocated and moved
    after = lookup(probe, ctx, first, coords)
    for a, b, (_, w, h, fmt) in zip(before, after, tex):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s %dx%d reads differently after the texel pool has grown" % (fmt, w, h)
    check_edges(after, images, coords)
    check_exact(lookup(probe, ctx, second, [centres(w, h) for _, w, h, _ in big]))
    return ctx


def test_oracle_textures_created_later_leave_earlier_ones_alone(orc):
    run_pool_growth(oracle_side(orc))


@pytest.mark.gpu
def test_hip_texel_pool_growth_keeps_every_texture(gpu_api):
    ctx = run_pool_growth(hip_side(gpu_api))
    assert ctx.texel_pool_bytes() == pool_bytes(edge_textures()[0]) + pool_bytes(exact_textures())


# ----------------------------------------------------------------------------------------------------------------------
# (3) the environment lookup at its seams
BACKGROUNDS = [(2, 1), (4, 2), (8, 4), (16, 8), (37, 19)]     # equirect (w, h) -> equal-area map size 1, 2, 4, 8, 16


def seam_directions(rs, S):
    c = (-1.0, 0.0, 1.0)
    axes = np.array([v for v in itertools.product(c, c, c) if any(v)])                                # the 26 sign combinations
    planes = rs.uniform(-1, 1, (3000, 3)); planes[:1000, 0] = 0; planes[1000:2000, 1] = 0; planes[2000:, 2] = 0
    grid = (np.mgrid[0:2 * S + 1, 0:2 * S + 1].reshape(2, -1).T / (2.0 * S)).astype(np.float32)      # texel borders and centres of the equal-area square
    x = np.concatenate([axes, planes, ss.square_to_equal_area_sphere(grid.astype(np.float64)), rs.normal(size=(4000, 3))])
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([x, np.nextafter(x[:2000], np.float32(2)), np.nextafter(x[:2000], np.float32(-2))])


def run_env_seams(side, w, h):
    make, probe = side
    rs = np.random.default_rng(1000 + w)
    ctx = make()
    img = np.ones((h, w, 4), np.float32); img[..., :3] = rs.uniform(0.05, 4.0, (h, w, 3))
    ctx.set_background(img, w, h)
    env = env_of(types.SimpleNamespace(env_textures=ctx.env()))
    assert env.size == 1 << (h.bit_length() - 1)
    x = seam_directions(rs, env.size)
    rep = check_values("env_incoming", probe(ctx, "env_incoming", x), x, env, rel=1e-4)
    assert rep["skipped"] == 0 and rep["records"] >= 11000, rep
    print("env seams %dx%d:" % (w, h), rep)
    return rep


@pytest.mark.parametrize("w,h", BACKGROUNDS)
def test_oracle_environment_lookup_at_its_seams(orc, w, h):
    run_env_seams(oracle_side(orc), w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", BACKGROUNDS)
def test_hip_environment_lookup_at_its_seams(gpu_api, w, h):
    run_env_seams(hip_side(gpu_api), w, h)


# ----------------------------------------------------------------------------------------------------------------------
# (4) the checkers notice: deliberately wrong decoders and samplers in numpy, fed to check_exact and check_edges
def wrong_decode(raw, w, h, fmt, mutation):
    n, dt = ss.TEXEL_FORMATS[fmt]
    if mutation == "rows_padded_to_4_bytes":       # row j read from byte j * pitch of the tightly packed buffer, pitch rounded up to 4 (what lies beyond reads 0)
        row = w * n * np.dtype(dt).itemsize; pitch = (row + 3) // 4 * 4
        b = np.frombuffer(np.ascontiguousarray(raw).tobytes() + bytes(pitch * h), np.uint8)
        raw = np.concatenate([b[j * pitch: j * pitch + row] for j in range(h)])
    img = ss.decode_texels(raw, w, h, fmt)
    c = np.frombuffer(np.ascontiguousarray(raw).tobytes(), dtype=dt, count=w * h * n).reshape(h, w, n)
    if mutation == "channel_swap" and n >= 2:
        img[..., [0, 1]] = img[..., [1, 0]]
    elif mutation == "divide_by_256" and dt == np.uint8 and fmt != "r8g8b8a8_srgb":
        img[..., :n] = c / 256.0
    elif mutation == "divide_by_256" and fmt == "r8g8b8a8_srgb":
        img[..., :3] = ss.srgb_eotf(c[..., :3] / 256.0); img[..., 3] = c[..., 3] / 256.0
    elif mutation == "srgb_curve_on_alpha" and fmt == "r8g8b8a8_srgb":
        img[..., 3] = ss.srgb_eotf(c[..., 3] / 255.0)
    elif mutation == "srgb_threshold_0.0031308" and fmt == "r8g8b8a8_srgb":     # the threshold of the INVERSE curve
        x = c[..., :3] / 255.0
        img[..., :3] = np.where(x <= 0.0031308, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    elif mutation == "half_subnormals_flushed" and dt == np.uint16:
        img[..., :n] = np.where((c >> 10) & 31 == 0, np.where(c >> 15 == 1, -0.0, 0.0), img[..., :n])
    elif mutation == "half_exponent_bias_off_by_one" and dt == np.uint16:
        img[..., :n] = np.where((c >> 10) & 31 == 0, img[..., :n], img[..., :n] * 2.0)
    elif mutation == "missing_alpha_0" and n < 4:
        img[..., 3] = 0.0
    return img


def wrong_sample(img, uv, mutation):
    h, w = img.shape[:2]
    uv = uv.astype(np.float64)
    if mutation == "xy_transposed":                  # texel (x, y) fetched from x * h + y
        img = img.reshape(w, h, 4).transpose(1, 0, 2)
    if mutation == "mirrored_instead_of_repeat":
        return ss.vk_sample_linear(img, uv, mirrored=True)
    if mutation == "nearest_instead_of_linear":
        return img[np.mod(np.floor(uv[:, 1] * h).astype(np.int64), h), np.mod(np.floor(uv[:, 0] * w).astype(np.int64), w)]
    if mutation in ("clamp_to_edge_instead_of_repeat", "no_half_texel_offset"):
        off = 0.0 if mutation == "no_half_texel_offset" else 0.5
        u, v = uv[:, 0] * w - off, uv[:, 1] * h - off
        i0, j0 = np.floor(u), np.floor(v)
        a, b = (u - i0)[:, None], (v - j0)[:, None]
        i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
        wrap = (lambda i, n: np.clip(i, 0, n - 1)) if mutation == "clamp_to_edge_instead_of_repeat" else (lambda i, n: np.mod(i, n))
        x0, x1, y0, y1 = wrap(i0, w), wrap(i0 + 1, w), wrap(j0, h), wrap(j0 + 1, h)
        return (1 - a) * (1 - b) * img[y0, x0] + a * (1 - b) * img[y0, x1] + (1 - a) * b * img[y1, x0] + a * b * img[y1, x1]
    return ss.vk_sample_linear(img, uv, mirrored=False)


DECODER_MUTATIONS = ["channel_swap", "divide_by_256", "srgb_curve_on_alpha", "srgb_threshold_0.0031308", "half_subnormals_flushed", "half_exponent_bias_off_by_one",
                     "missing_alpha_0", "rows_padded_to_4_bytes"]
SAMPLER_MUTATIONS = ["clamp_to_edge_instead_of_repeat", "mirrored_instead_of_repeat", "no_half_texel_offset", "nearest_instead_of_linear", "xy_transposed"]
# which checker must report what: the exact lookup sees every decoder mutation but a row pitch (its power-of-two rows are multiples of 4 bytes already) and, of
# the sampler's, the transposition; the edge lookup sees every sampler mutation and the decoder mutations that move a value by more than 1e-4 of the texel scale
EXACT_REPORTS = [m for m in DECODER_MUTATIONS if m != "rows_padded_to_4_bytes"] + ["xy_transposed"]
EDGES_REPORT = SAMPLER_MUTATIONS + ["channel_swap", "divide_by_256", "srgb_curve_on_alpha", "half_exponent_bias_off_by_one", "missing_alpha_0", "rows_padded_to_4_bytes"]


def mutant_exact(mutation):
    with np.errstate(invalid="ignore"):
        return [wrong_sample(wrong_decode(raw, w, h, fmt, mutation), centres(w, h), mutation).astype(np.float32) for raw, w, h, fmt in exact_textures()]


def mutant_edges(mutation):
    tex, images, coords = edge_textures(shapes=((3, 5), (13, 7), (1, 7)))
    return [wrong_sample(wrong_decode(raw, w, h, fmt, mutation), uv, mutation).astype(np.float32) for (raw, w, h, fmt), uv in zip(tex, coords)], images, coords


def test_checkers_pass_the_unmutated_numpy_sampler():
    """control: the stand-in the mutations are applied to passes both checkers when nothing is mutated"""
    check_exact(mutant_exact(None))
    check_edges(*mutant_edges(None))


def test_mutations_cover_the_list():
    assert len(set(DECODER_MUTATIONS + SAMPLER_MUTATIONS)) == 13 and set(EXACT_REPORTS) | set(EDGES_REPORT) == set(DECODER_MUTATIONS + SAMPLER_MUTATIONS)


@pytest.mark.parametrize("mutation", EXACT_REPORTS)
def test_exact_checker_reports(mutation):
    with pytest.raises(AssertionError, match="differ from the decoded texel"):
        check_exact(mutant_exact(mutation))


@pytest.mark.parametrize("mutation", EDGES_REPORT)
def test_edge_checker_reports(mutation):
    with pytest.raises(AssertionError, match="differ from the second source"):
        check_edges(*mutant_edges(mutation))

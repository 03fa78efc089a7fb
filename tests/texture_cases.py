"""The texture zoo of tests/test_texture_sampling.py (CPU) and tests/test_gpu_texture_sampling.py (GPU): non-square, non-power-of-two and thin textures in every upload format,
one scene that carries all of them, and the probe rows (include/mi355pt_testhooks.h kind 11, oracle.ptref.Oracle.texture_probe) every texture is sampled at.

Non-finite texture coordinates are outside the samplers' data contract ((int) of a NaN is undefined; tex_texel's clamp only keeps such a fetch in bounds): none is generated."""
import functools
import zlib
import numpy as np

from rtxpt_amd import scenes

SIZES = [(1, 1), (2, 1), (1, 7), (3, 3), (5, 4),
         (64, 2), (2, 64),                          # 1-wide mips below the mipLevels - 5 cap of sampleTexture
         (100, 60),                                 # mips 50, 25, 12, 6, 3, 1
         (255, 256), (257, 129),
         (64, 64), (128, 32)]                       # controls: the power-of-two branch
FORMATS = ["srgb8", "unorm8", "f32_alpha_bytes", "f32_alpha_floats", "f32_alpha_wide"]      # the last three: RGBA32F whose opacities are all k / 255 (a byte plane), arbitrary in [0, 1], partly outside [0, 1] (float planes)
CUTOFFS = [0.5, 0.3, 0.7, 0.45, 0.55]               # material AlphaCutoff per format (the scene quantises to trunc(c * 255) / 255)
UV_SCALES = [(1.0, 1.0), (-2.0, 3.0), (0.5, -1.5), (4.25, 4.25), (-1.0, -1.0), (2.5, 0.75)]


def _rng(*key): return np.random.default_rng(zlib.crc32(repr(key).encode()))


def make_pixels(w, h, fmt):
    """Seeded noise: (pixels [h, w, 4], upload format). The float formats' colours span five decades so that no tap of a filter hides behind another."""
    r = _rng("pixels", w, h, fmt)
    if fmt in ("srgb8", "unorm8"):
        return r.integers(0, 256, (h, w, 4)).astype(np.uint8), scenes.TEX_RGBA8_SRGB if fmt == "srgb8" else scenes.TEX_RGBA8_UNORM
    px = np.exp(1.5 * r.standard_normal((h, w, 4))).astype(np.float32)
    if fmt == "f32_alpha_bytes": px[..., 3] = r.integers(0, 256, (h, w)).astype(np.float32) / np.float32(255.0)
    elif fmt == "f32_alpha_floats": px[..., 3] = r.random((h, w), np.float32) * np.float32(0.999) + np.float32(0.0005)
    else: px[..., 3] = r.random((h, w), np.float32) * np.float32(1.5) - np.float32(0.25)
    return px, scenes.TEX_RGBA32F


def quantised_cutoff(c):
    """SubInstanceData's 8-bit cutoff as the alpha test reads it back."""
    return np.float32(int(np.float32(min(max(c, 0.0), 1.0)) * np.float32(255.0))) / np.float32(255.0)


class Tex:
    def __init__(self, index, w, h, fmt, pixels, upload, word):
        self.index, self.w, self.h, self.fmt, self.pixels, self.upload, self.word = index, w, h, fmt, pixels, upload, word
        self.name = "%dx%d %s" % (w, h, fmt); self.levels = int(np.floor(np.log2(max(w, h)))) + 1


@functools.lru_cache(maxsize=None)
def zoo():
    """(scene, textures, quads): every size in every format — neighbours in the texture table differ in plane format, and the byte planes of the small sizes (1, 2, 7, 9, 20
    bytes) leave the 16-byte padding between planes to do — each on an alpha-tested quad of its own: column = size, layer = format (a ray along +z meets one quad per layer).
    quads[q] = (texture, uv scale, uv offset, cutoff); the quad's two triangles are global primitives 2 q and 2 q + 1."""
    b = scenes.SceneBuilder(); texs, quads = [], []
    for si, (w, h) in enumerate(SIZES):
        for fi, fmt in enumerate(FORMATS):
            px, upload = make_pixels(w, h, fmt)
            word = b.add_texture(px, upload)
            t = Tex(len(texs), w, h, fmt, px, upload, word); texs.append(t)
            m = b.add_material(scenes.make_material(base=(0.8, 0.8, 0.8), base_tex=word, alpha_cutoff=CUTOFFS[fi]))
            su, sv = UV_SCALES[(si + fi) % len(UV_SCALES)]; off = (0.125 * fi, -0.25 * si)
            x, z = 1.5 * si, 0.5 * fi
            p, i, uv, n, tg = scenes.quad([x, 0, z], [x + 1, 0, z], [x + 1, 1, z], [x, 1, z])
            uv = (uv * np.float32([su, sv]) + np.float32(off)).astype(np.float32)
            b.begin_mesh(); b.add_geometry(p, i, m, uv=uv, normal=n, tangent=tg, geom_flags=scenes.GEOMF_ALPHA_TESTED); b.add_instance(b.end_mesh())
            quads.append((t, uv, quantised_cutoff(CUTOFFS[fi])))
    return b.finish(), texs, quads


def constant_scene(value=(0.25, 3.5, 0.0029296875, 0.625)):
    """The same sizes filled with one float texel each (RGBA32F): every function returns it at every row, to the bit — a + (c - c) * t is c, and the channels have so few
    mantissa bits that the N-tap filter's running sum k * c (k <= 16) and its division by N are exact too."""
    b = scenes.SceneBuilder(); texs = []
    for (w, h) in SIZES:
        px = np.tile(np.float32(value), (h, w, 1)); word = b.add_texture(px, scenes.TEX_RGBA32F)
        texs.append(Tex(len(texs), w, h, "constant", px, scenes.TEX_RGBA32F, word))
    m = b.add_material(scenes.make_material())
    p, i, uv, n, tg = scenes.quad([0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0])
    b.begin_mesh(); b.add_geometry(p, i, m, uv=uv, normal=n, tangent=tg); b.add_instance(b.end_mesh())
    return b.finish(), texs


# ---- probe rows: uint32 [n, 8] = (mode, texture, u, v, four mode words)
def _rows(mode, tex, u, v, w4=0, w5=0, w6=0, w7=0):
    u = np.atleast_1d(np.asarray(u, np.float32)); n = len(u)
    r = np.zeros((n, 8), np.uint32); r[:, 0] = mode; r[:, 1] = tex
    r[:, 2] = u.view(np.uint32); r[:, 3] = np.broadcast_to(np.asarray(v, np.float32), (n,)).copy().view(np.uint32)
    for col, val in ((4, w4), (5, w5), (6, w6), (7, w7)):
        val = np.asarray(val); r[:, col] = np.broadcast_to(val if val.dtype == np.uint32 else val.astype(np.float32).view(np.uint32), (n,))
    return r


SPECIAL = np.float32([0.0, 1.0, -1.0, -0.0])
SPECIAL_UV = np.stack(np.meshgrid(SPECIAL, SPECIAL, indexing="ij"), -1).reshape(-1, 2)


def _ladder(dim):
    """+-2^k and +-(2^k + 0.3) while |u * dim| < 2^23."""
    out = []; k = 0
    while (2.0 ** k + 0.3) * dim < 2.0 ** 23: out += [2.0 ** k, -(2.0 ** k), 2.0 ** k + 0.3, -(2.0 ** k + 0.3)]; k += 1
    return np.float32(out)


def bilinear_rows(t):
    """Mode 1, every mip of the texture: random uv in [-3, 3]^2, the special values, the ladder; at mip 0 every texel centre and every texel edge along each axis."""
    r = _rng("bilinear", t.w, t.h); out = []
    lu, lv = _ladder(t.w), _ladder(t.h); n = max(len(lu), len(lv)); lu, lv = np.resize(lu, n), np.resize(np.roll(lv, 1), n)
    for mip in range(t.levels):
        uv = (r.random((24, 2)) * 6 - 3).astype(np.float32)
        uv = np.concatenate([uv, SPECIAL_UV, np.stack([lu, (r.random(n) * 6 - 3).astype(np.float32)], 1), np.stack([np.roll(lu, 2), lv], 1)])
        out.append(_rows(1, t.index, uv[:, 0], uv[:, 1], np.uint32(mip)))
    iu, iv = np.arange(t.w + 1), np.arange(t.h + 1)
    cu = np.concatenate([(iu + 0.5) / t.w, iu / t.w]).astype(np.float32); cv = np.concatenate([(iv + 0.5) / t.h, iv / t.h]).astype(np.float32)
    out.append(_rows(1, t.index, cu, (r.random(len(cu)) * 6 - 3).astype(np.float32), np.uint32(0)))
    out.append(_rows(1, t.index, (r.random(len(cv)) * 6 - 3).astype(np.float32), cv, np.uint32(0)))
    k = min(len(cu), len(cv), 96); out.append(_rows(1, t.index, -cu[:k], cv[::-1][:k], np.uint32(0)))      # both axes at once: fraction 0 / 0.5 x fraction 0.5 / 0, left of the origin in u
    return np.concatenate(out)


def material_rows(t):
    """Mode 0 (sampleTexture with the texture's own packed word): lambda = 0.5 * baseLOD + lambdaNoDims at every integer level, between them, below 0, past the last, 1e9."""
    r = _rng("material", t.w, t.h); out = []
    base = 0.5 * (t.word >> 24)
    targets = [-2.0, -0.5] + [l + f for l in range(t.levels) for f in (0.0, 0.25, 0.9375)] + [t.levels + 0.7, 1e9]
    for lam in targets:
        uv = np.concatenate([(r.random((16, 2)) * 6 - 3).astype(np.float32), SPECIAL_UV])
        out.append(_rows(0, t.word, uv[:, 0], uv[:, 1], np.float32(lam - base) if lam < 1e8 else np.float32(1e9)))
    return np.concatenate(out)


def gradient_pairs(t):
    """(gx, gy) [m, 2] each: tap counts 1 .. 16 and the clamp (length ratios k - 0.5, far from the integers where float32 and float64 could disagree about ceil), equal lengths,
    a zero minor gradient, both zero; footprints from below a texel to wider than the texture; along the axes and oblique, either gradient the longer."""
    r = _rng("gradients", t.w, t.h); gx, gy = [], []
    wh = np.float64([t.w, t.h])
    for ratio in [1.0] + [k - 0.5 for k in range(2, 17)] + [25.5, 39.5]:
        for pmax in (0.4, 3.0, 20.0, 150.0):
            for oblique in (False, True):
                a, bb = (r.random(2) * 2 * np.pi) if oblique else (0.0, 0.5 * np.pi)
                major = np.float64([np.cos(a), np.sin(a)]); minor = np.float64([np.cos(bb), np.sin(bb)])
                major = major / np.linalg.norm(major * wh) * pmax; minor = minor / np.linalg.norm(minor * wh) * (pmax / ratio)
                if ratio == 1.0: minor = -major if oblique else major            # lx == ly to the bit
                if (len(gx) & 1): gx.append(minor); gy.append(major)
                else: gx.append(major); gy.append(minor)
    for g in ((0.03, 0.0), (0.0, 0.4), (0.011, -0.007), (1.5, 2.0)):
        gx.append(g); gy.append((0.0, 0.0)); gx.append((0.0, 0.0)); gy.append(g)      # a zero minor gradient: 16 taps
    gx.append((0.0, 0.0)); gy.append((0.0, 0.0))                                     # both zero: level 0
    return np.float32(gx), np.float32(gy)


def anisotropic_rows(t):
    r = _rng("anisotropic", t.w, t.h); gx, gy = gradient_pairs(t); out = []
    for k in range(3):
        uv = SPECIAL_UV[r.integers(0, 16, len(gx))] if k == 2 else (r.random((len(gx), 2)) * 6 - 3).astype(np.float32)
        out.append(_rows(2, t.index, uv[:, 0], uv[:, 1], gx[:, 0], gx[:, 1], gy[:, 0], gy[:, 1]))
    return np.concatenate(out)


def near_rows(t): return np.concatenate([material_rows(t), bilinear_rows(t), anisotropic_rows(t)])


def far_rows(t):
    """THE FAR RANGE, mode 1: 2^25 <= |u * dim| <= 2^30 at the level that is fetched, on every level with a side that is no power of two — where a float32
    `x - floor(x / dim) * dim` leaves [0, dim). Empty for a texture without such a level."""
    r = _rng("far", t.w, t.h); out = []
    for mip in range(t.levels):
        mw, mh = max(1, t.w >> mip), max(1, t.h >> mip)
        if not ((mw & (mw - 1)) | (mh & (mh - 1))): continue
        n = 120
        big = lambda dim: (np.where(r.random(n) < 0.5, -1.0, 1.0) * 2.0 ** (25 + 5 * r.random(n)) / dim).astype(np.float32)
        near = lambda: (r.random(n) * 6 - 3).astype(np.float32)
        u = np.concatenate([big(mw), near(), big(mw)]); v = np.concatenate([near(), big(mh), big(mh)])
        a = np.abs(u[: n].astype(np.float64) * mw); assert (a >= 2.0 ** 25).all() and (a <= 2.0 ** 30).all()
        out.append(_rows(1, t.index, u, v, np.uint32(mip)))
    return np.concatenate(out) if out else np.zeros((0, 8), np.uint32)


def alpha_candidates(n=20000):
    """Random (primitive, u, v) on the zoo scene's quads: uint32 rows of the device's alpha-test probe (kind 10)."""
    sc, texs, quads = zoo(); r = _rng("alpha", n)
    prim = r.integers(0, 2 * len(quads), n).astype(np.uint32)
    u = r.random(n, np.float32); v = r.random(n, np.float32); f = u + v > 1; u[f] = 1 - u[f]; v[f] = 1 - v[f]
    rows = np.zeros((n, 3), np.uint32); rows[:, 0] = prim; rows[:, 1] = u.view(np.uint32); rows[:, 2] = v.view(np.uint32)
    return rows


def alpha_texcoords(rows):
    """The float32 texture coordinate the alpha test forms for each candidate: (t0 * (1 - (u + v)) + t1 * u) + t2 * v of the triangle's three vertices."""
    sc, texs, quads = zoo()
    prim = rows[:, 0].astype(np.int64); u, v = rows[:, 1].copy().view(np.float32), rows[:, 2].copy().view(np.float32)
    uvq = np.stack([q[1] for q in quads])                                     # [quads, 4, 2]
    corner = np.where((prim & 1)[:, None] == 0, np.int64([0, 1, 2]), np.int64([0, 2, 3]))      # scenes.quad: triangles (0, 1, 2), (0, 2, 3)
    t = uvq[(prim >> 1)[:, None], corner]                                     # [n, 3, 2]
    b0 = np.float32(1.0) - (u + v)
    return ((t[:, 0] * b0[:, None]).astype(np.float32) + (t[:, 1] * u[:, None]).astype(np.float32)).astype(np.float32) + (t[:, 2] * v[:, None]).astype(np.float32)


def through_rays(n=20000):
    """Rays along +z (slightly tilted) through the columns of quads: each meets up to one alpha-tested quad per layer."""
    r = _rng("rays", n)
    col = r.integers(0, len(SIZES), n)
    o = np.stack([1.5 * col + r.random(n), r.random(n), np.full(n, -1.0)], 1)
    d = np.stack([0.08 * (r.random(n) - 0.5), 0.08 * (r.random(n) - 0.5), np.ones(n)], 1); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), 1e15)], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def room():
    """(scene, camera keywords) of the whole-frame test: a floor and a row of upright quads with non-square, non-power-of-two base-colour and normal maps, an emissive
    texture (100 x 60, stretched) overhead, one alpha-tested leaf with a float alpha plane, seen by a camera that grazes the floor: the ray cone reaches fractional and
    capped levels."""
    b = scenes.SceneBuilder(); r = _rng("room")
    def normal_map(w, h):
        n = np.concatenate([0.5 + 0.35 * (r.random((h, w, 2)) - 0.5), np.ones((h, w, 1)), np.ones((h, w, 1))], -1)
        return b.add_texture((n * 255).astype(np.uint8), scenes.TEX_RGBA8_UNORM)
    base = [b.add_texture(*make_pixels(w, h, f)) for (w, h, f) in ((257, 129, "srgb8"), (100, 60, "srgb8"), (5, 4, "unorm8"), (64, 2, "srgb8"), (1, 7, "srgb8"))]
    nrm = [normal_map(255, 256), normal_map(3, 3), normal_map(100, 60), normal_map(2, 64), normal_map(128, 32)]
    glow = np.exp(0.8 * r.standard_normal((60, 100, 4))).astype(np.float32); emissive = b.add_texture(glow, scenes.TEX_RGBA32F)
    leaf_px, leaf_fmt = make_pixels(100, 60, "f32_alpha_floats"); leaf_px = np.minimum(leaf_px, np.float32(1.0)); leaf_px[..., 3] = make_pixels(100, 60, "f32_alpha_floats")[0][..., 3]
    leaf = b.add_texture(leaf_px, leaf_fmt)
    def add(corners, mat, uv_scale=(1.0, 1.0), flags=0):
        p, i, uv, n, tg = scenes.quad(*corners)
        b.begin_mesh(); b.add_geometry(p, i, mat, uv=(uv * np.float32(uv_scale)).astype(np.float32), normal=n, tangent=tg, geom_flags=flags); b.add_instance(b.end_mesh())
    add(([-4, 0, -4], [-4, 0, 8], [4, 0, 8], [4, 0, -4]), b.add_material(scenes.make_material(base=(0.9, 0.9, 0.9), base_tex=base[0], normal_tex=nrm[0], roughness=0.6)), (3.0, 2.0))
    for k in range(4):
        x, z = -3.0 + 1.5 * k, 2.0 + 0.8 * k
        add(([x, 0, z], [x, 1.5, z], [x + 1.2, 1.5, z], [x + 1.2, 0, z]), b.add_material(scenes.make_material(base=(0.8, 0.8, 0.8), base_tex=base[k + 1], normal_tex=nrm[k + 1], roughness=0.8)), (1.0 + k, -1.5))
    add(([-1.5, 2.5, 0.5], [1.5, 2.5, 0.5], [1.5, 2.5, 4.0], [-1.5, 2.5, 4.0]), b.add_material(scenes.make_material(base=(0.5, 0.5, 0.5), emissive=(6.0, 5.0, 4.0), emissive_tex=emissive)), (1.7, 0.9))
    add(([-0.6, 0, 0.5], [-0.6, 1.0, 0.5], [0.6, 1.0, 0.5], [0.6, 0, 0.5]), b.add_material(scenes.make_material(base=(0.7, 0.9, 0.6), base_tex=leaf, alpha_cutoff=0.5)), (1.0, 1.0), scenes.GEOMF_ALPHA_TESTED)
    return b.finish(), dict(pos=(0.3, 0.12, -2.5), direction=(-0.05, -0.02, 1.0), up=(0, 1, 0), fov_y=1.0)

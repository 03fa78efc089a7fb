"""A float32 numpy restatement of what a texture ingest makes of its source (rtxpt_amd/csrc/pt_texture_ingest.h): level 0, the mip chain in the written order —
((p00 + p01) + (p10 + p11)) * 0.25, every operation rounded to float32 —, the rule that gives an alpha plane bytes or floats, and the layout of the two pools. What the
host path, the device path (PT_DEVICE_TEXTURES_ON_DEVICE) and the header on the host (tests/texture_ingest_check.cpp) are held to, bit for bit.

Also the second texture set of tests/test_gpu_device_textures.py (the first is tests/texture_cases.zoo()): the sizes at which the chain changes its path."""
import functools
import zlib
import numpy as np

from rtxpt_amd import scenes
import texture_cases as tc

F32 = np.float32
TEX_RGBA8_UNORM, TEX_RGBA8_SRGB, TEX_RGBA32F = 0, 1, 2

# a side reaches 1 while the other goes on; the odd-side clamp on either axis; an odd pair around a power of two; a thin one; more than one block and more than one wave per
# row with a chain of 11 levels
INGEST_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (63, 65), (257, 2), (1024, 512)]
INGEST_FORMATS = ["srgb8", "unorm8", "f32_alpha_bytes", "f32_alpha_floats"]


def level0(pixels, fmt, pow32):
    """float32 [h, w, 4]: byte / 255 in float32, the sRGB transfer function on the colour channels of an sRGB source (pow32: the project's float32 power), floats as they are."""
    if fmt == TEX_RGBA32F: return np.array(pixels, np.float32)
    t = (np.asarray(pixels, np.uint8).astype(np.float32) / F32(255.0)).astype(np.float32)
    if fmt == TEX_RGBA8_SRGB:
        c = t[..., :3].copy()
        lin = (c / F32(12.92)).astype(np.float32)
        base = ((c + F32(0.055)).astype(np.float32) / F32(1.055)).astype(np.float32)
        curve = np.asarray(pow32(base.ravel(), np.full(base.size, 2.4, np.float32)), np.float32).reshape(c.shape)
        t[..., :3] = np.where(c <= F32(0.04045), lin, curve)
    return t


def level_count(w, h):
    lv, m = 1, max(w, h)
    while m > 1: m >>= 1; lv += 1
    return lv


def chain(tex0):
    """Levels 0 .. level_count - 1 in float32, each [mh, mw, 4]: sides max(1, side >> l), source indices min(2 x, pw - 1) and min(2 x + 1, pw - 1) per axis."""
    mips = [np.asarray(tex0, np.float32)]
    while max(mips[-1].shape[:2]) > 1:
        p = mips[-1]; ph, pw = p.shape[:2]; mh, mw = max(1, ph >> 1), max(1, pw >> 1)
        x0, x1 = np.minimum(2 * np.arange(mw), pw - 1), np.minimum(2 * np.arange(mw) + 1, pw - 1)
        y0, y1 = np.minimum(2 * np.arange(mh), ph - 1), np.minimum(2 * np.arange(mh) + 1, ph - 1)
        top = (p[y0][:, x0] + p[y0][:, x1]).astype(np.float32); bottom = (p[y1][:, x0] + p[y1][:, x1]).astype(np.float32)
        mips.append(((top + bottom).astype(np.float32) * F32(0.25)).astype(np.float32))
    assert len(mips) == level_count(tex0.shape[1], tex0.shape[0])
    return mips


def alpha_byte(a):
    """(int)(a * 255.0f + 0.5f), for opacities in [0, 1]."""
    return ((np.asarray(a, np.float32) * F32(255.0)).astype(np.float32) + F32(0.5)).astype(np.float32).astype(np.int64)


def alpha_is_byte(a):
    """Per opacity: in [0, 1] and returned by the quotient of its own rounded byte."""
    a = np.asarray(a, np.float32); inside = (a >= 0) & (a <= 1)
    q = alpha_byte(np.where(inside, a, F32(0.0)))
    return inside & ((q.astype(np.float32) / F32(255.0)).astype(np.float32) == a)


def alpha_plane(tex0):
    """(fmt, plane) of a level 0: fmt 0 and uint8 [texels] where every opacity is k / 255, else fmt 1 and float32 [texels]."""
    a = np.ascontiguousarray(tex0[..., 3], np.float32).ravel()
    if alpha_is_byte(a).all(): return 0, alpha_byte(a).astype(np.uint8)
    return 1, a.copy()


def layout(sizes, plane_fmts):
    """The tables of both pools: per texture (base, [offset of every level from the base]) in texels and the byte offset of its alpha plane; the texels of the material textures;
    the bytes of the alpha pool (every plane on a 16-byte boundary, the pool's end too, never empty)."""
    base, at, out = 0, 0, []
    for (w, h), fmt in zip(sizes, plane_fmts):
        offs, off = [], 0
        for l in range(level_count(w, h)): offs.append(off); off += max(1, w >> l) * max(1, h >> l)
        at = (at + 15) & ~15
        out.append((base, offs, at)); base += off; at += w * h * (1 if fmt == 0 else 4)
    return out, base, max(16, (at + 15) & ~15)


def digest(arrays):
    c = 0
    for a in arrays: c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


class Set:
    """A texture set as a scene: textures only matter, one untextured quad keeps the geometry valid."""
    def __init__(self, entries):
        b = scenes.SceneBuilder(); self.texs = []
        for (w, h, fmt, px, upload) in entries:
            word = b.add_texture(px, upload); self.texs.append(tc.Tex(len(self.texs), w, h, fmt, px, upload, word))
        m = b.add_material(scenes.make_material())
        p, i, uv, n, tg = scenes.quad([0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0])
        b.begin_mesh(); b.add_geometry(p, i, m, uv=uv, normal=n, tangent=tg); b.add_instance(b.end_mesh())
        self.scene = b.finish()


@functools.lru_cache(maxsize=None)
def ingest_set():
    """Every size of INGEST_SIZES in every format of INGEST_FORMATS."""
    return Set([(w, h, f) + tc.make_pixels(w, h, f) for (w, h) in INGEST_SIZES for f in INGEST_FORMATS])


@functools.lru_cache(maxsize=None)
def many_small(n=300):
    """n textures of 4 x 4, the formats in turn: the launch count must not follow the number of textures, and a small staging buffer cuts inside a texture and between two."""
    out = []
    for k in range(n):
        f = INGEST_FORMATS[k % len(INGEST_FORMATS)]; r = tc._rng("small", k)
        if f in ("srgb8", "unorm8"): px, up = r.integers(0, 256, (4, 4, 4)).astype(np.uint8), (scenes.TEX_RGBA8_SRGB if f == "srgb8" else scenes.TEX_RGBA8_UNORM)
        else:
            px = np.exp(r.standard_normal((4, 4, 4))).astype(np.float32); up = scenes.TEX_RGBA32F
            px[..., 3] = r.integers(0, 256, (4, 4)).astype(np.float32) / F32(255.0) if f == "f32_alpha_bytes" else r.random((4, 4), np.float32)
        out.append((4, 4, f, px, up))
    return Set(out)


_REFERENCE = {}


def reference(which, pow32):
    """[(levels, (plane fmt, plane))] of a texture set ("zoo", "ingest", "small"), computed once and left unchanged."""
    if which not in _REFERENCE:
        texs = {"zoo": lambda: tc.zoo()[1], "ingest": lambda: ingest_set().texs, "small": lambda: many_small().texs}[which]()
        out = []
        for t in texs:
            m = chain(level0(t.pixels, t.upload, pow32)); out.append((m, alpha_plane(m[0])))
        _REFERENCE[which] = out
    return _REFERENCE[which]

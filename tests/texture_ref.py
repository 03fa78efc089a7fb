"""A float64 restatement of the project's texture sampler in plain numpy: what pt_scene.h (device) and oracle/ptref/scene.h (oracle) are both held to.

The definition. A texture is w x h RGBA texels. Level 0 is what the upload makes of the source: k / 255 in float32 for 8-bit sources, the sRGB transfer function on the
colour channels of an sRGB source in float32, float32 sources as they are. From there on everything is float64: level l + 1 is the 2 x 2 box filter of level l (side
max(1, side >> 1); a source index past an odd side's last texel is clamped to it), texel centres lie at (i + 0.5) / dim, addressing wraps with an exact integer modulo,
a fetch at one level is bilinear, a fetch at a fractional level blends the two neighbouring levels, and the anisotropic filter averages N trilinear taps spaced evenly along
the longer of two gradients (EXT_texture_filter_anisotropic: N = min(ceil(Pmax / Pmin), 16), level log2(Pmax / N)).

What stays float32: the COORDINATE STEP — fx = float32(float32(u * w) - 0.5), its floor and its fraction, the level arithmetic (0.5 * baseLOD + lambda, the clamp, the floor,
the fraction), the gradient lengths, the tap count and the tap positions. Those are inputs of the filter, formed in float32 by both texts under test; doing them here in the
same precision keeps a weight's rounding from being charged to the filter. Two float32 library functions enter them: the power of the sRGB decode and the logarithm of the
anisotropic level. The project has its own (pt_dmath.h, held to references by tests of their own); a caller hands them in (`pow32`, `log2_32`), the defaults are numpy's.

The tolerance, derived (u = 2^-24, the relative error of one float32 rounding; M = the largest |texel| of the channel at level 0, which bounds every level):
  * a box-filter level forms (a + b) + (c + d) and scales by 0.25 (exact): three rounded additions, at most u (|a + b| + |c + d| + |sum|) / 4 <= 2 u M of new error on top of
    the (averaged, hence not grown) error of the level above. A texel of level L carries at most 2 L u M; the bound grants 3 L u M, one rounding per addition.
  * lerp(a, b, t) = a + (b - a) * t rounds three times: the difference, the product, the sum — at most u (2 t |b - a| + |result|) <= 3 u M for texels of one sign, and
    inherits at most max(error of a, error of b). Bilinear nests two (6 u M), trilinear three (9 u M).
  * so a fetch that reaches level L >= 1 is within (2 L + 9) u M <= (3 L + 8) u M, a fetch of level 0 alone within 6 u M <= 8 u M:
        |value - ref64| <= (3 L + 8) * 2^-24 * M        per channel, L = the deepest level the fetch reads.
  * the one signed channel of the zoo (opacities in [-0.25, 1.25]: |b - a| <= 1.2 M) has a first-order worst case of 3.4 u M per lerp, which exceeds the bound by at most
    1.2 u M at L < 3 and only if every rounding of the chain falls the same way at t -> 1; the N-tap average adds a running sum of N values and a division. Neither is in the
    count above. The tests print the largest observed error / bound per texture; were one above 1 the missing step would be one of these two.
"""
import numpy as np

F32 = np.float32
U24 = 2.0 ** -24
FLT_MIN, FLT_MAX = np.finfo(np.float32).tiny, np.finfo(np.float32).max
TEX_RGBA8_UNORM, TEX_RGBA8_SRGB, TEX_RGBA32F = 0, 1, 2


def level0(pixels, fmt, pow32=None):
    """The float32 texels the upload makes of a source: [h, w, 4]."""
    if fmt == TEX_RGBA32F: return np.array(pixels, np.float32)
    t = np.asarray(pixels, np.uint8).astype(np.float32) / F32(255.0)
    if fmt == TEX_RGBA8_SRGB:
        pw = pow32 or (lambda x, y: np.power(x, y, dtype=np.float32))
        c = t[..., :3]
        t[..., :3] = np.where(c <= F32(0.04045), c / F32(12.92), pw(((c + F32(0.055)) / F32(1.055)).astype(np.float32), np.full(c.shape, 2.4, np.float32)).reshape(c.shape))
    return t


def build_mips(tex0):
    """Levels 0 .. floor(log2(max(w, h))) in float64, each [mh, mw, 4]."""
    mips = [np.asarray(tex0, np.float32).astype(np.float64)]
    while max(mips[-1].shape[:2]) > 1:
        p = mips[-1]; ph, pw = p.shape[:2]; mh, mw = max(1, ph >> 1), max(1, pw >> 1)
        x0, x1 = np.minimum(2 * np.arange(mw), pw - 1), np.minimum(2 * np.arange(mw) + 1, pw - 1)
        y0, y1 = np.minimum(2 * np.arange(mh), ph - 1), np.minimum(2 * np.arange(mh) + 1, ph - 1)
        mips.append(0.25 * (p[y0][:, x0] + p[y0][:, x1] + p[y1][:, x0] + p[y1][:, x1]))
    return mips


def _coord(u, dim):
    """The float32 coordinate step along one axis: (first texel before wrapping, as int64; the weight of the second)."""
    fx = (np.asarray(u, np.float32) * F32(dim)).astype(np.float32) - F32(0.5)
    fl = np.floor(fx)
    return fl.astype(np.int64), (fx - fl).astype(np.float64)


def bilinear_level(m, u, v):
    """Bilinear fetch of one level `m` [mh, mw, 4] at float32 coordinates u, v [n] -> float64 [n, 4]."""
    mh, mw = m.shape[:2]
    x0, ax = _coord(u, mw); y0, ay = _coord(v, mh)
    xa, xb, ya, yb = x0 % mw, (x0 + 1) % mw, y0 % mh, (y0 + 1) % mh
    ax, ay = ax[:, None], ay[:, None]
    a = m[ya, xa] + (m[ya, xb] - m[ya, xa]) * ax
    b = m[yb, xa] + (m[yb, xb] - m[yb, xa]) * ax
    return a + (b - a) * ay


def bilinear(mips, mip, u, v):
    """sample_bilinear at integer levels `mip` [n] (or one level)."""
    u, v = np.atleast_1d(np.asarray(u, np.float32)), np.atleast_1d(np.asarray(v, np.float32))
    mip = np.broadcast_to(np.asarray(mip, np.int64), u.shape)
    out = np.zeros((len(u), 4))
    for l in np.unique(mip):
        k = mip == l; out[k] = bilinear_level(mips[l], u[k], v[k])
    return out


def trilinear(mips, u, v, lam):
    """sample_trilinear at float32 levels `lam` [n] -> (float64 [n, 4], the deepest level each row read [n])."""
    u, v, lam = (np.atleast_1d(np.asarray(a, np.float32)) for a in (u, v, lam))
    last = len(mips) - 1
    l = np.minimum(np.maximum(lam, F32(0.0)), F32(last)); l0 = np.floor(l); f = (l - l0).astype(np.float64)
    m0 = l0.astype(np.int64); m1 = np.minimum(m0 + 1, last)
    a = bilinear(mips, m0, u, v)
    two = (f != 0.0) & (m1 != m0)
    if two.any():
        b = bilinear(mips, m1[two], u[two], v[two])
        a[two] = a[two] + (b - a[two]) * f[two, None]
    return a, np.where(two, m1, m0)


def sample_texture(mips, word, lam_no_dims, u, v):
    """The material path (sampleTexture): the packed texture word's baseLOD and its mipLevels - 5 cap in float32, then trilinear."""
    base_lod, levels = F32(word >> 24), F32((word >> 16) & 0xFF)
    lam = (F32(0.5) * base_lod + np.atleast_1d(np.asarray(lam_no_dims, np.float32))).astype(np.float32)
    lam = np.minimum(lam, np.maximum(levels - F32(5.0), F32(0.0)))
    return trilinear(mips, u, v, lam)


def anisotropic_setup(w, h, gx, gy, log2_32=None):
    """The float32 footprint arithmetic of the N-tap filter: (n [rows] float32, lod [rows] float32, major [rows, 2] float32)."""
    gx, gy = np.asarray(gx, np.float32).reshape(-1, 2), np.asarray(gy, np.float32).reshape(-1, 2)
    lg = log2_32 or (lambda x: np.log2(x, dtype=np.float32))
    def length(g):
        a, b = (g[:, 0] * F32(w)).astype(np.float32), (g[:, 1] * F32(h)).astype(np.float32)
        return np.sqrt(((a * a).astype(np.float32) + (b * b).astype(np.float32)).astype(np.float32), dtype=np.float32)
    lx, ly = length(gx), length(gy)
    pmax, pmin = np.maximum(lx, ly), np.minimum(lx, ly)
    major = np.where((lx >= ly)[:, None], gx, gy)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(pmin > 0, np.ceil((pmax / pmin).astype(np.float32)), F32(16.0)).astype(np.float32)
        n = np.minimum(np.maximum(n, F32(1.0)), F32(16.0))
        arg = np.minimum(np.maximum((pmax / n).astype(np.float32), FLT_MIN), FLT_MAX).astype(np.float32)
    lod = np.where(pmax > 0, np.asarray(lg(arg), np.float32).reshape(arg.shape), F32(0.0)).astype(np.float32)
    return n, lod, major


def anisotropic_taps(mips, u, v, n, lod, major):
    """The average of n[row] trilinear taps at level lod[row], spaced evenly along major[row] about (u, v) -> (float64 [rows, 4], deepest level [rows])."""
    u, v = np.atleast_1d(np.asarray(u, np.float32)), np.atleast_1d(np.asarray(v, np.float32))
    n, lod, major = np.asarray(n, np.float32), np.asarray(lod, np.float32), np.asarray(major, np.float32)
    acc = np.zeros((len(u), 4)); deep = np.zeros(len(u), np.int64)
    for i in range(16):
        k = i < n
        if not k.any(): break
        o = ((F32(i) + F32(0.5)) / n[k]).astype(np.float32) - F32(0.5)
        tu, tv = u[k] + (major[k, 0] * o).astype(np.float32), v[k] + (major[k, 1] * o).astype(np.float32)
        val, lv = trilinear(mips, tu, tv, lod[k])
        acc[k] += val; deep[k] = np.maximum(deep[k], lv)
    return acc / n[:, None].astype(np.float64), deep


def anisotropic(mips, u, v, gx, gy, log2_32=None):
    """sample_grad_anisotropic -> (float64 [n, 4], deepest level [n], tap count [n], lod [n])."""
    h, w = mips[0].shape[:2]
    n, lod, major = anisotropic_setup(w, h, gx, gy, log2_32)
    val, deep = anisotropic_taps(mips, u, v, n, lod, major)
    return val, deep, n, lod


def bound(mips, deepest):
    """(3 L + 8) * 2^-24 * max |texel of the channel|: [n, 4] for the deepest levels [n] the rows read (module docstring)."""
    M = np.abs(mips[0]).reshape(-1, 4).max(0)
    return (3.0 * np.asarray(deepest, np.float64)[:, None] + 8.0) * U24 * M[None, :]


def numpy_anisotropic(tex, uv, gx, gy):
    """One anisotropic fetch of the colour channels of a float texture [h, w, >= 3], w != h allowed, with the footprint (tap count, level) worked out in float64
    -> (rgb, tap count, lod): the emissive-bake test's reference (tests/test_emissive_bake_anisotropy.py)."""
    t4 = np.zeros(tex.shape[:2] + (4,), np.float32); t4[..., :min(4, tex.shape[2])] = tex[..., :4]
    mips = build_mips(t4)
    h, w = tex.shape[:2]
    lx, ly = np.hypot(gx[0] * w, gx[1] * h), np.hypot(gy[0] * w, gy[1] * h)
    pmax, pmin = max(lx, ly), min(lx, ly); major = np.array(gx if lx >= ly else gy)
    n = min(max(np.ceil(pmax / pmin), 1.0), 16.0) if pmin > 0 else 16.0
    lod = min(max(np.log2(pmax / n), 0.0), len(mips) - 1.0) if pmax > 0 else 0.0
    val, _ = anisotropic_taps(mips, [uv[0]], [uv[1]], [n], [lod], [major])
    return val[0, :3], n, lod

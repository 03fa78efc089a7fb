"""An independent numpy restatement of the bloom pass (rtxpt_amd/csrc/pt_bloom.h, docs/WIDENING.md N7) and of pt_bloom_kernel. A sibling of taa_ref.py with the same arithmetic
rules: every step one binary32 operation in the stated order (numpy float32 arrays and constants), coordinates clamped to the image (an edge texel repeats), the 4 x 4 block
summed from 0 in scan-line order and then multiplied by 0.0625, the blur as acc = c x g[0], acc = acc + (l_i + r_i) x g[i] for i = 1 .. R and then acc / G — first along x, then
along y — the bilinear 2 x 2 in the order (0, 0) (1, 0) (0, 1) (1, 1) summed from 0, out = s + (b - s) x intensity. The taps are evaluated in double with math.exp (the C
library's exp, the function the library calls) and rounded to binary32; their sum G is accumulated in binary32. The device is held to it bit for bit
(tests/test_gpu_zzzzz_bloom.py); tests/test_bloom.py holds it to answers worked by hand. None of this is Donut's BloomPass, and nothing here is compared with it.

Parameters are anything indexable by the names of PtBloomParams (a dict from params(), or a record of rtxpt_amd.BLOOM_PARAMS_DTYPE)."""
import math
import numpy as np
import taa_ref as taa

f32 = np.float32
sanitise = taa.sanitise

# SampleUI.h:305-307; maxRadiance is the project's own
DEFAULTS = dict(radius=8.0, intensity=0.004, maxRadiance=10000.0, enable=1)
MAX_TAPS = 48


def params(**kw):
    unknown = set(kw) - set(DEFAULTS); assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def skipped(P):
    """the reference's skip condition (Sample.cpp:1834): !(EnableBloom && BloomIntensity > 0 && BloomRadius > 0)"""
    return not (int(P["enable"]) and f32(P["intensity"]) > 0 and f32(P["radius"]) > 0)


def kernel(radius):
    """pt_bloom_kernel: (g[0 .. R] as float32, G as float32); ValueError for the radii the library refuses"""
    radius = f32(radius)
    if not (radius > 0 and radius <= 64): raise ValueError("radius %r: only (0, 64]" % (radius,))
    sigma = 0.25 * float(radius)
    R = max(1, math.ceil(3.0 * sigma)); assert R <= MAX_TAPS
    g = np.array([1.0] + [math.exp(-float(i * i) / (2.0 * sigma * sigma)) for i in range(1, R + 1)]).astype(f32)
    G = f32(1)
    for i in range(1, R + 1): G = f32(G + g[i] * f32(2))
    return g, G


def reduce(s):
    """the sanitised picture [h, w, 3] -> Q [ceil(h / 4), ceil(w / 4), 3]"""
    h, w = s.shape[:2]
    qh, qw = (h + 3) // 4, (w + 3) // 4
    ys, xs = np.mgrid[0:qh, 0:qw]
    acc = np.zeros((qh, qw, 3), f32)
    for j in range(4):
        for i in range(4): acc = acc + s[np.clip(4 * ys + j, 0, h - 1), np.clip(4 * xs + i, 0, w - 1)]
    return acc * f32(0.0625)


def blur_axis(q, g, G, axis):
    """one axis of the blur over [qh, qw, 3]: axis 1 is x, axis 0 is y"""
    n = q.shape[axis]
    idx = np.arange(n)
    acc = q * g[0]
    for i in range(1, len(g)):
        l, r = np.take(q, np.clip(idx - i, 0, n - 1), axis), np.take(q, np.clip(idx + i, 0, n - 1), axis)
        acc = acc + (l + r) * g[i]
    return acc / G


def blur(q, radius):
    """Q -> B: first along x (T), then along y"""
    g, G = kernel(radius)
    return blur_axis(blur_axis(q, g, G, 1), g, G, 0)


def _tap(n):
    """full-resolution coordinates 0 .. n - 1 -> (first tap, fraction) in the quarter-resolution image"""
    u = (np.arange(n).astype(f32) + f32(0.5)) * f32(0.25) - f32(0.5)
    fl = np.floor(u).astype(f32)
    return fl.astype(np.int64), u - fl


def upsample(B, w, h):
    """the bilinear value of B [qh, qw, 3] at every full-resolution pixel -> [h, w, 3]"""
    qh, qw = B.shape[:2]
    (ix, tx), (iy, ty) = _tap(w), _tap(h)
    ix, iy, tx, ty = ix[None, :], iy[:, None], tx[None, :], ty[:, None]
    one = f32(1)
    bw = [(one - tx) * (one - ty), tx * (one - ty), (one - tx) * ty, tx * ty]
    r = np.zeros((h, w, 3), f32)
    for k in range(4): r = r + B[np.clip(iy + (k >> 1), 0, qh - 1), np.clip(ix + (k & 1), 0, qw - 1)] * bw[k][..., None]
    return r


def composite(s, b, intensity):
    """out.rgb = s + (b - s) x intensity"""
    return s + (b - s) * f32(intensity)


def bloom(source, P, stages=None):
    """pt_bloom over the picture [h, w, 4] -> the bloomed picture [h, w, 4] (the skipped pass: a copy of the source). stages (a dict): receives the sanitised colour s, the
    reduced image Q, the blurred image B and its upsampled value b."""
    source = np.asarray(source, f32)
    if skipped(P): return source.copy()
    h, w = source.shape[:2]
    with np.errstate(all="ignore"):
        s = sanitise(source, P["maxRadiance"])
        Q = reduce(s)
        B = blur(Q, P["radius"])
        b = upsample(B, w, h)
        out = composite(s, b, P["intensity"])
    if stages is not None: stages.update(s=s, Q=Q, B=B, b=b)
    return np.concatenate([out, np.ones((h, w, 1), f32)], -1)

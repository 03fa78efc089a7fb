"""An independent numpy restatement of the temporal anti-aliasing resolve (rtxpt_amd/csrc/pt_taa.h, docs/WIDENING.md N6) and of pt_taa_jitter. A sibling of relax_ref.py with the
same arithmetic rules: every step one binary32 operation in the stated order (numpy float32 arrays and constants), luminance as (x + y) + z, min / max as comparisons, the 3 x 3
in scan-line order (dy outer, dx inner) with coordinates clamped to the frame, Catmull-Rom rows summed left to right from 0 and then the rows top to bottom from 0, the bilinear
2 x 2 in the order (0, 0) (1, 0) (0, 1) (1, 1). The device is held to it bit for bit (tests/test_gpu_zzzz_taa_resolve.py); tests/test_taa_resolve.py holds it to answers
worked by hand. None of this is Donut's TemporalAntiAliasingPass, and nothing here is compared with it.

Parameters are anything indexable by the names of PtTaaParams (a dict from params(), or a record of rtxpt_amd.TAA_PARAMS_DTYPE)."""
import math
import numpy as np
import denoiser_inputs_ref as ref

f32 = np.float32
FLT_MAX = ref.FLT_MAX
fmax, fmin, luminance = ref.fmax, ref.fmin, ref.luminance

# SampleUI.cpp:1198-1200, 161, Sample.cpp:1311; clampingFactor, maxRadiance and luminanceWeighted are the project's own
DEFAULTS = dict(newFrameWeight=0.1, clampingFactor=1.0, maxRadiance=10000.0, enableHistoryClamping=1, useHistoryClampRelax=1, useCatmullRomFilter=1, luminanceWeighted=1)
HISTORY_CLAMP_RELAX_MUL = f32(3)
JITTER_HALTON, JITTER_R2 = 1, 2
R2_ALPHA = (0.7548776662466927, 0.5698402909980532)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS); assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def sanitise(colour, max_radiance):
    """[h, w, >= 3] -> the sanitised rgb [h, w, 3]: a component that is not finite counts as 0, then [0, maxRadiance]"""
    c = np.asarray(colour, f32)[..., :3]
    with np.errstate(invalid="ignore"):
        c = np.where(np.abs(c) <= FLT_MAX, c, f32(0)).astype(f32)
    return fmin(fmax(c, f32(0)), f32(max_radiance))


def _clamped(a, ys, xs):
    h, w = a.shape[:2]
    return a[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)]


def dilated_motion(mv):
    """the motion vector of the 3 x 3 tap with the largest squared length; the first in scan-line order among equals"""
    mv = np.asarray(mv, f32)[..., :2]
    h, w = mv.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        len2 = mv[..., 0] * mv[..., 0] + mv[..., 1] * mv[..., 1]
        best, best_len = _clamped(mv, ys - 1, xs - 1).copy(), _clamped(len2, ys - 1, xs - 1).copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                m, l = _clamped(mv, ys + dy, xs + dx), _clamped(len2, ys + dy, xs + dx)
                take = l > best_len
                best = np.where(take[..., None], m, best).astype(f32); best_len = np.where(take, l, best_len).astype(f32)
    return best


def catmull_rom(t):
    """the weights of the taps at floor - 1 .. floor + 2 for the fraction t"""
    t = np.asarray(t, f32); one, half = f32(1), f32(0.5)
    return [t * (f32(-0.5) + t * (one - half * t)), one + (t * t) * (f32(-2.5) + f32(1.5) * t), t * (half + t * (f32(2) - f32(1.5) * t)), (t * t) * (f32(-0.5) + half * t)]


def sample_history(hist, px, py, catmull=True):
    """the history [h, w, >= 3] at the previous positions (px, py) (pixels; texel centres at + 0.5) -> [.., 3]; positions must be finite"""
    hist = np.asarray(hist, f32)[..., :3]
    px, py = np.asarray(px, f32), np.asarray(py, f32)
    fx, fy = px - f32(0.5), py - f32(0.5)
    flx, fly = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
    tx, ty = fx - flx, fy - fly
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    r = np.zeros(px.shape + (3,), f32)
    if catmull:
        wx, wy = catmull_rom(tx), catmull_rom(ty)
        for j in range(4):
            s = np.zeros(px.shape + (3,), f32)
            for i in range(4): s = s + _clamped(hist, iy - 1 + j, ix - 1 + i) * wx[i][..., None]
            r = r + s * wy[j][..., None]
    else:
        one = f32(1)
        bw = [(one - tx) * (one - ty), tx * (one - ty), (one - tx) * ty, tx * ty]
        for k in range(4): r = r + _clamped(hist, iy + (k >> 1), ix + (k & 1)) * bw[k][..., None]
    return fmax(r, f32(0))


def neighbourhood(c):
    """per channel mean and sigma of the 3 x 3 around every pixel of the sanitised colour [h, w, 3]"""
    h, w = c.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    s1, s2 = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            t = _clamped(c, ys + dy, xs + dx)
            s1 = s1 + t; s2 = s2 + t * t
    mean, m2 = s1 / f32(9), s2 / f32(9)
    return mean, np.sqrt(fmax(m2 - mean * mean, f32(0))).astype(f32)


def resolve(colour, motion, relax, history, P, stages=None):
    """pt_taa_resolve. colour: the radiance buffer [h, w, 4]; motion: the build pass's motion vectors as float32 [h, w, >= 2] (pixels); relax: nrdCombinedHistoryClampRelax
    as uint8 [h, w], or None where the library reads it as 0; history: the previous call's result, or None (first frame, reset, dropped). Returns [h, w, 4], alpha 1.
    stages (a dict): receives the sanitised colour, the dilated motion, validity, and the history as sampled and as clamped."""
    h, w = np.asarray(colour).shape[:2]
    c = sanitise(colour, P["maxRadiance"]); lum_c = luminance(c)
    out = np.concatenate([c, np.ones((h, w, 1), f32)], -1)
    if stages is not None: stages["colour"] = c
    if history is None: return out
    with np.errstate(all="ignore"):
        mv = dilated_motion(motion)
        ys, xs = np.mgrid[0:h, 0:w]
        px, py = (xs.astype(f32) + f32(0.5)) + mv[..., 0], (ys.astype(f32) + f32(0.5)) + mv[..., 1]
        valid = (px >= 0) & (px <= f32(w)) & (py >= 0) & (py <= f32(h))
        hst = sample_history(history, np.where(valid, px, f32(0.5)).astype(f32), np.where(valid, py, f32(0.5)).astype(f32), bool(int(P["useCatmullRomFilter"])))
        if stages is not None: stages.update(motion=mv, valid=valid, history=hst.copy())
        if int(P["enableHistoryClamping"]):
            mean, sigma = neighbourhood(c)
            rl = ref.load_unorm8(np.asarray(relax, np.uint8)) if relax is not None and int(P["useHistoryClampRelax"]) else np.zeros((h, w), f32)
            k = f32(P["clampingFactor"]) * (f32(1) + HISTORY_CLAMP_RELAX_MUL * rl)
            lo, hi = mean - sigma * k[..., None], mean + sigma * k[..., None]
            hst = fmin(fmax(hst, lo), hi)
            if stages is not None: stages.update(mean=mean, sigma=sigma)
        if stages is not None: stages["history_clamped"] = hst.copy()
        alpha = f32(P["newFrameWeight"])
        if int(P["luminanceWeighted"]):
            wc, wh = f32(1) / (f32(1) + lum_c), f32(1) / (f32(1) + luminance(hst))
            a, b = alpha * wc, (f32(1) - alpha) * wh
            beta = a / (a + b)
        else:
            beta = np.full((h, w), alpha, f32)
        r = hst + (c - hst) * beta[..., None]
    out[..., :3] = np.where(valid[..., None], r, c)
    return out


def _radical_inverse(i, b):
    num, den = 0, 1
    while i: num = num * b + i % b; den *= b; i //= b
    return num / den      # (one correctly rounded double division of two exact integers)


def jitter(sequence, frame_index):
    """pt_taa_jitter: (x, y) as float32, in [-0.5, 0.5); ValueError for the sequences the library refuses"""
    i = int(frame_index) + 1
    if sequence == JITTER_HALTON: v = (_radical_inverse(i, 2) - 0.5, _radical_inverse(i, 3) - 0.5)
    elif sequence == JITTER_R2: v = tuple(math.fmod(0.5 + i * a, 1.0) - 0.5 for a in R2_ALPHA)
    else: raise ValueError("sequence %r: only 1 (Halton) and 2 (R2)" % (sequence,))
    return tuple(f32(0.49999997) if f32(x) >= f32(0.5) else f32(x) for x in v)

"""An independent numpy restatement of the temporal upscaling resolve (rtxpt_amd/csrc/pt_taau.h, docs/WIDENING.md N8) and of pt_upscale_tex_lod_bias. A sibling of taa_ref.py
with the same arithmetic rules: every step one binary32 operation in the stated order (numpy float32 arrays and constants), min / max as comparisons, the nine taps in scan-line
order (dy outer, dx inner), texels from the clamped coordinate and distances from the unclamped one. As the product reuses TAA_SampleHistory / TAA_ClampHistory / TAA_Blend,
this file takes the sanitiser, the history sampler, the relax multiplier and the defaults from taa_ref; the clamp and the blend are taa_ref.resolve's own lines applied to the
nine taps' sums (taa_ref has them inline, over the pixel's own 3 x 3). The device is held to it bit for bit (tests/test_gpu_zzzzzz_taa_upscale.py); tests/test_taa_upscale.py
holds it to answers worked by hand and to taa_ref.resolve at ratio 1.

Parameters are anything indexable by the names of PtTaaUpscaleParams' fields, the nested PtTaaParams flattened (a dict from params(), or a record of
rtxpt_amd.TAA_UPSCALE_PARAMS_DTYPE)."""
import numpy as np
import denoiser_inputs_ref as ref
import taa_ref as taa

f32 = np.float32
fmax, fmin, luminance = ref.fmax, ref.fmin, ref.luminance

DEFAULTS = dict(taa.DEFAULTS, kernelRadius=1.0, confidenceWeighted=1)      # the two new fields are the project's own


def params(**kw):
    unknown = set(kw) - set(DEFAULTS); assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def taa_params(P):
    """the PtTaaParams part, for taa_ref.resolve"""
    return {k: P[k] for k in taa.DEFAULTS}


def tex_lod_bias(render_w, render_h, display_w, display_h):
    """pt_upscale_tex_lod_bias (Sample.cpp:1504): the products in uint32, the quotient and the root in float32; log2 is the platform's"""
    num, den = np.uint32((display_w * display_h) & 0xFFFFFFFF), np.uint32((render_w * render_h) & 0xFFFFFFFF)
    return -np.log2(np.sqrt(f32(num) / f32(den), dtype=f32), dtype=f32)


def footprint(w, h, W, H, jitter=(0.0, 0.0), radius=1.0):
    """per display pixel: the nearest sample (i0, j0) [H, W] each, and the nine taps' weights [H, W, 3 (dy), 3 (dx)]"""
    jx, jy = f32(jitter[0]), f32(jitter[1]); R = f32(radius)
    rx, ry, inv_r2 = f32(w) / f32(W), f32(h) / f32(H), f32(1) / (R * R)
    Ys, Xs = np.mgrid[0:H, 0:W]
    u, v = (Xs.astype(f32) + f32(0.5)) * rx, (Ys.astype(f32) + f32(0.5)) * ry
    i0 = np.clip(np.floor(u + jx).astype(np.int64), 0, w - 1); j0 = np.clip(np.floor(v + jy).astype(np.int64), 0, h - 1)
    wk = np.zeros((H, W, 3, 3), f32)
    for dy in (-1, 0, 1):
        ddy = (((j0 + dy).astype(f32) + f32(0.5)) - jy) - v
        for dx in (-1, 0, 1):
            ddx = (((i0 + dx).astype(f32) + f32(0.5)) - jx) - u
            a = fmax(f32(1) - (ddx * ddx + ddy * ddy) * inv_r2, f32(0))
            wk[:, :, dy + 1, dx + 1] = a * a
    return i0, j0, wk


def upscale(colour, motion, relax, history, P, display, jitter=(0.0, 0.0), stages=None):
    """pt_taa_upscale. colour: the radiance buffer [h, w, 4] at the render size; motion: the build pass's motion vectors as float32 [h, w, >= 2] (render pixels; None: zero);
    relax: nrdCombinedHistoryClampRelax as uint8 [h, w], or None where the library reads it as 0; history: the previous call's result [H, W, 4], or None (first frame, reset,
    dropped); display: (W, H); jitter: the frame's camera offset in render pixels. Returns [H, W, 4], alpha 1.
    stages (a dict): receives the current colour, the weights, the nearest samples, the dilated motion, validity, the previous positions and the history as sampled."""
    h, w = np.asarray(colour).shape[:2]; W, H = display
    assert w <= W <= 4 * w and h <= H <= 4 * h
    c = taa.sanitise(colour, P["maxRadiance"])
    mvs = np.zeros((h, w, 2), f32) if motion is None else np.asarray(motion, f32)[..., :2]
    i0, j0, wk = footprint(w, h, W, H, jitter, P["kernelRadius"])
    cl = lambda a, ys, xs: a[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)]
    with np.errstate(all="ignore"):
        len2 = mvs[..., 0] * mvs[..., 0] + mvs[..., 1] * mvs[..., 1]
        num, s1, s2 = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
        den, conf = np.zeros((H, W), f32), np.zeros((H, W), f32)
        best, best_len = cl(mvs, j0 - 1, i0 - 1).copy(), cl(len2, j0 - 1, i0 - 1).copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                t, k = cl(c, j0 + dy, i0 + dx), wk[:, :, dy + 1, dx + 1]
                num = num + t * k[..., None]; den = den + k; conf = fmax(conf, k)
                s1 = s1 + t; s2 = s2 + t * t
                m, l = cl(mvs, j0 + dy, i0 + dx), cl(len2, j0 + dy, i0 + dx)
                take = l > best_len
                best = np.where(take[..., None], m, best).astype(f32); best_len = np.where(take, l, best_len).astype(f32)
        cur = num / den[..., None]; lum_c = luminance(cur)
        out = np.concatenate([cur, np.ones((H, W, 1), f32)], -1)
        if stages is not None: stages.update(current=cur, weights=wk, nearest=(i0, j0), confidence=conf, motion=best)
        if history is None: return out
        sx, sy = f32(W) / f32(w), f32(H) / f32(h)
        Ys, Xs = np.mgrid[0:H, 0:W]
        px, py = (Xs.astype(f32) + f32(0.5)) + best[..., 0] * sx, (Ys.astype(f32) + f32(0.5)) + best[..., 1] * sy
        valid = (px >= 0) & (px <= f32(W)) & (py >= 0) & (py <= f32(H))
        hst = taa.sample_history(history, np.where(valid, px, f32(0.5)).astype(f32), np.where(valid, py, f32(0.5)).astype(f32), bool(int(P["useCatmullRomFilter"])))
        if stages is not None: stages.update(valid=valid, previous=(px, py), history=hst.copy())
        if int(P["enableHistoryClamping"]):
            mean, m2 = s1 / f32(9), s2 / f32(9)
            sigma = np.sqrt(fmax(m2 - mean * mean, f32(0))).astype(f32)
            rl = ref.load_unorm8(np.asarray(relax, np.uint8))[j0, i0] if relax is not None and int(P["useHistoryClampRelax"]) else np.zeros((H, W), f32)
            k = f32(P["clampingFactor"]) * (f32(1) + taa.HISTORY_CLAMP_RELAX_MUL * rl)
            lo, hi = mean - sigma * k[..., None], mean + sigma * k[..., None]
            hst = fmin(fmax(hst, lo), hi)
        if stages is not None: stages["history_clamped"] = hst.copy()
        alpha = f32(P["newFrameWeight"]) * conf if int(P["confidenceWeighted"]) else np.full((H, W), f32(P["newFrameWeight"]), f32)
        if int(P["luminanceWeighted"]):
            wc, wh = f32(1) / (f32(1) + lum_c), f32(1) / (f32(1) + luminance(hst))
            a, b = alpha * wc, (f32(1) - alpha) * wh
            beta = a / (a + b)
        else:
            beta = alpha
        r = hst + (cur - hst) * beta[..., None]
    out[..., :3] = np.where(valid[..., None], r, cur)
    return out


def bilinear(img, display):
    """the bilinear enlargement of [h, w, c] to display = (W, H): sampled at u - 0.5 with clamped coordinates, in float64 (a yardstick of the tests, not the product's)"""
    img = np.asarray(img, np.float64); h, w = img.shape[:2]; W, H = display
    u, v = (np.arange(W) + 0.5) * w / W - 0.5, (np.arange(H) + 0.5) * h / H - 0.5
    x0, y0 = np.floor(u).astype(int), np.floor(v).astype(int); tx, ty = (u - x0)[None, :, None], (v - y0)[:, None, None]
    g = lambda ys, xs: img[np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]]
    return (g(y0, x0) * (1 - tx) + g(y0, x0 + 1) * tx) * (1 - ty) + (g(y0 + 1, x0) * (1 - tx) + g(y0 + 1, x0 + 1) * tx) * ty

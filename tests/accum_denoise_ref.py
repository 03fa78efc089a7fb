"""An independent numpy restatement of the reference-mode denoiser (include/mi355pt.h pt_accum_denoise, rtxpt_amd/csrc/pt_accum_denoise.h, docs/WIDENING.md N13): a
dual-buffer non-local-means filter over the mean of a pixel's samples (A) and the mean of its even-indexed ones (H). Every step is one binary32 operation in the stated order
(numpy float32 arrays and constants); all coordinates are clamped to the frame (an edge pixel repeats). It vectorises over the picture and loops over the search offsets.
The device is held to it bit for bit (tests/test_gpu_accum_denoise.py); tests/test_accum_denoise_reference.py holds it to answers worked by hand.

Parameters are anything indexable by the names of PtAccumDenoiseParams (a dict from params(), or a record of rtxpt_amd.ACCUM_DENOISE_PARAMS_DTYPE)."""
import numpy as np

f32 = np.float32

# starting values that nobody has measured against pictures
DEFAULTS = dict(searchRadius=5, patchRadius=2, k=0.45, alpha=1.0, epsilon=1e-10, maxRadiance=65504.0)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS); assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def params_ok(P):
    """what the library accepts: every comparison is false for a NaN"""
    r, f = int(P["searchRadius"]), int(P["patchRadius"])
    k, alpha, eps, mr = f32(P["k"]), f32(P["alpha"]), f32(P["epsilon"]), f32(P["maxRadiance"])
    return bool(1 <= r <= 8 and 0 <= f <= 3 and f32(0.05) <= k <= f32(4) and f32(0) <= alpha <= f32(4) and f32(1e-20) <= eps <= f32(1) and f32(0) < mr <= f32(1e15))


def _shift(a, ox, oy):
    """a(x + o) with clamped coordinates"""
    h, w = a.shape[:2]
    return a[np.clip(np.arange(h) + oy, 0, h - 1)][:, np.clip(np.arange(w) + ox, 0, w - 1)]


def prepare(A, H, max_radiance):
    """-> (H' [h, w, 3], O' [h, w, 3], V [h, w, 3], valid [h, w] bool)"""
    A = np.asarray(A, f32); H = np.asarray(H, f32); mr = f32(max_radiance)
    with np.errstate(all="ignore"):
        a, hh = A[..., :3], H[..., :3]
        O = (a + a) - hh
        valid = np.all(np.abs(a) <= mr, -1) & np.all(np.abs(hh) <= mr, -1) & np.all(np.abs(O) <= mr, -1)      # (false for a NaN)
    Hs = np.where(valid[..., None], hh, f32(0)).astype(f32)
    Os = np.where(valid[..., None], O, f32(0)).astype(f32)
    d = Hs - Os
    s = (d * d) * f32(0.5)
    rows = (_shift(s, -1, 0) + s) + _shift(s, 1, 0)
    V = ((_shift(rows, 0, -1) + rows) + _shift(rows, 0, 1)) / f32(9.0)
    return Hs, Os, V.astype(f32), valid


def distance(U, V, ox, oy, P):
    """e [h, w]: buffer U's distance of every pixel x to x + o, the three channels summed (e_r + e_g) + e_b"""
    alpha, eps = f32(P["alpha"]), f32(P["epsilon"]); kk = f32(f32(P["k"]) * f32(P["k"]))
    Un, Vn = _shift(U, ox, oy), _shift(V, ox, oy)
    d = U - Un
    with np.errstate(over="ignore"):
        e = ((d * d) - alpha * (V + np.where(V < Vn, V, Vn))) / (eps + kk * (V + Vn))
        return ((e[..., 0] + e[..., 1]) + e[..., 2]).astype(f32)


def patch_sum(e, f):
    """S [h, w]: rows left to right, then columns top to bottom, coordinates clamped"""
    with np.errstate(over="ignore", invalid="ignore"):
        row = _shift(e, -f, 0)
        for i in range(-f + 1, f + 1): row = row + _shift(e, i, 0)
        S = _shift(row, 0, -f)
        for j in range(-f + 1, f + 1): S = S + _shift(row, 0, j)
    return S.astype(f32)


def weight(S, f):
    """w = max(1 - max(D2, 0) x 0.25, 0)^4 with D2 = S / (float)(3 (2f + 1)^2)"""
    with np.errstate(over="ignore"):
        D2 = S / f32(3 * (2 * f + 1) * (2 * f + 1))
        t = f32(1) - np.where(D2 > f32(0), D2, f32(0)) * f32(0.25)
    t = np.where(t > f32(0), t, f32(0)).astype(f32)
    t2 = t * t
    return t2 * t2


def offset_weights(Hs, Os, V, valid, ox, oy, P):
    """(w from H', w from O') [h, w] for one search offset: 0 where x + o is outside the frame or invalid"""
    h, w = valid.shape
    f = int(P["patchRadius"])
    ys, xs = np.mgrid[0:h, 0:w]
    inside = (xs + ox >= 0) & (xs + ox < w) & (ys + oy >= 0) & (ys + oy < h)
    take = inside & _shift(valid, ox, oy)
    wH = np.where(take, weight(patch_sum(distance(Hs, V, ox, oy, P), f), f), f32(0)).astype(f32)
    wO = np.where(take, weight(patch_sum(distance(Os, V, ox, oy, P), f), f), f32(0)).astype(f32)
    return wH, wO


def run(A, H, P):
    """-> dict(denoised [h, w, 4], odd O' [h, w, 3], variance V [h, w, 3], valid [h, w] uint8, FO, FH [h, w, 3], sumW_H, sumW_O [h, w])"""
    assert params_ok(P), P
    A = np.ascontiguousarray(A, f32); H = np.ascontiguousarray(H, f32)
    assert A.shape == H.shape and A.ndim == 3 and A.shape[2] == 4
    r = int(P["searchRadius"])
    Hs, Os, V, valid = prepare(A, H, P["maxRadiance"])
    h, w = valid.shape
    sumWH = np.zeros((h, w), f32); sumWO = np.zeros((h, w), f32); sumCH = np.zeros((h, w, 3), f32); sumCO = np.zeros((h, w, 3), f32)
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            wH, wO = offset_weights(Hs, Os, V, valid, ox, oy, P)
            sumWH = sumWH + wH; sumCH = sumCH + wH[..., None] * _shift(Os, ox, oy)      # weights from H' average O'
            sumWO = sumWO + wO; sumCO = sumCO + wO[..., None] * _shift(Hs, ox, oy)      # weights from O' average H'
    with np.errstate(invalid="ignore", divide="ignore"):
        FO = sumCH / sumWH[..., None]; FH = sumCO / sumWO[..., None]
        D = (FO + FH) * f32(0.5)
    out = A.copy()
    out.view(np.uint32)[..., :3] = np.where(valid[..., None], D.astype(f32).view(np.uint32), A.view(np.uint32)[..., :3])      # an invalid pixel keeps A's bytes
    return dict(denoised=out, odd=Os, variance=V, valid=valid.astype(np.uint8), FO=FO, FH=FH, sumW_H=sumWH, sumW_O=sumWO)


def denoise(A, H, P):
    return run(A, H, P)["denoised"]

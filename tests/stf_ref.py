"""A float32 numpy restatement of the stochastic texture filter (rtxpt_amd/csrc/pt_stf.h): which texel a lookup picks, with the same operations in the same order, and — in
float64 — the candidate texels of a lookup with their analytic probabilities.

The definition (pt_stf.h states it; lambda = 0.5 * baseLOD + lambdaNoDims capped at mipLevels - 5, as sampleTexture forms it; u = four numbers in [0, 1)):
  level   l = clamp(lambda, 0, levels - 1), l0 = floor(l), m0 = l0, m1 = min(m0 + 1, levels - 1), f = l - l0
          LINEAR, CUBIC: m = m1 if u.z < f else m0;      POINT: m = m0 if f < 0.5 else m1
  texel   per axis at level m (side = max(1, dim >> m)):
          POINT   x = floor(coord * side)
          LINEAR  fx = coord * side - 0.5, flx = floor(fx), ax = fx - flx, x = flx + (1 if u.x < ax else 0)
          CUBIC   w0 .. w3 = the cubic B-spline weights at ax (bspline_weights32), c0 = w0, c1 = c0 + w1, c2 = c1 + w2, x = flx - 1 + (u.x >= c0) + (u.x >= c1) + (u.x >= c2)
  wrap    the remainder of the final integer-valued coordinate by the side. The device forms it in float32 by two routes that are exact for |x| <= 2^30 (pt_scene.h
          wrap_texel_npot and the power-of-two scaling; the deterministic samplers' far-range tests hold them to that), so it is an exact integer modulo here.

Probabilities are those of a continuous uniform u: P(u < a) = a. The device's u is k / 2^24, so P(u < a) = ceil(a * 2^24) / 2^24 there: off by less than 2^-24.
"""
import zlib
import numpy as np

F32 = np.float32
POINT, LINEAR, CUBIC, GAUSSIAN = 0, 1, 2, 3
ONE_BELOW = np.nextafter(F32(1.0), F32(0.0))      # the largest float below 1: the largest u


def lambda32(word, lam_no_dims):
    """sampleTexture's two lines in float32."""
    word = np.asarray(word, np.uint32)
    base_lod, levels = (word >> 24).astype(np.float32), ((word >> 16) & 0xFF).astype(np.float32)
    lam = (F32(0.5) * base_lod + np.asarray(lam_no_dims, np.float32)).astype(np.float32)
    return np.minimum(lam, np.maximum(levels - F32(5.0), F32(0.0))).astype(np.float32)


def levels32(lam, levels):
    """(m0, m1, f): sample_trilinear's level arithmetic in float32; `levels` = the texture's level count."""
    last = (np.asarray(levels, np.int64) - 1)
    l = np.minimum(np.maximum(np.asarray(lam, np.float32), F32(0.0)), last.astype(np.float32)).astype(np.float32)
    l0 = np.floor(l).astype(np.float32)
    m0 = l0.astype(np.int64); m1 = np.minimum(m0 + 1, last)
    return m0, m1, (l - l0).astype(np.float32)


def bspline_weights32(t):
    """stf_bspline_weights: [n, 4] float32, every operation rounded to float32 in pt_stf.h's order."""
    t = np.asarray(t, np.float32); sixth = F32(1.0) / F32(6.0); s = (F32(1.0) - t).astype(np.float32)
    w0 = (((s * s).astype(np.float32) * s).astype(np.float32) * sixth).astype(np.float32)
    w1 = ((((((F32(3.0) * t).astype(np.float32) - F32(6.0)).astype(np.float32) * t).astype(np.float32) * t).astype(np.float32) + F32(4.0)).astype(np.float32) * sixth).astype(np.float32)
    a = ((F32(-3.0) * t).astype(np.float32) + F32(3.0)).astype(np.float32)
    a = ((a * t).astype(np.float32) + F32(3.0)).astype(np.float32)
    w2 = ((((a * t).astype(np.float32)) + F32(1.0)).astype(np.float32) * sixth).astype(np.float32)
    w3 = (((t * t).astype(np.float32) * t).astype(np.float32) * sixth).astype(np.float32)
    return np.stack([w0, w1, w2, w3], -1)


def bspline_weights64(t):
    """The cubic B-spline's four weights at fraction t (the float32 fraction, promoted) in float64: the reference of the CUBIC filter's expectation."""
    t = np.asarray(t, np.float64); s = 1.0 - t
    return np.stack([s ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0, (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0, t ** 3 / 6.0], -1)


def thresholds32(w):
    """c0, c1, c2 of the CUBIC tap choice: [n, 3] float32."""
    c0 = w[..., 0]; c1 = (c0 + w[..., 1]).astype(np.float32); c2 = (c1 + w[..., 2]).astype(np.float32)
    return np.stack([c0, c1, c2], -1)


def frac32(coord, side):
    """(flx as float32, ax as float32) of one axis: the coordinate step of LINEAR and CUBIC."""
    fx = ((np.asarray(coord, np.float32) * np.asarray(side, np.float32)).astype(np.float32) - F32(0.5)).astype(np.float32)
    fl = np.floor(fx).astype(np.float32)
    return fl, (fx - fl).astype(np.float32)


def _axis(filt, coord, side, u):
    """The integer-valued coordinate of one axis before the wrap, as float32 (the device adds the tap offset in float32: at 2^30 it is absorbed)."""
    side = np.asarray(side, np.float32)
    if filt == POINT: return np.floor((np.asarray(coord, np.float32) * side).astype(np.float32)).astype(np.float32)
    fl, ax = frac32(coord, side)
    if filt == LINEAR: return (fl + np.where(u < ax, F32(1.0), F32(0.0)).astype(np.float32)).astype(np.float32)
    c = thresholds32(bspline_weights32(ax))
    k = ((u >= c[:, 0]).astype(np.float32) + (u >= c[:, 1]).astype(np.float32)).astype(np.float32) + (u >= c[:, 2]).astype(np.float32)
    return ((fl - F32(1.0)).astype(np.float32) + k.astype(np.float32)).astype(np.float32)


def pick(filt, w, h, levels, word, lam_no_dims, u, v, rnd):
    """(mip, x, y) int64 [n] of the lookups: textures of w x h texels with `levels` levels (arrays or scalars), packed texture words, lambdaNoDims, coordinates, rnd [n, 4]."""
    u, v = np.atleast_1d(np.asarray(u, np.float32)), np.atleast_1d(np.asarray(v, np.float32)); n = len(u)
    rnd = np.broadcast_to(np.asarray(rnd, np.float32), (n, 4))
    w, h, levels = (np.broadcast_to(np.asarray(a, np.int64), (n,)) for a in (w, h, levels))
    m0, m1, f = levels32(lambda32(np.broadcast_to(np.asarray(word, np.uint32), (n,)), np.broadcast_to(np.asarray(lam_no_dims, np.float32), (n,))), levels)
    mip = np.where(f < F32(0.5), m0, m1) if filt == POINT else np.where(rnd[:, 2] < f, m1, m0)
    mw, mh = np.maximum(1, w >> mip), np.maximum(1, h >> mip)
    x = _axis(filt, u, mw.astype(np.float32), rnd[:, 0]).astype(np.int64) % mw
    y = _axis(filt, v, mh.astype(np.float32), rnd[:, 1]).astype(np.int64) % mh
    return mip, x, y


def candidates(filt, w, h, levels, word, lam_no_dims, u, v):
    """Every texel a lookup can pick, with its probability over uniform u: (mip [n, k], x [n, k], y [n, k], p [n, k] float64), k = 1 (POINT), 8 (LINEAR), 32 (CUBIC).
    Candidates of probability 0 (f == 0, a clamped second level, a zero fraction) are listed with p = 0."""
    u, v = np.atleast_1d(np.asarray(u, np.float32)), np.atleast_1d(np.asarray(v, np.float32)); n = len(u)
    w, h, levels = (np.broadcast_to(np.asarray(a, np.int64), (n,)) for a in (w, h, levels))
    m0, m1, f = levels32(lambda32(np.broadcast_to(np.asarray(word, np.uint32), (n,)), np.broadcast_to(np.asarray(lam_no_dims, np.float32), (n,))), levels)
    if filt == POINT:
        mip, x, y = pick(POINT, w, h, levels, word, lam_no_dims, u, v, np.zeros((n, 4), np.float32))
        return mip[:, None], x[:, None], y[:, None], np.ones((n, 1))
    M, X, Y, P = [], [], [], []
    f64 = f.astype(np.float64)
    for mip, pm in ((m0, 1.0 - f64), (m1, f64)):
        mw, mh = np.maximum(1, w >> mip), np.maximum(1, h >> mip)
        (flx, ax), (fly, ay) = frac32(u, mw.astype(np.float32)), frac32(v, mh.astype(np.float32))
        if filt == LINEAR:
            offs = (0, 1); px = np.stack([1.0 - ax.astype(np.float64), ax.astype(np.float64)], -1); py = np.stack([1.0 - ay.astype(np.float64), ay.astype(np.float64)], -1)
        else:
            offs = (-1, 0, 1, 2)
            def probs(a):
                c = np.minimum(thresholds32(bspline_weights32(a)).astype(np.float64), 1.0)      # (a threshold the sums round above 1 is never reached: u < 1)
                return np.stack([c[:, 0], c[:, 1] - c[:, 0], c[:, 2] - c[:, 1], 1.0 - c[:, 2]], -1)
            px, py = probs(ax), probs(ay)
        for j, oy in enumerate(offs):
            for i, ox in enumerate(offs):
                # (the device forms the tap's coordinate in float32 — flx + 0 / 1, (flx - 1) + k — and so does this: beyond 2^24 texels neighbouring coordinates collapse)
                tap = (lambda fl, o: (fl + F32(o)).astype(np.float32)) if filt == LINEAR else (lambda fl, o: ((fl - F32(1.0)).astype(np.float32) + F32(o + 1)).astype(np.float32))
                M.append(mip); X.append(tap(flx, ox).astype(np.int64) % mw); Y.append(tap(fly, oy).astype(np.int64) % mh)
                P.append(pm * px[:, i] * py[:, j])
    return np.stack(M, -1), np.stack(X, -1), np.stack(Y, -1), np.stack(P, -1)


# ---- probe rows (include/mi355pt_testhooks.h kind 12): uint32 [n, 12] = (mode, packed texture word, u, v, lambdaNoDims, filter, four mode words, two unused)
def _rng(*key): return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rows12(word, u, v, lam, filt, rnd):
    u = np.atleast_1d(np.asarray(u, np.float32)); n = len(u)
    r = np.zeros((n, 12), np.uint32); r[:, 1] = word; r[:, 5] = filt
    r[:, 2] = u.view(np.uint32); r[:, 3] = np.broadcast_to(np.asarray(v, np.float32), (n,)).copy().view(np.uint32)
    r[:, 4] = np.broadcast_to(np.asarray(lam, np.float32), (n,)).copy().view(np.uint32)
    r[:, 6:10] = np.broadcast_to(np.asarray(rnd, np.float32), (n, 4)).copy().view(np.uint32)
    return r


def random_u(r, n):
    """n x 4 numbers of the device's kind: k / 2^24."""
    return (r.integers(0, 1 << 24, (n, 4)).astype(np.float32) / F32(16777216.0)).astype(np.float32)


def lookup_rows(t, material_rows):
    """(word, u, v, lambdaNoDims) float / uint arrays of the lookups every filter is tested at on texture `t` (tests/texture_cases.py Tex): texture_cases.material_rows (every
    integer level, between levels, below 0, past the last, 1e9; random and special uv) and rows of this file's own — lambda negative, integer, fractional and above the cap,
    each with uv on texel centres, on texel edges, negative, above 1, and in the far range up to 2^30 texels."""
    r = _rng("stf", t.w, t.h)
    m = material_rows(t); u = [m[:, 2].copy().view(np.float32)]; v = [m[:, 3].copy().view(np.float32)]; lam = [m[:, 4].copy().view(np.float32)]
    base = 0.5 * (t.word >> 24); cap = max(t.levels - 5.0, 0.0)
    for target in (-1.5, 0.0, 1.0, 0.37, 1.5, min(cap, 2.0) + 0.75, cap + 3.0):
        for mip in sorted({0, min(1, t.levels - 1), min(int(max(target, 0)), t.levels - 1)}):
            mw, mh = max(1, t.w >> mip), max(1, t.h >> mip)
            iu, iv = np.arange(-1, mw + 2), np.arange(-1, mh + 2)
            cu = np.concatenate([(iu + 0.5) / mw, iu / mw, -(iu + 0.5) / mw, 1.0 + iu / mw]).astype(np.float32)
            cv = np.concatenate([(iv + 0.5) / mh, iv / mh, -(iv + 0.5) / mh, 1.0 + iv / mh]).astype(np.float32)
            k = min(len(cu), len(cv), 48); su = r.permutation(len(cu))[:k]; sv = r.permutation(len(cv))[:k]
            u += [cu[su], (r.random(k) * 6 - 3).astype(np.float32)]; v += [(r.random(k) * 6 - 3).astype(np.float32), cv[sv]]
            lam += [np.full(2 * k, target - base, np.float32)]
        n = 24                                                        # the far range: 2^25 .. 2^30 texels at level 0, either sign, on either axis or both
        big = lambda dim: (np.where(r.random(n) < 0.5, -1.0, 1.0) * 2.0 ** (25 + 5 * r.random(n)) / dim).astype(np.float32)
        near = lambda: (r.random(n) * 6 - 3).astype(np.float32)
        u += [big(t.w), near(), big(t.w)]; v += [near(), big(t.h), big(t.h)]; lam += [np.full(3 * n, target - base, np.float32)]
    u, v, lam = np.concatenate(u), np.concatenate(v), np.concatenate(lam)
    assert (np.abs(u.astype(np.float64)) * t.w <= 2.0 ** 30).all() and (np.abs(v.astype(np.float64)) * t.h <= 2.0 ** 30).all()
    return np.full(len(u), t.word, np.uint32), u, v, lam


def threshold_u(filt, w, h, levels, word, lam, u, v, r):
    """Per lookup, numbers u that sit on the decision thresholds: 0, the largest float below 1, and — per component — the float just below and exactly at each threshold
    (LINEAR: ax, ay, f; CUBIC: c0 .. c2 of either axis at the level the other components select, f). One threshold per row, the other components random: [n, 4]."""
    n = len(u); rnd = random_u(r, n)
    m0, m1, f = levels32(lambda32(word, lam), np.full(n, levels))
    which = r.integers(0, 6, n)
    rnd[which == 0] = F32(0.0); rnd[which == 1] = ONE_BELOW
    at = r.random(n) < 0.5                                            # exactly at the threshold, or just below it
    lev = which == 2
    thr = f.copy()
    rnd[lev, 2] = np.where(at[lev], thr[lev], np.nextafter(thr[lev], F32(-1.0)))
    mip = np.where(rnd[:, 2] < f, m1, m0) if filt != POINT else np.where(f < F32(0.5), m0, m1)
    mw, mh = np.maximum(1, w >> mip).astype(np.float32), np.maximum(1, h >> mip).astype(np.float32)
    for comp, (coord, side) in enumerate(((u, mw), (v, mh))):
        _, a = frac32(coord, side)
        if filt == CUBIC:
            c = thresholds32(bspline_weights32(a)); a = c[np.arange(n), r.integers(0, 3, n)]
        sel = (which == 3 + comp) | (which == 5)
        rnd[sel, comp] = np.where(at[sel], a[sel], np.nextafter(a[sel], F32(-1.0)))
    return np.clip(rnd, F32(0.0), ONE_BELOW).astype(np.float32)


def probe_rows(t, filt, material_rows):
    """Mode-0 rows of probe 12 for one texture and filter: every lookup of lookup_rows twice — with random u, and with u on the thresholds."""
    word, u, v, lam = lookup_rows(t, material_rows); r = _rng("stf-u", t.w, t.h, filt)
    a = rows12(word, u, v, lam, filt, random_u(r, len(u)))
    b = rows12(word, u, v, lam, filt, threshold_u(filt, t.w, t.h, t.levels, word, lam, u, v, r))
    return np.concatenate([a, b])


def pick_rows(t, rows):
    """pick() of probe rows of one texture."""
    f32 = lambda c: rows[:, c].copy().view(np.float32)
    return pick(int(rows[0, 5]), t.w, t.h, t.levels, rows[:, 1], f32(4), f32(2), f32(3), rows[:, 6:10].copy().view(np.float32))


def build_mips32(level0):
    """The float32 levels the library stores (pt_api.hip build_mips: (a + b) + (c + d), then * 0.25, per channel in float32; a source index past an odd side's last texel is
    clamped to it): a list of [mh, mw, 4] float32."""
    mips = [np.asarray(level0, np.float32)]
    while max(mips[-1].shape[:2]) > 1:
        p = mips[-1]; ph, pw = p.shape[:2]; mh, mw = max(1, ph >> 1), max(1, pw >> 1)
        x0, x1 = np.minimum(2 * np.arange(mw), pw - 1), np.minimum(2 * np.arange(mw) + 1, pw - 1)
        y0, y1 = np.minimum(2 * np.arange(mh), ph - 1), np.minimum(2 * np.arange(mh) + 1, ph - 1)
        s = ((p[y0][:, x0] + p[y0][:, x1]).astype(np.float32) + (p[y1][:, x0] + p[y1][:, x1]).astype(np.float32)).astype(np.float32)
        mips.append((s * F32(0.25)).astype(np.float32))
    return mips

"""The reference-mode denoiser's numpy restatement (tests/accum_denoise_ref.py; include/mi355pt.h pt_accum_denoise, docs/WIDENING.md N13) held to answers worked by hand and to
a second, scalar restatement written pixel by pixel in this file. No device: tests/test_gpu_accum_denoise.py holds the kernels to the restatement bit for bit.
The hand-worked frames use A = H (so O = H, s = 0, V = 0) with epsilon = 1: a channel's e is then (U(x) - U(x+o))^2 exactly, and grey pixels give e = 3 d^2."""
import numpy as np
import pytest

from tests import accum_denoise_ref as ad

f32 = np.float32


def _bits(a): return np.ascontiguousarray(a, f32).view(np.uint32)


def _grey(g):
    """[h, w] -> RGBA with alpha 1"""
    g = np.asarray(g, f32)
    return np.ascontiguousarray(np.concatenate([np.repeat(g[..., None], 3, -1), np.ones(g.shape + (1,), f32)], -1))


def _noisy(h, w, seed, spread=0.25):
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.1, 2.0, (h, w, 1)).astype(f32) * np.array([1.0, 0.8, 0.6], f32)
    H = np.concatenate([base + rng.normal(0, spread, (h, w, 3)).astype(f32), np.ones((h, w, 1), f32)], -1).astype(f32)
    O = np.concatenate([base + rng.normal(0, spread, (h, w, 3)).astype(f32), np.ones((h, w, 1), f32)], -1).astype(f32)
    A = ((H + O) * f32(0.5)).astype(f32); A[..., 3] = rng.uniform(0, 1, (h, w)).astype(f32)
    return A, H


# ---- a second restatement: one pixel, scalar by scalar, straight from the header's text
def _clamp(v, n): return min(max(v, 0), n - 1)


def _scalar_pixel(A, H, P, x, y):
    h, w = A.shape[:2]
    r, f = int(P["searchRadius"]), int(P["patchRadius"])
    alpha, eps, mr = f32(P["alpha"]), f32(P["epsilon"]), f32(P["maxRadiance"]); kk = f32(f32(P["k"]) * f32(P["k"]))
    cache = {}

    def stage(px, py):
        key = (px, py)
        if key not in cache:
            a, hh = A[py, px, :3], H[py, px, :3]
            with np.errstate(all="ignore"):
                O = [f32(f32(a[c] + a[c]) - hh[c]) for c in range(3)]
                ok = all(abs(v) <= mr for v in list(a) + list(hh) + O)
            cache[key] = ([f32(hh[c]) if ok else f32(0) for c in range(3)], [O[c] if ok else f32(0) for c in range(3)], ok)
        return cache[key]

    def s(px, py, c):
        Hs, Os, _ = stage(_clamp(px, w), _clamp(py, h))
        d = f32(Hs[c] - Os[c])
        return f32(f32(d * d) * f32(0.5))

    vcache = {}

    def V(px, py, c):
        px, py = _clamp(px, w), _clamp(py, h)
        key = (px, py, c)
        if key not in vcache:
            rows = [f32(f32(s(px - 1, py + j, c) + s(px, py + j, c)) + s(px + 1, py + j, c)) for j in (-1, 0, 1)]
            vcache[key] = f32(f32(f32(rows[0] + rows[1]) + rows[2]) / f32(9.0))
        return vcache[key]

    def e(px, py, ox, oy, which):
        px, py = _clamp(px, w), _clamp(py, h)                    # a clamped position is that pixel ...
        nx, ny = _clamp(px + ox, w), _clamp(py + oy, h)          # ... paired with its own clamped neighbour
        ec = []
        for c in range(3):
            u, un, v, vn = stage(px, py)[which][c], stage(nx, ny)[which][c], V(px, py, c), V(nx, ny, c)
            d = f32(u - un)
            with np.errstate(over="ignore"):
                ec.append(f32(f32(f32(d * d) - f32(alpha * f32(v + min(v, vn)))) / f32(eps + f32(kk * f32(v + vn)))))
        return f32(f32(ec[0] + ec[1]) + ec[2])

    sumW = [f32(0), f32(0)]; sumC = [[f32(0)] * 3, [f32(0)] * 3]
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            nx, ny = x + ox, y + oy
            take = 0 <= nx < w and 0 <= ny < h and stage(nx, ny)[2]
            for which in (0, 1):
                wgt = f32(0)
                if take:
                    rows = []
                    for j in range(-f, f + 1):
                        row = e(x - f, y + j, ox, oy, which)
                        for i in range(-f + 1, f + 1): row = f32(row + e(x + i, y + j, ox, oy, which))
                        rows.append(row)
                    S = rows[0]
                    for row in rows[1:]: S = f32(S + row)
                    D2 = f32(S / f32(3 * (2 * f + 1) ** 2))
                    t = max(f32(f32(1) - f32(max(D2, f32(0)) * f32(0.25))), f32(0)); t2 = f32(t * t); wgt = f32(t2 * t2)
                other = stage(nx, ny)[1 - which] if take else [f32(0)] * 3
                sumW[which] = f32(sumW[which] + wgt)
                sumC[which] = [f32(sumC[which][c] + f32(wgt * other[c])) for c in range(3)]
    if not stage(x, y)[2]: return A[y, x].copy()
    FO = [f32(sumC[0][c] / sumW[0]) for c in range(3)]; FH = [f32(sumC[1][c] / sumW[1]) for c in range(3)]
    return np.array([f32(f32(FO[c] + FH[c]) * f32(0.5)) for c in range(3)] + [A[y, x, 3]], f32)


# ---- 1. a constant picture comes back bit for bit
def test_constant_picture_is_unchanged():
    A = _grey(np.full((9, 11), 0.5)); A[..., 3] = f32(0.25)
    R = ad.run(A, A.copy(), ad.params())
    assert np.array_equal(_bits(R["denoised"]), _bits(A)) and R["valid"].all() and not R["variance"].any()
    # the weight sum counts the offsets that stay inside the frame: 6 x 6 in a corner, 11 columns x the frame's 9 rows in the middle
    assert R["sumW_H"][0, 0] == 36 and R["sumW_H"][4, 5] == 99 and np.array_equal(R["sumW_H"], R["sumW_O"])


# ---- 2. a zero-variance step keeps its edge and its flat sides
def test_zero_variance_step_is_unchanged():
    g = np.full((9, 12), 0.5, f32); g[:, 6:] = 2.0
    A = _grey(g)
    out = ad.denoise(A, A.copy(), ad.params())
    assert np.array_equal(_bits(out), _bits(A))


# ---- 3. one pixel, every number written out
def test_one_pixel_worked_by_hand():
    """3 x 3, r = 1, f = 0, A = H, epsilon = 1, alpha = 1: V = 0, e = 3 d^2, D2 = e / 3 = d^2, w = max(1 - d^2 / 4, 0)^4. The centre is 1; its nine neighbours in offset order:
        value  0     0     2     0     1(self) 1     4     1     1.5
        d^2    1     1     1     1     0       0     9     0     0.25
        e      3     3     3     3     0       0     27    0     0.75
        t      .75   .75   .75   .75   1       1     0     1     .9375
        w      .31640625 (x4)          1       1     0     1     .7724761962890625
    sumW = 4 x .31640625 + 3 + .7724761962890625 = 5.0381011962890625 and sumC = .31640625 x 2 + 3 + .7724761962890625 x 1.5 = 4.79152679443359375, both exact in binary32;
    the quotient is rounded once. Both directions agree (H = O), so D = (F + F) x 0.5 = F."""
    g = np.array([[0, 0, 2], [0, 1, 1], [4, 1, 1.5]], f32)
    A = _grey(g); P = ad.params(searchRadius=1, patchRadius=0, epsilon=1.0, alpha=1.0, k=0.5)
    Hs, Os, V, valid = ad.prepare(A, A.copy(), P["maxRadiance"])
    assert valid.all() and not V.any() and np.array_equal(Hs, Os)
    want_e = [3, 3, 3, 3, 0, 0, 27, 0, 0.75]
    want_w = [0.31640625] * 4 + [1, 1, 0, 1, 0.7724761962890625]
    offsets = [(ox, oy) for oy in (-1, 0, 1) for ox in (-1, 0, 1)]
    for (ox, oy), e, w in zip(offsets, want_e, want_w):
        E = ad.distance(Hs, V, ox, oy, P)
        assert E[1, 1] == f32(e), (ox, oy)
        wH, wO = ad.offset_weights(Hs, Os, V, valid, ox, oy, P)
        assert wH[1, 1] == f32(w) == wO[1, 1], (ox, oy)
    R = ad.run(A, A.copy(), P)
    assert R["sumW_H"][1, 1] == f32(5.0381011962890625) == R["sumW_O"][1, 1]
    F = f32(4.79152679443359375) / f32(5.0381011962890625)
    assert F == f32(0.9510580897331238)
    assert np.array_equal(_bits(R["denoised"][1, 1]), _bits(np.array([F, F, F, 1], f32)))
    assert np.array_equal(_bits(R["FO"][1, 1]), _bits(R["FH"][1, 1]))


# ---- 4. the two clamps at the border
def test_clamped_borders_5x3():
    """5 x 3, columns 0 1 1 1 1, A = H, epsilon = 1, r = 1, f = 1. Pixel (0, 1):
    - offset (-1, 0) leaves the frame: w = 0, although the clamped neighbour is the pixel itself and its distance would be 0. Its weight sum therefore has six terms, not nine.
    - offset (+1, 0): the patch's taps at x = -1 are clamped to x = 0, and e there is pixel 0's own e — pixel 0 against pixel 1, 3 x 1^2 = 3 — not position -1 against position 0
      (both pixel 0: 0). Row sums 3 + 3 + 0 = 6 in each of the three rows, S = 18, D2 = 18 / 27, w = (1 - D2 x 0.25)^4."""
    g = np.tile(np.array([0, 1, 1, 1, 1], f32), (3, 1))
    A = _grey(g); P = ad.params(searchRadius=1, patchRadius=1, epsilon=1.0, alpha=1.0, k=0.5)
    Hs, Os, V, valid = ad.prepare(A, A.copy(), P["maxRadiance"])
    wH, _ = ad.offset_weights(Hs, Os, V, valid, -1, 0, P)
    assert wH[1, 0] == 0 and wH[1, 1] > 0
    assert ad.patch_sum(ad.distance(Hs, V, 1, 0, P), 1)[1, 0] == f32(18)
    wH, _ = ad.offset_weights(Hs, Os, V, valid, 1, 0, P)
    t = f32(1) - f32(f32(18) / f32(27)) * f32(0.25); t2 = f32(t * t); want = f32(t2 * t2)
    t = f32(1) - f32(f32(9) / f32(27)) * f32(0.25); t2 = f32(t * t); other = f32(t2 * t2)      # what pairing position -1 with position 0 would give
    assert wH[1, 0] == want and want != other
    # the pixel's own sums, through the scalar restatement as well
    R = ad.run(A, A.copy(), P)
    assert np.array_equal(_bits(R["denoised"][1, 0]), _bits(_scalar_pixel(A, A.copy(), P, 0, 1)))
    # offsets (0, -1), (0, 0), (0, 1) weigh 1 (the same column), the three at +1 weigh `want`, the three at -1 nothing
    assert R["sumW_H"][1, 0] == f32(f32(f32(f32(f32(f32(0) + f32(1)) + want) + f32(1)) + want) + f32(1)) + want


# ---- 5. the separable sum: its error and its order
def test_separable_sum_error_and_order():
    rng = np.random.default_rng(7)
    e = rng.uniform(-3.0, 40.0, (14, 17)).astype(f32)
    f = 3
    S = ad.patch_sum(e, f)
    ys, xs = np.mgrid[0:14, 0:17]
    S64 = np.zeros((14, 17)); mag = np.zeros((14, 17))
    for j in range(-f, f + 1):
        for i in range(-f, f + 1):
            t = e[np.clip(ys + j, 0, 13), np.clip(xs + i, 0, 16)].astype(np.float64)
            S64 += t; mag += np.abs(t)
    # 49 terms in 48 binary32 additions: |S - exact| <= 48 u sum|e| to first order, u = 2^-24
    assert np.all(np.abs(S.astype(np.float64) - S64) <= 48 * 2.0 ** -24 * mag)
    # columns first, rows second: the same 49 numbers, another association, other bits
    other = ad.patch_sum(e.T, f).T
    assert np.all(np.abs(other.astype(np.float64) - S64) <= 48 * 2.0 ** -24 * mag) and not np.array_equal(_bits(S), _bits(other))


# ---- 6. pixels that cannot be filtered pass through and weigh nothing
def test_invalid_pixels_pass_through_and_give_no_weight():
    A, H = _noisy(9, 12, 3)
    planted = {(0, 0): np.nan, (4, 5): np.inf, (8, 11): 3e38, (2, 7): -np.inf}
    for (y, x), v in planted.items(): A[y, x, 1] = f32(v)
    H[6, 3, 0] = f32(np.nan)                                       # invalid through H alone
    A[1, 9, :3] = f32(60000.0); H[1, 9, :3] = f32(0.0)             # A and H in range, O = 120000 is not
    bad = sorted(list(planted) + [(6, 3), (1, 9)])
    P = ad.params()
    R = ad.run(A, H, P)
    mask = np.ones((9, 12), bool)
    for y, x in bad:
        mask[y, x] = False
        assert np.array_equal(_bits(R["denoised"][y, x]), _bits(A[y, x])), (y, x)
        assert R["valid"][y, x] == 0 and not R["odd"][y, x].any()
    assert R["valid"][mask].all() and np.isfinite(R["denoised"][mask]).all() and np.isfinite(R["variance"]).all()
    assert np.all(R["sumW_H"][mask] >= 1) and np.all(R["sumW_O"][mask] >= 1)
    assert np.array_equal(_bits(R["denoised"][..., 3]), _bits(A[..., 3]))
    # no weight: whatever an invalid pixel holds, every other pixel's result is the same
    A2, H2 = A.copy(), H.copy()
    for y, x in bad: A2[y, x, :3] = f32(-np.inf); H2[y, x, :3] = f32(1e30)
    R2 = ad.run(A2, H2, P)
    assert np.array_equal(_bits(R2["denoised"])[mask], _bits(R["denoised"])[mask])
    # and the scalar restatement agrees next to one of them
    for x, y in ((1, 0), (5, 3), (10, 8)):
        assert np.array_equal(_bits(R["denoised"][y, x]), _bits(_scalar_pixel(A, H, P, x, y))), (x, y)


# ---- 7. the ends of the two radii, against the scalar restatement
@pytest.mark.parametrize("r,f", [(1, 0), (8, 3), (8, 0), (1, 3)])
def test_parameter_ends(r, f):
    A, H = _noisy(5, 6, 11 + r + f)
    P = ad.params(searchRadius=r, patchRadius=f)
    R = ad.run(A, H, P)
    assert np.isfinite(R["denoised"]).all() and np.all(R["sumW_H"] >= 1)
    for x, y in ((0, 0), (3, 2)):
        assert np.array_equal(_bits(R["denoised"][y, x]), _bits(_scalar_pixel(A, H, P, x, y))), (x, y)


def test_parameter_bounds():
    assert ad.params_ok(ad.params())
    for kw in (dict(searchRadius=0), dict(searchRadius=9), dict(patchRadius=4), dict(k=0.04), dict(k=4.5), dict(k=np.nan), dict(alpha=-0.1), dict(alpha=4.5), dict(alpha=np.nan),
               dict(epsilon=0.0), dict(epsilon=1e-21), dict(epsilon=1.5), dict(epsilon=np.nan), dict(maxRadiance=0.0), dict(maxRadiance=2e15), dict(maxRadiance=np.inf),
               dict(maxRadiance=np.nan)):
        assert not ad.params_ok(ad.params(**kw)), kw
    for kw in (dict(searchRadius=1), dict(searchRadius=8), dict(patchRadius=0), dict(patchRadius=3), dict(k=0.05), dict(k=4.0), dict(alpha=0.0), dict(alpha=4.0),
               dict(epsilon=1e-20), dict(epsilon=1.0), dict(maxRadiance=1e15)):
        assert ad.params_ok(ad.params(**kw)), kw


# ---- 8. the statistical condition: a noisy step gets closer to the truth, also at the edge
@pytest.mark.parametrize("sigma", [0.05, 0.2])
def test_noisy_step_moves_towards_the_truth(sigma):
    """40 x 48, 0.5 | 2.0; H and O independent Gaussian noise around it (default_rng(1)), A = (H + O) / 2. At the defaults the denoised picture's mean squared error to the truth
    must be below a quarter of A's, and over the four columns at the edge below A's there."""
    h, w = 40, 48
    truth = np.full((h, w, 3), 0.5, f32); truth[:, w // 2:] = 2.0
    rng = np.random.default_rng(1)
    H = (truth + rng.normal(0, sigma, truth.shape)).astype(f32); O = (truth + rng.normal(0, sigma, truth.shape)).astype(f32)
    A = ((H + O) * f32(0.5)).astype(f32)
    a4 = np.concatenate([A, np.ones((h, w, 1), f32)], -1); h4 = np.concatenate([H, np.ones((h, w, 1), f32)], -1)
    D = ad.denoise(a4, h4, ad.params())[..., :3]
    mse = lambda p, sl=slice(None): float(np.mean((p[:, sl].astype(np.float64) - truth[:, sl]) ** 2))
    edge = slice(w // 2 - 2, w // 2 + 2)
    print("sigma %g: mse denoised %.4g against %.4g (ratio %.4g); at the edge %.4g against %.4g" % (sigma, mse(D), mse(A), mse(D) / mse(A), mse(D, edge), mse(A, edge)))
    assert mse(D) < 0.25 * mse(A)
    assert mse(D, edge) < mse(A, edge)

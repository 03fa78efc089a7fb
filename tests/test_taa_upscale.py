"""The temporal upscaling resolve (pt_taa_upscale, rtxpt_amd/csrc/pt_taau.h) on the CPU: its numpy restatement (tests/taau_ref.py) held to answers that do not come from it —
taa_ref.resolve at ratio 1 (bit for bit, on the worked sequences of the resolve's tests), a flat field, weights and normalised sums worked with fractions.Fraction, the
footprint of one lit render pixel summed over the whole frame in exact rationals, history fetches two display pixels away, and a usefulness condition on two analytic scenes
against an 8 x 8 supersampled truth — then pt_upscale_tex_lod_bias and the public interface. The device is held to the restatement bit for bit in
tests/test_gpu_zzzzzz_taa_upscale.py."""
import itertools, os, re, sys
from fractions import Fraction
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import taa_ref as taa
import taau_ref as taau
import test_taa_resolve as cpu_taa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
image, flat, motion, ramp, same, bits = cpu_taa.image, cpu_taa.flat, cpu_taa.motion, cpu_taa.ramp, cpu_taa.same, cpu_taa.bits
SIZES = cpu_taa.SIZES
FLAGS = cpu_taa.FLAGS + ("confidenceWeighted",)
PLAIN = dict(cpu_taa.PLAIN, confidenceWeighted=0)
PAIRS = [((32, 24), (64, 48)), ((32, 24), (48, 36)), ((32, 24), (96, 72)), ((35, 10), (70, 20))]      # (render, display)
JITTERS = [(0.0, 0.0), (0.25, -0.375), (-0.5, 0.49999997)]
ENTRY_POINTS = ("pt_taa_upscale_default_params", "pt_taa_upscale", "pt_upscaled_size", "pt_upscaled_device_buffer", "pt_get_upscaled", "pt_bloom_upscaled",
                "pt_get_upscaled_bloomed", "pt_tonemap_upscaled", "pt_average_luminance_upscaled", "pt_upscale_tex_lod_bias")


def resolve_sequences(w, h):
    """(name, PtTaaParams keywords, [(colour, motion, calls)]): the sequences tests/test_taa_resolve.py works by hand, as frames"""
    z = motion(w, h); const = lambda v: motion(w, h, lambda x, y: v); seq = []
    dirty = image(w, h, lambda x, y: (0.25 * x, 0.5 * y, 1.0))
    dirty[1, 2, :3] = (np.nan, np.inf, -np.inf); dirty[2, 3, :3] = (-1.0, 20000.0, -0.0); dirty[h - 1, w - 1, :3] = (3e38, 1e-40, 10000.0)
    seq.append(("sanitise", {}, [(dirty, const((3, -2)), 1), (dirty, const((np.nan, 0)), 1), (dirty, z, 1)]))
    seq.append(("sanitise_max_half", dict(maxRadiance=0.5), [(dirty, z, 2)]))
    seq.append(("step", dict(newFrameWeight=0.5, **cpu_taa.PLAIN), [(flat(w, h, 0.25), z, 1), (flat(w, h, 0.75), z, 2)]))
    pattern = image(w, h, lambda x, y: float((3 * x + 5 * y) % 7)); black = flat(w, h, 0.0)
    for cm in (1, 0):
        for mv in ((3, 0), (0.5, 0), (0.75, 0), (0, -2), (-4, 3)):
            seq.append(("motion_%g_%g_cr%d" % (mv + (cm,)), dict(newFrameWeight=0.5, useCatmullRomFilter=cm, **cpu_taa.PLAIN), [(pattern, z, 1), (black, const(mv), 1)]))
    one = lambda at, v: motion(w, h, lambda x, y: v if (x, y) == at else (0, 0))
    tie = {(3, 2): (1, 0), (5, 2): (0, 1), (4, 4): (-1, 0)}
    dil = [one((4, 3), (2, 0)), motion(w, h, lambda x, y: tie.get((x, y), (0, 0))), one((1, 1), (1, 1)), one((w - 1, h - 1), (-1, -1))]
    if w > 32: dil.append(one((32, 8), (-2, 0)))
    seq.append(("dilation", dict(newFrameWeight=0.5, **cpu_taa.PLAIN), [(pattern, z, 1)] + [(black, m, 1) for m in dil]))
    for cm in (1, 0):
        for mv in ((0.5, 0.0), (0.25, -0.5), (-0.75, 0.5), (1.0, -1.0)):
            moved = image(w, h, lambda x, y: ramp(x + mv[0], y + mv[1]))
            seq.append(("ramp_%g_%g_cr%d" % (mv + (cm,)), dict(useCatmullRomFilter=cm), [(image(w, h, ramp), z, 1), (moved, const(mv), 1)]))
    for name, kw in (("ghost", {}), ("ghost_plain_weight", dict(luminanceWeighted=0)), ("ghost_kept", cpu_taa.PLAIN)):
        seq.append((name, kw, [(flat(w, h, 1.0), z, 1), (black, z, 1)]))
    thirds = image(w, h, lambda x, y: float((x + 2 * y) % 3))
    for name, kw in (("box", {}), ("box_no_relax", dict(useHistoryClampRelax=0)), ("box_factor_0", dict(clampingFactor=0.0)), ("box_factor_2", dict(clampingFactor=2.0))):
        seq.append((name, kw, [(flat(w, h, 64.0), z, 1), (thirds, z, 1)]))
    seq.append(("luminance_weight", dict(newFrameWeight=0.5, enableHistoryClamping=0), [(flat(w, h, 1.0), z, 1), (flat(w, h, 3.0), z, 1)]))
    rng = np.random.default_rng(5)
    noise = lambda: np.concatenate([rng.uniform(0.25, 4.0, (h, w, 3)).astype(f32), np.ones((h, w, 1), f32)], -1)
    wander = lambda: rng.choice(np.array([-1.5, -0.75, -0.25, 0, 0.5, 1.25], f32), (h, w, 2))
    frames = [(noise(), wander(), 1) for _ in range(4)]
    for combo in itertools.product((0, 1), repeat=4):
        seq.append(("random_%d%d%d%d" % combo, dict(zip(cpu_taa.FLAGS, combo)), frames))
    return seq


@pytest.mark.parametrize("w,h", SIZES)
def test_ratio_one_is_the_resolve_bit_for_bit(w, h):
    """W x H = w x h, jitter (0, 0), kernelRadius 1: the centre weight is exactly 1, the other eight exactly 0, the best tap's weight 1"""
    relax = np.full((h, w), 255, np.uint8); relax[::2] = 51; relax[1, 1] = 0
    i0, j0, wk = taau.footprint(w, h, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    assert np.array_equal(i0, xs) and np.array_equal(j0, ys) and np.all(wk[:, :, 1, 1] == 1) and wk.sum() == w * h
    for name, kw, frames in resolve_sequences(w, h):
        for conf in (1, 0):
            P = taau.params(confidenceWeighted=conf, **kw)
            a = b = None
            for f, (colour, mv, calls) in enumerate(frames):
                for k in range(calls):
                    a = taa.resolve(colour, mv, relax, a, taau.taa_params(P))
                    b = taau.upscale(colour, mv, relax, b, P, (w, h))
                    assert same(a, b), (name, conf, f, k)


@pytest.mark.parametrize("render,display", PAIRS)
def test_flat_field_stays_flat_with_every_flag_combination(render, display):
    """the products by 0.5 are exact, so the normalised sum is exactly 0.5 whatever the weights are"""
    (w, h), (W, H) = render, display
    c, mv = flat(w, h, 0.5), motion(w, h)
    relax = np.full((h, w), 255, np.uint8); relax[::2] = 0
    want = flat(W, H, 0.5); want[..., 3] = 1
    for combo in itertools.product((0, 1), repeat=5):
        P = taau.params(**dict(zip(FLAGS, combo)))
        for j in JITTERS:
            hist = None
            for f in range(3):
                hist = taau.upscale(c, mv, relax, hist, P, display, j)
                assert same(hist, want), (combo, j, f)


def _round(q):
    """the binary32 nearest to the rational q: one rounding (through a double it would be two; the neighbours are compared exactly)"""
    c = f32(float(q))
    return min((c, np.nextafter(c, f32(-np.inf)), np.nextafter(c, f32(np.inf))), key=lambda v: abs(Fraction(float(v)) - q))


def _hand(taps):
    """[(colour, weight)] with exact binary32 values -> float32(sum c w / sum w): one rounding"""
    num, den = sum(Fraction(float(c)) * Fraction(float(k)) for c, k in taps), sum(Fraction(float(k)) for c, k in taps)
    assert f32(float(num)) == float(num) and f32(float(den)) == float(den)      # (the sums themselves are exact in binary32)
    return _round(num / den), den


def test_weights_and_normalised_sums_by_hand_at_twice_the_size():
    w, h = 11, 9; W, H = 22, 18
    c = image(w, h, lambda x, y: (float((3 * x + 5 * y) % 7), 0.25 * x, 0.5 * y))      # dyadic colours
    near, side = f32(0.765625), f32(0.140625)                               # (1 - 0.125)^2, (1 - 0.625)^2; the diagonal neighbour: 1 - 1.125 < 0
    st = {}
    out = taau.upscale(c, None, None, None, taau.params(), (W, H), stages=st)
    i0, j0 = st["nearest"]; wk = st["weights"]

    def check(X, Y, taps, total):
        for ch in range(3):
            want, den = _hand([(c[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1), ch], k) for (x, y), k in taps])
            assert den == total and bits(out[Y, X, ch]) == bits(want), (X, Y, ch, out[Y, X, ch], want)
        got = {(int(i0[Y, X]) + dx, int(j0[Y, X]) + dy): wk[Y, X, dy + 1, dx + 1] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if wk[Y, X, dy + 1, dx + 1] != 0}
        assert got == dict(taps), (X, Y, got)

    # an even pixel (8, 6): centre (4.25, 3.25), nearest sample (4.5, 3.5); the near side is left / up
    check(8, 6, [((4, 3), near), ((3, 3), side), ((4, 2), side)], Fraction(1046875, 1000000))
    # an odd pixel (9, 7): centre (4.75, 3.75), the same nearest sample; the near side is right / down
    check(9, 7, [((4, 3), near), ((5, 3), side), ((4, 4), side)], Fraction(1046875, 1000000))
    check(9, 6, [((4, 3), near), ((5, 3), side), ((4, 2), side)], Fraction(1046875, 1000000))
    # the corners: the near-side taps lie outside the frame — their texels are the clamped ones, their distances (and weights) the unclamped ones
    check(0, 0, [((0, 0), near), ((-1, 0), side), ((0, -1), side)], Fraction(1046875, 1000000))
    check(W - 1, H - 1, [((w - 1, h - 1), near), ((w, h - 1), side), ((w - 1, h), side)], Fraction(1046875, 1000000))
    check(W - 1, 0, [((w - 1, 0), near), ((w, 0), side), ((w - 1, -1), side)], Fraction(1046875, 1000000))
    assert same(out[0, 0, :3], c[0, 0, :3]) and np.all(out[..., 3] == 1)
    # jitter (0.25, -0.25): render pixel i samples at i + 0.25, row j at j + 0.75. Display pixel (8, 6), centre (4.25, 3.25): column 4 is dead on, rows 3 and 2 are both 0.5 away
    out = taau.upscale(c, None, None, None, taau.params(), (W, H), (0.25, -0.25), stages=st)
    i0, j0 = st["nearest"]; wk = st["weights"]
    assert (i0[6, 8], j0[6, 8]) == (4, 3)
    check(8, 6, [((4, 2), f32(0.5625)), ((4, 3), f32(0.5625))], Fraction(1125, 1000))
    assert same(out[6, 8, :3], (c[2, 4, :3] + c[3, 4, :3]) * f32(0.5))
    # kernelRadius 2 at jitter 0: the weights of pixel (8, 6) are (1 - d^2 / 4)^2 for all nine taps
    taau.upscale(c, None, None, None, taau.params(kernelRadius=2.0), (W, H), stages=st)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            d2 = Fraction(4 + dx) + Fraction(1, 2) - Fraction(17, 4); e2 = Fraction(3 + dy) + Fraction(1, 2) - Fraction(13, 4)
            a = max(1 - (d2 * d2 + e2 * e2) / 4, 0)
            assert st["weights"][6, 8, dy + 1, dx + 1] == f32(float(a * a)), (dx, dy)


def _exact_footprint(w, h, W, H, lit, jitter):
    """the lit render pixel's share of every display pixel in exact rationals, summed over ALL render pixels (not the nine taps): sample i at i + 0.5 - j, weight
    max(1 - d^2, 0)^2 of the distance to the display centre (X + 0.5) w / W"""
    jx, jy = Fraction(jitter[0]), Fraction(jitter[1]); out = {}
    for Y in range(H):
        for X in range(W):
            u, v = (X + Fraction(1, 2)) * w / W, (Y + Fraction(1, 2)) * h / H
            k = lambda i, j: max(1 - ((i + Fraction(1, 2) - jx - u) ** 2 + (j + Fraction(1, 2) - jy - v) ** 2), 0) ** 2
            mine = k(*lit)
            if mine: out[(X, Y)] = mine / sum(k(i, j) for j in range(-1, h + 1) for i in range(-1, w + 1))
    return out


def test_one_lit_render_pixel_has_the_hand_worked_footprint_and_moves_against_the_jitter():
    w, h = 11, 9; W, H = 22, 18; lit = (5, 4)
    c = image(w, h, lambda x, y: 1.0 if (x, y) == lit else 0.0)
    outs = {}
    for j in ((0.0, 0.0), (0.5, -0.5), (0.25, 0.25)):
        out = outs[j] = taau.upscale(c, None, None, None, taau.params(), (W, H), j)
        want = _exact_footprint(w, h, W, H, lit, j)
        got = {(X, Y): out[Y, X, 0] for Y in range(H) for X in range(W) if out[Y, X, 0] != 0}
        assert set(got) == set(want), (j, sorted(got), sorted(want))
        for k in want: assert got[k] == _round(want[k]), (j, k)
    # at jitter 0 the footprint is the 4 x 4 display pixels around the sample at display (11, 9), without its corners
    assert {k for k in _exact_footprint(w, h, W, H, lit, (0.0, 0.0))} == {(X, Y) for X in range(9, 13) for Y in range(7, 11)} - {(9, 7), (12, 7), (9, 10), (12, 10)}
    # the sign convention: jitter (0.5, -0.5) moves the sample by (-0.5, +0.5) render pixels = (-1, +1) display pixels, bit for bit
    a, b = outs[(0.0, 0.0)], outs[(0.5, -0.5)]
    assert same(b[1:, :-1], a[:-1, 1:]) and not same(a, b)


def test_motion_is_scaled_to_display_pixels_and_bounded_by_the_display_size():
    w, h = 11, 9; W, H = 22, 18
    hist = image(W, H, lambda x, y: float((3 * x + 5 * y) % 7)); cur = flat(w, h, 0.0)
    P = taau.params(newFrameWeight=0.5, **PLAIN)
    for cm in (1, 0):
        st = {}
        out = taau.upscale(cur, motion(w, h, lambda x, y: (1, 0)), None, hist, dict(P, useCatmullRomFilter=cm), (W, H), stages=st)
        for Y in range(H):
            for X in range(W):
                if X + 2 < W:                                                # previous position X + 2.5 <= W: beyond w, inside the display
                    assert st["valid"][Y, X] and np.all(st["history"][Y, X] == hist[Y, X + 2, 0]) and np.all(out[Y, X, :3] == f32(0.5) * hist[Y, X + 2, 0])
                else:
                    assert not st["valid"][Y, X] and np.all(out[Y, X, :3] == 0)
        out = taau.upscale(cur, motion(w, h, lambda x, y: (0, -1.5)), None, hist, dict(P, useCatmullRomFilter=cm), (W, H), stages=st)
        for Y in range(H):
            assert np.all(st["valid"][Y] == (Y >= 3)) and (Y < 3 or np.all(st["history"][Y, :, 0] == hist[Y - 3, :, 0]))
    # the previous position W exactly is still inside (motion 0.25 render pixels = 0.5 display pixels at the last column); a NaN motion takes the no-history path
    out = taau.upscale(cur, motion(w, h, lambda x, y: (0.25, 0)), None, hist, dict(P, useCatmullRomFilter=0), (W, H), stages=st)
    assert st["valid"][:, W - 1].all() and np.all(out[:, W - 1, 0] == f32(0.5) * hist[:, W - 1, 0])
    out = taau.upscale(flat(w, h, 0.25), motion(w, h, lambda x, y: (np.nan, 0)), None, hist, taau.params(), (W, H), stages=st)
    assert not st["valid"].any() and np.all(out[..., :3] == f32(0.25)) and np.all(out[..., 3] == 1)
    # a non-integer ratio: 13 x 7 -> 20 x 10 scales x by 20 / 13 and y by 10 / 7, in binary32
    st = {}
    taau.upscale(flat(13, 7, 0.0), motion(13, 7, lambda x, y: (1, 1)), None, flat(20, 10, 1.0), P, (20, 10), stages=st)
    px, py = st["previous"]
    assert px[0, 0] == f32(0.5) + f32(20) / f32(13) and py[0, 0] == f32(0.5) + f32(10) / f32(7)


def _scene(name, w, h):
    if name == "sine": return lambda x, y: 0.5 + 0.5 * np.sin(2 * np.pi * (11 * x / w + 5 * y / h))
    return lambda x, y: np.where((y / h - 0.5) > 0.37 * (x / w - 0.5), 1.125, 0.125)


def _render(fn, w, h, jitter):
    """point-sampled at (i + 0.5 - jx, j + 0.5 - jy) in float64, then float32; grey"""
    ys, xs = np.mgrid[0:h, 0:w]
    g = fn(xs + 0.5 - float(jitter[0]), ys + 0.5 - float(jitter[1])).astype(f32)
    return np.concatenate([np.repeat(g[..., None], 3, -1), np.ones((h, w, 1), f32)], -1)


def _truth(fn, w, h, W, H, n=8):
    """the n x n box supersample of every display pixel, positions in render pixels"""
    Ys, Xs = np.mgrid[0:H, 0:W]; acc = np.zeros((H, W))
    for b in range(n):
        for a in range(n): acc += fn((Xs + (a + 0.5) / n) * w / W, (Ys + (b + 0.5) / n) * h / H)
    return acc / (n * n)


def _rms(a, b): return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))


USEFULNESS = {}


@pytest.mark.parametrize("plain", [0, 1])
@pytest.mark.parametrize("render,display", PAIRS)
@pytest.mark.parametrize("scene", ["sine", "edge"])
def test_thirty_two_jittered_frames_beat_both_bilinear_enlargements(scene, render, display, plain):
    """The condition of docs/WIDENING.md N8: the RMS of the 32nd upscaled frame against the supersampled truth is at most 0.8 x the smaller of (a) the bilinear enlargement of
    taa_ref.resolve over the same 32 frames at the render size and (b) the bilinear enlargement of one unjittered frame. 0.8 comes from a float64 prototype of these formulas
    (worst ratio 0.72: sine, 3 x, against (b)); a flipped jitter sign gives 1.0 to 1.9 and an ignored jitter 0.9 to 1.2."""
    (w, h), (W, H) = render, display
    fn = _scene(scene, w, h); truth = _truth(fn, w, h, W, H)
    P = taau.params(**(dict(enableHistoryClamping=0, luminanceWeighted=0) if plain else {}))
    up = res = None; z = motion(w, h)
    for f in range(32):
        j = taa.jitter(taa.JITTER_HALTON, f)
        frame = _render(fn, w, h, j)
        up = taau.upscale(frame, z, None, up, P, display, j)
        res = taa.resolve(frame, z, None, res, taau.taa_params(P))
    e = _rms(up[..., 0], truth)
    a = _rms(taau.bilinear(res, display)[..., 0], truth); b = _rms(taau.bilinear(_render(fn, w, h, (0.0, 0.0)), display)[..., 0], truth)
    ratio = e / min(a, b)
    print("TAAU usefulness %s %dx%d -> %dx%d %s: rms %.6g, resolved+bilinear %.6g, single+bilinear %.6g, ratio %.4f" % (scene, w, h, W, H, "plain" if plain else "defaults", e, a, b, ratio))
    assert np.all(np.isfinite(up)) and ratio <= 0.8, (e, a, b, ratio)


def test_tex_lod_bias():
    import rtxpt_amd as pt
    for fn in (taau.tex_lod_bias, pt.upscale_tex_lod_bias):
        assert fn(1920, 1080, 3840, 2160) == -1 and fn(960, 540, 3840, 2160) == -2 and fn(1280, 720, 2560, 1440) == -1
        assert fn(1920, 1080, 1920, 1080) == 0 and fn(35, 10, 35, 10) == 0
        got = fn(2560, 1440, 3840, 2160); assert got.dtype == f32
        assert abs(float(got) - float(-np.log2(np.sqrt(np.float32(2.25))))) <= 1e-6, got
    for bad in ((0, 1080, 3840, 2160), (1920, 0, 3840, 2160), (1920, 1080, 0, 2160), (1920, 1080, 3840, 0)):
        with pytest.raises(pt.PtError) as e: pt.upscale_tex_lod_bias(*bad)
        assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT


def test_header_declares_and_library_exports_the_entry_points():
    import rtxpt_amd as pt
    text = open(os.path.join(ROOT, "include", "mi355pt.h")).read()
    for n in ENTRY_POINTS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % n, text), n
        assert n in pt.EXPORTS, n
    assert "} PtTaaUpscaleParams;" in text
    L = pt.load_library()
    for n in ENTRY_POINTS: assert hasattr(L, n), n
    d = pt.taa_upscale_default_params()
    assert d.dtype.itemsize == 36 and d.dtype.names == tuple(taau.DEFAULTS) and d.dtype.names[:7] == pt.TAA_PARAMS_DTYPE.names
    for k, v in taau.DEFAULTS.items(): assert d[k] == f32(v) if isinstance(v, float) else d[k] == v, k      # the restatement's defaults are the library's
    t = pt.taa_default_params()
    for k in t.dtype.names: assert d[k] == t[k], k
    assert pt.taa_upscale_default_params(kernelRadius=2.0)["kernelRadius"] == 2.0
    for n in ("taa_upscale", "upscaled", "upscaled_size", "upscaled_device_buffer", "bloom_upscaled", "upscaled_bloomed", "tonemap_upscaled", "average_luminance_upscaled"):
        assert callable(getattr(pt.PathTracer, n)), n

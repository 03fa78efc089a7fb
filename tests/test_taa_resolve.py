"""The temporal anti-aliasing resolve (pt_taa_resolve, rtxpt_amd/csrc/pt_taa.h) on the CPU: its numpy restatement (tests/taa_ref.py) held to answers that do not come from it —
values worked by hand on 11 x 9, 13 x 7 and 35 x 10 frames (the last a full 32 x 8 pass tile plus a partial one in both axes), moments worked with fractions.Fraction, a
closed-form exponential average evaluated in float64 straight from the input frames — and pt_taa_jitter's restatement to the published definitions of the two sequences; then
the public interface (include/mi355pt.h declares the entry points, libmi355pt.so exports them, the host-only pt_taa_jitter equals the restatement). Colours are small dyadic
rationals, so the expected values are exact. The device is held to the restatement bit for bit in tests/test_gpu_zzzz_taa_resolve.py."""
import itertools, os, re, sys
from fractions import Fraction
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import taa_ref as taa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZES = [(11, 9), (13, 7), (35, 10)]
ENTRY_POINTS = ("pt_taa_default_params", "pt_taa_resolve", "pt_resolved_device_buffer", "pt_get_resolved", "pt_tonemap_resolved", "pt_taa_jitter")
FLAGS = ("enableHistoryClamping", "useHistoryClampRelax", "useCatmullRomFilter", "luminanceWeighted")
PLAIN = dict(luminanceWeighted=0, enableHistoryClamping=0)      # out = h + (c - h) x newFrameWeight, nothing else


def bits(a): return np.asarray(a, f32).view(np.uint32)
def same(a, b): return np.array_equal(bits(a), bits(b))


def image(w, h, fn):
    """[h, w, 4] float32 with rgb = fn(x, y) (a scalar or three values) and alpha 7 (the resolve must not pass it on)"""
    a = np.zeros((h, w, 4), f32); a[..., 3] = 7
    for y in range(h):
        for x in range(w): a[y, x, :3] = fn(x, y)
    return a


def flat(w, h, v): return image(w, h, lambda x, y: v)
def motion(w, h, fn=lambda x, y: (0, 0)): return image(w, h, lambda x, y: tuple(fn(x, y)) + (0,))[..., :2].copy()
def ramp(x, y): return x + 2 * y


@pytest.mark.parametrize("w,h", SIZES)
def test_first_frame_is_the_sanitised_input(w, h):
    c = image(w, h, lambda x, y: (0.25 * x, 0.5 * y, 1.0))
    c[1, 2, :3] = (np.nan, np.inf, -np.inf); c[2, 3, :3] = (-1.0, 20000.0, -0.0); c[h - 1, w - 1, :3] = (3e38, 1e-40, 10000.0)
    want = c.copy(); want[..., 3] = 1
    want[1, 2, :3] = 0; want[2, 3, :3] = (0, 10000, 0); want[h - 1, w - 1, :3] = (10000, 1e-40, 10000)
    mv = motion(w, h, lambda x, y: (3, -2))
    hist = flat(w, h, 9.0)
    for P in (taa.params(), taa.params(**PLAIN)):
        assert same(taa.resolve(c, mv, None, None, P), want)                 # no history: first frame, reset, dropped
    # with a history, a pixel whose previous position is NaN takes the same way
    mv_nan = motion(w, h, lambda x, y: (np.nan, 0))
    assert same(taa.resolve(c, mv_nan, None, hist, taa.params()), want)
    assert same(taa.resolve(c, mv, None, None, taa.params(maxRadiance=0.5))[..., :3], np.minimum(want[..., :3], f32(0.5)))


@pytest.mark.parametrize("w,h", SIZES)
def test_flat_field_stays_flat_with_every_flag_combination(w, h):
    c, mv = flat(w, h, 0.5), motion(w, h)
    relax = np.full((h, w), 255, np.uint8); relax[::2] = 0
    want = flat(w, h, 0.5); want[..., 3] = 1
    for combo in itertools.product((0, 1), repeat=4):
        P = taa.params(**dict(zip(FLAGS, combo)))
        hist = None
        for f in range(8):
            hist = taa.resolve(c, mv, relax, hist, P)
            assert same(hist, want), (combo, f)


@pytest.mark.parametrize("w,h", SIZES)
def test_step_between_frames_blends_by_the_new_frame_weight(w, h):
    P = taa.params(newFrameWeight=0.5, **PLAIN); mv = motion(w, h)
    a = taa.resolve(flat(w, h, 0.25), mv, None, None, P); assert np.all(a[..., :3] == f32(0.25))
    b = taa.resolve(flat(w, h, 0.75), mv, None, a, P); assert np.all(b[..., :3] == f32(0.5)) and np.all(b[..., 3] == 1)
    c = taa.resolve(flat(w, h, 0.75), mv, None, b, P); assert np.all(c[..., :3] == f32(0.625))
    # newFrameWeight 1 is the current frame whatever the history, also luminance-weighted: beta = w_c / (w_c + 0) = 1
    d = taa.resolve(flat(w, h, 0.75), mv, None, flat(w, h, 4.0), taa.params(newFrameWeight=1.0, enableHistoryClamping=0)); assert np.all(d[..., :3] == f32(0.75))


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("catmull", [1, 0])
def test_integer_motion_fetches_the_texel_itself(w, h, catmull):
    P = taa.params(newFrameWeight=0.5, useCatmullRomFilter=catmull, **PLAIN)
    hist = image(w, h, lambda x, y: float((3 * x + 5 * y) % 7))
    cur = flat(w, h, 0.0)
    st = {}
    out = taa.resolve(cur, motion(w, h, lambda x, y: (3, 0)), None, hist, P, stages=st)
    for y in range(h):
        for x in range(w):
            if x + 3 < w:                                                    # previous position x + 3.5 <= w
                assert np.all(st["history"][y, x] == hist[y, x + 3, 0]) and np.all(out[y, x, :3] == f32(0.5) * hist[y, x + 3, 0])
                assert st["valid"][y, x]
            else:                                                            # it leaves the frame: the current colour
                assert not st["valid"][y, x] and np.all(out[y, x, :3] == 0)
    # the previous position w exactly (pixel w - 1 with mv 0.5) is still inside: both taps clamp to the last column
    out = taa.resolve(cur, motion(w, h, lambda x, y: (0.5, 0)), None, hist, taa.params(newFrameWeight=0.5, useCatmullRomFilter=0, **PLAIN))
    assert np.all(out[:, w - 1, 0] == f32(0.5) * hist[:, w - 1, 0])
    out = taa.resolve(cur, motion(w, h, lambda x, y: (0.75, 0)), None, hist, P)
    assert np.all(out[:, w - 1, :3] == 0)                                   # w + 0.25: outside


@pytest.mark.parametrize("w,h", SIZES)
def test_motion_is_dilated_by_the_longest_vector_and_ties_go_to_the_first(w, h):
    hist = image(w, h, lambda x, y: float((3 * x + 5 * y) % 7)); cur = flat(w, h, 0.0)
    P = taa.params(newFrameWeight=0.5, **PLAIN)
    cx, cy = 4, 3
    st = {}
    taa.resolve(cur, motion(w, h, lambda x, y: (2, 0) if (x, y) == (cx, cy) else (0, 0)), None, hist, P, stages=st)
    for y in range(h):
        for x in range(w):
            near = abs(x - cx) <= 1 and abs(y - cy) <= 1
            assert tuple(st["motion"][y, x]) == ((2, 0) if near else (0, 0))
            assert np.all(st["history"][y, x] == hist[y, x + 2 if near else x, 0])
    # the tile edge of the device's 32 x 8 tiles: a vector at (32, 8) reaches (31, 7), which another block resolves
    if w > 32:
        taa.resolve(cur, motion(w, h, lambda x, y: (-2, 0) if (x, y) == (32, 8) else (0, 0)), None, hist, P, stages=st)
        assert tuple(st["motion"][7, 31]) == (-2, 0) and tuple(st["motion"][9, 33]) == (-2, 0) and tuple(st["motion"][6, 31]) == (0, 0)
    # equal lengths: (1, 0) at (cx - 1, cy - 1) comes before (0, 1) at (cx + 1, cy - 1) and (-1, 0) at (cx, cy + 1) in scan-line order
    tie = {(cx - 1, cy - 1): (1, 0), (cx + 1, cy - 1): (0, 1), (cx, cy + 1): (-1, 0)}
    taa.resolve(cur, motion(w, h, lambda x, y: tie.get((x, y), (0, 0))), None, hist, P, stages=st)
    assert tuple(st["motion"][cy, cx]) == (1, 0)
    assert tuple(st["motion"][cy, cx + 1]) == (0, 1)                        # (its 3 x 3 does not hold the first one)
    assert tuple(st["motion"][cy + 1, cx]) == (-1, 0)
    # an edge pixel repeats: the clamped 3 x 3 of (0, 0) is rows 0, 0, 1 x columns 0, 0, 1
    taa.resolve(cur, motion(w, h, lambda x, y: (1, 1) if (x, y) == (1, 1) else (0, 0)), None, hist, P, stages=st)
    assert tuple(st["motion"][0, 0]) == (1, 1) and tuple(st["motion"][0, 3]) == (0, 0)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("catmull", [1, 0])
@pytest.mark.parametrize("mv", [(0.5, 0.0), (0.25, -0.5), (-0.75, 0.5), (1.0, -1.0)])
def test_fractional_motion_reproduces_a_linear_ramp_exactly(w, h, catmull, mv):
    hist = image(w, h, ramp)
    # through the sampler alone ...
    ys, xs = np.mgrid[2:h - 2, 2:w - 2]
    px, py = (xs + 0.5 + mv[0]).astype(f32), (ys + 0.5 + mv[1]).astype(f32)
    got = taa.sample_history(hist, px, py, bool(catmull))
    want = (xs + mv[0]) + 2 * (ys + mv[1])
    assert np.array_equal(got[..., 0].astype(np.float64), want) and same(got[..., 0], got[..., 2])
    # ... and through the resolve: the current frame is the moved ramp, so c == h and the blend returns h whatever beta is (clamping on: the ramp's own 3 x 3 holds c)
    cur = image(w, h, lambda x, y: ramp(x + mv[0], y + mv[1]))
    out = taa.resolve(cur, motion(w, h, lambda x, y: mv), None, hist, taa.params(useCatmullRomFilter=catmull))
    assert np.array_equal(out[2:h - 2, 2:w - 2, 1].astype(np.float64), want)


@pytest.mark.parametrize("w,h", SIZES)
def test_ghost_is_removed_by_the_clamp_and_kept_without_it(w, h):
    hist, cur, mv = flat(w, h, 1.0), flat(w, h, 0.0), motion(w, h)
    for lw in (0, 1):
        assert np.all(taa.resolve(cur, mv, None, hist, taa.params(luminanceWeighted=lw))[..., :3] == 0)
    out = taa.resolve(cur, mv, None, hist, taa.params(**PLAIN))
    assert np.all(out[..., :3] == f32(1) - f32(0.1))                        # 1 + (0 - 1) x alpha


def _fraction_moments(values):
    """mean and sigma of nine exactly representable values: exact rationals, rounded to binary32 once per operation the text states (divisions and the root)"""
    s1, s2 = sum(Fraction(float(v)) for v in values), sum(Fraction(float(v)) ** 2 for v in values)
    assert f32(float(s1)) == float(s1) and f32(float(s2)) == float(s2)      # (the sums themselves are exact in binary32)
    mean, m2 = f32(float(s1 / 9)), f32(float(s2 / 9))
    var = f32(m2 - f32(mean * mean))
    return mean, f32(np.sqrt(max(var, f32(0))))


@pytest.mark.parametrize("w,h", SIZES)
def test_relax_widens_the_box_fourfold(w, h):
    cur = image(w, h, lambda x, y: float((x + 2 * y) % 3))                  # not flat: every 3 x 3 of the interior holds 0, 1, 2 three times each
    hist, mv = flat(w, h, 64.0), motion(w, h)
    x, y = 5, 4
    mean, sigma = _fraction_moments([cur[y + dy, x + dx, 0] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    assert mean == 1 and 0.8 < sigma < 0.82                                 # sqrt(2 / 3)
    for byte, k in ((0, f32(1)), (255, f32(4)), (51, f32(1) + f32(3) * (f32(51) / f32(255)))):
        st = {}
        relax = np.full((h, w), byte, np.uint8)
        taa.resolve(cur, mv, relax, hist, taa.params(), stages=st)
        assert np.all(st["history"] == 64)
        assert np.all(bits(st["history_clamped"][y, x]) == bits(f32(mean + f32(sigma * k)))), (byte, st["history_clamped"][y, x])
        assert st["mean"][y, x, 0] == mean and bits(st["sigma"][y, x, 0]) == bits(sigma)
        off = {}
        taa.resolve(cur, mv, relax, hist, taa.params(useHistoryClampRelax=0), stages=off)
        assert np.all(bits(off["history_clamped"][y, x]) == bits(f32(mean + sigma)))      # unchanged whatever the buffer holds
    # clampingFactor scales the box; 0 collapses it onto the mean
    st = {}
    taa.resolve(cur, mv, None, hist, taa.params(clampingFactor=0.0), stages=st); assert np.all(st["history_clamped"][y, x] == mean)
    taa.resolve(cur, mv, None, hist, taa.params(clampingFactor=2.0), stages=st); assert np.all(bits(st["history_clamped"][y, x]) == bits(f32(mean + f32(sigma * f32(2)))))
    # a history below the box comes up to mean - sigma
    taa.resolve(cur + f32(8), mv, None, flat(w, h, 0.0), taa.params(), stages=st)
    m8, s8 = _fraction_moments([cur[y + dy, x + dx, 0] + 8 for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    assert np.all(bits(st["history_clamped"][y, x]) == bits(f32(m8 - s8)))


def test_luminance_weighted_blend_by_hand():
    """one pixel's worth: c = (3, 3, 3) -> w_c = 1 / 4, h = (1, 1, 1) -> w_h = 1 / 2, alpha = 0.5: beta = 0.125 / (0.125 + 0.25) = 1 / 3"""
    w, h = SIZES[0]
    lum1 = f32(f32(f32(0.2126) + f32(0.7152)) + f32(0.0722))                # Luminance((1, 1, 1)) as the text sums it
    out = taa.resolve(flat(w, h, 3.0), motion(w, h), None, flat(w, h, 1.0), taa.params(newFrameWeight=0.5, enableHistoryClamping=0))
    lum3 = f32(f32(f32(3) * f32(0.2126) + f32(3) * f32(0.7152)) + f32(3) * f32(0.0722))
    wc, wh = f32(1) / (f32(1) + lum3), f32(1) / (f32(1) + lum1)
    a, b = f32(0.5) * wc, f32(0.5) * wh
    want = f32(1) + f32(2) * (a / (a + b))
    assert np.all(bits(out[..., :3]) == bits(want)) and abs(float(want) - (1 + 2 / 3)) < 1e-6
    assert float(want) < 2                                                  # the bright sample counts for less than with the plain weight (2)


@pytest.mark.parametrize("w,h", SIZES)
def test_twelve_random_frames_equal_the_closed_form_exponential_average(w, h):
    """clamping off, weighting off, motion (1, 0): out_n(x) = sum_k alpha (1 - alpha)^k c_(n - k)(x + k) + (1 - alpha)^K c_(n - K)(x + K), where the track starts at frame
    n - K — the first frame, or the frame on which the previous position left the picture. float64 from the input frames; 1e-6 is binary32 rounding over 12 blends."""
    rng = np.random.default_rng(5)
    frames = [rng.uniform(0.25, 4.0, (h, w)).astype(f32) for _ in range(12)]
    alpha = 0.25; P = taa.params(newFrameWeight=alpha, **PLAIN); mv = motion(w, h, lambda x, y: (1, 0))
    hist = None
    for n, fr in enumerate(frames):
        hist = taa.resolve(np.repeat(fr[..., None], 4, -1), mv, None, hist, P)
        want = np.zeros((h, w))
        for x in range(w):
            K = min(n, w - 1 - x)                                           # frames back along the track until it starts
            acc = frames[n - K][:, x + K].astype(np.float64) * (1 - alpha) ** K
            for k in range(K): acc += alpha * (1 - alpha) ** k * frames[n - k][:, x + k].astype(np.float64)
            want[:, x] = acc
        assert np.allclose(hist[..., 0], want, rtol=1e-6, atol=0), n
        assert same(hist[..., 0], hist[..., 1]) and np.all(hist[..., 3] == 1)


def test_jitter_sequences_are_the_published_ones():
    halton = [(Fraction(1, 2), Fraction(1, 3)), (Fraction(1, 4), Fraction(2, 3)), (Fraction(3, 4), Fraction(1, 9)), (Fraction(1, 8), Fraction(4, 9)),
              (Fraction(5, 8), Fraction(7, 9)), (Fraction(3, 8), Fraction(2, 9)), (Fraction(7, 8), Fraction(5, 9)), (Fraction(1, 16), Fraction(8, 9))]
    for i, (a, b) in enumerate(halton):
        x, y = taa.jitter(taa.JITTER_HALTON, i)
        assert x == f32(float(a - Fraction(1, 2))) and y == f32(float(b - Fraction(1, 2))), i
    for i in (0, 1, 2, 7, 100, 1023, 65535):
        x, y = taa.jitter(taa.JITTER_R2, i)
        for got, a in ((x, 0.7548776662466927), (y, 0.5698402909980532)):
            v = 0.5 + (i + 1) * a
            assert got == f32((v - np.floor(v)) - 0.5)
    for seq in (taa.JITTER_HALTON, taa.JITTER_R2):
        pts = np.array([taa.jitter(seq, i) for i in range(1024)])
        assert pts.dtype == f32 and np.all(pts >= -0.5) and np.all(pts < 0.5)
        assert abs(pts.mean()) < 0.01 and len({tuple(p) for p in pts}) == 1024      # centred on the pixel, no repeats
    for seq in (0, 3, 4):
        with pytest.raises(ValueError): taa.jitter(seq, 0)


def test_header_declares_and_library_exports_the_entry_points():
    import rtxpt_amd as pt
    text = open(os.path.join(ROOT, "include", "mi355pt.h")).read()
    for n in ENTRY_POINTS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % n, text), n
        assert n in pt.EXPORTS, n
    assert "} PtTaaParams;" in text
    L = pt.load_library()
    for n in ENTRY_POINTS: assert hasattr(L, n), n
    d = pt.taa_default_params()
    assert d.dtype.itemsize == 28 and d.dtype.names == tuple(taa.DEFAULTS)
    for k, v in taa.DEFAULTS.items(): assert d[k] == f32(v) if isinstance(v, float) else d[k] == v, k      # the restatement's defaults are the library's
    assert pt.taa_default_params(newFrameWeight=0.5)["newFrameWeight"] == 0.5


def test_library_jitter_equals_the_restatement():
    """pt_taa_jitter is host only: it runs without a device"""
    import rtxpt_amd as pt
    for seq in (pt.TAA_JITTER_HALTON, pt.TAA_JITTER_R2):
        for i in list(range(64)) + [1023, 65535, 2 ** 24, 2 ** 32 - 1]:
            assert pt.taa_jitter(seq, i) == taa.jitter(seq, i), (seq, i)
    for seq in (0, 3, 4):
        with pytest.raises(pt.PtError) as e: pt.taa_jitter(seq, 0)
        assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT

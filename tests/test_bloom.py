"""The bloom pass (pt_bloom, rtxpt_amd/csrc/pt_bloom.h) on the CPU: its numpy restatement (tests/bloom_ref.py) held to answers that do not come from it — values worked by hand
on 11 x 9, 13 x 7, 35 x 10 (the sizes of test_taa_resolve.py: every one has partial 4 x 4 blocks, and at radius 64 the quarter-resolution image is narrower than the 48 taps, so
every tap clamps) and 70 x 37 frames, the taps from decimal arithmetic, a float64 normalised Gaussian, exact dyadic ramps, conservation of the picture's sum — then the public
interface (include/mi355pt.h declares the entry points, libmi355pt.so exports them, the host-only pt_bloom_kernel equals the restatement). The device is held to the
restatement bit for bit in tests/test_gpu_zzzzz_bloom.py."""
import decimal, os, re, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_ref as bloom
import test_taa_resolve as cpu_taa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZES = cpu_taa.SIZES + [(70, 37)]
ENTRY_POINTS = ("pt_bloom_default_params", "pt_bloom_kernel", "pt_bloom", "pt_bloomed_device_buffer", "pt_get_bloomed", "pt_tonemap_bloomed", "pt_average_luminance_bloomed")
SKIPS = (dict(enable=0), dict(intensity=0.0), dict(radius=0.0))
RADII, INTENSITIES = (0.5, 3.0, 8.0, 64.0), (0.004, 0.5, 1.0)
EPS = 2.0 ** -24      # half an ulp of binary32, relative: one rounding step
bits, same, image, flat = cpu_taa.bits, cpu_taa.same, cpu_taa.image, cpu_taa.flat


def dirty_frame(w, h, tiny=1e-40):
    """the frame of test_first_frame_is_the_sanitised_input and the same frame sanitised by hand (its clean twin; alpha stays 7)"""
    c = image(w, h, lambda x, y: (0.25 * x, 0.5 * y, 1.0))
    c[1, 2, :3] = (np.nan, np.inf, -np.inf); c[2, 3, :3] = (-1.0, 20000.0, -0.0); c[h - 1, w - 1, :3] = (3e38, tiny, 10000.0)
    want = c.copy()
    want[1, 2, :3] = 0; want[2, 3, :3] = (0, 10000, 0); want[h - 1, w - 1, :3] = (10000, tiny, 10000)
    return c, want


def lit_block(w, h, x0, y0, v=1.0):
    """black except the 4 x 4 block at (x0, y0) .. (x0 + 3, y0 + 3)"""
    return image(w, h, lambda x, y: v if x0 <= x < x0 + 4 and y0 <= y < y0 + 4 else 0.0)


@pytest.mark.parametrize("w,h", SIZES)
def test_skipped_pass_is_the_source_byte_for_byte(w, h):
    c, _ = dirty_frame(w, h)
    assert np.isnan(c).any() and np.all(c[..., 3] == 7)
    for kw in SKIPS:
        out = bloom.bloom(c, bloom.params(**kw))
        assert out is not c and np.array_equal(out.view(np.uint8), c.view(np.uint8)), kw
    assert not np.array_equal(bloom.bloom(c, bloom.params()).view(np.uint8), c.view(np.uint8))


@pytest.mark.parametrize("w,h", SIZES)
def test_sanitised_values_enter_both_the_colour_and_the_blur(w, h):
    c, clean = dirty_frame(w, h)
    P = bloom.params(intensity=0.5)
    st = {}
    out = bloom.bloom(c, P, stages=st)
    assert same(st["s"], clean[..., :3])                                     # s is the hand-sanitised frame
    assert same(out, bloom.bloom(clean, P))                                  # ... and so is what was reduced: the clean twin blooms to the same picture
    assert np.all(np.isfinite(out)) and np.all(out[..., :3] >= 0) and np.all(out[..., 3] == 1)
    # the NaN pixel is black in s: at intensity 0.5 it shows half the blur and nothing else
    assert same(out[1, 2, :3], st["b"][1, 2] * f32(0.5))
    half = np.minimum(clean[..., :3], f32(0.5))
    st = {}
    out = bloom.bloom(c, bloom.params(intensity=0.5, maxRadiance=0.5), stages=st)
    assert same(st["s"], half) and st["Q"].max() <= 0.5 and np.all(out[..., :3] <= 0.5)
    twin = clean.copy(); twin[..., :3] = half
    assert same(out, bloom.bloom(twin, P))


@pytest.mark.parametrize("w,h", SIZES)
def test_flat_fields_stay_flat_bit_for_bit(w, h):
    for v in (0.5, 2.0, 0.25):
        want = flat(w, h, v); want[..., 3] = 1
        for r in RADII:
            for k in INTENSITIES:
                assert same(bloom.bloom(flat(w, h, v), bloom.params(radius=r, intensity=k)), want), (v, r, k)


def test_reduce_repeats_the_edge_and_takes_the_exact_mean():
    w, h = 35, 10
    s = bloom.sanitise(image(w, h, lambda x, y: 4.0 if x >= 32 else 0.0), 10000.0)
    Q = bloom.reduce(s)
    assert Q.shape == (3, 9, 3) and np.all(Q[:, 8] == 4) and np.all(Q[:, :8] == 0)      # columns 32, 33, 34 and 34 again; rows 8, 9, 9, 9
    vals = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 1, 2, 3], [0, 5, 0, 11]]
    s = bloom.sanitise(image(w, h, lambda x, y: (vals[y - 4][x - 8], 2 * vals[y - 4][x - 8], 0) if 8 <= x < 12 and 4 <= y < 8 else 0.0), 10000.0)
    Q = bloom.reduce(s)
    total = sum(sum(r) for r in vals)
    assert total % 16 and tuple(Q[1, 2]) == (total / 16, 2 * total / 16, 0)
    assert np.count_nonzero(Q[..., 0]) == 1
    # the bottom right corner block of 35 x 10 holds (34, 8) (34, 9) and their repeats: columns 32 33 34 34 x rows 8 9 9 9
    s = bloom.sanitise(image(w, h, lambda x, y: 16.0 if (x, y) == (34, 9) else 0.0), 10000.0)
    assert bloom.reduce(s)[2, 8, 0] == 6                                     # 2 columns x 3 rows of the 16 places


def test_taps_for_radius_4_by_hand():
    g, G = bloom.kernel(4.0)
    decimal.getcontext().prec = 60
    want = [f32(float(decimal.Decimal(e).exp())) for e in ("0", "-0.5", "-2", "-4.5")]      # sigma = 1: exp(-i^2 / 2)
    assert len(g) == 4 and g.dtype == f32 and G.dtype == f32
    assert all(bits(a) == bits(b) for a, b in zip(g, want)), (g, want)
    acc = f32(1)
    for i in (1, 2, 3): acc = f32(acc + f32(want[i] * f32(2)))
    assert bits(G) == bits(acc) and abs(float(G) - 2.5066) < 0.03           # near sqrt(2 pi), truncated at 3 sigma
    for r, R in ((0.01, 1), (1.33, 1), (1.34, 2), (8, 6), (64, 48)):
        assert len(bloom.kernel(r)[0]) == R + 1, r
    for r in (0.0, -1.0, 64.5, np.nan, np.inf):
        with pytest.raises(ValueError): bloom.kernel(r)


def test_impulse_is_centred_symmetric_and_separable():
    w, h = 35, 10
    st = {}
    bloom.bloom(lit_block(w, h, 16, 4), bloom.params(radius=4.0), stages=st)
    Q, B = st["Q"][..., 0], st["B"][..., 0]
    assert Q[1, 4] == 1 and np.count_nonzero(Q) == 1
    g, G = bloom.kernel(4.0)
    centre = f32(f32(f32(f32(1) * f32(1)) / G) * f32(1)) / G
    assert bits(B[1, 4]) == bits(centre)
    assert same(B, B[:, ::-1]) and same(B, B[::-1, :])
    assert np.all(B[:, 1:8] > 0) and np.all(B[:, 0] == 0) and np.all(B[:, 8] == 0)      # three taps reach columns 1 .. 7
    lhs, rhs = B * B[1, 4], B[:, 4:5] * B[1:2, :]
    ulp = np.spacing(np.maximum(lhs, rhs))
    assert np.all(np.abs(lhs - rhs) <= 4 * ulp)


@pytest.mark.parametrize("radius", [3.0, 8.0])
def test_blur_agrees_with_a_float64_normalised_gaussian(radius):
    """64 x 2^-24 relative per texel: the blur takes 2 (R + 2) rounding steps per axis (R + 1 products, R sums of pairs ... the division), R <= 6, on positive values"""
    w, h = 200, 120
    rng = np.random.default_rng(7)
    src = np.concatenate([rng.uniform(0.25, 4.0, (h, w, 3)).astype(f32), np.ones((h, w, 1), f32)], -1)
    st = {}
    bloom.bloom(src, bloom.params(radius=radius), stages=st)
    Q = st["Q"].astype(np.float64)
    sigma = 0.25 * radius; R = max(1, int(np.ceil(3 * sigma)))
    wts = np.exp(-np.arange(-R, R + 1) ** 2 / (2 * sigma * sigma)); wts /= wts.sum()
    want = Q
    for axis in (1, 0):
        n = want.shape[axis]; idx = np.arange(n)
        want = sum(np.take(want, np.clip(idx + d, 0, n - 1), axis) * wts[d + R] for d in range(-R, R + 1))
    rel = np.abs(st["B"].astype(np.float64) - want) / want
    print("bloom blur against float64, radius %g: largest relative difference %.3g (bound %.3g)" % (radius, rel.max(), 64 * EPS))
    assert rel.max() <= 64 * EPS


@pytest.mark.parametrize("w,h", SIZES)
def test_composite_returns_a_quarter_resolution_ramp_exactly(w, h):
    src = image(w, h, lambda x, y: float(x // 4))                           # constant per 4 x 4 block: Q(X, Y) = X
    st = {}
    out = bloom.bloom(src, bloom.params(radius=0.01, intensity=1.0), stages=st)
    assert same(st["B"], st["Q"]) and np.all(st["Q"][..., 0] == np.arange((w + 3) // 4)[None, :])      # radius 0.01: the blur is the identity
    want = (np.arange(w) + 0.5) / 4 - 0.5
    assert np.array_equal(out[:, 2:w - 2, 1].astype(np.float64), np.broadcast_to(want[2:w - 2], (h, w - 4)))
    # the clamped border: pixels 0 and 1 see tap -1 as tap 0
    assert np.all(out[:, :2, 0] == 0)
    # intensity 0.5 over a black colour is half the blur, exactly
    b = st["b"]
    assert same(bloom.composite(np.zeros_like(b), b, 0.5), b * f32(0.5)) and same(bloom.composite(np.zeros_like(b), b, 0.5), b / f32(2))
    assert same(bloom.composite(b, b, 0.3), b)                               # and s == b returns s whatever the intensity


def test_energy_is_kept_and_the_glow_reaches_twelve_pixels():
    """sum(out) == sum(s): the reduce is a mean over 16 pixels that the bilinear step hands back to 16 pixels, and the taps are divided by their own sum. Every value is a sum
    of products of non-negative numbers, at most 17 (reduce) + 2 x 16 (blur, R = 6) + 8 (bilinear) + 3 (composite) = 60 rounding steps deep: 64 x 2^-24 relative."""
    w, h = 200, 120
    src = lit_block(w, h, 96, 56, 64.0)
    for k in (1.0, 0.5, 0.004):
        out = bloom.bloom(src, bloom.params(radius=8.0, intensity=k))[..., 0].astype(np.float64)
        total = 16 * 64.0
        print("bloom energy, intensity %g: sum(out) / sum(s) - 1 = %.3g (bound %.3g)" % (k, out.sum() / total - 1, 64 * EPS))
        assert abs(out.sum() - total) <= 64 * EPS * total
    out = bloom.bloom(src, bloom.params(radius=8.0, intensity=1.0))[..., 0]
    ys, xs = np.mgrid[0:h, 0:w]
    dx = np.maximum(np.maximum(96 - xs, xs - 99), 0); dy = np.maximum(np.maximum(56 - ys, ys - 59), 0)
    ring = (np.maximum(dx, dy) >= 12) & (np.maximum(dx, dy) <= 16)
    assert ring.sum() > 0 and np.all(out[ring] > 0)
    assert np.all(out[np.maximum(dx, dy) > 32] == 0)                         # 6 taps + the bilinear foot: nothing beyond 4 x (6 + 1) + 4 pixels
    assert 0 < out.max() < 64


def test_header_declares_and_library_exports_the_entry_points():
    import rtxpt_amd as pt
    text = open(os.path.join(ROOT, "include", "mi355pt.h")).read()
    for n in ENTRY_POINTS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % n, text), n
        assert n in pt.EXPORTS, n
    assert "} PtBloomParams;" in text
    L = pt.load_library()
    for n in ENTRY_POINTS: assert hasattr(L, n), n
    d = pt.bloom_default_params()
    assert d.dtype.itemsize == 16 and d.dtype.names == tuple(bloom.DEFAULTS)
    assert (d["radius"], d["intensity"], d["maxRadiance"], d["enable"]) == (f32(8), f32(0.004), f32(10000), 1)
    for k, v in bloom.DEFAULTS.items(): assert d[k] == f32(v) if isinstance(v, float) else d[k] == v, k      # the restatement's defaults are the library's
    assert pt.bloom_default_params(radius=3.0)["radius"] == 3.0


def test_library_taps_equal_the_restatement():
    """pt_bloom_kernel is host only: it runs without a device"""
    import rtxpt_amd as pt
    for r in (0.01, 1.0, 4.0, 8.0, 33.3, 64.0):
        g, G = pt.bloom_kernel(r); want_g, want_G = bloom.kernel(r)
        assert g.shape == want_g.shape and np.array_equal(bits(g), bits(want_g)) and bits(G) == bits(want_G), r
    for r in (0.0, -1.0, 64.5, np.nan, np.inf):
        with pytest.raises(pt.PtError) as e: pt.bloom_kernel(r)
        assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT, r
    R = len(bloom.kernel(8.0)[0]) - 1
    with pytest.raises(pt.PtError) as e: pt.bloom_kernel(8.0, capacity=R)
    assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT
    assert len(pt.bloom_kernel(8.0, capacity=R + 1)[0]) == R + 1

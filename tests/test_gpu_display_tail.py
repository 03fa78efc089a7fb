"""The display tail over every picture a host can show (run with -m gpu): the radiance buffer, the resolved picture, the bloomed one, the upscaled one and its bloom, and the
denoised accumulation — one table, the same rows for each. A record of behaviour that the tail's entry points share: each tone map equals ptref.tonemap of that picture's
read-back byte for byte, each average luminance is ptref.average_luminance of it, each device buffer has that picture's pitch; the frame-size and the display-size bloomed
pictures do not know of each other; every entry point refuses in its own order; event timing is optional and changes no picture. Small frames only (13 x 7 -> 20 x 9 and
35 x 10 -> 53 x 17: no power of two, non-integer ratios): these kernels go wrong at edges and odd sizes. Only the public API is used."""
import ctypes, os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_ref as bloom
import test_taa_resolve as cpu_taa
import test_gpu_zzz_denoiser_inputs as dni
import test_gpu_zzz_relax_denoiser as gz
import test_gpu_zzzz_taa_resolve as gtaa
import test_gpu_zzzzz_bloom as gbloom
from rtxpt_amd import scenes

pytestmark = pytest.mark.gpu
_eq, _code, _push_colour, _push_motion = dni._eq, gtaa._code, gtaa._push_colour, gtaa._push_motion
f32 = np.float32
CASES = [((13, 7), (20, 9)), ((35, 10), (53, 17))]                               # (render, display)
assert all(r in cpu_taa.SIZES and r[0] <= d[0] <= 4 * r[0] and r[1] <= d[1] <= 4 * r[1] and d[0] % r[0] and d[1] % r[1] for r, d in CASES)
BLOOM = dict(radius=8.0, intensity=0.5)
_cache = {}


def _tonemaps():
    import rtxpt_amd as pt
    return (pt.default_tonemap(), pt.default_tonemap(exposure_compensation=-2.0, toneMapOperator="reinhard"), pt.default_tonemap(autoExposure=1, avgLuminance=0.3))


def _noise(w, h, seed):
    return np.concatenate([np.random.default_rng(seed).uniform(0.25, 4.0, (h, w, 3)).astype(f32), np.ones((h, w, 1), f32)], -1)


def _bits(a): return np.ascontiguousarray(a).view(np.uint8)


# (name, read-back, tone map, average luminance or None, device buffer or None, 0: frame size / 1: display size) — None where include/mi355pt.h has no such entry point
PICTURES = [
    ("radiance", lambda t: t.radiance(), lambda t, tm: t.tonemap(tm), lambda t: t.average_luminance(), None, 0),
    ("resolved", lambda t: t.get_resolved(), lambda t, tm: t.tonemap_resolved(tm), None, lambda t: t.resolved_device_buffer(), 0),
    ("bloomed", lambda t: t.bloomed(), lambda t, tm: t.tonemap_bloomed(tm), lambda t: t.average_luminance_bloomed(), lambda t: t.bloomed_device_buffer(), 0),
    ("upscaled", lambda t: t.upscaled(), lambda t, tm: t.tonemap_upscaled(tm), lambda t: t.average_luminance_upscaled(), lambda t: t.upscaled_device_buffer(), 1),
    ("upscaled_bloomed", lambda t: t.upscaled_bloomed(), lambda t, tm: t.tonemap_upscaled(tm, bloomed=True), lambda t: t.average_luminance_upscaled(bloomed=True), None, 1),
    ("accum_denoised", lambda t: t.accum_denoised(), lambda t, tm: t.tonemap_accum_denoised(tm), lambda t: t.average_luminance_accum_denoised(), lambda t: t.accum_denoised_device_buffer(), 0),
]


def _all_pictures(render, display):
    """one context per case with all six pictures there, and their read-backs (made once, shared by the rows, never written)"""
    if render not in _cache:
        import rtxpt_amd as pt
        w, h = render
        t, _, _ = gz._pushed_tracer(w, h)
        colour = _noise(w, h, 3)
        _push_motion(t, cpu_taa.motion(w, h), w, h); _push_colour(t, colour, w, h)
        t.taa_resolve(reset_history=True); t.bloom(pt.bloom_default_params(**BLOOM), source=1)
        t.taa_upscale(None, display, (0.25, -0.375), reset_history=True); t.bloom_upscaled(pt.bloom_default_params(**BLOOM))
        t.accum_denoise_host_inputs(colour, (colour * f32(0.75) + _noise(w, h, 4) * f32(0.25)).astype(f32))
        back = {name: read(t) for name, read, _, _, _, _ in PICTURES}
        assert _eq(back["radiance"], colour)
        for name, _, _, _, _, size in PICTURES:
            W, H = (render, display)[size]
            assert back[name].shape == (H, W, 4) and np.all(np.isfinite(back[name])) and back[name][..., :3].max() > 0, name
        _cache[render] = (t, back)
    return _cache[render]


# ---- 1. every picture against its reference
@pytest.mark.parametrize("render,display", CASES)
@pytest.mark.parametrize("picture", PICTURES, ids=[p[0] for p in PICTURES])
def test_every_tail_equals_the_reference_over_its_picture(picture, render, display):
    from oracle import ptref
    name, read, tonemap, luminance, device_buffer, size = picture
    t, back = _all_pictures(render, display)
    W, H = (render, display)[size]
    for i, tm in enumerate(_tonemaps()):
        out = tonemap(t, tm)
        assert out.shape == (H, W, 4) and np.array_equal(out, ptref.tonemap(back[name], tm)), "%s, tone map setting %d" % (name, i)
    if luminance:
        lum, want = luminance(t), ptref.average_luminance(back[name])
        print("%s %r: average luminance %.9g, reference %.9g, relative difference %.3g" % (name, (W, H), lum, want, abs(lum / want - 1)))
        assert np.isfinite(lum) and lum > 0 and abs(lum / want - 1) < 2e-5, (name, lum, want)      # the tolerance of tests/test_display_path.py for pt_average_luminance
    if device_buffer:
        ptr, pitch = device_buffer(t)
        assert ptr and pitch == 16 * W, (name, ptr, pitch)
    assert np.array_equal(_bits(read(t)), _bits(back[name]))                     # the tail writes no picture


def test_the_pictures_are_six_buffers():
    t, back = _all_pictures(*CASES[0])
    ptrs = [buf(t)[0] for _, _, _, _, buf, _ in PICTURES if buf]
    assert len(set(ptrs)) == len(ptrs)
    assert not _eq(back["bloomed"], back["resolved"]) and not _eq(back["upscaled_bloomed"], back["upscaled"]) and not _eq(back["accum_denoised"], back["radiance"])


# ---- 2. the two bloom states are independent
@pytest.mark.parametrize("render,display", CASES)
def test_the_frame_size_and_the_display_size_bloom_do_not_know_of_each_other(render, display):
    import rtxpt_amd as pt
    w, h = render
    P, Q = pt.bloom_default_params(**BLOOM), pt.bloom_default_params(radius=4.0, intensity=1.0)
    colour = _noise(w, h, 5)

    def upscaled_tracer():
        t, _, _ = gz._pushed_tracer(w, h)
        _push_motion(t, cpu_taa.motion(w, h), w, h); _push_colour(t, colour, w, h)
        return t, t.taa_upscale(None, display, (0.0, 0.0), reset_history=True)

    t, up = upscaled_tracer()                                                    # pt_bloom only: the display-size bloom is not there
    got = t.bloom(P, source=0)
    assert _code(lambda: t.tonemap_upscaled(bloomed=True)) == pt.PT_ERROR_NOT_READY and _code(lambda: t.average_luminance_upscaled(bloomed=True)) == pt.PT_ERROR_NOT_READY
    assert _code(t.upscaled_bloomed) == pt.PT_ERROR_NOT_READY
    assert _eq(got, bloom.bloom(colour, bloom.params(**BLOOM)))
    t.close()
    t, up = upscaled_tracer()                                                    # pt_bloom_upscaled only, on a context that never had a pt_bloom
    big = t.bloom_upscaled(P)
    for r in (t.tonemap_bloomed, t.average_luminance_bloomed, t.bloomed, t.bloomed_device_buffer): assert _code(r) == pt.PT_ERROR_NOT_READY
    small = t.bloom(P, source=0)                                                 # both: each of its own size, each the restatement of its own source
    assert small.shape == (h, w, 4) and big.shape == (display[1], display[0], 4)
    assert _eq(small, bloom.bloom(colour, bloom.params(**BLOOM))) and _eq(big, bloom.bloom(up, bloom.params(**BLOOM)))
    assert np.array_equal(_bits(t.upscaled_bloomed()), _bits(big))
    other = t.bloom(Q, source=0)                                                 # a second pt_bloom with other parameters: the display-size picture keeps its bits
    assert not _eq(other, small) and np.array_equal(_bits(t.upscaled_bloomed()), _bits(big)) and np.array_equal(_bits(t.bloomed()), _bits(other))
    again = t.bloom_upscaled(Q)                                                  # ... and the other way round
    assert not _eq(again, big) and np.array_equal(_bits(t.bloomed()), _bits(other))
    t.close()


# ---- 3. the order of the refusals, one row per entry point
BAD_BLOOM = [dict(radius=65.0), dict(intensity=np.nan), dict(maxRadiance=0.0)]
# (entry point, call with parameters P, the code on a context with a frame size and nothing else, a word of the message): the codes are those of the library before the tail
# was gathered into one file. pt_bloom and pt_bloom_upscaled look at the parameters before the readiness of their source, pt_bloom_accum_denoised after it.
BLOOM_ROWS = [
    ("pt_bloom, source 0", lambda t, P: t.bloom(P, source=0), "PT_ERROR_INVALID_ARGUMENT", "bloom parameters"),
    ("pt_bloom, source 1", lambda t, P: t.bloom(P, source=1), "PT_ERROR_INVALID_ARGUMENT", "bloom parameters"),
    ("pt_bloom, source 2", lambda t, P: t.bloom(P, source=2), "PT_ERROR_INVALID_ARGUMENT", "bloom source"),
    ("pt_bloom_upscaled", lambda t, P: t.bloom_upscaled(P), "PT_ERROR_INVALID_ARGUMENT", "bloom parameters"),
    ("pt_bloom_accum_denoised", lambda t, P: t.bloom_accum_denoised(P), "PT_ERROR_NOT_READY", "pt_accum_denoise"),
]


@pytest.mark.parametrize("row", BLOOM_ROWS, ids=[r[0] for r in BLOOM_ROWS])
def test_bloom_entry_points_refuse_in_their_own_order(row):
    import rtxpt_amd as pt
    name, call, code, word = row
    t = gbloom._plain_tracer(13, 7)
    for kw in BAD_BLOOM:
        with pytest.raises(pt.PtError) as e: call(t, pt.bloom_default_params(**kw))
        assert e.value.code == getattr(pt, code) and word in str(e.value), (name, kw, str(e.value))
    # with good parameters the sources that are not there are what is refused
    want = dict([("pt_bloom, source 0", None), ("pt_bloom, source 2", pt.PT_ERROR_INVALID_ARGUMENT)]).get(name, pt.PT_ERROR_NOT_READY)
    if want is None: assert call(t, pt.bloom_default_params()).shape == (7, 13, 4)
    else: assert _code(lambda: call(t, pt.bloom_default_params())) == want
    t.close()


# (entry point, the arguments between the context and the rgba8 pointer as a function of the parameters' pointer, 0: frame size / 1: display size)
TONEMAP_ROWS = [
    ("pt_tonemap", lambda tm: (tm,), 0),
    ("pt_tonemap_resolved", lambda tm: (tm,), 0),
    ("pt_tonemap_bloomed", lambda tm: (tm,), 0),
    ("pt_tonemap_upscaled", lambda tm: (tm, ctypes.c_uint32(0)), 1),
    ("pt_tonemap_upscaled, bloomed", lambda tm: (tm, ctypes.c_uint32(1)), 1),
    ("pt_tonemap_accum_denoised", lambda tm: (tm,), 0),
]


@pytest.mark.parametrize("row", TONEMAP_ROWS, ids=[r[0] for r in TONEMAP_ROWS])
def test_tone_map_entry_points_refuse_in_the_same_order(row):
    """readiness, then the size of the caller's buffer, then the operator"""
    import rtxpt_amd as pt
    name, middle, size = row
    render, display = CASES[0]
    ready, _ = _all_pictures(render, display)
    W, H = (render, display)[size]
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    tm = pt.default_tonemap(); six = pt.default_tonemap(); six["toneMapOperator"] = 6
    o8 = np.zeros((H, W, 4), np.uint8)
    f = getattr(ready.L, name.split(",")[0]); f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_uint32] * (len(middle(None)) - 1) + [ctypes.c_void_p, ctypes.c_size_t]
    call = lambda t, p, n: f(t.h, *(middle(vp(p)) + (vp(o8), n)))
    assert call(ready, tm, o8.nbytes - 1) == pt.PT_ERROR_INVALID_ARGUMENT and b"too small" in ready.L.pt_get_last_error(ready.h)
    assert call(ready, six, o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT and b"operator" in ready.L.pt_get_last_error(ready.h)
    assert call(ready, six, o8.nbytes - 1) == pt.PT_ERROR_INVALID_ARGUMENT and b"too small" in ready.L.pt_get_last_error(ready.h)
    assert np.all(o8 == 0)                                                       # (a refused call writes nothing)
    assert call(ready, tm, o8.nbytes) == pt.PT_OK and o8.any()
    # the picture is not there: a context without a frame size for the radiance buffer, one with a frame size and nothing else for the others
    bare = pt.PathTracer() if name == "pt_tonemap" else gbloom._plain_tracer(*render)
    for p, n in ((tm, o8.nbytes - 1), (six, o8.nbytes), (tm, 0)): assert call(bare, p, n) == pt.PT_ERROR_NOT_READY, (name, n)
    bare.close()


# ---- 4. timing stays optional
def _rendered_for_adaptive(w, h):
    import rtxpt_amd as pt
    sc, cam = scenes.cornell_box("C1")
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), scenes.config_settings("C1"), w, h)
    t.render_adaptive(pt.adaptive_default_params(minSamples=4, step=2, maxSamples=4, threshold=0.0))
    return t


def test_a_timed_call_after_an_untimed_one_times_and_changes_no_picture():
    render, display = CASES[0]; w, h = render
    t, _, _ = gz._pushed_tracer(w, h)
    _push_motion(t, cpu_taa.motion(w, h), w, h); _push_colour(t, _noise(w, h, 6), w, h)
    a = _rendered_for_adaptive(w, h)
    A, Hf = _noise(w, h, 7), _noise(w, h, 8)
    passes = [("taa_resolve", lambda **kw: t.taa_resolve(reset_history=True, **kw)),
              ("taa_upscale", lambda **kw: t.taa_upscale(None, display, (0.25, -0.375), reset_history=True, **kw)),
              ("bloom", lambda **kw: t.bloom(source=1, **kw)),
              ("bloom_upscaled", lambda **kw: t.bloom_upscaled(**kw)),
              ("accum_denoise", lambda **kw: a.accum_denoise(**kw)),
              ("accum_denoise_host_inputs", lambda **kw: t.accum_denoise_host_inputs(A, Hf, **kw))]
    for name, call in passes:
        first = call()
        timed, ms = call(timed=True)
        print("%s: %.6f ms" % (name, ms))
        assert np.isfinite(ms) and ms >= 0, (name, ms)
        again = call()
        assert np.array_equal(_bits(first), _bits(timed)) and np.array_equal(_bits(first), _bits(again)), name
    t.close(); a.close()

"""The bloom pass on the device (run with -m gpu): pt_bloom against the numpy restatement (tests/bloom_ref.py) bit for bit, the bloomed buffer after every call — the worked
frames of tests/test_bloom.py at 11 x 9, 13 x 7 and 35 x 10 (colour through pt_unpack_shard on a world of one), one frame sized from the blur kernels' tiles, the resolved
picture as the source (and the resolve's history left alone), the skipped pass, pt_tonemap_bloomed, pt_average_luminance_bloomed, rendered frames of both modes, and the
refusals."""
import ctypes, os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_ref as bloom
import taa_ref as taa
import stable_planes_cases as spc
import test_bloom as cpu_bloom
import test_taa_resolve as cpu_taa
import test_gpu_zzz_denoiser_inputs as dni
import test_gpu_zzz_relax_denoiser as gz
import test_gpu_zzzz_taa_resolve as gtaa
from rtxpt_amd import scenes

pytestmark = pytest.mark.gpu
_eq, _diff, _code, _push_colour, _push_motion = dni._eq, dni._diff, gtaa._code, gtaa._push_colour, gtaa._push_motion
f32 = np.float32
image, flat, motion = cpu_taa.image, cpu_taa.flat, cpu_taa.motion
RADII, INTENSITIES = (0.5, 4.0, 8.0, 64.0), (0.004, 0.5, 1.0)


def _params(**kw):
    import rtxpt_amd as pt
    return pt.bloom_default_params(**kw)


def _plain_tracer(w, h):
    """a context with a frame size and nothing rendered: all that source 0 needs"""
    sc, cam = scenes.stable_planes_zoo()
    return dni._tracer(sc, scenes.bridge_camera(w, h, **cam), scenes.config_settings("C2"), w, h)


def _check(t, colour, kw, tag, source=0):
    """pt_bloom on what the device holds as `colour` against the restatement; the source is left as it was"""
    got = t.bloom(_params(**kw), source=source)
    want = bloom.bloom(colour, bloom.params(**kw))
    assert _eq(got, want), "%s %r: differs in %d values" % (tag, kw, _diff(got, want))
    return want


def worked_frames(w, h):
    """(name, colour): the frames tests/test_bloom.py works by hand (the dirty frame without its denormal, as in the resolve's device test)"""
    vals = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 1, 2, 3], [0, 5, 0, 11]]
    rng = np.random.default_rng(11)
    return [("dirty", cpu_bloom.dirty_frame(w, h, tiny=0.5)[0]),
            ("flat_0.5", flat(w, h, 0.5)), ("flat_2", flat(w, h, 2.0)), ("flat_0.25", flat(w, h, 0.25)),
            ("right_edge", image(w, h, lambda x, y: 4.0 if x >= w - 3 else 0.0)),
            ("hand_block", image(w, h, lambda x, y: (vals[y - 4][x - 4], 2 * vals[y - 4][x - 4], 0) if 4 <= x < 8 and 4 <= y < 8 else 0.0)),
            ("corner", image(w, h, lambda x, y: 16.0 if (x, y) == (w - 1, h - 1) else 0.0)),
            ("impulse", cpu_bloom.lit_block(w, h, 4, 4)),
            ("ramp", image(w, h, lambda x, y: float(x // 4))),
            ("random", np.concatenate([rng.uniform(0.25, 4.0, (h, w, 3)).astype(f32), np.full((h, w, 1), 7, f32)], -1))]


@pytest.mark.parametrize("w,h", cpu_taa.SIZES)
def test_worked_frames_equal_the_restatement(w, h):
    t = _plain_tracer(w, h)
    for name, colour in worked_frames(w, h):
        _push_colour(t, colour, w, h)
        for r in RADII:
            for k in INTENSITIES:
                out = _check(t, colour, dict(radius=r, intensity=k), name)
                if name.startswith("flat_"): assert np.all(out[..., :3] == colour[0, 0, 0])
                assert np.all(out[..., 3] == 1)
        if name == "dirty": _check(t, colour, dict(intensity=0.5, maxRadiance=0.5), name)
        if name == "ramp":
            out = _check(t, colour, dict(radius=0.01, intensity=1.0), name)
            assert np.array_equal(out[:, 2:w - 2, 0].astype(np.float64), np.broadcast_to(((np.arange(w) + 0.5) / 4 - 0.5)[2:w - 2], (h, w - 4)))
        assert _eq(t.radiance(), colour)                                     # the source is never written
    t.close()


@pytest.mark.parametrize("radius", [8.0, 64.0])
def test_a_frame_of_two_full_blur_tiles_and_a_partial_one_in_both_axes(radius):
    """531 x 274: the quarter-resolution image is 133 x 69. k_bloom_blur_x works on 64 x 4 tiles (133 = 2 x 64 + 5, 69 = 17 x 4 + 1), k_bloom_blur_y on 8 x 32 tiles
    (133 = 16 x 8 + 5, 69 = 2 x 32 + 5): two full tiles and a partial one along each pass's own axis, partial tiles across it, and partial 4 x 4 blocks at the right (531 =
    4 x 132 + 3) and at the bottom (274 = 4 x 68 + 2). Radius 8 stages 6 halo texels, radius 64 all 48: wider than a y tile is tall and nearly as wide as an x tile."""
    w, h = 531, 274
    rng = np.random.default_rng(3)
    colour = np.concatenate([(rng.random((h, w, 3)) * 4).astype(f32), np.ones((h, w, 1), f32)], -1)
    for (x, y), v in {(0, 0): np.nan, (w - 1, h - 1): np.inf, (256, 128): -np.inf, (255, 127): -3.0, (w - 1, 0): np.nan, (130, 273): 3e38, (64 * 4, 32 * 4 - 1): -0.0}.items():
        colour[y, x, :3] = v
    t = _plain_tracer(w, h)
    _push_colour(t, colour, w, h)
    out = _check(t, colour, dict(radius=radius, intensity=0.5), "tiles")
    assert np.all(np.isfinite(out))
    assert _eq(t.radiance(), colour)
    t.close()


@pytest.mark.parametrize("w,h", cpu_taa.SIZES)
def test_resolved_picture_as_the_source_and_its_history_left_alone(w, h):
    t, _, _ = gz._pushed_tracer(w, h)
    TP, tp = gtaa._params(), taa.params()
    z = motion(w, h); dirty = cpu_bloom.dirty_frame(w, h, tiny=0.5)[0]
    held = _push_motion(t, z, w, h); _push_colour(t, dirty, w, h)
    first = t.taa_resolve(TP, reset_history=True)
    assert _eq(first, taa.resolve(dirty, held, None, None, tp))
    for kw in (dict(), dict(radius=4.0, intensity=0.5), dict(enable=0)):
        _check(t, first, kw, "source 1", source=1)
        assert _eq(t.get_resolved(), first) and _eq(t.radiance(), dirty)    # both sources byte-identical after the call
    # the next frame resolves against `first` as if no bloom had run
    second_colour = np.concatenate([np.random.default_rng(2).uniform(0.25, 4.0, (h, w, 3)).astype(f32), np.ones((h, w, 1), f32)], -1)
    gtaa._new_frame(t, w, h); held = _push_motion(t, motion(w, h, lambda x, y: (0.5, -0.25)), w, h); _push_colour(t, second_colour, w, h)
    second = t.taa_resolve(TP)
    want = taa.resolve(second_colour, held, None, first, tp)
    assert _eq(second, want), _diff(second, want)
    assert not _eq(second, taa.resolve(second_colour, held, None, None, tp))                       # (the history was really read)
    _check(t, second, dict(radius=8.0, intensity=1.0), "source 1, second frame", source=1)
    assert _eq(t.get_resolved(), second)
    t.close()


@pytest.mark.parametrize("w,h", cpu_taa.SIZES)
def test_skipped_pass_copies_the_source_bytes(w, h):
    t = _plain_tracer(w, h)
    dirty = cpu_bloom.dirty_frame(w, h, tiny=0.5)[0]; assert np.isnan(dirty).any() and np.all(dirty[..., 3] == 7)
    _push_colour(t, dirty, w, h)
    for kw in cpu_bloom.SKIPS:
        t.bloom(_params(), source=0)                                         # something else in the buffer first
        got = t.bloom(_params(**kw), source=0)
        assert np.array_equal(got.view(np.uint8), t.radiance().view(np.uint8)) and _eq(got, dirty), kw
        # downstream calls still work, on the same bytes as their radiance-buffer twins (the luminance of a picture with a NaN in it is NaN, there as here)
        assert np.array_equal(t.tonemap_bloomed(), t.tonemap()) and np.array_equal(f32(t.average_luminance_bloomed()), f32(t.average_luminance()), equal_nan=True)
    t.close()


def _zoo_resolved():
    t, frame, camd, cfg, prm = dni._zoo_frame("zoo_fp32")
    w, h = spc.W, spc.H
    t.denoise_frame(prm, dni._dn(camd, w, h), gz._settings())
    t.taa_resolve(gtaa._params(), reset_history=True); t.taa_resolve(gtaa._params())
    return t, w, h


def test_tonemap_and_average_luminance_of_the_bloomed_picture():
    import rtxpt_amd as pt
    from oracle import ptref
    t, w, h = _zoo_resolved()
    resolved = t.get_resolved()
    got = t.bloom(_params(radius=8.0, intensity=0.5), source=1)
    assert _eq(got, bloom.bloom(resolved, bloom.params(radius=8.0, intensity=0.5))) and not _eq(got, resolved)
    ptr, pitch = t.bloomed_device_buffer(); assert ptr and pitch == 16 * w and ptr not in (t.resolved_device_buffer()[0],)
    for tm in (pt.default_tonemap(), pt.default_tonemap(exposure_compensation=-2.0, toneMapOperator="reinhard"), pt.default_tonemap(autoExposure=1, avgLuminance=0.3)):
        out = t.tonemap_bloomed(tm)
        assert out.shape == (h, w, 4) and np.array_equal(out, ptref.tonemap(t.bloomed(), tm))
    assert not np.array_equal(t.tonemap_bloomed(), t.tonemap_resolved())
    lum, want = t.average_luminance_bloomed(), ptref.average_luminance(t.bloomed())
    assert np.isfinite(lum) and lum > 0 and abs(lum / want - 1) < 2e-5, (lum, want)      # the tolerance of tests/test_display_path.py for pt_average_luminance
    assert lum != t.average_luminance()
    t.close()


def test_rendered_frames_of_both_modes_equal_the_restatement():
    import rtxpt_amd as pt
    t, w, h = _zoo_resolved()                                                # realtime: build, fill, denoise, resolve -> bloom(source 1) at the defaults
    resolved = t.get_resolved(); assert resolved[..., :3].max() > 0
    got, ms = t.bloom(_params(), source=1, timed=True)
    want = bloom.bloom(resolved, bloom.params())
    assert _eq(got, want), _diff(got, want)
    assert np.isfinite(ms) and ms >= 0 and not _eq(got, resolved)
    t.close()
    sc, cam = scenes.cornell_box("C1")                                       # reference mode: pt_render -> bloom(source 0)
    g = pt.PathTracer(device=0); g.set_scene(sc); g.set_camera(scenes.bridge_camera(32, 32, **cam)); g.set_settings(scenes.config_settings("C1")); g.resize(32, 32)
    g.render(0, 2)
    rad = g.radiance(); assert rad[..., :3].max() > 0
    got = g.bloom(_params(), source=0)
    want = bloom.bloom(rad, bloom.params())
    assert _eq(got, want), _diff(got, want)
    assert _eq(g.radiance(), rad)
    g.close()


def test_state_and_refusals():
    import rtxpt_amd as pt
    w, h = 13, 7
    t = _plain_tracer(w, h)
    readers = (lambda: t.bloomed(), lambda: t.bloomed_device_buffer(), lambda: t.tonemap_bloomed(), lambda: t.average_luminance_bloomed())
    for r in readers: assert _code(r) == pt.PT_ERROR_NOT_READY                                    # before any pt_bloom
    assert _code(lambda: t.bloom(_params(), source=1)) == pt.PT_ERROR_NOT_READY                   # no resolved picture
    for r in readers: assert _code(r) == pt.PT_ERROR_NOT_READY                                    # (a refused call blooms nothing)
    assert _code(lambda: t.bloom(_params(), source=2)) == pt.PT_ERROR_INVALID_ARGUMENT
    bad = [dict(radius=65.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(intensity=1.5), dict(intensity=-0.5), dict(intensity=np.nan),
           dict(maxRadiance=0.0), dict(maxRadiance=-1.0), dict(maxRadiance=np.nan), dict(maxRadiance=np.inf)]
    for kw in bad: assert _code(lambda: t.bloom(_params(**kw), source=0)) == pt.PT_ERROR_INVALID_ARGUMENT, kw
    for r in readers: assert _code(r) == pt.PT_ERROR_NOT_READY
    L, P = t.L, _params()
    f = L.pt_bloom; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
    assert f(t.h, None, 0, None) == pt.PT_ERROR_INVALID_ARGUMENT and f(None, P.ctypes.data_as(ctypes.c_void_p), 0, None) == pt.PT_ERROR_INVALID_ARGUMENT
    colour = flat(w, h, 0.5); _push_colour(t, colour, w, h)
    _, ms = t.bloom(_params(radius=64.0, intensity=1.0), source=0, timed=True)                    # the ends of the ranges are inside
    assert np.isfinite(ms) and ms >= 0
    _, ms = t.bloom(_params(enable=0), source=0, timed=True); assert np.isfinite(ms) and ms >= 0
    for r in readers: r()
    t.resize(w, h)                                                           # pt_resize to the same size keeps the bloomed picture
    for r in readers: r()
    t.resize(w + 3, h + 2)
    for r in readers: assert _code(r) == pt.PT_ERROR_NOT_READY
    assert t.bloom(_params(), source=0).shape == (h + 2, w + 3, 4)
    t.resize(w, h)
    for r in readers: assert _code(r) == pt.PT_ERROR_NOT_READY
    out = np.zeros((h, w, 4), f32); o8 = np.zeros((h, w, 4), np.uint8); tm = pt.default_tonemap(); v = ctypes.c_float()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    t.bloom(_params(), source=0)
    g = L.pt_get_bloomed; g.argtypes = [ctypes.c_void_p] * 2; g.restype = ctypes.c_int32
    assert g(t.h, None) == pt.PT_ERROR_INVALID_ARGUMENT and g(None, vp(out)) == pt.PT_ERROR_INVALID_ARGUMENT and g(t.h, vp(out)) == pt.PT_OK
    d = L.pt_bloomed_device_buffer; d.argtypes = [ctypes.c_void_p] * 3; d.restype = ctypes.c_int32
    ptr = ctypes.c_void_p()
    assert d(t.h, None, None) == pt.PT_ERROR_INVALID_ARGUMENT and d(None, ctypes.byref(ptr), None) == pt.PT_ERROR_INVALID_ARGUMENT and d(t.h, ctypes.byref(ptr), None) == pt.PT_OK and ptr.value
    m = L.pt_tonemap_bloomed; m.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t]; m.restype = ctypes.c_int32
    assert m(t.h, None, vp(o8), o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT and m(t.h, vp(tm), None, o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT
    assert m(None, vp(tm), vp(o8), o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT and m(t.h, vp(tm), vp(o8), o8.nbytes - 1) == pt.PT_ERROR_INVALID_ARGUMENT
    assert m(t.h, vp(tm), vp(o8), o8.nbytes) == pt.PT_OK
    a = L.pt_average_luminance_bloomed; a.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; a.restype = ctypes.c_int32
    assert a(t.h, None) == pt.PT_ERROR_INVALID_ARGUMENT and a(None, ctypes.byref(v)) == pt.PT_ERROR_INVALID_ARGUMENT and a(t.h, ctypes.byref(v)) == pt.PT_OK
    p = L.pt_bloom_default_params; p.argtypes = [ctypes.c_void_p]; p.restype = ctypes.c_int32
    assert p(None) == pt.PT_ERROR_INVALID_ARGUMENT
    t.close()

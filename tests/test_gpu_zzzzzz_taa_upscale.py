"""The temporal upscaling resolve on the device (run with -m gpu): pt_taa_upscale against the numpy restatement (tests/taau_ref.py) bit for bit, the upscaled buffer after every
call — worked sequences at five (render -> display) pairs (one partial display tile, non-integer ratios, 4 x 4 display tiles whose staged footprints start mid-frame, the upper
ratio bound, the identity), seven jitters and both history filters; the identity with pt_taa_resolve on the device; rendered zoo frames behind pt_denoise_frame and the
moving-camera realtime frames at 2 x — then what the call must leave alone (the radiance buffer, pt_taa_resolve's history, pt_bloom's picture), the history drops, the display
tail (pt_bloom_upscaled, pt_tonemap_upscaled, pt_average_luminance_upscaled), a two-rank sharded frame, the refusals, and one usefulness check on rendered frames: sixteen
jittered 64 x 48 frames upscaled to 128 x 96 are nearer to a converged 128 x 96 render than one unjittered 64 x 48 frame enlarged bilinearly."""
import ctypes, os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoiser_inputs_ref as ref
import bloom_ref as bloom
import taa_ref as taa
import taau_ref as taau
import stable_planes_cases as spc
import realtime_cases as rc
import test_taa_resolve as cpu_taa
import test_gpu_zzz_denoiser_inputs as dni
import test_gpu_zzz_relax_denoiser as gz
import test_gpu_zzzz_taa_resolve as gtaa
from rtxpt_amd import scenes

pytestmark = pytest.mark.gpu
_eq, _diff, _code, _push_colour, _push_motion, _new_frame, _device_inputs, _rms = dni._eq, dni._diff, gtaa._code, gtaa._push_colour, gtaa._push_motion, gtaa._new_frame, gtaa._device_inputs, gtaa._rms
f32 = np.float32
image, flat, motion, ramp = cpu_taa.image, cpu_taa.flat, cpu_taa.motion, cpu_taa.ramp
PLAIN = dict(cpu_taa.PLAIN, confidenceWeighted=0)
# (render, display): one display tile, partial in both axes; non-integer ratios; 4 x 4 display tiles with partial last ones; the upper ratio bound, 3 x 6 tiles; the identity
PAIRS = [((11, 9), (22, 18)), ((13, 7), (20, 10)), ((35, 10), (105, 30)), ((20, 12), (80, 48)), ((35, 10), (35, 10))]
JITTERS = [(0.0, 0.0), (0.25, -0.375), (-0.5, 0.49999997)] + [taa.jitter(taa.JITTER_HALTON, i) for i in range(4)]


def _params(**kw):
    import rtxpt_amd as pt
    return pt.taa_upscale_default_params(**kw)


def sequences(w, h):
    """(name, parameter keywords, [(colour [h, w, 4], motion [h, w, 2])]): the families of the resolve's worked sequences, at the render size"""
    z = motion(w, h); const = lambda v: motion(w, h, lambda x, y: v)
    dirty = image(w, h, lambda x, y: (0.25 * x, 0.5 * y, 1.0))
    dirty[1, 2, :3] = (np.nan, np.inf, -np.inf); dirty[2, 3, :3] = (-1.0, 20000.0, -0.0); dirty[h - 1, w - 1, :3] = (3e38, 0.5, 10000.0)
    pattern = image(w, h, lambda x, y: float((3 * x + 5 * y) % 7)); black = flat(w, h, 0.0); thirds = image(w, h, lambda x, y: float((x + 2 * y) % 3))
    rng = np.random.default_rng(7)
    noise = lambda: np.concatenate([rng.uniform(0.25, 4.0, (h, w, 3)).astype(f32), np.full((h, w, 1), 7, f32)], -1)
    wander = lambda: rng.choice(np.array([-1.5, -0.75, -0.25, 0, 0.5, 1.25], f32), (h, w, 2))
    one = lambda at, v: motion(w, h, lambda x, y: v if (x, y) == at else (0, 0))
    # single vectors: mid-frame, the corners' neighbours, and (10, 2) — at 3 x and 4 x its display pixels sit on a 32-pixel tile border, the dilation reaches lanes of both
    # blocks and the previous position lies in the other block's pixels
    dil = [one((4, 3), (2, 0)), one((1, 1), (1, 1)), one((w - 1, h - 1), (-1, -1)), one((10, 2), (-2, 0)), one((8, 2), (2.5, 1)), one((w - 2, 0), (0.5, 0.25))]
    return [("sanitise", {}, [(dirty, const((3, -2))), (dirty, const((np.nan, 0))), (dirty, z)]),
            ("sanitise_max_half", dict(maxRadiance=0.5), [(dirty, z), (dirty, z)]),
            ("flat", {}, [(flat(w, h, 0.5), z)] * 3),
            ("constant_motion", dict(newFrameWeight=0.5, **PLAIN), [(pattern, z), (black, const((1, 0))), (pattern, const((0, -2))), (black, const((-4, 3)))]),
            ("fractional_motion", {}, [(noise(), const((0.5, -0.25))) for _ in range(3)] + [(image(w, h, ramp), const((-0.75, 0.5)))]),
            ("dilation", dict(newFrameWeight=0.5, **PLAIN), [(pattern, z)] + [(black, m) for m in dil]),
            ("box", dict(clampingFactor=2.0, useHistoryClampRelax=0), [(flat(w, h, 64.0), z), (thirds, z), (thirds + f32(8), z)]),
            ("random", {}, [(noise(), wander()) for _ in range(4)]),
            ("random_radius_2_plain_weight", dict(kernelRadius=2.0, confidenceWeighted=0, luminanceWeighted=0), [(noise(), wander()) for _ in range(3)]),
            ("random_radius_1.5_no_clamp", dict(kernelRadius=1.5, enableHistoryClamping=0), [(noise(), wander()) for _ in range(3)])]


def _run(t, w, h, display, kw, frames, tag, first_jitter=0):
    """each frame's inputs go in once and are upscaled once, the restatement alongside; the first call of a sequence resets; frame f takes jitter first_jitter + f"""
    P = _params(**kw); hist = None
    for f, (colour, mv) in enumerate(frames):
        j = JITTERS[(first_jitter + f) % len(JITTERS)]
        held = _push_motion(t, mv, w, h); _push_colour(t, colour, w, h)
        got = t.taa_upscale(P, display, j, reset_history=hist is None)
        hist = taau.upscale(colour, held, None, hist, P, display, j)
        assert got.shape == (display[1], display[0], 4) and _eq(got, hist), "%s frame %d jitter %r: differs in %d values" % (tag, f, j, _diff(got, hist))
    return hist


@pytest.mark.parametrize("catmull", [1, 0])
@pytest.mark.parametrize("render,display", PAIRS)
def test_worked_sequences_equal_the_restatement(render, display, catmull):
    w, h = render
    t, _, _ = gz._pushed_tracer(w, h)
    for s, (name, kw, frames) in enumerate(sequences(w, h)):
        for first in range(len(JITTERS)) if name.startswith("random") or name == "dilation" else (s % len(JITTERS),):
            out = _run(t, w, h, display, dict(kw, useCatmullRomFilter=catmull), frames, "%s %r" % (name, display), first)
            if name == "flat": assert np.all(out[..., :3] == f32(0.5))
            assert np.all(out[..., 3] == 1)
    assert t.upscaled_size() == display and t.upscaled_device_buffer()[1] == 16 * display[0]
    t.close()


def test_ratio_one_equals_the_resolve_on_the_device():
    """W x H = w x h, jitter (0, 0), kernelRadius 1: the two passes, each with its own history, give the same bytes frame after frame"""
    w, h = 35, 10
    t, _, _ = gz._pushed_tracer(w, h)
    for name, kw, frames in sequences(w, h):
        if "radius" in name: continue
        U = _params(**kw); T = gtaa._params(**{k: v for k, v in kw.items() if k in taa.DEFAULTS})
        for f, (colour, mv) in enumerate(frames):
            _push_motion(t, mv, w, h); _push_colour(t, colour, w, h)
            a = t.taa_resolve(T, reset_history=f == 0); b = t.taa_upscale(U, (w, h), (0.0, 0.0), reset_history=f == 0)
            assert _eq(a, b), "%s frame %d: differs in %d values" % (name, f, _diff(a, b))
    assert t.upscaled_device_buffer()[0] != t.resolved_device_buffer()[0]
    t.close()


@pytest.mark.parametrize("name", ["zoo_fp32", "zoo_two_planes_no_psr"])
def test_zoo_frames_equal_the_restatement(name):
    """a rendered frame behind pt_denoise_frame, upscaled three times at 2 x: the later calls reproject through the frame's fractional motion vectors into the pass's own
    history and clamp with a relax buffer that is not zero; the radiance buffer stays byte-identical, the two buffers swap, the timed call computes the same"""
    t, frame, camd, cfg, prm = dni._zoo_frame(name)
    w, h = spc.W, spc.H; D = (2 * w, 2 * h)
    t.denoise_frame(prm, dni._dn(camd, w, h), gz._settings())
    colour, mv, relax = _device_inputs(t)
    assert relax.max() > 0 and np.any(mv != np.floor(mv))
    a = t.taa_upscale(_params(), D, JITTERS[3]); pa, pitch = t.upscaled_device_buffer(); assert pa and pitch == 16 * D[0]
    want_a = taau.upscale(colour, mv, relax, None, taau.params(), D, JITTERS[3]); assert _eq(a, want_a), _diff(a, want_a)
    b, ms = t.taa_upscale(_params(), D, JITTERS[4], timed=True); pb, _ = t.upscaled_device_buffer(); assert pb and pb != pa and ms > 0
    want_b = taau.upscale(colour, mv, relax, want_a, taau.params(), D, JITTERS[4]); assert _eq(b, want_b), _diff(b, want_b)
    assert not _eq(want_b, taau.upscale(colour, mv, relax, want_a, taau.params(useHistoryClampRelax=0), D, JITTERS[4]))      # (the relax buffer is really read)
    kw = dict(useHistoryClampRelax=0, useCatmullRomFilter=0, kernelRadius=1.25)
    c = t.taa_upscale(_params(**kw), D, None); assert t.upscaled_device_buffer()[0] == pa                                     # a NULL jitter reads as (0, 0)
    want_c = taau.upscale(colour, mv, relax, want_b, taau.params(**kw), D); assert _eq(c, want_c), _diff(c, want_c)
    assert _eq(t.radiance(), colour) and _eq(t.upscaled(), c)
    t.close()


def test_moving_camera_frames_carry_their_history():
    make, cfg, w, h, frames, subs, step, kw = rc.cases()["zoo_realtime"]
    sc, cam = make(); D = (2 * w, 2 * h)
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), cfg, w, h)
    hist = None
    for f in range(2):
        cur, prev = rc.camera(cam, step, f), rc.camera(cam, step, max(f - 1, 0))
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cur), prev_world_to_clip=scenes.view_projection(w, h, **prev), sub_samples=subs, **kw)
        camd = scenes.bridge_camera(w, h, **cur); t.set_camera(camd)
        t.realtime_frame(f * subs, prm); t.denoise_spec_hit_t()
        t.denoise_frame(prm, dni._dn(camd, w, h), gz._settings())
        colour, mv, relax = _device_inputs(t)
        got = t.taa_upscale(_params(), D, JITTERS[3 + f])
        st = {}
        hist = taau.upscale(colour, mv, relax, hist, taau.params(), D, JITTERS[3 + f], stages=st)
        assert _eq(got, hist), "frame %d: differs in %d values" % (f, _diff(got, hist))
    assert np.any(mv != 0) and st["valid"].any() and not _eq(hist[..., :3], st["current"])      # the second frame did blend with the first
    t.close()


def test_other_passes_buffers_are_left_alone():
    """the radiance buffer; pt_taa_resolve's history (a pt_taa_upscale between two pt_taa_resolve calls does not change the second); pt_bloom's picture"""
    w, h = 13, 7; D = (20, 10)
    t, _, _ = gz._pushed_tracer(w, h)
    rng = np.random.default_rng(2)
    noise = lambda: np.concatenate([rng.uniform(0.25, 4.0, (h, w, 3)).astype(f32), np.ones((h, w, 1), f32)], -1)
    c0, c1 = noise(), noise()
    held = _push_motion(t, motion(w, h), w, h); _push_colour(t, c0, w, h)
    first = t.taa_resolve(gtaa._params(), reset_history=True)
    bloomed = t.bloom(source=1)
    t.taa_upscale(_params(), D, JITTERS[1], reset_history=True); t.bloom_upscaled()
    assert _eq(t.radiance(), c0) and _eq(t.get_resolved(), first) and _eq(t.bloomed(), bloomed)
    _new_frame(t, w, h); held = _push_motion(t, motion(w, h, lambda x, y: (0.5, -0.25)), w, h); _push_colour(t, c1, w, h)
    up = t.taa_upscale(_params(), D, JITTERS[2]); t.bloom_upscaled(); t.tonemap_upscaled(bloomed=True); t.average_luminance_upscaled()
    assert _eq(t.radiance(), c1) and _eq(t.get_resolved(), first) and _eq(t.bloomed(), bloomed)
    second = t.taa_resolve(gtaa._params())
    want = taa.resolve(c1, held, None, first, taa.params())
    assert _eq(second, want), _diff(second, want)
    assert not _eq(second, taa.resolve(c1, held, None, None, taa.params()))                        # (the history was really read)
    assert _eq(t.upscaled(), up)                                                                   # and the resolve leaves the upscaled picture alone
    t.close()


def test_history_drops_behave_as_a_reset():
    """another display size, a resize to another size, pt_set_geometry, and a build pass that was not upscaled; the controls: consecutive build passes and a second call on
    one frame keep the history"""
    import rtxpt_amd as pt
    w, h = 13, 7; D = (26, 14)
    t, _, _ = gz._pushed_tracer(w, h)
    P = _params(newFrameWeight=0.5, **PLAIN)
    a, b, z = flat(w, h, 0.25), flat(w, h, 0.75), motion(w, h)
    pic = lambda v, d=D: np.concatenate([np.full((d[1], d[0], 3), v, f32), np.ones((d[1], d[0], 1), f32)], -1)

    def two_frames(between, second=D):
        _new_frame(t, w, h); _push_motion(t, z, w, h); _push_colour(t, a, w, h); t.taa_upscale(P, D, reset_history=True)
        between()
        _push_motion(t, z, w, h); _push_colour(t, b, w, h)
        return t.taa_upscale(P, second)

    assert _eq(two_frames(lambda: _new_frame(t, w, h)), pic(0.5))                                 # the control: consecutive build passes
    assert _eq(two_frames(lambda: None), pic(0.5))                                                # a second call on one frame
    assert _eq(two_frames(lambda: (_new_frame(t, w, h), _new_frame(t, w, h))), pic(0.75))         # a build pass was skipped
    # another display size (at these ratios the weights are not dyadic and a flat 0.75 is flat only to an ulp: the expected picture is the restatement's reset frame)
    for other in ((20, 10), (26, 15)):
        fresh = taau.upscale(b, z, None, None, taau.params(newFrameWeight=0.5, **PLAIN), other)
        assert abs(fresh[..., :3] - 0.75).max() < 1e-6 and _eq(two_frames(lambda: _new_frame(t, w, h), second=other), fresh) and _eq(two_frames(lambda: None, second=other), fresh)
    sc, _ = scenes.stable_planes_zoo()
    assert _eq(two_frames(lambda: (t.set_scene(sc), _new_frame(t, w, h))), pic(0.75))             # pt_set_geometry
    def resized():
        t.resize(w + 3, h + 2)
        assert _code(lambda: t.taa_upscale(P, (w + 3, h + 2))) == pt.PT_ERROR_NOT_READY
        for r in (t.upscaled, t.upscaled_size, t.upscaled_device_buffer, t.tonemap_upscaled, t.average_luminance_upscaled, t.bloom_upscaled): assert _code(r) == pt.PT_ERROR_NOT_READY
        t.resize(w, h); _new_frame(t, w, h)
    assert _eq(two_frames(resized), pic(0.75))
    t.resize(w, h); _new_frame(t, w, h); _push_motion(t, z, w, h); _push_colour(t, a, w, h)       # pt_resize to the same size keeps it: 0.75 + (0.25 - 0.75) x 0.5
    assert _eq(t.taa_upscale(P, D), pic(0.5))
    t.close()


def test_the_display_tail_runs_at_the_display_size():
    import rtxpt_amd as pt
    from oracle import ptref
    t, frame, camd, cfg, prm = dni._zoo_frame("zoo_fp32")
    w, h = spc.W, spc.H; D = (2 * w - 3, 2 * h - 1)
    t.denoise_frame(prm, dni._dn(camd, w, h), gz._settings())
    t.taa_upscale(_params(), D, JITTERS[3], reset_history=True); up = t.taa_upscale(_params(), D, JITTERS[4])
    assert up.shape == (D[1], D[0], 4) and up[..., :3].max() > 0 and np.all(np.isfinite(up))
    tms = (pt.default_tonemap(), pt.default_tonemap(exposure_compensation=-2.0, toneMapOperator="reinhard"), pt.default_tonemap(autoExposure=1, avgLuminance=0.3))
    assert _code(lambda: t.upscaled_bloomed()) == pt.PT_ERROR_NOT_READY and _code(lambda: t.tonemap_upscaled(bloomed=True)) == pt.PT_ERROR_NOT_READY
    assert _code(lambda: t.average_luminance_upscaled(bloomed=True)) == pt.PT_ERROR_NOT_READY
    for kw in (dict(), dict(radius=4.0, intensity=0.5), dict(radius=64.0, intensity=1.0)):
        got = t.bloom_upscaled(pt.bloom_default_params(**kw))
        want = bloom.bloom(up, bloom.params(**kw))
        assert got.shape == up.shape and _eq(got, want), "%r: differs in %d values" % (kw, _diff(got, want))
        assert _eq(t.upscaled(), up)
    for kw in (dict(enable=0), dict(intensity=0.0), dict(radius=0.0)):                             # the skip rule: the source's bytes
        got, ms = t.bloom_upscaled(pt.bloom_default_params(**kw), timed=True)
        assert np.array_equal(got.view(np.uint8), up.view(np.uint8)) and np.isfinite(ms) and ms >= 0, kw
    bl = t.bloom_upscaled(pt.bloom_default_params(radius=8.0, intensity=0.5)); assert not _eq(bl, up)
    for b, picture in ((False, up), (True, bl)):
        for tm in tms:
            out = t.tonemap_upscaled(tm, bloomed=b)
            assert out.shape == (D[1], D[0], 4) and np.array_equal(out, ptref.tonemap(picture, tm))
        lum, want = t.average_luminance_upscaled(bloomed=b), ptref.average_luminance(picture)
        assert np.isfinite(lum) and lum > 0 and abs(lum / want - 1) < 2e-5, (b, lum, want)        # the tolerance of tests/test_display_path.py for pt_average_luminance
    assert not np.array_equal(t.tonemap_upscaled(), t.tonemap_upscaled(bloomed=True))
    t.taa_upscale(_params(), D, JITTERS[5])                                                        # the next upscale gives the bloomed picture up
    assert _code(lambda: t.upscaled_bloomed()) == pt.PT_ERROR_NOT_READY
    t.close()


def test_tile_sharded_frame_equals_the_unsharded_one():
    import rtxpt_amd as pt, torch
    sc, camd, cfg, prm, _ = spc.setup("zoo_fp32"); w, h = spc.W, spc.H; D = (2 * w, 2 * h)
    dn = dni._dn(camd, w, h); S = gz._settings()
    ranks = [dni._tracer(sc, camd, cfg, w, h, shard_rank=r, shard_count=2) for r in range(2)]
    for t in ranks: t.build_stable_planes(spc.SAMPLE, prm); t.fill_stable_planes(spc.SAMPLE, prm, sub_samples=spc.SUBSAMPLES)
    assert _code(lambda: ranks[0].taa_upscale(_params(), D)) == pt.PT_ERROR_NOT_READY             # the planes of the other rank have not arrived
    n = ranks[1].stable_planes_shard_bytes(1); b = torch.empty(n // 4, dtype=torch.int32, device="cuda"); ranks[1].pack_stable_planes(b.data_ptr(), n)
    ranks[0].unpack_stable_planes(b.data_ptr(), n, 1); ranks[0].denoise_spec_hit_t()
    u, _, _, _, _ = dni._zoo_frame("zoo_fp32")
    outs = []
    for t in (ranks[0], u):
        t.denoise_frame(prm, dn, S)
        outs.append([t.taa_upscale(_params(), D, JITTERS[3]), t.taa_upscale(_params(), D, JITTERS[4])])
    for x, y in zip(*outs): assert _eq(x, y)
    assert not _eq(outs[1][0], outs[1][1])
    for t in ranks + [u]: t.close()


def test_refusals():
    import rtxpt_amd as pt
    w, h = 11, 9; D = (22, 18)
    sc, cam = scenes.stable_planes_zoo()
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), scenes.config_settings("C2"), w, h)
    readers = (t.upscaled, t.upscaled_size, t.upscaled_device_buffer, t.tonemap_upscaled, t.average_luminance_upscaled, t.bloom_upscaled, t.upscaled_bloomed)
    assert _code(lambda: t.taa_upscale(_params(), D)) == pt.PT_ERROR_NOT_READY                    # no build pass yet
    for r in readers: assert _code(r) == pt.PT_ERROR_NOT_READY
    _new_frame(t, w, h)
    for r in readers: assert _code(r) == pt.PT_ERROR_NOT_READY                                    # a build pass, but nothing upscaled
    nan, inf = np.nan, np.inf
    bad = [dict(newFrameWeight=0.0), dict(newFrameWeight=-0.5), dict(newFrameWeight=1.5), dict(newFrameWeight=nan), dict(maxRadiance=0.0), dict(maxRadiance=-1.0),
           dict(maxRadiance=nan), dict(maxRadiance=inf), dict(clampingFactor=-1.0), dict(clampingFactor=nan), dict(clampingFactor=inf),
           dict(kernelRadius=0.99), dict(kernelRadius=2.01), dict(kernelRadius=0.0), dict(kernelRadius=-1.0), dict(kernelRadius=nan), dict(kernelRadius=inf), dict(kernelRadius=-inf)]
    for kw in bad: assert _code(lambda: t.taa_upscale(_params(**kw), D)) == pt.PT_ERROR_INVALID_ARGUMENT, kw
    for d in ((w - 1, h), (w, h - 1), (4 * w + 1, h), (w, 4 * h + 1), (0, 0), (0, h), (w, 0), (2 ** 32 - 1, 2 ** 32 - 1), (4 * w + 1, 4 * h + 1)):
        assert _code(lambda: t.taa_upscale(_params(), d)) == pt.PT_ERROR_INVALID_ARGUMENT, d
    for j in ((0.51, 0.0), (0.0, -0.51), (nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, -inf), (0.50000006, 0.0), (1e30, -1e30)):
        assert _code(lambda: t.taa_upscale(_params(), D, j)) == pt.PT_ERROR_INVALID_ARGUMENT, j
    for r in readers: assert _code(r) == pt.PT_ERROR_NOT_READY                                    # (a refused call upscales nothing)
    # the ends of the ranges are inside
    for d, j, kw in (((w, h), (0.5, -0.5), dict(kernelRadius=1.0, newFrameWeight=1.0, clampingFactor=0.0)), ((4 * w, 4 * h), (-0.5, 0.5), dict(kernelRadius=2.0)), ((w, 4 * h), (0.0, 0.0), {}), ((4 * w, h), (0.0, 0.0), {})):
        out = t.taa_upscale(_params(**kw), d, j); assert out.shape == (d[1], d[0], 4) and t.upscaled_size() == d
    first = t.taa_upscale(_params(), D, reset_history=True)
    for kw in bad[:3]: assert _code(lambda: t.taa_upscale(_params(**kw), D)) == pt.PT_ERROR_INVALID_ARGUMENT
    assert _code(lambda: t.taa_upscale(_params(), (w - 1, h))) == pt.PT_ERROR_INVALID_ARGUMENT
    assert _eq(t.upscaled(), first) and t.upscaled_size() == D                                    # a refused call changes nothing
    L, P = t.L, _params(); vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    f = L.pt_taa_upscale; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
    assert f(t.h, None, D[0], D[1], None, 0, None) == pt.PT_ERROR_INVALID_ARGUMENT and f(None, vp(P), D[0], D[1], None, 0, None) == pt.PT_ERROR_INVALID_ARGUMENT
    N = D[0] * D[1]
    out = np.zeros((D[1], D[0], 4), f32); o8 = np.zeros((D[1], D[0], 4), np.uint8); tm = pt.default_tonemap(); v = ctypes.c_float(); bp = pt.bloom_default_params()
    for name in ("pt_get_upscaled", "pt_get_upscaled_bloomed"):
        if name.endswith("bloomed"): t.bloom_upscaled()
        g = getattr(L, name); g.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]; g.restype = ctypes.c_int32
        assert g(t.h, None, 4 * N) == pt.PT_ERROR_INVALID_ARGUMENT and g(None, vp(out), 4 * N) == pt.PT_ERROR_INVALID_ARGUMENT
        assert g(t.h, vp(out), 4 * N - 1) == pt.PT_ERROR_INVALID_ARGUMENT and g(t.h, vp(out), 0) == pt.PT_ERROR_INVALID_ARGUMENT and g(t.h, vp(out), 4 * N) == pt.PT_OK
    s = L.pt_upscaled_size; s.argtypes = [ctypes.c_void_p] * 3; s.restype = ctypes.c_int32
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert s(t.h, None, ctypes.byref(b)) == pt.PT_ERROR_INVALID_ARGUMENT and s(t.h, ctypes.byref(a), None) == pt.PT_ERROR_INVALID_ARGUMENT and s(None, ctypes.byref(a), ctypes.byref(b)) == pt.PT_ERROR_INVALID_ARGUMENT
    d = L.pt_upscaled_device_buffer; d.argtypes = [ctypes.c_void_p] * 3; d.restype = ctypes.c_int32
    ptr = ctypes.c_void_p()
    assert d(t.h, None, None) == pt.PT_ERROR_INVALID_ARGUMENT and d(None, ctypes.byref(ptr), None) == pt.PT_ERROR_INVALID_ARGUMENT and d(t.h, ctypes.byref(ptr), None) == pt.PT_OK and ptr.value
    m = L.pt_tonemap_upscaled; m.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]; m.restype = ctypes.c_int32
    assert m(t.h, None, 0, vp(o8), o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT and m(t.h, vp(tm), 0, None, o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT
    assert m(None, vp(tm), 0, vp(o8), o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT and m(t.h, vp(tm), 0, vp(o8), o8.nbytes - 1) == pt.PT_ERROR_INVALID_ARGUMENT
    assert m(t.h, vp(tm), 2, vp(o8), o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT and m(t.h, vp(tm), 0, vp(o8), o8.nbytes) == pt.PT_OK and m(t.h, vp(tm), 1, vp(o8), o8.nbytes) == pt.PT_OK
    al = L.pt_average_luminance_upscaled; al.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; al.restype = ctypes.c_int32
    assert al(t.h, 0, None) == pt.PT_ERROR_INVALID_ARGUMENT and al(None, 0, ctypes.byref(v)) == pt.PT_ERROR_INVALID_ARGUMENT and al(t.h, 2, ctypes.byref(v)) == pt.PT_ERROR_INVALID_ARGUMENT
    assert al(t.h, 0, ctypes.byref(v)) == pt.PT_OK and al(t.h, 1, ctypes.byref(v)) == pt.PT_OK
    bu = L.pt_bloom_upscaled; bu.argtypes = [ctypes.c_void_p] * 3; bu.restype = ctypes.c_int32
    assert bu(t.h, None, None) == pt.PT_ERROR_INVALID_ARGUMENT and bu(None, vp(bp), None) == pt.PT_ERROR_INVALID_ARGUMENT
    for kw in (dict(radius=65.0), dict(radius=nan), dict(intensity=1.5), dict(intensity=nan), dict(maxRadiance=0.0), dict(maxRadiance=inf)):
        assert _code(lambda: t.bloom_upscaled(pt.bloom_default_params(**kw))) == pt.PT_ERROR_INVALID_ARGUMENT, kw
    assert _code(lambda: t.bloom(source=2)) == pt.PT_ERROR_INVALID_ARGUMENT                       # pt_bloom's third source stays refused
    p = L.pt_taa_upscale_default_params; p.argtypes = [ctypes.c_void_p]; p.restype = ctypes.c_int32
    assert p(None) == pt.PT_ERROR_INVALID_ARGUMENT
    lb = L.pt_upscale_tex_lod_bias; lb.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_void_p]; lb.restype = ctypes.c_int32
    assert lb(w, h, D[0], D[1], None) == pt.PT_ERROR_INVALID_ARGUMENT
    t.close()


def test_sixteen_jittered_upscaled_frames_are_nearer_to_the_converged_picture_than_one_enlarged_frame():
    """A small bistro-like scene, static camera, traced at 64 x 48 for a 128 x 96 display: the texture LOD bias plus pt_upscale_tex_lod_bias, one centre sample per pixel
    (perPixelJitterAAScale 0), sixteen R2-jittered realtime frames through the denoiser into pt_taa_upscale. Reference: 64 accumulated samples of pt_render at 128 x 96 with
    perPixelJitterAAScale 1. An inequality, not a threshold; also printed, not asserted: the same sixteen frames through pt_taa_resolve at 64 x 48, enlarged bilinearly
    (docs/WIDENING.md N8 quotes a run)."""
    import rtxpt_amd as pt
    w, h, frames = 64, 48, 16; D = (128, 96)
    sc, cam = scenes.bistro_like(scale=0.02, tex_size=128)
    g = dni._tracer(sc, scenes.bridge_camera(D[0], D[1], **cam), scenes.default_settings(perPixelJitterAAScale=1.0), D[0], D[1])
    g.render(0, 64); converged = g.radiance(); g.close()
    base = scenes.default_settings()
    S_rt = scenes.default_settings(perPixelJitterAAScale=0.0, texLODBias=float(base["texLODBias"]) + float(pt.upscale_tex_lod_bias(w, h, D[0], D[1])))
    assert float(S_rt["texLODBias"]) == float(base["texLODBias"]) - 1.0
    clip = scenes.view_projection(w, h, **cam)
    S = gz._settings()

    def tracer(): return dni._tracer(sc, scenes.bridge_camera(w, h, **cam), S_rt, w, h)

    def frame(t, i, jitter):
        camd = scenes.bridge_camera(w, h, jitter=jitter, **cam); t.set_camera(camd)
        prm = scenes.stable_planes_params(w, h, clip)
        off = clip.copy(); off[:, 0] += f32(2 * jitter[0] / w) * clip[:, 3]; off[:, 1] += f32(-2 * jitter[1] / h) * clip[:, 3]
        prm["matWorldToClip"] = off.reshape(16)                              # the view-projection with the jitter offset; the NoOffset matrices make the motion vectors
        t.realtime_frame(i, prm); t.denoise_spec_hit_t()
        return t.denoise_frame(prm, dni._dn(camd, w, h), S, reset_history=i == 0)

    t = tracer()
    single = _rms(taau.bilinear(frame(t, 0, (0.0, 0.0)), D), converged)
    t.close()
    t = tracer()
    for i in range(frames):
        j = pt.taa_jitter(pt.TAA_JITTER_R2, i)
        frame(t, i, j)
        up = t.taa_upscale(_params(), D, j)
        resolved = t.taa_resolve(gtaa._params())
    sixteen, at_render_size = _rms(up, converged), _rms(taau.bilinear(resolved, D), converged)
    print("TAAU usefulness: RMS to the 64-sample 128 x 96 render: one unjittered 64 x 48 frame enlarged %.6g, sixteen resolved 64 x 48 frames enlarged %.6g, the 16th upscaled frame %.6g"
          % (single, at_render_size, sixteen))
    assert np.all(np.isfinite(up)) and sixteen < single, (sixteen, single)
    t.close()

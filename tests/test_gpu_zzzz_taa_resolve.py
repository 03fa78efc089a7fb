"""The temporal anti-aliasing resolve on the device (run with -m gpu): pt_taa_resolve against the numpy restatement (tests/taa_ref.py) bit for bit, the resolved buffer after
every call — the worked sequences of tests/test_taa_resolve.py at 11 x 9, 13 x 7 and 35 x 10 (colour through pt_unpack_shard on a world of one or through merged field frames,
motion through pt_unpack_stable_planes), rendered zoo frames behind pt_denoise_frame (fractional motion into the pass's own history, a relax buffer that is not zero), the
two moving-camera realtime frames — then what the call must leave alone (the radiance buffer), pt_tonemap_resolved, the history drops, a two-rank sharded frame, the refusals,
and one usefulness check: sixteen jittered, resolved realtime frames are nearer to a converged anti-aliased render than one unjittered frame is."""
import ctypes, itertools, os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoiser_inputs_ref as ref
import taa_ref as taa
import stable_planes_cases as spc
import realtime_cases as rc
import test_denoiser_inputs as cpu
import test_relax_denoiser as cpu_rx
import test_taa_resolve as cpu_taa
import test_gpu_zzz_denoiser_inputs as dni
import test_gpu_zzz_relax_denoiser as gz
from rtxpt_amd import scenes

pytestmark = pytest.mark.gpu
_eq, _diff = dni._eq, dni._diff
f32 = np.float32
image, flat, motion, ramp, PLAIN, FLAGS = cpu_taa.image, cpu_taa.flat, cpu_taa.motion, cpu_taa.ramp, cpu_taa.PLAIN, cpu_taa.FLAGS


def _params(**kw):
    import rtxpt_amd as pt
    return pt.taa_default_params(**kw)


def _code(call):
    import rtxpt_amd as pt
    with pytest.raises(pt.PtError) as e: call()
    return e.value.code


def _new_frame(t, w, h):
    """a build pass: the next frame (the planes it leaves are replaced by what the test pushes)"""
    t.build_stable_planes(0, scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **scenes.stable_planes_zoo()[1])))


def _push_motion(t, mv, w, h):
    """motion vectors [h, w, 2] into the build pass's buffer through pt_unpack_stable_planes; returns them as the device holds them (binary16 -> float32)"""
    fr = ref.make_frame(w, h); fr["motion_vectors"][..., :2] = ref.f32_to_half(np.asarray(mv, f32))
    dni._push(t, fr, w, h)
    back = t.get_stable_planes()["motion_vectors"]; assert np.array_equal(back, fr["motion_vectors"])
    return ref.half_to_f32(back)[..., :2]


def _push_colour(t, colour, w, h):
    """[h, w, 4] into the radiance buffer through pt_unpack_shard (rank 0 of a world of one: the pixels in pt_shard_layout order)"""
    import rtxpt_amd as pt, torch
    px = pt.shard_layout(w, h, 0, 1); xs, ys = px >> 16, px & 0xFFFF
    b = torch.from_numpy(np.ascontiguousarray(np.asarray(colour, f32)[ys, xs])).to("cuda")
    t.unpack_shard(b.data_ptr(), b.numel() * 4, 0)
    assert _eq(t.radiance(), colour)


def _run(t, w, h, kw, frames, tag, hist=None):
    """frames: [(colour [h, w, 4], motion [h, w, 2], calls)]: each frame's inputs go in once and are resolved `calls` times, the restatement alongside; the first call of a
    sequence resets. Returns the restatement's last result."""
    P = _params(**kw)
    for f, (colour, mv, calls) in enumerate(frames):
        held = _push_motion(t, mv, w, h); _push_colour(t, colour, w, h)
        for k in range(calls):
            got = t.taa_resolve(P, reset_history=hist is None)
            hist = taa.resolve(colour, held, None, hist, P)
            assert _eq(got, hist), "%s frame %d call %d: differs in %d values" % (tag, f, k, _diff(got, hist))
    return hist


def _const_mv(w, h, v): return motion(w, h, lambda x, y: v)


def worked_sequences(w, h):
    """(name, parameter keywords, frames) — the sequences tests/test_taa_resolve.py works by hand"""
    z = motion(w, h); seq = []
    dirty = image(w, h, lambda x, y: (0.25 * x, 0.5 * y, 1.0))
    dirty[1, 2, :3] = (np.nan, np.inf, -np.inf); dirty[2, 3, :3] = (-1.0, 20000.0, -0.0); dirty[h - 1, w - 1, :3] = (3e38, 0.5, 10000.0)
    seq.append(("sanitise", {}, [(dirty, _const_mv(w, h, (3, -2)), 1), (dirty, _const_mv(w, h, (np.nan, 0)), 1), (dirty, z, 1)]))
    seq.append(("sanitise_max_half", dict(maxRadiance=0.5), [(dirty, z, 2)]))
    for combo in itertools.product((0, 1), repeat=4):
        seq.append(("flat_%d%d%d%d" % combo, dict(zip(FLAGS, combo)), [(flat(w, h, 0.5), z, 8)]))
    seq.append(("step", dict(newFrameWeight=0.5, **PLAIN), [(flat(w, h, 0.25), z, 1), (flat(w, h, 0.75), z, 2)]))
    pattern = image(w, h, lambda x, y: float((3 * x + 5 * y) % 7)); black = flat(w, h, 0.0)
    for cm in (1, 0):
        for mv in ((3, 0), (0.5, 0), (0.75, 0), (0, -2), (-4, 3)):
            seq.append(("motion_%g_%g_cr%d" % (mv + (cm,)), dict(newFrameWeight=0.5, useCatmullRomFilter=cm, **PLAIN), [(pattern, z, 1), (black, _const_mv(w, h, mv), 1)]))
    one = lambda at, v: motion(w, h, lambda x, y: v if (x, y) == at else (0, 0))
    tie = {(3, 2): (1, 0), (5, 2): (0, 1), (4, 4): (-1, 0)}
    dil = [one((4, 3), (2, 0)), motion(w, h, lambda x, y: tie.get((x, y), (0, 0))), one((1, 1), (1, 1)), one((w - 1, h - 1), (-1, -1)), one((w - 2, 0), (0.5, 0.25))]
    if w > 32: dil.append(one((32, 8), (-2, 0)))      # reaches (31, 7), which another block resolves
    seq.append(("dilation", dict(newFrameWeight=0.5, **PLAIN), [(pattern, z, 1)] + [(black, m, 1) for m in dil]))
    for cm in (1, 0):
        for mv in ((0.5, 0.0), (0.25, -0.5), (-0.75, 0.5), (1.0, -1.0)):
            moved = image(w, h, lambda x, y: ramp(x + mv[0], y + mv[1]))
            seq.append(("ramp_%g_%g_cr%d" % (mv + (cm,)), dict(useCatmullRomFilter=cm), [(image(w, h, ramp), z, 1), (moved, _const_mv(w, h, mv), 1)]))
    for name, kw in (("ghost", {}), ("ghost_plain_weight", dict(luminanceWeighted=0)), ("ghost_kept", PLAIN)):
        seq.append((name, kw, [(flat(w, h, 1.0), z, 1), (black, z, 1)]))
    thirds = image(w, h, lambda x, y: float((x + 2 * y) % 3))
    for name, kw in (("box", {}), ("box_no_relax", dict(useHistoryClampRelax=0)), ("box_factor_0", dict(clampingFactor=0.0)), ("box_factor_2", dict(clampingFactor=2.0))):
        seq.append((name, kw, [(flat(w, h, 64.0), z, 1), (thirds, z, 1)]))
    seq.append(("box_from_below", {}, [(black, z, 1), (thirds + f32(8), z, 1)]))
    seq.append(("luminance_weight", dict(newFrameWeight=0.5, enableHistoryClamping=0), [(flat(w, h, 1.0), z, 1), (flat(w, h, 3.0), z, 1)]))
    rng = np.random.default_rng(5)
    noise = lambda: np.concatenate([rng.uniform(0.25, 4.0, (h, w, 3)).astype(f32), np.ones((h, w, 1), f32)], -1)
    seq.append(("random_exponential", dict(newFrameWeight=0.25, **PLAIN), [(noise(), _const_mv(w, h, (1, 0)), 1) for _ in range(12)]))
    wander = lambda: rng.choice(np.array([-1.5, -0.75, -0.25, 0, 0.5, 1.25], f32), (h, w, 2))
    for cm in (1, 0):
        seq.append(("random_defaults_cr%d" % cm, dict(useCatmullRomFilter=cm), [(noise(), wander(), 1) for _ in range(4)]))
    return seq


@pytest.mark.parametrize("w,h", cpu_taa.SIZES)
def test_worked_sequences_equal_the_restatement(w, h):
    t, _, _ = gz._pushed_tracer(w, h)
    for name, kw, frames in worked_sequences(w, h):
        out = _run(t, w, h, kw, frames, name)
        if name == "step": assert np.all(out[..., :3] == f32(0.625))
        if name == "ghost": assert np.all(out[..., :3] == 0)
        if name == "ghost_kept": assert np.all(out[..., :3] == f32(1) - f32(0.1))
        if name.startswith("flat_"): assert np.all(out[..., :3] == f32(0.5))
        assert np.all(out[..., 3] == 1)
    t.close()


@pytest.mark.parametrize("w,h", cpu_taa.SIZES)
def test_merged_field_frames_equal_the_restatement(w, h):
    """the colour as the realtime path leaves it: field frames through prepare / denoise / merge (each held to its own restatement on the way), the relax buffer as the
    prepare pass left it, motion in the build pass's buffer"""
    t, camd, cfg = gz._pushed_tracer(w, h)
    prm, dn = cpu._params(active=1, w=w, h=h)
    mvs = [(0, 0), (0.5, -0.25), (2, 1)]
    hist_dn, st, hist = {}, None, None
    for f, (rad, mv) in enumerate(zip((lambda x, y: float(2 ** (x % 3)), lambda x, y: float(2 ** ((x + y) % 3)), 0.5), mvs)):
        frame = cpu_rx.field_frame(w, h, radiance=rad)
        frame["motion_vectors"][..., :2] = ref.f32_to_half(_const_mv(w, h, mv))
        dni._push(t, frame, w, h)
        st = gz._sequence(t, frame, prm, dn, camd, cfg, gz._settings(), w, h, 0, hist_dn, "field frame %d" % f, state=st, reset=f == 0)
        before = t.radiance()
        got = t.taa_resolve(_params(), reset_history=f == 0)
        hist = taa.resolve(st["output_color"], ref.half_to_f32(frame["motion_vectors"])[..., :2], st["nrd_combined_history_clamp_relax"], hist, taa.params())
        assert _eq(got, hist), "frame %d: differs in %d values" % (f, _diff(got, hist))
        assert _eq(t.radiance(), before)
    t.close()


def _device_inputs(t):
    """what pt_taa_resolve reads, as the device holds it after pt_denoise_frame: (colour, motion as float32, relax)"""
    return t.radiance(), ref.half_to_f32(t.get_stable_planes()["motion_vectors"])[..., :2], t.get_denoiser_inputs(("nrd_combined_history_clamp_relax",))["nrd_combined_history_clamp_relax"]


@pytest.mark.parametrize("name", ["zoo_fp32", "zoo_two_planes_no_psr"])
def test_zoo_frames_equal_the_restatement(name):
    """a rendered frame behind pt_denoise_frame, resolved twice: the second call reprojects through the frame's fractional motion vectors into the first call's result and
    clamps with a relax buffer that is not zero; the radiance buffer stays byte-identical, the two buffers swap, the timed call computes the same"""
    t, frame, camd, cfg, prm = dni._zoo_frame(name)
    w, h = spc.W, spc.H
    t.denoise_frame(prm, dni._dn(camd, w, h), gz._settings())
    colour, mv, relax = _device_inputs(t)
    assert relax.max() > 0 and np.any(mv != np.floor(mv)) and np.all(colour[..., 3] == 1)
    a = t.taa_resolve(_params()); pa, pitch = t.resolved_device_buffer(); assert pa and pitch == 16 * w
    want_a = taa.resolve(colour, mv, relax, None, taa.params()); assert _eq(a, want_a), _diff(a, want_a)
    b, ms = t.taa_resolve(_params(), timed=True); pb, _ = t.resolved_device_buffer(); assert pb and pb != pa and ms > 0
    want_b = taa.resolve(colour, mv, relax, want_a, taa.params()); assert _eq(b, want_b), _diff(b, want_b)
    assert not _eq(want_b, taa.resolve(colour, mv, relax, want_a, taa.params(useHistoryClampRelax=0)))      # (the relax buffer is really read)
    c = t.taa_resolve(_params(useHistoryClampRelax=0, useCatmullRomFilter=0)); assert t.resolved_device_buffer()[0] == pa
    want_c = taa.resolve(colour, mv, relax, want_b, taa.params(useHistoryClampRelax=0, useCatmullRomFilter=0)); assert _eq(c, want_c), _diff(c, want_c)
    assert _eq(t.radiance(), colour)
    t.close()


def test_a_relax_buffer_of_an_older_build_pass_reads_as_zero():
    """after the next build pass and before any NRD prepare of it, the relax buffer still holds the last frame's bytes: the resolve must not read them"""
    t, frame, camd, cfg, prm = dni._zoo_frame("zoo_fp32")
    w, h = spc.W, spc.H
    t.denoise_frame(prm, dni._dn(camd, w, h), gz._settings())
    first = t.taa_resolve(_params())
    t.build_stable_planes(spc.SAMPLE, prm)
    colour, mv, relax = _device_inputs(t); assert relax.max() > 0
    got = t.taa_resolve(_params())
    want = taa.resolve(colour, mv, None, first, taa.params())
    assert _eq(got, want), _diff(got, want)
    assert not _eq(want, taa.resolve(colour, mv, relax, first, taa.params()))
    t.denoiser_prepare_nrd(prm, dni._dn(camd, w, h), 2, True)               # a prepare of this build pass: the buffer counts again (this call cleared it and added plane 2's)
    colour, mv, relax = _device_inputs(t)
    got = t.taa_resolve(_params()); again = taa.resolve(colour, mv, relax, want, taa.params())
    assert _eq(got, again), _diff(got, again)
    t.close()


def test_moving_camera_frames_carry_their_history():
    make, cfg, w, h, frames, subs, step, kw = rc.cases()["zoo_realtime"]
    sc, cam = make()
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), cfg, w, h)
    hist = None
    for f in range(2):
        cur, prev = rc.camera(cam, step, f), rc.camera(cam, step, max(f - 1, 0))
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cur), prev_world_to_clip=scenes.view_projection(w, h, **prev), sub_samples=subs, **kw)
        camd = scenes.bridge_camera(w, h, **cur); t.set_camera(camd)
        t.realtime_frame(f * subs, prm); t.denoise_spec_hit_t()
        t.denoise_frame(prm, dni._dn(camd, w, h), gz._settings())
        colour, mv, relax = _device_inputs(t)
        got = t.taa_resolve(_params())
        st = {}
        hist = taa.resolve(colour, mv, relax, hist, taa.params(), stages=st)
        assert _eq(got, hist), "frame %d: differs in %d values" % (f, _diff(got, hist))
    assert np.any(mv != 0) and st["valid"].any() and not _eq(hist[..., :3], st["colour"])      # the second frame did blend with the first
    t.close()


def test_tonemap_resolved():
    import rtxpt_amd as pt
    from oracle import ptref
    t, frame, camd, cfg, prm = dni._zoo_frame("zoo_fp32")
    w, h = spc.W, spc.H
    t.denoise_frame(prm, dni._dn(camd, w, h), gz._settings())
    rad = t.radiance(); assert np.all(np.isfinite(rad)) and rad[..., :3].min() >= 0 and rad[..., :3].max() < 10000 and rad[..., :3].max() > 0
    tms = [pt.default_tonemap(), pt.default_tonemap(exposure_compensation=-2.0, toneMapOperator="reinhard"), pt.default_tonemap(autoExposure=1, avgLuminance=0.3)]
    assert _code(lambda: t.tonemap_resolved()) == pt.PT_ERROR_NOT_READY
    first = t.taa_resolve(_params(), reset_history=True)                              # finite and in range: the reset frame is the input
    assert _eq(first, taa.resolve(rad, None, None, None, taa.params())) and np.array_equal(first, rad)
    for tm in tms: assert np.array_equal(t.tonemap_resolved(tm), t.tonemap(tm))
    second = t.taa_resolve(_params()); assert not _eq(second, rad)
    for tm in tms:
        got = t.tonemap_resolved(tm)
        assert got.shape == (h, w, 4) and np.array_equal(got, ptref.tonemap(t.get_resolved(), tm))
    assert not np.array_equal(t.tonemap_resolved(), t.tonemap())
    t.close()


def test_history_drops_behave_as_a_reset():
    """a resize to another size, pt_set_geometry, and a build pass that was not resolved; and, as the control, the next build pass keeps the history"""
    import rtxpt_amd as pt
    w, h = 13, 7
    t, _, _ = gz._pushed_tracer(w, h)
    P = _params(newFrameWeight=0.5, **PLAIN)
    a, b, z = flat(w, h, 0.25), flat(w, h, 0.75), motion(w, h)
    fresh, blended = flat(w, h, 0.75), flat(w, h, 0.5); fresh[..., 3] = 1; blended[..., 3] = 1

    def two_frames(between):
        _new_frame(t, w, h); _push_motion(t, z, w, h); _push_colour(t, a, w, h); t.taa_resolve(P, reset_history=True)
        between()
        _push_motion(t, z, w, h); _push_colour(t, b, w, h)
        return t.taa_resolve(P)

    assert _eq(two_frames(lambda: _new_frame(t, w, h)), blended)                                  # the control: consecutive build passes
    assert _eq(two_frames(lambda: None), blended)                                                 # a second call on one frame
    assert _eq(two_frames(lambda: (_new_frame(t, w, h), _new_frame(t, w, h))), fresh)             # a build pass was skipped
    sc, _ = scenes.stable_planes_zoo()
    assert _eq(two_frames(lambda: (t.set_scene(sc), _new_frame(t, w, h))), fresh)                 # pt_set_geometry
    def resized():
        t.resize(w + 3, h + 2)
        assert _code(lambda: t.taa_resolve(P)) == pt.PT_ERROR_NOT_READY and _code(lambda: t.get_resolved()) == pt.PT_ERROR_NOT_READY
        assert _code(lambda: t.resolved_device_buffer()) == pt.PT_ERROR_NOT_READY
        t.resize(w, h); _new_frame(t, w, h)
    assert _eq(two_frames(resized), fresh)
    t.resize(w, h); _new_frame(t, w, h); _push_motion(t, z, w, h); _push_colour(t, a, w, h)       # pt_resize to the same size keeps it: 0.75 + (0.25 - 0.75) x 0.5
    assert _eq(t.taa_resolve(P), blended)
    t.close()


def test_tile_sharded_frame_equals_the_unsharded_one():
    import rtxpt_amd as pt, torch
    sc, camd, cfg, prm, _ = spc.setup("zoo_fp32"); w, h = spc.W, spc.H
    dn = dni._dn(camd, w, h); S = gz._settings()
    ranks = [dni._tracer(sc, camd, cfg, w, h, shard_rank=r, shard_count=2) for r in range(2)]
    for t in ranks: t.build_stable_planes(spc.SAMPLE, prm); t.fill_stable_planes(spc.SAMPLE, prm, sub_samples=spc.SUBSAMPLES)
    assert _code(lambda: ranks[0].taa_resolve(_params())) == pt.PT_ERROR_NOT_READY                # the planes of the other rank have not arrived
    n = ranks[1].stable_planes_shard_bytes(1); b = torch.empty(n // 4, dtype=torch.int32, device="cuda"); ranks[1].pack_stable_planes(b.data_ptr(), n)
    ranks[0].unpack_stable_planes(b.data_ptr(), n, 1); ranks[0].denoise_spec_hit_t()
    u, _, _, _, _ = dni._zoo_frame("zoo_fp32")
    outs = []
    for t in (ranks[0], u):
        t.denoise_frame(prm, dn, S)
        outs.append([t.taa_resolve(_params()), t.taa_resolve(_params())])
    for x, y in zip(*outs): assert _eq(x, y)
    assert not _eq(outs[1][0], outs[1][1])
    for t in ranks + [u]: t.close()


def test_refusals():
    import rtxpt_amd as pt
    w, h = 11, 9
    sc, cam = scenes.stable_planes_zoo()
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), scenes.config_settings("C2"), w, h)
    assert _code(lambda: t.taa_resolve(_params())) == pt.PT_ERROR_NOT_READY                       # no build pass yet
    assert _code(lambda: t.get_resolved()) == pt.PT_ERROR_NOT_READY and _code(lambda: t.resolved_device_buffer()) == pt.PT_ERROR_NOT_READY
    _new_frame(t, w, h)
    assert _code(lambda: t.get_resolved()) == pt.PT_ERROR_NOT_READY                               # a build pass, but nothing resolved
    bad = [dict(newFrameWeight=0.0), dict(newFrameWeight=-0.5), dict(newFrameWeight=1.5), dict(newFrameWeight=np.nan), dict(maxRadiance=0.0), dict(maxRadiance=-1.0),
           dict(maxRadiance=np.nan), dict(maxRadiance=np.inf), dict(clampingFactor=-1.0), dict(clampingFactor=np.nan), dict(clampingFactor=np.inf)]
    for kw in bad: assert _code(lambda: t.taa_resolve(_params(**kw))) == pt.PT_ERROR_INVALID_ARGUMENT, kw
    assert _code(lambda: t.get_resolved()) == pt.PT_ERROR_NOT_READY                               # (a refused call resolves nothing)
    L, P = t.L, _params()
    f = L.pt_taa_resolve; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]; f.restype = ctypes.c_int32
    assert f(t.h, None, 0, None) == pt.PT_ERROR_INVALID_ARGUMENT and f(None, P.ctypes.data_as(ctypes.c_void_p), 0, None) == pt.PT_ERROR_INVALID_ARGUMENT
    t.taa_resolve(_params(newFrameWeight=1.0, clampingFactor=0.0))                                # the ends of the ranges are inside
    out = np.zeros((h, w, 4), f32); o8 = np.zeros((h, w, 4), np.uint8); tm = pt.default_tonemap()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    g = L.pt_get_resolved; g.argtypes = [ctypes.c_void_p] * 2; g.restype = ctypes.c_int32
    assert g(t.h, None) == pt.PT_ERROR_INVALID_ARGUMENT and g(None, vp(out)) == pt.PT_ERROR_INVALID_ARGUMENT and g(t.h, vp(out)) == pt.PT_OK
    d = L.pt_resolved_device_buffer; d.argtypes = [ctypes.c_void_p] * 3; d.restype = ctypes.c_int32
    ptr = ctypes.c_void_p()
    assert d(t.h, None, None) == pt.PT_ERROR_INVALID_ARGUMENT and d(None, ctypes.byref(ptr), None) == pt.PT_ERROR_INVALID_ARGUMENT and d(t.h, ctypes.byref(ptr), None) == pt.PT_OK and ptr.value
    m = L.pt_tonemap_resolved; m.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t]; m.restype = ctypes.c_int32
    assert m(t.h, None, vp(o8), o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT and m(t.h, vp(tm), None, o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT
    assert m(None, vp(tm), vp(o8), o8.nbytes) == pt.PT_ERROR_INVALID_ARGUMENT and m(t.h, vp(tm), vp(o8), o8.nbytes - 1) == pt.PT_ERROR_INVALID_ARGUMENT
    assert m(t.h, vp(tm), vp(o8), o8.nbytes) == pt.PT_OK
    j = L.pt_taa_jitter; j.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]; j.restype = ctypes.c_int32
    assert j(1, 0, None) == pt.PT_ERROR_INVALID_ARGUMENT
    p = L.pt_taa_default_params; p.argtypes = [ctypes.c_void_p]; p.restype = ctypes.c_int32
    assert p(None) == pt.PT_ERROR_INVALID_ARGUMENT
    t.close()


def _rms(a, b): return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


def test_sixteen_jittered_resolved_frames_are_nearer_to_the_converged_picture_than_one_unjittered_frame():
    """A small bistro-like scene, 64 x 48, static camera; realtime frames with one centre sample per pixel (perPixelJitterAAScale 0: the camera jitter is the only sub-pixel
    offset, as in the reference's realtime mode). Reference: 64 accumulated samples of pt_render with perPixelJitterAAScale 1. An inequality, not a threshold; both figures
    are printed (docs/WIDENING.md N6 quotes a run)."""
    import rtxpt_amd as pt
    w, h, frames = 64, 48, 16
    sc, cam = scenes.bistro_like(scale=0.02, tex_size=128)
    g = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), scenes.default_settings(perPixelJitterAAScale=1.0), w, h)
    g.render(0, 64); converged = g.radiance(); g.close()
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), scenes.default_settings(perPixelJitterAAScale=0.0), w, h)
    clip = scenes.view_projection(w, h, **cam)
    S = gz._settings()

    def frame(i, jitter):
        camd = scenes.bridge_camera(w, h, jitter=jitter, **cam); t.set_camera(camd)
        prm = scenes.stable_planes_params(w, h, clip)
        off = clip.copy(); off[:, 0] += f32(2 * jitter[0] / w) * clip[:, 3]; off[:, 1] += f32(-2 * jitter[1] / h) * clip[:, 3]
        prm["matWorldToClip"] = off.reshape(16)                              # the view-projection with the jitter offset; the NoOffset matrices make the motion vectors
        t.realtime_frame(i, prm); t.denoise_spec_hit_t()
        return t.denoise_frame(prm, dni._dn(camd, w, h), S, reset_history=i == 0)

    single = _rms(frame(0, (0.0, 0.0)), converged)
    t.close()
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), scenes.default_settings(perPixelJitterAAScale=0.0), w, h)
    for i in range(frames):
        frame(i, pt.taa_jitter(pt.TAA_JITTER_R2, i))
        resolved = t.taa_resolve(_params())
    sixteen = _rms(resolved, converged)
    print("TAA usefulness: RMS to the 64-sample render: one unjittered realtime frame %.6g, the 16th jittered resolved frame %.6g" % (single, sixteen))
    assert np.all(np.isfinite(resolved)) and sixteen < single, (sixteen, single)
    t.close()

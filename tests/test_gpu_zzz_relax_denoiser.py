"""The device denoiser on the device (run with -m gpu): pt_denoise_plane / pt_denoise_frame against the numpy restatement (tests/relax_ref.py) bit for bit — both denoised
buffers and the history lengths after every call, and the merged picture — over hand-built frames pushed through pt_unpack_stable_planes, rendered zoo frames, and the two
moving-camera frames of the realtime zoo case with the history carried from frame 0 into frame 1; then pt_denoise_frame against the calls made one by one, a resize between
frames, a two-rank sharded frame, and the refusals."""
import os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoiser_inputs_ref as ref
import relax_ref as rx
import stable_planes_cases as spc
import realtime_cases as rc
import test_denoiser_inputs as cpu
import test_relax_denoiser as cpu_rx
import test_gpu_zzz_denoiser_inputs as dni
from rtxpt_amd import scenes

pytestmark = pytest.mark.gpu
_eq, _diff = dni._eq, dni._diff


def _settings(**kw):
    import rtxpt_amd as pt
    return pt.denoise_default_settings(**kw)


def _check_plane(t, st, prm, S, hist, p, w, h, tag, reset=False):
    """pt_denoise_plane of plane p over the NRD buffers both sides hold, against the restatement; returns the restatement's (diff, spec)"""
    t.denoise_plane(prm, S, p, reset)
    got = t.get_denoised(p)
    d, s, n, hist[p] = rx.denoise_plane(st, S, hist.get(p), w, h, reset)
    for name, a, b in (("diffuse", got[0], d), ("specular", got[1], s), ("history lengths", got[2], n)):
        assert _eq(a, b), "%s plane %d: %s differs in %d values" % (tag, p, name, _diff(a, b))
    return d, s


def _sequence(t, frame, prm, dn, camd, cfg, S, w, h, base, hist, tag, state=None, reset=False):
    """Sample::Denoise's loop, one call at a time, the restatement alongside; returns the restatement's final state"""
    active = int(min(max(int(prm["activeStablePlaneCount"]), 1), 3))
    st = ref.empty_state(w, h) if state is None else state
    for i, p in enumerate(range(active - 1, -1, -1)):
        t.denoiser_prepare_nrd(prm, dn, p, i == 0)
        st = ref.nrd_prepare(st, frame, prm, dn, w, h, p, i == 0, *ref.camera_rays(camd, cfg, w, h, base + p))
        d, s = _check_plane(t, st, prm, S, hist, p, w, h, tag, reset)
        dp, sp, pitch = t.denoised_device_buffers(p); assert dp and sp and pitch == 16 * w
        t.denoiser_merge_nrd(p, dp, sp)
        st["output_color"] = ref.nrd_merge(st, frame, w, h, p, d, s)
        assert _eq(t.radiance(), st["output_color"]), "%s plane %d: merged colour differs in %d values" % (tag, p, _diff(t.radiance(), st["output_color"]))
    return st


def _pushed_tracer(w, h):
    sc, cam = scenes.stable_planes_zoo()
    camd = scenes.bridge_camera(w, h, **cam); cfg = scenes.config_settings("C2")
    t = dni._tracer(sc, camd, cfg, w, h)
    t.build_stable_planes(0, scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam)))
    return t, camd, cfg


def test_hand_frames_equal_the_restatement():
    """test_denoiser_inputs.hand_cases(): three / two / one plane, two frames each (the second with history, motion vectors 0), 11 x 9 and 13 x 7"""
    tracers = {}
    for case in cpu.hand_cases():
        frame, prm, dn, w, h = case["frame"], case["sp"], case["dn"], case["w"], case["h"]
        if (w, h) not in tracers: tracers[(w, h)] = _pushed_tracer(w, h)
        t, camd, cfg = tracers[(w, h)]
        hist, st = {}, None
        for f in range(2):
            dni._push(t, frame, w, h)
            st = _sequence(t, frame, prm, dn, camd, cfg, _settings(), w, h, 0, hist, "%s frame %d" % (case["name"], f), state=st, reset=f == 0)
    for t, _, _ in tracers.values(): t.close()


# the worked fields of tests/test_relax_denoiser.py as frame sequences: (name, settings keywords, [field_frame keywords per frame])
_LEFT = lambda x, y: x < 5
FIELD_SEQUENCES = [
    ("flat_with_sky", {}, [dict(sky=lambda x, y: x == 10)] * 2),
    ("flat_8_iterations", dict(atrousIterationNum=8), [dict(radiance=0.5)]),
    ("flat_2_iterations", dict(atrousIterationNum=2), [dict(radiance=0.5)]),
    ("depth_step", {}, [dict(radiance=lambda x, y: 1.0 if _LEFT(x, y) else 0.0, depth=lambda x, y: 2.0 if _LEFT(x, y) else 4.0)]),
    ("normal_step", {}, [dict(radiance=lambda x, y: 1.0 if _LEFT(x, y) else 0.0, normal=lambda x, y: (0, 0, 1) if _LEFT(x, y) else (1, 0, 0))]),
    ("static_three_frames", {}, [dict(radiance=0.25), dict(radiance=0.5), dict(radiance=1.0)]),
    ("static_cap_2", dict(diffuseMaxAccumulatedFrameNum=2, specularMaxFastAccumulatedFrameNum=1), [dict(radiance=0.25), dict(radiance=0.5), dict(radiance=1.0), dict(radiance=4.0)]),
    ("integer_motion", {}, [dict(radiance=lambda x, y: 1.0 if x == 6 else 0.0), dict(radiance=0.0, mv=(3, 0, 0))]),
    ("fractional_motion", {}, [dict(radiance=lambda x, y: float(2 ** (x % 3))), dict(radiance=1.0, mv=(1.25, -0.5, 0.0))]),
    ("clamp_to_fast", dict(diffuseMaxFastAccumulatedFrameNum=1, specularMaxFastAccumulatedFrameNum=2),
     [dict(radiance=lambda x, y: float(2 ** (x % 3))), dict(radiance=lambda x, y: float(2 ** ((x + 1) % 3))), dict(radiance=lambda x, y: float(2 ** ((x + y) % 3)))]),
    ("disocclusion", {}, [dict(depth=2.0), dict(depth=3.0), dict(depth=3.25)]),
    ("mix_off", dict(useDisocclusionThresholdMix=0), [dict(depth=2.0), dict(depth=2.2)]),
    ("roughness_0", {}, [dict(radiance=lambda x, y: float(2 ** (x % 2)), roughness=0.0)] * 2),      # (the prepare pass floors it at 0.2: the guide carries 0.2)
    ("firefly", {}, [dict(radiance=lambda x, y: 64.0 if (x, y) == (5, 4) else 1.0)]),
    ("firefly_off_no_colour_stop", dict(enableAntiFirefly=0, luminanceSigmaScale=0.0), [dict(radiance=lambda x, y: 64.0 if (x, y) == (5, 4) else float(2 ** ((x + y) % 2)))]),
]


@pytest.mark.parametrize("w,h", cpu_rx.SIZES)
def test_worked_fields_equal_the_restatement(w, h):
    t, camd, cfg = _pushed_tracer(w, h)
    prm, dn = cpu._params(active=1, w=w, h=h)
    for name, skw, frames in FIELD_SEQUENCES:
        hist, st = {}, None
        for f, kw in enumerate(frames):
            frame = cpu_rx.field_frame(w, h, **kw)
            dni._push(t, frame, w, h)
            st = _sequence(t, frame, prm, dn, camd, cfg, _settings(**skw), w, h, 0, hist, "%s frame %d" % (name, f), state=st, reset=f == 0)
            if name == "static_three_frames": assert np.all(t.get_denoised(0)[2] == f + 1)
    t.close()


@pytest.mark.parametrize("name", ["zoo_fp32", "zoo_two_planes_no_psr"])
def test_zoo_frames_equal_the_restatement(name):
    """a rendered frame at its own small size; denoised twice, so the second call reprojects through the frame's (fractional) motion vectors into the first call's history"""
    t, frame, camd, cfg, prm = dni._zoo_frame(name)
    w, h = spc.W, spc.H
    dn = dni._dn(camd, w, h)
    hist, st = {}, None
    for f in range(2): st = _sequence(t, frame, prm, dn, camd, cfg, _settings(), w, h, spc.SAMPLE, hist, "%s call %d" % (name, f), state=st)
    assert any(np.any(t.get_denoised(p)[2] > 1) for p in hist)      # (some history was found)
    t.close()


def test_moving_camera_frames_carry_their_history():
    make, cfg, w, h, frames, subs, step, kw = rc.cases()["zoo_realtime"]
    sc, cam = make()
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), cfg, w, h)
    hist, st = {}, None
    for f in range(2):
        cur, prev = rc.camera(cam, step, f), rc.camera(cam, step, max(f - 1, 0))
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cur), prev_world_to_clip=scenes.view_projection(w, h, **prev), sub_samples=subs, **kw)
        camd = scenes.bridge_camera(w, h, **cur); t.set_camera(camd)
        t.realtime_frame(f * subs, prm); t.denoise_spec_hit_t(); frame = t.get_stable_planes()
        st = _sequence(t, frame, prm, dni._dn(camd, w, h), camd, cfg, _settings(), w, h, f * subs, hist, "frame %d" % f, state=st)
    lengths = t.get_denoised(0)[2]
    assert np.any(lengths == 2) and np.any(lengths == 1)      # history kept where the surface was seen before, dropped where it was not
    t.close()


def test_a_plane_that_sat_out_a_frame_starts_again():
    """three planes, then a frame with two active planes, then three again: plane 2's history would be two frames old, so it is not used; planes 0 and 1 go on accumulating"""
    cases = {c["name"]: c for c in cpu.hand_cases()}
    w, h = cases["three_planes"]["w"], cases["three_planes"]["h"]
    t, camd, cfg = _pushed_tracer(w, h)
    hist, st = {}, None
    for f, name in enumerate(("three_planes", "two_planes", "three_planes")):
        c = cases[name]
        if f: t.build_stable_planes(0, scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **scenes.stable_planes_zoo()[1])))      # a new frame
        dni._push(t, c["frame"], w, h)
        if f == 2: hist.pop(2)      # what the library must do on its own
        st = _sequence(t, c["frame"], c["sp"], c["dn"], camd, cfg, _settings(), w, h, 0, hist, "frame %d (%s)" % (f, name), state=st)
    assert t.get_denoised(2)[2].max() == 1 and t.get_denoised(0)[2].max() == 3
    t.close()


def test_denoise_frame_equals_the_calls_made_one_by_one():
    case = cpu.hand_cases()[0]
    frame, prm, dn, w, h = case["frame"], case["sp"], case["dn"], case["w"], case["h"]
    S = _settings()
    a, camd, cfg = _pushed_tracer(w, h); b, _, _ = _pushed_tracer(w, h)
    for f in range(2):
        for t in (a, b): dni._push(t, frame, w, h)
        for i, p in enumerate((2, 1, 0)):
            a.denoiser_prepare_nrd(prm, dn, p, i == 0); a.denoise_plane(prm, S, p, False); dp, sp, _ = a.denoised_device_buffers(p); a.denoiser_merge_nrd(p, dp, sp)
        whole = b.denoise_frame(prm, dn, S)
        assert _eq(whole, a.radiance()), "frame %d: pt_denoise_frame differs in %d values" % (f, _diff(whole, a.radiance()))
        for p in range(3):
            for x, y in zip(a.get_denoised(p), b.get_denoised(p)): assert _eq(x, y)
    assert np.any(a.radiance()[..., :3] > 0)
    a.close(); b.close()


def test_a_resize_between_frames_behaves_as_a_reset():
    import rtxpt_amd as pt
    case = cpu.hand_cases()[0]
    frame, prm, dn, w, h = case["frame"], case["sp"], case["dn"], case["w"], case["h"]
    t, camd, cfg = _pushed_tracer(w, h)
    hist = {}
    for f in range(2):
        dni._push(t, frame, w, h)
        _sequence(t, frame, prm, dn, camd, cfg, _settings(), w, h, 0, hist, "frame %d" % f)
    assert np.all(t.get_denoised(0)[2][:, :10] == 2)
    t.resize(w + 3, h + 2)
    with pytest.raises(pt.PtError) as e: t.get_denoised(0)
    assert e.value.code == pt.PT_ERROR_NOT_READY
    t.resize(w, h)
    t.build_stable_planes(0, scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **scenes.stable_planes_zoo()[1])))
    dni._push(t, frame, w, h)
    _sequence(t, frame, prm, dn, camd, cfg, _settings(), w, h, 0, {}, "after the resize")      # equals the restatement without any history
    assert np.all(t.get_denoised(0)[2][:, :10] == 1)
    t.close()


def test_tile_sharded_frame_equals_the_unsharded_one():
    import rtxpt_amd as pt, torch
    sc, camd, cfg, prm, _ = spc.setup("zoo_fp32"); w, h = spc.W, spc.H
    dn = dni._dn(camd, w, h); S = _settings()
    ranks = [dni._tracer(sc, camd, cfg, w, h, shard_rank=r, shard_count=2) for r in range(2)]
    for t in ranks: t.build_stable_planes(spc.SAMPLE, prm); t.fill_stable_planes(spc.SAMPLE, prm, sub_samples=spc.SUBSAMPLES)
    with pytest.raises(pt.PtError) as e: ranks[0].denoise_frame(prm, dn, S)
    assert e.value.code == pt.PT_ERROR_NOT_READY
    n = ranks[1].stable_planes_shard_bytes(1); b = torch.empty(n // 4, dtype=torch.int32, device="cuda"); ranks[1].pack_stable_planes(b.data_ptr(), n)
    ranks[0].unpack_stable_planes(b.data_ptr(), n, 1); ranks[0].denoise_spec_hit_t()
    u, frame, _, _, _ = dni._zoo_frame("zoo_fp32")
    outs = []
    for t in (ranks[0], u):
        o = [t.denoise_frame(prm, dn, S)]
        for p in range(3): o.extend(t.get_denoised(p))
        outs.append(o)
    for x, y in zip(*outs): assert _eq(x, y)
    for t in ranks + [u]: t.close()


def test_refusals():
    import rtxpt_amd as pt
    case = cpu.hand_cases()[0]
    frame, prm, dn, w, h = case["frame"], case["sp"], case["dn"], case["w"], case["h"]
    sc, cam = scenes.stable_planes_zoo()
    t = dni._tracer(sc, scenes.bridge_camera(w, h, **cam), scenes.config_settings("C2"), w, h)
    S = _settings()
    def code(call):
        with pytest.raises(pt.PtError) as e: call()
        return e.value.code
    assert code(lambda: t.denoise_plane(prm, S, 0)) == pt.PT_ERROR_NOT_READY                  # no planes at all
    t.build_stable_planes(0, scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam))); dni._push(t, frame, w, h)
    assert code(lambda: t.denoise_plane(prm, S, 3)) == pt.PT_ERROR_INVALID_ARGUMENT
    for n in (0, 1, 9): assert code(lambda: t.denoise_plane(prm, _settings(atrousIterationNum=n), 0)) == pt.PT_ERROR_INVALID_ARGUMENT
    assert code(lambda: t.denoise_frame(prm, dn, _settings(atrousIterationNum=9))) == pt.PT_ERROR_INVALID_ARGUMENT
    assert code(lambda: t.denoise_plane(prm, S, 0)) == pt.PT_ERROR_NOT_READY                  # no prepare on this frame
    assert code(lambda: t.denoised_device_buffers(0)) == pt.PT_ERROR_NOT_READY and code(lambda: t.get_denoised(0)) == pt.PT_ERROR_NOT_READY
    t.denoiser_prepare_nrd(prm, dn, 1, True)
    assert code(lambda: t.denoise_plane(prm, S, 0)) == pt.PT_ERROR_NOT_READY                  # the prepare was of another plane
    t.denoise_plane(prm, S, 1)
    assert code(lambda: t.denoise_plane(prm, S, 1)) == pt.PT_ERROR_NOT_READY                  # one denoise per prepare
    assert code(lambda: t.denoised_device_buffers(3)) == pt.PT_ERROR_INVALID_ARGUMENT
    assert all(t.denoised_device_buffers(1)[:2])
    t.denoiser_prepare_nrd(prm, dn, 0, False)
    t.build_stable_planes(0, scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam)))
    assert code(lambda: t.denoise_plane(prm, S, 0)) == pt.PT_ERROR_NOT_READY                  # a new frame: the prepare was of the last one
    t.close()

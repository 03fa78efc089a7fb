"""The device denoiser (pt_denoise_plane, rtxpt_amd/csrc/pt_relax.h) on the CPU: its numpy restatement (tests/relax_ref.py) held to answers worked by hand on 11 x 9 and 13 x 7
frames (neither a multiple of the 8-pixel addressing tiles nor of the 32 x 8 pass tiles), to a convolution written here with np.convolve only, and the public interface
(include/mi355pt.h declares the entry points, libmi355pt.so exports them). Radiance values are powers of two, so the expected values are exact. The device is held to the
restatement bit for bit in tests/test_gpu_zzz_relax_denoiser.py.

Frames are built with denoiser_inputs_ref's make_frame / put / make_record and go through its nrd_prepare: a record with noisy radiance (2a, 2a, 2a, a) and BSDF estimates 1
comes out as demodulated diffuse = specular = a exactly; identity view and rays along -z make viewZ = -SceneLength."""
import os, re, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoiser_inputs_ref as ref
import relax_ref as rx
import test_denoiser_inputs as cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIZES = [(11, 9), (13, 7)]
ENTRY_POINTS = ("pt_denoise_default_settings", "pt_denoise_plane", "pt_denoised_device_buffers", "pt_get_denoised", "pt_denoise_frame", "pt_denoise_pass_times")


def _const(v): return v if callable(v) else (lambda x, y: v)


def field_frame(w, h, radiance=0.5, depth=2.0, normal=(0, 0, 1), mv=(0, 0, 0), sky=lambda x, y: False, roughness=0.5):
    """a one-plane frame; every argument a constant or a function of (x, y)"""
    radiance, depth, normal, mv = _const(radiance), _const(depth), _const(normal), _const(mv)
    fr = ref.make_frame(w, h)
    for y in range(h):
        for x in range(w):
            a = radiance(x, y)
            ref.put(fr, x, y, 0, 1, ref.make_record(scene_length=np.inf if sky(x, y) else depth(x, y), normal=normal(x, y), mv=mv(x, y), roughness=roughness, noisy=(2 * a, 2 * a, 2 * a, a),
                                                    diff_est=(1, 1, 1), spec_est=(1, 1, 1)), w, h)
    return fr


def nrd_state(fr, w, h):
    sp, dn = cpu._params(active=1, w=w, h=h)
    o = np.zeros((h, w, 3), f32); d = np.zeros((h, w, 3), f32); d[..., 2] = -1
    return ref.nrd_prepare(ref.empty_state(w, h), fr, sp, dn, w, h, 0, True, o, d)


def field(w, h, **kw): return nrd_state(field_frame(w, h, **kw), w, h)


def bits(a): return np.asarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("w,h", SIZES)
def test_flat_field_stays_flat_for_every_iteration_count(w, h):
    st = field(w, h, sky=lambda x, y: x == w - 1)
    assert np.all(st["nrd_view_z"][:, :-1] == f32(-2)) and np.all(st["nrd_diff_radiance_hit_dist"][:, :-1, :3] == f32(0.5))
    for n in range(2, 9):
        stages = {}
        d, s, lengths, _ = rx.denoise_plane(st, rx.settings(atrousIterationNum=n), None, w, h, stages=stages)
        assert len(stages["iterations"]) == n
        for it_d, it_s in stages["iterations"] + [(d, s)]:
            assert np.array_equal(bits(it_d[:, :-1, :3]), bits(np.full((h, w - 1, 3), 0.5, f32))) and np.array_equal(bits(it_s[:, :-1, :3]), bits(np.full((h, w - 1, 3), 0.5, f32)))
            assert np.all(it_d[:, -1] == 0) and np.all(it_s[:, -1] == 0)                     # the sky column keeps 0, its neighbours are still 0.5
        assert np.all(d[..., 3] == 0) and np.all(s[..., 3] == 0)                             # .w: 0 for diffuse, the hit distance (0 here) for specular
        assert np.all(lengths[:, :-1] == 1) and np.all(lengths[:, -1] == 0)


def test_specular_w_carries_the_hit_distance_through():
    w, h = SIZES[0]
    st = field(w, h)
    st["nrd_spec_radiance_hit_dist"][..., 3] = np.arange(w * h, dtype=f32).reshape(h, w)
    d, s, _, _ = rx.denoise_plane(st, rx.settings(), None, w, h)
    assert np.array_equal(s[..., 3], st["nrd_spec_radiance_hit_dist"][..., 3]) and np.all(d[..., 3] == 0)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["depth", "normal"])
def test_no_value_crosses_a_depth_or_a_normal_step(w, h, kind):
    left = lambda x, y: x < 5
    kw = dict(depth=lambda x, y: 2.0 if left(x, y) else 4.0) if kind == "depth" else dict(normal=lambda x, y: (0, 0, 1) if left(x, y) else (1, 0, 0))
    st = field(w, h, radiance=lambda x, y: 1.0 if left(x, y) else 0.0, **kw)
    for n in (2, 5, 8):
        d, s, _, _ = rx.denoise_plane(st, rx.settings(atrousIterationNum=n), None, w, h)
        for out in (d, s):
            assert np.array_equal(bits(out[:, :5, :3]), bits(np.ones((h, 5, 3), f32))) and np.all(out[:, 5:, :3] == 0)


def test_static_camera_accumulates_with_alpha_one_over_length():
    w, h = SIZES[0]
    a, b, c = field(w, h, radiance=0.25), field(w, h, radiance=0.5), field(w, h, radiance=1.0)
    S = rx.settings()
    _, _, l1, hist = rx.denoise_plane(a, S, None, w, h)
    stages = {}
    _, _, l2, hist2 = rx.denoise_plane(b, S, hist, w, h, stages=stages)
    assert np.all(l1 == 1) and np.all(l2 == 2)                                              # lengths 2 and 2 (diffuse, specular)
    for acc in stages["accumulated"]: assert np.all(acc[..., :3] == f32(0.375))              # a + (b - a) / 2
    stages = {}
    _, _, l3, _ = rx.denoise_plane(c, S, hist2, w, h, stages=stages)
    third = f32(0.375) + (f32(1) - f32(0.375)) * (f32(1) / f32(3))
    assert np.all(l3 == 3) and np.all(bits(stages["accumulated"][0][..., :3]) == bits(third)) and np.all(bits(stages["accumulated"][1][..., :3]) == bits(third))
    # diffuseMaxAccumulatedFrameNum = 2: the diffuse length stays 2 (alpha 1/2), the specular one goes on to 3
    stages = {}
    _, _, l3, _ = rx.denoise_plane(c, rx.settings(diffuseMaxAccumulatedFrameNum=2), hist2, w, h, stages=stages)
    assert np.all(l3[..., 0] == 2) and np.all(l3[..., 1] == 3) and np.all(stages["accumulated"][0][..., :3] == f32(0.6875)) and np.all(bits(stages["accumulated"][1][..., :3]) == bits(third))
    # resetHistory: length 1, the output is that frame's input alone
    d, s, lr, _ = rx.denoise_plane(c, S, hist2, w, h, reset=True)
    assert np.all(lr == 1) and np.all(d[..., :3] == 1) and np.all(s[..., :3] == 1)


def test_integer_motion_fetches_the_pixel_three_to_the_right():
    w, h = SIZES[0]
    first = field(w, h, radiance=lambda x, y: 1.0 if x == 6 else 0.0)
    second = field(w, h, radiance=0.0, mv=(3, 0, 0))
    S = rx.settings()
    _, _, _, hist = rx.denoise_plane(first, S, None, w, h)
    stages = {}
    _, _, lengths, _ = rx.denoise_plane(second, S, hist, w, h, stages=stages)
    acc = stages["accumulated"][0][..., 0]
    assert np.all(acc[:, 3] == f32(0.5)) and np.all(np.delete(acc, 3, axis=1) == 0)           # the marked column of frame 1 is what x = 3 accumulates with: 1 + (0 - 1) / 2
    assert np.all(lengths[:, :8] == 2) and np.all(lengths[:, 8:] == 1)                      # x + 3 >= 11: the tap falls outside the frame


def test_disocclusion_thresholds_and_the_mix():
    w, h = SIZES[0]
    S = rx.settings()
    _, _, _, hist = rx.denoise_plane(field(w, h, depth=2.0), S, None, w, h)
    far = field(w, h, depth=3.0)
    assert np.all(rx.denoise_plane(far, S, hist, w, h)[2] == 1)                             # |2 - 3| beyond 0.03 x 3: the history is dropped
    far["nrd_disocclusion_threshold_mix"][...] = 255
    assert np.all(rx.denoise_plane(far, S, hist, w, h)[2] == 1)                             # threshold 0.2: a 50 % change is still dropped
    near = field(w, h, depth=2.2)
    assert np.all(rx.denoise_plane(near, S, hist, w, h)[2] == 1)                            # mix 0: threshold 0.03
    near["nrd_disocclusion_threshold_mix"][...] = 255
    assert np.all(rx.denoise_plane(near, S, hist, w, h)[2] == 2)                            # mix 1: threshold 0.2 keeps a 10 % change
    assert np.all(rx.denoise_plane(near, rx.settings(useDisocclusionThresholdMix=0), hist, w, h)[2] == 1)      # ... and the mix switched off drops it again


@pytest.mark.parametrize("w,h", SIZES)
def test_anti_firefly_clamps_a_single_bright_pixel(w, h):
    st = field(w, h, radiance=1.0)
    # (set after the prepare pass, whose own radiance clamp would cap the pixel at luminance 128 first)
    st["nrd_diff_radiance_hit_dist"][4, 5, :3] = 1024; st["nrd_spec_radiance_hit_dist"][4, 5, :3] = 1024
    d, s, _, _ = rx.denoise_plane(st, rx.settings(), None, w, h)
    assert np.all(d[..., :3] == 1) and np.all(s[..., :3] == 1)                               # at most 1 at the pixel, and the field stays 1
    d, s, _, _ = rx.denoise_plane(st, rx.settings(enableAntiFirefly=0), None, w, h)
    assert d[4, 5, 0] > 1


def test_roughness_zero_keeps_the_centre_tap():
    """the prepare pass floors the roughness at 0.2; the filter does not rely on it: with roughness 0 the specular cone is one direction, the centre tap still counts (its stops
    are 1 by definition), so the result is finite and, on a flat field, the input"""
    w, h = SIZES[0]
    st = field(w, h, radiance=0.5)
    st["nrd_normal_roughness"][..., 3] = 0
    d, s, _, _ = rx.denoise_plane(st, rx.settings(), None, w, h)
    assert np.all(d[..., :3] == f32(0.5)) and np.all(s[..., :3] == f32(0.5)) and np.all(np.isfinite(s)) and np.all(np.isfinite(d))


# ---- the independent anchor: with the colour stop off, one flat surface is filtered by the plain separable dilated B3 kernel, renormalised at the frame edge
def _conv_rows(a, k): return np.stack([np.convolve(r, k, "full")[len(k) // 2:len(k) // 2 + len(r)] for r in a])


def _b3_filter(img, iterations):
    img = np.asarray(img, np.float64)
    for i in range(iterations):
        k = np.zeros(4 * (1 << i) + 1); k[::1 << i] = np.array([1, 4, 6, 4, 1]) / 16.0
        conv = lambda a: _conv_rows(_conv_rows(a, k).T, k).T
        img = conv(img) / conv(np.ones_like(img))
    return img


@pytest.mark.parametrize("w,h", SIZES)
def test_without_the_colour_stop_the_filter_is_the_b3_convolution(w, h):
    st = field(w, h, radiance=1.0)
    S = rx.settings(luminanceSigmaScale=0.0, enableAntiFirefly=0)
    rng = np.random.default_rng(7)
    for n in (2, 5):
        noise = rng.uniform(0.5, 1.5, (h, w, 3)).astype(f32)
        st["nrd_diff_radiance_hit_dist"][..., :3] = noise; st["nrd_spec_radiance_hit_dist"][..., :3] = noise[..., ::-1]
        S["atrousIterationNum"] = n
        d, s, _, _ = rx.denoise_plane(st, S, None, w, h)
        for c in range(3):
            assert np.allclose(d[..., c], _b3_filter(noise[..., c], n), rtol=1e-5, atol=0)
            assert np.allclose(s[..., c], _b3_filter(noise[..., 2 - c], n), rtol=1e-5, atol=0)


def test_variance_reduction_is_the_filters_own_sum_of_squared_weights():
    """The filter is linear here, so the variance of an output pixel under independent input noise of variance v is v x the sum of its squared weights. The weights come from the
    kernels (the filter of unit impulses); the variance is measured over 24 noise fields per pixel and compared as the mean over the frame, within a factor 2 for the finite sample."""
    w, h = SIZES[0]; n = 2
    st = field(w, h, radiance=1.0)
    S = rx.settings(luminanceSigmaScale=-1.0, enableAntiFirefly=0, atrousIterationNum=n)
    sum_w2 = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            e = np.zeros((h, w)); e[y, x] = 1
            sum_w2 += _b3_filter(e, n) ** 2      # (the weight of input (x, y) in every output pixel)
    rng = np.random.default_rng(11); outs = []
    for _ in range(24):
        noise = rng.uniform(0.5, 1.5, (h, w)).astype(f32)
        st["nrd_diff_radiance_hit_dist"][..., :3] = noise[..., None]
        outs.append(rx.denoise_plane(st, S, None, w, h)[0][..., 0].astype(np.float64))
    measured = np.var(np.stack(outs), axis=0, ddof=1).mean(); expected = (1.0 / 12.0) * sum_w2.mean()
    assert sum_w2.max() < 0.2                                                                # (two iterations already average over tens of pixels)
    assert expected / 2 <= measured <= expected * 2, (measured, expected)


def test_hand_cases_run_through_the_whole_loop():
    """Sample::Denoise's loop with this denoiser over the frames of test_denoiser_inputs.hand_cases(): two frames with history; sky stays 0, everything is finite"""
    for case in cpu.hand_cases():
        fr, sp, dn, w, h = case["frame"], case["sp"], case["dn"], case["w"], case["h"]
        o = np.zeros((h, w, 3), f32); d = np.zeros((h, w, 3), f32); d[..., 2] = -1
        hist = {}; st = None
        for f in range(2):
            st, per = rx.denoise_frame(fr, sp, dn, rx.settings(), w, h, {p: (o, d) for p in range(3)}, hist, state=st)
            assert np.all(np.isfinite(st["output_color"]))
            lengths = per[0][2]; land = np.arange(w) != 10      # plane 0: a surface everywhere but the sky column x = 10
            assert np.all(lengths[:, land] == f + 1) and np.all(lengths[:, 10] == 0) and np.all(per[0][0][:, 10] == 0) and np.all(per[0][1][:, 10] == 0)


def test_header_declares_and_library_exports_the_entry_points():
    import rtxpt_amd as pt
    text = open(os.path.join(ROOT, "include", "mi355pt.h")).read()
    for n in ENTRY_POINTS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % n, text), n
        assert n in pt.EXPORTS, n
    assert "} PtDenoiseSettings;" in text
    L = pt.load_library()
    for n in ENTRY_POINTS: assert hasattr(L, n), n
    d = pt.denoise_default_settings()
    assert d.dtype.itemsize == 48
    want = dict(atrousIterationNum=5, depthThreshold=f32(0.004), lobeAngleFraction=f32(0.7), diffuseMaxAccumulatedFrameNum=25, specularMaxAccumulatedFrameNum=40,
                diffuseMaxFastAccumulatedFrameNum=5, specularMaxFastAccumulatedFrameNum=6, enableAntiFirefly=1, disocclusionThreshold=f32(0.03),
                disocclusionThresholdAlternate=f32(0.2), useDisocclusionThresholdMix=1)
    for k, v in want.items(): assert d[k] == v, k
    assert d["luminanceSigmaScale"] > 0
    for k, v in rx.DEFAULTS.items(): assert d[k] == f32(v) if isinstance(v, float) else d[k] == v, k      # the restatement's defaults are the library's

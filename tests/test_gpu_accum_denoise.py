"""The reference-mode denoiser on the device (run with -m gpu; include/mi355pt.h pt_accum_denoise, rtxpt_amd/csrc/pt_accum_denoise.h / .hip / _api.hip, docs/WIDENING.md N13):
the dual-buffer non-local-means filter over the mean of a pixel's samples and the mean of its even-indexed ones. Everything is compared bit for bit with
tests/accum_denoise_ref.py, the numpy restatement: the denoised picture and what the prepare launch left (the staged odd-sample means, the variance, the valid mask).
Worked and random frames go in through pt_accum_denoise_host_inputs; a rendered frame (the Cornell box C1 at 44 x 20 with render_adaptive at 4 / 2 / 16, the frame of
tests/test_gpu_adaptive.py) goes through pt_accum_denoise itself. The kernel's tile is 16 x 16: 37 x 35 is two full tiles and a partial one along both axes."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_denoise_ref as ad

pytestmark = pytest.mark.gpu
f32 = np.float32

SIZES = [(11, 9), (13, 7), (35, 10), (37, 35)]
PARAMS = [dict(searchRadius=1, patchRadius=0), dict(), dict(searchRadius=8, patchRadius=3), dict(searchRadius=8, patchRadius=0), dict(searchRadius=1, patchRadius=3),
          dict(k=0.9, alpha=0.0), dict(k=0.2, alpha=2.5, epsilon=1e-4, maxRadiance=100.0)]
W, H = 44, 20
MIN, STEP, MAX = 4, 2, 16
_cache = {}


def _bits(a): return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else np.ascontiguousarray(a)


def _once(key, make):
    if key not in _cache: _cache[key] = make()
    return _cache[key]


def _params(**kw):
    import rtxpt_amd as pt
    return pt.accum_denoise_default_params(**kw)


def _code(call):
    import rtxpt_amd as pt
    with pytest.raises(pt.PtError) as e: call()
    return e.value.code


def _blank(w, h, **kw):
    """a context with a frame size and nothing else: all that pt_accum_denoise_host_inputs needs"""
    import rtxpt_amd as pt
    t = pt.PathTracer(**kw); t.resize(w, h)
    return t


def _rendered():
    """the module's context with a scene (the frame of tests/test_gpu_adaptive.py)"""
    def make():
        import rtxpt_amd as pt
        from rtxpt_amd import scenes
        sc, cam = scenes.cornell_box("C1")
        t = pt.PathTracer(); t.set_scene(sc); t.set_camera(scenes.bridge_camera(W, H, **cam)); t.set_settings(scenes.config_settings("C1")); t.resize(W, H)
        return t
    return _once("rendered", make)


def _adaptive(threshold, **kw):
    import rtxpt_amd as pt
    return pt.adaptive_default_params(**dict(dict(minSamples=MIN, step=STEP, maxSamples=MAX, threshold=threshold, darkFloor=0.01), **kw))


def step_frame(w, h):
    """0.5 | 2.0 with A = H: no variance, so the filter returns it bit for bit"""
    g = np.full((h, w), 0.5, f32); g[:, w // 2:] = 2.0
    A = np.ascontiguousarray(np.concatenate([np.repeat(g[..., None], 3, -1), np.full((h, w, 1), 0.75, f32)], -1))
    return A, A.copy()


def random_frame(w, h, seed):
    """a noisy coloured ramp as two independent halves, with NaN, +-inf, 3e38 and -0.0 planted at the corners and on both sides of the kernel's tile seams"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    base = (0.2 + 1.5 * (xs >= w // 2) + 0.02 * ys)[..., None].astype(f32) * np.array([1.0, 0.7, 0.4], f32)
    Hh = (base + rng.normal(0, 0.15, (h, w, 3)).astype(f32)).astype(f32); O = (base + rng.normal(0, 0.15, (h, w, 3)).astype(f32)).astype(f32)
    A = np.concatenate([(Hh + O) * f32(0.5), rng.uniform(0, 1, (h, w, 1)).astype(f32)], -1).astype(f32)
    Hf = np.concatenate([Hh, rng.uniform(0, 1, (h, w, 1)).astype(f32)], -1).astype(f32)
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + [(x, y) for x in (15, 16, 31, 32) for y in (3, 15, 16, 31, 32) if x < w and y < h]
    vals = [np.nan, np.inf, -np.inf, 3e38, -0.0]
    for i, (x, y) in enumerate(spots):
        v = f32(vals[i % len(vals)])
        if i % 2: Hf[y, x, i % 3] = v
        else: A[y, x, i % 3] = v
    A[h // 2, 1, :3] = f32(-0.0); Hf[h // 2, 1, :3] = f32(-0.0)
    return np.ascontiguousarray(A), np.ascontiguousarray(Hf)


def _assert_equals_restatement(t, got, A, Hf, P, what):
    want = ad.run(A, Hf, P)
    state = t.accum_denoise_state()
    for k, g, w_ in (("denoised", got, want["denoised"]), ("odd", state["odd"], want["odd"]), ("variance", state["variance"], want["variance"]), ("valid", state["valid"], want["valid"])):
        a, b = _bits(g), _bits(w_)
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs in %d words" % (what, k, int((a != b).sum()) if a.shape == b.shape else -1)
    return want


# ---- 1. worked and random frames through pt_accum_denoise_host_inputs
@pytest.mark.parametrize("w,h", SIZES)
def test_host_frames_equal_the_restatement(w, h):
    t = _blank(w, h)
    A, Hf = step_frame(w, h)
    got = t.accum_denoise_host_inputs(A, Hf)
    _assert_equals_restatement(t, got, A, Hf, _params(), "step %dx%d" % (w, h))
    assert np.array_equal(_bits(got), _bits(A))                                   # worked: a zero-variance step comes back as it went in
    A, Hf = random_frame(w, h, 5 + w)
    with np.errstate(invalid="ignore"):
        invalid = ~np.isfinite(A[..., :3]).all(-1) | ~np.isfinite(Hf[..., :3]).all(-1) | (np.abs(A[..., :3]) > 100).any(-1) | (np.abs(Hf[..., :3]) > 100).any(-1)
    assert invalid.sum() >= 4
    for kw in PARAMS:
        P = _params(**kw)
        got = t.accum_denoise_host_inputs(A, Hf, P)
        want = _assert_equals_restatement(t, got, A, Hf, P, "random %dx%d %r" % (w, h, kw))
        assert np.array_equal(want["valid"] == 0, invalid) and np.array_equal(_bits(got)[invalid], _bits(A)[invalid]) and np.isfinite(got[~invalid]).all()
        assert not np.array_equal(_bits(got)[~invalid][:, :3], _bits(A)[~invalid][:, :3])      # the filter did something
    # a second call's bits equal the first's
    again = t.accum_denoise_host_inputs(A, Hf, P)
    assert np.array_equal(_bits(again), _bits(got))
    t.close()


# ---- 2. a rendered frame through pt_accum_denoise
@pytest.mark.parametrize("which", ["threshold_zero", "median_block_error"])
def test_rendered_frame_equals_the_restatement_and_the_host_route(which):
    t = _rendered()
    thr = 0.0
    if which == "median_block_error":      # the median block error at the first evaluation, as tests/test_gpu_adaptive.py chooses it
        t.render_adaptive(_adaptive(0.0, maxSamples=MIN))
        thr = f32(np.median(t.adaptive_state()["block_error"]))
    stats, _ = t.render_adaptive(_adaptive(thr))
    A, st = t.radiance(), t.adaptive_state()
    if which == "median_block_error": assert len(np.unique(st["counts"])) >= 2, "nothing retired early: %s" % (np.unique(st["counts"]),)
    else: assert np.all(st["counts"] == MAX)
    for kw in (dict(), dict(searchRadius=3, patchRadius=1, k=0.7)):
        P = _params(**kw)
        got, ms = t.accum_denoise(P, timed=True)
        assert np.isfinite(ms) and ms >= 0
        _assert_equals_restatement(t, got, A, st["half"], P, "%s %r" % (which, kw))
        assert not np.array_equal(_bits(got), _bits(A))
        # neither the radiance buffer, the even-sample buffer nor the counts were written
        after = t.adaptive_state()
        assert np.array_equal(_bits(t.radiance()), _bits(A)) and np.array_equal(_bits(after["half"]), _bits(st["half"])) and np.array_equal(after["counts"], st["counts"])
        # the host route over the same arrays: the same bits, and again nothing of the accumulation touched
        host = t.accum_denoise_host_inputs(A, st["half"], P)
        assert np.array_equal(_bits(host), _bits(got))
        assert np.array_equal(_bits(t.radiance()), _bits(A)) and np.array_equal(_bits(t.adaptive_state()["half"]), _bits(st["half"]))
        assert np.array_equal(_bits(t.accum_denoise(P)), _bits(got))              # a second call's bits equal the first's


# ---- 3. the display tail on the denoised picture
def test_display_tail_reads_the_denoised_picture():
    import rtxpt_amd as pt
    import bloom_ref as bloom
    from oracle import ptref
    t = _rendered()
    t.render_adaptive(_adaptive(0.0))
    bp = pt.bloom_default_params(radius=8.0, intensity=0.5)
    before = t.bloom(bp, source=0)
    D = t.accum_denoise()
    for tm in (pt.default_tonemap(), pt.default_tonemap(exposure_compensation=-2.0, toneMapOperator="reinhard")):
        out = t.tonemap_accum_denoised(tm)
        assert out.shape == (H, W, 4) and np.array_equal(out, ptref.tonemap(D, tm))
    assert not np.array_equal(t.tonemap_accum_denoised(), t.tonemap())
    lum, want = t.average_luminance_accum_denoised(), ptref.average_luminance(D)
    assert np.isfinite(lum) and lum > 0 and abs(lum / want - 1) < 2e-5, (lum, want)      # the tolerance of tests/test_display_path.py for pt_average_luminance
    got, ms = t.bloom_accum_denoised(bp, timed=True)
    assert np.isfinite(ms) and ms >= 0
    assert np.array_equal(_bits(got), _bits(bloom.bloom(D, bloom.params(radius=8.0, intensity=0.5)))) and np.array_equal(_bits(t.bloomed()), _bits(got))
    assert np.array_equal(t.tonemap_bloomed(), ptref.tonemap(got, pt.default_tonemap()))
    assert np.array_equal(_bits(t.accum_denoised()), _bits(D))                    # the source of the bloom is never written
    # pt_bloom itself: source 0 as before, source 2 still refused
    assert np.array_equal(_bits(t.bloom(bp, source=0)), _bits(before)) and not np.array_equal(_bits(before), _bits(got))
    assert _code(lambda: t.bloom(bp, source=2)) == pt.PT_ERROR_INVALID_ARGUMENT
    assert _code(lambda: t.bloom_accum_denoised(pt.bloom_default_params(radius=65.0))) == pt.PT_ERROR_INVALID_ARGUMENT
    d, pitch = t.accum_denoised_device_buffer()
    assert d and pitch == W * 16


# ---- 4. refusals and lifetimes
def test_refusals_and_lifetimes():
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    t = _rendered()
    readers = (t.accum_denoised, t.accum_denoised_device_buffer, t.accum_denoise_state, t.tonemap_accum_denoised, t.average_luminance_accum_denoised, t.bloom_accum_denoised)

    def nothing_there():
        assert _code(t.accum_denoise) == pt.PT_ERROR_NOT_READY
        for read in readers: assert _code(read) == pt.PT_ERROR_NOT_READY, read.__name__

    t.resize(W, H)
    nothing_there()                                                              # before any adaptive render
    t.render(0, MIN)
    nothing_there()                                                              # a plain render is not one
    t.reset_accumulation()
    t.render_adaptive(_adaptive(0.0, maxSamples=MIN))
    first = t.accum_denoise()
    # every bound, from outside and from inside, and NaN
    bad = [dict(searchRadius=0), dict(searchRadius=9), dict(patchRadius=4), dict(k=0.049), dict(k=4.1), dict(k=np.nan), dict(alpha=-0.01), dict(alpha=4.1), dict(alpha=np.nan),
           dict(epsilon=0.0), dict(epsilon=0.9e-20), dict(epsilon=1.1), dict(epsilon=np.nan), dict(maxRadiance=0.0), dict(maxRadiance=-1.0), dict(maxRadiance=1.1e15),
           dict(maxRadiance=np.inf), dict(maxRadiance=np.nan)]
    A = t.radiance(); Hf = t.adaptive_state()["half"]
    for kw in bad:
        assert _code(lambda: t.accum_denoise(_params(**kw))) == pt.PT_ERROR_INVALID_ARGUMENT, kw
        assert _code(lambda: t.accum_denoise_host_inputs(A, Hf, _params(**kw))) == pt.PT_ERROR_INVALID_ARGUMENT, kw
    assert np.array_equal(_bits(t.accum_denoised()), _bits(first))                # a refused call leaves the picture
    good = [dict(searchRadius=1), dict(searchRadius=8), dict(patchRadius=0), dict(patchRadius=3), dict(k=0.05), dict(k=4.0), dict(alpha=0.0), dict(alpha=4.0),
            dict(epsilon=1e-20), dict(epsilon=1.0), dict(maxRadiance=1e15)]
    for kw in good: assert t.accum_denoise(_params(**kw)).shape == (H, W, 4), kw
    assert np.array_equal(_bits(t.accum_denoise()), _bits(first))                 # a second call's bits equal the first's
    # the picture and the readiness end where the accumulation is reset
    t.reset_accumulation(); nothing_there()
    t.render_adaptive(_adaptive(0.0, maxSamples=MIN)); t.accum_denoise()
    t.resize(W, H); nothing_there()
    t.render_adaptive(_adaptive(0.0, maxSamples=MIN))
    assert np.array_equal(_bits(t.accum_denoise()), _bits(first))
    t.render_adaptive(_adaptive(0.0, maxSamples=MIN))                             # a new adaptive render drops the picture, not the readiness
    for read in readers: assert _code(read) == pt.PT_ERROR_NOT_READY, read.__name__
    assert np.array_equal(_bits(t.accum_denoise()), _bits(first))
    sc, _ = scenes.cornell_box("C1")
    t.animate(instances=sc["instances"]); nothing_there()                         # pt_animate restarts the accumulation, also with the pose it had
    t.render_adaptive(_adaptive(0.0, maxSamples=MIN))
    assert np.isfinite(t.accum_denoise()[..., :3]).all()
    # the host route needs only a frame size, and leaves a picture that a reset drops as well
    b = _blank(W, H)
    assert _code(b.accum_denoise) == pt.PT_ERROR_NOT_READY
    assert np.array_equal(_bits(b.accum_denoise_host_inputs(A, Hf)), _bits(first))
    b.reset_accumulation()
    assert _code(b.accum_denoised) == pt.PT_ERROR_NOT_READY
    b.close()
    e = pt.PathTracer()
    assert _code(lambda: e.accum_denoise_host_inputs(np.zeros((0, 0, 4), f32), np.zeros((0, 0, 4), f32))) == pt.PT_ERROR_NOT_READY      # no frame size
    e.close()


def test_a_rank_of_a_sharded_layout_is_refused():
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    sc, cam = scenes.cornell_box("C1")
    for rank in range(2):
        t = pt.PathTracer(shard_rank=rank, shard_count=2)
        t.set_scene(sc); t.set_camera(scenes.bridge_camera(W, H, **cam)); t.set_settings(scenes.config_settings("C1")); t.resize(W, H)
        t.render_adaptive(_adaptive(0.0, maxSamples=MIN))
        assert _code(t.accum_denoise) == pt.PT_ERROR_UNSUPPORTED
        assert _code(t.accum_denoised) == pt.PT_ERROR_NOT_READY
        # whole pictures from elsewhere are fine on any layout
        A, Hf = step_frame(W, H)
        assert np.array_equal(_bits(t.accum_denoise_host_inputs(A, Hf)), _bits(A))
        t.close()

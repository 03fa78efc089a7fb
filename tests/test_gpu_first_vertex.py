"""Vertex 0 in place on the device (run with -m gpu; rtxpt_amd/csrc/pt_frame.hip RenderFrame::enable_first_vertex_in_place, pt_trace.hip k_extend_first, k_first_split_rays,
k_classify<UNIFORM>, k_shade<..., FIRST>): a compacted batch of pt_render whose first pass is a wavefront pass starts without k_generate, and that pass's launches form the vertex-0
state — the camera ray, the pixel id, the sample index, constants of the frame — where they use it. Same operations on the same operands: every comparison here is bit for bit against
the CPU oracle rendering the same frame, ray and hit counts included (the batch cases: a band of rows, the whole frame and the counts against the same build's serial-kernel frame; the
tile shard: against the unsharded frame), with MI355PT_FIRST_VERTEX_IN_PLACE at 1 (the default) and at 0 (k_generate in front of every batch). The switch is read at pt_create, so the
environment is set before a tracer is made. Covered: the classify variant with fused and separate traversal launches, the serial-kernel frame and the home-slot layout (which keep
k_generate), odd counts below one block with and without the tail kernel, a sample split that is no power of two, continued accumulation (sampleFirst + s), the thin lens and the
sub-pixel jitter of computeCameraRay, bounceCount 0 (every path terminates at its first hit: one flags word for all), a moved camera on a context whose pool holds the previous frame's
state, two and four pipelined batches, a tile shard. Semantics preserved: the reference's Rtxpt/Shaders/PathTracer/PathTracer.hlsli:47-119 (EmptyPathInitialize, SetupPathPrimaryRay)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWITCH = "MI355PT_FIRST_VERTEX_IN_PLACE"
_cache = {}


def _bits(a): return np.asarray(a).view(np.uint32)


def _once(key, make):
    if key not in _cache: _cache[key] = make()
    return _cache[key]


def _bistro(): return _once("bistro", lambda: __import__("rtxpt_amd").scenes.bistro_like(scale=0.05, tex_size=128))


def _oracle(sc, camd, S, w, h, first, n, rect=None):
    """frame, (extendRays, shadowRays, hits) of the oracle; rect = (x0, y0, x1, y1): only those pixels are rendered and counted"""
    from oracle import ptref
    o = ptref.Oracle(lp16=bool(int(S["useFp16Types"]))); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h)
    o.render(first, n, rect=rect)
    c = o.counters(); out = (o.radiance(), (c["extendRays"], c["shadowRays"], c["hits"])); o.close()
    return out


def _tracer(monkeypatch, switch, sc, camd, S, w, h, **kw):
    import rtxpt_amd as pt
    monkeypatch.setenv(SWITCH, str(switch))
    t = pt.PathTracer(**kw); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h)
    return t


def _frame(t, first, n):
    t.reset_accumulation(); st = t.render(first, n)
    return t.radiance(), (int(st["extendRays"]), int(st["shadowRays"]), int(st["hits"]))


def _assert_equal(got, want, what):
    a, b = _bits(got[0]), _bits(want[0])
    assert np.array_equal(a, b), "%s: %d pixels differ from the oracle" % (what, int((a != b).any(-1).sum()))
    assert got[1] == want[1], "%s: ray / hit counts %s, the oracle's %s" % (what, got[1], want[1])


# ---- 1. the classify variant: 320 x 180 x 2 = 115 200 paths in one batch, above PT_CLASSIFY_FROM (65 536)
def _bistro_case(**settings):
    from rtxpt_amd import scenes
    sc, cam = _bistro(); w, h = 320, 180
    camd = scenes.bridge_camera(w, h, **cam); S = scenes.default_settings(useFp16Types=1, **settings)
    key = "bistro_320x180x2" + "".join("_%s%s" % kv for kv in sorted(settings.items()))
    return sc, camd, S, w, h, _once(key, lambda: _oracle(sc, camd, S, w, h, 0, 2))


@pytest.mark.parametrize("switch", [1, 0])
@pytest.mark.parametrize("config", ["as_is", "fused_0", "serial_kernels", "compact_pool_0"])
def test_classified_first_pass_matches_oracle(config, switch, monkeypatch):
    sc, camd, S, w, h, want = _bistro_case()
    if config == "compact_pool_0": monkeypatch.setenv("MI355PT_COMPACT_POOL", "0")      # the home-slot layout: k_generate whatever the switch says
    t = _tracer(monkeypatch, switch, sc, camd, S, w, h)
    if config == "fused_0": t.set_fused_traversal(0)
    elif config == "serial_kernels": t.set_serial_kernels(True)      # not a composed frame: k_generate
    got = _frame(t, 0, 2); t.close()
    assert want[1][1] > 0
    _assert_equal(got, want, "%s, switch %d" % (config, switch))


# ---- 2. small odd frames: 33 x 17 = 561 pixels, smaller than one block and below PT_CLASSIFY_FROM; 3 spp: a sample split that is no power of two
def _c2(eye_shift=0.0, **camera):
    from rtxpt_amd import scenes
    sc, cam = scenes.cornell_box("C2"); S = scenes.config_settings("C2").copy(); cam = dict(cam, **camera)
    if eye_shift:
        e = np.array(cam["pos"], np.float32).copy(); e[0] += np.float32(eye_shift); cam["pos"] = e
    return sc, scenes.bridge_camera(33, 17, **cam), S


@pytest.mark.parametrize("switch", [1, 0])
@pytest.mark.parametrize("tail", [0, 4096])      # 4096: vertex 0 goes to the tail kernel, which reads the pool — k_generate must have run
@pytest.mark.parametrize("spp", [1, 3])
def test_small_odd_frames_match_oracle(spp, tail, switch, monkeypatch):
    sc, camd, S = _c2()
    want = _once("c2_33x17x%d" % spp, lambda: _oracle(sc, camd, S, 33, 17, 0, spp))
    t = _tracer(monkeypatch, switch, sc, camd, S, 33, 17); t.set_tail_paths(tail)
    got = _frame(t, 0, spp); t.close()
    _assert_equal(got, want, "%d spp, tail %d, switch %d" % (spp, tail, switch))


# ---- 3. continued accumulation: the second call's samples are sampleFirst + s
@pytest.mark.parametrize("switch", [1, 0])
def test_continued_accumulation_matches_oracle(switch, monkeypatch):
    sc, camd, S = _c2()
    want = _once("c2_33x17x4", lambda: _oracle(sc, camd, S, 33, 17, 0, 4))
    t = _tracer(monkeypatch, switch, sc, camd, S, 33, 17); t.set_tail_paths(0)
    t.reset_accumulation(); a = t.render(0, 2); b = t.render(2, 2); img = t.radiance(); t.close()
    counts = tuple(int(a[k]) + int(b[k]) for k in ("extendRays", "shadowRays", "hits"))
    _assert_equal((img, counts), want, "render(0, 2) + render(2, 2), switch %d" % switch)


# ---- 4. the thin lens and the sub-pixel jitter of computeCameraRay
@pytest.mark.parametrize("switch", [1, 0])
def test_thin_lens_and_jitter_match_oracle(switch, monkeypatch):
    sc, camd, S = _c2(aperture_radius=0.05, jitter=(0.25, -0.375))
    assert float(camd["ApertureRadius"]) > 0 and tuple(float(v) for v in camd["Jitter"]) != (0.0, 0.0)
    want = _once("c2_lens_33x17x3", lambda: _oracle(sc, camd, S, 33, 17, 0, 3))
    t = _tracer(monkeypatch, switch, sc, camd, S, 33, 17); t.set_tail_paths(0)
    got = _frame(t, 0, 3); t.close()
    _assert_equal(got, want, "thin lens, switch %d" % switch)


# ---- 5. bounceCount 0: every path carries PF_terminateAtNextBounce from generation (k_classify<UNIFORM>'s flags word puts every hit into the terminating class)
@pytest.mark.parametrize("switch", [1, 0])
def test_uniform_terminate_flag_matches_oracle(switch, monkeypatch):
    sc, camd, S, w, h, want = _bistro_case(bounceCount=0)
    t = _tracer(monkeypatch, switch, sc, camd, S, w, h)
    got = _frame(t, 0, 2); t.close()
    assert want[1][1] == 0      # (a vertex that terminates samples no light)
    _assert_equal(got, want, "bounceCount 0, switch %d" % switch)


# ---- 6. stale state: the pool keeps the previous frame's state where k_generate used to overwrite it; a reader of vertex-0 state that was missed shows up here
@pytest.mark.parametrize("switch", [1, 0])
def test_moved_camera_sees_no_stale_state(switch, monkeypatch):
    from rtxpt_amd import scenes
    sc, camd, S, w, h, want = _bistro_case()
    _, cam = _bistro(); e = np.array(cam["pos"], np.float32).copy(); e[0] += np.float32(0.125)
    elsewhere = scenes.bridge_camera(w, h, **dict(cam, pos=e))
    t = _tracer(monkeypatch, switch, sc, elsewhere, S, w, h); _frame(t, 0, 2)
    t.set_camera(camd); again = _frame(t, 0, 2); t.close()
    f = _tracer(monkeypatch, switch, sc, camd, S, w, h); fresh = _frame(f, 0, 2); f.close()
    assert np.array_equal(_bits(again[0]), _bits(fresh[0])) and again[1] == fresh[1]
    _assert_equal(again, want, "moved camera, switch %d" % switch)


# ---- 7. pipelined batches: every batch forms the vertex-0 state of its own slice of the owned pixels (FirstVertex: ownedPixels + pixFirst)
BAND = (228, 292)      # the rows compared with the oracle: 64 rows across the middle of the frame, where a batch's owned pixels end and the next one's begin


@pytest.mark.parametrize("spp,batches", [(2, 2), (4, 4)])
def test_pipelined_batches_match_oracle_band(spp, batches, monkeypatch):
    """1024 x 520 at 2 spp is 1 064 960 paths per call (two batches), at 4 spp 2 129 920 (four). Rows 228..291 against the oracle, bit for bit; the tracer reports no counts per
    rectangle, so the counts, and the whole frame, are held to the same build's serial-kernel frame (one batch, k_generate), which case 1 holds to the oracle at a smaller size."""
    from rtxpt_amd import scenes
    sc, cam = _bistro(); w, h = 1024, 520
    assert "MI355PT_BATCHES" not in os.environ
    assert batches == (1 if w * h * spp < (1 << 20) else 2 if w * h * spp < (1 << 21) else 4)
    camd = scenes.bridge_camera(w, h, **cam); S = scenes.default_settings(useFp16Types=1)
    want = _oracle(sc, camd, S, w, h, 0, spp, rect=(0, BAND[0], w, BAND[1]))[0]
    b = _bits(want)[BAND[0]:BAND[1]]
    frames = {}
    for switch in (1, 0):
        t = _tracer(monkeypatch, switch, sc, camd, S, w, h); frames[switch] = _frame(t, 0, spp)
        if switch == 1: t.set_serial_kernels(True); one = _frame(t, 0, spp)
        t.close()
    for switch, got in frames.items():
        a = _bits(got[0])[BAND[0]:BAND[1]]
        assert np.array_equal(a, b), "switch %d, rows %d..%d: %d pixels differ from the oracle" % (switch, BAND[0], BAND[1] - 1, int((a != b).any(-1).sum()))
        assert got[1][1] > 0 and np.array_equal(_bits(got[0]), _bits(one[0])) and got[1] == one[1], "switch %d against the serial-kernel frame" % switch


# ---- 8. a tile shard: the batch's owned pixels are the rank's tiles, not a rectangle
def test_tile_shard_equals_the_unsharded_frame(monkeypatch):
    import rtxpt_amd as pt
    sc, camd, S, w, h, want = _bistro_case()
    own = pt.shard_layout(w, h, 1, 2); ys, xs = (own & 0xFFFF).astype(np.int64), (own >> 16).astype(np.int64)
    assert 0 < own.size < w * h
    shards = {}
    for switch in (1, 0):
        t = _tracer(monkeypatch, switch, sc, camd, S, w, h, shard_rank=1, shard_count=2); shards[switch] = _frame(t, 0, 2); t.close()
    for switch, got in shards.items():
        assert np.array_equal(_bits(got[0])[ys, xs], _bits(want[0])[ys, xs]), "switch %d: the rank's tiles differ from the oracle's frame" % switch
    assert shards[1][1] == shards[0][1] and shards[1][1][0] >= own.size * 2

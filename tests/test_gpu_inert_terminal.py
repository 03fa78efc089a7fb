"""Terminal hits that cannot emit are dropped before k_shade (run with -m gpu; rtxpt_amd/csrc/pt_wavefront.hip k_classify<false, DROP>, pt_scene.h inert_bits_of /
inert_when_terminal, pt_build.hip k_inert_bits). A path whose PF_terminateAtNextBounce flag is set is shaded at its next hit for that hit's emission term alone; on a primitive that can
neither emit nor stand in for an analytic light, and whose hit the nested-dielectric check cannot reject, the vertex changes nothing anybody reads, and k_classify writes it into no
class. Held here: the frame is bit-equal to the CPU oracle's, ray and hit counts included, with MI355PT_DROP_INERT_TERMINAL at 1 (the default) and at 0; the two switch positions give
bit-identical radiance and equal counts; the dropped count (include/mi355pt_testhooks.h pt_get_inert_terminal) is > 0 with the switch on and 0 with it off, 0 for a scene in which
every material can emit, 0 with NEE-AT and its depth export; the device's table equals the numpy restatement of the predicate after set_scene, after a material edit and after a
light bake that adds a proxy link. The scene (tests/inert_terminal_cases.py) puts terminal vertices on an opaque wall, an emissive quad, an analytic-light proxy, a non-thin glass box
with a nested priority, a thin alpha-tested card and a panel whose emission rounds to zero in binary16. 512 x 256 x 4 spp = 524 288 paths: with bounceCount 2 and 3 the bounce bound
flags whole passes terminal while they still hold more than PT_CLASSIFY_FROM (65 536) paths, so k_classify runs on them; Russian roulette is on. The switch is read at pt_create."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import inert_terminal_cases as itc      # noqa: E402

SWITCH = "MI355PT_DROP_INERT_TERMINAL"
W, H, SPP = 512, 256, 4
_cache = {}


def _bits(a): return np.asarray(a).view(np.uint32)


def _once(key, make):
    if key not in _cache: _cache[key] = make()
    return _cache[key]


def _zoo(): return _once("zoo", itc.zoo)


def _settings(lp, bounces, quality, **kw):
    from rtxpt_amd import scenes
    S = scenes.default_settings(useFp16Types=lp, bounceCount=bounces, nestedDielectricsQuality=quality, **kw)
    assert int(S["enableRussianRoulette"]) == 1
    return S


def _oracle(sc, camd, S, w, h, n, rect=None):
    from oracle import ptref
    o = ptref.Oracle(lp16=bool(int(S["useFp16Types"]))); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h)
    o.render(0, n, rect=rect)
    c = o.counters(); out = (o.radiance(), (c["extendRays"], c["shadowRays"], c["hits"])); o.close()
    return out


def _tracer(monkeypatch, switch, sc, camd, S, w, h, **kw):
    import rtxpt_amd as pt
    monkeypatch.setenv(SWITCH, str(switch))
    t = pt.PathTracer(test_hooks=True, **kw); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h)
    return t


def _frame(t, n):
    """frame, (extendRays, shadowRays, hits), dropped"""
    t.reset_accumulation(); st = t.render(0, n)
    return t.radiance(), (int(st["extendRays"]), int(st["shadowRays"]), int(st["hits"])), t.inert_terminal()[1]


def _camera(w, h):
    from rtxpt_amd import scenes
    return scenes.bridge_camera(w, h, **_zoo()[1])


def _assert_frames_equal(got, want, what):
    a, b = _bits(got[0]), _bits(want[0])
    print("%s: %d differing pixels, counts %s / %s" % (what, int((a != b).any(-1).sum()), got[1], want[1]))
    assert np.array_equal(a, b), "%s: %d pixels differ" % (what, int((a != b).any(-1).sum()))
    assert got[1] == want[1], "%s: ray / hit counts %s against %s" % (what, got[1], want[1])


# ---- 1. one batch, both lp builds, bounceCount 2 and 3, nestedDielectricsQuality 0, 1 and 2: the oracle, and switch on against switch off
CASES = [(2, 0), (3, 0), (3, 1), (2, 2), (3, 2)]


@pytest.mark.parametrize("bounces,quality", CASES)
@pytest.mark.parametrize("lp", [0, 1])
def test_frame_matches_oracle_with_and_without_the_drop(lp, bounces, quality, monkeypatch):
    sc, _ = _zoo(); camd = _camera(W, H); S = _settings(lp, bounces, quality)
    want = _once(("oracle", lp, bounces, quality), lambda: _oracle(sc, camd, S, W, H, SPP))
    frames = {}
    for switch in (1, 0):
        t = _tracer(monkeypatch, switch, sc, camd, S, W, H); frames[switch] = _frame(t, SPP); t.close()
    print("lp %d, bounceCount %d, quality %d: dropped %d of %d hits (switch off: %d)" % (lp, bounces, quality, frames[1][2], frames[1][1][2], frames[0][2]))
    _assert_frames_equal(frames[1], want, "switch on against the oracle")
    _assert_frames_equal(frames[0], want, "switch off against the oracle")
    _assert_frames_equal(frames[1], frames[0], "switch on against switch off")
    assert want[1][1] > 0 and frames[1][2] > 0 and frames[0][2] == 0
    assert frames[1][2] < frames[1][1][2]      # (the first vertex's hits at least are shaded)


# ---- 2. where else a classified pass runs: the home-slot layout, serial-kernel frames, visibility launches of their own
@pytest.mark.parametrize("config", ["compact_pool_0", "serial_kernels", "fused_0"])
def test_other_compositions_match_oracle(config, monkeypatch):
    sc, _ = _zoo(); camd = _camera(W, H); S = _settings(1, 3, 1)
    want = _once(("oracle", 1, 3, 1), lambda: _oracle(sc, camd, S, W, H, SPP))
    if config == "compact_pool_0": monkeypatch.setenv("MI355PT_COMPACT_POOL", "0")
    t = _tracer(monkeypatch, 1, sc, camd, S, W, H)
    if config == "serial_kernels": t.set_serial_kernels(True)
    elif config == "fused_0": t.set_fused_traversal(0)
    got = _frame(t, SPP); t.close()
    _assert_frames_equal(got, want, config)
    assert got[2] > 0


# ---- 3. two and four pipelined batches: every batch has its own class counters
BAND = (96, 160)


@pytest.mark.parametrize("w,h,batches", [(1024, 256, 2), (1024, 512, 4)])
def test_pipelined_batches(w, h, batches, monkeypatch):
    """1024 x 256 x 4 spp is 1 048 576 paths (two batches), 1024 x 512 x 4 spp 2 097 152 (four). Rows 96..159 against the oracle, bit for bit; the tracer reports no counts per
    rectangle, so the whole frame and the counts are held to the same build with the switch off, which case 1 holds to the oracle."""
    assert "MI355PT_BATCHES" not in os.environ
    assert batches == (1 if w * h * SPP < (1 << 20) else 2 if w * h * SPP < (1 << 21) else 4)
    sc, _ = _zoo(); camd = _camera(w, h); S = _settings(1, 3, 1)
    want = _oracle(sc, camd, S, w, h, SPP, rect=(0, BAND[0], w, BAND[1]))[0]
    frames = {}
    for switch in (1, 0):
        t = _tracer(monkeypatch, switch, sc, camd, S, w, h); frames[switch] = _frame(t, SPP); t.close()
    for switch, got in frames.items():
        a, b = _bits(got[0])[BAND[0]:BAND[1]], _bits(want)[BAND[0]:BAND[1]]
        assert np.array_equal(a, b), "switch %d, rows %d..%d: %d pixels differ from the oracle" % (switch, BAND[0], BAND[1] - 1, int((a != b).any(-1).sum()))
    _assert_frames_equal(frames[1], frames[0], "%d batches, switch on against switch off" % batches)
    assert frames[1][2] > 0 and frames[0][2] == 0


# ---- 4. nothing to drop: every material can emit (the panel's 1e-9 on all of them: zero in binary16, "can emit" all the same)
@pytest.mark.parametrize("lp", [0, 1])
def test_all_emissive_scene_drops_nothing(lp, monkeypatch):
    sc = itc.all_emissive(_zoo()[0]); camd = _camera(W, H); S = _settings(lp, 2, 0)
    want = _oracle(sc, camd, S, W, H, SPP)
    t = _tracer(monkeypatch, 1, sc, camd, S, W, H); got = _frame(t, SPP); bits = t.inert_terminal()[0]; t.close()
    _assert_frames_equal(got, want, "all emissive, lp %d" % lp)
    assert got[2] == 0 and not (bits & itc.INERT_NO_LIGHT).any()


# ---- 5. somebody else observes a terminal hit: NEE-AT's shading kernels export a depth per hit
def test_neeat_and_depth_export_drop_nothing(monkeypatch):
    """With the baker in the loop every sample is a frame of its own: 1024 x 512 pixels, so that a sample's 524 288 paths keep the passes the bounce bound flags terminal
    above the classification threshold — the plain frame of the same context does drop there."""
    from rtxpt_amd import scenes
    w, h = 1024, 512
    sc, cam = _zoo(); camd = _camera(w, h); S = _settings(1, 2, 0)
    out = {}
    for switch in (1, 0):
        t = _tracer(monkeypatch, switch, sc, camd, S, w, h)
        plain = _frame(t, 1)
        t.set_neeat(True); t.set_view_projection(scenes.view_projection(w, h, **cam))
        out[switch] = (plain, _frame(t, 2)); t.close()
    print("dropped: plain %d / %d, NEE-AT with depth export %d / %d (switch on / off)" % (out[1][0][2], out[0][0][2], out[1][1][2], out[0][1][2]))
    assert out[1][0][2] > 0 and out[0][0][2] == 0      # the same context drops without NEE-AT ...
    assert out[1][1][2] == 0 and out[0][1][2] == 0      # ... and not with it
    _assert_frames_equal(out[1][0], out[0][0], "plain, switch on against switch off")
    _assert_frames_equal(out[1][1], out[0][1], "NEE-AT, switch on against switch off")


# ---- 6. the device's table against the predicate restated from the scene description
def test_device_table_follows_materials_and_light_links(monkeypatch):
    import rtxpt_amd as pt
    monkeypatch.setenv(SWITCH, "1")
    sc0, _ = itc.zoo(proxy_link=False)
    t = pt.PathTracer(test_hooks=True); t.set_scene(sc0)
    bits = t.inert_terminal()[0]
    assert np.array_equal(bits, itc.prim_bits(sc0)) and len(bits) == 40
    assert itc.inert(bits, 0).sum() == 10 + 12 + 2 and itc.inert(bits, 2).sum() == 10 + 2
    assert not (t.subinstances()[:, 3] != 0xFFFFFFFF).any()                   # no proxy link yet: the flag alone keeps the box out
    # a material edit: the white walls become emissive
    sc1 = dict(sc0); m = sc1["materials"].copy(); e = m["EmissiveColor"].copy(); e[0] = (0.0, 0.0, 0.25); m["EmissiveColor"] = e; sc1["materials"] = m
    t.set_scene(sc1); bits1 = t.inert_terminal()[0]
    assert np.array_equal(bits1, itc.prim_bits(sc1)) and not np.array_equal(bits1, bits) and (bits1[:6] & itc.INERT_NO_LIGHT).sum() == 0
    # a light bake that adds the proxy link (the instance now names its light), then one that only changes the lights
    sc2, _ = itc.zoo(proxy_link=True); sc2 = dict(sc2); sc2["materials"] = m
    t.set_scene(sc2); bits2 = t.inert_terminal()[0]
    assert (t.subinstances()[:, 3] != 0xFFFFFFFF).sum() == 1 and np.array_equal(bits2, itc.prim_bits(sc2))
    base, ex = sc2["lights"]; sc3 = dict(sc2); sc3["lights"] = (base[:2].copy(), ex[:2].copy())
    t.set_scene(sc3); bits3 = t.inert_terminal()[0]; t.close()
    assert np.array_equal(bits3, itc.prim_bits(sc3)) and np.array_equal(bits3, bits2)

"""The deferred radiance update of visible visibility rays on the device (run with -m gpu; rtxpt_amd/csrc/pt_trace.hip t8_shadow_body, t8_resolve_shadow_body): the
traversal loop only marks a visibility ray that ends visible (q2[i].w = 1), and the resolve pass behind every visibility launch — k_resolve_shadow, the visibility half of
k_resolve_pair — sweeps the launch's queue entries and adds the marked contributions to their paths (with the NEE-AT reservoir update and roulette fix-up, and into the
stable-plane fill pass's mark pool). Where the sum is made must not change anything: every comparison here is bit for bit against the CPU oracle rendering the same frame, ray
and hit counts included (the batch cases: a band of rows, counts against the serial-kernel frame) — through launch_shadow and launch_trace_pair, with and without the tail kernel, on a frame smaller than one block of the sweep, on a frame without
any visibility ray followed by one with them on the same context (no stale marks), on two and on four pipelined batches, with NEE-AT feedback, in the stable-plane fill pass and in the
grouped mode (NEEFullSamples > 1, which keeps k_resolve_nee and runs no sweep). Semantics preserved: the reference's Rtxpt/Shaders/PathTracer/PathTracerNEE.hlsli:185-275
(the light sample of a vertex lands before the emission of the next one is added)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

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


def _tracer(sc, camd, S, w, h, **kw):
    import rtxpt_amd as pt
    t = pt.PathTracer(**kw); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h)
    return t


def _frame(t, first, n):
    t.reset_accumulation(); st = t.render(first, n)
    return t.radiance(), (int(st["extendRays"]), int(st["shadowRays"]), int(st["hits"]))


def _assert_equal(got, want, what):
    a, b = _bits(got[0]), _bits(want[0])
    assert np.array_equal(a, b), "%s: %d pixels differ from the oracle" % (what, int((a != b).any(-1).sum()))
    assert got[1] == want[1], "%s: ray / hit counts %s, the oracle's %s" % (what, got[1], want[1])


# ---- 1. launch_shadow and launch_trace_pair, the serial-kernel frame, the tail kernel
def _bistro_case():
    from rtxpt_amd import scenes
    sc, cam = _bistro(); w, h = 320, 180
    camd = scenes.bridge_camera(w, h, **cam); S = scenes.default_settings(useFp16Types=1)
    return sc, camd, S, w, h, _once("bistro_320x180x2", lambda: _oracle(sc, camd, S, w, h, 0, 2))


@pytest.mark.parametrize("config", ["fused_0", "fused_1", "serial_kernels", "tail_0", "tail_32768"])
def test_launch_paths_match_oracle(config):
    sc, camd, S, w, h, want = _bistro_case()
    t = _tracer(sc, camd, S, w, h)
    if config == "fused_0": t.set_fused_traversal(0)
    elif config == "fused_1": t.set_fused_traversal(1)
    elif config == "serial_kernels": t.set_serial_kernels(True)
    elif config == "tail_0": t.set_tail_paths(0)
    else: t.set_tail_paths(32768)
    got = _frame(t, 0, 2); t.close()
    assert want[1][1] > 0
    _assert_equal(got, want, config)


# ---- 2. odd counts, a sweep shorter than one block
def _c2(nee, eye_shift=0.0):
    from rtxpt_amd import scenes
    sc, cam = scenes.cornell_box("C2"); S = scenes.config_settings("C2").copy(); S["NEEEnabled"] = nee
    if eye_shift:
        cam = dict(cam); e = np.array(cam["pos"], np.float32).copy(); e[0] += np.float32(eye_shift); cam["pos"] = e
    return sc, scenes.bridge_camera(33, 17, **cam), S


def test_small_odd_frame_matches_oracle():
    """33 x 17, 1 spp: 561 paths, every launch's queue count odd and most of them below the 256 entries of one block of the sweep"""
    sc, camd, S = _c2(1)
    want = _oracle(sc, camd, S, 33, 17, 0, 1)
    for fused in (0, 1):
        t = _tracer(sc, camd, S, 33, 17); t.set_fused_traversal(fused)
        got = _frame(t, 0, 1); t.close()
        assert want[1][1] > 0
        _assert_equal(got, want, "fused %d" % fused)


# ---- 3. a frame without visibility rays, and no stale marks. (No caller launches a sweep of no entries: without visibility rays finish_pass skips launch_shadow and
# nothing is pending for launch_trace_pair, so count == 0 in k_resolve_shadow<false> is valid by construction — the loop runs no iteration — and not reached here.)
def test_no_visibility_rays_then_a_moved_camera():
    sc, camd, S0 = _c2(0)
    t = _tracer(sc, camd, S0, 33, 17)
    got = _frame(t, 0, 1)
    assert got[1][1] == 0
    _assert_equal(got, _oracle(sc, camd, S0, 33, 17, 0, 1), "NEEEnabled=0")
    # marks of earlier frames stay in the queue's memory; the first frame with NEE leaves thousands, the moved camera's frame must not see them
    sc, camd, S1 = _c2(1)
    t.set_settings(S1); _frame(t, 0, 1)
    sc, camd2, S1 = _c2(1, eye_shift=0.125)
    t.set_camera(camd2); again = _frame(t, 0, 1); t.close()
    f = _tracer(sc, camd2, S1, 33, 17); fresh = _frame(f, 0, 1); f.close()
    assert np.array_equal(_bits(again[0]), _bits(fresh[0])) and again[1] == fresh[1]
    _assert_equal(again, _oracle(sc, camd2, S1, 33, 17, 0, 1), "moved camera")


# ---- 4. pipelined batches: every batch has its own slice of the shadow queue (slice_batch: q0..q3 + base x entries per path) and its own sweep with its own count
BAND = (228, 292)      # the rows compared with the oracle: 64 rows across the middle of the frame, where a batch's owned pixels end and the next one's begin


@pytest.mark.parametrize("spp,batches", [(2, 2), (4, 4)])
def test_pipelined_batches_match_oracle_band(spp, batches):
    """1024 x 520 at 2 spp is 1 064 960 paths per call, at 4 spp 2 129 920: pt_frame.hip batch_count gives one batch below 1 << 20 paths, PT_PIPELINE_MID_BATCHES = 2 below
    PT_PIPELINE_FULL_AT = 1 << 21, PT_PIPELINE_BATCHES = 4 from there (where the batches' traversal launches, launch_trace_pair's among them, run under a grid bound).
    The frame's rows 228..291 against the oracle, bit for bit. The tracer reports no counts per rectangle, so ray and hit counts are NOT held to the oracle here: they, and
    the whole frame, are held to the same build's serial-kernel frame (one batch, one stream, launches of their own), which case 1 holds to the oracle at a smaller size."""
    from rtxpt_amd import scenes
    sc, cam = _bistro(); w, h = 1024, 520
    assert "MI355PT_BATCHES" not in os.environ
    assert batches == (1 if w * h * spp < (1 << 20) else 2 if w * h * spp < (1 << 21) else 4)
    camd = scenes.bridge_camera(w, h, **cam); S = scenes.default_settings(useFp16Types=1)
    want = _oracle(sc, camd, S, w, h, 0, spp, rect=(0, BAND[0], w, BAND[1]))[0]
    t = _tracer(sc, camd, S, w, h); got = _frame(t, 0, spp)
    t.set_serial_kernels(True); one = _frame(t, 0, spp); t.close()
    a, b = _bits(got[0])[BAND[0]:BAND[1]], _bits(want)[BAND[0]:BAND[1]]
    assert np.array_equal(a, b), "rows %d..%d: %d pixels differ from the oracle" % (BAND[0], BAND[1] - 1, int((a != b).any(-1).sum()))
    assert got[1][1] > 0 and np.array_equal(_bits(got[0]), _bits(one[0])) and got[1] == one[1]


# ---- 5. NEE-AT feedback: the reservoir update and the roulette fix-up move with the contribution
def test_neeat_feedback_frame():
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    import pin_scenes
    name = "bistro_like_neeat_lp16"
    make, S, w, h, first, n, opts = pin_scenes.neeat_cases()[name]
    assert opts["feedback"] and int(S["NEEFullSamples"]) == 1
    sc, cam = make()
    out = []
    for serial in (False, True):
        t = pt.PathTracer(); t.set_scene(sc); t.set_settings(S); t.set_camera(scenes.bridge_camera(w, h, **cam)); t.resize(w, h)
        baked = len(t.lights()["lights"])
        t.set_local_light_sampling(pin_scenes.neeat_table(opts, baked, w, h), jitter=opts["jitter"], ratio=opts["ratio"], ssc_threshold=opts["ssc_threshold"], feedback=True)
        t.set_serial_kernels(serial); st = t.render(first, n)
        out.append((t.radiance(), (int(st["extendRays"]), int(st["shadowRays"])), [t.light_feedback(s) for s in range(n)])); t.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and out[0][1] == out[1][1]
    for (w0, c0), (w1, c1) in zip(out[0][2], out[1][2]): assert np.array_equal(_bits(w0), _bits(w1)) and np.array_equal(c0, c1)
    g = np.load(os.path.join(ROOT, "tests", "golden", "neeat_golden.npz"))
    assert name in g.files
    for frame, rays, fb in out:
        assert np.array_equal(_bits(frame), _bits(g[name])), "the frame differs from the reference text's"
        assert rays == tuple(int(v) for v in g[name + "_rays"])
        for s, (wgt, cand) in enumerate(fb):
            assert np.array_equal(_bits(wgt), _bits(g["%s_fbw%d" % (name, s)])) and np.array_equal(cand, g["%s_fbc%d" % (name, s)]), "feedback reservoirs of sample %d" % s


# ---- 6. the stable-plane fill pass: the visible entries land in its mark pool
def _live(out, w, h):
    from rtxpt_amd import scenes
    hd = out["header"]; P = out["planes"].reshape(-1, 20); rows = []
    for pl in range(3):
        ys, xs = np.nonzero(hd[pl] != 0xFFFFFFFF)
        for x, y in zip(xs.tolist(), ys.tolist()): rows.append(P[scenes.stable_planes_address(x, y, pl, w, h)])
    return np.array(rows, np.uint32)


def test_stable_plane_fill_matches_oracle():
    from rtxpt_amd import scenes
    from oracle import ptref
    w, h, sample, subs = 320, 180, 2, 2
    sc, cam = scenes.stable_planes_zoo(); S = scenes.config_settings("C2"); S["useFp16Types"] = 1
    camd = scenes.bridge_camera(w, h, **cam)
    prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam), sub_samples=subs)
    o = ptref.Oracle(lp16=True); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h)
    want = o.build_stable_planes(sample, prm); c0 = o.counters()
    for s in range(subs): o.fill_stable_planes(sample + s, prm, want)
    c1 = o.counters(); o.close()
    t = _tracer(sc, camd, S, w, h)
    t.build_stable_planes(sample, prm)
    got = t.fill_stable_planes(sample, prm, sub_samples=subs); t.close()
    assert c1["shadowRays"] - c0["shadowRays"] > 0
    assert np.array_equal(got["header"], want["header"])
    assert np.array_equal(_live(got, w, h), _live(want, w, h)), "plane records (noisy radiance included)"
    assert np.array_equal(got["spec_hit_t"].view(np.uint32), want["spec_hit_t"].view(np.uint32))
    assert (int(got["stats"]["extendRays"]), int(got["stats"]["shadowRays"])) == (c1["extendRays"] - c0["extendRays"], c1["shadowRays"] - c0["shadowRays"])


# ---- 7. the grouped mode: marks in the loop as before, k_resolve_nee folds them, no sweep
def test_grouped_nee_samples_match_oracle():
    from rtxpt_amd import scenes
    sc, cam = _bistro(); w, h = 160, 90
    camd = scenes.bridge_camera(w, h, **cam); S = scenes.default_settings(useFp16Types=1, NEEFullSamples=2)
    want = _oracle(sc, camd, S, w, h, 0, 2)
    t = _tracer(sc, camd, S, w, h); got = _frame(t, 0, 2); t.close()
    assert want[1][1] > 0
    _assert_equal(got, want, "NEEFullSamples=2")

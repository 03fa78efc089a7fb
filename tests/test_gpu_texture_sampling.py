"""The texture samplers at non-power-of-two and thin sizes, GPU half (tests/test_texture_sampling.py is the CPU half): the device's pt_scene.h samplers through probe 11
against the oracle's bit for bit and against the float64 restatement within the derived bound, the traversal's alpha test on byte and float alpha planes, traced rays
through alpha-tested quads, a whole frame of a room of such textures, and the far range (2^25 <= |u * dim| <= 2^30 on sides that are no power of two)."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rtxpt_amd import scenes
from oracle import ptref
import texture_cases as tc
import texture_ref as tr
from test_texture_sampling import alpha_reference, dm, worst_ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    import rtxpt_amd as pt
    sc, texs, quads = tc.zoo()
    g = pt.PathTracer(test_hooks=True); g.set_scene(sc); g.set_settings(scenes.default_settings())
    g.set_camera(scenes.bridge_camera(8, 8, pos=(9, 0.5, -4), direction=(0, 0, 1), up=(0, 1, 0), fov_y=1.0)); g.resize(8, 8)
    yield g
    g.close()


@pytest.fixture(scope="module")
def oracle():
    sc, texs, quads = tc.zoo()
    o = ptref.Oracle(); o.set_scene(sc); o.set_settings(scenes.default_settings()); o.resize(8, 8)
    return o


@pytest.fixture(scope="module")
def mips():
    pw = dm(5)
    return [tr.build_mips(tr.level0(t.pixels, t.upload, pow32=pw)) for t in tc.zoo()[1]]


def _bitwise(device, oracle, rows_of):
    sc, texs, quads = tc.zoo(); total = 0
    for t in texs:
        rows = rows_of(t)
        if not len(rows): continue
        got = device.probe(11, rows, (len(rows), 4)); want = oracle.texture_probe(rows); total += len(rows)
        bad = (got.view(np.uint32) != want.view(np.uint32)).any(1)
        assert not bad.any(), "%s: %d of %d rows differ; first: row %s device %s oracle %s" % (t.name, int(bad.sum()), len(rows), rows[bad][0].tolist(), got[bad][0], want[bad][0])
        yield t, rows, got
    assert total > 0


def test_device_samplers_equal_the_oracle_and_hold_the_derived_bound(device, oracle, mips):
    for t, rows, got in _bitwise(device, oracle, tc.near_rows):
        worst, (i, c) = worst_ratio(got, t, mips[t.index], rows)
        print("device %-26s %5d rows, largest error / bound %.3f (row %d mode %d channel %d)" % (t.name, len(rows), worst, i, rows[i, 0], c))
        assert worst <= 1.0, (t.name, worst, rows[i].tolist())


def test_device_samplers_equal_the_oracle_in_the_far_range(device, oracle, mips):
    for t, rows, got in _bitwise(device, oracle, tc.far_rows):
        worst, (i, c) = worst_ratio(got, t, mips[t.index], rows)
        print("device far %-26s %5d rows, largest error / bound %.3f" % (t.name, len(rows), worst))
        assert worst <= 1.0, (t.name, worst, rows[i].tolist())


def test_device_alpha_test_agrees_with_the_float64_opacity(device, mips):
    """Probe 10 (alpha_test_slot through the build-time AlphaRec and the byte / float alpha planes) on 20 000 candidates: wherever the float64 opacity is further from the
    cutoff than the derived bound — at least 99 % of them — the device decides as the reference does."""
    rows = tc.alpha_candidates(); opaque, decided = alpha_reference(rows, mips)
    got = device.probe(10, rows, (len(rows), 2), out_dtype=np.uint32)
    assert decided.mean() >= 0.99
    bad = decided & ((got[:, 0] != 0) != opaque)
    assert not bad.any(), "%d of %d decided candidates differ; first: %s" % (int(bad.sum()), int(decided.sum()), rows[bad][0].tolist())
    assert np.array_equal(got[:, 0], got[:, 1])                                 # no ExcludeFromNEE geometry here: visibility rays see the same answer
    print("alpha probe: %d of %d candidates counted, %d opaque" % (int(decided.sum()), len(rows), int(opaque.sum())))


def test_traced_rays_through_alpha_tested_quads_equal_the_oracle(device, oracle):
    """The copy of the alpha test inside the traversal loop: closest hits and visibility of ~20 000 rays, each through up to five alpha-tested quads."""
    rays = tc.through_rays()
    hits, _ = device.trace_closest(rays); want = oracle.trace_closest(rays)
    assert np.array_equal(hits.view(np.uint32), want.view(np.uint32))
    miss = hits.view(np.uint32)[:, 1] == 0xFFFFFFFF
    assert 0.01 < miss.mean() < 0.6                                           # some rays pass all five layers, most are stopped somewhere
    layer = (hits.view(np.uint32)[~miss, 1] >> 1) % len(tc.FORMATS)
    assert all((layer == f).sum() > 100 for f in range(len(tc.FORMATS)))       # every format's layer stops some and lets others through
    vrays = rays.copy(); vrays[:, 7] = 3.0
    vis, _ = device.trace_visibility(vrays)
    assert np.array_equal(vis, oracle.trace_visibility(vrays)) and 0 < int(vis.sum()) < len(vis)


@pytest.mark.parametrize("fp16", [0, 1])
def test_room_frame_equals_the_oracle(fp16):
    import rtxpt_amd as pt
    sc, cam = tc.room(); w, h = 64, 48
    S = scenes.default_settings(useFp16Types=fp16); camd = scenes.bridge_camera(w, h, **cam)
    o = ptref.Oracle(lp16=bool(fp16)); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h); o.render(0, 2)
    want = o.radiance(); c = o.counters()
    assert np.isfinite(want).all() and (want[..., :3] > 0).mean() > 0.5
    for tail in (0, 4096):
        g = pt.PathTracer(); g.set_scene(sc); g.set_camera(camd); g.set_settings(S); g.resize(w, h); g.set_tail_paths(tail)
        st = g.render(0, 2); got = g.radiance()
        bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
        assert not bad.any(), "useFp16Types %d, tail %d: %d of %d pixels differ" % (fp16, tail, int(bad.sum()), bad.size)
        assert (st["extendRays"], st["shadowRays"], st["hits"]) == (c["extendRays"], c["shadowRays"], c["hits"])
        if tail == 0:      # the emissive bake: the anisotropic filter on a w != h texture
            Lg, Lo = g.lights(), o.lights()
            assert all(np.array_equal(Lg[k], Lo[k]) for k in ("lights", "lightsEx", "proxyCounters", "proxyIndices"))
            assert sum(((r[3] >> 24) & 0xF) == 1 for r in Lg["lights"]) == 2
        g.close()

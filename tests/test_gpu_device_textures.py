"""The texture pool made on the device (PT_DEVICE_TEXTURES_ON_DEVICE, rtxpt_amd/csrc/pt_texture_ingest.hip) and pt_update_texture: every level, every alpha plane and both
tables bit for bit the host path's and the float32 restatement's (tests/texture_ingest_ref.py); the samplers, the alpha test, traced rays, the emissive bake and a whole frame
on the device-made pool against the oracle; one texture replaced in place against a fresh scene; an environment change that leaves the material textures alone; and the shape
of an ingest — what it keeps on the host and how many kernels it launches."""
import contextlib
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rtxpt_amd as pt
from rtxpt_amd import scenes
from oracle import ptref
import texture_cases as tc
import texture_ref as tr
import texture_ingest_ref as ti
from test_texture_sampling import alpha_reference, dm, worst_ratio
from test_gpu_texture_sampling import _bitwise

pytestmark = pytest.mark.gpu

STAGING_DEFAULT = 64 << 20          # PT_TEXTURE_STAGING_BYTES


@contextlib.contextmanager
def _environment(**kv):
    """The two switches pt_create reads, set for one context only (None: unset — the flag of PtDeviceDesc alone decides)."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def context(scene, on, staging=None, hooks=True):
    with _environment(MI355PT_DEVICE_TEXTURES=None, MI355PT_TEXTURE_STAGING_BYTES=staging):
        g = pt.PathTracer(test_hooks=hooks, device_textures=on)
    g.set_scene(scene); g.set_settings(scenes.default_settings())
    g.set_camera(scenes.bridge_camera(8, 8, pos=(9, 0.5, -4), direction=(0, 0, 1), up=(0, 1, 0), fov_y=1.0)); g.resize(8, 8)
    return g


def pool_of(g, texs):
    """Everything the read-backs return: per texture (levels, (plane fmt, plane)); asking for one level more is refused."""
    out = []
    for t in texs:
        levels = [g.texture_level(t.index, l) for l in range(t.levels)]
        with pytest.raises(pt.PtError): g.texture_level(t.index, t.levels)
        out.append((levels, g.alpha_plane(t.index)))
    with pytest.raises(pt.PtError): g.texture_level(len(texs), 0)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_pools_equal(got, want, texs, who):
    assert len(got) == len(want) == len(texs)
    for t, (gl, (gf, gp)), (wl, (wf, wp)) in zip(texs, got, want):
        assert len(gl) == len(wl) == t.levels, (who, t.name)
        for l, (a, b) in enumerate(zip(gl, wl)):
            assert a.shape == b.shape == (max(1, t.h >> l), max(1, t.w >> l), 4), (who, t.name, l, a.shape, b.shape)
            assert same_bits(a, b), "%s: %s level %d: %d texels differ" % (who, t.name, l, int((a.view(np.uint32) != b.view(np.uint32)).any(-1).sum()))
        assert gf == wf, (who, t.name, "plane format", gf, wf)
        assert same_bits(gp, wp), (who, t.name, "alpha plane")


@pytest.fixture(scope="module")
def pow32(): return dm(5)


@pytest.fixture(scope="module")
def zoo_device():
    g = context(tc.zoo()[0], True); yield g; g.close()


@pytest.fixture(scope="module")
def oracle():
    o = ptref.Oracle(); o.set_scene(tc.zoo()[0]); o.set_settings(scenes.default_settings()); o.resize(8, 8)
    return o


@pytest.fixture(scope="module")
def mips(pow32):
    return [tr.build_mips(tr.level0(t.pixels, t.upload, pow32=pow32)) for t in tc.zoo()[1]]


def test_levels_and_planes_equal_the_host_path(zoo_device, pow32):
    sets = [("zoo", tc.zoo()[0], tc.zoo()[1]), ("ingest", ti.ingest_set().scene, ti.ingest_set().texs), ("small", ti.many_small().scene, ti.many_small().texs)]
    for name, scene, texs in sets:
        host = context(scene, False); dev = zoo_device if name == "zoo" else context(scene, True)
        sh, sd = host.texture_ingest_stats(), dev.texture_ingest_stats()
        assert (sh["onDevice"], sd["onDevice"]) == (0, 1)
        ph, pd = pool_of(host, texs), pool_of(dev, texs)
        assert_pools_equal(pd, ph, texs, name + ": device path against host path")
        assert_pools_equal(pd, ti.reference(name, pow32), texs, name + ": device path against the restatement")
        assert sh["poolTexels"] == sd["poolTexels"] == sum(l.shape[0] * l.shape[1] for levels, _ in ph for l in levels)      # the same layout: no gaps, the same total
        assert sh["level0Texels"] == sd["level0Texels"] == sum(t.w * t.h for t in texs) and sh["sourceBytes"] == sd["sourceBytes"] == sum(np.asarray(t.pixels).nbytes for t in texs)
        host.close()
        if dev is not zoo_device: dev.close()


def test_samplers_and_alpha_test_equal_the_oracle(zoo_device, oracle, mips):
    for rows_of in (tc.near_rows, tc.far_rows):
        for t, rows, got in _bitwise(zoo_device, oracle, rows_of):
            worst, (i, c) = worst_ratio(got, t, mips[t.index], rows)
            assert worst <= 1.0, (t.name, worst, rows[i].tolist())
    rows = tc.alpha_candidates(); opaque, decided = alpha_reference(rows, mips)
    got = zoo_device.probe(10, rows, (len(rows), 2), out_dtype=np.uint32)
    assert decided.mean() >= 0.99
    bad = decided & ((got[:, 0] != 0) != opaque)
    assert not bad.any(), "%d of %d decided candidates differ; first: %s" % (int(bad.sum()), int(decided.sum()), rows[bad][0].tolist())
    assert np.array_equal(got[:, 0], got[:, 1])


def _traced(g):
    rays = tc.through_rays(); vrays = rays.copy(); vrays[:, 7] = 3.0
    return g.trace_closest(rays)[0].view(np.uint32), g.trace_visibility(vrays)[0]


def _room_frame(sc, fp16, on):
    cam = tc.room()[1]; w, h = 64, 48
    S = scenes.default_settings(useFp16Types=fp16); camd = scenes.bridge_camera(w, h, **cam)
    with _environment(MI355PT_DEVICE_TEXTURES=None):
        g = pt.PathTracer(device_textures=on)
    g.set_scene(sc); g.set_camera(camd); g.set_settings(S); g.resize(w, h)
    return g, S, camd


def test_traced_rays_and_room_frame(zoo_device, oracle):
    rays = tc.through_rays(); vrays = rays.copy(); vrays[:, 7] = 3.0
    hits, vis = _traced(zoo_device)
    assert np.array_equal(hits, oracle.trace_closest(rays).view(np.uint32)) and np.array_equal(vis, oracle.trace_visibility(vrays)) and 0 < int(vis.sum()) < len(vis)
    sc = tc.room()[0]; w, h = 64, 48
    for fp16 in (0, 1):
        g, S, camd = _room_frame(sc, fp16, True)
        assert g.texture_ingest_stats()["onDevice"] == 1
        o = ptref.Oracle(lp16=bool(fp16)); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h); o.render(0, 2)
        want = o.radiance(); c = o.counters()
        st = g.render(0, 2); got = g.radiance()
        bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
        assert not bad.any(), "useFp16Types %d: %d of %d pixels differ" % (fp16, int(bad.sum()), bad.size)
        assert (st["extendRays"], st["shadowRays"], st["hits"]) == (c["extendRays"], c["shadowRays"], c["hits"])
        Lg, Lo = g.lights(), o.lights()      # the emissive bake reads the device-made texels
        assert all(np.array_equal(Lg[k], Lo[k]) for k in ("lights", "lightsEx", "proxyCounters", "proxyIndices"))
        g.close()


def _new_pixels(t, seed, fmt=None):
    r = tc._rng("update", t.index, seed); fmt = fmt or t.fmt
    if fmt in ("srgb8", "unorm8"): return r.integers(0, 256, (t.h, t.w, 4)).astype(np.uint8)
    px = np.exp(1.5 * r.standard_normal((t.h, t.w, 4))).astype(np.float32)
    if fmt == "f32_alpha_bytes": px[..., 3] = r.integers(0, 256, (t.h, t.w)).astype(np.float32) / np.float32(255.0)
    else: px[..., 3] = r.random((t.h, t.w), np.float32) * np.float32(0.999) + np.float32(0.0005)
    return px


def _with_textures(sc, new):
    out = dict(sc); out["textures"] = [(w, h, fmt, new.get(i, px)) for i, (w, h, fmt, px) in enumerate(sc["textures"])]
    return out


def test_update_texture_equals_a_fresh_scene():
    sc, texs, quads = tc.zoo(); nf = len(tc.FORMATS)
    col = tc.SIZES.index((100, 60)); pick = [texs[col * nf + tc.FORMATS.index(f)] for f in ("srgb8", "unorm8", "f32_alpha_floats")]
    small = texs[tc.SIZES.index((5, 4)) * nf + tc.FORMATS.index("f32_alpha_bytes")]      # its byte plane (20 bytes) sits between other planes
    new = {t.index: _new_pixels(t, 1) for t in pick}
    rows = tc.alpha_candidates()
    for on in (True, False):
        g = context(sc, on); hits0, vis0 = _traced(g); build0 = g.build_stats()["buildMs"]
        before = pool_of(g, texs)
        for t in pick: g.update_texture(t.index, new[t.index])
        st = g.texture_ingest_stats()
        fresh = context(_with_textures(sc, new), on)
        want = pool_of(fresh, texs); got = pool_of(g, texs)
        assert_pools_equal(got, want, texs, "updated against fresh, device textures %s" % on)
        for t in texs:
            if t.index in new: assert not same_bits(got[t.index][0][0], before[t.index][0][0]), t.name                      # the update did arrive
            else: assert_pools_equal([got[t.index]], [before[t.index]], [t], "untouched texture")
        assert np.array_equal(g.probe(10, rows, (len(rows), 2), out_dtype=np.uint32), fresh.probe(10, rows, (len(rows), 2), out_dtype=np.uint32))
        hits, vis = _traced(g); fh, fv = _traced(fresh)
        assert np.array_equal(hits, fh) and np.array_equal(vis, fv) and not np.array_equal(hits, hits0)
        if on:
            assert g.build_stats()["buildMs"] == build0, "pt_update_texture built the BVH again"      # the time of the one and only build
            assert st["onDevice"] == 1 and st["level0Texels"] == pick[-1].w * pick[-1].h and st["launches"] <= 15 + 4 + 2 * st["stagingChunks"]
        # a byte plane that receives opacities other than k / 255 becomes a float plane (here the geometry may be finalised again); the reverse keeps the float plane
        assert g.alpha_plane(small.index)[0] == 0
        switched = dict(new); switched[small.index] = _new_pixels(small, 2, "f32_alpha_floats")
        g.update_texture(small.index, switched[small.index])
        fresh2 = context(_with_textures(sc, switched), on)
        assert g.alpha_plane(small.index)[0] == 1
        assert_pools_equal(pool_of(g, texs), pool_of(fresh2, texs), texs, "byte plane to float plane, device textures %s" % on)
        assert np.array_equal(g.probe(10, rows, (len(rows), 2), out_dtype=np.uint32), fresh2.probe(10, rows, (len(rows), 2), out_dtype=np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(_traced(g), _traced(fresh2)))
        back = _new_pixels(small, 3, "f32_alpha_bytes"); g.update_texture(small.index, back)
        fmt, plane = g.alpha_plane(small.index)
        assert fmt == (1 if on else 0) and (not on or same_bits(plane, back[..., 3].ravel()))
        # refused: another size, another format, no such texture
        t = pick[0]
        for bad in (lambda: g.update_texture(t.index, np.zeros((t.h, t.w + 1, 4), np.uint8)), lambda: g.update_texture(t.index, np.zeros((t.h, t.w, 4), np.float32)),
                    lambda: g.update_texture_desc(t.index, new[t.index], pt.PT_TEX_RGBA8_UNORM), lambda: g.update_texture(len(texs), new[t.index])):
            with pytest.raises(pt.PtError) as e: bad()
            assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT
        for c in (g, fresh, fresh2): c.close()
    # the emissive texture of the room: the lights are baked again from the new texels, the frame follows
    rsc = tc.room()[0]; emissive = 10                     # texture_cases.room(): five base-colour maps, five normal maps, then the emissive texture
    assert rsc["textures"][emissive][:3] == (100, 60, scenes.TEX_RGBA32F)
    glow = np.exp(0.8 * tc._rng("update", "glow").standard_normal((60, 100, 4))).astype(np.float32)
    g, S, camd = _room_frame(rsc, 0, True); g.render(0, 2); before = g.radiance(); build0 = g.build_stats()["buildMs"]
    g.update_texture(emissive, glow); g.reset_accumulation(); g.render(0, 2)
    f, _, _ = _room_frame(_with_textures(rsc, {emissive: glow}), 0, True); f.render(0, 2)
    Lg, Lf = g.lights(), f.lights()
    assert all(np.array_equal(Lg[k], Lf[k]) for k in ("lights", "lightsEx", "proxyCounters", "proxyIndices"))
    assert same_bits(g.radiance(), f.radiance()) and not same_bits(g.radiance(), before) and g.build_stats()["buildMs"] == build0
    g.close(); f.close()


def test_environment_change_leaves_material_textures_alone():
    rsc = dict(tc.room()[0]); r = tc._rng("env")
    env = lambda w, h: ((r.random((h, w, 3)) * 2.0).astype(np.float32), np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), np.float32([1.0, 1.0, 1.0]))
    first, second = env(16, 8), env(64, 32)               # the second does not fit the room the pool left for the first
    rsc["env"] = first; rsc["env_cube_dim"] = 64
    texs = [tc.Tex(i, w, h, "", px, fmt, 0) for i, (w, h, fmt, px) in enumerate(rsc["textures"])]
    g, S, camd = _room_frame(rsc, 0, True); g.render(0, 2)
    stats = g.texture_ingest_stats(); pool = pool_of(g, texs); first_frame = g.radiance()
    assert stats["onDevice"] == 1 and stats["level0Texels"] == sum(t.w * t.h for t in texs)
    g.set_environment(second); g.reset_accumulation(); g.render(0, 2)
    assert g.texture_ingest_stats() == stats, "an environment change ran a texture ingest"      # times included: the very same ingest
    assert_pools_equal(pool_of(g, texs), pool, texs, "after the environment change")
    fsc = dict(rsc); fsc["env"] = second
    f, _, _ = _room_frame(fsc, 0, True); f.render(0, 2)
    assert same_bits(g.radiance(), f.radiance()) and not same_bits(g.radiance(), first_frame)
    h, _, _ = _room_frame(fsc, 0, False); h.render(0, 2)                                     # and the host path agrees about that frame
    assert same_bits(f.radiance(), h.radiance())
    for c in (g, f, h): c.close()


def test_ingest_shape(zoo_device, pow32):
    for name, s, staging in (("zoo", None, None), ("small", ti.many_small(), None), ("small", ti.many_small(), 1000), ("ingest", ti.ingest_set(), 1 << 16)):
        scene, texs = (tc.zoo()[0], tc.zoo()[1]) if s is None else (s.scene, s.texs)
        host = context(scene, False); dev = zoo_device if (s is None) else context(scene, True, staging)
        sh, sd = host.texture_ingest_stats(), dev.texture_ingest_stats()
        print(name, staging, sd, "host path holds", sh["hostBytesHeld"])
        assert sd["onDevice"] == 1 and sh["onDevice"] == 0
        assert sd["sourceBytes"] == sum(np.asarray(t.pixels).nbytes for t in texs)
        assert sd["hostBytesHeld"] <= (staging or STAGING_DEFAULT) + sd["sourceBytes"]
        assert 4 * sd["hostBytesHeld"] <= sh["hostBytesHeld"] and sh["hostBytesHeld"] >= 16 * sd["level0Texels"]
        assert sd["stagingChunks"] >= 1 and sd["launches"] <= 15 + 4 + 2 * sd["stagingChunks"]
        if staging:
            assert sd["stagingChunks"] >= sd["sourceBytes"] // staging                      # the override took: pieces of at most half the buffer
            assert_pools_equal(pool_of(dev, texs), ti.reference(name, pow32), texs, "%s with %d bytes of staging" % (name, staging))
            assert_pools_equal(pool_of(dev, texs), pool_of(host, texs), texs, "%s with %d bytes of staging, against the host path" % (name, staging))
        host.close()
        if dev is not zoo_device: dev.close()

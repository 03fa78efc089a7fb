"""Stochastic texture filtering on the device (run with -m gpu; tests/test_stf_reference.py is the CPU half): probe 12 against the numpy restatement tests/stf_ref.py and the
texels the device itself stores, the random source against the sample-stream probe, frames of constant textures bit-equal with the filter on and off on every route that
loads a surface (shading kernels, tail kernel, stable-plane build and fill), determinism and keying by (pixel, vertex, sample) on a textured room, convergence of the LINEAR
frame to the trilinear frame at the rate of an unbiased estimator, and the interface's refusals."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rtxpt_amd import scenes
import texture_cases as tc
import stf_ref as sr

pytestmark = pytest.mark.gpu
FILTERS = [sr.POINT, sr.LINEAR, sr.CUBIC]


def _same(a, b): return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.fixture(scope="module")
def device():
    import rtxpt_amd as pt
    sc, texs, quads = tc.zoo()
    g = pt.PathTracer(test_hooks=True); g.set_scene(sc); g.set_settings(scenes.default_settings())
    g.set_camera(scenes.bridge_camera(8, 8, pos=(9, 0.5, -4), direction=(0, 0, 1), up=(0, 1, 0), fov_y=1.0)); g.resize(8, 8)
    yield g
    g.close()


@pytest.fixture(scope="module")
def stored(device):
    """Every level of every texture of the zoo as the device stores it (pt_get_texture_level), read once."""
    return [[device.texture_level(t.index, l) for l in range(t.levels)] for t in tc.zoo()[1]]


@pytest.mark.parametrize("filt", FILTERS)
def test_probe_equals_the_restatement_and_returns_stored_texels(device, stored, filt):
    texs = tc.zoo()[1]
    per = [(t, sr.probe_rows(t, filt, tc.material_rows)) for t in texs]
    rows = np.concatenate([r for _, r in per])
    got = device.probe(12, rows, (len(rows), 8), out_dtype=np.uint32); at = 0
    for t, rr in per:
        g = got[at:at + len(rr)]; at += len(rr)
        mip, x, y = sr.pick_rows(t, rr)
        bad = (g[:, 4] != mip) | (g[:, 5] != x) | (g[:, 6] != y)
        assert not bad.any(), "%s filter %d: %d of %d rows differ; first: %s device %s restatement %s" % (t.name, filt, int(bad.sum()), len(rr), rr[bad][0].tolist(), g[bad][0, 4:7].tolist(), [int(mip[bad][0]), int(x[bad][0]), int(y[bad][0])])
        texel = np.zeros((len(rr), 4), np.float32)
        for l in np.unique(mip): k = mip == l; texel[k] = stored[t.index][l][y[k], x[k]]
        assert np.array_equal(g[:, :4], texel.view(np.uint32)), (t.name, filt)
        assert not g[:, 7].any()
    print("filter %d: %d rows" % (filt, len(rows)))


def test_probe_refuses_what_the_scene_does_not_have(device):
    t = tc.zoo()[1][0]; ok = sr.rows12(t.word, [0.5], [0.5], 0.0, sr.LINEAR, np.zeros((1, 4), np.float32))
    for col, val in ((0, 2), (1, (t.word & 0xFFFF0000) | 0xFFFF), (5, 3)):
        bad = ok.copy(); bad[0, col] = val
        with pytest.raises(Exception): device.probe(12, bad, (1, 8), out_dtype=np.uint32)
    device.probe(12, ok, (1, 8), out_dtype=np.uint32)


def test_random_source_is_the_sample_stream_of_pixel_vertex_and_sample(device):
    """Probe 12 mode 1 == the first four numbers of probe 2's stream for the same (pixel, vertex, sample): SampleGenerator over the vertex base, effect seed Base, uniform mode."""
    r = np.random.default_rng(12); n = 600
    px = ((r.integers(0, 4096, n) << 16) | r.integers(0, 4096, n)).astype(np.uint32); vx = r.integers(0, 48, n).astype(np.uint32); sm = r.integers(0, 1 << 24, n).astype(np.uint32)
    a = np.zeros((n, 12), np.uint32); a[:, 0] = 1; a[:, 6] = px; a[:, 7] = vx; a[:, 8] = sm
    b = np.zeros((n, 6), np.uint32); b[:, 0] = px; b[:, 1] = vx; b[:, 2] = sm; b[:, 3] = 0; b[:, 4] = 3; b[:, 5] = 4
    got = device.probe(12, a, (n, 8), out_dtype=np.uint32); want = device.probe(2, b, (n, 8))
    assert np.array_equal(got[:, :4], want[:, :4].view(np.uint32)) and not got[:, 4:].any()
    u = got[:, :4].copy().view(np.float32); assert (u >= 0).all() and (u < 1).all() and len(np.unique(u)) > 4 * n - 8


# ---- frames
def _constant_textured_scene():
    """Materials whose base, normal, metal-rough and emissive lookups all read constant textures of odd sizes: whichever texel a filter picks holds the same value."""
    b = scenes.SceneBuilder()
    const = lambda w, h, v: b.add_texture(np.tile(np.float32(v), (h, w, 1)), scenes.TEX_RGBA32F)
    base, nrm, mr, glow = const(100, 60, (0.5, 0.25, 0.75, 1.0)), const(5, 4, (0.5, 0.5, 1.0, 1.0)), const(64, 2, (1.0, 0.5, 0.25, 1.0)), const(257, 129, (0.25, 3.5, 0.0029296875, 0.625))
    def add(corners, mat, uv_scale):
        p, i, uv, n, tg = scenes.quad(*corners)
        b.begin_mesh(); b.add_geometry(p, i, mat, uv=(uv * np.float32(uv_scale)).astype(np.float32), normal=n, tangent=tg); b.add_instance(b.end_mesh())
    add(([-4, 0, -4], [-4, 0, 8], [4, 0, 8], [4, 0, -4]), b.add_material(scenes.make_material(base=(0.9, 0.9, 0.9), base_tex=base, normal_tex=nrm, roughness=0.6)), (3.0, 2.0))
    add(([-2, 0, 3], [-2, 1.5, 3], [2, 1.5, 3], [2, 0, 3]), b.add_material(scenes.make_material(base=(0.8, 0.8, 0.8), base_tex=base, roughness=0.2)), (2.0, -1.5))
    add(([-1.5, 2.5, 0.5], [1.5, 2.5, 0.5], [1.5, 2.5, 4.0], [-1.5, 2.5, 4.0]), b.add_material(scenes.make_material(base=(0.5, 0.5, 0.5), emissive=(6.0, 5.0, 4.0), emissive_tex=glow)), (1.7, 0.9))
    return b.finish(), dict(pos=(0.3, 0.12, -2.5), direction=(-0.05, -0.02, 1.0), up=(0, 1, 0), fov_y=1.0)


def _tracer(sc, cam, w, h, S, **kw):
    import rtxpt_amd as pt
    g = pt.PathTracer(**kw); g.set_scene(sc); g.set_camera(scenes.bridge_camera(w, h, **cam)); g.set_settings(S); g.resize(w, h)
    return g


CONSTANT_SCENES = {"texture_cases.constant_scene": lambda: (tc.constant_scene()[0], dict(pos=(0.5, 0.5, -2.0), direction=(0, 0, 1), up=(0, 1, 0), fov_y=1.0)),
                   "constant textures on every slot": _constant_textured_scene}


@pytest.mark.parametrize("name", list(CONSTANT_SCENES))
def test_constant_textures_render_the_same_frame_with_every_filter(name):
    """Plumbing without arithmetic drift: a constant texture has constant mips, picking among equal texels changes nothing — pt_render through the shading kernels (tail 0) and
    the tail kernel (tail 4096), the stable-plane build and fill passes: plane records, radiance and guides."""
    sc, cam = CONSTANT_SCENES[name](); w, h = 48, 32; S = scenes.default_settings()
    prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam), sub_samples=1)
    want = {}
    for filt in [None] + FILTERS:
        for tail in (0, 4096):
            g = _tracer(sc, cam, w, h, S); g.set_tail_paths(tail)
            if filt is not None: g.set_texture_filtering(True, filt)
            st = g.render(0, 2); img = g.radiance(); key = (st["extendRays"], st["shadowRays"], st["hits"])
            if filt is None and tail == 0: want["img"], want["rays"] = img, key
            assert _same(img, want["img"]) and key == want["rays"], (name, filt, tail)
            if tail == 0:
                g.build_stable_planes(3, prm); planes = g.fill_stable_planes(3, prm)
                if filt is None: want["planes"] = planes
                for k in ("header", "planes", "spec_hit_t", "depth", "motion_vectors", "stable_radiance", "throughput"): assert _same(planes[k], want["planes"][k]), (name, filt, k)
            g.close()
    if name != "texture_cases.constant_scene": assert (want["img"][..., :3] > 0).mean() > 0.5


@pytest.mark.parametrize("fp16", [0, 1])
def test_room_frame_is_deterministic_and_keyed_by_pixel_vertex_and_sample(fp16):
    import torch
    sc, cam = tc.room(); w, h = 64, 48; S = scenes.default_settings(useFp16Types=fp16)
    def frame(filt, tail=0, calls=((0, 4),), **kw):
        g = _tracer(sc, cam, w, h, S, **kw); g.set_tail_paths(tail)
        if filt is not None: g.set_texture_filtering(True, filt)
        for first, count in calls: g.render(first, count)
        return g
    off = frame(None); a = frame(sr.LINEAR); b = frame(sr.LINEAR); img = a.radiance()
    assert np.isfinite(img).all() and not _same(img, off.radiance())                   # the filter is in the frame ...
    assert _same(img, b.radiance())                                                     # ... and the frame does not depend on the run,
    c = frame(sr.LINEAR, tail=4096); assert _same(img, c.radiance())                    # on the kernel that shades a vertex (pool slots and queue positions differ),
    d = frame(sr.LINEAR, calls=((0, 2), (2, 2))); assert _same(img, d.radiance())       # on how the samples are dealt to calls,
    for g in (off, b, c, d): g.close()
    # or on which rank owns a pixel: two interleaved tile shards, packed, carried over the host and unpacked into rank 0
    ranks = [frame(sr.LINEAR, shard_rank=r, shard_count=2) for r in range(2)]
    n, nbytes = ranks[1].shard_info(); buf = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda"); ranks[1].pack_shard(buf.data_ptr(), nbytes)
    host = buf.cpu(); back = host.to("cuda"); torch.cuda.synchronize()
    ranks[0].unpack_shard(back.data_ptr(), nbytes, 1)
    assert _same(ranks[0].radiance(), img)
    # a change of the setting resets the accumulation; switching back off gives the deterministic frame again
    a.set_texture_filtering(False); a.render(0, 4); off2 = frame(None); assert _same(a.radiance(), off2.radiance())
    for g in ranks + [a, off2]: g.close()


def _glow_scene():
    """One quad with an emissive noise texture that fills the view; nothing else emits. fov 1 rad at distance 1.6 sees 1.75 of the quad's 2 units: 224 of the 256 texels
    across 96 pixels, 2.3 texels a pixel — the ray cone's level falls between mips 1 and 2."""
    b = scenes.SceneBuilder()
    glow = b.add_texture(*tc.make_pixels(256, 256, "unorm8"))
    p, i, uv, n, tg = scenes.quad([-1, -1, 0], [-1, 1, 0], [1, 1, 0], [1, -1, 0])
    b.begin_mesh(); b.add_geometry(p, i, b.add_material(scenes.make_material(base=(0.0, 0.0, 0.0), emissive=(1.0, 1.0, 1.0), emissive_tex=glow)), uv=uv, normal=n, tangent=tg); b.add_instance(b.end_mesh())
    return b.finish(), dict(pos=(0.0, 0.0, -1.6), direction=(0, 0, 1), up=(0, 1, 0), fov_y=1.0)


def test_linear_frame_converges_to_the_trilinear_frame():
    """Radiance is linear in the emissive texel and both modes trace the same paths, so err(N) = the relative L2 distance between the LINEAR and the trilinear frame after the
    same N samples falls as 1 / sqrt(N) for an unbiased estimator with independent samples: err(64) / err(1024) = 4; a constant bias pulls the ratio towards 1. Asserted: >= 3.
    Measured on the MI355X: err(64) 0.04826, err(1024) 0.01199, ratio 4.024 (docs/WIDENING.md N11)."""
    sc, cam = _glow_scene(); w = h = 96
    S = scenes.default_settings(useFp16Types=0); S["bounceCount"] = 1; S["NEEEnabled"] = 0; S["fireflyFilterThreshold"] = 0.0; S["enableRussianRoulette"] = 0
    tri = _tracer(sc, cam, w, h, S); lin = _tracer(sc, cam, w, h, S); lin.set_texture_filtering(True, sr.LINEAR)
    err = {}; done = 0
    for n in (1, 64, 1024):
        tri.render(done, n - done); lin.render(done, n - done); done = n
        a, b = tri.radiance()[..., :3].astype(np.float64), lin.radiance()[..., :3].astype(np.float64)
        if n == 1:
            lit = (a > 0).any(-1); assert lit.mean() > 0.9
            assert ((a != b).any(-1) & lit).sum() > 0.5 * lit.sum()                      # the level is fractional: most pixels pick another texel than the blend
        err[n] = float(np.linalg.norm(a - b) / np.linalg.norm(a))
    tri.close(); lin.close()
    ratio = err[64] / err[1024]
    print("err(1) %.5f err(64) %.5f err(1024) %.5f ratio err(64) / err(1024) %.3f" % (err[1], err[64], err[1024], ratio))
    assert ratio >= 3.0, (err, ratio)


def test_interface():
    import rtxpt_amd as pt
    assert pt.texture_filtering_default_params() == (0, pt.PT_STF_FILTER_LINEAR, 0, pytest.approx(np.float32(0.3)))
    g = pt.PathTracer()
    def code(*a, **kw):
        with pytest.raises(pt.PtError) as e: g.set_texture_filtering(*a, **kw)
        return e.value.code
    assert code(True, pt.PT_STF_FILTER_GAUSSIAN) == 5                                    # PT_ERROR_UNSUPPORTED
    assert code(True, pt.PT_STF_FILTER_LINEAR, magnification=1) == 5
    assert code(True, 4) == 1 and code(True, 1, magnification=4) == 1 and code(2, 1) == 1  # PT_ERROR_INVALID_ARGUMENT
    f = g.L.pt_set_texture_filtering; assert f(g.h, None) == 1 and g.L.pt_texture_filtering_default_params(None) == 1
    for filt in FILTERS: g.set_texture_filtering(True, filt)
    g.set_texture_filtering(False)
    g.close()

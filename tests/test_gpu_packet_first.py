"""Vertex 0 as 32-ray packets (run with -m gpu; rtxpt_amd/csrc/pt_traverse8k.h traverse8_packets, pt_trace.hip k_extend_first_packets, k_extend_first_listed, pt_frame.hip
RenderFrame::enable_first_vertex_packets): the first traversal launch of a compacted batch walks the camera rays of 32 consecutive paths on one shared stack per wave; a packet over
its step cap or stack bound commits nothing and leaves its rays to the per-ray kernel behind it. The closest hit is the minimum of (t, primitive) over the triangles a ray accepts,
whatever the order in which they are looked at, so every case here holds radiance bits, extendRays, shadowRays and hits to the CPU oracle AND to the same context with
MI355PT_FIRST_VERTEX_PACKETS=0 (k_extend_first, one ray per lane pair). The switches are read at pt_create, so the environment is set before a tracer is made; the tail kernel is
switched off (set_tail_paths(0)), or the small frames would never reach the launch.

The shapes are the smallest at which the kernel can go wrong: 1 x 1 (one ray, 31 idle pairs), 8 x 8, 37 x 19 (edge blocks of the owned-pixel list are shorter than 8 pixels: packets
straddle blocks), 64 x 36; 1, 3, 4 and 5 samples from a non-zero first sample (3 and 5 do not divide 32: a packet mixes pixel counts); 1, 2 and 4 pipelined batches; tile shards of 2
and 3 (owned lists with gaps); a thin lens (origins differ within a packet); an alpha-tested card across part of the view; an empty scene; a frame where every ray misses; the step cap
at 1 (every packet is left over) and at 4 (most are) — in the street scene the per-ray kernel then also cuts leftover rays into sub-trees, since every wave runs dry after one chunk;
the stack bound at 2 entries; both lp-type builds."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWITCH, STEP_CAP, STACK = "MI355PT_FIRST_VERTEX_PACKETS", "MI355PT_PACKET_STEP_CAP", "MI355PT_PACKET_STACK"
_cache = {}


def _bits(a): return np.asarray(a).view(np.uint32)


def _once(key, make):
    if key not in _cache: _cache[key] = make()
    return _cache[key]


def _oracle(sc, camd, S, w, h, first, n, rect=None):
    from oracle import ptref
    o = ptref.Oracle(lp16=bool(int(S["useFp16Types"]))); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h)
    o.render(first, n, rect=rect)
    c = o.counters(); out = (o.radiance(), (c["extendRays"], c["shadowRays"], c["hits"])); o.close()
    return out


def _tracer(monkeypatch, switch, sc, camd, S, w, h, env=None, **kw):
    import rtxpt_amd as pt
    for k in (STEP_CAP, STACK): monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(SWITCH, str(switch))
    for k, v in (env or {}).items(): monkeypatch.setenv(k, str(v))
    t = pt.PathTracer(**kw); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h); t.set_tail_paths(0)
    return t


def _frame(t, first, n):
    t.reset_accumulation(); st = t.render(first, n)
    return t.radiance(), (int(st["extendRays"]), int(st["shadowRays"]), int(st["hits"]))


def _same(a, b): return np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1]


def _check(monkeypatch, key, sc, camd, S, w, h, first, n, env=None):
    """packets on and off, each against the oracle, bit for bit and count for count"""
    want = _once(key, lambda: _oracle(sc, camd, S, w, h, first, n))
    got = {}
    for switch in (1, 0):
        t = _tracer(monkeypatch, switch, sc, camd, S, w, h, env=env); got[switch] = _frame(t, first, n); t.close()
    for switch in (1, 0):
        a, b = _bits(got[switch][0]), _bits(want[0])
        assert np.array_equal(a, b), "%s, switch %d: %d pixels differ from the oracle" % (key, switch, int((a != b).any(-1).sum()))
        assert got[switch][1] == want[1], "%s, switch %d: ray / hit counts %s, the oracle's %s" % (key, switch, got[switch][1], want[1])
    assert _same(got[1], got[0])
    return want


def _street(w, h, lp16=1, **camera):
    from rtxpt_amd import scenes
    sc, cam = _once("street", lambda: scenes.bistro_like(scale=0.05, tex_size=128))
    return sc, scenes.bridge_camera(w, h, **dict(cam, **camera)), scenes.default_settings(useFp16Types=lp16)


# ---- 1. frame sizes, 4 spp: 32 consecutive paths are 8 pixels of a row of an 8 x 8 block, or fewer pixels of several rows where the block is cut by the frame's edge
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (37, 19), (64, 36)])
def test_frame_sizes_match_oracle(w, h, monkeypatch):
    sc, camd, S = _street(w, h)
    want = _check(monkeypatch, "street_%dx%dx4" % (w, h), sc, camd, S, w, h, 0, 4)
    assert want[1][0] >= w * h * 4


# ---- 2. sample counts that do and do not divide 32, continuing at sample 2
@pytest.mark.parametrize("spp", [1, 3, 4, 5])
def test_sample_counts_from_a_later_sample_match_oracle(spp, monkeypatch):
    sc, camd, S = _street(37, 19)
    _check(monkeypatch, "street_37x19_first2x%d" % spp, sc, camd, S, 37, 19, 2, spp)


# ---- 3. pipelined batches: every batch walks the packets of its own slice of the owned pixels (one batch: every other case)
BAND = (252, 268)      # sixteen rows across the middle of the frame, where a batch's owned pixels end and the next one's begin


@pytest.mark.parametrize("spp,batches", [(2, 2), (4, 4)])
def test_pipelined_batches_match_oracle_band(spp, batches, monkeypatch):
    """1024 x 520 at 2 spp is 1 064 960 paths per call (two batches), at 4 spp 2 129 920 (four). Rows 252..267 against the oracle, bit for bit; the tracer reports no counts per
    rectangle, so the counts, and the whole frame, are held to the same build's serial-kernel frame (one batch, k_generate, no packets), as tests/test_gpu_first_vertex.py does."""
    w, h = 1024, 520
    assert "MI355PT_BATCHES" not in os.environ
    assert batches == (1 if w * h * spp < (1 << 20) else 2 if w * h * spp < (1 << 21) else 4)
    sc, camd, S = _street(w, h)
    b = _bits(_oracle(sc, camd, S, w, h, 0, spp, rect=(0, BAND[0], w, BAND[1]))[0])[BAND[0]:BAND[1]]
    frames = {}
    for switch in (1, 0):
        t = _tracer(monkeypatch, switch, sc, camd, S, w, h); frames[switch] = _frame(t, 0, spp)
        if switch == 1: t.set_serial_kernels(True); one = _frame(t, 0, spp)
        t.close()
    for switch, got in frames.items():
        a = _bits(got[0])[BAND[0]:BAND[1]]
        assert np.array_equal(a, b), "switch %d, rows %d..%d: %d pixels differ from the oracle" % (switch, BAND[0], BAND[1] - 1, int((a != b).any(-1).sum()))
        assert got[1][1] > 0 and _same(got, one), "switch %d against the serial-kernel frame" % switch


# ---- 4. tile shards: a rank's owned list is its tiles, with gaps; the ranks' pixels are the oracle's, and their counts add up to the oracle's
@pytest.mark.parametrize("world", [2, 3])
def test_tile_shards_match_oracle(world, monkeypatch):
    import rtxpt_amd as pt
    w, h = 64, 36
    sc, camd, S = _street(w, h)
    want = _once("street_64x36x4", lambda: _oracle(sc, camd, S, w, h, 0, 4))
    total = {1: np.zeros(3, np.int64), 0: np.zeros(3, np.int64)}; covered = 0
    for rank in range(world):
        own = pt.shard_layout(w, h, rank, world); ys, xs = (own & 0xFFFF).astype(np.int64), (own >> 16).astype(np.int64)
        assert own.size < w * h
        covered += own.size
        if own.size == 0: continue
        for switch in (1, 0):
            t = _tracer(monkeypatch, switch, sc, camd, S, w, h, shard_rank=rank, shard_count=world); got = _frame(t, 0, 4); t.close()
            assert np.array_equal(_bits(got[0])[ys, xs], _bits(want[0])[ys, xs]), "rank %d of %d, switch %d: the rank's tiles differ from the oracle's frame" % (rank, world, switch)
            total[switch] += np.array(got[1], np.int64)
    assert covered == w * h
    for switch in (1, 0): assert tuple(int(v) for v in total[switch]) == want[1], "switch %d: the ranks' counts %s, the oracle's %s" % (switch, total[switch], want[1])


# ---- 5. a thin lens: the rays of a packet start at different points of the aperture
def test_thin_lens_matches_oracle(monkeypatch):
    sc, camd, S = _street(37, 19, aperture_radius=0.02, jitter=(0.25, -0.375))
    assert float(camd["ApertureRadius"]) > 0
    _check(monkeypatch, "street_lens_37x19x3", sc, camd, S, 37, 19, 0, 3)


# ---- 6. an alpha-tested card across part of the view (a checkerboard of holes: neighbouring rays of a packet accept and reject the same triangle), in front of a lit room
def _card_room():
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder(); mm = scenes.make_material
    white = b.add_material(mm(base=(0.725, 0.71, 0.68), roughness=0.6)); red = b.add_material(mm(base=(0.63, 0.065, 0.05)))
    light = b.add_material(mm(base=(0.78, 0.78, 0.78), emissive=(17.0, 12.0, 4.0)))
    a = np.zeros((64, 64, 4), np.uint8); a[..., :3] = (200, 180, 90)
    yy, xx = np.mgrid[0:64, 0:64]; a[..., 3] = np.where(((xx // 8) + (yy // 8)) % 2 == 0, 255, 0)
    card = b.add_material(mm(base=(1, 1, 1), base_tex=b.add_texture(a, scenes.TEX_RGBA8_UNORM), alpha_cutoff=0.5))
    X, Y, Z = 0.5528, 0.5488, 0.5592
    b.begin_mesh()
    for pts, mat in ((((0, 0, 0), (0, 0, Z), (X, 0, Z), (X, 0, 0)), white), (((0, Y, 0), (X, Y, 0), (X, Y, Z), (0, Y, Z)), white), (((0, 0, Z), (0, Y, Z), (X, Y, Z), (X, 0, Z)), white),
                     (((0, 0, 0), (0, Y, 0), (0, Y, Z), (0, 0, Z)), red), (((X, 0, 0), (X, 0, Z), (X, Y, Z), (X, Y, 0)), red)):
        p, i, uv, n, t = scenes.quad(*pts); b.add_geometry(p, i, mat, uv=uv, normal=n, tangent=t)
    ly = Y - 0.0002
    p, i, uv, n, t = scenes.quad((0.213, ly, 0.227), (0.343, ly, 0.227), (0.343, ly, 0.332), (0.213, ly, 0.332)); b.add_geometry(p, i, light, uv=uv, normal=n, tangent=t)
    b.add_instance(b.end_mesh())
    p, i, uv, n, t = scenes.quad((0.20, 0.05, 0.10), (0.20, 0.45, 0.10), (0.52, 0.45, 0.10), (0.52, 0.05, 0.10), uv_scale=3.0)
    b.begin_mesh(); b.add_geometry(p, i, card, uv=uv, normal=n, tangent=t, geom_flags=scenes.GEOMF_ALPHA_TESTED); b.add_instance(b.end_mesh())
    b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1))
    cam = dict(pos=(0.278, 0.273, -0.8), direction=(0, 0, 1), up=(0, 1, 0), fov_y=0.6859, near_z=0.01, far_z=100.0, focal_distance=1.0)
    return b.finish(), cam


def test_alpha_tested_card_matches_oracle(monkeypatch):
    from rtxpt_amd import scenes
    sc, cam = _once("card_room", _card_room)
    _check(monkeypatch, "card_37x19x4", sc, scenes.bridge_camera(37, 19, **cam), scenes.default_settings(useFp16Types=1), 37, 19, 0, 4)


# ---- 7. nothing to hit: a scene without geometry (no root: no packet takes a step), and a room behind the camera (every packet ends at the root)
def test_empty_scene_matches_oracle(monkeypatch):
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder(); b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1)); sc = b.finish()
    cam = dict(pos=(0.278, 0.273, -0.8), direction=(0, 0, 1), up=(0, 1, 0), fov_y=0.6859, near_z=0.01, far_z=100.0, focal_distance=1.0)
    want = _check(monkeypatch, "empty_37x19x3", sc, scenes.bridge_camera(37, 19, **cam), scenes.default_settings(useFp16Types=1), 37, 19, 0, 3)
    assert want[1] == (37 * 19 * 3, 0, 0)


def test_every_ray_misses_matches_oracle(monkeypatch):
    from rtxpt_amd import scenes
    sc, cam = _once("card_room", _card_room)
    want = _check(monkeypatch, "away_37x19x3", sc, scenes.bridge_camera(37, 19, **dict(cam, direction=(0, 0, -1))), scenes.default_settings(useFp16Types=1), 37, 19, 0, 3)
    assert want[1] == (37 * 19 * 3, 0, 0)


# ---- 8. the leftover path: a step cap of 1 hands every packet over at the root, 4 hands over all but the packets that miss early; a stack of 2 entries hands over the packets whose
# nodes push more (MI355PT_PACKET_STEP_CAP, MI355PT_PACKET_STACK). 2304 leftover rays of the street scene keep the per-ray kernel's waves going past their only chunk, so its
# straggler rounds run too
@pytest.mark.parametrize("env", [{STEP_CAP: 1}, {STEP_CAP: 4}, {STACK: 2}], ids=["step_cap_1", "step_cap_4", "stack_2"])
def test_leftover_packets_match_oracle(env, monkeypatch):
    sc, camd, S = _street(64, 36)
    _check(monkeypatch, "street_64x36x4", sc, camd, S, 64, 36, 0, 4, env=env)


def test_leftover_packets_of_the_card_room_match_oracle(monkeypatch):
    from rtxpt_amd import scenes
    sc, cam = _once("card_room", _card_room)
    _check(monkeypatch, "card_37x19x4", sc, scenes.bridge_camera(37, 19, **cam), scenes.default_settings(useFp16Types=1), 37, 19, 0, 4, env={STEP_CAP: 4})


# ---- 9. both lp-type builds (useFp16Types 1: every other case)
def test_fp32_build_matches_oracle(monkeypatch):
    sc, camd, S = _street(37, 19, lp16=0)
    _check(monkeypatch, "street_fp32_37x19x4", sc, camd, S, 37, 19, 0, 4)

"""Vertex 0 as 64-ray packets, one lane per ray (run with -m gpu; rtxpt_amd/csrc/pt_traverse8k.h traverse8_packets64, pt_trace.hip k_extend_first_packets64 and
k_route_packets64, MI355PT_FIRST_VERTEX_PACKETS=2): lane L of a wave holds ray 64 p + L of packet p, tests all eight children of the shared node and both triangles of a
leaf for it, and reports its own hit; a packet over its step cap or stack bound commits nothing and leaves its up to 64 rays to the per-ray kernel. The closest hit is the
minimum of (t, primitive) over the triangles a ray accepts, whatever the order in which they are looked at, so every case holds radiance bits, extendRays, shadowRays and
hits to the CPU oracle AND to the same frame with the switch at 1 (the 32-ray pair packets) and at 0 (k_extend_first). The switches are read at pt_create, so the
environment is set before a tracer is made; the tail kernel is switched off (set_tail_paths(0)), or the small frames would never reach the launch.

Frames, chosen where a 64-ray packet can go wrong: 1 x 1 at 1 spp (one ray, 63 idle lanes), 3 x 3 at 5 spp (45 rays: one short packet), 9 x 7 at 3 spp (189 rays: two full
packets and a short one), 16 x 16 at 4 spp (exactly 16 full packets). Bounds: step cap 1 (every packet is left over), step cap 4, stack bound 2, and the default bounds,
where the packets must commit rays themselves. Scenes: no geometry (no root), one triangle, an alpha-tested card in front of an emitter, a thin lens. Both lp-type builds, a
two-way tile shard, two and four pipelined batches."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWITCH, STEP_CAP, STACK = "MI355PT_FIRST_VERTEX_PACKETS", "MI355PT_PACKET_STEP_CAP", "MI355PT_PACKET_STACK"
SWITCHES = (2, 1, 0)
CAM = dict(pos=(0.278, 0.273, -0.8), direction=(0, 0, 1), up=(0, 1, 0), fov_y=0.6859, near_z=0.01, far_z=100.0, focal_distance=1.0)
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


def _check(monkeypatch, key, sc, camd, S, w, h, first, n, env=None):
    """the switch at 2, 1 and 0, each against the oracle and against each other, bit for bit and count for count"""
    want = _once(key, lambda: _oracle(sc, camd, S, w, h, first, n))
    got = {}
    for switch in SWITCHES:
        t = _tracer(monkeypatch, switch, sc, camd, S, w, h, env=env); got[switch] = _frame(t, first, n); t.close()
    for switch in SWITCHES:
        a, b = _bits(got[switch][0]), _bits(want[0])
        assert np.array_equal(a, b), "%s, switch %d: %d pixels differ from the oracle" % (key, switch, int((a != b).any(-1).sum()))
        assert got[switch][1] == want[1], "%s, switch %d: ray / hit counts %s, the oracle's %s" % (key, switch, got[switch][1], want[1])
    for switch in (1, 0):
        assert np.array_equal(_bits(got[2][0]), _bits(got[switch][0])) and got[2][1] == got[switch][1], "%s: switch 2 against switch %d" % (key, switch)
    return want


def _street(w, h, lp16=1, **camera):
    from rtxpt_amd import scenes
    sc, cam = _once("street", lambda: scenes.bistro_like(scale=0.05, tex_size=128))
    return sc, scenes.bridge_camera(w, h, **dict(cam, **camera)), scenes.default_settings(useFp16Types=lp16)


# ---- 1. frame sizes: one ray in a packet; one short packet; two full packets and a short one; exactly 16 full packets
@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (3, 3, 5), (9, 7, 3), (16, 16, 4)])
def test_frame_sizes_match_oracle(w, h, spp, monkeypatch):
    sc, camd, S = _street(w, h)
    want = _check(monkeypatch, "street_%dx%dx%d" % (w, h, spp), sc, camd, S, w, h, 0, spp)
    assert want[1][0] >= w * h * spp


# ---- 2. the leftover path: a step cap of 1 hands every packet over at the root, 4 hands over all but the packets that miss early; a stack of 2 entries hands over the
# packets whose nodes push more
@pytest.mark.parametrize("env", [{STEP_CAP: 1}, {STEP_CAP: 4}, {STACK: 2}], ids=["step_cap_1", "step_cap_4", "stack_2"])
def test_leftover_packets_match_oracle(env, monkeypatch):
    sc, camd, S = _street(16, 16)
    _check(monkeypatch, "street_16x16x4", sc, camd, S, 16, 16, 0, 4, env=env)


def _pinhole_rays(cam, w, h, spp):
    """w x h x spp rays from the camera's position through a regular grid (consecutive rays are neighbours, as the camera rays of a packet are): rows of
    origin | tmin = 0 | direction | tmax = kMaxRayTravel"""
    f = np.asarray(cam["direction"], np.float64); f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(cam["up"], np.float64)); r /= np.linalg.norm(r); u = np.cross(r, f)
    t = np.tan(0.5 * float(cam["fov_y"]))
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    sx = ((xs + (ss + 0.5) / spp) / w * 2 - 1) * t * w / h; sy = (1 - (ys + 0.5) / h * 2) * t
    d = f[None] + sx.reshape(-1, 1) * r[None] + sy.reshape(-1, 1) * u[None]; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((d.shape[0], 8), np.float32)
    rays[:, 0:3] = np.asarray(cam["pos"], np.float32); rays[:, 4:7] = d.astype(np.float32); rays[:, 7] = np.float32(1e15)
    return rays


def test_default_bounds_leave_fewer_rays_than_traced(monkeypatch):
    """the default step cap and stack bound: the packets commit rays themselves (leftover count below the ray count), every ray is committed or left over exactly once, and the
    records are the per-ray route's. pt_trace_route's packet route follows the context's mode, so this is traverse8_packets64 on stored rays (k_route_packets64)."""
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    sc, cam = _once("street", lambda: scenes.bistro_like(scale=0.05, tex_size=128))
    rays = _pinhole_rays(cam, 16, 16, 4); n = rays.shape[0]
    for k in (STEP_CAP, STACK): monkeypatch.delenv(k, raising=False)
    out = {}
    for switch in (2, 1):
        monkeypatch.setenv(SWITCH, str(switch))
        g = pt.PathTracer(test_hooks=True); g.set_scene(sc); g.set_settings(scenes.default_settings())
        try:
            out[switch] = g.trace_route("packets", rays)
            if switch == 2: ext = g.trace_route("extend", rays)
        finally:
            g.close()
    for switch in (2, 1):
        st = out[switch][1]
        print("switch %d: packet_rays %d leftover_rays %d of %d" % (switch, st["packet_rays"], st["leftover_rays"], n))
        assert st["overflow"] == 0 and st["packet_rays"] + st["leftover_rays"] == n
        assert st["leftover_rays"] < n, "switch %d: every ray was left over at the default bounds" % switch
        assert np.array_equal(_bits(out[switch][0]), _bits(ext[0])), "switch %d: records differ from the per-ray route's" % switch
    assert out[2][1]["leftover_rays"] % 64 == 0 and out[1][1]["leftover_rays"] % 32 == 0      # (1024 rays: whole packets)
    assert (_bits(ext[0])[:, 1] != 0xFFFFFFFF).any()


# ---- 3. scenes
def test_empty_scene_matches_oracle(monkeypatch):
    """no geometry: the root is invalid, no packet takes a step, every ray reports a miss"""
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder(); b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1)); sc = b.finish()
    want = _check(monkeypatch, "empty_9x7x3", sc, scenes.bridge_camera(9, 7, **CAM), scenes.default_settings(useFp16Types=1), 9, 7, 0, 3)
    assert want[1] == (9 * 7 * 3, 0, 0)


def test_one_triangle_matches_oracle(monkeypatch):
    """a root with one leaf of one triangle across part of the view: lanes of one packet hit and miss it"""
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder(); mat = b.add_material(scenes.make_material(base=(0.6, 0.5, 0.4), roughness=0.7))
    p = np.array([(0.10, 0.10, 0.2), (0.45, 0.12, 0.2), (0.25, 0.45, 0.25)], np.float32)
    nrm = np.cross(p[1] - p[0], p[2] - p[0]); nrm /= np.linalg.norm(nrm); tan = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
    b.begin_mesh(); b.add_geometry(p, np.array([0, 1, 2], np.uint32), mat, uv=np.array([[0, 0], [1, 0], [0, 1]], np.float32), normal=np.tile(nrm, (3, 1)), tangent=np.tile(np.append(tan, 1.0), (3, 1)))
    b.add_instance(b.end_mesh())
    b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1)); sc = b.finish()
    want = _check(monkeypatch, "triangle_9x7x3", sc, scenes.bridge_camera(9, 7, **CAM), scenes.default_settings(useFp16Types=1), 9, 7, 0, 3)
    assert 0 < want[1][2] and want[1][0] >= 9 * 7 * 3      # some camera rays hit it


def _card_room():
    """an alpha-tested card (a checkerboard of holes: neighbouring rays of a packet accept and reject the same triangle) in front of a lit room"""
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
    return b.finish()


def test_alpha_tested_card_matches_oracle(monkeypatch):
    from rtxpt_amd import scenes
    sc = _once("card_room", _card_room)
    _check(monkeypatch, "card_9x7x3", sc, scenes.bridge_camera(9, 7, **CAM), scenes.default_settings(useFp16Types=1), 9, 7, 0, 3)


def test_thin_lens_matches_oracle(monkeypatch):
    """the rays of a packet start at different points of the aperture"""
    sc, camd, S = _street(9, 7, aperture_radius=0.02, jitter=(0.25, -0.375))
    assert float(camd["ApertureRadius"]) > 0
    _check(monkeypatch, "street_lens_9x7x3", sc, camd, S, 9, 7, 0, 3)


# ---- 4. both lp-type builds (useFp16Types 1: every other case)
def test_fp32_build_matches_oracle(monkeypatch):
    sc, camd, S = _street(9, 7, lp16=0)
    _check(monkeypatch, "street_fp32_9x7x3", sc, camd, S, 9, 7, 0, 3)


# ---- 5. a two-way tile shard: a rank's owned list is its tiles, with gaps; the ranks' pixels are the oracle's, and their counts add up to the oracle's
def test_two_way_tile_shard_matches_oracle(monkeypatch):
    import rtxpt_amd as pt
    w, h, world = 64, 36, 2      # (a 16 x 16 frame is one rank's alone)
    sc, camd, S = _street(w, h)
    want = _once("street_64x36x4", lambda: _oracle(sc, camd, S, w, h, 0, 4))
    total = {s: np.zeros(3, np.int64) for s in SWITCHES}; covered = 0
    for rank in range(world):
        own = pt.shard_layout(w, h, rank, world); ys, xs = (own & 0xFFFF).astype(np.int64), (own >> 16).astype(np.int64)
        assert 0 < own.size < w * h
        covered += own.size
        for switch in SWITCHES:
            t = _tracer(monkeypatch, switch, sc, camd, S, w, h, shard_rank=rank, shard_count=world); got = _frame(t, 0, 4); t.close()
            assert np.array_equal(_bits(got[0])[ys, xs], _bits(want[0])[ys, xs]), "rank %d of %d, switch %d: the rank's tiles differ from the oracle's frame" % (rank, world, switch)
            total[switch] += np.array(got[1], np.int64)
    assert covered == w * h
    for switch in SWITCHES: assert tuple(int(v) for v in total[switch]) == want[1], "switch %d: the ranks' counts %s, the oracle's %s" % (switch, total[switch], want[1])


# ---- 6. pipelined batches: every batch walks the packets of its own slice of the owned pixels (one batch: every other case)
BAND = (256, 264)      # eight rows across the middle of the frame, where a batch's owned pixels end and the next one's begin


@pytest.mark.parametrize("spp,batches", [(2, 2), (4, 4)])
def test_pipelined_batches_match_oracle_band(spp, batches, monkeypatch):
    """1024 x 520 at 2 spp is 1 064 960 paths per call (two batches), at 4 spp 2 129 920 (four). Rows 256..263 against the oracle, bit for bit; the tracer reports no counts per
    rectangle, so the counts, and the whole frame, are held to the frames with the switch at 1 and at 0."""
    w, h = 1024, 520
    assert "MI355PT_BATCHES" not in os.environ
    assert batches == (1 if w * h * spp < (1 << 20) else 2 if w * h * spp < (1 << 21) else 4)
    sc, camd, S = _street(w, h)
    b = _bits(_oracle(sc, camd, S, w, h, 0, spp, rect=(0, BAND[0], w, BAND[1]))[0])[BAND[0]:BAND[1]]
    frames = {}
    for switch in SWITCHES:
        t = _tracer(monkeypatch, switch, sc, camd, S, w, h); frames[switch] = _frame(t, 0, spp); t.close()
    for switch, got in frames.items():
        a = _bits(got[0])[BAND[0]:BAND[1]]
        assert np.array_equal(a, b), "switch %d, rows %d..%d: %d pixels differ from the oracle" % (switch, BAND[0], BAND[1] - 1, int((a != b).any(-1).sum()))
        assert got[1][1] > 0 and np.array_equal(_bits(got[0]), _bits(frames[0][0])) and got[1] == frames[0][1], "switch %d against switch 0" % switch

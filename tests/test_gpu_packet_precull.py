"""The 64-ray packets' interval test of a node's children (run with -m gpu; rtxpt_amd/csrc/pt_packet_precull.h, pt_traverse8k.h traverse8_packets64<true>,
MI355PT_PACKET_PRECULL): before the eight per-ray slab tests of a node step, each child's box is tested once against the packet's interval of origins and reciprocal
directions, and the per-ray tests run only for the children that test keeps. It may drop a child only if no ray's own test enters it, so nothing a frame computes can
change: every case holds radiance bits, extendRays, shadowRays and hits to the CPU oracle AND to the same frame with the switch at 0 AND to the frame with
MI355PT_FIRST_VERTEX_PACKETS=0 (one ray per lane pair, no packets), and the hit records of stored rays through pt_trace_route's packet route to the switch at 0 and to the
per-ray route. The switches are read at pt_create, so the environment is set before a tracer is made.

Cases, chosen where the interval test can go wrong: packets that are partly valid (1 x 1, 8 x 8, 24 x 16 frames at 1, 3 and 4 spp); a thin lens as wide as the room (a wide
origin interval); a camera inside a box with a 170 degree field of view (reciprocals of both signs on an axis: no test for that packet); rays exactly along an axis (two
reciprocals at ray_safe_rcp's clamp); flat geometry (a node of zero extent on an axis); an alpha-tested card in front of an emitter; no geometry; one triangle; step cap 1
and 4 and a stack of 2 (leftover rays); two shards; four batches; both lp builds. The scenes are tests/pin_scenes.py's (a few thousand triangles at the most)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PACKETS, PRECULL, STEP_CAP, STACK = "MI355PT_FIRST_VERTEX_PACKETS", "MI355PT_PACKET_PRECULL", "MI355PT_PACKET_STEP_CAP", "MI355PT_PACKET_STACK"
# (packets, precull): the interval test on; off; no packets at all
MODES = {"precull": (2, 1), "plain": (2, 0), "per_ray": (0, 1)}
_cache = {}


def _bits(a): return np.asarray(a).view(np.uint32)


def _once(key, make):
    if key not in _cache: _cache[key] = make()
    return _cache[key]


def _pin(name):
    import pin_scenes
    return _once("pin_" + name, lambda: pin_scenes.cases()[name][0]())


def _oracle(sc, camd, S, w, h, first, n, rect=None):
    from oracle import ptref
    o = ptref.Oracle(lp16=bool(int(S["useFp16Types"]))); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h)
    o.render(first, n, rect=rect)
    c = o.counters(); out = (o.radiance(), (c["extendRays"], c["shadowRays"], c["hits"])); o.close()
    return out


def _setenv(monkeypatch, mode, env=None):
    for k in (STEP_CAP, STACK): monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(PACKETS, str(MODES[mode][0])); monkeypatch.setenv(PRECULL, str(MODES[mode][1]))
    for k, v in (env or {}).items(): monkeypatch.setenv(k, str(v))


def _frame(monkeypatch, mode, sc, camd, S, w, h, first, n, env=None, **kw):
    import rtxpt_amd as pt
    _setenv(monkeypatch, mode, env)
    t = pt.PathTracer(**kw); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h); t.set_tail_paths(0)
    try:
        t.reset_accumulation(); st = t.render(first, n)
        return t.radiance(), (int(st["extendRays"]), int(st["shadowRays"]), int(st["hits"]))
    finally:
        t.close()


def _check(monkeypatch, key, sc, camd, S, w, h, first, n, env=None):
    """the three modes, each against the oracle and against each other, bit for bit and count for count"""
    want = _once("oracle_" + key, lambda: _oracle(sc, camd, S, w, h, first, n))
    got = {m: _frame(monkeypatch, m, sc, camd, S, w, h, first, n, env=env) for m in MODES}
    for m in MODES:
        a, b = _bits(got[m][0]), _bits(want[0])
        assert np.array_equal(a, b), "%s, %s: %d pixels differ from the oracle" % (key, m, int((a != b).any(-1).sum()))
        assert got[m][1] == want[1], "%s, %s: ray / hit counts %s, the oracle's %s" % (key, m, got[m][1], want[1])
    for m in ("plain", "per_ray"):
        assert np.array_equal(_bits(got["precull"][0]), _bits(got[m][0])) and got["precull"][1] == got[m][1], "%s: precull against %s" % (key, m)
    return want


def _routes(monkeypatch, sc, rays, **opt):
    """hit records of stored rays: the packet route with the interval test, without it, and the per-ray route; returns the three and the packet routes' stats"""
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    out = {}
    for m in ("precull", "plain"):
        _setenv(monkeypatch, m)
        g = pt.PathTracer(test_hooks=True); g.set_scene(sc); g.set_settings(scenes.default_settings())
        try:
            out[m] = g.trace_route("packets", rays, **opt)
            if m == "plain": out["per_ray"] = g.trace_route("extend", rays)
        finally:
            g.close()
    n = rays.shape[0]
    for m in ("precull", "plain"):
        st = out[m][1]
        assert st["overflow"] == 0 and st["packet_rays"] + st["leftover_rays"] == n, "%s: %s" % (m, st)
        assert np.array_equal(_bits(out[m][0]), _bits(out["per_ray"][0])), "%s: %d hit records differ from the per-ray route's" % (m, int((_bits(out[m][0]) != _bits(out["per_ray"][0])).any(-1).sum()))
    for k in ("packet_rays", "leftover_rays"):
        assert out["precull"][1][k] == out["plain"][1][k], "the interval test changed what the packets commit: %s against %s" % (out["precull"][1], out["plain"][1])
    return out


def _street(w, h, lp16=1, **camera):
    from rtxpt_amd import scenes
    sc, cam = _pin("bistro_like")
    return sc, scenes.bridge_camera(w, h, **dict(cam, **camera)), scenes.default_settings(useFp16Types=lp16)


def _room(w, h, **camera):
    from rtxpt_amd import scenes
    sc, cam = _pin("c2")
    return sc, scenes.bridge_camera(w, h, **dict(cam, **camera)), scenes.config_settings("C2"), cam


# ---- 1. frame sizes: one ray; one short packet; whole and short packets, at sample counts that put one, three and four rays of a pixel in a packet
@pytest.mark.parametrize("spp", [1, 3, 4])
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (24, 16)])
def test_frame_sizes_match_oracle(w, h, spp, monkeypatch):
    sc, camd, S = _street(w, h)
    want = _check(monkeypatch, "street_%dx%dx%d" % (w, h, spp), sc, camd, S, w, h, 0, spp)
    assert want[1][0] >= w * h * spp


# ---- 2. the packet's intervals
def test_wide_lens_matches_oracle(monkeypatch):
    """an aperture of the room's size: the origins of a packet's rays fill a box as large as the nodes they are tested against"""
    sc, camd, S, cam = _room(24, 16, aperture_radius=0.25, focal_distance=1.2, jitter=(0.25, -0.375))
    assert float(camd["ApertureRadius"]) == np.float32(0.25)
    _check(monkeypatch, "room_lens_24x16x3", sc, camd, S, 24, 16, 0, 3)


def test_camera_inside_box_170_degrees_matches_oracle(monkeypatch):
    """inside the room, 170 degrees: the packets around the view's centre hold directions of both signs on x and y and have no interval test; the others have"""
    sc, camd, S, cam = _room(24, 16, pos=(0.278, 0.273, 0.15), direction=(0, 0, 1), fov_y=float(np.radians(170.0)))
    want = _check(monkeypatch, "room_inside_24x16x4", sc, camd, S, 24, 16, 0, 4)
    assert want[1][2] > 0


def test_view_along_an_axis_matches_oracle(monkeypatch):
    """the camera looks exactly along +z from the room's middle: the centre rays' x and y components are zero or next to it"""
    sc, camd, S, cam = _room(9, 9, pos=(0.278, 0.273, -0.8), direction=(0, 0, 1), up=(0, 1, 0))
    _check(monkeypatch, "room_axis_9x9x4", sc, camd, S, 9, 9, 0, 4)


@pytest.mark.parametrize("axis,sign", [(2, 1.0), (2, -1.0), (0, 1.0), (1, -1.0)])
def test_parallel_rays_along_an_axis_match_per_ray_route(axis, sign, monkeypatch):
    """stored rays with a direction of exactly +-1 on one axis and 0 on the others, from a grid of origins across the room: two reciprocals of every ray sit at
    ray_safe_rcp's clamp, all of one sign (a zero counts as positive), so the interval test runs — with reciprocals of 1.3e30"""
    sc, cam = _pin("c2")
    n = 16 * 16
    u, v = np.meshgrid((np.arange(16) + 0.5) / 16 * 0.55, (np.arange(16) + 0.5) / 16 * 0.55, indexing="ij")
    rays = np.zeros((n, 8), np.float32)
    others = [a for a in range(3) if a != axis]
    rays[:, others[0]] = u.reshape(-1); rays[:, others[1]] = v.reshape(-1); rays[:, axis] = -1.0 * sign
    rays[:, 4 + axis] = sign; rays[:, 7] = np.float32(1e15)
    out = _routes(monkeypatch, sc, rays)
    assert (_bits(out["per_ray"][0])[:, 1] != 0xFFFFFFFF).any()
    assert out["precull"][1]["packet_rays"] > 0


# ---- 3. scenes
def _flat_scene():
    """one quad in the plane z = 0.3 and one in the plane x = 0.1: the root's children, and the root on neither axis, have zero extent on an axis"""
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder(); mat = b.add_material(scenes.make_material(base=(0.6, 0.5, 0.4), roughness=0.7))
    b.begin_mesh()
    for pts in (((0.10, 0.10, 0.3), (0.45, 0.10, 0.3), (0.45, 0.45, 0.3), (0.10, 0.45, 0.3)), ((0.1, 0.05, 0.0), (0.1, 0.5, 0.0), (0.1, 0.5, 0.25), (0.1, 0.05, 0.25))):
        p, i, uv, n, t = scenes.quad(*pts); b.add_geometry(p, i, mat, uv=uv, normal=n, tangent=t)
    b.add_instance(b.end_mesh())
    b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1))
    return b.finish()


def _one_flat_quad():
    """one quad in the plane z = 0.3 alone: every node has zero extent on z"""
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder(); mat = b.add_material(scenes.make_material(base=(0.6, 0.5, 0.4), roughness=0.7))
    p, i, uv, n, t = scenes.quad((0.10, 0.10, 0.3), (0.45, 0.10, 0.3), (0.45, 0.45, 0.3), (0.10, 0.45, 0.3))
    b.begin_mesh(); b.add_geometry(p, i, mat, uv=uv, normal=n, tangent=t); b.add_instance(b.end_mesh())
    b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1))
    return b.finish()


@pytest.mark.parametrize("name,make", [("flat_pair", _flat_scene), ("flat_quad", _one_flat_quad)])
def test_flat_geometry_matches_oracle(name, make, monkeypatch):
    from rtxpt_amd import scenes
    from test_gpu_packet64 import CAM
    sc = _once(name, make)
    want = _check(monkeypatch, name + "_9x7x3", sc, scenes.bridge_camera(9, 7, **CAM), scenes.default_settings(useFp16Types=1), 9, 7, 0, 3)
    assert want[1][2] > 0      # some camera rays hit a quad
    # ... and along the flat axis, from origins IN the other quad's plane (x = 0.1: an origin on a plane of the box)
    rays = np.zeros((64, 8), np.float32); k = np.arange(64)
    rays[:, 0] = 0.1 + 0.005 * (k % 8) * (k >= 8); rays[:, 1] = 0.12 + 0.04 * (k // 8); rays[:, 2] = -0.5; rays[:, 6] = 1.0; rays[:, 7] = np.float32(1e15)
    _routes(monkeypatch, sc, rays)


def test_alpha_tested_card_matches_oracle(monkeypatch):
    from rtxpt_amd import scenes
    from test_gpu_packet64 import CAM, _card_room
    sc = _once("card_room", _card_room)
    _check(monkeypatch, "card_9x7x3", sc, scenes.bridge_camera(9, 7, **CAM), scenes.default_settings(useFp16Types=1), 9, 7, 0, 3)


def test_empty_scene_matches_oracle(monkeypatch):
    """no geometry: the root is invalid, no packet takes a step"""
    from rtxpt_amd import scenes
    from test_gpu_packet64 import CAM
    b = scenes.SceneBuilder(); b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1)); sc = b.finish()
    want = _check(monkeypatch, "empty_9x7x3", sc, scenes.bridge_camera(9, 7, **CAM), scenes.default_settings(useFp16Types=1), 9, 7, 0, 3)
    assert want[1] == (9 * 7 * 3, 0, 0)


def test_one_triangle_matches_oracle(monkeypatch):
    """a root with one leaf of one triangle (seven empty slots: inverted boxes, which the interval test must drop or leave to the rays) across part of the view"""
    from rtxpt_amd import scenes
    from test_gpu_packet64 import CAM
    b = scenes.SceneBuilder(); mat = b.add_material(scenes.make_material(base=(0.6, 0.5, 0.4), roughness=0.7))
    p = np.array([(0.10, 0.10, 0.2), (0.45, 0.12, 0.2), (0.25, 0.45, 0.25)], np.float32)
    nrm = np.cross(p[1] - p[0], p[2] - p[0]); nrm /= np.linalg.norm(nrm); tan = (p[1] - p[0]) / np.linalg.norm(p[1] - p[0])
    b.begin_mesh(); b.add_geometry(p, np.array([0, 1, 2], np.uint32), mat, uv=np.array([[0, 0], [1, 0], [0, 1]], np.float32), normal=np.tile(nrm, (3, 1)), tangent=np.tile(np.append(tan, 1.0), (3, 1)))
    b.add_instance(b.end_mesh())
    b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1)); sc = b.finish()
    want = _check(monkeypatch, "triangle_9x7x3", sc, scenes.bridge_camera(9, 7, **CAM), scenes.default_settings(useFp16Types=1), 9, 7, 0, 3)
    assert 0 < want[1][2] and want[1][0] >= 9 * 7 * 3


# ---- 4. the leftover path: a step cap of 1 hands every packet over at the root, 4 all but the packets that miss early; a stack of 2 the packets whose nodes push more
@pytest.mark.parametrize("env", [{STEP_CAP: 1}, {STEP_CAP: 4}, {STACK: 2}], ids=["step_cap_1", "step_cap_4", "stack_2"])
def test_leftover_packets_match_oracle(env, monkeypatch):
    sc, camd, S = _street(24, 16)
    _check(monkeypatch, "street_24x16x4", sc, camd, S, 24, 16, 0, 4, env=env)


def test_stored_camera_rays_leave_the_same_packets_over(monkeypatch):
    """the default bounds and a step cap of 4 on stored pinhole rays: the packets commit and leave over the same rays with and without the interval test (it changes no step
    count), and the records are the per-ray route's"""
    from test_gpu_packet64 import _pinhole_rays
    sc, cam = _pin("bistro_like")
    rays = _pinhole_rays(cam, 24, 16, 4)
    out = _routes(monkeypatch, sc, rays)
    assert out["precull"][1]["leftover_rays"] < rays.shape[0]
    assert (_bits(out["per_ray"][0])[:, 1] != 0xFFFFFFFF).any()
    _routes(monkeypatch, sc, rays, step_cap=4)
    _routes(monkeypatch, sc, rays, stack_bound=2)


# ---- 5. both lp-type builds (useFp16Types 1: every other case on the street)
def test_fp32_build_matches_oracle(monkeypatch):
    sc, camd, S = _street(24, 16, lp16=0)
    _check(monkeypatch, "street_fp32_24x16x3", sc, camd, S, 24, 16, 0, 3)


# ---- 6. a two-way tile shard: a rank's owned list is its tiles, with gaps; the ranks' pixels are the oracle's, and their counts add up to the oracle's
def test_two_way_tile_shard_matches_oracle(monkeypatch):
    import rtxpt_amd as pt
    w, h, world = 64, 36, 2
    sc, camd, S = _street(w, h)
    want = _once("oracle_street_64x36x4", lambda: _oracle(sc, camd, S, w, h, 0, 4))
    total = {m: np.zeros(3, np.int64) for m in MODES}; covered = 0
    for rank in range(world):
        own = pt.shard_layout(w, h, rank, world); ys, xs = (own & 0xFFFF).astype(np.int64), (own >> 16).astype(np.int64)
        assert 0 < own.size < w * h
        covered += own.size
        for m in MODES:
            got = _frame(monkeypatch, m, sc, camd, S, w, h, 0, 4, shard_rank=rank, shard_count=world)
            assert np.array_equal(_bits(got[0])[ys, xs], _bits(want[0])[ys, xs]), "rank %d of %d, %s: the rank's tiles differ from the oracle's frame" % (rank, world, m)
            total[m] += np.array(got[1], np.int64)
    assert covered == w * h
    for m in MODES: assert tuple(int(v) for v in total[m]) == want[1], "%s: the ranks' counts %s, the oracle's %s" % (m, total[m], want[1])


# ---- 7. four pipelined batches: every batch walks the packets of its own slice of the owned pixels
BAND = (256, 264)      # eight rows across the middle of the frame, where a batch's owned pixels end and the next one's begin


def test_four_batches_match_oracle_band(monkeypatch):
    """1024 x 520 at 4 spp is 2 129 920 paths per call: four batches. Rows 256..263 against the oracle, bit for bit; the whole frame and the counts against the other modes."""
    w, h, spp = 1024, 520, 4
    assert "MI355PT_BATCHES" not in os.environ
    sc, camd, S = _street(w, h)
    b = _bits(_oracle(sc, camd, S, w, h, 0, spp, rect=(0, BAND[0], w, BAND[1]))[0])[BAND[0]:BAND[1]]
    frames = {m: _frame(monkeypatch, m, sc, camd, S, w, h, 0, spp) for m in MODES}
    for m, got in frames.items():
        a = _bits(got[0])[BAND[0]:BAND[1]]
        assert np.array_equal(a, b), "%s, rows %d..%d: %d pixels differ from the oracle" % (m, BAND[0], BAND[1] - 1, int((a != b).any(-1).sum()))
        assert got[1][1] > 0 and np.array_equal(_bits(got[0]), _bits(frames["per_ray"][0])) and got[1] == frames["per_ray"][1], "%s against per_ray" % m

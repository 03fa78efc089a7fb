"""The per-ray traversal loop after its issue diet (run with -m gpu; rtxpt_amd/csrc/pt_scene.h alpha_test_slot / unorm8_to_float, pt_traverse8p.h: the pushes), through the
launches a frame runs (pt_trace_route) and held to the oracle bit for bit. Four blocks, each on contexts of at most a few hundred triangles and 4096 rays:

  alpha zoo      cards with an 8-bit power-of-two alpha texture, an 8-bit 5 x 3 one, a 1 x 1 one, a float-source one (alpha plane format 1), a card flagged alpha-tested
                 whose material has no texture (record.tex == ~0: the record is fetched, nothing else) and a card excluded from NEE (visibility rays ignore it); texture
                 coordinates reach outside [0, 1) on both sides, so every wrap branch runs. Two layers of cards and a wall behind them: a ray that a card lets through
                 meets another card. Routes extend, shadow, packets: every record (primitive, t, u, v / visible flag) is the oracle's.
  the cutoff     a 16 x 16 8-bit alpha texture holds every byte once (texel (i, j) = 16 j + i); sixteen unit cards, one per material, cutoffs k / 255; 256 rays per card,
                 one through every texel centre, parallel to z. Everything in the barycentrics and the texture coordinate is dyadic and short (unit right triangles at
                 even x, origins at multiples of 1 / 32), so u, v, the interpolated coordinate and the bilinear weights (0) are exact and the opacity IS the texel's
                 quotient byte / 255: a ray is stopped iff byte >= k — the integer rule, no float in it. A quotient one ulp off flips the byte == k rows.
  deep stacks    blades: large triangles in planes through the z axis, all overlapping around it; rays along the axis enter every box of the tree. A host walk of the
                 read-back BVH8 (tests/bvh_ref.py's decode, T8_HIT's rule, every hit child but the nearest pushed) gives, for the rays parallel to the axis (which miss
                 every blade: nothing is pruned, the walk is the device's), the deepest stack in traversal order — front to back for closest-hit rays, by child slot for
                 occlusion rays; for every ray whatever, the order-free bound "all children but one of every node of a root-to-leaf path". Asserted: some ray needs more
                 than BVH8_STACK entries on either route (the guarded pushes with the global tail run) and none can need more than BVH8_STACK + T8_SPILL_DEPTH; a ray's
                 stack is shallow and deep in turn, so a wave takes either text from one iteration to the next. Hits against tests/hit_ref.py within its bounds (at most 2 % skipped) and against
                 the oracle bit for bit, overflow word 0, default grid and a grid of one block.
  a small frame  64 x 64 at 2 spp of the zoo scene, one batch and two (MI355PT_BATCHES is read once per process: the two-batch frames come from a child process), fused
                 and separate traversal launches: radiance bits and ray counts are the oracle's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu
BVH8_STACK, T8_SPILL_DEPTH = 13, 96          # pt_scene.h PT_BVH8_STACK, pt_trace_plan.h T8_SPILL_DEPTH
K_MAX_RAY_TRAVEL = np.float32(1e15)
MISS = 0xFFFFFFFF
MAX_SKIPPED = 0.02
CUTOFF_BYTES = [0, 1, 2, 63, 64, 127, 128, 129, 191, 192, 253, 254, 255, 3, 100, 200]
_cache = {}


def _once(key, make):
    if key not in _cache: _cache[key] = make()
    return _cache[key]


def _bits(a): return np.ascontiguousarray(a).view(np.uint32)


def _card(b, scenes, x, y, z, mat, uv_scale=(1.0, 1.0), uv_off=(0.0, 0.0), flags=None):
    p, i, uv, n, t = scenes.quad([x, y, z], [x + 1, y, z], [x + 1, y + 1, z], [x, y + 1, z])
    uv = (uv * np.float32(uv_scale) + np.float32(uv_off)).astype(np.float32)
    b.begin_mesh(); b.add_geometry(p, i, mat, uv=uv, normal=n, tangent=t, geom_flags=scenes.GEOMF_ALPHA_TESTED if flags is None else flags); b.add_instance(b.end_mesh())


# ---- the alpha zoo
def _zoo_scene():
    from rtxpt_amd import scenes
    r = np.random.default_rng(0xA1FA)
    b = scenes.SceneBuilder(); mm = scenes.make_material
    def tex8(w, h, fmt):
        a = r.integers(0, 256, (h, w, 4)).astype(np.uint8); return b.add_texture(a, fmt)
    f = np.exp(r.standard_normal((6, 7, 4))).astype(np.float32); f[..., 3] = r.random((6, 7), np.float32) * np.float32(1.2) - np.float32(0.1)
    one = np.zeros((1, 1, 4), np.uint8); one[..., :3] = 180; one[..., 3] = 127          # 127 / 255 against the cutoff trunc(0.5 * 255) / 255: equal, the card stops the ray
    mats = [b.add_material(mm(base=(1, 1, 1), base_tex=tex8(64, 32, scenes.TEX_RGBA8_UNORM), alpha_cutoff=0.5)),
            b.add_material(mm(base=(1, 1, 1), base_tex=tex8(5, 3, scenes.TEX_RGBA8_SRGB), alpha_cutoff=0.4)),
            b.add_material(mm(base=(1, 1, 1), base_tex=b.add_texture(one, scenes.TEX_RGBA8_UNORM), alpha_cutoff=0.5)),
            b.add_material(mm(base=(1, 1, 1), base_tex=b.add_texture(f, scenes.TEX_RGBA32F), alpha_cutoff=0.6)),
            b.add_material(mm(base=(0.7, 0.6, 0.5))),                                       # flagged alpha-tested below, no texture: AlphaRec.tex == ~0
            b.add_material(mm(base=(1, 1, 1), base_tex=tex8(16, 16, scenes.TEX_RGBA8_UNORM), alpha_cutoff=0.5))]
    wall = b.add_material(mm(base=(0.6, 0.6, 0.6), roughness=0.8))
    uvs = [((3.0, -2.0), (-1.25, 0.5)), ((-2.5, 1.5), (0.75, -1.0)), ((1.0, 1.0), (-3.0, 2.0)), ((-1.0, -1.0), (0.3, 0.3)), ((1.0, 1.0), (0.0, 0.0)), ((2.0, 2.0), (-0.5, -1.5))]
    AT, NEE = scenes.GEOMF_ALPHA_TESTED, scenes.GEOMF_EXCLUDE_FROM_NEE
    for layer in range(2):
        for k in range(6):
            m = (k + 2 * layer) % 6          # the second layer holds the cards in another order
            col, row = k % 3, k // 3
            _card(b, scenes, 1.5 * col, 1.5 * row, 1.0 * layer, mats[m], uvs[m][0], uvs[m][1], flags=(AT | NEE) if m == 5 else AT)
    p, i, uv, n, t = scenes.quad([-1, -1, 2.5], [5, -1, 2.5], [5, 3.5, 2.5], [-1, 3.5, 2.5])
    b.begin_mesh(); b.add_geometry(p, i, wall, uv=uv, normal=n, tangent=t); b.add_instance(b.end_mesh())
    b.set_environment(scenes.sky_equirect(64, 32), color_multiplier=(1, 1, 1))
    return b.finish()


ZOO_CAM = dict(pos=(2.0, 1.25, -7.0), direction=(0, 0, 1), up=(0, 1, 0), fov_y=0.6859, near_z=0.01, far_z=100.0, focal_distance=1.0)


def _zoo_rays(n=4096):
    r = np.random.default_rng(0x5EED)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0] = r.uniform(-1.5, 5.5, n); rays[:, 1] = r.uniform(-0.2, 2.7, n); rays[:, 2] = -1.0
    d = np.stack([r.uniform(-0.15, 0.15, n), r.uniform(-0.15, 0.15, n), np.ones(n)], 1); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 4:7] = d; rays[:, 7] = K_MAX_RAY_TRAVEL
    sh = rays.copy(); sh[::2, 7] = 2.6          # every other visibility ray ends between the cards and the wall
    return rays, sh


def _routes(sc, rays, shadow_rays, variants=False):
    """(device records per label, oracle closest, oracle visibility) of one scene on one context"""
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    from oracle import ptref
    o = ptref.Oracle(); o.set_scene(sc); o.set_settings(scenes.default_settings())
    try:
        closest = o.trace_closest(rays); visible = o.trace_visibility(shadow_rays)
    finally:
        o.close()
    g = pt.PathTracer(test_hooks=True); g.set_scene(sc); g.set_settings(scenes.default_settings())
    runs = {}
    try:
        for route, inp in (("extend", rays), ("shadow", shadow_rays), ("packets", rays)):
            runs[route] = (route,) + g.trace_route(route, inp)
            if variants and route != "packets": runs[route + " one block"] = (route,) + g.trace_route(route, inp, max_blocks=1)
        rb = g.get_bvh8() if variants else None
    finally:
        g.close()
    return runs, closest, visible, rb


def _hold_to_oracle(what, runs, closest, visible):
    for label, (route, out, st) in runs.items():
        assert st["overflow"] == 0, (what, label, st)
        if route == "shadow":
            assert np.array_equal(out, visible), "%s (%s): %d of %d rays differ from the oracle's visibility" % (what, label, int((out != visible).sum()), out.size)
        else:
            same = (_bits(out) == _bits(closest)).all(1)
            assert same.all(), "%s (%s): %d of %d closest-hit records differ from the oracle's (first: ray %d)" % (what, label, int((~same).sum()), same.size, int(np.argmin(same)))


def test_alpha_zoo_every_record_is_the_oracles():
    sc = _once("zoo", _zoo_scene); rays, sh = _zoo_rays()
    runs, closest, visible, _ = _routes(sc, rays, sh)
    _hold_to_oracle("alpha zoo", runs, closest, visible)
    prim = _bits(closest)[:, 1]
    # the zoo does what it is for: rays end on both layers, on the wall and nowhere, and visibility rays come out both ways
    assert ((prim >= 12) & (prim < 24)).any() and ((prim == 24) | (prim == 25)).any() and (prim == MISS).any()
    assert set(np.unique(prim[prim < 12] // 2)) == set(range(6)), np.unique(prim)          # every card of the first layer stops some ray
    assert visible.min() == 0 and visible.max() == 1
    print("alpha zoo: first layer %d, second layer %d, wall %d, miss %d of %d rays; visible %d of %d" % (int((prim < 12).sum()), int(((prim >= 12) & (prim < 24)).sum()),
          int(((prim == 24) | (prim == 25)).sum()), int((prim == MISS).sum()), prim.size, int(visible.sum()), visible.size))


# ---- equality at the cutoff
def _cutoff_scene():
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder()
    a = np.zeros((16, 16, 4), np.uint8); a[..., :3] = 128
    a[..., 3] = (16 * np.arange(16)[:, None] + np.arange(16)[None, :]).astype(np.uint8)          # texel (x = i, y = j) holds 16 j + i
    tex = b.add_texture(a, scenes.TEX_RGBA8_UNORM)
    for m, k in enumerate(CUTOFF_BYTES):
        # SubInstanceData keeps trunc(saturate(c) * 255) as a byte; the record's cutoff is (float)k / 255.0f
        mat = b.add_material(scenes.make_material(base=(1, 1, 1), base_tex=tex, alpha_cutoff=(k + 0.5) / 255.0))
        _card(b, scenes, 2.0 * m, 0.0, 0.0, mat)
    return b.finish()


def test_a_ray_is_stopped_iff_its_texel_byte_reaches_the_cutoff_byte():
    sc = _once("cutoff", _cutoff_scene)
    j, i = np.mgrid[0:16, 0:16]; i, j = i.ravel(), j.ravel()
    rays = np.zeros((16 * 256, 8), np.float32); byte = np.zeros(16 * 256, np.int64); k = np.zeros(16 * 256, np.int64)
    for m, kb in enumerate(CUTOFF_BYTES):
        s = slice(256 * m, 256 * (m + 1))
        rays[s, 0] = 2.0 * m + (i + 0.5) / 16.0; rays[s, 1] = (j + 0.5) / 16.0; rays[s, 2] = -1.0; rays[s, 6] = 1.0; rays[s, 7] = K_MAX_RAY_TRAVEL
        byte[s] = 16 * j + i; k[s] = kb
    assert (rays[:, 0].astype(np.float64) * 32 == np.round(rays[:, 0].astype(np.float64) * 32)).all()          # the origins are multiples of 1 / 32: exact in float32
    stopped = byte >= k          # the integer rule
    runs, closest, visible, _ = _routes(sc, rays, rays)
    _hold_to_oracle("cutoff", runs, closest, visible)
    for label, (route, out, st) in runs.items():
        got = (out == 0) if route == "shadow" else (_bits(out)[:, 1] != MISS)
        bad = got != stopped
        assert not bad.any(), "cutoff (%s): %d rays differ from byte >= k; first: byte %d, k %d, stopped %s" % (label, int(bad.sum()), byte[np.argmax(bad)], k[np.argmax(bad)], got[np.argmax(bad)])
        if route != "shadow":
            h = stopped; card = np.repeat(np.arange(16), 256)
            assert (_bits(out)[h, 1] // 2 == card[h]).all() and (out[h, 0] == 1.0).all()          # ... on the ray's own card, at t = 1 exactly
    assert stopped[k == byte].all() and int((k == byte).sum()) == 16          # every byte == k row is in the set, and is a stop


# ---- deep stacks
def _blades(n=560, R=4.0, L=3.0):
    r = np.random.default_rng(0xB1AD)
    th = np.deg2rad(np.linspace(25.0, 65.0, n)); r.shuffle(th)
    z0 = r.uniform(0.0, 40.0, n)
    c, s = np.cos(th), np.sin(th)
    p = np.stack([np.stack([-R * c, -R * s, z0], 1), np.stack([R * c, R * s, z0], 1), np.stack([0.25 * R * c, 0.25 * R * s, z0 + L], 1)], 1)          # [n, 3, 3]
    return p.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.uint32)


def _blade_scene():
    from rtxpt_amd import scenes
    p, i = _blades()
    b = scenes.SceneBuilder(); m = b.add_material(scenes.make_material())
    b.begin_mesh(); b.add_geometry(p, i, m); b.add_instance(b.end_mesh())
    return b.finish()


def _blade_rays(n=2048):
    """even rows: parallel to the axis, off it (they lie in no blade's plane and cross none: misses that enter every box); odd rows: tilted, through the blades"""
    r = np.random.default_rng(0xD33F)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0] = r.uniform(-0.3, 0.3, n); rays[:, 1] = r.uniform(-0.3, 0.3, n); rays[:, 2] = -1.0
    # (the blades' planes pass through the axis at 25 .. 65 degrees: a parallel ray in the second or fourth quadrant keeps ox sin + |oy| cos >= 0.06 away from all of them)
    rays[::2, 0] = r.uniform(0.05, 0.3, n // 2); rays[::2, 1] = -r.uniform(0.05, 0.3, n // 2)
    d = np.stack([r.uniform(-0.02, 0.02, n), r.uniform(-0.02, 0.02, n), np.ones(n)], 1); d[::2, :2] = 0.0; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 4:7] = d; rays[:, 7] = K_MAX_RAY_TRAVEL
    return rays


def _walk_depths(rb, rays_xy_oz):
    """For rays (ox, oy, oz) along +z: the deepest stack of the device's walk in closest-hit order (front to back, ties to the lower child slot) and in occlusion order (by
    child slot), and the order-free bound of the tree. A child is entered if its decoded box holds (ox, oy) and T8_HIT's rule admits its z interval (it always does for a
    box ahead of the origin); the near key is the float32 tn = max(zlo - oz, 0) with its three low bits cleared, as the device ranks it."""
    import bvh_ref
    P = bvh_ref.parse(rb); ref = P["ref"]; N = ref.shape[0]
    lo = np.stack([bvh_ref.decode32(P["qlo"][..., a], P["scale"][:, None, a], P["org"][:, None, a]) for a in range(3)], -1)          # [N, 8, 3] float32
    hi = np.stack([bvh_ref.decode32(P["qhi"][..., a], P["scale"][:, None, a], P["org"][:, None, a]) for a in range(3)], -1)
    valid = ref != bvh_ref.EMPTY; inner = valid & ((ref & bvh_ref.LEAF_BIT) == 0)
    def bound(nd):
        kids = [int(ref[nd, c]) for c in range(8) if inner[nd, c]]
        return int(valid[nd].sum()) - 1 + max([bound(k) for k in kids] + [0])
    def walk(ox, oy, oz, ordered):
        stack, cur, deepest = [], 0, 0
        while True:
            if cur != bvh_ref.EMPTY and not (cur & bvh_ref.LEAF_BIT):
                kids = []
                for c in range(8):
                    if not valid[cur, c]: continue
                    l, h = lo[cur, c], hi[cur, c]
                    tn = max(np.float32(l[2] - np.float32(oz)), np.float32(0.0)); tf = np.float32(h[2] - np.float32(oz))
                    if l[0] <= ox <= h[0] and l[1] <= oy <= h[1] and tn <= tf * np.float32(1.0000012):
                        kids.append(((int(np.float32(tn).view(np.uint32)) & ~7) if ordered else 0, c, int(ref[cur, c])))
                kids.sort()
                if kids:
                    stack.extend(k[2] for k in reversed(kids[1:])); deepest = max(deepest, len(stack)); cur = kids[0][2]; continue
            if not stack: return deepest
            cur = stack.pop()
    out = np.array([[walk(float(x), float(y), float(z), True), walk(float(x), float(y), float(z), False)] for x, y, z in rays_xy_oz])
    return out, bound(0)


def test_deep_stacks_take_both_push_paths_and_lose_nothing():
    import hit_ref
    sc = _once("blades", _blade_scene); rays = _blade_rays()
    runs, closest, visible, rb = _routes(sc, rays, rays, variants=True)
    par = rays[0:64:2]          # parallel rays of the first wave's chunk
    depths, bound = _walk_depths(rb, par[:, 0:3])
    print("deep stacks: %d nodes; walk depth closest-hit order min / max %d / %d, occlusion order %d / %d; order-free bound %d" % (rb["nodes"].shape[0], depths[:, 0].min(), depths[:, 0].max(), depths[:, 1].min(), depths[:, 1].max(), bound))
    assert depths[:, 0].max() > BVH8_STACK and depths[:, 1].max() > BVH8_STACK, depths.max(0)          # the guarded pushes and the global tail run on either route
    assert bound <= BVH8_STACK + T8_SPILL_DEPTH, bound                                                # ... and no ray can overflow the tail
    V = hit_ref.world_triangles(sc); ref = hit_ref.Reference(V, rays)
    assert ref.skipped_share() <= MAX_SKIPPED, ref.skipped_share()
    assert ref.any_hit.any() and ref.all_miss[::2].all()          # the parallel rays miss every blade: the walk above is theirs
    for label, (route, out, st) in runs.items():
        if route == "shadow": hit_ref.check_visibility(ref, out, "blades (%s)" % label)
        else: hit_ref.check_closest(ref, out, "blades (%s)" % label)
    _hold_to_oracle("blades", runs, closest, visible)


# ---- a small frame
def _frames(fused_modes=(1, 0)):
    """{fused mode: (radiance, (extendRays, shadowRays, hits))} of the zoo frame in this process"""
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    sc = _once("zoo", _zoo_scene); S = scenes.default_settings(useFp16Types=1); camd = scenes.bridge_camera(64, 64, **ZOO_CAM)
    out = {}
    for mode in fused_modes:
        t = pt.PathTracer(); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(64, 64); t.set_tail_paths(0); t.set_fused_traversal(mode)
        try:
            t.reset_accumulation(); st = t.render(0, 2)
            out[mode] = (t.radiance().copy(), (int(st["extendRays"]), int(st["shadowRays"]), int(st["hits"])))
        finally:
            t.close()
    return out


def _oracle_frame():
    from rtxpt_amd import scenes
    from oracle import ptref
    sc = _once("zoo", _zoo_scene); S = scenes.default_settings(useFp16Types=1); camd = scenes.bridge_camera(64, 64, **ZOO_CAM)
    o = ptref.Oracle(lp16=True); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(64, 64)
    o.render(0, 2); c = o.counters(); out = (o.radiance(), (c["extendRays"], c["shadowRays"], c["hits"])); o.close()
    return out


@pytest.mark.parametrize("batches", [1, 2])
def test_small_frame_of_the_zoo_equals_the_oracle(batches, tmp_path):
    want = _once("zoo frame", _oracle_frame)
    if batches == 1:
        assert "MI355PT_BATCHES" not in os.environ
        got = _frames()
    else:
        path = str(tmp_path / "frames.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=300, env=dict(os.environ, MI355PT_BATCHES="2"), cwd=ROOT)
        assert r.returncode == 0, "exit %d\n%s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        z = np.load(path); got = {m: (z["rad%d" % m], tuple(int(v) for v in z["cnt%d" % m])) for m in (1, 0)}
    assert want[1][0] >= 64 * 64 * 2
    for mode, (rad, cnt) in got.items():
        a, b = _bits(rad), _bits(want[0])
        assert np.array_equal(a, b), "%d batch(es), fused %d: %d pixels differ from the oracle" % (batches, mode, int((a != b).any(-1).sum()))
        assert cnt == tuple(int(v) for v in want[1]), "%d batch(es), fused %d: counts %s, the oracle's %s" % (batches, mode, cnt, want[1])


if __name__ == "__main__":          # the two-batch leg: MI355PT_BATCHES is set by the parent test
    sys.path.insert(0, ROOT)
    f = _frames()
    np.savez(sys.argv[1], **{"rad%d" % m: f[m][0] for m in f}, **{"cnt%d" % m: np.array(f[m][1], np.int64) for m in f})

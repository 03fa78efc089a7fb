"""The child slots of the wide tree, ordered for occlusion rays (run with -m gpu; rtxpt_amd/csrc/pt_build_wide.h wide_occlusion_slots, pt_build.hip k_collapse8): an any-hit
query walks a node's hit children in slot order, so the collapse hands the slots out by descending (area of the child's quantised box) / (triangles below the child). The hit
definition does not depend on the tree, so nothing a frame or a query returns may change; only the slots do. MI355PT_OCCLUSION_SLOT_ORDER=0 at pt_create restores collapse order.

  * frames with the switch at 1 and at 0 equal each other and the oracle, bit for bit, with equal ray and hit counts: pin scenes in both lp builds, an alpha-tested card between
    an emitter and the floor, a single triangle, an empty scene; fused and separate traversal launches; four pipelined batches against the reference-text fixture
  * pt_trace_visibility on a few thousand random segments through alpha-tested geometry equals the oracle's answer
  * through the read-back hook: both trees hold, node by node, the same multiset of (child, quantised box); both pass the checker of tests/bvh_ref.py; the children fill the
    first n slots; a numpy restatement of the rule, applied to the collapse-order tree, gives the slots of the ordered tree
  * a refit (pt_animate) keeps every child in its slot"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SWITCH = "MI355PT_OCCLUSION_SLOT_ORDER"
EMPTY, LEAF_BIT = 0xFFFFFFFF, 0x80000000


def _bits(a): return np.asarray(a).view(np.uint32)


def _tracer(switch, **kw):
    """the switch is read at pt_create"""
    import rtxpt_amd as pt
    old = os.environ.get(SWITCH); os.environ[SWITCH] = str(switch)
    try:
        return pt.PathTracer(**kw)
    finally:
        if old is None: os.environ.pop(SWITCH, None)
        else: os.environ[SWITCH] = old


# ---- the scenes
def _card_under_the_light():
    """a Cornell-like room whose only emitter hangs above an alpha-tested checkerboard card: every visibility ray from the floor to the emitter meets the card's two triangles"""
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
    cy = Y - 0.12
    p, i, uv, n, t = scenes.quad((0.10, cy, 0.12), (0.46, cy, 0.12), (0.46, cy, 0.44), (0.10, cy, 0.44), uv_scale=3.0)
    b.begin_mesh(); b.add_geometry(p, i, card, uv=uv, normal=n, tangent=t, geom_flags=scenes.GEOMF_ALPHA_TESTED); b.add_instance(b.end_mesh())
    cam = dict(pos=(0.278, 0.273, -0.8), direction=(0, 0, 1), up=(0, 1, 0), fov_y=0.6859, near_z=0.01, far_z=100.0, focal_distance=1.0)
    return b.finish(), cam


def _single_triangle():
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder(); m = b.add_material(scenes.make_material(base=(0.7, 0.6, 0.5)))
    b.begin_mesh(); b.add_geometry(np.array([[-1, 0, 1], [1, 0, 1], [0, 1.5, 1.2]], np.float32), np.array([0, 1, 2], np.uint32), m); b.add_instance(b.end_mesh())
    b.set_environment(scenes.sky_equirect(64, 32))
    return b.finish(), dict(pos=(0.0, 0.6, -3.0), direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov_y=0.9)


def _empty():
    from rtxpt_amd import scenes
    b = scenes.SceneBuilder(); b.add_material(scenes.make_material()); b.set_environment(scenes.sky_equirect(64, 32))
    return b.finish(), dict(pos=(0.0, 1.0, -4.0), direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov_y=0.9)


@functools.lru_cache(maxsize=None)
def _case(name):
    """name -> (scene, bridge camera, settings, w, h, first, n), built once"""
    import pin_scenes
    from rtxpt_amd import scenes
    lp = 1 if name.endswith("_lp16") else 0; base = name[:-5] if lp else name
    own = {"card": _card_under_the_light, "triangle": _single_triangle, "empty": _empty}
    if base in own:
        sc, cam = own[base](); S, w, h, first, n = scenes.default_settings(useFp16Types=lp), 64, 36, 0, 2
    else:
        make, S, w, h, first, n = (pin_scenes.cases_lp16() if lp else pin_scenes.cases())[base]
        sc, cam = make()
    return sc, scenes.bridge_camera(w, h, **cam), S, w, h, first, n


@functools.lru_cache(maxsize=None)
def _oracle_frame(name):
    """the oracle's frame and (extend rays, visibility rays, hits), computed once and shared"""
    from oracle import ptref
    sc, camd, S, w, h, first, n = _case(name)
    o = ptref.Oracle(lp16=name.endswith("_lp16")); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h); o.render(first, n)
    rad = o.radiance().copy(); rad.setflags(write=False); c = o.counters()
    return rad, (c["extendRays"], c["shadowRays"], c["hits"])


FRAMES = ["c2", "c2_lp16", "bistro_like", "bistro_like_lp16", "bistro_like_c5_lp16", "card", "card_lp16", "triangle_lp16", "empty_lp16"]


@pytest.mark.parametrize("fused", [0, 1], ids=["separate", "fused"])
@pytest.mark.parametrize("name", FRAMES)
def test_frames_equal_the_oracle_with_either_slot_order(name, fused):
    sc, camd, S, w, h, first, n = _case(name)
    want, counts = _oracle_frame(name)
    for switch in (1, 0):
        t = _tracer(switch)
        try:
            t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h); t.set_fused_traversal(fused)
            st = t.render(first, n); got = t.radiance()
        finally:
            t.close()
        bad = (_bits(got) != _bits(want)).any(-1)
        assert not bad.any(), "%s, switch %d: %d of %d pixels differ from the oracle" % (name, switch, int(bad.sum()), bad.size)
        assert (st["extendRays"], st["shadowRays"], st["hits"]) == counts, (name, switch)
    if name.startswith("card"): assert counts[1] > 0


@pytest.mark.parametrize("name", ["bistro_like_xl", "bistro_like_xl_lp16"])
def test_four_batches_equal_the_reference_text_frame_with_either_slot_order(name):
    """1280 x 720 x 4 samples: four pipelined batches, straggler rounds, the tail kernel; fused launches with the ordered slots, separate ones with collapse order and back. The
    fixture (tests/golden/reference_integrator_golden_xl.npz) holds every sixteenth row, the digest of the whole frame and the ray counts."""
    import pin_scenes
    from rtxpt_amd import scenes
    make, S, w, h, first, n = pin_scenes.xl_cases()[name]
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_integrator_golden_xl.npz"))
    sc, cam = make(); camd = scenes.bridge_camera(w, h, **cam); frames = []
    for switch, fused in ((1, 1), (0, 0), (1, 0)):
        t = _tracer(switch)
        try:
            t.set_tail_paths(32768); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h); t.set_fused_traversal(fused)
            st = t.render(first, n); rad = t.radiance()
        finally:
            t.close()
        rows = rad[::pin_scenes.XL_ROW_STEP]
        assert not (_bits(rows) != _bits(g[name + "_rows"])).any(), (name, switch, fused)
        assert np.array_equal(pin_scenes.frame_digest(rad), g[name + "_sha256"]), (name, switch, fused)
        assert (st["extendRays"], st["shadowRays"]) == tuple(int(v) for v in g[name + "_rays"])
        frames.append((rad, st["hits"]))
    for rad, hits in frames[1:]: assert np.array_equal(_bits(rad), _bits(frames[0][0])) and hits == frames[0][1]


def test_visibility_of_random_segments_equals_the_oracle():
    """4 096 segments between random points of the bistro-like scene's bounds (alpha-tested foliage among the occluders), some of them short: the any-hit loop's answer, which is
    the only thing the slot order could change, against the oracle's, with the ordered slots and with collapse order"""
    from oracle import ptref
    sc, camd, S, w, h, first, n = _case("bistro_like_lp16")
    import hit_ref
    V = hit_ref.world_triangles(sc).reshape(-1, 3); lo, hi = V.min(0), V.max(0)
    rng = np.random.default_rng(0x0CC1)
    a = lo + rng.random((4096, 3)) * (hi - lo); b = lo + rng.random((4096, 3)) * (hi - lo)
    b[::4] = a[::4] + rng.normal(size=(1024, 3)) * 0.02 * np.linalg.norm(hi - lo)
    d = b - a; L = np.linalg.norm(d, axis=1)
    rays = np.zeros((4096, 8), np.float32); rays[:, 0:3] = a; rays[:, 4:7] = d / L[:, None]; rays[:, 7] = L
    o = ptref.Oracle(); o.set_scene(sc); want = o.trace_visibility(rays)
    assert 0.05 < want.mean() < 0.95, want.mean()          # both outcomes are well represented
    for switch in (1, 0):
        t = _tracer(switch)
        try:
            t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(w, h)
            got, _ = t.trace_visibility(rays)
        finally:
            t.close()
        assert np.array_equal(got, want), "switch %d: %d of %d segments differ" % (switch, int((got != want).sum()), len(want))


# ---- the tree itself, through the read-back hook
def _tree(rb):
    """per node and slot: the child's identity — (first triangle slot, triangles) of everything below it, which no numbering of the nodes changes — its codes, its triangle
    count; per node the same pair for the node itself"""
    nd = np.ascontiguousarray(rb["nodes"], np.uint32).reshape(-1, 32); N = nd.shape[0]
    ref = nd[:, 4:28:3].astype(np.int64); q0 = nd[:, 5:28:3].copy(); q1 = nd[:, 6:28:3].copy(); exps = nd[:, 3].copy()
    filled = ref != EMPTY; leaf = filled & ((ref & LEAF_BIT) != 0); inner = filled & ~leaf
    cfirst = np.where(leaf, (ref & 0x7FFFFFFF) >> 3, np.int64(1) << 30); ccnt = np.where(leaf, (ref & 7) + 1, 0)
    nfirst = np.zeros(N, np.int64); ncnt = np.zeros(N, np.int64); start = np.asarray(rb["level_start"], np.int64)
    assert len(start) == rb["levels"] + 1 and start[-1] == N
    for l in range(rb["levels"] - 1, -1, -1):
        a, b = int(start[l]), int(start[l + 1]); m = inner[a:b]; c = ref[a:b][m]
        cf = cfirst[a:b]; cf[m] = nfirst[c]; cc = ccnt[a:b]; cc[m] = ncnt[c]
        nfirst[a:b] = cf.min(1); ncnt[a:b] = cc.sum(1)
    cid = np.where(filled, (cfirst << 24) | ccnt, -1); nid = (nfirst << 24) | ncnt
    assert len(np.unique(nid)) == N
    order = np.argsort(nid)
    return dict(nid=nid[order], cid=cid[order], q0=q0[order], q1=q1[order], exps=exps[order], cnt=ccnt[order], filled=filled[order], n=(exps >> 24)[order], ref=ref[order])


def _rule_slots(t):
    """numpy restatement of wide_occlusion_slots over the children in the order of tree t: slot[node, k] of child k (8 for an empty slot)"""
    f32 = np.float32
    e = np.stack([t["exps"] & 255, (t["exps"] >> 8) & 255, (t["exps"] >> 16) & 255], 1).astype(np.int64); d = e.max(1, keepdims=True) - e
    s = np.where(d < 40, ((127 - np.minimum(d, 100)).astype(np.uint32) << 23).view(f32), f32(0))          # [N, 3]
    q0, q1 = t["q0"].astype(np.int64), t["q1"].astype(np.int64)
    dx = (((q0 >> 24) & 255) - (q0 & 255)).astype(f32) * s[:, None, 0]; dy = ((q1 & 255) - ((q0 >> 8) & 255)).astype(f32) * s[:, None, 1]
    dz = (((q1 >> 8) & 255) - ((q0 >> 16) & 255)).astype(f32) * s[:, None, 2]
    area = (dx * dy + dy * dz) + dz * dx
    assert area.dtype == f32
    with np.errstate(divide="ignore", invalid="ignore"):
        key = np.where(t["filled"], area / np.maximum(t["cnt"], 1).astype(f32), f32(-1))
    j = np.arange(8)
    before = (key[:, :, None] > key[:, None, :]) | ((key[:, :, None] == key[:, None, :]) & (j[None, :, None] < j[None, None, :]))          # [node, j, k]: child j goes before child k
    return np.where(t["filled"], before.sum(1), 8)


TREES = ["uniform-1", "uniform-9", "uniform-1000", "plane-1000", "sizes-4097", "piled-20000"]


@pytest.mark.parametrize("name", TREES + ["uniform-1000:sah", "uniform-1000:ploc"])
def test_both_trees_hold_the_same_children_and_the_rule_gives_the_slots(name):
    """name:sah — the host builder's topology (MI355PT_BVH_BUILDER=sah; its collapse is the device's k_collapse8 too); name:ploc — prefer_fast_build (the greedy collapse)"""
    import bvh_cases, bvh_ref
    name, _, builder = name.partition(":")
    c = bvh_cases.case(name); trees = {}
    for switch in (1, 0):
        if builder == "sah": os.environ["MI355PT_BVH_BUILDER"] = "sah"
        try:
            g = _tracer(switch, test_hooks=True, prefer_fast_build=(builder == "ploc"))
        finally:
            os.environ.pop("MI355PT_BVH_BUILDER", None)
        try:
            from rtxpt_amd import scenes
            g.set_scene(c["sc"]); g.set_settings(scenes.default_settings()); rb = g.get_bvh8()
        finally:
            g.close()
        bvh_ref.check(rb, c["V"]).require("%s, switch %d" % (name, switch))
        t = trees[switch] = _tree(rb)
        assert np.array_equal(t["filled"], np.arange(8)[None, :] < t["n"][:, None]), "children outside the first n slots"
    on, off = trees[1], trees[0]
    assert np.array_equal(on["nid"], off["nid"]) and np.array_equal(on["n"], off["n"]) and np.array_equal(on["exps"], off["exps"])
    # the same multiset of (child, codes) in every node
    def canon(t):
        k = np.argsort(t["cid"], axis=1, kind="stable")
        return np.stack([np.take_along_axis(t[f].astype(np.int64), k, 1) for f in ("cid", "q0", "q1")], -1)
    assert np.array_equal(canon(on), canon(off))
    # collapse order is what the switch at 0 leaves: the rule over it names the slot of every child of the ordered tree
    slot = _rule_slots(off); want = np.full((len(off["nid"]), 9), -1, np.int64); rows = np.arange(len(off["nid"]))[:, None]
    want[rows, slot] = off["cid"]
    moved = int((want[:, :8] != off["cid"]).any(1).sum())
    print("%s: %d wide nodes, the rule moves children in %d" % (name, len(off["nid"]), moved))
    assert np.array_equal(want[:, :8], on["cid"]), "%d nodes whose slots are not the rule's" % int((want[:, :8] != on["cid"]).any(1).sum())
    if len(off["nid"]) > 100: assert moved > 0


@pytest.mark.parametrize("how", ["vertices", "instances"])
def test_a_refit_keeps_every_child_in_its_slot(how):
    import bvh_cases, bvh_ref
    from rtxpt_amd import scenes
    c = bvh_cases.refit_case(1000, how); pose = c["poses"]["B"]
    g = _tracer(1, test_hooks=True)
    try:
        g.set_scene(c["sc"]); g.set_settings(scenes.default_settings()); first = g.get_bvh8()
        if how == "instances": g.animate(instances=pose["instances"])
        else: g.animate(positions=pose["positions"])
        after = g.get_bvh8()
    finally:
        g.close()
    bvh_ref.check(after, pose["V"]).require("refit-%s pose B" % how)
    assert np.array_equal(first["nodes"][:, 4:28:3], after["nodes"][:, 4:28:3]) and np.array_equal(first["level_start"], after["level_start"])
    assert not np.array_equal(first["nodes"][:, 5:28:3], after["nodes"][:, 5:28:3])          # (the boxes did move)
    off = _tracer(0, test_hooks=True)
    try:
        off.set_scene(c["sc"]); off.set_settings(scenes.default_settings()); plain = _tree(off.get_bvh8())
    finally:
        off.close()
    assert (_tree(first)["cid"] != plain["cid"]).any()          # the order the refit kept is the rule's, not collapse order

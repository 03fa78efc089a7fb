"""The device-built BVH8, node by node (run with -m gpu): every case of tests/bvh_cases.py is built, read back through PathTracer.get_bvh8() (include/mi355pt_testhooks.h) and
held to the checker tests/bvh_ref.py — structure, conservative under the traversal's own decode, the stored pads, tight within the derived K_STEPS = 2, smallest scale, origin;
every node and every triangle. The reference is the geometry; nothing depends on how a build numbered its nodes. The default builder on the whole zoo, the other builders (plain
PLOC, Karras, host SAH, pt_animate(rebuild=True)) on a subset, refits to a pose whose boxes shrink and back (the bytes of the first read-back again), two contexts (equal
canonical forms), the fill and the float64 cost of the default tree against plain PLOC's. The checker's own test with the derivations: tests/test_bvh_reference.py.

Measured on an MI355X: see DESIGN.md section 5, "What the tree is held to"."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_cases
import bvh_ref

pytestmark = pytest.mark.gpu
BUILDERS = ("ploc", "karras", "sah", "rebuild")


def _device(sc, builder=None):
    """a context with test hooks, one at a time. builder: None = the default (PLOC + re-insertion + cost-driven wide nodes), "ploc" = prefer_fast_build, "karras" / "sah" =
    MI355PT_BVH_BUILDER, "rebuild" = the default build followed by pt_animate(rebuild=True)"""
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    if builder in ("karras", "sah"): os.environ["MI355PT_BVH_BUILDER"] = builder
    try:
        g = pt.PathTracer(prefer_fast_build=(builder == "ploc"), test_hooks=True)
    finally:
        os.environ.pop("MI355PT_BVH_BUILDER", None)
    try:
        g.set_scene(sc); g.set_settings(scenes.default_settings())
        if builder == "rebuild": g.get_bvh8(); g.animate(instances=sc["instances"], rebuild=True)
        want = {None: 3, "ploc": 0, "karras": 1, "sah": 2, "rebuild": 0}[builder]
        if len(sc["indices"]) > 3: assert g.bvh_info()["builder"] == want, (g.bvh_info(), builder)
    except BaseException:
        g.close(); raise
    return g


def _check(g, V, what):
    rb = g.get_bvh8()
    t0 = time.perf_counter(); r = bvh_ref.check(rb, V); dt = time.perf_counter() - t0
    s = r.stats
    print("%s: %d nodes, %d triangles, %d levels, margin %.3g steps, slack %.3g steps (K_STEPS %d), %.2f children / node, cost %.6g, checker %.2f s"
          % (what, s["nodes"], s["tris"], s["levels"], s.get("margin_steps", float("nan")), s.get("slack_steps", float("nan")), bvh_ref.K_STEPS, s.get("mean_children", 0), s.get("cost", 0), dt))
    r.require(what)
    assert s["below_root"] == len(V) and dt < 5.0, (what, dt)
    return rb, r


@pytest.mark.parametrize("name", bvh_cases.NAMES)
def test_default_builder_on_the_whole_zoo(name):
    c = bvh_cases.case(name); g = _device(c["sc"])
    try:
        _check(g, c["V"], name)
    finally:
        g.close()


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", bvh_cases.BUILDER_NAMES)
def test_the_other_builders(name, builder):
    c = bvh_cases.case(name); g = _device(c["sc"], builder)
    try:
        _check(g, c["V"], "%s (%s)" % (name, builder))
    finally:
        g.close()


@pytest.mark.parametrize("builder", [None, "ploc", "rebuild"])
@pytest.mark.parametrize("name", ["identical-456", "identical-1000", "line-1000"])
def test_tied_merge_areas_do_not_build_a_chain(name, builder):
    """Equal merged areas over a whole PLOC window — identical triangles, or triangles on one line, whose every merged box has area 0 — used to go to the lower index alone: only
    slots 0 and 1 were mutual nearest neighbours, one merge a pass, a binary chain n deep and n / 7 wide levels (identical-456: 66, the first size beyond BVH_MAX_WIDE_LEVELS = 64,
    which cost the scene its fast refit; identical-1000: 143; line-1000: 998). k_ploc_nn now hands such ties (one box twice, or a merged box without area) to slot i ^ 1 first: a list of equal clusters pairs (2k, 2k + 1) and halves
    every pass, the binary tree is ceil(log2 n) deep and the wide tree no deeper."""
    c = bvh_cases.case(name); g = _device(c["sc"], builder)
    try:
        rb, _ = _check(g, c["V"], "%s (%s)" % (name, builder or "default"))
    finally:
        g.close()
    assert rb["levels"] <= int(np.ceil(np.log2(c["n"]))), rb["levels"]


def _animate(g, c, pose):
    if pose is None: inst, pos, ranges = c["sc"]["instances"], c["positions"], None
    else: inst, pos, ranges = pose["instances"], pose["positions"], pose["ranges"]
    if c["name"].startswith("refit-instances"): g.animate(instances=inst)
    elif c["name"].startswith("refit-ranges"): g.animate(positions=pos, vertex_ranges=c["poses"]["B"]["ranges"])
    else: g.animate(positions=pos)


@pytest.mark.parametrize("how", ["instances", "vertices", "ranges"])
@pytest.mark.parametrize("n", [9, 1000, 20000])
def test_refit_to_a_shrunken_pose_and_back(n, how):
    """A -> B (the whole checker against B's geometry: the tightness clause is what catches a box that did not shrink) -> A: nodes, triangle records, pads, bounds and the level
    table bit-equal to the first read-back — DESIGN.md section 4's "the bytes equal a from-scratch emission over the same topology". The first read-back is itself what the refit's
    level pass wrote (a build ends with one), so no field is exempt. And A again after a second, different detour C."""
    c = bvh_cases.refit_case(n, how); g = _device(c["sc"])
    try:
        first, _ = _check(g, c["V"], c["name"] + " A")
        _animate(g, c, c["poses"]["B"]); _check(g, c["poses"]["B"]["V"], c["name"] + " B")
        _animate(g, c, None); back, _ = _check(g, c["V"], c["name"] + " A again")
        differ = bvh_ref.same_bytes(first, back)
        print("%s: refit back to A, %d bytes differ" % (c["name"], differ))
        assert differ == 0
        _animate(g, c, c["poses"]["C"]); _check(g, c["poses"]["C"]["V"], c["name"] + " C")
        _animate(g, c, None)
        assert bvh_ref.same_bytes(first, g.get_bvh8()) == 0
    finally:
        g.close()


@pytest.mark.parametrize("n", [1000, 20000])
def test_two_contexts_build_the_same_tree_up_to_numbering(n):
    c = bvh_cases.case("uniform-%d" % n); out = []
    for _ in range(2):
        g = _device(c["sc"])
        try:
            rb, r = _check(g, c["V"], c["name"])
        finally:
            g.close()
        out.append((rb, r))
    (a, ra), (b, rb) = out
    assert np.array_equal(ra.stats["canonical"], rb.stats["canonical"]), "two builds of one scene differ in more than their numbering"
    assert np.array_equal(np.sort(a["nodes"][:, 3] >> 24), np.sort(b["nodes"][:, 3] >> 24)) and a["levels"] == b["levels"] and ra.stats["cost"] == rb.stats["cost"]
    assert np.array_equal(a["tris"], b["tris"])          # the leaf order comes from prefix sums, not from atomics


@pytest.mark.parametrize("name", ["uniform-20000", "piled-20000"])
def test_quality_of_the_default_tree(name):
    """the fill test_bvh_sah_host.py holds the host builder to, all twelve re-insertion passes, and a float64 wide-tree cost (every wide-node and every leaf visit costs its
    surface area, pt_build_wide.h) no higher than plain PLOC's on the same scene. Both cost-lowering stages are held to "lower" on the CPU at these modes (test_bvh_sah_host.py:
    the re-insertion checker's modes 0 - 2, the wide-node programme against the host's on modes 0, 2, 3)."""
    c = bvh_cases.case(name); cost = {}
    for builder in (None, "ploc"):
        g = _device(c["sc"], builder)
        try:
            _, r = _check(g, c["V"], "%s (%s)" % (name, builder or "default")); info = g.bvh_info()
        finally:
            g.close()
        cost[builder] = r.stats["cost"] / r.stats["root_area"]
        if builder is None:
            assert r.stats["mean_children"] > 5.5, r.stats["mean_children"]
            assert info["optimiserPasses"] == 12, info
    print("%s: wide-tree cost / root area: default %.6g, plain PLOC %.6g, ratio %.4f" % (name, cost[None], cost["ploc"], cost[None] / cost["ploc"]))
    assert cost[None] <= cost["ploc"]


def test_refusals():
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    c = bvh_cases.case("uniform-9")
    g = pt.PathTracer()
    try:
        g.set_scene(c["sc"]); g.set_settings(scenes.default_settings())
        with pytest.raises(RuntimeError): g.get_bvh8()
        assert not hasattr(g.L, "pt_get_bvh8")          # the shipped library exports nothing new
    finally:
        g.close()
    g = _device(c["sc"])
    try:
        with pytest.raises(pt.PtError): g.get_bvh8(short_by=1)
        _check(g, c["V"], "after the refusal")
    finally:
        g.close()
    b = scenes.SceneBuilder(); b.add_material(scenes.make_material())
    g = _device(b.finish())
    try:
        rb = g.get_bvh8()
        assert rb["nodes"].shape[0] == 0 and rb["tris"].shape[0] == 0 and rb["levels"] == 0 and bvh_ref.check(rb, np.zeros((0, 3, 3))).ok
    finally:
        g.close()

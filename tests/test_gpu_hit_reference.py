"""The device's hit test (run with -m gpu) — the leaf block of pt_traverse8.h (t8_leaf_block) under the device-built BVH8, default builder and host SAH, and after a refit — held to the
float64 restatement tests/hit_ref.py on the zoo of tests/hit_cases.py, and to the oracle bit for bit on the same rays. The CPU twin with the derivation of the bounds, the
zoo and the far-origin contract: tests/test_hit_reference.py, tests/hit_ref.py, tests/hit_cases.py.

Per ray: no leak, no false hit, the reported primitive is not a clear miss and sits at the reported t, t / u / v within the derived bounds (they hold for any float32
evaluation of the text, so the device gets the oracle's bound, not twice it), interval ends, visibility; rays through a shared edge hit; at most 2 % of a case's rays
skipped (asserted; largest share 1.2 %). Measured on an MI355X over the whole zoo, both builders: leaks 0, false hits 0, wrong primitives 0, largest error / bound
0.48 (t), 0.11 (u), 0.14 (v) — the oracle's figures, as every record is bit-identical with the oracle's (asserted)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hit_cases
import hit_ref

pytestmark = pytest.mark.gpu
MAX_SKIPPED = 0.02


def _device(sc, builder=None):
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    if builder: os.environ["MI355PT_BVH_BUILDER"] = builder
    try:
        g = pt.PathTracer()
    finally:
        os.environ.pop("MI355PT_BVH_BUILDER", None)
    g.set_scene(sc); g.set_settings(scenes.default_settings())
    if builder: assert g.bvh_info()["builder"] == {"sah": 2}[builder]
    return g


def _oracle(c):
    from rtxpt_amd import scenes
    from oracle import ptref
    o = ptref.Oracle(); o.set_scene(c["sc"]); o.set_settings(scenes.default_settings())
    if c["moved"] is not None: o.set_instances(c["moved"])
    return o


def _run(name, builder):
    c = hit_cases.case(name); ref = hit_cases.reference(name)
    assert ref.skipped_share() <= MAX_SKIPPED, "%s: the reference skips %.2f %% of the rays" % (name, 100 * ref.skipped_share())
    what = "%s (device%s)" % (name, ", " + builder if builder else "")
    g = _device(c["sc"], builder); o = _oracle(c)
    try:
        if c["moved"] is not None: g.animate(instances=c["moved"])          # a refit: the pads are formed again by the refit kernel
        hits, _ = g.trace_closest(c["rays"]); vis, _ = g.trace_visibility(c["rays"])
        print("%s: skipped share %.4f" % (what, ref.skipped_share()))
        hit_ref.check_closest(ref, hits, what)
        hit_ref.check_visibility(ref, vis, what)
        same = (hits.view(np.uint32) == o.trace_closest(c["rays"]).view(np.uint32)).all(1)
        assert same.all(), "%s: %d of %d closest-hit records differ from the oracle's" % (what, int((~same).sum()), same.size)
        assert np.array_equal(vis, o.trace_visibility(c["rays"])), what
    finally:
        g.close(); o.close()


@pytest.mark.parametrize("name", hit_cases.NAMES)
def test_device_hit_test_against_the_float64_reference(name):
    _run(name, None)


@pytest.mark.parametrize("name", hit_cases.BUILDER_NAMES)
def test_device_hit_test_against_the_float64_reference_host_sah_builder(name):
    _run(name, "sah")


def test_interval_ends_are_exclusive_where_the_arithmetic_is_exact():
    """tmin < t < tmax, both strict (hit_cases.exact_end_rays: every float32 operation of these rays is exact, the reported t is the exact t = 2)"""
    for sc, rays, expect in hit_cases.exact_end_rays():
        g = _device(sc)
        try:
            h, _ = g.trace_closest(rays); vis, _ = g.trace_visibility(rays)
        finally:
            g.close()
        assert np.array_equal(h.view(np.uint32)[:, 1] != hit_ref.MISS, expect), (h, expect)
        assert (h[expect, 0] == 2.0).all() and np.array_equal(vis == 0, expect)


@pytest.mark.parametrize("name", ["ico-origin", "ico-1e3-all"])
def test_rays_through_a_shared_edge_hit_one_of_its_two_triangles(name):
    """each triangle alone is borderline on the edge; their union is not (hit_ref.check_shared_edges)"""
    e = hit_cases.shared_edge_case(name)
    g = _device(e["sc"])
    try:
        hits, _ = g.trace_closest(e["rays"])
    finally:
        g.close()
    hit_ref.check_shared_edges(e["V"], e["rays"], e["T1"], e["k1"], e["T2"], e["k2"], hits, name + " (device)")


def test_a_ray_with_a_negative_tmin_is_refused_before_it_reaches_the_device():
    """tmin >= +0 is the contract (include/mi355pt.h): the traversal orders a node's children by the bit pattern of their entry distance max(slab, tmin), and a negative one
    made the push that follows index the stack with a wrapped count — found by this zoo when two of its interval variants fell below 0. pt_trace_closest /
    pt_trace_visibility check every ray on the host and return PT_ERROR_INVALID_ARGUMENT; the context stays usable."""
    import rtxpt_amd as pt
    g = _device(hit_cases.case("quadz-origin")["sc"])
    try:
        good = np.array([[0.25, 0.5, -2, 0, 0, 0, 1, 1e30]] * 4, np.float32)
        for bad in (-1e-3, -0.0, float("nan"), -float("inf")):
            rays = good.copy(); rays[2, 3] = bad
            with pytest.raises(pt.PtError): g.trace_closest(rays)
            with pytest.raises(pt.PtError): g.trace_visibility(rays)
        h, _ = g.trace_closest(good)
        assert (h.view(np.uint32)[:, 1] != hit_ref.MISS).all() and (h[:, 0] == 2.0).all()
    finally:
        g.close()


@pytest.mark.parametrize("name", ["quadz-origin", "box-origin", "ico-origin", "grid-origin"])
def test_no_leak_at_the_stated_origin_distance(name):
    """the far-origin contract of pt_trace_closest: zero leaks with the origin hit_cases.MAX_ORIGIN_DIAGONALS scene diagonals from the aim point"""
    c = hit_cases.case(name)
    rays = hit_cases.far_origin_rays(name, hit_cases.MAX_ORIGIN_DIAGONALS, 2000)
    ref = hit_ref.Reference(c["V"], rays)
    g = _device(c["sc"])
    try:
        hits, _ = g.trace_closest(rays); vis, _ = g.trace_visibility(rays)
    finally:
        g.close()
    hit_ref.check_closest(ref, hits, "%s at %d diagonals (device)" % (name, hit_cases.MAX_ORIGIN_DIAGONALS))
    hit_ref.check_visibility(ref, vis, name)

"""The traversal launches a FRAME runs (run with -m gpu), held to the float64 hit reference tests/hit_ref.py and to the oracle bit for bit, ray by ray.

tests/test_gpu_hit_reference.py reaches the device through pt_trace_closest / pt_trace_visibility: k_trace_probe, an instantiation of traverse8_pairs (no fixed interval, no
sub-tree tasks, no splitting) that no frame runs. pt_trace_route (include/mi355pt_testhooks.h, PathTracer.trace_route) sends the same zoo (tests/hit_cases.py) through
  extend         launch_extend: k_extend (fixed interval: the ray buffer carries the slab selectors; a dry wave cuts its rays into sub-tree tasks), k_extend_tasks<0..>
                 (sub-trees that start at an inner node with a carried best hit, the transposed index space, atomicMin on the hit key), k_resolve_extend ((u, v) by
                 intersect_tri_wt instead of the leaf block)
  extend_ranged  launch_extend(..., ranged): the stable-plane fill pass's first launch. The interval is firstHitInterval's — [0.99 t, 1.01 t] around the oracle's
                 full-interval hit, the whole interval where it misses — and the answer must be the full-interval record: a split ray's lower bound is only a hint
  shadow         launch_shadow on a grouped queue: k_shadow, k_shadow_tasks, k_resolve_shadow<true> — the any-hit variant, "already occluded" through bestKey
  packets        traverse8_packets on stored rays (k_route_packets, the sibling of k_extend_first_packets), then launch_extend over the leftover list
One context per case, every route on it; on the two tube cases and two small ones also the variants: a grid of ONE block (waves take many chunks, only the tail splits)
against the default grid (every wave is dry after one chunk), packets at step cap 8 and at stack bound 2, and a task queue too small for the launch.

Rays: the rows of a case with tmin = 0 — the base rays, their tmax rewritten to kMaxRayTravel (what every extend ray of a frame has), and, for the shadow route, the two
tmax variants behind them. The Reference and the oracle's answers are computed on these rays, once per case.

Asserted besides the per-ray checks: the reference skips at most 2 % of a case's rays; on both tube cases extend, extend_ranged and shadow split rays and feed task round 0
at the default grid, and extend splits a sub-tree AGAIN (task round 1) on at least one of them; the packets commit rays themselves on the small cases and leave rays over
on the tube cases at the default cap; at step cap 8 some case shows both outcomes; a task queue smaller than the launch's tasks is an error with the overflow bit set, not
a short answer; the refusals.

Measured on an MI355X — all thirteen cases, every route and variant: leaks 0, false hits 0, wrong primitives 0, every record the oracle's ((u, v) of k_resolve_extend
included); largest error / bound 0.43 (t), 0.11 (u), 0.11 (v); largest skipped share 0.14 %. Launches of this size (<= T8_SHORT_TAIL_BELOW rays) run two task rounds, so
rounds 2 and 3 are fed nothing. Split rays | sub-trees fed to task round 0 | to round 1 (round 1's count varies by a few dozen between runs: which sub-tree of a ray
lowers the merge key first decides what the others still visit):
                       extend                  extend_ranged           shadow                   one block: extend | extend_ranged | shadow
  tube-4096            1662 | 12409 | ~11500   1209 |  9928 | ~12000   2318 | 15576 | ~21800    81 | 476 | 307    70 | 374 | 272    72 | 393 | 391
  tube-4096-1e3-all    1673 | 12988 | ~11900   1228 |  9930 | ~12800   2342 | 16831 | ~17900    73 | 425 | 388    84 | 542 | 420    76 | 409 | 372
  fan-1e3-all            60 |   197 | 0          28 |   141 | 0         415 |  1959 | 0
  grid-refit-to-1e3       2 |     5 | 0           1 |     4 | 0           2 |    15 | 0         every other case: no ray is split
Packets, committed | left over: the quad, box, fan, grid and tiny cases 8000 | 0 resp. 3000 | 0; ico-origin 2936 | 64 (step cap 8: 256 | 2744, stack bound 2: 160 | 2840);
ico-1e5-size10 2648 | 352; box-1e3-all-verts at stack bound 2 800 | 7200; both tube cases 0 | 2048 at every setting (their leftover launch is the extend column).
A task queue of half the needed size: PT_ERROR_HIP, overflow word 2, task round 0 fed 12409 (extend) / 11499 (shadow, 2048 rays) and round 1 nothing — the task rounds
do not read a queue that overflowed (pt_trace.hip t8_extend_tasks_body: before, they read the unwritten entries below the capacity)."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hit_cases
import hit_ref

pytestmark = pytest.mark.gpu
MAX_SKIPPED = 0.02
K_MAX_RAY_TRAVEL = np.float32(1e15)          # pt_path.h kMaxRayTravel
TUBES = ["tube-4096", "tube-4096-1e3-all"]
SMALL_WITH_VARIANTS = ["box-1e3-all-verts", "ico-origin"]
CASES = ["quadz-1e3-own-axis", "box-1e3-all-verts", "box-1e5-size10-verts", "quadx-grazing", "box-tie", "ico-origin", "ico-1e5-size10", "fan-1e3-all", "grid-axis",
         "grid-refit-to-1e3", "tiny-in-1e3-scene"] + TUBES
CLOSEST_ROUTES = ("extend", "extend_ranged", "packets")


def _head(ref, k):
    """the Reference of the first k rays (every field of it is per ray)"""
    r = copy.copy(ref)
    for f in ("rays", "first", "first_prim", "first_Bt", "all_miss", "any_hit", "skip"): setattr(r, f, getattr(ref, f)[:k])
    return r


_measured = {}


def _measure(name):
    """Everything the device is asked for a case, on one context, and what it is held to: dict of n, rays (shadow rows), ranged (the base rows with firstHitInterval's
    intervals), ref (Reference of the shadow rows; _head(ref, n): of the base rows), closest / visible (the oracle's records), runs {label: (route, out, stats)} and
    errors {label: PtError}. Computed once; a failure is kept and raised again, not retried."""
    if name not in _measured:
        try:
            _measured[name] = _measure_once(name)
        except BaseException as e:
            _measured[name] = e
    if isinstance(_measured[name], BaseException): raise _measured[name]
    return _measured[name]


def _measure_once(name):
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    from oracle import ptref
    c = hit_cases.case(name); n = hit_cases.SPECS[name]["n"]; m = n // 5
    rays = c["rays"][:n + 2 * m].copy()
    assert (rays[:, 3] == 0).all() and (c["rays"][n + 2 * m:, 3] > 0).any()          # the rows with tmin = 0, and only those
    rays[:n, 7] = K_MAX_RAY_TRAVEL
    ref = hit_ref.Reference(c["V"], rays)
    o = ptref.Oracle(); o.set_scene(c["sc"]); o.set_settings(scenes.default_settings())
    try:
        if c["moved"] is not None: o.set_instances(c["moved"])
        closest = o.trace_closest(rays[:n]); visible = o.trace_visibility(rays)
    finally:
        o.close()
    # firstHitInterval (pt_stableplanes.h): t * 0.99f, t * 1.01f in float32 around a hit, the whole interval around a miss
    hit = closest.view(np.uint32)[:, 1] != hit_ref.MISS
    ranged = rays[:n].copy()
    ranged[hit, 3] = closest[hit, 0] * np.float32(0.99); ranged[hit, 7] = closest[hit, 0] * np.float32(1.01)
    assert (ranged[hit, 3] > 0).all() and (ranged[hit, 3] < closest[hit, 0]).all() and (closest[hit, 0] < ranged[hit, 7]).all()
    inputs = {"extend": rays[:n], "extend_ranged": ranged, "shadow": rays, "packets": rays[:n]}
    runs, errors = {}, {}
    g = pt.PathTracer(test_hooks=True); g.set_scene(c["sc"]); g.set_settings(scenes.default_settings())
    try:
        if c["moved"] is not None: g.animate(instances=c["moved"])          # a refit
        def run(label, route, **kw):
            out, st = g.trace_route(route, inputs[route], **kw)
            runs[label] = (route, out, st)
            print("routes %-22s %-24s split=%d tasks=%s packet_rays=%d leftover_rays=%d overflow=%d" % (name, label, st["split"], st["tasks"], st["packet_rays"], st["leftover_rays"], st["overflow"]))
        for route in ("extend", "extend_ranged", "shadow", "packets"): run(route, route)
        if name in TUBES + SMALL_WITH_VARIANTS:
            for route in ("extend", "extend_ranged", "shadow"): run(route + " one block", route, max_blocks=1)
            run("packets step cap 8", "packets", step_cap=8); run("packets stack bound 2", "packets", stack_bound=2)
        if name in TUBES:
            for route in ("extend", "shadow"):          # a task queue of half the sub-trees the launch cuts
                try:
                    g.trace_route(route, inputs[route], task_cap=max(1, runs[route][2]["tasks"][0] // 2))
                except pt.PtError as e:
                    if not (e.stats and e.stats["overflow"]): raise          # (any other error of the device ends the case here)
                    errors[route] = e
    finally:
        g.close()
    return dict(n=n, rays=rays, ranged=ranged, ref=ref, closest=closest, visible=visible, runs=runs, errors=errors)


@pytest.mark.parametrize("name", CASES)
def test_every_route_of_a_frame_against_the_float64_reference_and_the_oracle(name):
    M = _measure(name); n, ref = M["n"], M["ref"]; base = _head(ref, n)
    print("%s: %d triangles, %d + %d rays, skipped share %.4f" % (name, len(ref.V), n, len(M["rays"]) - n, ref.skipped_share()))
    assert ref.skipped_share() <= MAX_SKIPPED and base.skipped_share() <= MAX_SKIPPED, "%s: the reference skips %.2f %% of the rays" % (name, 100 * ref.skipped_share())
    assert ref.any_hit.any() and ref.all_miss.any()
    for label, (route, out, st) in M["runs"].items():
        what = "%s (%s)" % (name, label)
        assert st["overflow"] == 0, what
        if route == "shadow":
            hit_ref.check_visibility(ref, out, what)
            assert np.array_equal(out, M["visible"]), "%s: %d of %d rays differ from the oracle's visibility" % (what, int((out != M["visible"]).sum()), out.size)
        else:
            # (extend_ranged: the answer is the full-interval one, so it is held to the full-interval reference)
            hit_ref.check_closest(base, out, what)
            same = (out.view(np.uint32) == M["closest"].view(np.uint32)).all(1)
            assert same.all(), "%s: %d of %d closest-hit records differ from the oracle's (first: ray %d)" % (what, int((~same).sum()), same.size, int(np.argmin(same)))
        if route == "packets": assert st["packet_rays"] + st["leftover_rays"] == n, what          # every ray is committed by the packets or left over, once
        else: assert st["packet_rays"] == 0 and st["leftover_rays"] == 0, what
    R = M["runs"]
    if name in TUBES:
        for label in ("extend", "extend_ranged", "shadow"):
            assert R[label][2]["split"] >= 1 and R[label][2]["tasks"][0] > 0, (name, label, R[label][2])          # default grid: every wave is dry after one chunk
        assert R["packets"][2]["leftover_rays"] >= 1, (name, R["packets"][2])
    else:
        assert R["packets"][2]["packet_rays"] >= 1, (name, R["packets"][2])


def test_a_sub_tree_is_split_again_in_a_task_round():
    """k_extend_tasks<0> is itself CAN_SPLIT: a sub-tree that outlives its wave's others by T8_TAIL_ITERS_TASKS iterations goes to the other queue with the ray's key"""
    stats = {name: _measure(name)["runs"]["extend"][2] for name in TUBES}
    print(stats)
    assert any(st["tasks"][1] > 0 for st in stats.values()), stats


def test_packets_at_step_cap_8_commit_some_rays_and_leave_some_over():
    stats = {name: _measure(name)["runs"]["packets step cap 8"][2] for name in TUBES + SMALL_WITH_VARIANTS}
    print(stats)
    assert any(st["packet_rays"] > 0 and st["leftover_rays"] > 0 for st in stats.values()), stats


@pytest.mark.parametrize("name", TUBES)
def test_a_task_queue_too_small_is_an_error_not_a_short_answer(name):
    """pt_render's rule (check_frame_end): the rays whose sub-trees found no room are neither traced nor resolved, so the overflow word must fail the call"""
    M = _measure(name)
    for route in ("extend", "shadow"):
        need = M["runs"][route][2]["tasks"][0]
        assert need >= 2 and route in M["errors"], (name, route, need)
        e = M["errors"][route]
        assert e.code == 3 and e.stats is not None and e.stats["overflow"] & 2, (name, route, e, e.stats)          # PT_ERROR_HIP; bit 1: a task queue ran out of room
        assert e.stats["tasks"][0] > need // 2          # (the count goes on past the capacity: what a caller sizes the queue from)


def test_the_refusals():
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    sc = hit_cases.case("quadz-origin")["sc"]
    good = np.array([[0.25, 0.5, -2, 0, 0, 0, 1, 1e15]] * 4, np.float32)
    g = pt.PathTracer(test_hooks=True); g.set_scene(sc); g.set_settings(scenes.default_settings())
    try:
        for route in ("extend", "extend_ranged", "shadow", "packets"):
            for bad in (-1e-3, -0.0, float("nan"), -float("inf")):          # tmin >= +0: before anything reaches the device
                rays = good.copy(); rays[2, 3] = bad
                with pytest.raises(pt.PtError) as e: g.trace_route(route, rays)
                assert e.value.code == 1 and e.value.stats is None          # PT_ERROR_INVALID_ARGUMENT, and no launch ran
        for route in ("extend", "packets"):          # a fixed-interval route takes no other interval
            for col, val in ((7, 1e30), (7, 3.0), (3, 0.5)):
                rays = good.copy(); rays[1, col] = val
                with pytest.raises(pt.PtError) as e: g.trace_route(route, rays)
                assert e.value.code == 1
        rays = good.copy(); rays[3, 3] = 0.5
        with pytest.raises(pt.PtError) as e: g.trace_route("shadow", rays)          # a shadow-queue entry has no lower bound
        assert e.value.code == 1
        h, _ = g.trace_route("extend_ranged", rays)          # (the ranged route takes it: t = 2 lies inside)
        assert (h[:, 0] == 2.0).all()
        for route in (4, -1, 99):
            with pytest.raises(pt.PtError) as e: g.trace_route(route, good)
            assert e.value.code == 1
        with pytest.raises(pt.PtError): g.trace_route("extend", good[:0])
        for route in CLOSEST_ROUTES:          # the context is still usable
            h, st = g.trace_route(route, good)
            assert (h.view(np.uint32)[:, 1] != hit_ref.MISS).all() and (h[:, 0] == 2.0).all() and st["overflow"] == 0
        v, _ = g.trace_route("shadow", good)
        assert (v == 0).all()
    finally:
        g.close()
    shipped = pt.PathTracer(); shipped.set_scene(sc)
    try:
        assert not hasattr(shipped.L, "pt_trace_route")
        with pytest.raises(RuntimeError, match="not part of the shipped library"): shipped.trace_route("extend", good)
    finally:
        shipped.close()

"""The traversal's hit test is watertight (run with -m gpu). DXR promises a watertight ray / triangle test (what Bridge::traceScatterRay / traceVisibilityRay inherit from the
API, Rtxpt/Shaders/PathTracerBridgeDonut.hlsli:993-1055): a ray cannot slip between two triangles that share an edge or a vertex. Since round 5 the hit definition here
(pt_scene.h intersect_tri_wt) is the Woop-Benthin-Wald test — vertices sheared into the ray's frame, unfused edge functions, zeros resolved by the products' exact
rounding errors — over stored (shared) vertices; rounds 1-4 used fp32 Moeller-Trumbore with per-triangle barycentric rejects and leaked 12.6 % of the rays aimed exactly at a
shared edge, 19 % at a vertex and 1.0e-6 of random rays (profiles/r04q_watertight.txt).

Measurement on a closed, shared-vertex icosphere (20 480 triangles under a rotated, non-uniformly scaled instance transform), rays from inside — every ray must hit, a miss is a leak:
  * 10^7 rays aimed AT shared edges (a point of the edge, formed in float64 from the world-space vertices, so the ray passes within an fp32 rounding of the edge) and AT vertices:
    the worst case, where both neighbours see an edge function of 0 +- rounding;
  * the same with the target moved off the edge by k fp32 spacings of the coordinate;
  * 10^8 rays aimed at uniformly random surface points: what an image sees.
The device and the oracle share the definition and must agree ray for ray (asserted). Every count must be ZERO (asserted); the numbers go to profiles/ (r05*_watertight.txt).
This is one icosphere near the origin, and device and oracle share one text: scenes far from the origin, far ray origins, t / u / v and the interval ends against an independent
float64 reference are in tests/test_hit_reference.py and tests/test_gpu_hit_reference.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu



def _rays(W, I, n, kind, rng, offset_ulps=0.0):
    o = rng.normal(size=(n, 3)); o *= (0.25 * rng.random(n) ** (1 / 3) / np.linalg.norm(o, axis=1))[:, None]
    o += W.mean(0)
    tri = I[rng.integers(0, I.shape[0], n)]
    a, b, c = W[tri[:, 0]], W[tri[:, 1]], W[tri[:, 2]]
    if kind == "edge":
        s = rng.random(n)[:, None]
        tgt = a + s * (b - a)
        if offset_ulps:      # into the triangle, perpendicular to the edge, by `offset_ulps` spacings of an fp32 number of the coordinates' magnitude (~2)
            e = b - a; inward = (c - a) - e * ((c - a) * e).sum(1, keepdims=True) / (e * e).sum(1, keepdims=True)
            tgt = tgt + inward / np.linalg.norm(inward, axis=1, keepdims=True) * (offset_ulps * 2.0 ** -22)
    elif kind == "vertex":
        tgt = a
    else:
        u = rng.random(n); v = rng.random(n); f = u + v > 1; u[f] = 1 - u[f]; v[f] = 1 - v[f]
        tgt = a + u[:, None] * (b - a) + v[:, None] * (c - a)
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), 1e15)], 1).astype(np.float32)


def _misses(g, rays): return g.trace_closest(rays)[0].view(np.uint32)[:, 1] == 0xFFFFFFFF


def test_leak_rate_through_shared_edges_and_vertices():
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    from oracle import ptref
    sc, W, I = scenes.closed_icosphere(5)
    assert I.shape[0] == 20480
    g = pt.PathTracer(); g.set_scene(sc); g.set_settings(scenes.default_settings())
    o = ptref.Oracle(); o.set_scene(sc); o.set_settings(scenes.default_settings())
    rng = np.random.default_rng(0x5EED0411)
    lines = []
    escapes = 0
    for kind, total in (("edge", 8_000_000), ("vertex", 2_000_000)):
        miss = 0
        for chunk in range(total // 2_000_000):
            rays = _rays(W, I, 2_000_000, kind, rng)
            hits, _ = g.trace_closest(rays); m = hits.view(np.uint32)[:, 1] == 0xFFFFFFFF
            if chunk == 0:      # the oracle decides the same way, ray for ray: the first 50 000 rays and 20 000 of the leaked ones
                sel = np.unique(np.concatenate([np.arange(50_000), np.nonzero(m)[0][:20_000]]))
                assert np.array_equal(o.trace_closest(rays[sel]).view(np.uint32), hits[sel].view(np.uint32)), kind
            miss += int(m.sum())
        lines.append("aimed at a shared %-6s: %8d of %d rays escape (%.3f)" % (kind, miss, total, miss / total)); escapes += miss
    for k in (0.5, 1, 2, 4, 8, 16, 64):
        m = int(_misses(g, _rays(W, I, 2_000_000, "edge", rng, offset_ulps=k)).sum())
        lines.append("aimed %5.1f fp32 spacings inside the edge: %8d of 2000000 rays escape (%.2e)" % (k, m, m / 2e6)); escapes += m
    miss = 0; total = 100_000_000
    for chunk in range(total // 4_000_000): miss += int(_misses(g, _rays(W, I, 4_000_000, "interior", rng)).sum())
    lines.append("aimed at random surface points: %d of %d rays escape (%.2e)" % (miss, total, miss / total))
    print("\n".join("watertightness: " + l for l in lines))
    g.close(); o.close()
    assert escapes == 0 and miss == 0, lines

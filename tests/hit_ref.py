"""A float64 restatement of the hit test, exhaustive over the triangles, in plain numpy: what the traversal (device: pt_traverse8.h's leaf block, t8_leaf_block, over the BVH8; oracle:
oracle/ptref/scene.h) is held to. No BVH, no box half, no text shared with pt_scene.h.

The definition. A ray is (o, tmin, d, tmax) in float32 AS THE QUERY RECEIVES IT, a triangle three world-space float32 vertices as the scene build bakes them (world_triangles
below restates the float32 instance transform); both are widened to float64 and everything after that is float64. The ray meets the triangle's plane at the exact distance t;
(u, v) are the barycentrics of vertices 1 and 2 at that point (DXR's), b0 = 1 - u - v. The pair is a hit when all three barycentrics are >= 0 and tmin < t < tmax.
The values come from one route (Moeller-Trumbore: edge vectors, cross products), the error bounds and the signs from another (the ray's own frame, below); float64 carries
both ~2^29 times finer than the float32 arithmetic under test, so neither route's own rounding is visible in what follows.

What a float32 implementation can be charged with. intersect_tri_wt (pt_scene.h) translates the vertices to the origin, shears them into the ray's frame — kz the axis of the
largest |d|, Sz = 1 / d[kz], Sx = d[kx] Sz, Sy = d[ky] Sz, Ax = fma(-Sx, A[kz], A[kx]) — and takes the signs of the three 2-D edge functions U = Cx By - Cy Bx, V, W.
With r = 2^-24 (one float32 rounding, relative):
  * A[k] = v[k] - o[k] rounds once: error <= r |A[k]|.
  * Sz rounds once, Sx = d[kx] * Sz once more: relative 2 r. The product Sx A[kz] inside the fma therefore carries r |Sx A[kz]| (from A[kz]) + 2 r |Sx A[kz]| (from Sx),
    A[kx] brings r |A[kx]|, the fma rounds its result once:
        eps(Ax) <= r (|A[kx]| + 3 |Sx A[kz]| + |Ax|)                  the float32 error of a sheared coordinate
    and eps = the largest such term over the three vertices and both coordinates of the pair.
  * an edge function is two products and a difference: its operands bring eps (|By| + |Cx| + |Cy| + |Bx|) <= 4 eps L, L = the largest |sheared coordinate| of the pair, its
    own three roundings at most r (|Cx By| + |Cy Bx| + |U|) <= 3 r L^2:
        dU = 4 eps L + 3 r L^2                                          first order in r
  * the sign of a computed edge function is the exact one whenever |U| >= dU. The classification asks for 2 dU (the "small multiple" m of the barycentrics: b_i = U_i / det,
    det = U + V + W, so |U_i| >= 2 dU reads b_i >= m with m = 2 dU / |det|):
        CLEAR HIT    all three exact edge functions have one sign and |U_i| >= 2 dU, and tmin + 2 Bt < t < tmax - 2 Bt
        CLEAR MISS   one edge function <= -2 dU and another >= +2 dU (some barycentric <= -m whatever the sign of det: the implementation sees mixed signs), or the signs
                     are clear and t is outside the interval by 2 Bt, or every vertex's distance along the ray lies outside the interval (a reported t is a convex
                     combination of them), or the exact ray is parallel to the plane and its origin's projection is clearly off the projected segment (first rule)
        BORDERLINE   everything else. A ray with a borderline triangle at or in front of its first clear hit is SKIPPED; the tests cap the share of skipped rays.
  * values, for a clear hit (computed det >= |det| - 3 dU >= |det| / 2): u = V / det with det = (U + V) + W rounded twice, the reciprocal and the product once each
        Buv = 2 (1 + 3 |b|) dU / |det| + 4 r |b|
    and t = sum U_i z_i / det with z_i = Sz * A_i[kz] (two roundings on top of A's: 3 r |z_i|), three fused accumulations, the reciprocal, the product: the barycentrics' error
    moves t by at most 3 dU max|z_i - t| / (|det| / 2), the roundings by at most 10 r max|z_i|
        Bt = 6 (dU / |det|) max|z_i - t| + 10 r max|z_i|
    i.e. a few float32 spacings of |v - o| along the dominant axis, plus the barycentric error times the triangle's depth range.
Both bounds are first order and hold for the oracle and the device alike (neither contracts a * b + c except where the text writes fma). The tests print the largest observed
error / bound; a value above 1 means a step is missing above, not that the bound wants widening.

Memory: pairs are evaluated in chunks of PAIRS_PER_CHUNK (ray, triangle) pairs, ~60 float64 temporaries each: 20 000 rays x 1 000 triangles stay below 1 GB.
"""
import numpy as np

R32 = 2.0 ** -24
PAIRS_PER_CHUNK = 1 << 19
MISS = 0xFFFFFFFF
CLEAR_MISS, BORDERLINE, CLEAR_HIT = 0, 1, 2


def world_triangles(sc, instances=None):
    """The world-space float32 vertices of every global primitive, [T, 3, 3] float64, in primitive order (instance, geometry of its mesh, triangle): the float32 instance
    transform ((m0 x + m1 y) + m2 z) + m3 with every operation rounded to float32, as the scene builds form it."""
    inst = sc["instances"] if instances is None else instances
    out = []
    P = np.asarray(sc["positions"], np.float32).reshape(-1, 3); I = np.asarray(sc["indices"], np.uint32)
    for i in range(len(inst)):
        M = np.asarray(inst["transform"][i], np.float32).reshape(3, 4)
        first, count = int(sc["meshes"]["firstGeometry"][inst["meshIndex"][i]]), int(sc["meshes"]["numGeometries"][inst["meshIndex"][i]])
        for g in sc["geometries"][first:first + count]:
            idx = I[int(g["indexOffset"]):int(g["indexOffset"]) + int(g["numIndices"])].astype(np.int64) + int(g["vertexOffset"])
            p = P[idx]
            w = np.stack([((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3] for r in range(3)], 1)
            assert w.dtype == np.float32
            out.append(w.reshape(-1, 3, 3))
    return np.concatenate(out).astype(np.float64) if out else np.zeros((0, 3, 3))


def _dot(a, b): return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def pairs(V, rays):
    """Elementwise over broadcastable V [..., 3, 3] float64 and rays [..., 8] (float32 values): dict of cls, t, u, v, Bt, Buv, tlo (the smallest t a hit of this pair
    could be reported at), E (the three exact edge functions U, V, W: E[k] belongs to the edge opposite vertex k), dU, zmin / zmax (the vertices' distances along the ray)."""
    rays = np.asarray(rays, np.float64)
    o, tmin, d, tmax = rays[..., 0:3], rays[..., 3], rays[..., 4:7], rays[..., 7]
    P0, P1, P2 = V[..., 0, :], V[..., 1, :], V[..., 2, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # ---- the values: Moeller-Trumbore
        e1, e2 = P1 - P0, P2 - P0
        pv = _cross(np.broadcast_to(d, np.broadcast_shapes(d.shape, e2.shape)), e2)
        det3 = _dot(e1, pv); tv = o - P0; qv = _cross(tv, np.broadcast_to(e1, tv.shape))
        u = _dot(tv, pv) / det3; v = _dot(d, qv) / det3; t = _dot(e2, qv) / det3
        # ---- the bounds and the signs: the ray's own frame (kz: the largest |d|, ties to the lower axis; kx, ky the next two in cyclic order)
        ad = np.abs(d)
        kz = np.where((ad[..., 2] > ad[..., 0]) & (ad[..., 2] > ad[..., 1]), 2, np.where(ad[..., 1] > ad[..., 0], 1, 0))
        kx, ky = (kz + 1) % 3, (kz + 2) % 3
        def pick(a, k): return np.take_along_axis(a, np.broadcast_to(k[..., None], a.shape[:-1] + (1,)), -1)[..., 0]
        dz = pick(d, kz); Sx, Sy = pick(d, kx) / dz, pick(d, ky) / dz
        xs, ys, zs, eps = [], [], [], 0.0
        for Pv in (P0, P1, P2):
            A = Pv - o
            A = np.broadcast_to(A, np.broadcast_shapes(A.shape, d.shape))
            kzb = np.broadcast_to(kz, A.shape[:-1])
            akx, aky, akz = pick(A, np.broadcast_to(kx, A.shape[:-1])), pick(A, np.broadcast_to(ky, A.shape[:-1])), pick(A, kzb)
            x, y = akx - Sx * akz, aky - Sy * akz
            eps = np.maximum(eps, np.maximum(np.abs(akx) + 3.0 * np.abs(Sx * akz) + np.abs(x), np.abs(aky) + 3.0 * np.abs(Sy * akz) + np.abs(y)))
            xs.append(x); ys.append(y); zs.append(akz / dz)
        eps = R32 * eps
        (Ax, Bx, Cx), (Ay, By, Cy), (Az, Bz, Cz) = xs, ys, zs
        U, Vv, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        L = np.maximum.reduce([np.abs(a) for a in xs + ys])
        dU = 4.0 * eps * L + 3.0 * R32 * L * L
        det = U + Vv + W
        lo, hi = np.minimum(np.minimum(U, Vv), W), np.maximum(np.maximum(U, Vv), W)
        mixed = (lo <= -2.0 * dU) & (hi >= 2.0 * dU)
        inside = ((lo >= 2.0 * dU) | (hi <= -2.0 * dU)) & (dU > 0)
        zmin, zmax = np.minimum(np.minimum(Az, Bz), Cz), np.maximum(np.maximum(Az, Bz), Cz)
        zabs = np.maximum(np.abs(zmin), np.abs(zmax))
        b0 = 1.0 - u - v
        rel = dU / np.abs(det)
        Bt = 6.0 * rel * np.maximum(np.abs(zmax - t), np.abs(zmin - t)) + 10.0 * R32 * zabs
        Buv_u = 2.0 * (1.0 + 3.0 * np.abs(u)) * rel + 4.0 * R32 * np.abs(u)
        Buv_v = 2.0 * (1.0 + 3.0 * np.abs(v)) * rel + 4.0 * R32 * np.abs(v)
        zslack = 4.0 * R32 * zabs
        range_out = (zmax + zslack < tmin) | (zmin - zslack > tmax)
        t_in = inside & (t > tmin + 2.0 * Bt) & (t < tmax - 2.0 * Bt)
        t_out = inside & ((t < tmin - 2.0 * Bt) | (t > tmax + 2.0 * Bt))
        tlo = np.where(inside, t - 2.0 * Bt, zmin - zslack)
    cls = np.where(mixed | range_out | t_out, CLEAR_MISS, np.where(t_in, CLEAR_HIT, BORDERLINE)).astype(np.int8)
    return dict(cls=cls, t=t, u=u, v=v, b0=b0, Bt=Bt, Bu=Buv_u, Bv=Buv_v, tlo=tlo, E=np.stack([U, Vv, W], -1), dU=dU, zmin=zmin, zmax=zmax + zslack)


class Reference:
    """hit_ref over one (scene, ray set): per ray — first: the smallest exact t among the clear hits (inf: none), first_prim, first_Bt; any_hit: some clear hit; all_miss:
    every triangle a clear miss; skip: a borderline triangle at or in front of the first clear hit."""

    def __init__(self, V, rays):
        self.V = np.asarray(V, np.float64); self.rays = np.ascontiguousarray(rays, np.float32)
        n, T = len(self.rays), len(self.V)
        self.first = np.full(n, np.inf); self.first_prim = np.full(n, MISS, np.uint32); self.first_Bt = np.zeros(n)
        self.all_miss = np.ones(n, bool); border_lo = np.full(n, np.inf)
        step = max(1, PAIRS_PER_CHUNK // max(T, 1))
        for a in range(0, n, step):
            if T == 0: break
            r = pairs(self.V[None, :, :, :], self.rays[a:a + step, None, :])
            hit = r["cls"] == CLEAR_HIT
            th = np.where(hit, r["t"], np.inf); j = th.argmin(1); rows = np.arange(len(j))
            self.first[a:a + step] = th[rows, j]; self.first_Bt[a:a + step] = np.where(hit[rows, j], r["Bt"][rows, j], 0.0)
            self.first_prim[a:a + step] = np.where(hit[rows, j], j, MISS)
            self.all_miss[a:a + step] = (r["cls"] == CLEAR_MISS).all(1)
            border_lo[a:a + step] = np.where(r["cls"] == BORDERLINE, r["tlo"], np.inf).min(1)
        self.any_hit = np.isfinite(self.first)
        self.skip = (border_lo <= self.first) & (border_lo < np.inf)          # (no clear hit: any borderline triangle skips the ray)
        assert not (self.any_hit & self.all_miss).any()

    def skipped_share(self): return float(self.skip.mean()) if len(self.skip) else 0.0

    def of_prims(self, prims):
        """The pair (ray i, triangle prims[i]) for every ray with a valid prim: dict of pairs() rows (rows of invalid prims hold triangle 0)."""
        p = np.where(prims < len(self.V), prims, 0).astype(np.int64)
        return pairs(self.V[p], self.rays)


def check_closest(ref, hits, what=""):
    """The per-ray assertions of a closest-hit answer `hits` [n, 4] (t, prim bits, u, v) against a Reference; returns the figures (worst error / bound, counts)."""
    hits = np.ascontiguousarray(hits, np.float32)
    prim = hits.view(np.uint32)[:, 1].copy(); miss = prim == MISS; ok = ~ref.skip
    t, u, v = (hits[:, k].astype(np.float64) for k in (0, 2, 3))
    leaks = ok & ref.any_hit & miss
    false_hits = ok & ref.all_miss & ~miss
    assert (prim[~miss] < len(ref.V)).all(), "%s: a reported primitive id is out of range" % what
    rp = ref.of_prims(prim); rep = ok & ~miss
    beyond = rep & ref.any_hit & (t > ref.first + ref.first_Bt)
    wrong_prim = rep & ((rp["cls"] == CLEAR_MISS) | (np.abs(t - rp["t"]) > rp["Bt"]))
    val = rep & (rp["cls"] == CLEAR_HIT)
    with np.errstate(divide="ignore", invalid="ignore"):
        et, eu, ev = (np.where(val, a, 0.0) for a in (np.abs(t - rp["t"]) / rp["Bt"], np.abs(u - rp["u"]) / rp["Bu"], np.abs(v - rp["v"]) / rp["Bv"]))
    fig = dict(rays=len(prim), skipped=int(ref.skip.sum()), leaks=int(leaks.sum()), false_hits=int(false_hits.sum()), beyond_first=int(beyond.sum()), wrong_prim=int(wrong_prim.sum()),
               checked_values=int(val.sum()), worst_t=float(et.max(initial=0.0)), worst_u=float(eu.max(initial=0.0)), worst_v=float(ev.max(initial=0.0)))
    print("hit_ref closest %-44s %s" % (what, " ".join("%s=%s" % (k, ("%.3f" % x) if isinstance(x, float) else x) for k, x in fig.items())))
    assert fig["leaks"] == 0, "%s: %d of %d rays with a clear hit report a miss (first: ray %d)" % (what, fig["leaks"], len(prim), int(np.argmax(leaks)))
    assert fig["false_hits"] == 0, "%s: %d rays that clearly miss every triangle report a hit (first: ray %d)" % (what, fig["false_hits"], int(np.argmax(false_hits)))
    assert fig["beyond_first"] == 0, "%s: %d reported hits lie beyond the first clear hit (first: ray %d)" % (what, fig["beyond_first"], int(np.argmax(beyond)))
    assert fig["wrong_prim"] == 0, "%s: %d reported primitives are a clear miss or not at the reported t (first: ray %d)" % (what, fig["wrong_prim"], int(np.argmax(wrong_prim)))
    assert max(fig["worst_t"], fig["worst_u"], fig["worst_v"]) <= 1.0, "%s: t / u / v error over bound %.3f / %.3f / %.3f" % (what, fig["worst_t"], fig["worst_u"], fig["worst_v"])
    return fig


def check_visibility(ref, vis, what=""):
    """trace_visibility (1 = visible): 0 where a clear hit lies in the interval, 1 where every triangle is a clear miss."""
    vis = np.asarray(vis); ok = ~ref.skip
    assert np.isin(vis, (0, 1)).all()
    leaks = ok & ref.any_hit & (vis != 0); false_hits = ok & ref.all_miss & (vis != 1)
    print("hit_ref visibility %-41s rays=%d skipped=%d leaks=%d false_hits=%d" % (what, len(vis), int(ref.skip.sum()), int(leaks.sum()), int(false_hits.sum())))
    assert not leaks.any(), "%s: %d occluded rays report visible (first: ray %d)" % (what, int(leaks.sum()), int(np.argmax(leaks)))
    assert not false_hits.any(), "%s: %d rays that clearly miss every triangle report occluded (first: ray %d)" % (what, int(false_hits.sum()), int(np.argmax(false_hits)))
    return dict(leaks=int(leaks.sum()), false_hits=int(false_hits.sum()))


def check_shared_edges(V, rays, T1, k1, T2, k2, hits, what=""):
    """Rays aimed AT an edge shared by triangles T1[i] and T2[i] (k1 / k2: the vertex of each that is not on the edge). Each triangle alone is borderline there; the pair is
    not: when the four OUTER edge functions are clear (>= 2 dU) and of one sign, the exact ray crosses the interior of the union of the two triangles, and a watertight test
    reports a hit (DXR's promise; intersect_tri_wt keeps it because its unfused edge function negates exactly when the edge is walked the other way, so one of the two sees
    no sign mix) at a t within the two triangles' depth range. Returns the figures; asserts that at least 98 % of the rays qualify and that none of those escapes."""
    hits = np.ascontiguousarray(hits, np.float32); miss = hits.view(np.uint32)[:, 1] == MISS
    r1, r2 = pairs(V[T1], rays), pairs(V[T2], rays)
    def outer(r, k):
        keep = np.arange(3)[None, :] != k[:, None]
        E = r["E"][keep].reshape(-1, 2)
        return (np.abs(E) >= 2.0 * r["dU"][:, None]).all(1) & (np.sign(E[:, 0]) == np.sign(E[:, 1])), np.sign(E[:, 0])
    c1, s1 = outer(r1, k1); c2, s2 = outer(r2, k2)
    tmin, tmax = rays[:, 3].astype(np.float64), rays[:, 7].astype(np.float64)
    must = c1 & c2 & (s1 == s2) & (np.minimum(r1["zmin"], r2["zmin"]) > tmin) & (np.maximum(r1["zmax"], r2["zmax"]) < tmax)
    escapes = must & miss
    late = must & ~miss & (hits[:, 0] > np.maximum(r1["zmax"], r2["zmax"]))
    print("hit_ref shared edges %-39s rays=%d qualify=%d escapes=%d beyond=%d" % (what, len(rays), int(must.sum()), int(escapes.sum()), int(late.sum())))
    assert must.mean() >= 0.98, "%s: only %.1f %% of the edge rays cross the union clearly" % (what, 100 * must.mean())
    assert not escapes.any(), "%s: %d of %d rays through a shared edge escape (first: ray %d)" % (what, int(escapes.sum()), int(must.sum()), int(np.argmax(escapes)))
    assert not late.any(), "%s: %d rays through a shared edge report a hit behind both triangles" % (what, int(late.sum()))
    return dict(qualify=int(must.sum()), escapes=int(escapes.sum()))

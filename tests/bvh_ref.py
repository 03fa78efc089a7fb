"""The checker of the device-built BVH8 (tests/test_gpu_bvh_structure.py on the device, tests/test_bvh_reference.py on a small numpy-packed tree with one mutation at a time).

What it is given: the read-back of PathTracer.get_bvh8() — the 128-byte wide nodes, the 48-byte leaf-order triangle records with their stored pads, the six scene-bound floats
and the level table — and the scene's world-space triangles V [T, 3, 3] (tests/hit_ref.py world_triangles: the float32 vertices as float64). The reference is the geometry
itself: min / max of float32 values are exact, the decode is evaluated exactly, nothing of PLOC, the re-insertion or the collapse is restated and nothing depends on how a
build numbered its nodes. Every node, every child slot and every triangle is checked; a level of the tree is one numpy expression.

Clauses (the name in brackets is what a failure is reported under):
  [root] [ref] [leaf] [referenced] [partition] [permutation] [vertices] [childcount] [empty] [scales] [levels]     the structure, DESIGN.md section 4's layout
  [conservative]  per child slot and axis: decoded_lo <= fl32(tmin - pad) and decoded_hi >= fl32(tmax + pad) for every triangle below, with the record's own stored pad and
                  the float32 subtraction of pt_scene.h tri_box_accepts — exactly the nesting the hit definition needs. decoded = fmaf((float)q, s, o) rounded ONCE (decode32)
  [pads]          pad >= 4 * 2^-23 * max|coordinate| of the triangle's box (exact: a power-of-two multiple), and pad within PAD_REL of the float64 tri_pad with
                  scenePad = 2e-6 * |scene diagonal| from the read-back bounds
  [bounds]        the read-back scene bounds are the exact min / max of all vertices
  [tight]         per child slot and axis the decoded box lies within U -/+ (pad64(U) * (1 + PAD_REL) + K_STEPS * s + 1.5 u)   (U: the exact un-padded union below the child)
  [scale-min]     two halvings of an axis scale could not reach the node's maximum: the scale is the smallest power of two for which code 255 reaches it, or one doubling more
  [origin]        the node origin is the minimum of its children's padded boxes

PAD_REL = 1e-5. The project's float32 tri_pad has about eight roundings on its longest chain (scene extent, square, two sums, square root, times 2e-6f, the final sum, plus
the float32 constants), each at most 2^-24 = 6e-8 relative: 5e-7, twenty times below the constant.

K_STEPS = 2, derived from bvh8_child_codes (pt_build.hip), not measured. With x = (lo - o) / s the exact quotient, the start is floorf(fl32(fl32(lo - o) / s)): the subtraction
is off by 2^-24 relative, x <= 256, so the start is off from floor(x) by at most one either way, i.e. start >= x - 2. If the search loop does not move, the exact o + start * s
is >= lo - 2 s. If it moves it stops at the first q with decode(q) <= lo, and decode(q + 1) > lo puts the exact o + q s above lo - s - u/2. The hi side mirrors it. So the code is
at most 2 steps outside the child's float32 padded box.
What K_STEPS cannot hold is that decoded values, and the padded box itself, are float32: fl32(U_lo - pad) is up to u/2 below U_lo - pad and the decode rounds by up to u, where
u is the float32 spacing at the node's largest |coordinate| on that axis. Hence the term 1.5 u. In steps it is 1.5 * 2^-23 * |coordinate| / s <= 5e-5 * |coordinate| / extent
of the node: nothing near the origin, and the whole of the slack where one code step is below a float32 spacing of the origin (offsets of 1e5). It comes from the number
format, not from a run.
"""
import math

import numpy as np

MAX_LEAF = 2                  # PT_BVH_MAX_LEAF (pt_scene.h)
MAX_WIDE_LEVELS = 64          # BVH_MAX_WIDE_LEVELS (pt_build.h)
EMPTY = 0xFFFFFFFF
LEAF_BIT = 0x80000000
K_STEPS = 2                   # derived above
PAD_REL = 1e-5                # about eight float32 roundings of 6e-8 each, see above


def decode32(q, s, o):
    """fmaf((float)q, s, o): q * s + o rounded once to float32, elementwise. q * s must be exact in float64 (q an integer below 2^29, s a float32). The sum is formed with an
    error-free two-sum; float32(float64 sum) is already the single rounding unless the float64 sum sits exactly half way between two float32 values while the exact sum does
    not — then the residual decides."""
    a = np.asarray(q, np.float64) * np.asarray(s, np.float64); b = np.asarray(o, np.float64)
    a, b = np.broadcast_arrays(a, b)
    with np.errstate(over="ignore", invalid="ignore"):
        t = a + b; bb = t - a; err = (a - (t - bb)) + (b - bb)          # Knuth: t + err == a + b exactly
        r = t.astype(np.float32)
        lo = np.where(r.astype(np.float64) <= t, r, np.nextafter(r, np.float32(-np.inf))); hi = np.nextafter(lo, np.float32(np.inf))
        half = (t - lo.astype(np.float64) == hi.astype(np.float64) - t) & (err != 0) & np.isfinite(hi)
    return np.where(half, np.where(err > 0, hi, lo), r).astype(np.float32)


def spacing32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def scene_pad64(bounds):
    b = np.asarray(bounds, np.float64)
    return 2e-6 * float(np.sqrt(((b[3:] - b[:3]) ** 2).sum()))


def tri_pad64(mn, mx, scene_pad):
    """pt_scene.h tri_pad in float64, over boxes [..., 3]"""
    m = np.maximum(np.abs(mn), np.abs(mx)).max(-1)
    return np.maximum(2e-5 * (mx - mn).max(-1) + scene_pad, 4.0 * 2.0 ** -23 * m)


def _area(lo, hi):
    e = hi - lo
    return np.where(e[..., 0] < 0, 0.0, e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0])


def parse(rb):
    """the fields of a read-back: org [N, 3], scale [N, 3] (the floats the traversal reads), e [N, 3], cnt [N], ref [N, 8], qlo / qhi [N, 8, 3], q0 / q1 [N, 8]; verts [T, 3, 3]
    float32 (vertex, axis), prim [T], pad [T] float32"""
    nd = np.ascontiguousarray(rb["nodes"], np.uint32).reshape(-1, 32); tr = np.ascontiguousarray(rb["tris"], np.uint32).reshape(-1, 12)
    exps = nd[:, 3]; q0 = nd[:, 5:28:3]; q1 = nd[:, 6:28:3]
    f = tr.view(np.float32)
    return dict(org=nd[:, 0:3].copy().view(np.float32), scale=nd[:, 28:31].copy().view(np.float32), e=np.stack([exps & 255, (exps >> 8) & 255, (exps >> 16) & 255], 1),
                cnt=exps >> 24, ref=nd[:, 4:28:3].copy(), q0=q0, q1=q1, qlo=np.stack([q0 & 255, (q0 >> 8) & 255, (q0 >> 16) & 255], -1).astype(np.float64),
                qhi=np.stack([q0 >> 24, q1 & 255, (q1 >> 8) & 255], -1).astype(np.float64), tail=nd[:, 28:32],
                verts=np.stack([f[:, 0:3], f[:, 4:7], f[:, 8:11]], -1), prim=tr[:, 3].copy(), pad=f[:, 11].copy())


class Report:
    def __init__(self): self.errors = []; self.stats = {}
    def add(self, clause, bad, what):
        """bad: a boolean array (or bool); one entry per clause with the count and the first offender"""
        bad = np.asarray(bad)
        if bad.any(): self.errors.append((clause, "%s: %d, first at %s" % (what, int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]) if bad.ndim else "")))
    @property
    def ok(self): return not self.errors
    def clauses(self): return {c for c, _ in self.errors}
    def __str__(self): return "; ".join("[%s] %s" % e for e in self.errors) if self.errors else "ok"
    def require(self, what=""):
        assert self.ok, "%s: %s" % (what, self)
        return self


def check(rb, V, k_steps=K_STEPS, max_leaf=MAX_LEAF):
    """the whole checker; V [T, 3, 3]: the world-space float32 vertices of every primitive, in primitive order. Returns a Report: errors by clause, and stats (nodes, tris,
    levels, margin_steps: the smallest conservative margin, slack_steps: the largest distance of a decoded face beyond U -/+ (pad64 (1 + PAD_REL) + 1.5 u), both in code steps,
    cost, mean_children, canonical)."""
    R = Report(); p = parse(rb)
    N, T = p["ref"].shape[0], p["prim"].shape[0]
    V = np.asarray(V, np.float64).reshape(-1, 3, 3)
    levels = int(rb["levels"]); start = np.asarray(rb["level_start"], np.int64)
    R.stats.update(nodes=N, tris=T, levels=levels)
    if T == 0 or V.shape[0] == 0:
        R.add("root", N != 0 or T != V.shape[0], "an empty scene has no nodes and no triangles")
        return R
    R.add("root", N < 1, "no root")
    if N < 1: return R
    ref, cnt = p["ref"], p["cnt"]
    filled = ref != EMPTY; leaf = filled & ((ref & LEAF_BIT) != 0); inner = filled & ~leaf
    first = ((ref & 0x7FFFFFFF) >> 3).astype(np.int64); count = (ref & 7).astype(np.int64) + 1
    # ---- structure
    R.add("ref", inner & (ref >= N), "inner references beyond numNodes8")
    R.add("leaf", leaf & ((count > max_leaf) | (first + count > T)), "leaf references with more than %d triangles or beyond numTris" % max_leaf)
    okInner = inner & (ref < N)
    times = np.bincount(ref[okInner].astype(np.int64), minlength=N)
    R.add("root", times[0] != 0, "the root is referenced")
    R.add("referenced", np.concatenate([[False], times[1:] != 1]), "wide nodes not referenced exactly once")
    okLeaf = leaf & (first + count <= T)
    cover = np.zeros(T + 1, np.int64); np.add.at(cover, first[okLeaf], 1); np.add.at(cover, (first + count)[okLeaf], -1)
    R.add("partition", np.cumsum(cover)[:T] != 1, "triangles not in exactly one leaf")
    R.add("permutation", (T != V.shape[0]) or not np.array_equal(np.sort(p["prim"]), np.arange(V.shape[0], dtype=np.uint32)), "prim over the leaf order is not a permutation of the scene's primitives")
    if T == V.shape[0] and p["prim"].max() < V.shape[0]:
        R.add("vertices", (p["verts"].view(np.uint32) != V[p["prim"]].astype(np.float32).view(np.uint32)).any((1, 2)), "records whose vertices are not the float32 world-space vertices of their primitive")
    R.add("childcount", cnt != filled.sum(1), "exps >> 24 is not the number of non-empty slots")
    R.add("empty", ~filled & ((p["q0"] != 0x00FFFFFF) | (p["q1"] != 0)), "empty slots without the inverted box")
    R.add("scales", (p["tail"][:, :3] != (p["e"].astype(np.uint32) << 23)).any(1), "_pad[0..2] are not the floats 2^(e - 127) of exps")
    R.add("levels", levels > MAX_WIDE_LEVELS, "collapseLevels above BVH_MAX_WIDE_LEVELS")
    tiled = levels >= 1 and len(start) == levels + 1 and start[0] == 0 and start[-1] == N and (np.diff(start) > 0).all()
    R.add("levels", not tiled, "the levels do not tile [0, numNodes8)")
    if tiled:
        level = np.searchsorted(start, np.arange(N), side="right") - 1
        R.add("levels", okInner & (level[np.where(okInner, ref, 0)] <= level[:, None]), "inner children that do not lie in a deeper level")
    if not R.ok: return R          # the bottom-up pass below walks the structure just checked
    # ---- bottom-up: per child slot the exact union U, the union P of the triangles' own padded boxes, the primitives below
    vt = p["verts"]; tmin32, tmax32 = vt.min(1), vt.max(1); pad32 = p["pad"][:, None]
    tmin, tmax = tmin32.astype(np.float64), tmax32.astype(np.float64)
    plo, phi = (tmin32 - pad32).astype(np.float64), (tmax32 + pad32).astype(np.float64)          # float32 arithmetic: tri_box_accepts
    key = np.random.default_rng(0xB0C5).integers(1, 2 ** 63, V.shape[0], dtype=np.uint64)[p["prim"]]
    inf = np.inf
    sUlo = np.full((N, 8, 3), inf); sUhi = np.full((N, 8, 3), -inf); sPlo = np.full((N, 8, 3), inf); sPhi = np.full((N, 8, 3), -inf)
    sKey = np.zeros((N, 8), np.uint64); sCnt = np.zeros((N, 8), np.int64)
    for j in range(max_leaf):
        m = leaf & (count > j); t = (first + j)[m]
        sUlo[m] = np.minimum(sUlo[m], tmin[t]); sUhi[m] = np.maximum(sUhi[m], tmax[t]); sPlo[m] = np.minimum(sPlo[m], plo[t]); sPhi[m] = np.maximum(sPhi[m], phi[t])
        sKey[m] += key[t]; sCnt[m] += 1
    nUlo = np.empty((N, 3)); nUhi = np.empty((N, 3)); nPlo = np.empty((N, 3)); nPhi = np.empty((N, 3)); nKey = np.zeros(N, np.uint64); nCnt = np.zeros(N, np.int64)
    for l in range(levels - 1, -1, -1):
        a, b = int(start[l]), int(start[l + 1]); m = inner[a:b]; c = ref[a:b][m].astype(np.int64)
        for S, Nn in ((sUlo, nUlo), (sUhi, nUhi), (sPlo, nPlo), (sPhi, nPhi), (sKey, nKey), (sCnt, nCnt)):
            v = S[a:b]; v[m] = Nn[c]
        nUlo[a:b] = sUlo[a:b].min(1); nUhi[a:b] = sUhi[a:b].max(1); nPlo[a:b] = sPlo[a:b].min(1); nPhi[a:b] = sPhi[a:b].max(1)
        nKey[a:b] = sKey[a:b].sum(1, dtype=np.uint64); nCnt[a:b] = sCnt[a:b].sum(1)
    # ---- conservative, with the traversal's decode
    s = p["scale"].astype(np.float64)[:, None, :]; o = p["org"][:, None, :]
    dlo = decode32(p["qlo"], p["scale"][:, None, :], o).astype(np.float64); dhi = decode32(p["qhi"], p["scale"][:, None, :], o).astype(np.float64)
    F = filled[:, :, None]
    R.add("conservative", F & (dlo > sPlo), "child faces (node, slot, axis) whose decoded lo lies above a triangle's padded box")
    R.add("conservative", F & (dhi < sPhi), "child faces (node, slot, axis) whose decoded hi lies below a triangle's padded box")
    with np.errstate(invalid="ignore"):
        R.stats["margin_steps"] = float(np.minimum(np.where(F, (sPlo - dlo) / s, inf), np.where(F, (dhi - sPhi) / s, inf)).min())
    # ---- the stored pads and the scene bounds
    bounds = np.asarray(rb["bounds"], np.float32)
    R.add("bounds", np.concatenate([bounds[:3] != V.reshape(-1, 3).min(0), bounds[3:] != V.reshape(-1, 3).max(0)]), "scene bounds that are not the exact min / max of all vertices")
    sp = scene_pad64(bounds)
    want = tri_pad64(tmin, tmax, sp); have = p["pad"].astype(np.float64)
    R.add("pads", have < 4.0 * 2.0 ** -23 * np.maximum(np.abs(tmin), np.abs(tmax)).max(1), "pads below 4 float32 spacings of the box's largest |coordinate|")
    R.add("pads", ~(np.abs(have - want) <= PAD_REL * want), "pads more than 1e-5 relative from the float64 tri_pad")
    # ---- tight
    with np.errstate(invalid="ignore"):
        padU = np.where(filled, tri_pad64(np.where(F, sUlo, 0.0), np.where(F, sUhi, 0.0), sp), 0.0)[:, :, None]
        top = decode32(255.0, p["scale"], p["org"]).astype(np.float64)
        u = spacing32(np.maximum(np.abs(p["org"].astype(np.float64)), np.abs(top)))[:, None, :]
        fixed = padU * (1.0 + PAD_REL) + 1.5 * u
        outLo = np.where(F, ((sUlo - fixed) - dlo) / s, -inf); outHi = np.where(F, (dhi - (sUhi + fixed)) / s, -inf)
    R.add("tight", outLo > k_steps, "child faces (node, slot, axis) whose decoded lo is more than %g steps below U - pad" % k_steps)
    R.add("tight", outHi > k_steps, "child faces (node, slot, axis) whose decoded hi is more than %g steps above U + pad" % k_steps)
    R.stats["slack_steps"] = float(max(outLo.max(), outHi.max()))
    with np.errstate(invalid="ignore"):
        nmxUp = np.where(F, sUhi + padU * (1.0 + PAD_REL), -inf).max(1) + 0.5 * u[:, 0, :]
        quarter = decode32(255.0, (p["scale"].astype(np.float64) * 0.25).astype(np.float32), p["org"]).astype(np.float64)
        R.add("scale-min", (p["e"] >= 3) & (quarter >= nmxUp), "axis scales (node, axis) a quarter of which still reaches the node's maximum")
        mnLo = np.where(F, sUlo - padU * (1.0 + PAD_REL), inf).min(1) - 0.5 * u[:, 0, :]; mnHi = np.where(F, sUlo - padU * (1.0 - PAD_REL), inf).min(1) + 0.5 * u[:, 0, :]
    og = p["org"].astype(np.float64)
    R.add("origin", (og < mnLo) | (og > mnHi), "node origins (node, axis) that are not the minimum of the children's padded boxes")
    # ---- the canonical form, the cost, the fill
    canon = np.stack([nKey, nCnt.astype(np.uint64), cnt.astype(np.uint64)], 1)
    R.stats["canonical"] = canon[np.lexsort((canon[:, 2], canon[:, 1], canon[:, 0]))]
    R.stats["cost"] = math.fsum(_area(nUlo, nUhi)) + math.fsum(_area(sUlo, sUhi)[leaf])          # every wide-node visit and every leaf visit costs its surface area (pt_build_wide.h)
    R.stats["root_area"] = float(_area(nUlo[0], nUhi[0]))
    R.stats["mean_children"] = float(cnt.mean())
    R.stats["below_root"] = int(nCnt[0])
    return R


def same_bytes(a, b):
    """bytes that differ between two read-backs of one topology: nodes, triangle records (pads included), bounds, level table"""
    if a["nodes"].shape != b["nodes"].shape or a["tris"].shape != b["tris"].shape or a["levels"] != b["levels"]: return -1
    return sum(int((np.ascontiguousarray(a[k]).view(np.uint8) != np.ascontiguousarray(b[k]).view(np.uint8)).sum()) for k in ("nodes", "tris", "bounds", "level_start"))

"""The zoo of the hit-test reference tests (tests/test_hit_reference.py on the oracle, tests/test_gpu_hit_reference.py on the device; tests/test_gpu_traversal_routes.py takes
some of it through the traversal launches of a frame): small scenes (<= ~1 000 triangles; the two tube cases: 4 096) and ray sets (<= 20 000 rays) at the places where a float32 hit test goes wrong — geometry whose flat axis sits at a large coordinate, the offset given in the vertices or in the
instance transform, very small and very large scenes, ray origins very near and very far, axis-parallel / grazing / tied directions, and an instance moved after the build.

A case is a dict: name, sc (scene dict), V (world-space float32 vertices as float64 [T, 3, 3], tests/hit_ref.py world_triangles), rays [n, 8] float32, and — for the refit
cases — moved (the instance array the scene is animated to before the query; V belongs to that pose). reference(name) holds the float64 reference of a case, computed once.

Rays. Four of five are aimed at a point of a triangle whose three barycentrics lie in [0.05, 0.95]; one of five at a point 0.75 - 1.5 scene diagonals from the scene's centre
(off the geometry; where a case aims at some triangles only, diagonals and centre of those; the ray may still cross it: the reference decides). The float32 ray is what counts: the reference never sees the float64 ray it was rounded from.
On top, for a quarter of the aimed rays, four interval variants around the first clear hit of the reference (t1, bound Bt): tmax = t1 -/+ 4 Bt and tmin = t1 -/+ 4 Bt —
the hit must go away (or give way to the next surface) on one side and stay on the other.
"""
import functools
import math

import numpy as np

import hit_ref
from rtxpt_amd import scenes

DIAGONALS_FAR = (100, 300, 1000, 3000, 10000)      # origin distances, in scene diagonals, at which the leak rate is measured and printed (none of them is free of leaks)
MAX_ORIGIN_DIAGONALS = 8                            # the contract (include/mi355pt.h pt_trace_closest): no leak up to here — derived in test_hit_reference.py


def _quad(axis):
    p = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)
    return np.roll(p, axis - 2, axis=1), np.array([0, 1, 2, 0, 2, 3], np.uint32)


def _box():
    p = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float64)
    i = [0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5]
    return p, np.array(i, np.uint32)


def _icosphere():
    p, i = scenes.icosphere_mesh(2)
    assert i.shape[0] == 320
    return p.astype(np.float64), i.reshape(-1)


def _fan(n=48):
    """n slivers, 100 : 1, around one apex: length 1, 0.01 wide at the rim, the rim waving out of the plane"""
    a = 0.01 * np.arange(n + 1)
    rim = np.stack([np.cos(a), np.sin(a), 0.05 * np.sin(7.0 * a)], 1)
    p = np.concatenate([np.zeros((1, 3)), rim])
    i = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 2 + np.arange(n)], 1)
    return p, i.reshape(-1).astype(np.uint32)


def _grid(n=20):
    """a unit square in the plane z = 0 as n x n cells of two triangles, shared vertices: 800 axis-aligned triangles whose extent is 1 / 28 of the scene diagonal — their
    pad is little more than the scene's floor of it"""
    g = np.linspace(0.0, 1.0, n + 1); X, Y = np.meshgrid(g, g, indexing="ij")
    p = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel(); b = a + n + 1
    return p, np.stack([a, b, b + 1, a, b + 1, a + 1], 1).reshape(-1).astype(np.uint32)


def _tiny_in_large():
    """one axis-aligned triangle of 1e-3 inside a scene of diagonal 1e3 (two more triangles span it)"""
    h = 500.0 / math.sqrt(3.0)
    t = np.array([[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]]) + np.array([3.0, -2.0, 1.5])
    far = [np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1.0]]) + s * np.array([h, h, h]) - (s > 0) * np.array([1.0, 0, 1.0]) for s in (-1.0, 1.0)]
    return np.concatenate([t] + far), np.arange(9, dtype=np.uint32)


def _tube(n=4096, length=64.0, half=0.5, jitter=0.02):
    """n small triangles scattered through a long thin box, [0, length] x [-half, half]^2: each vertex is its triangle's centre plus uniform(-jitter, jitter)^3. A ray
    down the tube's axis that hits nothing walks the whole tree: the rays of a traversal launch that outlive their wave's other rays and are cut into sub-tree tasks
    (tests/test_gpu_traversal_routes.py)"""
    rng = np.random.default_rng(0x70BE)
    c = np.stack([rng.uniform(0.0, length, n), rng.uniform(-half, half, n), rng.uniform(-half, half, n)], 1)
    p = c[:, None, :] + rng.uniform(-jitter, jitter, (n, 3, 3))
    return p.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32)


TUBE = dict(length=64.0, half=0.5)
GEOMETRY = {"quadx": lambda: _quad(0), "quady": lambda: _quad(1), "quadz": lambda: _quad(2), "box": _box, "ico": _icosphere, "fan": _fan, "grid": _grid, "tiny": _tiny_in_large, "tube": _tube}
ROTATED = {"ico": (0.731, (1.7, 0.9, 1.3)), "fan": (0.4, (1.0, 0.8, 1.1))}      # rot_y, non-uniform scale of the instance


def make_scene(geom, size=1.0, offset=(0, 0, 0), place="verts"):
    """place: the offset sits in the vertices ("verts") or in the instance transform ("xform")"""
    p, i = GEOMETRY[geom]()
    off = np.asarray(offset, np.float64)
    rot, scl = ROTATED.get(geom, (0.0, (1.0, 1.0, 1.0)))
    if geom in ROTATED: place = "xform"
    p = p * size + (off if place == "verts" else 0.0)
    b = scenes.SceneBuilder(); m = b.add_material(scenes.make_material())
    b.begin_mesh(); b.add_geometry(p.astype(np.float32), i, m); mesh = b.end_mesh()
    b.add_instance(mesh, scenes.trs(tuple(off) if place == "xform" else (0, 0, 0), rot_y=rot, scale=scl))
    return b.finish()


def _unit(v): return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _directions(kind, nrm, rng):
    n = len(nrm)
    if kind == "random": return _unit(rng.normal(size=(n, 3)))
    if kind == "axis":          # exactly axis-parallel, along the axis the aimed triangle faces most; the two other components are +0.0 or -0.0
        k = np.abs(nrm).argmax(1)
        d = np.copysign(0.0, rng.choice([-1.0, 1.0], (n, 3)))
        d[np.arange(n), k] = rng.choice([-1.0, 1.0], n)
        return d
    if kind == "grazing":       # 1e-3 rad above the triangle's plane
        tng = _unit(np.cross(nrm, rng.normal(size=(n, 3))))
        return math.cos(1e-3) * tng + math.sin(1e-3) * rng.choice([-1.0, 1.0], (n, 1)) * nrm
    if kind == "tie":           # two components of equal magnitude; for half of the rays they are the two largest (the choice of kz is a tie)
        d = _unit(rng.normal(size=(n, 3))); order = np.argsort(-np.abs(d), 1); rows = np.arange(n)
        a = order[:, 0]; b = np.where(rng.random(n) < 0.5, order[:, 1], order[:, 2])
        d[rows, b] = np.copysign(np.abs(d[rows, a]), d[rows, b])
        return d
    raise ValueError(kind)


def make_rays(V, dist, kind, n, rng, aim=None, variants=True):
    """[n + 4 * (n // 5), 8] float32 rays against the world triangles V; dist: the origins' distance from the aim point in scene diagonals; aim: the triangles aimed at"""
    lo, hi = V.reshape(-1, 3).min(0), V.reshape(-1, 3).max(0); diag = float(np.linalg.norm(hi - lo)); centre, off = 0.5 * (lo + hi), diag
    if aim is not None:         # the points off the geometry lie around the aimed triangles, at their scale
        lo, hi = V[np.asarray(aim)].reshape(-1, 3).min(0), V[np.asarray(aim)].reshape(-1, 3).max(0); centre, off = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    n_on = n - n // 5
    tri = rng.choice(np.arange(len(V)) if aim is None else np.asarray(aim), n_on)
    b = 0.05 + 0.85 * rng.dirichlet([1.0, 1.0, 1.0], n_on)
    tgt = (b[:, :, None] * V[tri]).sum(1)
    nrm = _unit(np.cross(V[tri, 1] - V[tri, 0], V[tri, 2] - V[tri, 0]))
    d = _directions(kind, nrm, rng)
    off_tgt = centre + _unit(rng.normal(size=(n - n_on, 3))) * rng.uniform(0.75, 1.5, (n - n_on, 1)) * off
    d = np.concatenate([d, _unit(rng.normal(size=(n - n_on, 3)))]); tgt = np.concatenate([tgt, off_tgt])
    o = tgt - d * (dist * diag)
    rays = np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), 1e30)], 1).astype(np.float32)
    return _with_variants(V, rays, dist * diag) if variants else rays


def _with_variants(V, rays, length):
    """the n rays, then four interval variants of the first n // 5 (module docstring); length: the t a ray without a clear hit gets its variants around"""
    m = len(rays) // 5
    base = hit_ref.Reference(V, rays[:m])
    t1 = np.where(base.any_hit, base.first, length); mg = 4.0 * np.where(base.any_hit, base.first_Bt, 1e-5 * length)
    out = [rays]
    for col, val in ((7, t1 - mg), (7, t1 + mg), (3, t1 - mg), (3, t1 + mg)):
        r = rays[:m].copy(); r[:, col] = np.maximum(val, 0.0).astype(np.float32); out.append(r)          # (tmin >= +0: DXR's rule, and pt_trace_closest's)
    return np.concatenate(out)


def make_tube_rays(n, rng, offset, V):
    """[n + 4 * (n // 5), 8]: n rays down the tube, from a point of the square on the plane x = -1 to a point of the square on the plane x = length + 1 (both uniform),
    and their interval variants"""
    L, h = TUBE["length"], TUBE["half"]
    a = np.concatenate([np.full((n, 1), -1.0), rng.uniform(-h, h, (n, 2))], 1) + np.asarray(offset, np.float64)
    b = np.concatenate([np.full((n, 1), L + 1.0), rng.uniform(-h, h, (n, 2))], 1) + np.asarray(offset, np.float64)
    rays = np.concatenate([a, np.zeros((n, 1)), _unit(b - a), np.full((n, 1), 1e30)], 1).astype(np.float32)
    return _with_variants(V, rays, L + 2.0)


def _specs():
    S = []
    def add(name, geom, n, size=1.0, offset=(0, 0, 0), place="verts", dist=2.0, kind="random", aim=None, refit=None, builders=False):
        S.append(dict(name=name, geom=geom, n=n, size=size, offset=offset, place=place, dist=dist, kind=kind, aim=aim, refit=refit, builders=builders))
    small, large = 8000, 3000
    for k, g in enumerate(("quadx", "quady", "quadz", "box")):
        e = np.eye(3)
        add(g + "-origin", g, small)
        add(g + "-1e3-own-axis", g, small, offset=tuple(1e3 * e[k % 3]), builders=True)          # the quad's flat axis at 1000 (box: x)
        add(g + "-1e3-other-axis", g, small, offset=tuple(1e3 * e[(k + 1) % 3]))
        add(g + "-1e3-all-verts", g, small, offset=(1e3, 1e3, 1e3), builders=True)
        add(g + "-1e3-all-xform", g, small, offset=(1e3, 1e3, 1e3), place="xform")
        add(g + "-1e5-size10-verts", g, small, size=10.0, offset=(1e5, 1e5, 1e5), builders=True)
        add(g + "-1e5-size10-xform", g, small, size=10.0, offset=(1e5, 1e5, 1e5), place="xform")
        for kind in ("axis", "grazing", "tie"):
            add(g + "-" + kind, g, small, kind=kind)
            add(g + "-1e3-all-" + kind, g, small, offset=(1e3, 1e3, 1e3), kind=kind)
        for dist in (0.01, 100.0):
            add(g + "-dist%g" % dist, g, small, dist=dist)
        add(g + "-1e3-all-dist100", g, small, offset=(1e3, 1e3, 1e3), dist=100.0)
        add(g + "-refit-to-1e3", g, small, refit=(1e3, 1e3, 1e3))
    for g in ("quadz", "box"):
        add(g + "-size1e-3", g, small, size=1e-3); add(g + "-size1e4", g, small, size=1e4)
    for g in ("ico", "fan"):
        add(g + "-origin", g, large)
        add(g + "-1e3-all", g, large, offset=(1e3, 1e3, 1e3), builders=True)
        add(g + "-refit-to-1e3", g, large, refit=(1e3, 1e3, 1e3))
        for kind in ("axis", "tie"): add(g + "-" + kind, g, large, kind=kind)
    add("ico-1e5-size10", "ico", large, size=10.0, offset=(1e5, 1e5, 1e5), builders=True)
    add("ico-grazing", "ico", large, kind="grazing")
    add("ico-size1e-3", "ico", large, size=1e-3); add("ico-size1e4", "ico", large, size=1e4)
    add("ico-dist0.01", "ico", large, dist=0.01); add("ico-dist100", "ico", large, dist=100.0)
    add("grid-origin", "grid", large); add("grid-1e3-all", "grid", large, offset=(1e3, 1e3, 1e3), builders=True); add("grid-axis", "grid", large, kind="axis")
    add("grid-dist8", "grid", large, dist=float(MAX_ORIGIN_DIAGONALS)); add("grid-refit-to-1e3", "grid", large, refit=(1e3, 1e3, 1e3))
    add("tiny-in-1e3-scene", "tiny", small, dist=1e-5, aim=(0,))          # origins 0.01 units = 10 triangle sizes away
    add("tiny-in-1e3-scene-axis", "tiny", small, dist=1e-5, aim=(0,), kind="axis")
    # the deep cases (appended: a case's seed is its index): thousands of triangles, and rays that walk all of them
    add("tube-4096", "tube", 2048, kind="tube"); add("tube-4096-1e3-all", "tube", 2048, offset=(1e3, 1e3, 1e3), kind="tube")
    return S


SPECS = {s["name"]: s for s in _specs()}
NAMES = list(SPECS)
BUILDER_NAMES = [n for n in NAMES if SPECS[n]["builders"]]


@functools.lru_cache(maxsize=None)
def case(name):
    s = SPECS[name]
    sc = make_scene(s["geom"], s["size"], (0, 0, 0) if s["refit"] else s["offset"], s["place"])
    moved = None
    if s["refit"]:
        moved = sc["instances"].copy()
        moved["transform"][0][[3, 7, 11]] += np.asarray(s["refit"], np.float32)
    V = hit_ref.world_triangles(sc, moved)
    rng = np.random.default_rng(0x417C0DE + NAMES.index(name))
    rays = make_tube_rays(s["n"], rng, s["offset"], V) if s["kind"] == "tube" else make_rays(V, s["dist"], s["kind"], s["n"], rng, aim=s["aim"])
    return dict(name=name, sc=sc, V=V, rays=rays, moved=moved)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return hit_ref.Reference(c["V"], c["rays"])


def far_origin_rays(name, diagonals, n=4000):
    """random rays at the aimed points of a case's scene from `diagonals` scene diagonals away (no interval variants)"""
    c = case(name)
    return make_rays(c["V"], float(diagonals), "random", n, np.random.default_rng(0xFA4 + int(diagonals)), variants=False)


def exact_end_rays():
    """Rays whose whole float32 arithmetic is exact (dyadic coordinates, axis-parallel directions, unit quads in the three axis planes at the origin): the reported t IS the
    exact t = 2, so the interval ends can be put ON it. Returns a list of (scene, rays [6, 8], expect-hit [6]) — per quad: open interval (hit), tmax = 2 (miss: t < tmax),
    tmax = the next float32 above 2 (hit), tmin = 2 (miss: t > tmin), tmin = the next float32 below 2 (hit), and the same open ray from the other side (hit)."""
    out = []
    up, dn = np.nextafter(np.float32(2), np.float32(3)), np.nextafter(np.float32(2), np.float32(1))
    for axis in range(3):
        sc = make_scene(("quadx", "quady", "quadz")[axis])
        o = np.roll(np.array([0.25, 0.5, -2.0]), axis - 2); d = np.roll(np.array([-0.0, 0.0, 1.0]), axis - 2)
        rows = []
        for tmin, tmax, oo, dd in ((0, 1e30, o, d), (0, 2.0, o, d), (0, up, o, d), (2.0, 1e30, o, d), (dn, 1e30, o, d), (0, 1e30, np.where(d != 0, -o, o), -d)):
            rows.append(np.concatenate([oo, [tmin], dd, [tmax]]))
        out.append((sc, np.array(rows, np.float32), np.array([1, 0, 1, 0, 1, 1], bool)))
    return out


@functools.lru_cache(maxsize=None)
def shared_edge_case(name, n=10000):
    """Rays from inside a closed mesh of the zoo aimed at points of its shared edges (formed in float64 from the world-space vertices, so the float32 ray passes within a
    rounding of the edge): dict of sc, V, rays, T1, k1, T2, k2 (hit_ref.check_shared_edges). The mesh is consistently wound: the two triangles walk the edge in opposite directions."""
    c = case(name); V = c["V"]; I = np.asarray(c["sc"]["indices"], np.int64).reshape(-1, 3)
    edges = {}
    for t, tri in enumerate(I):
        for k in range(3):
            a, b = int(tri[(k + 1) % 3]), int(tri[(k + 2) % 3])
            edges.setdefault((min(a, b), max(a, b)), []).append((t, k, a, b))
    both = [e for e in edges.values() if len(e) == 2]
    assert len(both) == len(edges) and all(e[0][2] == e[1][3] and e[0][3] == e[1][2] for e in both)
    rng = np.random.default_rng(0xED6E + NAMES.index(name))
    pick = rng.integers(0, len(both), n)
    T1, k1, T2, k2 = (np.array([both[i][j][f] for i in pick]) for j, f in ((0, 0), (0, 1), (1, 0), (1, 1)))
    rows = np.arange(n)
    a, b = V[T1, (k1 + 1) % 3], V[T1, (k1 + 2) % 3]
    tgt = a + rng.uniform(0.05, 0.95, (n, 1)) * (b - a)
    lo, hi = V.reshape(-1, 3).min(0), V.reshape(-1, 3).max(0)
    o = 0.5 * (lo + hi) + _unit(rng.normal(size=(n, 3))) * (0.15 * (hi - lo).min() * rng.random((n, 1)) ** (1 / 3))
    d = _unit(tgt - o)
    rays = np.concatenate([o, np.zeros((n, 1)), d, np.full((n, 1), 1e30)], 1).astype(np.float32)
    return dict(sc=c["sc"], V=V, rays=rays, T1=T1, k1=k1, T2=T2, k2=k2)

"""The zoo of the BVH8 structure tests (tests/test_gpu_bvh_structure.py; the checker: tests/bvh_ref.py): seeded triangle soups and the shapes of tests/hit_cases.py at the sizes
at which a builder can go wrong, not the workload's —

  1, 2, 3                 at or below one leaf; the one-node special case of k_emit
  4, 5, 8, 9, 16, 17      around one and two full wide nodes
  33, 34                  the first sizes a PLOC window of 16 to either side does not cover
  256, 257, 1000, 4097    block edges of the 256-thread kernels and of the scan
  20 000                  several blocks
  66 000                  past 2^16

and, on a subset of the sizes, the geometry variants of VARIANTS below. Sizes from 1e-3 to 1e4 and offsets to 1e5, the range of hit_cases.py.
A case is a dict: name, n, sc (scene dict), V (hit_ref.world_triangles: the float32 world-space vertices, [T, 3, 3] float64). A refit case (refit_case) also has the poses B and C:
instances / positions to animate to, the vertex ranges that moved, and their V."""
import functools

import numpy as np

import hit_cases
import hit_ref
from rtxpt_amd import scenes

SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 34, 256, 257, 1000, 4097, 20000, 66000)
BUILDER_SIZES = (1, 9, 33, 1000, 20000)


def _soup(kind, n, rng):
    """[n, 3, 3] float64 triangles"""
    c = rng.random((n, 1, 3)) * 10.0; d = rng.normal(size=(n, 3, 3))
    if kind == "uniform": return c + 0.1 * d
    if kind == "piled":          # boxes of many sizes piled on 27 centres: mode 3 of the host checks
        return rng.integers(0, 3, (n, 1, 3)).astype(np.float64) + 10.0 ** rng.uniform(-3, 0, (n, 1, 1)) * d
    if kind == "identical": return np.broadcast_to(np.array([[0.5, 0.25, 1.0], [1.5, 0.25, 1.0], [0.5, 1.25, 2.0]]), (n, 3, 3)).copy()
    if kind == "plane": t = c + 0.1 * d; t[:, :, 2] = 0.0; return t
    if kind == "line": t = c + 0.1 * d; t[:, :, 1:] = 0.0; return t          # every vertex on the x axis: zero extent on two axes, every triangle a segment
    if kind == "offset-x": return c + 0.1 * d + np.array([1e5, 0, 0])
    if kind == "offset-all": return c + 0.1 * d + 1e5
    if kind == "sizes": return c * 1e3 + 10.0 ** rng.uniform(-3, 4, (n, 1, 1)) * d          # triangle sizes from 1e-3 to 1e4 in one scene
    if kind == "degenerate":          # points and segments among real triangles
        t = c + 0.1 * d; k = np.arange(n) % 3
        t[k == 1, 1] = t[k == 1, 0]; t[k == 1, 2] = t[k == 1, 0]; t[k == 2, 2] = t[k == 2, 1]
        return t
    raise ValueError(kind)


VARIANTS = {"piled": (17, 1000, 20000), "identical": (3, 33, 257, 456, 1000), "plane": (9, 1000), "line": (9, 1000), "offset-x": (2, 34, 4097), "offset-all": (1, 17, 1000, 4097),
            "sizes": (9, 1000, 4097), "degenerate": (5, 257, 1000), "two-instances": (8, 1000)}
SHAPES = ("box-1e5-size10-verts", "box-1e5-size10-xform", "ico-1e5-size10", "grid-1e3-all", "quadz-size1e-3", "quadz-size1e4", "fan-origin", "tiny-in-1e3-scene")      # hit_cases.py
NAMES = ["uniform-%d" % n for n in SIZES] + ["%s-%d" % (k, n) for k, ns in VARIANTS.items() for n in ns] + ["shape-" + s for s in SHAPES]
BUILDER_NAMES = ["uniform-%d" % n for n in BUILDER_SIZES] + ["identical-33", "identical-1000"]


def _scene(tris, transforms=(None,)):
    b = scenes.SceneBuilder(); m = b.add_material(scenes.make_material())
    p = np.asarray(tris, np.float32).reshape(-1, 3)
    b.begin_mesh(); b.add_geometry(p, np.arange(len(p), dtype=np.uint32), m); mesh = b.end_mesh()
    for t in transforms: b.add_instance(mesh, t)
    return b.finish()


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("shape-"):
        c = hit_cases.case(name[6:]); assert c["moved"] is None
        return dict(name=name, n=len(c["V"]), sc=c["sc"], V=c["V"])
    kind, n = name.rsplit("-", 1); n = int(n)
    rng = np.random.default_rng(0xB7 + NAMES.index(name))
    if kind == "two-instances":
        sc = _scene(_soup("uniform", n // 2, rng), (scenes.trs((0, 0, 0)), scenes.trs((40.0, -3.0, 1e3), rot_y=0.731, scale=(1.7, 0.9, 1.3))))
    else: sc = _scene(_soup(kind, n, rng))
    V = hit_ref.world_triangles(sc)
    assert len(V) == n
    return dict(name=name, n=n, sc=sc, V=V)


@functools.lru_cache(maxsize=None)
def refit_case(n, how):
    """pose A: four instances of a quarter-size soup spread 30 apart, each vertex scaled up by 4 about its mesh's centre (how = "vertices" / "ranges") or each instance scaled by 4
    (how = "instances"). Pose B: everything pulled together and shrunk — instances at the origin at scale 1 / the vertices at a sixteenth of their spread — so that most boxes
    shrink a lot. Pose C: a second, different detour (the extents of A, mirrored offsets). how = "ranges": only the two middle quarters of the vertices move, through vertex_ranges."""
    rng = np.random.default_rng(0xF17 + n)
    k = 4 if n % 4 == 0 else 3; m = n // k; assert m * k == n
    base = rng.random((m, 1, 3)) * 10.0 + 0.1 * rng.normal(size=(m, 3, 3))
    def xf(spread, scale, sign=1.0): return [scenes.trs((sign * spread * i, 0.5 * spread * (i % 2), -spread * (i // 2)), rot_y=0.3 * i, scale=(scale, scale, scale)) for i in range(k)]
    sc = _scene(base * (1.0 if how == "instances" else 4.0), xf(30.0, 4.0 if how == "instances" else 1.0))
    P = np.asarray(sc["positions"], np.float32).reshape(-1, 3).copy()
    poses = {}
    for tag, spread, scale, sign in (("B", 0.0, 1.0, 1.0), ("C", 55.0, 2.5, -1.0)):
        inst, pos, ranges = None, None, None
        if how == "instances":
            inst = sc["instances"].copy()
            for i, t in enumerate(xf(spread, scale, sign)): inst["transform"][i] = t
        else:
            f = 1.0 / 16.0 if tag == "B" else 0.6
            pos = ((P.astype(np.float64) - 20.0) * f + 20.0 * (tag == "C")).astype(np.float32)
            if how == "ranges":
                a, b = len(P) // 4, 3 * (len(P) // 4); keep = P.copy(); keep[a:b] = pos[a:b]; pos = keep; ranges = [(a, (b - a) // 2), (a + (b - a) // 2, b - a - (b - a) // 2)]
        moved = dict(sc, positions=pos.reshape(np.asarray(sc["positions"]).shape)) if pos is not None else sc
        poses[tag] = dict(instances=inst, positions=pos, ranges=ranges, V=hit_ref.world_triangles(moved, inst))
    return dict(name="refit-%s-%d" % (how, n), sc=sc, V=hit_ref.world_triangles(sc), poses=poses, positions=P)

"""The BVH8 checker's own test (tests/bvh_ref.py; its use on the device-built tree: tests/test_gpu_bvh_structure.py). A small numpy packer builds a valid BVH8 over a soup
with a median split — not a restatement of bvh8_pack: the codes come from a plain float64 floor / ceil plus one step outwards, the scale is searched upwards from below — and
the checker passes it. The packer's known slack: floor is at most one step inside, one more step is added, so it stays within the checker's K_STEPS = 2 and nothing is
relaxed. Then one mutation at a time, each of which has to be reported under the clause meant for it. The decode helper is held to exact rational arithmetic."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_ref as B


def soup(n, seed=1, size=0.05, offset=(0, 0, 0)):
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3)) + np.asarray(offset, np.float64)
    return (c + size * rng.normal(size=(n, 3, 3))).astype(np.float32).astype(np.float64)


def pack(V, max_leaf=B.MAX_LEAF):
    """a valid BVH8 over V [T, 3, 3] in the read-back's layout: breadth first, every wide node splits its triangles at the median of the longest axis until it has 8 groups"""
    T = len(V); tmin, tmax = V.min(1), V.max(1); cen = 0.5 * (tmin + tmax)
    bounds = np.concatenate([tmin.min(0), tmax.max(0)]).astype(np.float32); sp = B.scene_pad64(bounds)
    def padded(ids):
        lo, hi = tmin[ids].min(0), tmax[ids].max(0); pad = np.float32(B.tri_pad64(lo, hi, sp))
        return lo.astype(np.float32) - pad, hi.astype(np.float32) + pad
    nodes, order, start = [], [], [0]; level = [np.arange(T)]
    while level:
        nxt = []
        for ids in level:
            groups = [ids]
            while len(groups) < 8 and max(len(g) for g in groups) > max_leaf:
                g = groups.pop(int(np.argmax([len(g) for g in groups])))
                g = g[np.argsort(cen[g][:, int(np.argmax(tmax[g].max(0) - tmin[g].min(0)))], kind="stable")]
                groups += [g[:len(g) // 2], g[len(g) // 2:]]
            box = [padded(g) for g in groups]
            o = np.min([b[0] for b in box], 0); mx = np.max([b[1] for b in box], 0)
            e = np.ones(3, np.int64)
            for a in range(3):
                while e[a] < 254 and B.decode32(255.0, np.float32(2.0 ** (int(e[a]) - 127)), o[a]) < mx[a]: e[a] += 1
            s = (2.0 ** (e - 127.0)).astype(np.float32)
            rec = np.zeros(32, np.uint32); rec[0:3] = o.view(np.uint32); rec[3] = e[0] | e[1] << 8 | e[2] << 16 | len(groups) << 24; rec[28:31] = s.view(np.uint32)
            rec[4:28:3] = B.EMPTY; rec[5:28:3] = 0x00FFFFFF
            for k, (g, (lo, hi)) in enumerate(zip(groups, box)):
                ql = np.clip(np.floor((lo.astype(np.float64) - o) / s) - 1, 0, 255).astype(np.uint32); qh = np.clip(np.ceil((hi.astype(np.float64) - o) / s) + 1, 0, 255).astype(np.uint32)
                rec[5 + 3 * k] = ql[0] | ql[1] << 8 | ql[2] << 16 | qh[0] << 24; rec[6 + 3 * k] = qh[1] | qh[2] << 8
                if len(g) <= max_leaf: rec[4 + 3 * k] = B.LEAF_BIT | len(order) << 3 | (len(g) - 1); order += list(g)
                else: rec[4 + 3 * k] = start[-1] + len(level) + len(nxt); nxt.append(g)
            nodes.append(rec)
        start.append(start[-1] + len(level)); level = nxt
    order = np.array(order); tr = np.zeros((T, 12), np.float32)
    for a in range(3): tr[:, 4 * a:4 * a + 3] = V[order][:, :, a]
    tr[:, 11] = B.tri_pad64(tmin[order], tmax[order], sp)
    tr = tr.view(np.uint32); tr[:, 3] = order
    return dict(nodes=np.array(nodes, np.uint32), tris=tr, bounds=bounds, levels=len(start) - 1, level_start=np.array(start, np.uint32))


V300 = soup(300)


@pytest.fixture(scope="module")
def tree():
    rb = pack(V300)
    B.check(rb, V300).require("the packed tree")
    return rb


def _copy(rb): return {k: (v.copy() if hasattr(v, "copy") else v) for k, v in rb.items()}


def _slots(rb, leaf=None, where=lambda n, k, ref: True):
    """(node, slot, ref) of the non-empty slots; leaf: None = all, True / False = leaf / inner references"""
    out = []
    for n in range(len(rb["nodes"])):
        for k in range(8):
            r = int(rb["nodes"][n, 4 + 3 * k])
            if r != B.EMPTY and (leaf is None or bool(r >> 31) == leaf) and where(n, k, r): out.append((n, k, r))
    return out


@pytest.mark.parametrize("n,offset,size", [(1, (0, 0, 0), 0.05), (2, (0, 0, 0), 0.05), (3, (0, 0, 0), 0.05), (17, (0, 0, 0), 0.05), (300, (1e5, 0, 0), 0.05), (300, (1e5, 1e5, 1e5), 10.0), (1000, (0, 0, 0), 1e-3)])
def test_the_checker_passes_a_valid_tree(n, offset, size):
    V = soup(n, 7, size, offset)
    r = B.check(pack(V), V).require("n=%d offset=%s" % (n, offset))
    assert r.stats["below_root"] == n and r.stats["margin_steps"] >= 0 and r.stats["slack_steps"] <= B.K_STEPS


def test_the_empty_tree_passes_and_a_tree_without_its_scene_does_not():
    empty = dict(nodes=np.zeros((0, 32), np.uint32), tris=np.zeros((0, 12), np.uint32), bounds=np.zeros(6, np.float32), levels=0, level_start=np.zeros(1, np.uint32))
    assert B.check(empty, np.zeros((0, 3, 3))).ok
    assert "root" in B.check(pack(V300), np.zeros((0, 3, 3))).clauses()


def test_mutation_a_triangle_missing_from_the_leaves(tree):
    rb = _copy(tree); n, k, r = _slots(rb, True, lambda n, k, r: (r & 7) == 1)[0]
    rb["nodes"][n, 4 + 3 * k] = r - 1
    assert "partition" in B.check(rb, V300).clauses()


def test_mutation_a_triangle_in_two_leaves(tree):
    rb = _copy(tree); n, k, r = _slots(rb, True, lambda n, k, r: (r & 7) == 0 and ((r & 0x7FFFFFFF) >> 3) + 2 <= 300)[0]
    rb["nodes"][n, 4 + 3 * k] = r + 1
    assert "partition" in B.check(rb, V300).clauses()


def test_mutation_a_leaf_of_three(tree):
    rb = _copy(tree); n, k, r = _slots(rb, True, lambda n, k, r: ((r & 0x7FFFFFFF) >> 3) + 3 <= 300)[0]
    rb["nodes"][n, 4 + 3 * k] = (r & ~7) | 2
    assert "leaf" in B.check(rb, V300).clauses()


def test_mutation_a_node_referenced_twice(tree):
    rb = _copy(tree); (n, k, r), (_, _, other) = _slots(rb, False)[-2:]
    rb["nodes"][n, 4 + 3 * k] = other
    assert "referenced" in B.check(rb, V300).clauses()


def test_mutation_a_child_in_a_shallower_level(tree):
    """two inner references of different levels trade places: every node is still referenced once"""
    rb = _copy(tree); start = rb["level_start"]
    (n1, k1, r1) = _slots(rb, False, lambda n, k, r: n == 0)[0]
    (n2, k2, r2) = _slots(rb, False, lambda n, k, r: n >= start[1] and n != r1)[0]
    rb["nodes"][n1, 4 + 3 * k1] = r2; rb["nodes"][n2, 4 + 3 * k2] = r1
    c = B.check(rb, V300).clauses()
    assert "levels" in c and "referenced" not in c


def test_mutation_child_count_off_by_one(tree):
    rb = _copy(tree); rb["nodes"][3, 3] += np.uint32(1 << 24)
    assert B.check(rb, V300).clauses() == {"childcount"}


def _move_until_it_pokes(tree, field, shift, step):
    """move one code by one step at a time; the tree before the last step still passes the conservative clause, the last step does not"""
    n, k, _ = _slots(tree, True)[5]
    rb = _copy(tree)
    for _ in range(8):
        rb["nodes"][n, field + 3 * k] = np.uint32(int(rb["nodes"][n, field + 3 * k]) + (step << shift))
        c = B.check(rb, V300).clauses()
        if c: return c
    return set()


def test_mutation_one_qlo_raised_until_a_triangle_pokes_out(tree):
    assert _move_until_it_pokes(tree, 5, 8, +1) == {"conservative"}


def test_mutation_one_qhi_lowered_until_a_triangle_pokes_out(tree):
    assert _move_until_it_pokes(tree, 6, 8, -1) == {"conservative"}


def test_mutation_an_exponent_one_too_small(tree):
    rb = _copy(tree); rb["nodes"][2, 3] -= np.uint32(1); rb["nodes"][2, 28] -= np.uint32(1 << 23)
    assert "conservative" in B.check(rb, V300).clauses()


def test_mutation_a_loose_box(tree):
    """a stale box: conservative, but six steps wider than the geometry below it"""
    rb = _copy(tree)
    n, k, _ = [s for s in _slots(rb) if ((int(rb["nodes"][s[0], 5 + 3 * s[1]]) >> 16) & 255) >= 6][0]
    rb["nodes"][n, 5 + 3 * k] -= np.uint32(6 << 16)
    assert B.check(rb, V300).clauses() == {"tight"}


def test_mutation_a_tree_stale_by_a_translation(tree):
    """the tree of a pose translated by a tenth of the scene against the geometry it is checked with"""
    c = B.check(tree, V300 + np.float64(np.float32(0.125))).clauses()
    assert c & {"vertices", "conservative", "tight", "bounds"}
    rb = pack(V300); rb["nodes"][:, 0] = (rb["nodes"][:, 0].view(np.float32) - np.float32(0.125)).view(np.uint32)          # every box moved, the records left alone
    assert {"tight", "origin"} <= B.check(rb, V300).clauses()


def test_mutation_a_scale_one_doubling_too_many(tree):
    """exps + 2 on one axis with the codes formed again on the wider grid: conservative and tight in steps, but not the smallest scale"""
    V = soup(40, 3); rb = pack(V); p = B.parse(rb)
    s4 = np.float32(4.0) * p["scale"][0, 0]
    rb["nodes"][0, 3] += np.uint32(2); rb["nodes"][0, 28] = s4.view(np.uint32)
    for k in range(int(p["cnt"][0])):
        ql, qh = np.floor(p["qlo"][0, k, 0] / 4), np.ceil(p["qhi"][0, k, 0] / 4)
        rb["nodes"][0, 5 + 3 * k] = (rb["nodes"][0, 5 + 3 * k] & np.uint32(0x00FFFF00)) | np.uint32(ql) | np.uint32(int(qh) << 24)
    assert "scale-min" in B.check(rb, V).clauses()


def test_mutation_pad_scales_that_disagree_with_exps(tree):
    rb = _copy(tree); rb["nodes"][1, 29] += np.uint32(1 << 23)
    assert "scales" in B.check(rb, V300).clauses()


def test_mutation_a_pad_halved(tree):
    rb = _copy(tree); f = rb["tris"].view(np.float32); f[17, 11] *= np.float32(0.5)
    assert B.check(rb, V300).clauses() == {"pads"}


def test_mutation_a_primitive_twice_and_a_vertex_off_by_a_bit(tree):
    rb = _copy(tree); rb["tris"][4, 3] = rb["tris"][5, 3]
    assert "permutation" in B.check(rb, V300).clauses()
    rb = _copy(tree); rb["tris"][4, 0] ^= np.uint32(1)
    assert "vertices" in B.check(rb, V300).clauses()


def test_mutation_an_empty_slot_with_a_box_and_levels_that_do_not_tile(tree):
    rb = _copy(tree); n = [n for n in range(len(rb["nodes"])) if rb["nodes"][n, 3] >> 24 < 8][0]
    rb["nodes"][n, 5 + 3 * 7] = 0
    assert B.check(rb, V300).clauses() == {"empty"}
    rb = _copy(tree); rb["level_start"][-1] -= 1
    assert "levels" in B.check(rb, V300).clauses()


def test_canonical_form_ignores_numbering_and_sees_topology():
    V = soup(200, 5); a = pack(V); b = _copy(a)
    i, j = int(a["level_start"][1]), int(a["level_start"][1]) + 1          # two nodes of level 1 trade numbers
    b["nodes"][[i, j]] = b["nodes"][[j, i]]
    for n, k, r in _slots(b, False, lambda n, k, r: r in (i, j)): b["nodes"][n, 4 + 3 * k] = i + j - r
    ra, rb_ = B.check(a, V).require(), B.check(b, V).require()
    assert not np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(ra.stats["canonical"], rb_.stats["canonical"]) and ra.stats["cost"] == rb_.stats["cost"]
    c = B.check(pack(V, max_leaf=1), V, max_leaf=1).require()
    assert not np.array_equal(ra.stats["canonical"], c.stats["canonical"])
    assert 1.0 <= ra.stats["mean_children"] <= 8.0 and ra.stats["cost"] > ra.stats["root_area"] > 0


# ---- the decode helper
def _round32(x):
    """the float32 nearest to the rational x, ties to even: by comparison of rationals"""
    c = np.float32(float(x)); cands = sorted({float(np.nextafter(c, np.float32(-np.inf))), float(c), float(np.nextafter(c, np.float32(np.inf)))})
    best = min(cands, key=lambda v: (abs(Fraction(v) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def test_decode_where_the_sum_is_exact():
    rng = np.random.default_rng(11)
    q = rng.integers(0, 256, 4000).astype(np.float64); e = rng.integers(-20, 6, 4000); s = (2.0 ** e).astype(np.float32)
    o = (rng.integers(-2 ** 12, 2 ** 12, 4000) * 2.0 ** e).astype(np.float32)          # o a small multiple of s: q * s + o has at most 21 bits, every float32 operation is exact
    want = np.float32(q).astype(np.float32) * s + o
    assert want.dtype == np.float32 and np.array_equal(B.decode32(q, s, o), want)


def test_decode_rounds_once_where_a_float64_sum_would_round_twice():
    """q * s = 2^j (2^23 - 2^-23) sits 2^-46 relative below half a float32 spacing of o: the float64 sum rounds to the half-way point, its cast to float32 ties to even, and for
    an odd o that is the wrong neighbour. Both signs of o."""
    rng = np.random.default_rng(12); wrong = 0
    for _ in range(300):
        ex = int(rng.integers(-30, 60)); mant = int(rng.integers(2 ** 23, 2 ** 24)) | 1
        o = np.float32(mant * 2.0 ** (ex - 23)) * np.float32(rng.choice([-1.0, 1.0]))
        q = float(2 ** 23 + 1); s = np.float32((1.0 - 2.0 ** -23) * 2.0 ** (ex - 23 - 1 - 23))          # q * s = half a spacing of o, less 2^-46 of it
        exact = Fraction(q) * Fraction(float(s)) + Fraction(float(o))
        want = _round32(exact)
        got = B.decode32(q, s, o)
        assert got == want, (o, s, got, want)
        wrong += np.float32(q * float(s) + float(o)) != want
    assert wrong > 100          # the cases are what they claim to be: the float64 route is wrong for about half of them


def test_decode_against_rationals_on_node_like_operands():
    rng = np.random.default_rng(13)
    for _ in range(2000):
        o = np.float32(rng.normal() * 10.0 ** rng.integers(-3, 6)); s = np.float32(2.0 ** int(rng.integers(-126, 20))); q = float(rng.integers(0, 256))
        assert B.decode32(q, s, o) == _round32(Fraction(q) * Fraction(float(s)) + Fraction(float(o)))

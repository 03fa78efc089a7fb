"""pt_gltf_animation_skinning + pt_gltf_animation_palette carry everything the pose needs: a numpy restatement of the per-vertex function of rtxpt_amd/csrc/pt_skin.h — float64
sums in the host's order, float32 where the host stores one — applied to the description and a frame's palette reproduces pt_gltf_animation_positions bit for bit and
pt_gltf_animation_normals word for word, for every case of tests/skin_cases.py at its key times and between them. No device."""
import os, sys
import numpy as np
import pytest

import rtxpt_amd as pt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skin_cases

HAS_NORMAL, HAS_TANGENT = 2, 4      # PT_GEOM_HAS_NORMAL / PT_GEOM_HAS_TANGENT (include/mi355pt.h)


def pack_snorm8(v):
    c = np.clip(v.astype(np.float32), np.float32(-1), np.float32(1)); q = np.trunc(c * np.float32(127.0)).astype(np.int64) & 0xFF
    return sum(q[:, k] << (8 * k) for k in range(v.shape[1])).astype(np.uint32)


def length(q): return np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2])      # ((x x + y y) + z z), the host's order


def pose(desc, bind_positions, matrices, morph_weights):
    """(positions float32 [V, 3], normals uint32 [V] or None where untouched, tangents likewise) — vertices outside the ranges are returned as NaN / 0 with touched False"""
    V = len(desc.joints); P = np.full((V, 3), np.nan, np.float32); NW = np.zeros(V, np.uint32); TW = np.zeros(V, np.uint32); touchedN = np.zeros(V, bool); touchedT = np.zeros(V, bool); inside = np.zeros(V, bool)
    for r in desc.ranges:
        a, n = int(r["firstVertex"]), int(r["numVertices"]); sl = slice(a, a + n); inside[sl] = True
        hasN, hasT = bool(r["geometryFlags"] & HAS_NORMAL), bool(r["geometryFlags"] & HAS_TANGENT)
        bindN = desc.normals[sl]; bindT = desc.tangents[sl]; nF = bindN.copy(); tF = bindT.copy(); nw = pack_snorm8(nF); tw = pack_snorm8(tF)
        p = bind_positions[sl].astype(np.float64)
        if r["numTargets"]:
            k = int(r["numTargets"]); w = morph_weights[int(r["firstWeight"]):int(r["firstWeight"]) + k]; f = int(r["firstMorphDelta"])
            dP, dN, dT = (d[f:f + 3 * k * n].reshape(k, n, 3) for d in (desc.morph_position_deltas, desc.morph_normal_deltas, desc.morph_tangent_deltas))
            dn = np.zeros((n, 3)); dt = np.zeros((n, 3)); anyN = np.zeros(n, bool); anyT = np.zeros(n, bool)
            for i in range(k):
                p = p + w[i] * dP[i].astype(np.float64); dn = dn + w[i] * dN[i].astype(np.float64); dt = dt + w[i] * dT[i].astype(np.float64)
                anyN |= ((dN[i] != 0) & (w[i] != 0)).any(1); anyT |= ((dT[i] != 0) & (w[i] != 0)).any(1)
            p = p.astype(np.float32).astype(np.float64)                       # the morphed position is rounded to binary32 before the skin reads it
            for has, anyX, bind, d, xF, word, comps in ((hasN, anyN, bindN, dn, nF, nw, 3), (hasT, anyT, bindT, dt, tF, tw, 4)):
                q = bind[:, :3].astype(np.float64) + d; l = length(q); m = anyX & (l > 0) & has
                with np.errstate(all="ignore"): xF[m, :3] = (q / l[:, None]).astype(np.float32)[m]
                word[m] = pack_snorm8(xF[:, :comps])[m]
        out = p.astype(np.float32)
        if r["numMatrices"]:
            jm = matrices[int(r["firstMatrix"]):int(r["firstMatrix"]) + int(r["numMatrices"])]; wgt = desc.weights[sl]; jnt = desc.joints[sl].astype(np.int64)
            skinned = ((wgt[:, 0] + wgt[:, 1]) + wgt[:, 2]) + wgt[:, 3] > 0
            q = np.zeros((n, 3)); nrm = np.zeros((n, 3)); tan = np.zeros((n, 3)); n0 = nF.astype(np.float64); t0 = tF.astype(np.float64)
            for k in range(4):
                use = (wgt[:, k] != 0) & (jnt[:, k] < len(jm)); m = jm[np.where(use, jnt[:, k], 0)]; wk = wgt[:, k].astype(np.float64)      # m[:, 4 c + r]
                for rr in range(3):
                    q[:, rr] += np.where(use, wk * (m[:, rr] * p[:, 0] + m[:, 4 + rr] * p[:, 1] + m[:, 8 + rr] * p[:, 2] + m[:, 12 + rr]), 0.0)
                    tan[:, rr] += np.where(use, wk * (m[:, rr] * t0[:, 0] + m[:, 4 + rr] * t0[:, 1] + m[:, 8 + rr] * t0[:, 2]), 0.0)
                c00 = m[:, 5] * m[:, 10] - m[:, 9] * m[:, 6]; c01 = m[:, 9] * m[:, 2] - m[:, 1] * m[:, 10]; c02 = m[:, 1] * m[:, 6] - m[:, 5] * m[:, 2]
                det = m[:, 0] * c00 + m[:, 4] * c01 + m[:, 8] * c02
                C = [[c00, c01, c02], [m[:, 8] * m[:, 6] - m[:, 4] * m[:, 10], m[:, 0] * m[:, 10] - m[:, 8] * m[:, 2], m[:, 4] * m[:, 2] - m[:, 0] * m[:, 6]],
                     [m[:, 4] * m[:, 9] - m[:, 8] * m[:, 5], m[:, 8] * m[:, 1] - m[:, 0] * m[:, 9], m[:, 0] * m[:, 5] - m[:, 4] * m[:, 1]]]
                with np.errstate(all="ignore"):
                    for rr in range(3): nrm[:, rr] += np.where(use & (det != 0), wk * (C[rr][0] * n0[:, 0] + C[rr][1] * n0[:, 1] + C[rr][2] * n0[:, 2]) / det, 0.0)
            out[skinned] = q.astype(np.float32)[skinned]
            with np.errstate(all="ignore"):
                l = length(nrm); m = skinned & (l > 0); nw[m] = pack_snorm8((nrm / l[:, None]).astype(np.float32))[m]
                l = length(tan); m = skinned & (l > 0); tw[m] = pack_snorm8(np.concatenate([(tan / l[:, None]).astype(np.float32), tF[:, 3:4]], 1))[m]
        P[sl] = out
        if hasN: NW[sl] = nw; touchedN[sl] = True
        if hasT: TW[sl] = tw; touchedT[sl] = True
    return P, NW, TW, inside, touchedN, touchedT


@pytest.mark.parametrize("name", skin_cases.CASES)
def test_description_and_palette_reproduce_the_host_pose(name, tmp_path):
    case = skin_cases.make(name, tmp_path); a = pt.GltfAnimation(case["path"]); d = a.skinning()
    bindP, bindN, bindT = skin_cases.bind_streams(case["path"])
    assert d.num_matrices > 0 and len(d.ranges) > 0 and len(d.joints) == len(bindP)
    for t in case["times"]:
        m, w = a.palette(t); assert m.shape == (d.num_matrices, 16) and w.shape == (d.num_morph_weights,)
        P, NW, TW, inside, tN, tT = pose(d, bindP, m, w)
        want = a.positions(t); wantN, wantT = a.normals(t)
        assert np.array_equal(P[inside], want[inside]), (name, t)
        assert np.array_equal(want[~inside], bindP[~inside]), (name, t)      # what no range covers, no pose moves
        assert np.array_equal(NW[tN], wantN[tN]) and np.array_equal(TW[tT], wantT[tT]), (name, t)
        assert np.array_equal(wantN[~tN], bindN[~tN]) and np.array_equal(wantT[~tT], bindT[~tT]), (name, t)
    assert any(not np.array_equal(a.positions(t), bindP) for t in case["times"])      # (the cases do move)
    a.close()


@pytest.mark.parametrize("name", skin_cases.CASES)
def test_queries_and_ranges(name, tmp_path):
    case = skin_cases.make(name, tmp_path); a = pt.GltfAnimation(case["path"]); d = a.skinning()
    f = a.L.pt_gltf_animation_palette; assert f(a.h, 0, 0.0, None, 0, None, 0) == d.num_matrices      # capacity 0: a query
    assert len(d.joints) == a.L.pt_gltf_animation_positions(a.h, 0, 0.0, None, 0)
    m = np.zeros((d.num_matrices, 16)); w = np.zeros(max(1, d.num_morph_weights))
    if d.num_matrices > 1: assert f(a.h, 0, 0.0, pt._p(m), d.num_matrices - 1, pt._p(w), len(w)) == -pt.PT_ERROR_INVALID_ARGUMENT      # too small a capacity writes nothing
    cover = np.zeros(len(d.joints), np.int64)
    for r in d.ranges:
        cover[int(r["firstVertex"]):int(r["firstVertex"]) + int(r["numVertices"])] += 1
        assert int(r["firstMatrix"]) + int(r["numMatrices"]) <= d.num_matrices and int(r["firstWeight"]) + int(r["numTargets"]) <= d.num_morph_weights
        assert int(r["firstMorphDelta"]) + 3 * int(r["numTargets"]) * int(r["numVertices"]) <= len(d.morph_position_deltas)
    assert cover.max() <= 1                                  # every vertex lies in at most one range
    assert not cover[case["sentinels"]].any()               # ... and the static meshes in none (case E: before, between and after the deformed ranges)
    if name == "E": assert case["sentinels"][0] and case["sentinels"][-1] and len(d.ranges) == 2 and d.num_matrices == 4      # (one palette per mesh node)
    if name == "B": assert d.num_morph_weights == 2 and d.ranges[0]["numTargets"] == 2 and d.ranges[0]["numMatrices"] == 2
    if name == "C": assert d.num_matrices == 70 and d.ranges[0]["numVertices"] == 1061
    a.close()

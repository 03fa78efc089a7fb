// mi355pt — the pose of one vertex of a deformed mesh: morph targets, then the skin (glTF 2.0 3.7.2.2, 3.7.3; Donut's SkinnedMeshInstance pass in the reference, Sample.cpp:1065,
// 1170-1198 — Donut is not vendored, its skinning shader is not in the reference tree: the arithmetic is the specification's, UNPINNED). One text for both sides:
// pt_gltf.cpp's host pose (pt_gltf_animation_positions / _normals) calls these leaves vertex by vertex, pt_skin.hip's k_skin calls skin_vertex, which is the same leaves in the
// host's order. Every sum is binary64, every stored intermediate binary32 where the host stores one: the morphed position is rounded to binary32 before the skin reads it, the
// morphed normal / tangent are held as binary32. The build has no contraction and no fast math on either side and binary64 + - * / sqrt are correctly rounded on both, so the
// device's streams equal the host's bit for bit (tests/test_gpu_device_skinning.py).
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/mi355pt.h"

#if defined(__HIPCC__)
#define PT_SKIN_HD __host__ __device__
#else
#define PT_SKIN_HD
#endif

namespace ptskin {

PT_SKIN_HD inline uint32_t pack_snorm8(const float* v, int n) {   // Packing.hlsli:127-140
    uint32_t out = 0;
    for (int i = 0; i < n; i++) { float c = v[i] < -1.f ? -1.f : (v[i] > 1.f ? 1.f : v[i]); out |= ((uint32_t)((int)(c * 127.0f)) & 0xFFu) << (8 * i); }
    return out;
}

// The displacement of target i for vertex v of a geometry with numVertices vertices: deltas[((size_t)i * numVertices + v) * 3 + r] (`deltas` at the geometry's first float).
// p = base + SUM_i w_i target_i, summed in binary64 in target order, rounded to binary32. `out` may be `base`.
PT_SKIN_HD inline void morph_position(const float* base, const float* deltas, uint32_t numVertices, uint32_t v, const double* w, uint32_t count, float* out) {
    double p[3] = {base[0], base[1], base[2]};
    for (uint32_t i = 0; i < count; i++) for (int rr = 0; rr < 3; rr++) p[rr] += w[i] * (double)deltas[((size_t)i * numVertices + v) * 3 + rr];      // (per component: the targets in order)
    for (int rr = 0; rr < 3; rr++) out[rr] = (float)p[rr];
}
// n = normalize(bind + SUM_i w_i dn_i), likewise the tangent's xyz (glTF 2.0 3.7.2.2). A stream no target displaces with a non-zero weight, a geometry without the stream and
// a zero-length sum keep what nF (3 floats) / tF (4: xyz and the handedness, which stays) and *outN / *outT hold. outN / outT may be NULL.
PT_SKIN_HD inline void morph_frame(const float* bindN, const float* bindT, const float* deltasN, const float* deltasT, uint32_t numVertices, uint32_t v, const double* w, uint32_t count,
                                   uint32_t geometryFlags, float* nF, float* tF, uint32_t* outN, uint32_t* outT) {
    double dn[3] = {0, 0, 0}, dt[3] = {0, 0, 0}; bool anyN = false, anyT = false;
    for (uint32_t i = 0; i < count; i++) for (int rr = 0; rr < 3; rr++) {
        const float a = deltasN[((size_t)i * numVertices + v) * 3 + rr], b = deltasT[((size_t)i * numVertices + v) * 3 + rr];
        dn[rr] += w[i] * (double)a; dt[rr] += w[i] * (double)b; anyN = anyN || (a != 0.f && w[i] != 0.0); anyT = anyT || (b != 0.f && w[i] != 0.0); }
    if (anyN && (geometryFlags & PT_GEOM_HAS_NORMAL)) { double q[3], l = 0; for (int rr = 0; rr < 3; rr++) { q[rr] = bindN[rr] + dn[rr]; l += q[rr] * q[rr]; } l = sqrt(l);
        if (l > 0) { for (int rr = 0; rr < 3; rr++) nF[rr] = (float)(q[rr] / l); if (outN) *outN = pack_snorm8(nF, 3); } }
    if (anyT && (geometryFlags & PT_GEOM_HAS_TANGENT)) { double q[3], l = 0; for (int rr = 0; rr < 3; rr++) { q[rr] = bindT[rr] + dt[rr]; l += q[rr] * q[rr]; } l = sqrt(l);
        if (l > 0) { for (int rr = 0; rr < 3; rr++) tF[rr] = (float)(q[rr] / l); if (outT) *outT = pack_snorm8(tF, 4); } }
}

// a vertex of a skinned mesh whose weights sum to nothing (an unskinned primitive of the mesh) keeps its morphed pose
PT_SKIN_HD inline bool skinned(const float* wgt) { return wgt[0] + wgt[1] + wgt[2] + wgt[3] > 0.f; }
// q = SUM_k w_k J_k p over the palette `jm` (16 doubles a joint, column major: m[4 c + r]); zero weights and joints beyond the palette are skipped. `out` may be `p`.
PT_SKIN_HD inline void skin_position(const float* pF, const float* wgt, const uint16_t* jnt, const double* jm, uint32_t numMatrices, float* out) {
    const double p[3] = {pF[0], pF[1], pF[2]}; double q[3] = {0, 0, 0};
    for (int k = 0; k < 4; k++) { if (wgt[k] == 0.f || jnt[k] >= numMatrices) continue; const double* m = jm + 16 * (size_t)jnt[k];
        for (int rr = 0; rr < 3; rr++) q[rr] += (double)wgt[k] * (m[rr] * p[0] + m[4 + rr] * p[1] + m[8 + rr] * p[2] + m[12 + rr]); }
    for (int rr = 0; rr < 3; rr++) out[rr] = (float)q[rr];
}
// normal = normalize(SUM_k w_k inverse-transpose(J_k) n0), tangent = normalize(SUM_k w_k J_k t0.xyz) with t0.w kept; n0 / t0: the morphed normal (3) / tangent (4). A joint
// with a singular upper 3 x 3 has no normal term; a zero-length sum keeps *outN / *outT. outN / outT: NULL = not wanted.
PT_SKIN_HD inline void skin_frame(const float* n0, const float* t0, const float* wgt, const uint16_t* jnt, const double* jm, uint32_t numMatrices, uint32_t* outN, uint32_t* outT) {
    double nrm[3] = {0, 0, 0}, tan[3] = {0, 0, 0};
    for (int k = 0; k < 4; k++) { if (wgt[k] == 0.f || jnt[k] >= numMatrices) continue; const double* m = jm + 16 * (size_t)jnt[k];      // column major: m[4 c + r]
        // cofactors of the upper 3 x 3 = det * inverse-transpose
        const double c00 = m[5] * m[10] - m[9] * m[6], c01 = m[9] * m[2] - m[1] * m[10], c02 = m[1] * m[6] - m[5] * m[2];      // (rows of the cofactor matrix, indexed [row][col] of M)
        const double det = m[0] * c00 + m[4] * c01 + m[8] * c02;
        if (det != 0.0) {
            const double C[3][3] = {{c00, c01, c02},
                                    {m[8] * m[6] - m[4] * m[10], m[0] * m[10] - m[8] * m[2], m[4] * m[2] - m[0] * m[6]},
                                    {m[4] * m[9] - m[8] * m[5], m[8] * m[1] - m[0] * m[9], m[0] * m[5] - m[4] * m[1]}};      // C[r][c]: cofactor of M(r, c), M(r, c) = m[4 c + r]; inverse-transpose = C / det
            for (int rr = 0; rr < 3; rr++) nrm[rr] += (double)wgt[k] * (C[rr][0] * n0[0] + C[rr][1] * n0[1] + C[rr][2] * n0[2]) / det;
        }
        for (int rr = 0; rr < 3; rr++) tan[rr] += (double)wgt[k] * (m[rr] * t0[0] + m[4 + rr] * t0[1] + m[8 + rr] * t0[2]);
    }
    if (outN) { const double l = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
        if (l > 0) { float nn[3] = {(float)(nrm[0] / l), (float)(nrm[1] / l), (float)(nrm[2] / l)}; *outN = pack_snorm8(nn, 3); } }
    if (outT) { const double l = sqrt(tan[0] * tan[0] + tan[1] * tan[1] + tan[2] * tan[2]);
        if (l > 0) { float tt[4] = {(float)(tan[0] / l), (float)(tan[1] / l), (float)(tan[2] / l), t0[3]}; *outT = pack_snorm8(tt, 4); } }
}

// The whole pose of one vertex of range `r` (lv: its index inside the range): the leaves above in the order pt_gltf.cpp's pose takes them. bindP / bindN / bindT / jnt / wgt:
// the vertex's own bind position (3; the position the scene held when the description was set), bind normal (3) and tangent (4), joints (4) and weights (4); deltasP / N / T
// and matrices / morphWeights: the description's whole arrays (the host's or the device's). pos: 3 floats; *nWord / *tWord are written only where the geometry has the stream
// (a degenerate result leaves the packed bind value).
PT_SKIN_HD inline void skin_vertex(const PtSkinRange& r, uint32_t lv, const float* bindP, const float* bindN, const float* bindT, const uint16_t* jnt, const float* wgt,
                                   const float* deltasP, const float* deltasN, const float* deltasT, const double* matrices, const double* morphWeights,
                                   float* pos, uint32_t* nWord, uint32_t* tWord) {
    const bool hasN = (r.geometryFlags & PT_GEOM_HAS_NORMAL) != 0, hasT = (r.geometryFlags & PT_GEOM_HAS_TANGENT) != 0;
    float nF[3] = {bindN[0], bindN[1], bindN[2]}, tF[4] = {bindT[0], bindT[1], bindT[2], bindT[3]};
    uint32_t n = pack_snorm8(nF, 3), t = pack_snorm8(tF, 4);
    for (int rr = 0; rr < 3; rr++) pos[rr] = bindP[rr];
    if (r.numTargets) {
        const double* w = morphWeights + r.firstWeight;
        morph_position(pos, deltasP + r.firstMorphDelta, r.numVertices, lv, w, r.numTargets, pos);
        morph_frame(bindN, bindT, deltasN + r.firstMorphDelta, deltasT + r.firstMorphDelta, r.numVertices, lv, w, r.numTargets, r.geometryFlags, nF, tF, &n, &t);
    }
    if (r.numMatrices && skinned(wgt)) {
        const double* jm = matrices + 16 * (size_t)r.firstMatrix;
        skin_position(pos, wgt, jnt, jm, r.numMatrices, pos);
        if (hasN || hasT) skin_frame(nF, tF, wgt, jnt, jm, r.numMatrices, &n, &t);      // (a word of a stream the geometry lacks is dropped below)
    }
    if (hasN) *nWord = n;
    if (hasT) *tWord = t;
}

} // namespace ptskin

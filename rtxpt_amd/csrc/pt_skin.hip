// mi355pt — the device skinning pass (pt_animate_skinned; include/mi355pt.h): k_skin poses every vertex of the skinning description's ranges with pt_skin.h's skin_vertex —
// the text the host pose (pt_gltf.cpp) runs — and writes positions, normals and tangents of the scene's streams in place. Donut's SkinnedMeshInstance pass is its counterpart in
// the reference (Sample.cpp:1065, 1170-1198; Donut is not vendored: UNPINNED).
// One thread per deformed vertex, a flat index over the ranges; a prefix table (numRanges + 1 words) maps the index to its range by bisection. Per vertex the streams cost
// 64 B read (bind position 12, bind normal 12, bind tangent 16, joints 8, weights 16; 36 B more per morph target) and 20 B written (position 12, two packed words). The palette
// (128 B a joint, binary64) is read from global memory by every lane that uses the joint — a few KB that stay in the caches, and no limit on its size. Staging it in LDS
// (every block copying the whole palette first) measured slower at 100 000 and at 1 000 000 vertices and was dropped: docs/WIDENING.md N9 has both timings. The kernel is
// bound by its binary64 arithmetic (four cofactor matrices, eighteen correctly rounded divisions and two square roots a skinned vertex), not by HBM.
#include "pt_context.h"
#include "pt_skin.h"

using namespace ptk;

__global__ __launch_bounds__(256) void k_skin(SkinView s, const double* __restrict__ matrices, const double* __restrict__ morphWeights,
                                              float* __restrict__ positions, uint* __restrict__ normals, uint* __restrict__ tangents) {
    const uint i = blockIdx.x * 256u + threadIdx.x;
    if (i >= s.total) return;
    uint lo = 0u, hi = s.numRanges;                          // the last range that starts at or before i (rangeStart[0] = 0, rangeStart[numRanges] = total)
    while (hi - lo > 1u) { const uint mid = (lo + hi) >> 1; if (s.rangeStart[mid] <= i) lo = mid; else hi = mid; }
    const PtSkinRange r = s.ranges[lo];
    const uint lv = i - s.rangeStart[lo]; const size_t v = (size_t)r.firstVertex + lv;
    const ptk::float4 w4 = reinterpret_cast<const ptk::float4*>(s.weights)[v], t4 = reinterpret_cast<const ptk::float4*>(s.tangents)[v];      // 16 B a lane, consecutive lanes consecutive
    const ptk::uint2 j2 = reinterpret_cast<const ptk::uint2*>(s.joints)[v];
    const float wgt[4] = {w4.x, w4.y, w4.z, w4.w}, bindT[4] = {t4.x, t4.y, t4.z, t4.w};
    const uint16_t jnt[4] = {(uint16_t)(j2.x & 0xFFFFu), (uint16_t)(j2.x >> 16), (uint16_t)(j2.y & 0xFFFFu), (uint16_t)(j2.y >> 16)};
    const float bindP[3] = {s.bindPositions[3 * v], s.bindPositions[3 * v + 1], s.bindPositions[3 * v + 2]};
    const float bindN[3] = {s.normals[3 * v], s.normals[3 * v + 1], s.normals[3 * v + 2]};
    float pos[3];
    ptskin::skin_vertex(r, lv, bindP, bindN, bindT, jnt, wgt, s.deltasP, s.deltasN, s.deltasT, matrices, morphWeights, pos, normals + v, tangents + v);
    positions[3 * v] = pos[0]; positions[3 * v + 1] = pos[1]; positions[3 * v + 2] = pos[2];
}

void launch_skin(const SkinView& s, const double* matrices, const double* morphWeights, float* positions, uint* normals, uint* tangents, hipStream_t st) {
    if (!s.total) return;
    hipLaunchKernelGGL(k_skin, dim3((s.total + 255u) / 256u), dim3(256), 0, st, s, matrices, morphWeights, positions, normals, tangents);
}

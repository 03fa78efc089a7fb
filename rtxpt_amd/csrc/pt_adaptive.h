// mi355pt — adaptive sampling in reference mode (pt_render_adaptive; include/mi355pt.h, docs/WIDENING.md N12): the rank's pixels are sampled in rounds, and between rounds
// the 8 x 8 screen blocks whose error estimate has fallen below the threshold leave the list of pixels that are traced. Ours: the reference accumulates to a fixed
// AccumulationTarget. This file holds the per-pixel text and what the frame driver (pt_frame.hip) and the entry points (pt_adaptive_api.hip) hand to the launches;
// pt_adaptive.hip maps it onto waves.
// Part of the PRODUCT path (libmi355pt.so). Arithmetic contract of pt_vec.h: one binary32 operation at a time in the written order, no contraction; divide and sqrt correctly
// rounded (the Makefile's flags), so that tests/adaptive_ref.py restates every value bit for bit.
#pragma once
#include "pt_wavefront.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

// sample `index` (0-based) folded into the running mean of the samples before it: k_accumulate's expressions (AccumulationPass), which the accumulation buffer and the
// even-sample buffer share
static inline float4 Adaptive_Fold(float4 mean, float4 col, uint index) {
    const float blend = 1.0f / (float)(index + 1u);
    return (blend < 1.f) ? lerp4(mean, col, blend) : col;
}
// a pixel's error: the distance between the mean of all its samples (A) and the mean of the even-indexed ones (H), relative to the square root of its brightness.
// NaN and inf count as converged: they cannot be sampled away
static inline float Adaptive_PixelError(float4 A, float4 H, float darkFloor) {
    const float d = (fabsf(A.x - H.x) + fabsf(A.y - H.y)) + fabsf(A.z - H.z);
    const float b = (A.x + A.y) + A.z;
    float e = d / sqrtf(fmaxf(b, darkFloor));
    if (!(e < INFINITY)) e = 0.0f;
    return e;
}

#pragma clang force_cuda_host_device end

// a block of the active list: its pixels are entries [first, first + count) of the pixel list (count <= 64; fewer at the right and bottom frame edges)
struct AdaptiveBlock { uint first, count; };
static const uint kAdaptiveScanChunk = 256u;      // blocks a workgroup of k_adaptive_scan_chunks scans, one a lane
static inline uint adaptive_chunks(uint numBlocks) { return (numBlocks + kAdaptiveScanChunk - 1u) / kAdaptiveScanChunk; }

// One evaluation: the error of every active block, and the active lists without the blocks that retire, in the same order.
//   pixIn / blkIn [numBlocks]: the active lists; pixOut / blkOut: the new ones (room for the old ones' sizes); accum / half: the frame's two means; blockError: the frame's
//   block map, blocksX blocks a row; flags [numBlocks] and chunks [adaptive_chunks(numBlocks)]: scratch of the scan; totals: {pixels, blocks} of the new lists, left in device
//   memory
struct AdaptiveEval {
    const uint* pixIn; const AdaptiveBlock* blkIn; uint numBlocks; uint* pixOut; AdaptiveBlock* blkOut;
    const float4* accum; const float4* half; float* blockError; uint width, blocksX;
    uint2* flags; uint2* chunks; uint* totals; float threshold, darkFloor;
};
// What one round of pt_render_adaptive adds to a frame of the shared driver (pt_frame.hip render_pixel_list): k_adaptive_accumulate in place of k_accumulate, and — evaluate —
// the launches above behind it, on the context's main stream once every batch has accumulated. hostTotals: pinned, the copy of eval.totals; errorPassMs: the device time of
// the evaluation's launches, set by the driver
struct AdaptiveRound { float4* half; uint* counts; bool evaluate; AdaptiveEval eval; uint* hostTotals; float errorPassMs; };

// k_accumulate over pixels [0, numPix) of a list whose pixels all hold accumCountBase samples, which also keeps `half` (the mean of the even-indexed samples) and adds spp to
// the pixels' counts
void launch_adaptive_accumulate(PathPool pool, const uint* pixels, uint numPix, uint spp, float4* accum, float4* half, uint* counts, uint accumCountBase, uint width, hipStream_t st);
void launch_adaptive_evaluate(const AdaptiveEval& e, hipStream_t st);      // four launches on st; e.numBlocks > 0
} // namespace ptk

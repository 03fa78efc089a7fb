// mi355pt — adaptive sampling's entry points (include/mi355pt.h: pt_adaptive_default_params, pt_render_adaptive, pt_get_adaptive_state, pt_get_adaptive_active): the host side
// of pt_adaptive.h / pt_adaptive.hip. The loop over the rounds lives here; a round is a frame of the shared driver (pt_frame.hip render_pixel_list) over the active pixel list.
// The context keeps the even-sample buffer, the count map, the block error map, the owned list's block table and two pairs of active lists that swap at every evaluation.
#include <cmath>
#include <cstring>
#include "pt_context.h"

using namespace ptk;

void adaptive_drop(pt_context* c) {
    pt_context::Adaptive& A = c->adaptive;
    A.perPixel = A.tableValid = A.stateValid = false; A.ownedBlocks.clear();
    A.activePix = nullptr; A.activeBlk = nullptr; A.activeCount = A.activeBlocks = 0;
}
void adaptive_free(pt_context* c) {
    pt_context::Adaptive& A = c->adaptive;
    A.dBlkOwned.free(); A.dCounts.free(); A.dTotals.free(); A.dHalf.free(); A.dBlockError.free(); A.dFlags.free(); A.dChunks.free();
    for (int s = 0; s < 2; s++) { A.dBlk[s].free(); A.dPix[s].free(); }
    if (A.hostTotals) { (void)hipHostFree(A.hostTotals); A.hostTotals = nullptr; }
    adaptive_drop(c);
}

namespace {
bool params_ok(const PtAdaptiveParams& p) {      // (every comparison is false for a NaN)
    return p.step >= 2u && !(p.step & 1u) && p.minSamples >= p.step && p.maxSamples >= p.minSamples && p.minSamples % p.step == 0u && p.maxSamples % p.step == 0u &&
           p.threshold == p.threshold && p.darkFloor > 0.0f;
}
uint blocks_x(const pt_context* c) { return (c->width + 7u) / 8u; }
uint blocks_y(const pt_context* c) { return (c->height + 7u) / 8u; }
// the owned list as runs of 8 x 8 screen blocks: shard_pixel_lists emits a block's pixels contiguously, and two blocks that follow each other in the list differ
int32_t ensure_block_table(pt_context* c) {
    pt_context::Adaptive& A = c->adaptive;
    if (A.tableValid) return PT_OK;
    A.ownedBlocks.clear();
    uint lastBlock = 0xFFFFFFFFu;
    for (uint i = 0; i < (uint)c->owned.size(); i++) {
        const uint px = c->owned[i], block = ((px & 0xFFFFu) >> 3) * blocks_x(c) + (px >> 19);
        if (block != lastBlock) { A.ownedBlocks.push_back(AdaptiveBlock{i, 0u}); lastBlock = block; }
        A.ownedBlocks.back().count++;
    }
    for (const AdaptiveBlock& b : A.ownedBlocks) if (b.count > 64u) return fail(c, PT_ERROR_HIP, "adaptive sampling: an 8 x 8 block of the owned list with more than 64 pixels");
    const size_t nb = A.ownedBlocks.size(), np = c->owned.size();
    PT_CHECK_HIP(c, A.dBlkOwned.upload(A.ownedBlocks, c->stream));
    for (int s = 0; s < 2; s++) { PT_CHECK_HIP(c, A.dBlk[s].resize(nb)); PT_CHECK_HIP(c, A.dPix[s].resize(np)); }
    PT_CHECK_HIP(c, A.dFlags.resize(nb)); PT_CHECK_HIP(c, A.dChunks.resize(adaptive_chunks((uint)nb))); PT_CHECK_HIP(c, A.dTotals.resize(2));
    if (!A.hostTotals) PT_CHECK_HIP(c, hipHostMalloc(&A.hostTotals, 2 * sizeof(uint), hipHostMallocDefault));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    A.tableValid = true;
    return PT_OK;
}
}

extern "C" {

int32_t pt_adaptive_default_params(PtAdaptiveParams* out) {
    if (!out) return PT_ERROR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->minSamples = 16u; out->step = 8u; out->maxSamples = 1024u; out->threshold = 0.02f; out->darkFloor = 0.01f;      // ours, unmeasured (include/mi355pt.h)
    return PT_OK;
}

int32_t pt_render_adaptive(pt_context* c, const PtAdaptiveParams* params, PtAdaptiveStats* stats, PtFrameStats* frameStats) {
    if (!c || !params) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    if (!params_ok(*params))
        return fail(c, PT_ERROR_INVALID_ARGUMENT, "adaptive parameters: step even and >= 2, minSamples and maxSamples multiples of step, step <= minSamples <= maxSamples, "
                                                  "threshold not NaN, darkFloor > 0");
    if (c->neeat.enabled || c->feedbackRequired)
        return fail(c, PT_ERROR_INVALID_ARGUMENT, "adaptive sampling is not for NEE-AT (pt_set_neeat, the temporal feedback of pt_set_local_light_sampling): its reservoirs "
                                                  "couple pixels and frames, so a pixel's value would depend on which other pixels are still sampled");
    (void)hipSetDevice(c->device);
    int32_t r = prepare(c); if (r != PT_OK) return r;
    r = ensure_block_table(c); if (r != PT_OK) return r;
    pt_context::Adaptive& A = c->adaptive;
    const size_t N = (size_t)c->width * c->height, NB = (size_t)blocks_x(c) * blocks_y(c);
    PT_CHECK_HIP(c, A.dHalf.resize(N)); PT_CHECK_HIP(c, A.dCounts.resize(N)); PT_CHECK_HIP(c, A.dBlockError.resize(NB));
    // a new accumulation: the first sample of a pixel overwrites both means (blend 1), the maps start from zero for the pixels of other shards' sake
    A.stateValid = false; A.perPixel = true; c->accumCount = 0; accum_denoise_drop(c);
    PT_CHECK_HIP(c, hipMemsetAsync(c->dAccum.p, 0, sizeof(ptk::float4) * N, c->stream)); PT_CHECK_HIP(c, hipMemsetAsync(A.dHalf.p, 0, sizeof(ptk::float4) * N, c->stream));
    PT_CHECK_HIP(c, hipMemsetAsync(A.dCounts.p, 0, sizeof(uint) * N, c->stream)); PT_CHECK_HIP(c, hipMemsetAsync(A.dBlockError.p, 0, sizeof(float) * NB, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));

    PtAdaptiveStats S; memset(&S, 0, sizeof(S));
    PtFrameStats total; memset(&total, 0, sizeof(total));
    A.activePix = c->dOwned.p; A.activeBlk = A.dBlkOwned.p; A.activeCount = (uint)c->owned.size(); A.activeBlocks = (uint)A.ownedBlocks.size();
    uint n = 0, side = 0; bool retired = false;
    while (A.activeCount && n < params->maxSamples) {
        AdaptiveRound round; memset(&round, 0, sizeof(round));
        round.half = A.dHalf.p; round.counts = A.dCounts.p; round.evaluate = n + params->step >= params->minSamples; round.hostTotals = A.hostTotals;
        round.eval = AdaptiveEval{A.activePix, A.activeBlk, A.activeBlocks, A.dPix[side].p, A.dBlk[side].p, c->dAccum.p, A.dHalf.p, A.dBlockError.p, c->width, blocks_x(c),
                                  A.dFlags.p, A.dChunks.p, A.dTotals.p, params->threshold, params->darkFloor};
        PtFrameStats one;
        r = render_pixel_list(c, A.activePix, A.activeCount, n, params->step, n, &round, &one);
        if (r != PT_OK) return r;      // (the accumulation stays per pixel and without a readable state: reset it)
        add_frame_stats(total, one);
        n += params->step; S.rounds++; S.samplesTraced += (uint64_t)A.activeCount * params->step; S.maxCount = n;
        if (!round.evaluate) continue;
        S.evaluations++; S.errorPassMs += round.errorPassMs;
        const uint keptPixels = A.hostTotals[0], keptBlocks = A.hostTotals[1];
        if (keptPixels > A.activeCount || keptBlocks > A.activeBlocks) return fail(c, PT_ERROR_HIP, "adaptive sampling: the compacted lists grew");
        if (keptPixels < A.activeCount && !retired) { retired = true; S.minCount = n; }
        A.activePix = A.dPix[side].p; A.activeBlk = A.dBlk[side].p; A.activeCount = keptPixels; A.activeBlocks = keptBlocks; side ^= 1u;
    }
    if (!retired) S.minCount = S.maxCount;
    S.unconvergedPixels = A.activeCount;
    c->accumCount = S.maxCount; A.stateValid = true;
    if (stats) *stats = S;
    if (frameStats) *frameStats = total;
    return PT_OK;
}

int32_t pt_get_adaptive_state(pt_context* c, uint32_t* sampleCounts, float* halfRgba32f, float* blockError) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->adaptive.stateValid) return fail(c, PT_ERROR_NOT_READY, "no adaptive render of this frame size yet: pt_render_adaptive");
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)c->width * c->height, NB = (size_t)blocks_x(c) * blocks_y(c);
    if (sampleCounts) PT_CHECK_HIP(c, hipMemcpy(sampleCounts, c->adaptive.dCounts.p, sizeof(uint) * N, hipMemcpyDeviceToHost));
    if (halfRgba32f) PT_CHECK_HIP(c, hipMemcpy(halfRgba32f, c->adaptive.dHalf.p, sizeof(ptk::float4) * N, hipMemcpyDeviceToHost));
    if (blockError) PT_CHECK_HIP(c, hipMemcpy(blockError, c->adaptive.dBlockError.p, sizeof(float) * NB, hipMemcpyDeviceToHost));
    return PT_OK;
}

int32_t pt_get_adaptive_active(pt_context* c, uint32_t* pixels, uint32_t capacity) {
    if (!c) return -PT_ERROR_INVALID_ARGUMENT;
    if (!c->adaptive.stateValid) return -fail(c, PT_ERROR_NOT_READY, "no adaptive render of this frame size yet: pt_render_adaptive");
    const uint n = c->adaptive.activeCount;
    if (!capacity || !pixels) return (int32_t)n;
    if (capacity < n) return -fail(c, PT_ERROR_INVALID_ARGUMENT, "capacity below the count of active pixels");
    (void)hipSetDevice(c->device);
    if (n && hipMemcpy(pixels, c->adaptive.activePix, sizeof(uint) * n, hipMemcpyDeviceToHost) != hipSuccess) return -fail(c, PT_ERROR_HIP, "hipMemcpy of the active list");
    return (int32_t)n;
}

}

// mi355pt — the device denoiser's entry points (include/mi355pt.h: pt_denoise_default_settings, pt_denoise_plane, pt_denoised_device_buffers, pt_get_denoised, pt_denoise_frame,
// pt_denoise_pass_times): the host side of pt_relax.h / pt_relax.hip. Per plane the context keeps two histories (previous / current frame) and swaps them after every call.
#include <cstring>
#include "pt_context.h"
#include "pt_relax.h"

using namespace ptk;

static_assert(sizeof(::PtDenoiseSettings) == sizeof(ptk::RelaxSettings), "denoise settings ABI");

void relax_drop_history(pt_context* c) { for (int p = 0; p < 3; p++) { c->rxHistory[p] = false; c->rxDenoised[p] = false; } c->dnPreparedPlane = -1; }
void relax_free(pt_context* c) {
    for (int p = 0; p < 3; p++) { for (int s = 0; s < 2; s++) { for (int i = 0; i < 5; i++) c->dRxHist[p][s][i].free(); c->dRxOut[p][s].free(); } }
    c->dRxGuide.free(); for (int s = 0; s < 2; s++) { c->dRxPing[s].free(); c->dRxPong[s].free(); }
    for (hipEvent_t e : c->rxEvents) (void)hipEventDestroy(e);
    c->rxEvents.clear(); c->rxW = c->rxH = 0; relax_drop_history(c);
}

namespace {
RelaxHistory history(pt_context* c, uint plane, uint side) {
    DevBuf<ptk::float4>* h = c->dRxHist[plane][side];
    RelaxHistory H; H.DiffLen = h[0].p; H.SpecLen = h[1].p; H.FastDiffM1 = h[2].p; H.FastSpecM1 = h[3].p; H.M2Guide = h[4].p; return H;
}
// the shared buffers for this frame size, and plane `plane`'s own; another size than the last call's drops every plane's history
int32_t relax_alloc(pt_context* c, uint plane) {
    const size_t N = (size_t)c->width * c->height;
    if (c->rxW != c->width || c->rxH != c->height) { relax_drop_history(c); c->rxW = c->width; c->rxH = c->height; }
    PT_CHECK_HIP(c, c->dRxGuide.resize(N));
    for (int s = 0; s < 2; s++) { PT_CHECK_HIP(c, c->dRxPing[s].resize(N)); PT_CHECK_HIP(c, c->dRxPong[s].resize(N)); PT_CHECK_HIP(c, c->dRxOut[plane][s].resize(N)); }
    for (int s = 0; s < 2; s++) for (int i = 0; i < 5; i++) PT_CHECK_HIP(c, c->dRxHist[plane][s][i].resize(N));
    return PT_OK;
}
bool settings_ok(const PtDenoiseSettings& s) {
    return s.atrousIterationNum >= 2u && s.atrousIterationNum <= 8u && s.depthThreshold > 0.0f && s.lobeAngleFraction > 0.0f && s.lobeAngleFraction <= 1.0f &&
           s.diffuseMaxAccumulatedFrameNum >= 1u && s.specularMaxAccumulatedFrameNum >= 1u && s.diffuseMaxFastAccumulatedFrameNum >= 1u && s.specularMaxFastAccumulatedFrameNum >= 1u &&
           s.disocclusionThreshold >= 0.0f && s.disocclusionThresholdAlternate >= 0.0f && s.luminanceSigmaScale == s.luminanceSigmaScale;
}
}

extern "C" {

int32_t pt_denoise_default_settings(PtDenoiseSettings* out) {
    if (!out) return PT_ERROR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->atrousIterationNum = 5u; out->depthThreshold = 0.004f; out->lobeAngleFraction = 0.7f;                                  // NrdConfig.cpp:15-47
    out->diffuseMaxAccumulatedFrameNum = 25u; out->specularMaxAccumulatedFrameNum = 40u; out->diffuseMaxFastAccumulatedFrameNum = 5u; out->specularMaxFastAccumulatedFrameNum = 6u;
    out->enableAntiFirefly = 1u;
    out->disocclusionThreshold = 0.03f; out->disocclusionThresholdAlternate = 0.2f; out->useDisocclusionThresholdMix = 1u;      // SampleUI.h:294-296
    out->luminanceSigmaScale = 4.0f;
    return PT_OK;
}

int32_t pt_denoise_plane(pt_context* c, const PtStablePlanesParams* spParams, const PtDenoiseSettings* settings, uint32_t planeIndex, uint32_t resetHistory) {
    if (!c || !spParams || !settings) return PT_ERROR_INVALID_ARGUMENT;
    if (planeIndex >= cStablePlaneCount) return fail(c, PT_ERROR_INVALID_ARGUMENT, "plane index out of range (0..2)");
    if (!settings_ok(*settings)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "denoise settings out of range (atrousIterationNum 2..8, depthThreshold > 0, lobeAngleFraction in (0, 1], frame numbers >= 1)");
    int32_t r = dn_ready(c); if (r != PT_OK) return r;
    if (!c->dnW || c->dnW != c->width || c->dnH != c->height || c->dnPreparedPlane != (int)planeIndex)
        return fail(c, PT_ERROR_NOT_READY, "the denoiser runs on the NRD buffers of this plane: pt_denoiser_prepare_nrd of it on this frame first (one denoise per prepare)");
    (void)hipSetDevice(c->device);
    r = relax_alloc(c, planeIndex); if (r != PT_OK) return r;
    RelaxSettings S; memcpy(&S, settings, sizeof(S));
    const DenoiserBuffers D = dn_buffers(c);
    const uint w = c->width, h = c->height, side = c->rxSide[planeIndex], passes = 2u + S.atrousIterationNum;
    hipStream_t st = c->stream;
    if (c->rxTiming) while (c->rxEvents.size() < passes + 1u) { hipEvent_t e; PT_CHECK_HIP(c, hipEventCreate(&e)); c->rxEvents.push_back(e); }
    uint ev = 0;
    auto stamp = [&]() { if (c->rxTiming) (void)hipEventRecord(c->rxEvents[ev++], st); };
    const RelaxHistory cur = history(c, planeIndex, side ^ 1u);
    // the history must be of this build pass (a second call on one frame) or of the one before: a plane that sat out a frame starts again
    const bool hasHistory = c->rxHistory[planeIndex] && !resetHistory && c->spFrameSerial - c->rxFrameSerial[planeIndex] <= 1u;
    stamp(); launch_relax_temporal(D, S, history(c, planeIndex, side), cur, c->dRxGuide.p, w, h, hasHistory, st);
    stamp(); launch_relax_clamp(D, S, cur, c->dRxGuide.p, c->dRxPing[0].p, c->dRxPing[1].p, w, h, st);
    for (uint i = 0; i < S.atrousIterationNum; i++) {
        const bool last = i + 1u == S.atrousIterationNum;
        DevBuf<ptk::float4>* in = (i & 1u) ? c->dRxPong : c->dRxPing; DevBuf<ptk::float4>* out = last ? c->dRxOut[planeIndex] : ((i & 1u) ? c->dRxPing : c->dRxPong);
        stamp(); launch_relax_atrous(D, S, c->dRxGuide.p, in[0].p, in[1].p, out[0].p, out[1].p, i, last, w, h, st);
    }
    stamp();
    c->rxSide[planeIndex] = side ^ 1u; c->rxHistory[planeIndex] = true; c->rxFrameSerial[planeIndex] = c->spFrameSerial; c->rxDenoised[planeIndex] = true; c->dnPreparedPlane = -1;
    PT_CHECK_HIP(c, hipStreamSynchronize(st)); PT_CHECK_HIP(c, hipGetLastError());
    if (c->rxTiming) { c->rxPassMs.assign(passes, 0.0f); for (uint i = 0; i < passes; i++) PT_CHECK_HIP(c, hipEventElapsedTime(&c->rxPassMs[i], c->rxEvents[i], c->rxEvents[i + 1u])); }
    return PT_OK;
}

int32_t pt_denoised_device_buffers(pt_context* c, uint32_t planeIndex, void** diffDevice, void** specDevice, size_t* pitch) {
    if (!c || !diffDevice || !specDevice) return PT_ERROR_INVALID_ARGUMENT;
    if (planeIndex >= cStablePlaneCount) return fail(c, PT_ERROR_INVALID_ARGUMENT, "plane index out of range (0..2)");
    if (!c->rxDenoised[planeIndex] || c->rxW != c->width || c->rxH != c->height) return fail(c, PT_ERROR_NOT_READY, "no denoised plane of this frame size yet: pt_denoise_plane");
    *diffDevice = c->dRxOut[planeIndex][0].p; *specDevice = c->dRxOut[planeIndex][1].p; if (pitch) *pitch = (size_t)c->width * 16u;
    return PT_OK;
}

int32_t pt_get_denoised(pt_context* c, uint32_t planeIndex, float* diff, float* spec, float* historyLength) {
    void *d = nullptr, *s = nullptr;
    int32_t r = pt_denoised_device_buffers(c, planeIndex, &d, &s, nullptr); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)c->width * c->height;
    if (diff) PT_CHECK_HIP(c, hipMemcpy(diff, d, 16u * N, hipMemcpyDeviceToHost));
    if (spec) PT_CHECK_HIP(c, hipMemcpy(spec, s, 16u * N, hipMemcpyDeviceToHost));
    if (historyLength) {      // the .w of the current history's two radiance records, interleaved
        const RelaxHistory H = history(c, planeIndex, c->rxSide[planeIndex]);
        PT_CHECK_HIP(c, hipMemcpy2D(historyLength, 8u, (const char*)H.DiffLen + 12, 16u, 4u, N, hipMemcpyDeviceToHost));
        PT_CHECK_HIP(c, hipMemcpy2D(historyLength + 1, 8u, (const char*)H.SpecLen + 12, 16u, 4u, N, hipMemcpyDeviceToHost));
    }
    return PT_OK;
}

int32_t pt_denoise_frame(pt_context* c, const PtStablePlanesParams* spParams, const PtDenoiserParams* params, const PtDenoiseSettings* settings, uint32_t resetHistory) {
    if (!c || !spParams || !params || !settings) return PT_ERROR_INVALID_ARGUMENT;
    if (!settings_ok(*settings)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "denoise settings out of range (atrousIterationNum 2..8, depthThreshold > 0, lobeAngleFraction in (0, 1], frame numbers >= 1)");
    const uint active = spParams->activeStablePlaneCount < 1u ? 1u : (spParams->activeStablePlaneCount > cStablePlaneCount ? cStablePlaneCount : spParams->activeStablePlaneCount);
    for (int p = (int)active - 1; p >= 0; p--) {      // Sample.cpp:2589
        int32_t r = pt_denoiser_prepare_nrd(c, spParams, params, (uint32_t)p, p == (int)active - 1 ? 1u : 0u); if (r != PT_OK) return r;
        r = pt_denoise_plane(c, spParams, settings, (uint32_t)p, resetHistory); if (r != PT_OK) return r;
        r = pt_denoiser_merge_nrd(c, (uint32_t)p, (const float*)c->dRxOut[p][0].p, (const float*)c->dRxOut[p][1].p); if (r != PT_OK) return r;
    }
    return PT_OK;
}

int32_t pt_denoise_pass_times(pt_context* c, uint32_t enable, float* ms, uint32_t capacity, uint32_t* count) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    c->rxTiming = enable != 0u;
    const uint32_t n = (uint32_t)c->rxPassMs.size();
    if (ms) { if (capacity < n) return fail(c, PT_ERROR_INVALID_ARGUMENT, "capacity smaller than the number of passes (2 + atrousIterationNum)"); if (n) memcpy(ms, c->rxPassMs.data(), sizeof(float) * n); }
    if (count) *count = n;
    return PT_OK;
}

}

// mi355pt — the bloom pass's entry points (include/mi355pt.h: pt_bloom_default_params, pt_bloom_kernel, pt_bloom, pt_bloomed_device_buffer, pt_get_bloomed, pt_tonemap_bloomed,
// pt_average_luminance_bloomed): the host side of pt_bloom.h / pt_bloom.hip. The context keeps a third RGBA32F picture for the result — the reference blooms ProcessedOutputColor
// in place, but here the resolved picture is the next frame's history and the radiance buffer belongs to accumulation and the merge, so neither is written — and two
// quarter-resolution images for the blur.
#include <cmath>
#include <cstring>
#include "pt_context.h"
#include "pt_bloom.h"

using namespace ptk;

void bloom_drop(pt_context* c) { c->bloomReady = false; }
void bloom_free(pt_context* c) {
    c->dBloom.free();
    for (int s = 0; s < 2; s++) { c->dBloomQ[s].free(); if (c->bloomEvents[s]) { (void)hipEventDestroy(c->bloomEvents[s]); c->bloomEvents[s] = nullptr; } }
    c->bloomW = c->bloomH = 0; bloom_drop(c);
}

namespace {
bool params_ok(const PtBloomParams& p) {      // (every comparison is false for a NaN)
    return p.radius >= 0.0f && p.radius <= 64.0f && p.intensity >= 0.0f && p.intensity <= 1.0f && p.maxRadiance > 0.0f && p.maxRadiance <= kDenoiserViewZSkyMarker;
}
int32_t bloomed_ready(pt_context* c) {
    if (!c->bloomReady || c->bloomW != c->width || c->bloomH != c->height) return fail(c, PT_ERROR_NOT_READY, "no bloomed picture of this frame size yet: pt_bloom");
    return PT_OK;
}
// sigma = radius / 4 (the blur runs at quarter resolution), R = max(1, ceil(3 sigma)), g[i] = exp(-i^2 / (2 sigma^2)) in double rounded to float, G summed in float
bool taps(float radius, BloomTaps& K) {
    if (!(radius > 0.0f && radius <= 64.0f)) return false;
    const double sigma = 0.25 * (double)radius;
    int R = (int)ceil(3.0 * sigma); if (R < 1) R = 1;
    if (R > kBloomMaxTaps) return false;
    memset(&K, 0, sizeof(K));
    K.R = (uint)R; K.g[0] = 1.0f;
    for (int i = 1; i <= R; i++) K.g[i] = (float)exp(-(double)(i * i) / (2.0 * sigma * sigma));
    float G = 1.0f;
    for (int i = 1; i <= R; i++) G = G + K.g[i] * 2.0f;
    K.G = G;
    return true;
}
}

extern "C" {

int32_t pt_bloom_default_params(PtBloomParams* out) {
    if (!out) return PT_ERROR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->radius = 8.0f; out->intensity = 0.004f; out->maxRadiance = 10000.0f; out->enable = 1u;      // SampleUI.h:306; :307; ours; SampleUI.h:305
    return PT_OK;
}

int32_t pt_bloom_kernel(float radius, float* weights, uint32_t capacity, uint32_t* tapCount, float* weightSum) {
    BloomTaps K;
    if (!weights || !tapCount || !taps(radius, K) || capacity < K.R + 1u) return PT_ERROR_INVALID_ARGUMENT;
    memcpy(weights, K.g, sizeof(float) * (K.R + 1u)); *tapCount = K.R;
    if (weightSum) *weightSum = K.G;
    return PT_OK;
}

int32_t pt_bloom(pt_context* c, const PtBloomParams* params, uint32_t source, float* gpuMs) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (source > 1u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom source: 0 (the radiance buffer) or 1 (the resolved picture)");
    if (!params_ok(*params)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom parameters out of range (radius in [0, 64], intensity in [0, 1], maxRadiance > 0, all finite)");
    if (source == 0u) { if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first"); }
    else { int32_t r = taa_resolved_ready(c); if (r != PT_OK) return r; }
    return bloom_run(c, params, source == 0u ? c->dAccum.p : c->dTaa[c->taaSide].p, gpuMs);
}

}

int32_t bloom_run(pt_context* c, const PtBloomParams* params, const ptk::float4* src, float* gpuMs) {
    if (!params_ok(*params)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom parameters out of range (radius in [0, 64], intensity in [0, 1], maxRadiance > 0, all finite)");
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)c->width * c->height, NQ = (size_t)bloom_reduced(c->width) * bloom_reduced(c->height);
    const bool skipped = !(params->enable && params->intensity > 0.0f && params->radius > 0.0f);      // Sample.cpp:1834
    BloomTaps K;
    if (!skipped && !taps(params->radius, K)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom radius");
    if (gpuMs) for (int s = 0; s < 2; s++) if (!c->bloomEvents[s]) PT_CHECK_HIP(c, hipEventCreate(&c->bloomEvents[s]));
    if (!skipped) for (int s = 0; s < 2; s++) PT_CHECK_HIP(c, c->dBloomQ[s].resize(NQ));
    // the previous picture is given up only here, after the last host step that can fail without touching it: from the resize of its buffer on it is no longer whole
    bloom_drop(c); c->bloomW = c->width; c->bloomH = c->height;
    PT_CHECK_HIP(c, c->dBloom.resize(N));
    hipStream_t st = c->stream;
    if (gpuMs) PT_CHECK_HIP(c, hipEventRecord(c->bloomEvents[0], st));
    if (skipped) PT_CHECK_HIP(c, hipMemcpyAsync(c->dBloom.p, src, N * sizeof(ptk::float4), hipMemcpyDeviceToDevice, st));      // the source's bytes, alpha and NaNs included
    else launch_bloom(src, c->dBloomQ[0].p, c->dBloomQ[1].p, c->dBloom.p, K, params->intensity, params->maxRadiance, c->width, c->height, st);
    if (gpuMs) PT_CHECK_HIP(c, hipEventRecord(c->bloomEvents[1], st));
    PT_CHECK_HIP(c, hipStreamSynchronize(st)); PT_CHECK_HIP(c, hipGetLastError());
    if (gpuMs) PT_CHECK_HIP(c, hipEventElapsedTime(gpuMs, c->bloomEvents[0], c->bloomEvents[1]));
    c->bloomReady = true;
    return PT_OK;
}

extern "C" {

int32_t pt_bloomed_device_buffer(pt_context* c, void** devicePtr, size_t* pitch) {
    if (!c || !devicePtr) return PT_ERROR_INVALID_ARGUMENT;
    int32_t r = bloomed_ready(c); if (r != PT_OK) return r;
    *devicePtr = c->dBloom.p; if (pitch) *pitch = (size_t)c->width * 16u;
    return PT_OK;
}

int32_t pt_get_bloomed(pt_context* c, float* rgba) {
    if (!c || !rgba) return PT_ERROR_INVALID_ARGUMENT;
    int32_t r = bloomed_ready(c); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    PT_CHECK_HIP(c, hipMemcpy(rgba, c->dBloom.p, 16u * (size_t)c->width * c->height, hipMemcpyDeviceToHost));
    return PT_OK;
}

int32_t pt_tonemap_bloomed(pt_context* c, const PtToneMapParams* params, uint8_t* rgba8, size_t bytes) {
    if (!c || !params || !rgba8) return PT_ERROR_INVALID_ARGUMENT;
    int32_t r = bloomed_ready(c); if (r != PT_OK) return r;
    const size_t n = (size_t)c->width * c->height;
    if (bytes < n * 4) return fail(c, PT_ERROR_INVALID_ARGUMENT, "rgba8 buffer too small");
    if (params->toneMapOperator > 5u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "unknown tone map operator");
    (void)hipSetDevice(c->device);
    static_assert(sizeof(PtToneMapParams) == sizeof(ptk::ToneMapParams), "tone map parameter layout");
    ptk::ToneMapParams p; memcpy(&p, params, sizeof(p));
    DevBuf<uint> d; PT_CHECK_HIP(c, d.resize(n));
    launch_tonemap(c->dBloom.p, (uint)n, p, d.p, c->stream);      // pt_tonemap's kernel, pointed at the bloomed picture
    PT_CHECK_HIP(c, hipMemcpyAsync(rgba8, d.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipGetLastError());
    d.free();
    return PT_OK;
}

int32_t pt_average_luminance_bloomed(pt_context* c, float* avgLuminance) {
    if (!c || !avgLuminance) return PT_ERROR_INVALID_ARGUMENT;
    int32_t r = bloomed_ready(c); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)ptk::tm_pow2_floor(c->width) * ptk::tm_pow2_floor(c->height);
    DevBuf<float> d; PT_CHECK_HIP(c, d.resize(2 * n));
    float* result = nullptr; float logLum = 0.f;
    launch_average_log_luminance(c->dBloom.p, c->width, c->height, d.p, &result, c->stream);      // pt_average_luminance's kernels, pointed at the bloomed picture
    PT_CHECK_HIP(c, hipMemcpyAsync(&logLum, result, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipGetLastError());
    d.free();
    *avgLuminance = exp2f(logLum);                      // ToneMappingPasses.cpp:284
    return PT_OK;
}

}

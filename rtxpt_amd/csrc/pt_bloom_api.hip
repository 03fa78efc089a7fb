// mi355pt — the bloom pass's entry points (include/mi355pt.h: pt_bloom_default_params, pt_bloom_kernel, pt_bloom, pt_bloom_upscaled, pt_bloom_accum_denoised,
// pt_bloomed_device_buffer, pt_get_bloomed; pt_tonemap_bloomed and pt_average_luminance_bloomed are in pt_display.hip, over view_bloomed): the host side of pt_bloom.h /
// pt_bloom.hip. A bloomed picture is a BloomState (pt_context.h): an RGBA32F picture of its own for the result — the reference blooms ProcessedOutputColor in place, but here
// the resolved picture is the next frame's history and the radiance buffer belongs to accumulation and the merge, so no source is written — and two quarter-resolution images
// for the blur. The context has one at the frame size (pt_bloom, pt_bloom_accum_denoised) and one at the display size (pt_bloom_upscaled); one driver, bloom_run, fills either.
#include <cmath>
#include <cstring>
#include "pt_display.h"
#include "pt_bloom.h"

using namespace ptk;

void bloom_drop(pt_context* c) { c->bloom.ready = false; }
void bloom_free(pt_context* c) { c->bloom.free(); }
int32_t view_bloomed(pt_context* c, PictureView* v) {
    const BloomState& B = c->bloom;
    if (!B.ready || B.w != c->width || B.h != c->height) return fail(c, PT_ERROR_NOT_READY, "no bloomed picture of this frame size yet: pt_bloom");
    *v = {B.out.p, B.w, B.h};
    return PT_OK;
}

namespace {
int32_t check_params(pt_context* c, const PtBloomParams& p) {      // (every comparison is false for a NaN)
    if (p.radius >= 0.0f && p.radius <= 64.0f && p.intensity >= 0.0f && p.intensity <= 1.0f && p.maxRadiance > 0.0f && p.maxRadiance <= kDenoiserViewZSkyMarker) return PT_OK;
    return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom parameters out of range (radius in [0, 64], intensity in [0, 1], maxRadiance > 0, all finite)");
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
// The pass: `src` bloomed into B. The caller has checked the parameters (check_params) and resolved the source.
int32_t bloom_run(pt_context* c, BloomState& B, const PtBloomParams& params, const PictureView& src, float* gpuMs) {
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)src.w * src.h, NQ = (size_t)bloom_reduced(src.w) * bloom_reduced(src.h);
    const bool skipped = !(params.enable && params.intensity > 0.0f && params.radius > 0.0f);      // Sample.cpp:1834
    BloomTaps K;
    if (!skipped && !taps(params.radius, K)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom radius");
    if (gpuMs) PT_CHECK_HIP(c, B.timer.create());
    if (!skipped) for (int s = 0; s < 2; s++) PT_CHECK_HIP(c, B.q[s].resize(NQ));
    // the previous picture is given up only here, after the last host step that can fail without touching it: from the resize of its buffer on it is no longer whole
    B.ready = false; B.w = src.w; B.h = src.h;
    PT_CHECK_HIP(c, B.out.resize(N));
    hipStream_t st = c->stream;
    PT_CHECK_HIP(c, B.timer.begin(st, gpuMs != nullptr));
    if (skipped) PT_CHECK_HIP(c, hipMemcpyAsync(B.out.p, src.p, N * sizeof(ptk::float4), hipMemcpyDeviceToDevice, st));      // the source's bytes, alpha and NaNs included
    else launch_bloom(src.p, B.q[0].p, B.q[1].p, B.out.p, K, params.intensity, params.maxRadiance, src.w, src.h, st);
    PT_CHECK_HIP(c, B.timer.end(st));
    PT_CHECK_HIP(c, hipStreamSynchronize(st)); PT_CHECK_HIP(c, hipGetLastError());
    PT_CHECK_HIP(c, B.timer.read(gpuMs));
    B.ready = true;
    return PT_OK;
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

// The three passes differ in their source and in the order of their refusals, which a caller can see: pt_bloom looks at the source's number, the parameters and then the
// source; pt_bloom_upscaled at the parameters, then the source; pt_bloom_accum_denoised at the source, then the parameters.
int32_t pt_bloom(pt_context* c, const PtBloomParams* params, uint32_t source, float* gpuMs) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (source > 1u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom source: 0 (the radiance buffer) or 1 (the resolved picture)");
    int32_t r = check_params(c, *params); if (r != PT_OK) return r;
    PictureView src; r = source == 0u ? view_radiance(c, &src) : view_resolved(c, &src); if (r != PT_OK) return r;
    return bloom_run(c, c->bloom, *params, src, gpuMs);
}

int32_t pt_bloom_upscaled(pt_context* c, const PtBloomParams* params, float* gpuMs) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    int32_t r = check_params(c, *params); if (r != PT_OK) return r;
    PictureView src; r = view_upscaled(c, 0u, &src); if (r != PT_OK) return r;
    return bloom_run(c, c->taauBloom, *params, src, gpuMs);      // a display-size bloomed picture of its own: pt_tonemap_upscaled's picture 1
}

int32_t pt_bloom_accum_denoised(pt_context* c, const PtBloomParams* params, float* gpuMs) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    PictureView src; int32_t r = view_accum_denoised(c, &src); if (r != PT_OK) return r;
    r = check_params(c, *params); if (r != PT_OK) return r;
    return bloom_run(c, c->bloom, *params, src, gpuMs);          // the bloomed picture is pt_tonemap_bloomed's
}

int32_t pt_bloomed_device_buffer(pt_context* c, void** devicePtr, size_t* pitch) {
    if (!c || !devicePtr) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_bloomed(c, &v);
    return r != PT_OK ? r : display_device_buffer(v, devicePtr, pitch);
}

int32_t pt_get_bloomed(pt_context* c, float* rgba) {
    if (!c || !rgba) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_bloomed(c, &v);
    return r != PT_OK ? r : display_read_back(c, v, rgba, nullptr);
}

}

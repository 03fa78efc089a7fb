// mi355pt — the temporal upscaling resolve's entry points (include/mi355pt.h: pt_taa_upscale_default_params, pt_taa_upscale, pt_upscaled_size, pt_upscaled_device_buffer,
// pt_get_upscaled, pt_bloom_upscaled, pt_get_upscaled_bloomed, pt_tonemap_upscaled, pt_average_luminance_upscaled, pt_upscale_tex_lod_bias): the host side of pt_taau.h /
// pt_taau.hip and the display tail behind it. The context keeps two display-size RGBA32F buffers that swap after every call, as pt_taa_resolve's do — the one just written is
// the upscaled picture, the other one the history it was resolved against — and a display-size bloomed picture with its two quarter-resolution images. None of them is one of
// pt_taa_resolve's or pt_bloom's buffers, and neither those nor the radiance buffer are written here. The tail runs the existing kernels (launch_bloom, launch_tonemap,
// launch_average_log_luminance) at the display size.
#include <cmath>
#include <cstring>
#include "pt_context.h"
#include "pt_taau.h"
#include "pt_bloom.h"

using namespace ptk;

static_assert(sizeof(::PtTaaUpscaleParams) == sizeof(ptk::TaauParams), "upscaling resolve parameter ABI");

void taau_drop_history(pt_context* c) { c->taauHistory = false; c->taauResolved = false; c->taauBloomReady = false; }
void taau_free(pt_context* c) {
    c->dTaauBloom.free();
    for (int s = 0; s < 2; s++) {
        c->dTaau[s].free(); c->dTaauBloomQ[s].free();
        if (c->taauEvents[s]) { (void)hipEventDestroy(c->taauEvents[s]); c->taauEvents[s] = nullptr; }
        if (c->taauBloomEvents[s]) { (void)hipEventDestroy(c->taauBloomEvents[s]); c->taauBloomEvents[s] = nullptr; }
    }
    c->taauW = c->taauH = c->taauRenderW = c->taauRenderH = 0; taau_drop_history(c);
}

namespace {
bool params_ok(const PtTaaUpscaleParams& p) {      // (every comparison is false for a NaN)
    const PtTaaParams& t = p.taa;
    return t.newFrameWeight > 0.0f && t.newFrameWeight <= 1.0f && t.clampingFactor >= 0.0f && t.clampingFactor <= kDenoiserViewZSkyMarker && t.maxRadiance > 0.0f && t.maxRadiance <= kDenoiserViewZSkyMarker &&
           p.kernelRadius >= 1.0f && p.kernelRadius <= 2.0f;
}
bool bloom_params_ok(const PtBloomParams& p) {     // pt_bloom's ranges
    return p.radius >= 0.0f && p.radius <= 64.0f && p.intensity >= 0.0f && p.intensity <= 1.0f && p.maxRadiance > 0.0f && p.maxRadiance <= kDenoiserViewZSkyMarker;
}
int32_t upscaled_ready(pt_context* c) {
    if (!c->taauResolved || c->taauRenderW != c->width || c->taauRenderH != c->height) return fail(c, PT_ERROR_NOT_READY, "no upscaled picture of this frame size yet: pt_taa_upscale");
    return PT_OK;
}
// picture 0: the upscaled picture; 1: its bloom
int32_t picture(pt_context* c, uint32_t bloomed, const ptk::float4** p) {
    if (bloomed > 1u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloomed: 0 (the upscaled picture) or 1 (its bloom)");
    int32_t r = upscaled_ready(c); if (r != PT_OK) return r;
    if (bloomed && !c->taauBloomReady) return fail(c, PT_ERROR_NOT_READY, "no bloomed upscaled picture yet: pt_bloom_upscaled");
    *p = bloomed ? c->dTaauBloom.p : c->dTaau[c->taauSide].p;
    return PT_OK;
}
int32_t get_picture(pt_context* c, uint32_t bloomed, float* rgba, size_t floats) {
    if (!c || !rgba) return PT_ERROR_INVALID_ARGUMENT;
    const ptk::float4* src; int32_t r = picture(c, bloomed, &src); if (r != PT_OK) return r;
    const size_t n = (size_t)c->taauW * c->taauH;
    if (floats < n * 4) return fail(c, PT_ERROR_INVALID_ARGUMENT, "rgba buffer too small");
    (void)hipSetDevice(c->device);
    PT_CHECK_HIP(c, hipMemcpy(rgba, src, 16u * n, hipMemcpyDeviceToHost));
    return PT_OK;
}
}

extern "C" {

int32_t pt_taa_upscale_default_params(PtTaaUpscaleParams* out) {
    if (!out) return PT_ERROR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    int32_t r = pt_taa_default_params(&out->taa); if (r != PT_OK) return r;
    out->kernelRadius = 1.0f; out->confidenceWeighted = 1u;      // ours; ours
    return PT_OK;
}

int32_t pt_taa_upscale(pt_context* c, const PtTaaUpscaleParams* params, uint32_t displayWidth, uint32_t displayHeight, const float jitter[2], uint32_t resetHistory, float* gpuMs) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (!params_ok(*params)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "upscaling resolve parameters out of range (pt_taa_resolve's ranges; kernelRadius in [1, 2]; all finite)");
    const float jx = jitter ? jitter[0] : 0.0f, jy = jitter ? jitter[1] : 0.0f;
    if (!(jx >= -0.5f && jx <= 0.5f && jy >= -0.5f && jy <= 0.5f)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "jitter: render pixels in [-0.5, 0.5], finite");
    int32_t r = dn_ready(c); if (r != PT_OK) return r;
    const uint w = c->width, h = c->height, W = displayWidth, H = displayHeight;
    // (the kernel's staged footprint is sized from this bound: pt_taau.hip)
    if (W < w || (unsigned long long)W > 4ull * w || H < h || (unsigned long long)H > 4ull * h) return fail(c, PT_ERROR_INVALID_ARGUMENT, "display size outside [w, 4 w] x [h, 4 h]");
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)W * H;
    if (gpuMs) for (int s = 0; s < 2; s++) if (!c->taauEvents[s]) PT_CHECK_HIP(c, hipEventCreate(&c->taauEvents[s]));
    // another display size (or frame size): the history and the pictures are of another one. From here on the previous picture is given up.
    if (c->taauW != W || c->taauH != H || c->taauRenderW != w || c->taauRenderH != h) { taau_drop_history(c); c->taauW = W; c->taauH = H; c->taauRenderW = w; c->taauRenderH = h; }
    for (int s = 0; s < 2; s++) PT_CHECK_HIP(c, c->dTaau[s].resize(N));
    TaauParams P; memcpy(&P, params, sizeof(P));
    const TaauFrame F = TAAU_MakeFrame(w, h, W, H, jx, jy, P.kernelRadius);
    // pt_taa_resolve's two rules, the first with a serial of its own: the history is of this build pass or of the one before; the relax buffer is this build pass's
    const bool hasHistory = c->taauHistory && !resetHistory && c->spFrameSerial - c->taauFrameSerial <= 1u;
    const bool haveRelax = P.taa.useHistoryClampRelax && c->dnW == w && c->dnH == h && c->dnW && c->dnNrdSerial == c->spFrameSerial;
    const uint side = c->taauSide ^ 1u;
    hipStream_t st = c->stream;
    if (gpuMs) PT_CHECK_HIP(c, hipEventRecord(c->taauEvents[0], st));
    launch_taa_upscale(c->dAccum.p, c->dSpMotion.p, haveRelax ? c->dDnHistoryClamp.p : nullptr, hasHistory ? c->dTaau[side ^ 1u].p : nullptr, c->dTaau[side].p, P, F, st);
    if (gpuMs) PT_CHECK_HIP(c, hipEventRecord(c->taauEvents[1], st));
    c->taauSide = side; c->taauHistory = true; c->taauResolved = true; c->taauBloomReady = false; c->taauFrameSerial = c->spFrameSerial;
    PT_CHECK_HIP(c, hipStreamSynchronize(st)); PT_CHECK_HIP(c, hipGetLastError());
    if (gpuMs) PT_CHECK_HIP(c, hipEventElapsedTime(gpuMs, c->taauEvents[0], c->taauEvents[1]));
    return PT_OK;
}

int32_t pt_upscaled_size(pt_context* c, uint32_t* width, uint32_t* height) {
    if (!c || !width || !height) return PT_ERROR_INVALID_ARGUMENT;
    int32_t r = upscaled_ready(c); if (r != PT_OK) return r;
    *width = c->taauW; *height = c->taauH;
    return PT_OK;
}

int32_t pt_upscaled_device_buffer(pt_context* c, void** devicePtr, size_t* pitch) {
    if (!c || !devicePtr) return PT_ERROR_INVALID_ARGUMENT;
    int32_t r = upscaled_ready(c); if (r != PT_OK) return r;
    *devicePtr = c->dTaau[c->taauSide].p; if (pitch) *pitch = (size_t)c->taauW * 16u;
    return PT_OK;
}

int32_t pt_get_upscaled(pt_context* c, float* rgba, size_t floats) { return get_picture(c, 0u, rgba, floats); }
int32_t pt_get_upscaled_bloomed(pt_context* c, float* rgba, size_t floats) { return get_picture(c, 1u, rgba, floats); }

int32_t pt_bloom_upscaled(pt_context* c, const PtBloomParams* params, float* gpuMs) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (!bloom_params_ok(*params)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom parameters out of range (radius in [0, 64], intensity in [0, 1], maxRadiance > 0, all finite)");
    int32_t r = upscaled_ready(c); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    const uint W = c->taauW, H = c->taauH;
    const size_t N = (size_t)W * H, NQ = (size_t)bloom_reduced(W) * bloom_reduced(H);
    const ptk::float4* src = c->dTaau[c->taauSide].p;
    const bool skipped = !(params->enable && params->intensity > 0.0f && params->radius > 0.0f);      // Sample.cpp:1834, as pt_bloom
    BloomTaps K; memset(&K, 0, sizeof(K));
    if (!skipped && pt_bloom_kernel(params->radius, K.g, (uint32_t)kBloomMaxTaps + 1u, &K.R, &K.G) != PT_OK) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloom radius");
    if (gpuMs) for (int s = 0; s < 2; s++) if (!c->taauBloomEvents[s]) PT_CHECK_HIP(c, hipEventCreate(&c->taauBloomEvents[s]));
    if (!skipped) for (int s = 0; s < 2; s++) PT_CHECK_HIP(c, c->dTaauBloomQ[s].resize(NQ));
    c->taauBloomReady = false;
    PT_CHECK_HIP(c, c->dTaauBloom.resize(N));
    hipStream_t st = c->stream;
    if (gpuMs) PT_CHECK_HIP(c, hipEventRecord(c->taauBloomEvents[0], st));
    if (skipped) PT_CHECK_HIP(c, hipMemcpyAsync(c->dTaauBloom.p, src, N * sizeof(ptk::float4), hipMemcpyDeviceToDevice, st));      // the source's bytes
    else launch_bloom(src, c->dTaauBloomQ[0].p, c->dTaauBloomQ[1].p, c->dTaauBloom.p, K, params->intensity, params->maxRadiance, W, H, st);
    if (gpuMs) PT_CHECK_HIP(c, hipEventRecord(c->taauBloomEvents[1], st));
    PT_CHECK_HIP(c, hipStreamSynchronize(st)); PT_CHECK_HIP(c, hipGetLastError());
    if (gpuMs) PT_CHECK_HIP(c, hipEventElapsedTime(gpuMs, c->taauBloomEvents[0], c->taauBloomEvents[1]));
    c->taauBloomReady = true;
    return PT_OK;
}

int32_t pt_tonemap_upscaled(pt_context* c, const PtToneMapParams* params, uint32_t bloomed, uint8_t* rgba8, size_t bytes) {
    if (!c || !params || !rgba8) return PT_ERROR_INVALID_ARGUMENT;
    const ptk::float4* src; int32_t r = picture(c, bloomed, &src); if (r != PT_OK) return r;
    const size_t n = (size_t)c->taauW * c->taauH;
    if (bytes < n * 4) return fail(c, PT_ERROR_INVALID_ARGUMENT, "rgba8 buffer too small");
    if (params->toneMapOperator > 5u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "unknown tone map operator");
    (void)hipSetDevice(c->device);
    static_assert(sizeof(PtToneMapParams) == sizeof(ptk::ToneMapParams), "tone map parameter layout");
    ptk::ToneMapParams p; memcpy(&p, params, sizeof(p));
    DevBuf<uint> d; PT_CHECK_HIP(c, d.resize(n));
    launch_tonemap(src, (uint)n, p, d.p, c->stream);      // pt_tonemap's kernel, pointed at the display-size picture
    PT_CHECK_HIP(c, hipMemcpyAsync(rgba8, d.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipGetLastError());
    d.free();
    return PT_OK;
}

int32_t pt_average_luminance_upscaled(pt_context* c, uint32_t bloomed, float* avgLuminance) {
    if (!c || !avgLuminance) return PT_ERROR_INVALID_ARGUMENT;
    const ptk::float4* src; int32_t r = picture(c, bloomed, &src); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)ptk::tm_pow2_floor(c->taauW) * ptk::tm_pow2_floor(c->taauH);
    DevBuf<float> d; PT_CHECK_HIP(c, d.resize(2 * n));
    float* result = nullptr; float logLum = 0.f;
    launch_average_log_luminance(src, c->taauW, c->taauH, d.p, &result, c->stream);      // pt_average_luminance's kernels, pointed at the display-size picture
    PT_CHECK_HIP(c, hipMemcpyAsync(&logLum, result, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipGetLastError());
    d.free();
    *avgLuminance = exp2f(logLum);                      // ToneMappingPasses.cpp:284
    return PT_OK;
}

int32_t pt_upscale_tex_lod_bias(uint32_t renderW, uint32_t renderH, uint32_t displayW, uint32_t displayH, float* bias) {
    if (!bias || !renderW || !renderH || !displayW || !displayH) return PT_ERROR_INVALID_ARGUMENT;
    *bias = -log2f(sqrtf((displayW * displayH) / float(renderW * renderH)));      // Sample.cpp:1504, the products in uint32_t as there
    return PT_OK;
}

}

// mi355pt — the reference-mode denoiser's entry points (include/mi355pt.h: pt_accum_denoise_default_params, pt_accum_denoise, pt_accum_denoise_host_inputs,
// pt_accum_denoised_device_buffer, pt_get_accum_denoised, pt_get_accum_denoise_state; the display tail on the denoised picture — pt_tonemap_accum_denoised and
// pt_average_luminance_accum_denoised in pt_display.hip, pt_bloom_accum_denoised in pt_bloom_api.hip — goes over view_accum_denoised): the host side of pt_accum_denoise.h /
// pt_accum_denoise.hip. The context keeps a picture of its own for the result and the three buffers the prepare launch writes; the
// radiance buffer, the even-sample buffer and the counts are only read. Both calls run the same two launches; they differ in where A and H come from.
#include <cmath>
#include <cstring>
#include <vector>
#include "pt_display.h"
#include "pt_accum_denoise.h"

using namespace ptk;

void accum_denoise_drop(pt_context* c) { c->accumDenoise.ready = false; }
void accum_denoise_free(pt_context* c) {
    pt_context::AccumDenoise& D = c->accumDenoise;
    D.dOut.free(); D.dStageH.free(); D.dStageO.free(); D.dVar.free(); D.dInA.free(); D.dInH.free();
    D.events.destroy(); D.w = D.h = 0; accum_denoise_drop(c);
}

int32_t view_accum_denoised(pt_context* c, PictureView* v) {
    const pt_context::AccumDenoise& D = c->accumDenoise;
    if (!D.ready || D.w != c->width || D.h != c->height) return fail(c, PT_ERROR_NOT_READY, "no denoised picture of this accumulation yet: pt_accum_denoise");
    *v = {D.dOut.p, D.w, D.h};
    return PT_OK;
}

namespace {
bool params_ok(const PtAccumDenoiseParams& p) {      // (every comparison is false for a NaN)
    return p.searchRadius >= 1u && p.searchRadius <= (uint)kAccumDenoiseMaxSearch && p.patchRadius <= (uint)kAccumDenoiseMaxPatch && p.k >= 0.05f && p.k <= 4.0f &&
           p.alpha >= 0.0f && p.alpha <= 4.0f && p.epsilon >= 1e-20f && p.epsilon <= 1.0f && p.maxRadiance > 0.0f && p.maxRadiance <= 1e15f;
}
// the two launches over A and H (device pictures of the frame size), timed if asked
int32_t run(pt_context* c, const PtAccumDenoiseParams& p, const ptk::float4* A, const ptk::float4* H, float* gpuMs) {
    pt_context::AccumDenoise& D = c->accumDenoise;
    const size_t N = (size_t)c->width * c->height;
    if (gpuMs) PT_CHECK_HIP(c, D.events.create());
    // the previous picture is given up only here, after the last host step that can fail without touching it
    accum_denoise_drop(c); D.w = c->width; D.h = c->height;
    PT_CHECK_HIP(c, D.dOut.resize(N)); PT_CHECK_HIP(c, D.dStageH.resize(N)); PT_CHECK_HIP(c, D.dStageO.resize(N)); PT_CHECK_HIP(c, D.dVar.resize(N));
    AccumDenoiseArgs a;
    a.A = A; a.H = H; a.stageH = D.dStageH.p; a.stageO = D.dStageO.p; a.var = D.dVar.p; a.out = D.dOut.p;
    a.width = (int)c->width; a.height = (int)c->height; a.r = (int)p.searchRadius; a.f = (int)p.patchRadius;
    a.kk = p.k * p.k; a.alpha = p.alpha; a.epsilon = p.epsilon; a.maxRadiance = p.maxRadiance;
    hipStream_t st = c->stream;
    PT_CHECK_HIP(c, D.events.begin(st, gpuMs != nullptr));
    PT_CHECK_HIP(c, launch_accum_denoise(a, st));
    PT_CHECK_HIP(c, D.events.end(st));
    PT_CHECK_HIP(c, hipStreamSynchronize(st)); PT_CHECK_HIP(c, hipGetLastError());
    PT_CHECK_HIP(c, D.events.read(gpuMs));
    D.ready = true;
    return PT_OK;
}
const char* kParamText = "denoiser parameters out of range (searchRadius 1 .. 8, patchRadius 0 .. 3, k in [0.05, 4], alpha in [0, 4], epsilon in [1e-20, 1], "
                         "maxRadiance in (0, 1e15], none a NaN)";
}

extern "C" {

int32_t pt_accum_denoise_default_params(PtAccumDenoiseParams* out) {
    if (!out) return PT_ERROR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->searchRadius = 5u; out->patchRadius = 2u; out->k = 0.45f; out->alpha = 1.0f; out->epsilon = 1e-10f; out->maxRadiance = 65504.0f;      // ours, unmeasured (include/mi355pt.h)
    return PT_OK;
}

int32_t pt_accum_denoise(pt_context* c, const PtAccumDenoiseParams* params, float* gpuMs) {
    if (!c || !params) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (!params_ok(*params)) return fail(c, PT_ERROR_INVALID_ARGUMENT, kParamText);
    if (c->shardCount > 1) return fail(c, PT_ERROR_UNSUPPORTED, "pt_accum_denoise reads a pixel's neighbours in both means, and the even-sample buffer is not gathered: "
                                                                "the context must own the whole frame (or pt_accum_denoise_host_inputs on gathered pictures)");
    // the two means are the last adaptive render's only while the accumulation is still that render's
    if (!c->adaptive.stateValid || !c->adaptive.perPixel) return fail(c, PT_ERROR_NOT_READY, "no adaptive render in the accumulation buffer: pt_render_adaptive");
    (void)hipSetDevice(c->device);
    return run(c, *params, c->dAccum.p, c->adaptive.dHalf.p, gpuMs);
}

int32_t pt_accum_denoise_host_inputs(pt_context* c, const PtAccumDenoiseParams* params, const float* meanRgba32f, const float* halfRgba32f, float* gpuMs) {
    if (!c || !params || !meanRgba32f || !halfRgba32f) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (!params_ok(*params)) return fail(c, PT_ERROR_INVALID_ARGUMENT, kParamText);
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    (void)hipSetDevice(c->device);
    pt_context::AccumDenoise& D = c->accumDenoise;
    const size_t N = (size_t)c->width * c->height;
    PT_CHECK_HIP(c, D.dInA.upload((const ptk::float4*)meanRgba32f, N, c->stream)); PT_CHECK_HIP(c, D.dInH.upload((const ptk::float4*)halfRgba32f, N, c->stream));
    return run(c, *params, D.dInA.p, D.dInH.p, gpuMs);      // (the stream orders the launches behind the copies; run() waits for it before returning)
}

int32_t pt_accum_denoised_device_buffer(pt_context* c, void** devicePtr, size_t* pitch) {
    if (!c || !devicePtr) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_accum_denoised(c, &v);
    return r != PT_OK ? r : display_device_buffer(v, devicePtr, pitch);
}

int32_t pt_get_accum_denoised(pt_context* c, float* rgba) {
    if (!c || !rgba) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_accum_denoised(c, &v);
    return r != PT_OK ? r : display_read_back(c, v, rgba, nullptr);
}

int32_t pt_get_accum_denoise_state(pt_context* c, float* oddRgb, float* variance, uint8_t* validMask) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_accum_denoised(c, &v); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    const pt_context::AccumDenoise& D = c->accumDenoise;
    const size_t N = (size_t)v.w * v.h;
    std::vector<ptk::float4> t(N);
    if (oddRgb) {
        PT_CHECK_HIP(c, hipMemcpy(t.data(), D.dStageO.p, 16u * N, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; i++) { oddRgb[3 * i] = t[i].x; oddRgb[3 * i + 1] = t[i].y; oddRgb[3 * i + 2] = t[i].z; }
    }
    if (variance) {
        PT_CHECK_HIP(c, hipMemcpy(t.data(), D.dVar.p, 16u * N, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; i++) { variance[3 * i] = t[i].x; variance[3 * i + 1] = t[i].y; variance[3 * i + 2] = t[i].z; }
    }
    if (validMask) {
        PT_CHECK_HIP(c, hipMemcpy(t.data(), D.dStageH.p, 16u * N, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; i++) validMask[i] = t[i].w != 0.0f ? 1u : 0u;
    }
    return PT_OK;
}

}

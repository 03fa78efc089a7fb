// mi355pt — the temporal anti-aliasing resolve's entry points (include/mi355pt.h: pt_taa_default_params, pt_taa_resolve, pt_resolved_device_buffer, pt_get_resolved,
// pt_taa_jitter; pt_tonemap_resolved is in pt_display.hip, over view_resolved): the host side of pt_taa.h / pt_taa.hip. The context keeps two RGBA32F buffers (the
// reference's TemporalFeedback1 / 2) and swaps them after every call: the one just written is the resolved picture (ProcessedOutputColor), the other one the history it
// was resolved against.
#include <cstring>
#include "pt_display.h"
#include "pt_taa.h"

using namespace ptk;

static_assert(sizeof(::PtTaaParams) == sizeof(ptk::TaaParams), "TAA parameter ABI");

void taa_drop_history(pt_context* c) { c->taaHistory = false; c->taaResolved = false; }
int32_t view_resolved(pt_context* c, PictureView* v) {
    if (!c->taaResolved || c->taaW != c->width || c->taaH != c->height) return fail(c, PT_ERROR_NOT_READY, "no resolved picture of this frame size yet: pt_taa_resolve");
    *v = {c->dTaa[c->taaSide].p, c->width, c->height};
    return PT_OK;
}
void taa_free(pt_context* c) {
    for (int s = 0; s < 2; s++) c->dTaa[s].free();
    c->taaEvents.destroy(); c->taaW = c->taaH = 0; taa_drop_history(c);
}

namespace {
bool params_ok(const PtTaaParams& p) {      // (every comparison is false for a NaN)
    return p.newFrameWeight > 0.0f && p.newFrameWeight <= 1.0f && p.clampingFactor >= 0.0f && p.clampingFactor <= kDenoiserViewZSkyMarker && p.maxRadiance > 0.0f && p.maxRadiance <= kDenoiserViewZSkyMarker;
}
// Halton's radical inverse of i in base b: the digits of i mirrored at the point, as one quotient of integers
double radical_inverse(unsigned long long i, uint32_t b) {
    unsigned long long num = 0, den = 1;
    for (; i; i /= b) { num = num * b + i % b; den *= b; }
    return (double)num / (double)den;
}
}

extern "C" {

int32_t pt_taa_default_params(PtTaaParams* out) {
    if (!out) return PT_ERROR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->newFrameWeight = 0.1f; out->clampingFactor = 1.0f; out->maxRadiance = 10000.0f;                                        // SampleUI.cpp:1199; ours; ours
    out->enableHistoryClamping = 1u; out->useHistoryClampRelax = 1u; out->useCatmullRomFilter = 1u; out->luminanceWeighted = 1u;      // SampleUI.cpp:1198; :161; Sample.cpp:1311; ours
    return PT_OK;
}

int32_t pt_taa_resolve(pt_context* c, const PtTaaParams* params, uint32_t resetHistory, float* gpuMs) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (!params_ok(*params)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "TAA parameters out of range (newFrameWeight in (0, 1], clampingFactor >= 0, maxRadiance > 0, all finite)");
    int32_t r = dn_ready(c); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)c->width * c->height;
    if (c->taaW != c->width || c->taaH != c->height) { taa_drop_history(c); c->taaW = c->width; c->taaH = c->height; }
    for (int s = 0; s < 2; s++) PT_CHECK_HIP(c, c->dTaa[s].resize(N));
    TaaParams P; memcpy(&P, params, sizeof(P));
    // the history must be of this build pass (a second call on one frame) or of the one before: the rule of the denoiser's rxFrameSerial
    const bool hasHistory = c->taaHistory && !resetHistory && c->spFrameSerial - c->taaFrameSerial <= 1u;
    // CombinedHistoryClampRelax is this frame's only after an NRD prepare pass of this build pass
    const bool haveRelax = P.useHistoryClampRelax && c->dnW == c->width && c->dnH == c->height && c->dnW && c->dnNrdSerial == c->spFrameSerial;
    const uint side = c->taaSide ^ 1u;
    hipStream_t st = c->stream;
    PT_CHECK_HIP(c, c->taaEvents.begin(st, gpuMs != nullptr));
    launch_taa_resolve(c->dAccum.p, c->dSpMotion.p, haveRelax ? c->dDnHistoryClamp.p : nullptr, hasHistory ? c->dTaa[side ^ 1u].p : nullptr, c->dTaa[side].p, P, c->width, c->height, st);
    PT_CHECK_HIP(c, c->taaEvents.end(st));
    c->taaSide = side; c->taaHistory = true; c->taaResolved = true; c->taaFrameSerial = c->spFrameSerial;
    PT_CHECK_HIP(c, hipStreamSynchronize(st)); PT_CHECK_HIP(c, hipGetLastError());
    PT_CHECK_HIP(c, c->taaEvents.read(gpuMs));
    return PT_OK;
}

int32_t pt_resolved_device_buffer(pt_context* c, void** devicePtr, size_t* pitch) {
    if (!c || !devicePtr) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_resolved(c, &v);
    return r != PT_OK ? r : display_device_buffer(v, devicePtr, pitch);
}

int32_t pt_get_resolved(pt_context* c, float* rgba) {
    if (!c || !rgba) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_resolved(c, &v);
    return r != PT_OK ? r : display_read_back(c, v, rgba, nullptr);
}

int32_t pt_taa_jitter(uint32_t sequence, uint32_t frameIndex, float offset[2]) {
    if (!offset) return PT_ERROR_INVALID_ARGUMENT;
    const unsigned long long i = (unsigned long long)frameIndex + 1u;
    if (sequence == 1u) {           // Halton, bases 2 and 3
        offset[0] = (float)(radical_inverse(i, 2u) - 0.5); offset[1] = (float)(radical_inverse(i, 3u) - 0.5);
    } else if (sequence == 2u) {    // R2: the plastic number's powers 1 / g, 1 / g^2
        const double a[2] = {0.7548776662466927, 0.5698402909980532};
        for (int k = 0; k < 2; k++) { const double v = 0.5 + (double)i * a[k]; offset[k] = (float)((v - floor(v)) - 0.5); }
    } else return PT_ERROR_INVALID_ARGUMENT;      // 0 (MSAA) and 3 (white noise): Donut's sample table and generator are not in the reference tree
    // (a double just below 0.5 can round up to the float 0.5: the largest float below it keeps the interval half open)
    for (int k = 0; k < 2; k++) if (offset[k] >= 0.5f) offset[k] = 0.49999997f;
    return PT_OK;
}

}

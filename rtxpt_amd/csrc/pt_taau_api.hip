// mi355pt — the temporal upscaling resolve's entry points (include/mi355pt.h: pt_taa_upscale_default_params, pt_taa_upscale, pt_upscaled_size, pt_upscaled_device_buffer,
// pt_get_upscaled, pt_get_upscaled_bloomed, pt_upscale_tex_lod_bias): the host side of pt_taau.h / pt_taau.hip. The context keeps two display-size RGBA32F buffers that swap
// after every call, as pt_taa_resolve's do — the one just written is the upscaled picture, the other one the history it was resolved against — and a display-size bloomed
// picture (taauBloom). None of them is one of pt_taa_resolve's or pt_bloom's buffers, and neither those nor the radiance buffer are written here. The tail behind it —
// pt_bloom_upscaled (pt_bloom_api.hip), pt_tonemap_upscaled and pt_average_luminance_upscaled (pt_display.hip) — runs the existing passes over view_upscaled.
#include <cmath>
#include <cstring>
#include "pt_display.h"
#include "pt_taau.h"

using namespace ptk;

static_assert(sizeof(::PtTaaUpscaleParams) == sizeof(ptk::TaauParams), "upscaling resolve parameter ABI");

void taau_drop_history(pt_context* c) { c->taauHistory = false; c->taauResolved = false; c->taauBloom.ready = false; }
void taau_free(pt_context* c) {
    for (int s = 0; s < 2; s++) c->dTaau[s].free();
    c->taauEvents.destroy(); c->taauBloom.free();
    c->taauW = c->taauH = c->taauRenderW = c->taauRenderH = 0; taau_drop_history(c);
}

namespace {
bool params_ok(const PtTaaUpscaleParams& p) {      // (every comparison is false for a NaN)
    const PtTaaParams& t = p.taa;
    return t.newFrameWeight > 0.0f && t.newFrameWeight <= 1.0f && t.clampingFactor >= 0.0f && t.clampingFactor <= kDenoiserViewZSkyMarker && t.maxRadiance > 0.0f && t.maxRadiance <= kDenoiserViewZSkyMarker &&
           p.kernelRadius >= 1.0f && p.kernelRadius <= 2.0f;
}
int32_t upscaled_ready(pt_context* c) {
    if (!c->taauResolved || c->taauRenderW != c->width || c->taauRenderH != c->height) return fail(c, PT_ERROR_NOT_READY, "no upscaled picture of this frame size yet: pt_taa_upscale");
    return PT_OK;
}
int32_t get_picture(pt_context* c, uint32_t bloomed, float* rgba, size_t floats) {
    if (!c || !rgba) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_upscaled(c, bloomed, &v);
    return r != PT_OK ? r : display_read_back(c, v, rgba, &floats);
}
}

// picture 0: the upscaled picture; 1: its bloom
int32_t view_upscaled(pt_context* c, uint32_t bloomed, PictureView* v) {
    if (bloomed > 1u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bloomed: 0 (the upscaled picture) or 1 (its bloom)");
    int32_t r = upscaled_ready(c); if (r != PT_OK) return r;
    if (bloomed && !c->taauBloom.ready) return fail(c, PT_ERROR_NOT_READY, "no bloomed upscaled picture yet: pt_bloom_upscaled");
    *v = {bloomed ? c->taauBloom.out.p : c->dTaau[c->taauSide].p, c->taauW, c->taauH};
    return PT_OK;
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
    if (gpuMs) PT_CHECK_HIP(c, c->taauEvents.create());
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
    PT_CHECK_HIP(c, c->taauEvents.begin(st, gpuMs != nullptr));
    launch_taa_upscale(c->dAccum.p, c->dSpMotion.p, haveRelax ? c->dDnHistoryClamp.p : nullptr, hasHistory ? c->dTaau[side ^ 1u].p : nullptr, c->dTaau[side].p, P, F, st);
    PT_CHECK_HIP(c, c->taauEvents.end(st));
    c->taauSide = side; c->taauHistory = true; c->taauResolved = true; c->taauBloom.ready = false; c->taauFrameSerial = c->spFrameSerial;
    PT_CHECK_HIP(c, hipStreamSynchronize(st)); PT_CHECK_HIP(c, hipGetLastError());
    PT_CHECK_HIP(c, c->taauEvents.read(gpuMs));
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
    PictureView v; int32_t r = view_upscaled(c, 0u, &v);
    return r != PT_OK ? r : display_device_buffer(v, devicePtr, pitch);
}

int32_t pt_get_upscaled(pt_context* c, float* rgba, size_t floats) { return get_picture(c, 0u, rgba, floats); }
int32_t pt_get_upscaled_bloomed(pt_context* c, float* rgba, size_t floats) { return get_picture(c, 1u, rgba, floats); }

int32_t pt_upscale_tex_lod_bias(uint32_t renderW, uint32_t renderH, uint32_t displayW, uint32_t displayH, float* bias) {
    if (!bias || !renderW || !renderH || !displayW || !displayH) return PT_ERROR_INVALID_ARGUMENT;
    *bias = -log2f(sqrtf((displayW * displayH) / float(renderW * renderH)));      // Sample.cpp:1504, the products in uint32_t as there
    return PT_OK;
}

}

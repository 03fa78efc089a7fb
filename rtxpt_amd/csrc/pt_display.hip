// mi355pt — the display tail (include/mi355pt.h: pt_tonemap, pt_tonemap_resolved, pt_tonemap_bloomed, pt_tonemap_upscaled, pt_tonemap_accum_denoised, pt_average_luminance,
// pt_average_luminance_bloomed, pt_average_luminance_upscaled, pt_average_luminance_accum_denoised): the tone-map and luminance kernels, the four bodies over a picture view
// (pt_display.h) that every picture's tail goes through, and the entry points that are nothing but a resolver and one of them.
#include <cmath>
#include <cstring>
#include "pt_display.h"

namespace ptk {

// ToneMappingPass::Render + SRGBA8 store (ToneMapping.ps.hlsli:136-174): one thread per pixel, streaming 16 B in / 4 B out
__global__ void __launch_bounds__(256) k_tonemap(const float4* __restrict__ accum, uint num, ToneMapParams p, uint* __restrict__ out) {
    uint i = blockIdx.x * 256u + threadIdx.x;
    if (i < num) out[i] = tm_pixel(p, accum[i]);
}
void launch_tonemap(const float4* accum, uint num, const ToneMapParams& p, uint* outRgba8, hipStream_t st) {
    hipLaunchKernelGGL(k_tonemap, dim3((num + 255) / 256), dim3(256), 0, st, accum, num, p, outRgba8);
}
// auto-exposure luminance capture: log-luminance target, then its mip chain down to 1x1 (ping-pong between the two halves of `scratch`)
__global__ void __launch_bounds__(256) k_log_luminance(const float4* __restrict__ accum, uint W, uint H, uint LW, uint LH, float* __restrict__ out) {
    uint i = blockIdx.x * 256u + threadIdx.x;
    if (i < LW * LH) out[i] = tm_log_luminance_texel(accum, W, H, LW, LH, i % LW, i / LW);
}
__global__ void __launch_bounds__(256) k_luminance_mip(const float* __restrict__ src, uint w, uint h, uint ow, uint oh, float* __restrict__ dst) {
    uint i = blockIdx.x * 256u + threadIdx.x;
    if (i < ow * oh) dst[i] = tm_mip_texel(src, w, h, i % ow, i / ow);
}
void launch_average_log_luminance(const float4* accum, uint W, uint H, float* scratch, float** result, hipStream_t st) {
    uint w = tm_pow2_floor(W), h = tm_pow2_floor(H);
    float* a = scratch; float* b = scratch + (size_t)w * h;
    hipLaunchKernelGGL(k_log_luminance, dim3((w * h + 255) / 256), dim3(256), 0, st, accum, W, H, w, h, a);
    while (w > 1u || h > 1u) {
        uint ow = w > 1u ? w / 2u : 1u, oh = h > 1u ? h / 2u : 1u;
        hipLaunchKernelGGL(k_luminance_mip, dim3((ow * oh + 255) / 256), dim3(256), 0, st, a, w, h, ow, oh, b);
        float* t = a; a = b; b = t; w = ow; h = oh;
    }
    *result = a;
}

} // namespace ptk

namespace {
// a call's scratch allocation, freed on every way out of the call (DevBuf itself has no destructor: the context's members rely on that)
template <typename T> struct Scratch : DevBuf<T> { ~Scratch() { this->free(); } };
}

int32_t view_radiance(pt_context* c, PictureView* v) {
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    *v = {c->dAccum.p, c->width, c->height};
    return PT_OK;
}

int32_t display_tonemap(pt_context* c, const PictureView& v, const PtToneMapParams* params, uint8_t* rgba8, size_t bytes) {
    const size_t n = (size_t)v.w * v.h;
    if (bytes < n * 4) return fail(c, PT_ERROR_INVALID_ARGUMENT, "rgba8 buffer too small");
    if (params->toneMapOperator > 5u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "unknown tone map operator");
    (void)hipSetDevice(c->device);
    static_assert(sizeof(PtToneMapParams) == sizeof(ptk::ToneMapParams), "tone map parameter layout");
    ptk::ToneMapParams p; memcpy(&p, params, sizeof(p));
    Scratch<uint> d; PT_CHECK_HIP(c, d.resize(n));
    launch_tonemap(v.p, (uint)n, p, d.p, c->stream);
    PT_CHECK_HIP(c, hipMemcpyAsync(rgba8, d.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}

int32_t display_average_luminance(pt_context* c, const PictureView& v, float* avgLuminance) {
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)ptk::tm_pow2_floor(v.w) * ptk::tm_pow2_floor(v.h);
    Scratch<float> d; PT_CHECK_HIP(c, d.resize(2 * n));
    float* result = nullptr; float logLum = 0.f;
    launch_average_log_luminance(v.p, v.w, v.h, d.p, &result, c->stream);
    PT_CHECK_HIP(c, hipMemcpyAsync(&logLum, result, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipGetLastError());
    *avgLuminance = exp2f(logLum);                      // ToneMappingPasses.cpp:284
    return PT_OK;
}

int32_t display_read_back(pt_context* c, const PictureView& v, float* rgba, const size_t* floats) {
    const size_t n = (size_t)v.w * v.h;
    if (floats && *floats < n * 4) return fail(c, PT_ERROR_INVALID_ARGUMENT, "rgba buffer too small");
    (void)hipSetDevice(c->device);
    PT_CHECK_HIP(c, hipMemcpy(rgba, v.p, 16u * n, hipMemcpyDeviceToHost));
    return PT_OK;
}

int32_t display_device_buffer(const PictureView& v, void** devicePtr, size_t* pitch) {
    *devicePtr = const_cast<ptk::float4*>(v.p); if (pitch) *pitch = (size_t)v.w * 16u;
    return PT_OK;
}

extern "C" {

int32_t pt_tonemap(pt_context* c, const PtToneMapParams* params, uint8_t* rgba8, size_t bytes) {
    if (!c || !params || !rgba8) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_radiance(c, &v);
    return r != PT_OK ? r : display_tonemap(c, v, params, rgba8, bytes);
}
int32_t pt_tonemap_resolved(pt_context* c, const PtToneMapParams* params, uint8_t* rgba8, size_t bytes) {
    if (!c || !params || !rgba8) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_resolved(c, &v);
    return r != PT_OK ? r : display_tonemap(c, v, params, rgba8, bytes);
}
int32_t pt_tonemap_bloomed(pt_context* c, const PtToneMapParams* params, uint8_t* rgba8, size_t bytes) {
    if (!c || !params || !rgba8) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_bloomed(c, &v);
    return r != PT_OK ? r : display_tonemap(c, v, params, rgba8, bytes);
}
int32_t pt_tonemap_upscaled(pt_context* c, const PtToneMapParams* params, uint32_t bloomed, uint8_t* rgba8, size_t bytes) {
    if (!c || !params || !rgba8) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_upscaled(c, bloomed, &v);
    return r != PT_OK ? r : display_tonemap(c, v, params, rgba8, bytes);
}
int32_t pt_tonemap_accum_denoised(pt_context* c, const PtToneMapParams* params, uint8_t* rgba8, size_t bytes) {
    if (!c || !params || !rgba8) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_accum_denoised(c, &v);
    return r != PT_OK ? r : display_tonemap(c, v, params, rgba8, bytes);
}

int32_t pt_average_luminance(pt_context* c, float* avgLuminance) {
    if (!c || !avgLuminance) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_radiance(c, &v);
    return r != PT_OK ? r : display_average_luminance(c, v, avgLuminance);
}
int32_t pt_average_luminance_bloomed(pt_context* c, float* avgLuminance) {
    if (!c || !avgLuminance) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_bloomed(c, &v);
    return r != PT_OK ? r : display_average_luminance(c, v, avgLuminance);
}
int32_t pt_average_luminance_upscaled(pt_context* c, uint32_t bloomed, float* avgLuminance) {
    if (!c || !avgLuminance) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_upscaled(c, bloomed, &v);
    return r != PT_OK ? r : display_average_luminance(c, v, avgLuminance);
}
int32_t pt_average_luminance_accum_denoised(pt_context* c, float* avgLuminance) {
    if (!c || !avgLuminance) return PT_ERROR_INVALID_ARGUMENT;
    PictureView v; int32_t r = view_accum_denoised(c, &v);
    return r != PT_OK ? r : display_average_luminance(c, v, avgLuminance);
}

}

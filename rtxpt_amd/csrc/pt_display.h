// mi355pt — the display tail (pt_display.hip): tone map, average luminance, read-back and device pointer over a picture view. Every picture a host can show — the radiance
// buffer, the resolved picture, the bloomed one, the upscaled one and its bloom, the denoised accumulation — goes through the same four bodies; what differs is the view.
#pragma once
#include "pt_context.h"
#include "pt_tonemap.h"

namespace ptk {
void launch_tonemap(const float4* accum, uint num, const ToneMapParams& p, uint* outRgba8, hipStream_t st);
// scratch: 2 * pow2floor(W) * pow2floor(H) floats; *result points at the 1x1 mip inside scratch once the stream has drained
void launch_average_log_luminance(const float4* accum, uint W, uint H, float* scratch, float** result, hipStream_t st);
}

#pragma GCC visibility push(hidden)

struct PictureView { const ptk::float4* p = nullptr; uint w = 0, h = 0; };      // w x h RGBA32F, rows packed

// One resolver per picture, in the file that owns its buffers: the picture's readiness check (PT_ERROR_NOT_READY with its text), then the view
int32_t view_radiance(pt_context* c, PictureView* v);                            // pt_display.hip
int32_t view_resolved(pt_context* c, PictureView* v);                            // pt_taa_api.hip
int32_t view_bloomed(pt_context* c, PictureView* v);                             // pt_bloom_api.hip
int32_t view_upscaled(pt_context* c, uint32_t bloomed, PictureView* v);          // pt_taau_api.hip: 0 the upscaled picture, 1 its bloom, else PT_ERROR_INVALID_ARGUMENT
int32_t view_accum_denoised(pt_context* c, PictureView* v);                      // pt_accum_denoise_api.hip

// The four bodies. The caller has checked its pointers and resolved the view.
int32_t display_tonemap(pt_context* c, const PictureView& v, const PtToneMapParams* params, uint8_t* rgba8, size_t bytes);
int32_t display_average_luminance(pt_context* c, const PictureView& v, float* avgLuminance);
// floats: the capacity of `rgba` where the entry point has one to check, else nullptr
int32_t display_read_back(pt_context* c, const PictureView& v, float* rgba, const size_t* floats);
int32_t display_device_buffer(const PictureView& v, void** devicePtr, size_t* pitch);

#pragma GCC visibility pop

// mi355pt — the temporal anti-aliasing resolve after the realtime merge (pt_taa_resolve): the seam of Sample::PostProcessAA (Sample.cpp:2621-2639), which sends OutputColor through
// TemporalAntiAliasingPass::TemporalResolve into ProcessedOutputColor with two feedback textures. The pass itself is Donut's and is not in the reference tree: the filter is our
// own (docs/WIDENING.md N6), not Donut's text, and is not compared with Donut's output; the parameter names and defaults that have a citation in include/mi355pt.h are the
// reference's. This file holds the per-pixel text; pt_taa.hip maps it onto waves.
// Part of the PRODUCT path (libmi355pt.so). Arithmetic contract of pt_vec.h, as pt_relax.h: one binary32 operation at a time in the written order, no contraction; only + - x /,
// sqrtf_, floorf, min / max / compare, so that tests/taa_ref.py restates every value bit for bit.
#pragma once
#include "pt_denoiser.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

// include/mi355pt.h PtTaaParams
struct TaaParams { float newFrameWeight, clampingFactor, maxRadiance; uint enableHistoryClamping, useHistoryClampRelax, useCatmullRomFilter, luminanceWeighted; };

static const float kTaaHistoryClampRelaxMul = 3.0f;      // CombinedHistoryClampRelax = 1 widens the box to clampingFactor x (1 + 3), as the denoiser's clamp (pt_relax.h)

// a component that is not finite counts as 0; then [0, maxRadiance]
static inline float TAA_Sanitise(float v, float maxRadiance) { return fminf_(fmaxf_(fabsf(v) <= kDenoiserViewZSkyMarker ? v : 0.0f, 0.0f), maxRadiance); }
// the staged record of a pixel: the sanitised colour, its luminance in .w
static inline float4 TAA_Colour(float4 v, float maxRadiance) {
    const float3 c = make_float3(TAA_Sanitise(v.x, maxRadiance), TAA_Sanitise(v.y, maxRadiance), TAA_Sanitise(v.z, maxRadiance));
    return make_float4(c, Luminance(c));
}
// the staged motion record: mv.xy in pixels, the squared length in .z
static inline float4 TAA_Motion(uint2 packed) { const float4 mv = SP_UnpackHalf4(packed); return make_float4(mv.x, mv.y, mv.x * mv.x + mv.y * mv.y, 0.0f); }
static inline int TAA_ClampCoord(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// the previous position of a pixel under motion vector mv; false: no history there (NaN, or outside [0, w] x [0, h])
static inline bool TAA_PreviousPosition(int x, int y, float mvx, float mvy, uint width, uint height, float& px, float& py) {
    px = ((float)x + 0.5f) + mvx; py = ((float)y + 0.5f) + mvy;
    return px >= 0.0f && px <= (float)width && py >= 0.0f && py <= (float)height;
}

// Catmull-Rom weights of the four taps at floor - 1 .. floor + 2 for the fraction t: plain weights, they sum to 1 and reproduce linear functions
static inline void TAA_CatmullRom(float t, float w[4]) {
    w[0] = t * (-0.5f + t * (1.0f - 0.5f * t));
    w[1] = 1.0f + (t * t) * (-2.5f + 1.5f * t);
    w[2] = t * (0.5f + t * (2.0f - 1.5f * t));
    w[3] = (t * t) * (-0.5f + 0.5f * t);
}
static inline float3 TAA_madd(float3 a, float4 v, float w) { return make_float3(a.x + v.x * w, a.y + v.y * w, a.z + v.z * w); }
static inline float3 TAA_madd(float3 a, float3 v, float w) { return make_float3(a.x + v.x * w, a.y + v.y * w, a.z + v.z * w); }

// the history at previous position (px, py) (pixel units, texel centres at + 0.5); tap coordinates clamped to the frame. Catmull-Rom: 4 x 4 texels, each row summed left to
// right from 0, then the four rows top to bottom from 0; bilinear: the 2 x 2 in the order (0, 0) (1, 0) (0, 1) (1, 1), summed from 0. The result is clamped to >= 0.
static inline float3 TAA_SampleHistory(const float4* __restrict__ hist, float px, float py, uint width, uint height, bool catmullRom) {
    const float fx = px - 0.5f, fy = py - 0.5f;
    const float flx = floorf(fx), fly = floorf(fy), tx = fx - flx, ty = fy - fly;
    const int ix = (int)flx, iy = (int)fly, w = (int)width, h = (int)height;
    float3 r = make_float3(0.0f);
    if (catmullRom) {
        float wx[4], wy[4]; TAA_CatmullRom(tx, wx); TAA_CatmullRom(ty, wy);
        int qx[4];
        #pragma unroll
        for (int i = 0; i < 4; i++) qx[i] = TAA_ClampCoord(ix - 1 + i, w);
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            const float4* __restrict__ row = hist + (size_t)TAA_ClampCoord(iy - 1 + j, h) * width;
            float3 s = make_float3(0.0f);
            #pragma unroll
            for (int i = 0; i < 4; i++) s = TAA_madd(s, row[qx[i]], wx[i]);
            r = TAA_madd(r, s, wy[j]);
        }
    } else {
        const float bw[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
        #pragma unroll
        for (int k = 0; k < 4; k++) r = TAA_madd(r, hist[(size_t)TAA_ClampCoord(iy + (k >> 1), h) * width + TAA_ClampCoord(ix + (k & 1), w)], bw[k]);
    }
    return make_float3(fmaxf_(r.x, 0.0f), fmaxf_(r.y, 0.0f), fmaxf_(r.z, 0.0f));
}

// the history into the current 3 x 3's mean +- k sigma per channel (sum, sum2 over the nine taps); relax: CombinedHistoryClampRelax of the pixel (0: not read)
static inline float3 TAA_ClampHistory(float3 hst, float3 sum, float3 sum2, float clampingFactor, float relax) {
    const float3 mean = make_float3(sum.x / 9.0f, sum.y / 9.0f, sum.z / 9.0f), m2 = make_float3(sum2.x / 9.0f, sum2.y / 9.0f, sum2.z / 9.0f);
    const float3 var = m2 - mean * mean;
    const float3 sigma = make_float3(sqrtf_(fmaxf_(var.x, 0.0f)), sqrtf_(fmaxf_(var.y, 0.0f)), sqrtf_(fmaxf_(var.z, 0.0f)));
    const float k = clampingFactor * (1.0f + kTaaHistoryClampRelaxMul * relax);
    const float3 lo = mean - sigma * k, hi = mean + sigma * k;
    return make_float3(fminf_(fmaxf_(hst.x, lo.x), hi.x), fminf_(fmaxf_(hst.y, lo.y), hi.y), fminf_(fmaxf_(hst.z, lo.z), hi.z));
}

// out = h + (c - h) x beta: c == h returns h exactly. beta: newFrameWeight, or with luminanceWeighted alpha w_c / (alpha w_c + (1 - alpha) w_h), w = 1 / (1 + Luminance)
static inline float3 TAA_Blend(float3 c, float lumC, float3 hst, const TaaParams& P) {
    float beta = P.newFrameWeight;
    if (P.luminanceWeighted) {
        const float wc = 1.0f / (1.0f + lumC), wh = 1.0f / (1.0f + Luminance(hst));
        const float a = P.newFrameWeight * wc, b = (1.0f - P.newFrameWeight) * wh;
        beta = a / (a + b);
    }
    return hst + (c - hst) * beta;
}

#pragma clang force_cuda_host_device end

// colour: the radiance buffer; motion: the build pass's motion vectors (4 halves a pixel); relax: R8_UNORM or nullptr (reads as 0); history: the previous resolve or nullptr
void launch_taa_resolve(const float4* colour, const uint2* motion, const unsigned char* relax, const float4* history, float4* out, const TaaParams& P, uint width, uint height, hipStream_t st);
} // namespace ptk

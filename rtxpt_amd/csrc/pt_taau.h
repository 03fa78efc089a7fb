// mi355pt — the temporal upscaling resolve (pt_taa_upscale): the radiance buffer and motion vectors of a frame traced at the render size w x h, resolved into a history and a
// result at a display size W x H, w <= W <= 4 w and h <= H <= 4 h. The reference's realtime mode renders at the upscaler's optimal size (Sample.cpp:1684-1776) and keeps the
// display size for everything after PostProcessAA (:1830, :2190); its upscaler is DLSS, which is not ours to run: the filter is our own (docs/WIDENING.md N8) and is not
// compared with anybody's output. It is pt_taa_resolve's filter (pt_taa.h: TAA_SampleHistory, TAA_ClampHistory, TAA_Blend are used, not restated) behind a jitter-aware
// resampling of the current frame: at ratio 1, jitter (0, 0) and kernelRadius 1 it IS pt_taa_resolve, bit for bit.
// This file holds the per-pixel text; pt_taau.hip maps it onto waves.
// Part of the PRODUCT path (libmi355pt.so). Arithmetic contract of pt_vec.h, as pt_taa.h: one binary32 operation at a time in the written order, no contraction; only + - x /,
// sqrtf_, floorf, min / max / compare, so that tests/taau_ref.py restates every value bit for bit.
#pragma once
#include "pt_taa.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

// include/mi355pt.h PtTaaUpscaleParams
struct TaauParams { TaaParams taa; float kernelRadius; uint confidenceWeighted; };

// a call's constants, computed once on the host (TAAU_MakeFrame): rx = w / W, sx = W / w, invR2 = 1 / (R R); jitter: the frame's camera offset in render pixels
struct TaauFrame { float rx, ry, sx, sy, invR2, jx, jy; uint width, height, displayWidth, displayHeight; };
static inline TaauFrame TAAU_MakeFrame(uint w, uint h, uint W, uint H, float jx, float jy, float R) {
    TaauFrame F;
    F.rx = (float)w / (float)W; F.ry = (float)h / (float)H; F.sx = (float)W / (float)w; F.sy = (float)H / (float)h; F.invR2 = 1.0f / (R * R);
    F.jx = jx; F.jy = jy; F.width = w; F.height = h; F.displayWidth = W; F.displayHeight = H;
    return F;
}

// Convention (pt_path.h computeCameraRay with cam.Jitter = (jx, -jy)): render pixel i of a frame traced with jitter j samples the screen at i + 0.5 - j, in render pixels.
// the centre of display pixel X in render pixels
static inline float TAAU_Centre(int X, float r) { return ((float)X + 0.5f) * r; }
// the render pixel whose sample is nearest to u: floor(u + j), clamped to the frame
static inline int TAAU_Nearest(float u, float j, int n) { return TAA_ClampCoord((int)floorf(u + j), n); }
// the signed distance from u to the sample of (unclamped) render pixel i
static inline float TAAU_Distance(int i, float j, float u) { return (((float)i + 0.5f) - j) - u; }
// the resampling weight of a tap at distance (ddx, ddy): a = max(1 - d^2 / R^2, 0), squared
static inline float TAAU_Weight(float ddx, float ddy, float invR2) { const float a = fmaxf_(1.0f - (ddx * ddx + ddy * ddy) * invR2, 0.0f); return a * a; }

// what the nine taps around the nearest sample accumulate, in scan-line order (dy outer, dx inner)
struct TaauTaps {
    float3 num, sum, sum2; float den, conf; float4 mv;
    // first: the motion record of the first tap, the longest vector so far
    inline void begin(float4 first) { num = sum = sum2 = make_float3(0.0f); den = 0.0f; conf = 0.0f; mv = first; }
    // c: the tap's staged colour record (clamped coordinate); m: its motion record; wk: its weight (unclamped distance)
    inline void tap(float4 c, float4 m, float wk) {
        num = num + xyz(c) * wk; den = den + wk; conf = fmaxf_(conf, wk);
        sum = sum + xyz(c); sum2 = sum2 + xyz(c) * xyz(c);
        if (m.z > mv.z) mv = m;
    }
    // with kernelRadius >= 1 the nearest tap lies within sqrt(0.5) of the centre: a >= 0.5, den >= 0.25
    inline float3 current() const { return make_float3(num.x / den, num.y / den, num.z / den); }
};

// the display pixel's result from its taps: cur without a history or with a previous position outside [0, W] x [0, H]; else pt_taa_resolve's sample, clamp and blend
// at the display size, the new-frame weight scaled by the best tap's weight when confidenceWeighted. relax: CombinedHistoryClampRelax at the nearest sample (0: not read)
static inline float3 TAAU_Resolve(const TaauTaps& T, int X, int Y, const float4* __restrict__ history, float relax, const TaauParams& P, const TaauFrame& F) {
    const float3 cur = T.current();
    float px, py;
    if (!history || !TAA_PreviousPosition(X, Y, T.mv.x * F.sx, T.mv.y * F.sy, F.displayWidth, F.displayHeight, px, py)) return cur;
    float3 hst = TAA_SampleHistory(history, px, py, F.displayWidth, F.displayHeight, P.taa.useCatmullRomFilter != 0u);
    if (P.taa.enableHistoryClamping) hst = TAA_ClampHistory(hst, T.sum, T.sum2, P.taa.clampingFactor, relax);
    TaaParams B = P.taa;
    if (P.confidenceWeighted) B.newFrameWeight = P.taa.newFrameWeight * T.conf;
    return TAA_Blend(cur, Luminance(cur), hst, B);
}

#pragma clang force_cuda_host_device end

// colour, motion, relax: at the render size F.width x F.height, as launch_taa_resolve takes them; history (or nullptr) and out: at the display size
void launch_taa_upscale(const float4* colour, const uint2* motion, const unsigned char* relax, const float4* history, float4* out, const TaauParams& P, const TaauFrame& F, hipStream_t st);
} // namespace ptk

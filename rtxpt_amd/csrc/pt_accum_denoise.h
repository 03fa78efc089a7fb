// mi355pt — the reference-mode denoiser (pt_accum_denoise; include/mi355pt.h, docs/WIDENING.md N13): a dual-buffer non-local-means filter (Rousselle, Knaus, Zwicker 2012)
// over what adaptive sampling leaves — the mean of a pixel's samples (A) and the mean of its even-indexed ones (H). The seam is the reference's "Photo mode screenshot"
// (SampleUI.cpp:926-932, Sample::DenoisedScreenshot, Sample.cpp:2782-2815), which hands the accumulated picture to an external tool; the filter is ours.
// This file holds the per-pixel text; pt_accum_denoise.hip maps it onto waves, pt_accum_denoise_api.hip holds the entry points.
// Part of the PRODUCT path (libmi355pt.so). Arithmetic contract of pt_vec.h: one binary32 operation at a time in the written order, no contraction; divide correctly rounded
// (the Makefile's flags), so that tests/accum_denoise_ref.py restates every value bit for bit. The order of the additions is part of the interface.
#pragma once
#include "pt_taa.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

static const int kAccumDenoiseTile = 16;            // a workgroup's tile: 16 x 16 pixels, one a lane
static const int kAccumDenoiseMaxSearch = 8, kAccumDenoiseMaxPatch = 3;

// the odd-sample mean of a channel: A is the mean of both halves
static inline float AD_Odd(float a, float h) { return (a + a) - h; }
// finite and within the radiance bound (false for a NaN)
static inline bool AD_InRange(float v, float maxRadiance) { return fabsf(v) <= maxRadiance; }
// a pixel's staged halves: H' and O' (both 0 for an invalid pixel); returns valid(p)
static inline bool AD_Stage(float4 A, float4 H, float maxRadiance, float3& Hs, float3& Os) {
    const float3 O = make_float3(AD_Odd(A.x, H.x), AD_Odd(A.y, H.y), AD_Odd(A.z, H.z));
    const bool valid = AD_InRange(A.x, maxRadiance) && AD_InRange(A.y, maxRadiance) && AD_InRange(A.z, maxRadiance) &&
                       AD_InRange(H.x, maxRadiance) && AD_InRange(H.y, maxRadiance) && AD_InRange(H.z, maxRadiance) &&
                       AD_InRange(O.x, maxRadiance) && AD_InRange(O.y, maxRadiance) && AD_InRange(O.z, maxRadiance);
    Hs = valid ? make_float3(H.x, H.y, H.z) : make_float3(0.0f);
    Os = valid ? O : make_float3(0.0f);
    return valid;
}
// s: the sample variance of the two halves of a channel, which is the variance of one half
static inline float AD_HalfVariance(float h, float o) { const float d = h - o; return (d * d) * 0.5f; }
static inline float3 AD_HalfVariance3(float4 A, float4 H, float maxRadiance) {
    float3 Hs, Os; (void)AD_Stage(A, H, maxRadiance, Hs, Os);
    return make_float3(AD_HalfVariance(Hs.x, Os.x), AD_HalfVariance(Hs.y, Os.y), AD_HalfVariance(Hs.z, Os.z));
}
// V: the 3 x 3 box mean of s, coordinates clamped; rows (s[x - 1] + s[x]) + s[x + 1], columns (row[y - 1] + row[y]) + row[y + 1], then / 9
static inline float3 AD_Variance(const float4* __restrict__ A, const float4* __restrict__ H, int x, int y, int width, int height, float maxRadiance) {
    float3 rows[3];
    #pragma unroll
    for (int j = 0; j < 3; j++) {
        const size_t row = (size_t)TAA_ClampCoord(y - 1 + j, height) * (size_t)width;
        float3 s[3];
        #pragma unroll
        for (int i = 0; i < 3; i++) { const size_t p = row + (size_t)TAA_ClampCoord(x - 1 + i, width); s[i] = AD_HalfVariance3(A[p], H[p], maxRadiance); }
        rows[j] = (s[0] + s[1]) + s[2];
    }
    const float3 c = (rows[0] + rows[1]) + rows[2];
    return make_float3(c.x / 9.0f, c.y / 9.0f, c.z / 9.0f);
}
// one channel of the distance of pixel x to x + o in buffer U: u, v at x and un, vn at x + o; kk = k x k
static inline float AD_Distance(float u, float un, float v, float vn, float alpha, float epsilon, float kk) {
    const float d = u - un;
    return ((d * d) - alpha * (v + fminf_(v, vn))) / (epsilon + kk * (v + vn));
}
// w from the patch sum S of e over (2f + 1)^2 pixels and three channels: a polynomial stand-in for exp(-D2). (D2 is never a NaN: V is finite and epsilon > 0, so e lies in
// [-alpha / kk, +inf].)
static inline float AD_Weight(float S, float norm) {
    const float D2 = S / norm;
    const float t = fmaxf_(1.0f - fmaxf_(D2, 0.0f) * 0.25f, 0.0f), t2 = t * t;
    return t2 * t2;
}
static inline float AD_PatchNorm(int f) { return (float)(3 * (2 * f + 1) * (2 * f + 1)); }

#pragma clang force_cuda_host_device end

// what a call hands to the launches. A, H: the two means [height][width]; stageH (H'.xyz, w = 1 for a valid pixel, else 0), stageO (O'.xyz, 0) and var (V.xyz, 0): the
// prepare launch's output and the filter's input; out: the denoised picture
struct AccumDenoiseArgs {
    const float4* A; const float4* H; float4* stageH; float4* stageO; float4* var; float4* out;
    int width, height, r, f; float kk, alpha, epsilon, maxRadiance;
};
// the filter launch's dynamic LDS [bytes] for search radius r and patch radius f
size_t accum_denoise_lds_bytes(int r, int f);
// two launches on st: prepare, filter
hipError_t launch_accum_denoise(const AccumDenoiseArgs& a, hipStream_t st);
} // namespace ptk

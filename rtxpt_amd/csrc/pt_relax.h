// mi355pt — the device denoiser between pt_denoiser_prepare_nrd and pt_denoiser_merge_nrd: a RELAX-shaped spatio-temporal filter of our own (docs/WIDENING.md N5), one plane per
// call, history per plane as Sample::Denoise keeps one NRD instance per plane (Sample.cpp:2585-2612). This file holds the per-pixel text; pt_relax.hip maps it onto waves.
// Part of the PRODUCT path (libmi355pt.so). Arithmetic contract of pt_vec.h, as pt_denoiser.h: one binary32 operation at a time in the written order, no contraction; weights are
// written with + - x /, sqrtf_, min / max / compare only, so that tests/relax_ref.py restates every value bit for bit. None of this is NRD's text: the settings' names and defaults
// are the reference's (NrdConfig.cpp:15-47, SampleUI.h:294-296), every formula is stated in docs/WIDENING.md.
#pragma once
#include "pt_denoiser.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

// include/mi355pt.h PtDenoiseSettings
struct RelaxSettings {
    uint atrousIterationNum; float depthThreshold, lobeAngleFraction;
    uint diffuseMaxAccumulatedFrameNum, specularMaxAccumulatedFrameNum, diffuseMaxFastAccumulatedFrameNum, specularMaxFastAccumulatedFrameNum, enableAntiFirefly;
    float disocclusionThreshold, disocclusionThresholdAlternate; uint useDisocclusionThresholdMix; float luminanceSigmaScale;
};
// one plane's history of one frame, five 16-byte records per pixel in scan-line order
struct RelaxHistory {
    float4* DiffLen;        // accumulated diffuse radiance, diffuse history length
    float4* SpecLen;        // accumulated specular radiance, specular history length
    float4* FastDiffM1;     // fast diffuse history, first diffuse luminance moment
    float4* FastSpecM1;     // fast specular history, first specular luminance moment
    float4* M2Guide;        // second moments (diffuse, specular), then the guides the history is tested against: viewZ, the packed normal
};

static const float kRelaxHistoryClampSigma = 2.0f;         // k of the fast-history clamp: mean +- k sigma
static const float kRelaxHistoryClampRelaxMul = 3.0f;      // CombinedHistoryClampRelax = 1 widens k to k x (1 + 3)
static const float kRelaxLumEps = 1e-6f;
static const float kRelaxSpatialVarianceBelow = 4.0f;      // fewer frames of history than this: the variance is the spatial 5 x 5 estimate
static const float kRelaxMaxReprojection = 32768.0f;       // a previous position further out than this (or NaN) has no history

// a radiance component that is not finite counts as 0 (the prepare pass divides by BSDF estimates that can be 0)
static inline float RX_finite0(float v) { return fabsf(v) <= kDenoiserViewZSkyMarker ? v : 0.0f; }
static inline float3 RX_finite0(float4 v) { return make_float3(RX_finite0(v.x), RX_finite0(v.y), RX_finite0(v.z)); }
static inline float3 RX_div(float3 v, float s) { return make_float3(v.x / s, v.y / s, v.z / s); }
static inline float4 RX_div(float4 v, float s) { return make_float4(v.x / s, v.y / s, v.z / s, v.w / s); }
static inline float4 RX_madd(float4 a, float4 v, float w) { return make_float4(a.x + v.x * w, a.y + v.y * w, a.z + v.z * w, a.w + v.w * w); }

// the 16-byte guide record of a pixel: viewZ (FLT_MAX: sky), the octahedral normal, roughness, the shorter of the two history lengths
static inline float4 RX_PackGuide(float viewZ, uint octNormal, float roughness, float length) { return make_float4(viewZ, asfloat(octNormal), roughness, length); }
static inline float4 RX_zn(float z, float3 n) { return make_float4(z, n.x, n.y, n.z); }
static inline float3 RX_GuideNormal(float4 g) { return OctToNDirUnorm32(asuint(g.y)); }
// the record as the passes use it: viewZ, then the decoded normal
static inline float4 RX_DecodeGuide(float4 g) { if (g.x == kDenoiserViewZSkyMarker) return make_float4(g.x, 0.0f, 0.0f, 0.0f); return RX_zn(g.x, RX_GuideNormal(g)); }
static inline float3 RX_yzw(float4 v) { return make_float3(v.y, v.z, v.w); }

// the relative disocclusion threshold of a pixel
static inline float RX_DisocclusionThreshold(const RelaxSettings& S, unsigned char mix) {
    return S.useDisocclusionThresholdMix ? lerpf(S.disocclusionThreshold, S.disocclusionThresholdAlternate, DN_LoadUnorm8(mix)) : S.disocclusionThreshold;
}
// the cone test: a normal is accepted with 1 - cos <= lobeAngleFraction x lobe; the diffuse lobe is the hemisphere (1), the specular one roughness x the hemisphere. The
// temporal pass and the anti-firefly use the diffuse cone (1 - lobeAngleFraction), the a-trous normal stops fall linearly from 1 at cos = 1 to 0 at the cone (RX_Centre)
// same surface: |viewZ| within thr of the expected one, relative to it, and the normal inside the diffuse cone
static inline bool RX_SameSurface(float expectedAbsZ, float3 n, float absZ, float3 nT, float thr, float coneCos) {
    return fabsf(absZ - expectedAbsZ) <= thr * expectedAbsZ && dot(n, nT) >= coneCos;
}
// anti-firefly: luminance clamped to the largest one among the valid neighbours, colour scaled with it
static inline float3 RX_ClampLuminance(float3 c, float lum, float maxLum) { return lum > maxLum ? c * (maxLum / lum) : c; }

// the temporal accumulation of one signal. h: the reprojected history (radiance + length), hf: the fast history + first moment, hm2: the second moment; valid: any valid tap
struct RelaxAccum { float3 acc, fast; float len, m1, m2; };
static inline RelaxAccum RX_Accumulate(bool valid, float3 c, float lum, float4 h, float4 hf, float hm2, uint maxFrames, uint maxFastFrames) {
    RelaxAccum r;
    if (!valid) { r.acc = c; r.fast = c; r.len = 1.0f; r.m1 = lum; r.m2 = lum * lum; return r; }
    r.len = fminf_(h.w + 1.0f, (float)maxFrames);
    const float alpha = 1.0f / r.len, alphaFast = 1.0f / fminf_(r.len, (float)maxFastFrames);
    r.acc = xyz(h) + (c - xyz(h)) * alpha;
    r.fast = xyz(hf) + (c - xyz(hf)) * alphaFast;
    r.m1 = hf.w + (lum - hf.w) * alpha;
    r.m2 = hm2 + (lum * lum - hm2) * alpha;
    return r;
}

// the fast-history clamp of one signal over the n valid taps of a 3 x 3 (sum, sum2: per channel); relax: CombinedHistoryClampRelax of the pixel
static inline float3 RX_ClampToFast(float3 acc, float3 sum, float3 sum2, float n, float relax) {
    const float3 mean = RX_div(sum, n), m2 = RX_div(sum2, n);
    const float3 var = m2 - mean * mean;
    const float3 sigma = make_float3(sqrtf_(fmaxf_(var.x, 0.0f)), sqrtf_(fmaxf_(var.y, 0.0f)), sqrtf_(fmaxf_(var.z, 0.0f)));
    const float k = kRelaxHistoryClampSigma + relax * (kRelaxHistoryClampSigma * kRelaxHistoryClampRelaxMul);
    const float3 lo = mean - sigma * k, hi = mean + sigma * k;
    return make_float3(fminf_(fmaxf_(acc.x, lo.x), hi.x), fminf_(fmaxf_(acc.y, lo.y), hi.y), fminf_(fmaxf_(acc.z, lo.z), hi.z));
}

// ---- the a-trous pass. B3 row (1, 4, 6, 4, 1) / 16 by |offset|
static inline float RX_B3(int o) { o = o < 0 ? -o : o; return o == 0 ? 0.375f : (o == 1 ? 0.25f : 0.0625f); }

// what a pixel's filter needs of its centre
struct RelaxCentre {
    float absZ, invDepth; float3 n; float coneDiff, invConeDiff, coneSpec, invConeSpec; float lumDiff, lumSpec, varDiff, varSpec, invSigmaDiff, invSigmaSpec; bool lumStop;      // (the stops' denominators as reciprocals: one division per centre, none per tap)
};
static inline RelaxCentre RX_Centre(const RelaxSettings& S, float4 g /* viewZ, normal */, float roughness, float4 d, float4 s) {
    RelaxCentre C;
    C.absZ = fabsf(g.x); C.invDepth = 1.0f / fmaxf_(S.depthThreshold * C.absZ, 1e-20f); C.n = RX_yzw(g);
    const float lobeSpec = S.lobeAngleFraction * roughness;
    C.coneDiff = 1.0f - S.lobeAngleFraction; C.invConeDiff = 1.0f / fmaxf_(S.lobeAngleFraction, 1e-6f);
    C.coneSpec = 1.0f - lobeSpec; C.invConeSpec = 1.0f / fmaxf_(lobeSpec, 1e-6f);
    C.lumDiff = Luminance(xyz(d)); C.lumSpec = Luminance(xyz(s)); C.varDiff = d.w; C.varSpec = s.w; C.lumStop = S.luminanceSigmaScale > 0.0f;
    C.invSigmaDiff = C.invSigmaSpec = 1.0f;
    return C;
}
static inline void RX_CentreSigma(const RelaxSettings& S, RelaxCentre& C) {
    C.invSigmaDiff = 1.0f / (S.luminanceSigmaScale * sqrtf_(fmaxf_(C.varDiff, 0.0f)) + kRelaxLumEps);
    C.invSigmaSpec = 1.0f / (S.luminanceSigmaScale * sqrtf_(fmaxf_(C.varSpec, 0.0f)) + kRelaxLumEps);
}
// the geometry weights of a tap: B3 x depth stop, then the two normal stops. The centre tap is its own surface: its stops are 1 by definition, so the weight sums are never 0
// whatever the roughness (the prepare pass floors it at 0.2; a roughness of 0 makes the specular cone a single direction, which a decoded normal's n . n = 1 - ulp would miss)
static inline void RX_GeometryWeights(const RelaxCentre& C, float b, bool centre, float4 gT, float& wDiff, float& wSpec) {
    if (centre) { wDiff = b; wSpec = b; return; }
    const float wz = saturate(1.0f - fabsf(fabsf(gT.x) - C.absZ) * C.invDepth);
    const float dn = dot(C.n, RX_yzw(gT));
    const float g = b * wz;
    wDiff = g * saturate((dn - C.coneDiff) * C.invConeDiff);
    wSpec = g * saturate((dn - C.coneSpec) * C.invConeSpec);
}
// the spatial variance estimate of the first iteration (history shorter than kRelaxSpatialVarianceBelow): luminance moments under the diffuse geometry weights
struct RelaxEstimate { float w, d1, d2, s1, s2; };
static inline void RX_EstimateTap(const RelaxCentre& C, float b, bool centre, float4 gT, float4 dT, float4 sT, RelaxEstimate& E) {
    float wd, ws; RX_GeometryWeights(C, b, centre, gT, wd, ws);
    const float ld = Luminance(xyz(dT)), ls = Luminance(xyz(sT));
    E.w = E.w + wd; E.d1 = E.d1 + wd * ld; E.d2 = E.d2 + wd * (ld * ld); E.s1 = E.s1 + wd * ls; E.s2 = E.s2 + wd * (ls * ls);
}
static inline void RX_EstimateResolve(const RelaxEstimate& E, RelaxCentre& C) {
    const float d1 = E.d1 / E.w, d2 = E.d2 / E.w, s1 = E.s1 / E.w, s2 = E.s2 / E.w;
    C.varDiff = fmaxf_(d2 - d1 * d1, 0.0f); C.varSpec = fmaxf_(s2 - s1 * s1, 0.0f);
}
struct RelaxSums { float3 d, s; float vd, vs, wd, ws; };
static inline void RX_FilterTap(const RelaxCentre& C, float b, bool centre, float4 gT, float4 dT, float4 sT, RelaxSums& A) {
    float wd, ws; RX_GeometryWeights(C, b, centre, gT, wd, ws);
    if (C.lumStop) {
        wd = wd * saturate(1.0f - fabsf(Luminance(xyz(dT)) - C.lumDiff) * C.invSigmaDiff);
        ws = ws * saturate(1.0f - fabsf(Luminance(xyz(sT)) - C.lumSpec) * C.invSigmaSpec);
    }
    A.d = A.d + xyz(dT) * wd; A.s = A.s + xyz(sT) * ws;
    A.vd = A.vd + (wd * wd) * (centre ? C.varDiff : dT.w); A.vs = A.vs + (ws * ws) * (centre ? C.varSpec : sT.w);
    A.wd = A.wd + wd; A.ws = A.ws + ws;
}
static inline float4 RX_FilterResolve(float3 sum, float v, float w) { return make_float4(RX_div(sum, w), v / (w * w)); }

#pragma clang force_cuda_host_device end

// what the three passes of a plane share: the prepare pass's buffers, the guide records, the two ping-pong pairs (radiance + variance), the plane's two denoised buffers
struct RelaxPassBuffers { float4* Guide; float4* PingDiff; float4* PingSpec; float4* PongDiff; float4* PongSpec; float4* OutDiff; float4* OutSpec; };

void launch_relax_temporal(const DenoiserBuffers& D, const RelaxSettings& S, const RelaxHistory& prev, const RelaxHistory& cur, float4* guide, uint width, uint height, bool hasHistory, hipStream_t st);
void launch_relax_clamp(const DenoiserBuffers& D, const RelaxSettings& S, const RelaxHistory& cur, const float4* guide, float4* outDiff, float4* outSpec, uint width, uint height, hipStream_t st);
// iteration `iteration` (step 1 << iteration); last: the result goes out as the denoised radiance (.w: 0 for diffuse, the prepare pass's hit distance for specular)
void launch_relax_atrous(const DenoiserBuffers& D, const RelaxSettings& S, const float4* guide, const float4* inDiff, const float4* inSpec, float4* outDiff, float4* outSpec, uint iteration, bool last,
                         uint width, uint height, hipStream_t st);
} // namespace ptk

// mi355pt — the denoiser's side of a realtime stable-plane frame: the inputs a denoiser reads and the merge of its outputs (DESIGN.md "What comes next" 5, docs/WIDENING.md N4).
// Part of the PRODUCT path (libmi355pt.so). Written to the arithmetic contract stated in pt_vec.h: one binary32 operation at a time in the written order, no contraction, fp16 by
// software round-to-nearest-even. Reference anchors (paths relative to /root/reference/Rtxpt/):
//   ProcessingPasses/PostProcess.hlsl:60-84      ComputeNeighbourDisocclusionRelaxation, ComputeDisocclusionRelaxation
//   ProcessingPasses/PostProcess.hlsl:94-159     ComputeSpecularMotionVector
//   ProcessingPasses/PostProcess.hlsl:161-173    NRDRadianceClamp
//   ProcessingPasses/PostProcess.hlsl:198-440    DENOISER_PREPARE_INPUTS + DENOISER_DLSS_RR (Sample.cpp:2712-2719)
//   ProcessingPasses/PostProcess.hlsl:442-573    DENOISER_PREPARE_INPUTS for NRD, one plane per dispatch (Sample.cpp:2561-2619)
//   ProcessingPasses/PostProcess.hlsl:577-690    DENOISER_FINAL_MERGE, with NRD/DenoiserNRD.hlsli:24-48 PostDenoiseProcess after the host's unpack
//   Shaders/PathTracer/StablePlanes.hlsli:65-72  StablePlane::GetNormal / GetRoughness / GetNoisyRadiance / GetNoisyDiffRadiance / GetNoisySpecRadiance
// NRD's own packing (NRD_FrontEnd_PackNormalAndRoughness, RELAX_ / REBLUR_FrontEnd_*) and unpacking belong to the denoiser the host brings: the prepare pass stores the exact fp32
// arguments the text hands to those functions, and the merge takes the host's unpacked radiance.
#pragma once
#include "pt_stableplanes_launch.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

// what the host sets per frame besides PtStablePlanesParams (Sample.cpp:1509-1540; include/mi355pt.h PtDenoiserParams)
struct DenoiserParams {
    float matWorldToView[16];                              // donut PlanarViewConstants::matWorldToView, row-major for row vectors (the NRD viewZ)
    float preExposedGrayLuminance;                         // ptConsts.preExposedGrayLuminance
    float denoiserRadianceClampK;                          // ptConsts.denoiserRadianceClampK (UI default 8)
    float DLSSRRBrightnessClampK;                          // ptConsts.DLSSRRBrightnessClampK, already multiplied by the grey luminance (Sample.cpp:1526)
    float stablePlanesSuppressPrimaryIndirectSpecularK;    // ptConsts.stablePlanesSuppressPrimaryIndirectSpecularK (0.6 on, 0 off: Sample.cpp:1536)
};

// the buffers of the two prepare passes, each imageWidth x imageHeight in scan-line order (RenderTargets.cpp:160-190)
struct DenoiserBuffers {
    uint* RRDiffuseAlbedo; uint* RRSpecAlbedo; uint2* RRNormalsAndRoughness; uint* RRSpecMotionVectors;      // R11G11B10F, R11G11B10F, RGBA16F, RG16F
    float* ViewZ; uint2* MotionVectors; float4* NormalRoughness; float4* DiffRadianceHitDist; float4* SpecRadianceHitDist; float* Roughness;      // NRD: R32F, RGBA16F, then the fp32 front-end arguments
    unsigned char* DisocclusionThresholdMix; unsigned char* CombinedHistoryClampRelax;      // R8_UNORM (RenderTargets.cpp:177-182)
};

static const float kDenoiserViewZSkyMarker = 3.402823466e+38f;      // PostProcess.hlsl:18 VIEWZ_SKY_MARKER = FLT_MAX

// R8_UNORM store and load. The rounding of the reference's store is the hardware's; here it is clamp to [0, 1] (NaN -> 0), x 255, round to nearest, ties to even.
static inline unsigned char DN_StoreUnorm8(float v) { return (unsigned char)(uint)rintf(saturate(v) * 255.0f); }
static inline float DN_LoadUnorm8(unsigned char q) { return (float)(uint)q / 255.0f; }
// HLSL max(0, v) as IEEE maxNum: a NaN operand yields the other one
static inline float DN_max0(float v) { return v > 0.0f ? v : 0.0f; }
static inline float DN_max3(float3 v) { return fmaxf_(fmaxf_(v.x, v.y), v.z); }      // ColorHelpers.hlsli:19-27 max3 = max(max(a, b), c)
static inline float3 DN_reflect(float3 i, float3 n) { const float d2 = 2.0f * dot(i, n); return i - n * d2; }      // HLSL reflect: i - 2 * dot(i, n) * n

// StablePlanes.hlsli:65-72 on a record
static inline float3 DN_GetNormal(const StablePlane& sp) { return OctToNDirUnorm32(sp.PackedNormal); }
static inline float DN_GetRoughness(const StablePlane& sp) { return f16tof32(sp.VertexIndexAndRoughness & 0xFFFFu); }
static inline float4 DN_GetNoisyRadianceAndSpecRA(const StablePlane& sp) {
    const float2 a = Fp16ToFp32(sp.PackedNoisyRadianceAndSpecAvg[0]), b = Fp16ToFp32(sp.PackedNoisyRadianceAndSpecAvg[1]); return make_float4(a.x, a.y, b.x, b.y);
}
static inline float3 DN_GetNoisyDiffRadiance(const StablePlane& sp) {
    const float4 l = DN_GetNoisyRadianceAndSpecRA(sp); const float totalAvg = Average(xyz(l));
    return xyz(l) * saturate(1.0f - (l.w * 1.0f) / (totalAvg + 1e-12f));      // kSpecHeuristicBoost = 1
}
static inline float3 DN_GetNoisySpecRadiance(const StablePlane& sp) {
    const float4 l = DN_GetNoisyRadianceAndSpecRA(sp); const float totalAvg = Average(xyz(l));
    return xyz(l) * saturate((l.w * 1.0f) / (totalAvg + 1e-12f));
}
// Packing.hlsli:197 UnpackTwoFp32ToFp16(uint3): a from the high halves, b from the low ones
static inline void DN_UnpackTwo(const uint w[3], float3& a, float3& b) {
    a = make_float3(f16tof32(w[0] >> 16), f16tof32(w[1] >> 16), f16tof32(w[2] >> 16));
    b = make_float3(f16tof32(w[0] & 0xFFFFu), f16tof32(w[1] & 0xFFFFu), f16tof32(w[2] & 0xFFFFu));
}

// PostProcess.hlsl:94-159 (the "#else" branch: scaled by clipToWindowScale)
static inline float2 DN_ComputeSpecularMotionVector(float3 primaryHitPosWorld, float3 primaryRayDirWorld, float3 primaryHitNormalWorld, float3 reflectionRayWorld,
                                                    const float* worldToClipMatrix, const float* prevWorldToClipMatrix, const float* clipToWindowScale) {
    float3 principalAxis = primaryHitNormalWorld;
    float zObj = dot(principalAxis, reflectionRayWorld);
    if (zObj < 0.0f) { principalAxis = make_float3(-principalAxis.x, -principalAxis.y, -principalAxis.z); zObj = -zObj; }
    zObj = fmaxf_(zObj, 1e-5f);
    const float3 n = principalAxis;
    const float s = n.z < 0.0f ? -1.0f : 1.0f;
    const float a = -1.0f / (s + n.z);
    const float b = n.x * n.y * a;
    const float3 xAxis = make_float3(1.0f + s * n.x * n.x * a, s * b, -s * n.x);
    const float3 yAxis = make_float3(b, s + n.y * n.y * a, -n.y);
    const float xObj = dot(xAxis, reflectionRayWorld);
    const float yObj = dot(yAxis, reflectionRayWorld);
    const float3 imagePosInReflectorSpace = make_float3(xObj, yObj, -zObj);
    const float3 imageInWorld = primaryHitPosWorld + primaryRayDirWorld * length(imagePosInReflectorSpace);
    const float4 prevClip = SP_mul_row(imageInWorld, prevWorldToClipMatrix);
    const float2 prevNdc = make_float2(prevClip.x / prevClip.w, prevClip.y / prevClip.w);
    const float4 currClip = SP_mul_row(imageInWorld, worldToClipMatrix);
    const float2 currNdc = make_float2(currClip.x / currClip.w, currClip.y / currClip.w);
    const float2 v = make_float2(prevNdc.x - currNdc.x, prevNdc.y - currNdc.y);
    return make_float2(v.x * clipToWindowScale[0], v.y * clipToWindowScale[1]);
}

// PostProcess.hlsl:161-173
static inline float3 DN_NRDRadianceClamp(float3 radiance, float rangeK, float preExposedGrayLuminance) {
    const float kClampMax = fminf_(255.0f, preExposedGrayLuminance * rangeK);      // (kClampMin is computed by the text and not used)
    const float lum = Luminance(radiance);
    if (lum > kClampMax) radiance = radiance * (kClampMax / lum);
    return radiance;
}

// PostProcess.hlsl:60-72: a neighbour clamped into the frame (at an edge: the pixel itself), plane stablePlaneIndex
static inline float DN_NeighbourDisocclusionRelaxation(const StablePlanesContext& sp, int px, int py, uint stablePlaneIndex, float3 rayDirC, int ox, int oy) {
    const float kEdge = 0.02f;
    int nx = px + ox, ny = py + oy;
    nx = nx < 0 ? 0 : (nx > (int)sp.C.imageWidth - 1 ? (int)sp.C.imageWidth - 1 : nx);
    ny = ny < 0 ? 0 : (ny > (int)sp.C.imageHeight - 1 ? (int)sp.C.imageHeight - 1 : ny);
    if (sp.GetBranchID((uint)nx, (uint)ny, stablePlaneIndex) == cStablePlaneInvalidBranchID) return kEdge;
    const float3 rayDirN = OctToNDirUnorm32(sp.B.Planes[sp.PixelToAddress((uint)nx, (uint)ny, stablePlaneIndex)].PackedNormal);
    return 1.0f - dot(rayDirC, rayDirN);
}
// PostProcess.hlsl:74-92 (the diagonals are "#if 0" there)
static inline float DN_DisocclusionRelaxation(const StablePlanesContext& sp, int px, int py, uint stablePlaneIndex, float3 rayDirC) {
    float r = 0.0f;
    r += DN_NeighbourDisocclusionRelaxation(sp, px, py, stablePlaneIndex, rayDirC, -1, 0);
    r += DN_NeighbourDisocclusionRelaxation(sp, px, py, stablePlaneIndex, rayDirC, 1, 0);
    r += DN_NeighbourDisocclusionRelaxation(sp, px, py, stablePlaneIndex, rayDirC, 0, -1);
    r += DN_NeighbourDisocclusionRelaxation(sp, px, py, stablePlaneIndex, rayDirC, 0, 1);
    return saturate((r - 0.00002f) * 25.0f);
}

// ---- PostProcess.hlsl:198-440, DENOISER_PREPARE_INPUTS with DENOISER_DLSS_RR (MIX_STABLE_RADIANCE, MIX_BY_THROUGHPUT, ALLOW_MIX_NORMALS all 1). Planes are read only where their
// branch id is valid, except the specular-MV block, which reads plane 0 as the text does. Output colour: RGBA32F here (RGBA16F in the reference).
static inline void DN_PrepareDLSSRR(const StablePlanesContext& sp, const DenoiserParams& P, const DenoiserBuffers& D, uint px, uint py, float4* outputColor) {
    const size_t pix = (size_t)py * sp.C.imageWidth + px;
    const uint dominantStablePlaneIndex = sp.LoadDominantIndex(px, py);
    const uint active = sp.C.activeStablePlaneCount;
    float3 combinedRadiance = sp.LoadStableRadiance(px, py);
    const float3 rm = ReinhardMax(combinedRadiance);
    const float3 stableAlbedo = make_float3(sqrtf_(rm.x), sqrtf_(rm.y), sqrtf_(rm.z));
    const float stableAlbedoAvg = Average(stableAlbedo);
    float3 guideNormals = make_float3(0.0f, 0.0f, 1e-6f), diffAlbedo = make_float3(0.0f), specAlbedo = make_float3(0.0f);
    float roughness = 0.0f;

    float spWeights[3] = {0.0f, 0.0f, 0.0f};
    {
        const float kTW = 0.2f, kNW = 0.01f, kDW = 0.05f;
        float spAvailable[3] = {1.0f, 0.0f, 0.0f}, thpWeights[3] = {1.0f, 0.0f, 0.0f};
        for (uint i = 1; i < active; i++) {
            if (sp.GetBranchID(px, py, i) == cStablePlaneInvalidBranchID) continue;
            float3 throughput, motionVectors; DN_UnpackTwo(sp.B.Planes[sp.PixelToAddress(px, py, i)].PackedThpAndMVs, throughput, motionVectors);
            const float weight = saturate(Average(throughput));
            thpWeights[i] = weight;
            thpWeights[0] = saturate(thpWeights[0] - weight);
            spAvailable[i] = 1.0f;
        }
        for (int j = 0; j < 3; j++) spWeights[j] = spWeights[j] + thpWeights[j] * kTW;
        for (int j = 0; j < 3; j++) spWeights[j] = spWeights[j] + 1.0f * kNW;
        if (dominantStablePlaneIndex < 3u) spWeights[dominantStablePlaneIndex] += kDW;      // (the build pass stores 0..2; a header word with 3 in its low bits adds nothing)
        for (int j = 0; j < 3; j++) spWeights[j] = spWeights[j] * spAvailable[j];
        const float sum = (spWeights[0] + spWeights[1]) + spWeights[2];
        for (int j = 0; j < 3; j++) spWeights[j] = spWeights[j] / sum;
        // primaryLayer: `if (spWeights.x >= max(spWeights.y, spWeights.y))` — the second operand really is y twice in the text. It only feeds a debug view, so nothing here
        // depends on it; tests/denoiser_inputs_ref.py restates it.
    }
    for (uint i = 0; i < active; i++) {
        if (sp.GetBranchID(px, py, i) == cStablePlaneInvalidBranchID) continue;
        const StablePlane rec = sp.B.Planes[sp.PixelToAddress(px, py, i)];
        if (!SP_isfinite(rec.SceneLength)) continue;      // skip sky
        combinedRadiance = combinedRadiance + xyz(DN_GetNoisyRadianceAndSpecRA(rec));
        const float weight = spWeights[i];
        if (weight > 1e-6f) {
            float3 diffBSDFEstimate, specBSDFEstimate; DN_UnpackTwo(rec.DenoiserPackedBSDFEstimate, diffBSDFEstimate, specBSDFEstimate);
            guideNormals = guideNormals + DN_GetNormal(rec) * weight;
            roughness = roughness + weight * DN_GetRoughness(rec);
            diffAlbedo = diffAlbedo + diffBSDFEstimate * weight;
            specAlbedo = specAlbedo + specBSDFEstimate * weight;
        }
    }
    const float3 stableAlbedoGreyMix = lerp3(stableAlbedo, make_float3(0.5f), 0.2f);
    diffAlbedo = lerp3(diffAlbedo, stableAlbedoGreyMix, stableAlbedoAvg / (Average(diffAlbedo) + sqrtf_(stableAlbedoAvg) + 1e-7f));
    const float guideNormalsLength = length(guideNormals);
    if (guideNormalsLength < 1e-5f) guideNormals = make_float3(0.0f, 0.0f, 1.0f);
    else guideNormals = make_float3(guideNormals.x / guideNormalsLength, guideNormals.y / guideNormalsLength, guideNormals.z / guideNormalsLength);
    const float minAlbedo = 0.05f;
    if (Average(diffAlbedo + specAlbedo) < minAlbedo) diffAlbedo = diffAlbedo + make_float3(minAlbedo);
    // with DLSSRRBrightnessClampK = 0 every pixel whose max3 > 0 is scaled by 0 / max: its colour becomes 0, as the text does
    const float maxRadiance = DN_max3(combinedRadiance);
    if (maxRadiance > P.DLSSRRBrightnessClampK) combinedRadiance = combinedRadiance * (P.DLSSRRBrightnessClampK / maxRadiance);
    outputColor[pix] = make_float4(combinedRadiance, 1.0f);
    D.RRDiffuseAlbedo[pix] = Pack_R11G11B10_FLOAT(diffAlbedo);
    D.RRSpecAlbedo[pix] = Pack_R11G11B10_FLOAT(specAlbedo);
    D.RRNormalsAndRoughness[pix] = SP_PackHalf4(make_float4(guideNormals, roughness));

    // specular motion vectors from the hit distance: plane 0 without a look at its branch id, and the test on the MIXED guide roughness, as in the text
    const StablePlane m = sp.B.Planes[sp.PixelToAddress(px, py, 0)];
    const float3 primaryHitPosWorld = m.RayOrigin + m.RayDir * m.SceneLength;
    const float3 primaryRayDirWorld = m.RayDir;
    const float3 primaryHitNormalWorld = DN_GetNormal(m);
    float3 reflectionRayWorld = DN_reflect(primaryRayDirWorld, primaryHitNormalWorld);
    const float specHitT = sp.B.SpecularHitT[pix];
    reflectionRayWorld = reflectionRayWorld * specHitT;
    const float4 mv = SP_UnpackHalf4(sp.B.MotionVectors[pix]);
    float2 specMotionVector = make_float2(mv.x, mv.y);
    if (specHitT > 1e-3f && roughness < kSpecularRoughnessThreshold)
        specMotionVector = DN_ComputeSpecularMotionVector(primaryHitPosWorld, primaryRayDirWorld, primaryHitNormalWorld, reflectionRayWorld, sp.C.matWorldToClipNoOffset,
                                                          sp.C.prevMatWorldToClipNoOffset, sp.C.clipToWindowScale);
    D.RRSpecMotionVectors[pix] = (f32tof16(specMotionVector.y) << 16) | f32tof16(specMotionVector.x);
}

// ---- PostProcess.hlsl:442-573, DENOISER_PREPARE_INPUTS for NRD, plane stablePlaneIndex. cameraRayO / cameraRayD: Bridge::computeCameraRay of the pixel with sample index
// sampleBaseIndex + g_MiniConst.params.x, and params.x is the plane index (PathTracerBridgeDonut.hlsli:510-513, 543-553): plane p's viewZ uses the camera ray of sub-sample p.
// CombinedHistoryClampRelax accumulates over the planes of a frame; the reference clears it once per frame (RenderTargets::Clear, Sample.cpp:2130), here the call with
// initWithStableRadiance clears it (before its own plane adds to it). The R8 values are quantised when stored, so the next plane reads back what was stored.
static inline void DN_PrepareNRD(const StablePlanesContext& sp, const DenoiserParams& P, const DenoiserBuffers& D, uint px, uint py, uint stablePlaneIndex, bool initWithStableRadiance,
                                 float3 cameraRayO, float3 cameraRayD, float4* outputColor) {
    const size_t pix = (size_t)py * sp.C.imageWidth + px;
    if (initWithStableRadiance) { outputColor[pix] = make_float4(sp.LoadStableRadiance(px, py), 1.0f); D.CombinedHistoryClampRelax[pix] = 0; }
    bool hasSurface = false;
    const uint spBranchID = sp.GetBranchID(px, py, stablePlaneIndex);
    if (spBranchID != cStablePlaneInvalidBranchID) {
        const StablePlane rec = sp.B.Planes[sp.PixelToAddress(px, py, stablePlaneIndex)];
        if (SP_isfinite(rec.SceneLength)) {      // skip sky
            hasSurface = true;
            float3 diffBSDFEstimate, specBSDFEstimate; DN_UnpackTwo(rec.DenoiserPackedBSDFEstimate, diffBSDFEstimate, specBSDFEstimate);
            const float3 virtualWorldPos = cameraRayO + cameraRayD * rec.SceneLength;
            const float virtualViewspaceZ = SP_mul_row(virtualWorldPos, P.matWorldToView).z;
            float3 thp, motionVectors; DN_UnpackTwo(rec.PackedThpAndMVs, thp, motionVectors);
            D.ViewZ[pix] = virtualViewspaceZ;
            D.MotionVectors[pix] = SP_PackHalf4(make_float4(motionVectors, 0.0f));
            const float kMinRoughness = 0.2f;
            float finalRoughness = fmaxf_(kMinRoughness, DN_GetRoughness(rec));
            float disocclusionRelax = 0.0f;
            float specularSuppressionMul = 1.0f;
            if (stablePlaneIndex == 0 && P.stablePlanesSuppressPrimaryIndirectSpecularK != 0.0f && sp.C.activeStablePlaneCount > 1) {
                bool shouldSuppress = true;
                for (uint i = 1; i < sp.C.activeStablePlaneCount; i++) shouldSuppress &= sp.GetBranchID(px, py, i) != cStablePlaneInvalidBranchID;
                const float roughnessModifiedSuppression = P.stablePlanesSuppressPrimaryIndirectSpecularK;
                specularSuppressionMul = shouldSuppress ? saturate(1.0f - roughnessModifiedSuppression) : specularSuppressionMul;
            }
            const int vertexIndex = (int)StablePlanesVertexIndexFromBranchID(spBranchID);
            if (vertexIndex > 1) disocclusionRelax = DN_DisocclusionRelaxation(sp, (int)px, (int)py, stablePlaneIndex, DN_GetNormal(rec));
            D.DisocclusionThresholdMix[pix] = DN_StoreUnorm8(disocclusionRelax);
            D.CombinedHistoryClampRelax[pix] = DN_StoreUnorm8(saturate(DN_LoadUnorm8(D.CombinedHistoryClampRelax[pix]) + disocclusionRelax * saturate(Luminance(thp))));
            finalRoughness = saturate(finalRoughness + disocclusionRelax);
            float3 denoiserDiffRadiance = DN_GetNoisyDiffRadiance(rec);
            float3 denoiserSpecRadiance = DN_GetNoisySpecRadiance(rec);
            denoiserDiffRadiance = make_float3(denoiserDiffRadiance.x / diffBSDFEstimate.x, denoiserDiffRadiance.y / diffBSDFEstimate.y, denoiserDiffRadiance.z / diffBSDFEstimate.z);
            denoiserSpecRadiance = make_float3(denoiserSpecRadiance.x / specBSDFEstimate.x, denoiserSpecRadiance.y / specBSDFEstimate.y, denoiserSpecRadiance.z / specBSDFEstimate.z);
            denoiserSpecRadiance = denoiserSpecRadiance * specularSuppressionMul;
            D.NormalRoughness[pix] = make_float4(DN_GetNormal(rec), finalRoughness);      // NRD_FrontEnd_PackNormalAndRoughness(normal, finalRoughness, 0)
            const float rangeK = P.denoiserRadianceClampK * 16.0f;
            denoiserDiffRadiance = DN_NRDRadianceClamp(denoiserDiffRadiance, rangeK, P.preExposedGrayLuminance);
            denoiserSpecRadiance = DN_NRDRadianceClamp(denoiserSpecRadiance, rangeK, P.preExposedGrayLuminance);
            float specHitT = 0.0f;
            if (sp.LoadDominantIndex(px, py) == stablePlaneIndex) specHitT = sp.B.SpecularHitT[pix];
            D.DiffRadianceHitDist[pix] = make_float4(denoiserDiffRadiance, 0.0f);        // RELAX_ / REBLUR_FrontEnd_PackRadiance...(diff, 0, true)
            D.SpecRadianceHitDist[pix] = make_float4(denoiserSpecRadiance, specHitT);    // RELAX_FrontEnd_PackRadianceAndHitDist(spec, specHitT, true); REBLUR takes specHitT, viewZ and
            D.Roughness[pix] = DN_GetRoughness(rec);                                     // the raw roughness through REBLUR_FrontEnd_GetNormHitDist
        }
    }
    if (!hasSurface) D.ViewZ[pix] = kDenoiserViewZSkyMarker;
}

// ---- PostProcess.hlsl:577-690 DENOISER_FINAL_MERGE + DenoiserNRD::PostDenoiseProcess after the host's unpack: remodulate and add where viewZ is not the sky marker
static inline void DN_MergeNRD(const StablePlanesContext& sp, const DenoiserBuffers& D, uint px, uint py, uint stablePlaneIndex, const float4* diff, const float4* spec, float4* outputColor) {
    const size_t pix = (size_t)py * sp.C.imageWidth + px;
    if (D.ViewZ[pix] == kDenoiserViewZSkyMarker) return;
    const StablePlane& rec = sp.B.Planes[sp.PixelToAddress(px, py, stablePlaneIndex)];
    float3 diffBSDFEstimate, specBSDFEstimate; DN_UnpackTwo(rec.DenoiserPackedBSDFEstimate, diffBSDFEstimate, specBSDFEstimate);
    float3 d = xyz(diff[pix]), s = xyz(spec[pix]);
    d = make_float3(d.x * diffBSDFEstimate.x, d.y * diffBSDFEstimate.y, d.z * diffBSDFEstimate.z);
    s = make_float3(s.x * specBSDFEstimate.x, s.y * specBSDFEstimate.y, s.z * specBSDFEstimate.z);
    const float3 sum = d + s;
    float4 o = outputColor[pix];
    o.x = o.x + DN_max0(sum.x); o.y = o.y + DN_max0(sum.y); o.z = o.z + DN_max0(sum.z);
    outputColor[pix] = o;
}

#pragma clang force_cuda_host_device end

void launch_dn_prepare_dlss_rr(const StablePlanesContext& sp, const DenoiserParams& P, const DenoiserBuffers& D, float4* outputColor, hipStream_t st);
void launch_dn_prepare_nrd(const PathKernelContext& k, const StablePlanesContext& sp, const DenoiserParams& P, const DenoiserBuffers& D, uint planeIndex, bool init, uint sampleBaseIndex,
                           float4* outputColor, hipStream_t st);
void launch_dn_merge_nrd(const StablePlanesContext& sp, const DenoiserBuffers& D, uint planeIndex, const float4* diff, const float4* spec, float4* outputColor, hipStream_t st);
} // namespace ptk

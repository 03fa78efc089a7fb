// ORACLE pin (test infrastructure only): what the three denoiser passes of Rtxpt/ProcessingPasses/PostProcess.hlsl (DENOISER_PREPARE_INPUTS with and without
// DENOISER_DLSS_RR, DENOISER_FINAL_MERGE) and DenoiserNRD::PostDenoiseProcess (Rtxpt/NRD/DenoiserNRD.hlsli) take from outside their own text, so that the text itself can be
// compiled and run thread by thread (hlsl_tu.py main_pt emits it right after this file; refpt_denoiser_* in hlsl_pt_wrappers.inc drive it). Included inside namespace hl::pp.
// Everything here is this project's text; each stand-in says what it stands for and whether it is an assumption.
//
//   1. typed render targets: the formats of Rtxpt/SampleCommon/RenderTargets.cpp, converted on store and on load with the oracle's conversions (ptref::f32tof16,
//      ptref::f16tof32, ptref::Pack_R11G11B10_FLOAT). ASSUMPTION: the R8_UNORM store. D3D leaves the last bit of a float -> UNORM conversion to the hardware; the stand-in is
//      clamp to [0, 1] (NaN -> 0), x 255, round to nearest, ties to even. The load is q / 255.
//   2. NRD front end / back end (NRD.hlsli, NRDEncoding.hlsli are not part of the reference checkout): RECORDERS, not restatements. The front-end functions hand back the
//      fp32 arguments the text gave them, the back-end unpack functions are the identity: the boundary include/mi355pt.h documents.
//   3. HLSL intrinsics the shim does not have yet: reflect, clamp on int2, and max(0, float3) with D3D's NaN rule.
//   4. resource bindings (Bindings/ShaderResourceBindings.hlsli, DenoiserNRD.hlsli:25-31, PostProcess.hlsl:584-593) as globals the wrappers point at the caller's arrays.

// ---- 1. typed render targets
// RenderTargets.cpp:177-182   DenoiserDisocclusionThresholdMix, CombinedHistoryClampRelax    R8_UNORM
// RenderTargets.cpp:82-84     DenoiserMotionVectors                                          RGBA16_FLOAT
// RenderTargets.cpp:186-190   RRDiffuseAlbedo, RRSpecAlbedo                                  R11G11B10_FLOAT
// RenderTargets.cpp:191-193   RRNormalsAndRoughness                                          RGBA16_FLOAT
// RenderTargets.cpp:194-196   RRSpecMotionVectors                                            RG16_FLOAT
// RenderTargets.cpp:123-125   DenoiserViewspaceZ                                             R32_FLOAT (a plain float array)
// RenderTargets.cpp:139-141   SpecularHitT                                                   R32_FLOAT (a plain float array)
// RenderTargets.cpp:77-80, 90-92   ScreenMotionVectors, StableRadiance                       RGBA16_FLOAT, read only here: the wrappers decode them to float4 once (exact)
// RenderTargets.cpp:167-175   OutputColor is RGBA16_FLOAT in the reference; this project keeps it in RGBA32F, so the stand-in is a float4 array
// RenderTargets.cpp:102-113, 127-129   DenoiserDiff / SpecRadianceHitDist, DenoiserNormalRoughness hold NRD's packed values: behind the recorders, float4 arrays here
struct FmtUnorm8 { typedef unsigned char S; typedef float V;
    static S store(float v) { return (S)(uint)rintf(P::saturate(v) * 255.0f); }      // ASSUMPTION (see above); P::saturate(NaN) = 0; rintf in the default rounding mode: ties to even
    static float load(S q) { return (float)(uint)q / 255.0f; } };
struct Half4 { uint16_t v[4]; }; struct Half2 { uint16_t v[2]; };
struct FmtRGBA16F { typedef Half4 S; typedef float4 V;
    static S store(float4 c) { S s; s.v[0] = (uint16_t)P::f32tof16(c.x); s.v[1] = (uint16_t)P::f32tof16(c.y); s.v[2] = (uint16_t)P::f32tof16(c.z); s.v[3] = (uint16_t)P::f32tof16(c.w); return s; }
    static float4 load(S s) { return float4(P::f16tof32(s.v[0]), P::f16tof32(s.v[1]), P::f16tof32(s.v[2]), P::f16tof32(s.v[3])); } };
struct FmtRG16F { typedef Half2 S; typedef float2 V;
    static S store(float2 c) { S s; s.v[0] = (uint16_t)P::f32tof16(c.x); s.v[1] = (uint16_t)P::f32tof16(c.y); return s; }
    static float2 load(S s) { return float2(P::f16tof32(s.v[0]), P::f16tof32(s.v[1])); } };
struct FmtR11G11B10F { typedef uint S; typedef float4 V;                              // write-only in these passes
    static S store(float4 c) { return P::Pack_R11G11B10_FLOAT(P::make_float3(c.x, c.y, c.z)); }
    static float4 load(S) { return float4(); } };
// a UAV / SRV of such a format: an element converts when it is read and when it is assigned; accesses outside the texture read 0 and are dropped (D3D)
template <class Fmt> struct TypedTarget {
    typename Fmt::S* p = nullptr; uint w = 0, h = 0;
    struct Ref { typename Fmt::S* q;
        operator typename Fmt::V() const { return q ? Fmt::load(*q) : typename Fmt::V(); }
        void operator=(typename Fmt::V v) const { if (q) *q = Fmt::store(v); } };
    Ref operator[](uint2 c) const { return Ref{(p && c.x < w && c.y < h) ? p + (size_t)c.y * w + c.x : nullptr}; }
};

// ---- 2. NRD recorders. g_nrdCalls, when set, receives the two REBLUR_FrontEnd_GetNormHitDist calls of the thread that runs (pixel g_nrdPixel): hitDist, roughness each.
static float* g_nrdCalls = nullptr; static uint g_nrdCallCount = 0; static size_t g_nrdPixel = 0;
static inline float4 NRD_FrontEnd_PackNormalAndRoughness(float3 N, float roughness, float materialID) { return float4(N, roughness); }
static inline float REBLUR_FrontEnd_GetNormHitDist(float hitDist, float viewZ, float4 hitDistParams, float roughness) {
    if (g_nrdCalls && g_nrdCallCount < 2) { g_nrdCalls[4 * g_nrdPixel + 2 * g_nrdCallCount] = hitDist; g_nrdCalls[4 * g_nrdPixel + 2 * g_nrdCallCount + 1] = roughness; }
    g_nrdCallCount++; return hitDist; }
static inline float4 REBLUR_FrontEnd_PackRadianceAndNormHitDist(float3 radiance, float normHitDist, bool sanitize) { return float4(radiance, normHitDist); }
static inline float4 RELAX_FrontEnd_PackRadianceAndHitDist(float3 radiance, float hitDist, bool sanitize) { return float4(radiance, hitDist); }
static inline float4 REBLUR_BackEnd_UnpackRadianceAndNormHitDist(float4 data) { return data; }
static inline float4 RELAX_BackEnd_UnpackRadiance(float4 data) { return data; }

// ---- 3. intrinsics
static inline float3 reflect(float3 i, float3 n) { return i - n * (2.0f * dot(i, n)); }      // HLSL reflect: i - 2 * dot(i, n) * n (the factor 2 is exact wherever it is applied)
using hl::clamp;
static inline int2 clamp(int2 v, int2 lo, int2 hi) { return int2(min(max(v.x, lo.x), hi.x), min(max(v.y, lo.y), hi.y)); }
// `max(0, v)` of the final merge. D3D's max returns the other operand when one is NaN (the functional specification's max, DXIL FMax); the shim's max is the oracle's
// NaN-unaware `a > b ? a : b`, which hands a NaN second operand through. The merge is where a NaN (0 / 0 of the demodulation, times 0) arrives as that operand.
using hl::max;
static inline float3 max(int a, float3 b) { const float f = (float)a; return float3(b.x > f ? b.x : f, b.y > f ? b.y : f, b.z > f ? b.z : f); }

// ---- 4. bindings
static RWTexture2DArray<uint> u_StablePlanesHeader; static RWStructuredBuffer<StablePlane> u_StablePlanesBuffer; static RWTexture2D<float4> u_StableRadiance, u_OutputColor;
static int u_FeedbackBuffer, u_DebugLinesBuffer, u_DebugDeltaPathTree, u_DeltaPathSearchStack;      // DebugContext::Init's arguments: the stand-in context takes and ignores them
static TypedTarget<FmtR11G11B10F> u_RRDiffuseAlbedo, u_RRSpecAlbedo; static TypedTarget<FmtRGBA16F> u_RRNormalsAndRoughness, u_DenoiserMotionVectors; static TypedTarget<FmtRG16F> u_RRSpecMotionVectors;
static RWTexture2D<float> u_DenoiserViewspaceZ; static RWTexture2D<float4> u_DenoiserNormalRoughness, u_DenoiserDiffRadianceHitDist, u_DenoiserSpecRadianceHitDist;
static TypedTarget<FmtUnorm8> u_DenoiserDisocclusionThresholdMix, u_CombinedHistoryClampRelax;
// DENOISER_FINAL_MERGE's own bindings (PostProcess.hlsl:584-593)
static RWTexture2D<float4> u_InputOutput; static Texture2D<float4> t_DiffRadiance, t_SpecRadiance; static Texture2D<float> t_DenoiserViewspaceZ;
static TypedTarget<FmtUnorm8> t_DenoiserDisocclusionThresholdMix; static StructuredBuffer<StablePlane> t_StablePlanesBuffer;

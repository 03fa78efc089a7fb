// mi355pt — the bake passes (pt_bake.hip): environment cube and importance map, emissive triangles, light weights and proxies, the NEE-AT frame passes.
#pragma once
#include "pt_path.h"
#include "pt_neeat.h"
#include <hip/hip_runtime.h>

namespace ptk {
// EnvMapBaker: lat-long source (sc.envTex) + directional lights -> RGBA16F cube with mips (cube.mipOffset / dim / mipLevels filled by the caller)
void launch_env_cube_bake(const DeviceScene& sc, const EnvDirectionalLight* lights, uint nLights, uint2* texels, const EnvCube& cube, hipStream_t st);
void launch_env_cube_compress(uint2* texels, const EnvCube& cube, uint quality, hipStream_t st);      // every level through BC6UCompress.hlsl's encoder (quality 1: EncodeP1; 2: + the two-region modes) and the BC6H decode, in place
void launch_env_importance(const DeviceScene& sc, uint dim, uint sx, uint sy, float4* out, hipStream_t st);
void launch_bake_emissive(const DeviceScene& sc, const uint* subInstList, const uint* subInstTriOffset, uint numEmissiveSubInst, uint totalTris, uint lightBase,
                          PolymorphicLightInfo* lights, PolymorphicLightInfoEx* lightsEx, hipStream_t st);
// light weights (power^0.8), their in-order sum, proxy counts; then (after an exclusive scan of the counts by the caller) the proxy index fill
void launch_light_weights(const PolymorphicLightInfo* lights, const PolymorphicLightInfoEx* lightsEx, uint n, float* w, const LightFrustumBoost& boost, hipStream_t st);      // ComputeWeight (+ the frustum boost) per light
// weight sum (in light order) + ComputeProxyCounts; usage != null: NEE-AT's feedback term (n + 1 usage counts, the last one = pixels without valid feedback)
void launch_light_proxy_counts(const float* w, uint n, float* sum, uint budget, bool uniform, uint maxPerLight, uint* counts, const uint* usage, uint totalMaxFeedbackCount, float globalFeedbackUseWeight, hipStream_t st);
void launch_neeat_boost_weights(const float* base, const float* hist, uint nHist, uint n, float mul, float* cur, hipStream_t st);
void launch_neeat_begin(const NeeAtFrame& F, float* snapW, uint* snapC, bool preFilter, uint totalThreads, hipStream_t st);
void launch_neeat_end(const NeeAtFrame& F, hipStream_t st);
void launch_light_proxy_fill(const uint* counts, const uint* offsets, uint n, uint* proxies, uint capacity, hipStream_t st);
} // namespace ptk

// mi355pt — the bake passes: what a scene or a frame prepares on the device before paths are traced. One thread per texel, triangle, light, pixel or tile.
#include "pt_bake.h"
#include <cstdio>
#include <cstdlib>

namespace ptk {
// ---- EnvMapBaker on the device (EnvMapBaker.hlsl:194-246, 268-371; pt_envcube.h): BaseLayerCS makes four texels of mip 0 and their mip-1 texel per thread,
// MIPReduceCS the further levels from the stored (fp16) texels; solid-angle weighted, summation order of the shader
__device__ __forceinline__ float4 env_generate_texel(const DeviceScene& sc, const EnvDirectionalLight* __restrict__ lights, uint nLights, uint px, uint py, uint face, uint dim) {
    float3 envCol = env_sample_source(sc, CubemapGetDirectionFor(face, make_float2(((float)px + 0.0f + 0.5f) / (float)dim, ((float)py + 0.0f + 0.5f) / (float)dim)));
    for (uint i = 0; i < nLights; i++) envCol = envCol + EnvComputeLightContribution(px, py, face, lights[i], dim);
    if (sc.sky) {                                       // g_Const.ProcSkyEnabled (EnvMapBaker.hlsl:224-236): toLocal swaps y and z
        const float3 cubeDir = CubemapGetDirectionFor(face, make_float2(((float)px + 0.5f) / (float)dim, ((float)py + 0.5f) / (float)dim));
        const float3 cubeDirRight = CubemapGetDirectionFor(face, make_float2((((float)px + 1.0f) + 0.5f) / (float)dim, ((float)py + 0.5f) / (float)dim)) - cubeDir;
        const float3 cubeDirBottom = CubemapGetDirectionFor(face, make_float2(((float)px + 0.5f) / (float)dim, (((float)py + 1.0f) + 0.5f) / (float)dim)) - cubeDir;
        envCol = envCol + ProceduralSky(make_float3(cubeDir.x, cubeDir.z, cubeDir.y), *sc.sky, sc.skyLowRes, cubeDir, cubeDirRight, cubeDirBottom);
    }
    envCol = envCol * kEnvMapRadianceScale;
    envCol = clamp3(envCol, 0.0f, HLF_MAX);
    return make_float4(envCol.x, envCol.y, envCol.z, 1.0f);
}
__device__ __forceinline__ float4 env_reduce(float4 e00, float4 e01, float4 e10, float4 e11, float4 wsa) {
    float wsum = wsa.x + wsa.y + wsa.z + wsa.w;
    float4 s = (e00 * wsa.x + e01 * wsa.y) + e10 * wsa.z + e11 * wsa.w;
    return make_float4(s.x / wsum, s.y / wsum, s.z / wsum, s.w / wsum);
}
// LowResPrePassLayerCS (EnvMapBaker.hlsl:247-265): the clouds of the procedural sky at half the cube's resolution, one thread per texel, RGBA16F
__global__ void __launch_bounds__(256) k_env_sky_lowres(DeviceScene sc, uint2* __restrict__ texels, uint res) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= 6u * res * res) return;
    const uint face = i / (res * res), r = i - face * res * res, y = r / res, x = r - y * res;
    const float3 direction = CubemapGetDirectionFor(face, make_float2(((float)x + 0.5f) / (float)res, ((float)y + 0.5f) / (float)res));
    texels[i] = env_pack_rgba16f(ProceduralSkyLowRes(x, y, face, make_float3(direction.x, direction.z, direction.y), *sc.sky));
}
__global__ void __launch_bounds__(256) k_env_cube_base(DeviceScene sc, const EnvDirectionalLight* __restrict__ lights, uint nLights, uint2* __restrict__ texels, EnvCube cube) {
    const uint dim = cube.dim, h = dim / 2u;
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= 6u * h * h) return;
    const uint face = i / (h * h), r = i - face * h * h, y = r / h, x = r - y * h;
    float4 e00 = env_generate_texel(sc, lights, nLights, 2 * x, 2 * y, face, dim), e01 = env_generate_texel(sc, lights, nLights, 2 * x, 2 * y + 1, face, dim),
           e10 = env_generate_texel(sc, lights, nLights, 2 * x + 1, 2 * y, face, dim), e11 = env_generate_texel(sc, lights, nLights, 2 * x + 1, 2 * y + 1, face, dim);
    uint2* m0 = texels + cube.mipOffset[0] + (size_t)face * dim * dim;
    m0[(size_t)(2 * y) * dim + 2 * x] = env_pack_rgba16f(e00); m0[(size_t)(2 * y + 1) * dim + 2 * x] = env_pack_rgba16f(e01);
    m0[(size_t)(2 * y) * dim + 2 * x + 1] = env_pack_rgba16f(e10); m0[(size_t)(2 * y + 1) * dim + 2 * x + 1] = env_pack_rgba16f(e11);
    if (cube.mipLevels > 1u) texels[cube.mipOffset[1] + ((size_t)face * h + y) * h + x] = env_pack_rgba16f(env_reduce(e00, e01, e10, e11, CubemapTexelSolidAngle4((float)dim, 2 * x, 2 * y)));
}
__global__ void __launch_bounds__(256) k_env_cube_mip(uint2* __restrict__ texels, EnvCube cube, uint level) {
    const uint d = cube.dim >> level, s = d * 2u;
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= 6u * d * d) return;
    const uint face = i / (d * d), r = i - face * d * d, y = r / d, x = r - y * d;
    const uint2* src = texels + cube.mipOffset[level - 1u] + (size_t)face * s * s;
    texels[cube.mipOffset[level] + ((size_t)face * d + y) * d + x] = env_pack_rgba16f(env_reduce(
        env_unpack_rgba16f(src[(size_t)(2 * y) * s + 2 * x]), env_unpack_rgba16f(src[(size_t)(2 * y + 1) * s + 2 * x]),
        env_unpack_rgba16f(src[(size_t)(2 * y) * s + 2 * x + 1]), env_unpack_rgba16f(src[(size_t)(2 * y + 1) * s + 2 * x + 1]), CubemapTexelSolidAngle4((float)s, 2 * x, 2 * y)));
}
// BC6UCompress.hlsl CSMain (QUALITY 0) + the texture unit's BC6H_UF16 decode, in place: one thread per 4x4 block of one cube level (pt_envcube.h)
__global__ void __launch_bounds__(64) k_env_cube_bc6(uint2* __restrict__ level, uint dim, uint quality) {
    const uint nb = dim / 4u; uint i = blockIdx.x * 64u + threadIdx.x; if (i >= 6u * nb * nb) return;
    const uint face = i / (nb * nb), r = i - face * nb * nb, by = r / nb, bx = r - by * nb;
    env_cube_bc6_round_trip_block(level, dim, face, bx, by, quality);
}
void launch_env_cube_compress(uint2* texels, const EnvCube& cube, uint quality, hipStream_t st) {
    for (uint l = 0; l < cube.mipLevels; l++) { const uint d = cube.dim >> l, nb = d / 4u; hipLaunchKernelGGL(k_env_cube_bc6, dim3((6u * nb * nb + 63u) / 64u), dim3(64), 0, st, texels + cube.mipOffset[l], d, quality); }
}
void launch_env_cube_bake(const DeviceScene& sc, const EnvDirectionalLight* lights, uint nLights, uint2* texels, const EnvCube& cube, hipStream_t st) {
    const uint h = cube.dim / 2u;
    if (sc.sky) hipLaunchKernelGGL(k_env_sky_lowres, dim3((6u * h * h + 255u) / 256u), dim3(256), 0, st, sc, const_cast<uint2*>(sc.skyLowRes.texels), h);
    hipLaunchKernelGGL(k_env_cube_base, dim3((6u * h * h + 255u) / 256u), dim3(256), 0, st, sc, lights, nLights, texels, cube);
    for (uint l = 2; l < cube.mipLevels; l++) { const uint d = cube.dim >> l; hipLaunchKernelGGL(k_env_cube_mip, dim3((6u * d * d + 255u) / 256u), dim3(256), 0, st, texels, cube, l); }
}

// BuildMIPDescentImportanceMapCS (Rtxpt/Lighting/Distant/EnvMapImportanceSamplingBaker.hlsl:57-90) on the baked cube
__global__ void __launch_bounds__(256) k_env_importance(DeviceScene sc, uint dim, uint sx, uint sy, float4* __restrict__ out) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= dim * dim) return;
    uint x = i % dim, y = i / dim;
    float L = 0.f; float3 R = make_float3(0.f);
    const float invSamples = 1.f / (float)(sx * sy);
    for (uint j = 0; j < sy; j++) for (uint ii = 0; ii < sx; ii++) {
        float2 p = make_float2(((float)(x * sx + ii) + 0.5f) / (float)(dim * sx), ((float)(y * sy + j) + 0.5f) / (float)(dim * sy));
        float3 dir = oct_to_ndir_equal_area_unorm(p);
        // t_EnvMapCube.SampleLevel(s_LinearWrap, dir, 0) (:77) — the uncompressed cube (EnvMapBaker.cpp:635)
        float3 radiance = xyz(env_cube_sample_level(sc.envCubeSource, dir, 0.f));
        L += (Luminance(radiance) + Average(radiance)) * 0.5f;
        R += radiance;
    }
    // u_RadianceMap is RGBA16_FLOAT (EnvMapImportanceSamplingBaker.cpp:170)
    out[i] = env_round_rgba16f(make_float4(R.x * invSamples, R.y * invSamples, R.z * invSamples, L * invSamples));
}

// BakeEmissiveTriangles (Rtxpt/Lighting/LightsBaker.hlsl:544-716): one thread per emissive triangle, output in sub-instance order
__global__ void __launch_bounds__(256) k_bake_emissive(DeviceScene sc, const uint* __restrict__ subInstList, const uint* __restrict__ subInstTriOffset, uint numEmissiveSubInst,
                                                       uint totalTris, uint lightBase, PolymorphicLightInfo* __restrict__ lights, PolymorphicLightInfoEx* __restrict__ lightsEx) {
    uint t = blockIdx.x * 256u + threadIdx.x; if (t >= totalTris) return;
    uint lo = 0, hi = numEmissiveSubInst;                 // last k with offset[k] <= t
    while (hi - lo > 1) { uint mid = (lo + hi) >> 1; if (subInstTriOffset[mid] <= t) lo = mid; else hi = mid; }
    uint s = subInstList[lo], tri = t - subInstTriOffset[lo];
    uint2 ig = sc.subInstToInstGeom[s];
    const InstanceDesc& inst = sc.instances[ig.x];
    const GeometryDesc& g = sc.geometries[ig.y];
    const PTMaterialData& mat = sc.materials[g.materialIndex];
    const uint* idx = sc.indices + g.indexOffset + 3u * tri;
    uint i0 = g.vertexOffset + idx[0], i1 = g.vertexOffset + idx[1], i2 = g.vertexOffset + idx[2];
    const float* P = sc.positions;
    float3 p0 = xform_point(inst.transform, make_float3(P[3 * i0], P[3 * i0 + 1], P[3 * i0 + 2]));
    float3 p1 = xform_point(inst.transform, make_float3(P[3 * i1], P[3 * i1 + 1], P[3 * i1 + 2]));
    float3 p2 = xform_point(inst.transform, make_float3(P[3 * i2], P[3 * i2 + 1], P[3 * i2 + 2]));
    float3 radiance = mat.EmissiveColor;
    if ((mat.Flags & PTMaterialFlags_UseEmissiveTexture) && (g.flags & GEOM_HAS_UV)) {
        float2 uv0 = sc.uvs[i0], uv1 = sc.uvs[i1], uv2 = sc.uvs[i2];
        float2 e0 = uv1 - uv0, e1 = uv2 - uv1, e2 = uv0 - uv2;
        float l0 = length(e0), l1 = length(e1), l2 = length(e2);
        float2 shortE, longE1, longE2;
        if (l0 < l1 && l0 < l2) { shortE = e0; longE1 = e1; longE2 = e2; } else if (l1 < l2) { shortE = e1; longE1 = e2; longE2 = e0; } else { shortE = e2; longE1 = e0; longE2 = e1; }
        float2 sg = shortE * (2.0f / 3.0f); float2 lg = (longE1 + longE2) * (1.0f / 3.0f);
        const TexInfo& tex = sc.textures[mat.EmissiveTextureIndex & 0xFFFFu];
        float2 c = (uv0 + uv1 + uv2) * (1.0f / 3.0f);
        // emissiveTexture.SampleGrad(s_materialSampler, centerUV, shortGradient, longGradient) (:647)
        radiance = radiance * xyz(sample_grad_anisotropic(sc, tex, c, sg, lg));
    }
    radiance = max3v(radiance, make_float3(0.f));
    bool isFlipped = det3(inst.transform) < 0.f;
    TriangleLight tl; tl.base = p0;
    if (!isFlipped) { tl.edge1 = p1 - p0; tl.edge2 = p2 - p0; } else { tl.edge1 = p2 - p0; tl.edge2 = p1 - p0; }
    if (fmaxf_(radiance.x, fmaxf_(radiance.y, radiance.z)) < 1e-7f) radiance = make_float3(0.f);
    tl.radiance = radiance; tl.normal = make_float3(0.f); tl.surfaceArea = 0;
    PolymorphicLightInfoFull lf = tl.Store(0);
    lights[lightBase + t] = lf.Base; lightsEx[lightBase + t] = lf.Extended;
}

void launch_env_importance(const DeviceScene& sc, uint dim, uint sx, uint sy, float4* out, hipStream_t st) {
    hipLaunchKernelGGL(k_env_importance, dim3((dim * dim + 255) / 256), dim3(256), 0, st, sc, dim, sx, sy, out);
}
// ---- light weights and the sampling-proxy table on the device (ComputeWeights / ComputeProxyCounts / the proxy fill of LightsBaker.hlsl:738-751, 836-948), so
// that a per-frame re-bake of animated emissives (C5) needs no D2H / host loop / H2D. Arithmetic = the host loop it replaces (and the oracle's): weight =
// power^0.8 with the deterministic pow, thresholded; the weight SUM is taken in light order by ONE lane, because a float sum is only reproducible in a fixed
// order (7 k lights: ~10 us; the table limit of 512 k lights: ~1 ms); counts = ceil((budget - N) * w / sum), capped; offsets by an exclusive scan (integers);
// the fill is per proxy.
__global__ void __launch_bounds__(256) k_light_weights(const PolymorphicLightInfo* __restrict__ lights, const PolymorphicLightInfoEx* __restrict__ lightsEx, uint n, float* __restrict__ w, LightFrustumBoost boost) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= n) return;
    PolymorphicLightInfoFull lf; lf.Base = lights[i]; lf.Extended = lightsEx[i];
    float wt = dm_pow(PolymorphicLight_GetPower(lf), 0.8f);
    if (!(wt >= 1e-8f)) wt = 0.f;                         // RTXPT_LIGHTING_MIN_WEIGHT_THRESHOLD
    w[i] = light_importance_frustum_boost(boost, lf, wt);      // ImportanceBooster, frustum term (off unless the host supplied its view-projection matrix)
}
// the sum in light order: the block stages 256 weights at a time in LDS (coalesced loads), lane 0 adds them one after the other
__global__ void __launch_bounds__(256) k_light_weight_sum(const float* __restrict__ w, uint n, float* __restrict__ sum) {
    __shared__ float stage[256];
    float s = 0.f;
    for (uint base = 0; base < n; base += 256u) {
        const uint i = base + threadIdx.x;
        stage[threadIdx.x] = (i < n) ? w[i] : 0.f;
        __syncthreads();
        if (threadIdx.x == 0) { const uint m = (n - base < 256u) ? n - base : 256u; for (uint k = 0; k < m; k++) s += stage[k]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) *sum = s;
}
// usage != null (NEE-AT, last frame left feedback): the weight is pulled towards the number of pixels that asked for the light (pt_neeat.h
// neeat_feedback_light_weight)
__global__ void __launch_bounds__(256) k_light_proxy_counts(const float* __restrict__ w, uint n, const float* __restrict__ sum, uint budget, uint uniform, uint maxPerLight, uint* __restrict__ counts,
                                                            const uint* __restrict__ usage, uint totalMaxFeedbackCount, float globalFeedbackUseWeight) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= n) return;
    float lightWeight = w[i];
    if (usage) lightWeight = neeat_feedback_light_weight(lightWeight, usage[i], *sum, totalMaxFeedbackCount, usage[n], globalFeedbackUseWeight);
    uint cnt = 0;
    if (lightWeight > 0) cnt = uniform ? 1u : (uint)ceilf(((float)(budget - n) * lightWeight) / *sum);
    counts[i] = cnt < maxPerLight ? cnt : maxPerLight;
}
// ComputeWeights of a NEE-AT frame: the baked weight, boosted where the light got brighter than 1.1 x what it weighed last frame (ImportanceBooster,
// LightsBaker.hlsl:137-147)
__global__ void __launch_bounds__(256) k_neeat_boost_weights(const float* __restrict__ base, const float* __restrict__ hist, uint nHist, uint n, float mul, float* __restrict__ cur) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= n) return;
    cur[i] = hist ? neeat_intensity_delta_boost(base[i], i < nHist ? hist[i] : 0.f, mul) : base[i];
}
// ---- NEE-AT feedback passes (pt_neeat.h): one thread per pixel / low-resolution pixel / tile; every pass reads what the previous one wrote and writes only
// its own slot
__global__ void __launch_bounds__(256) k_neeat_prefilter(NeeAtFrame F, const float* __restrict__ snapW, const uint* __restrict__ snapC) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= F.W * F.H) return;
    neeat_prefilter_pixel(F, snapW, snapC, (int)(i % F.W), (int)(i / F.W));
}
// P0's counts: neighbouring pixels mostly ask for the same few lights, and same-address atomics serialise in the L2. Two merges before anything reaches memory
// (the reference merges equal lanes with WaveMatch, LightsBaker.hlsl:1287-1305): the lanes of a wave (an 8 x 8 pixel block) that count the same light become
// one entry, and the sixteen waves of a block (32 x 32 pixels) add their entries into a small LDS hash table that is flushed once — one global atomic per
// distinct light and 32 x 32 pixels.
static const uint NEEAT_P0_TABLE = 512u;      // LDS hash slots per block (a full table falls back to a global atomic per entry)
__global__ void __launch_bounds__(1024) k_neeat_p0(NeeAtFrame F, uint totalThreads) {
    __shared__ uint hKey[NEEAT_P0_TABLE]; __shared__ uint hCnt[NEEAT_P0_TABLE];
    const uint NONE = 0xFFFFFFFFu, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint k = threadIdx.x; k < NEEAT_P0_TABLE; k += 1024u) { hKey[k] = NONE; hCnt[k] = 0u; }
    // the dispatch's threads beyond the frame count as "no valid feedback"
    if (blockIdx.x == 0u && threadIdx.x == 0u && totalThreads > F.W * F.H) atomicAdd(&F.perLightCounters[F.totalLightCount], totalThreads - F.W * F.H);
    __syncthreads();
    const uint regionsX = (F.W + 31u) / 32u;
    const uint px = (blockIdx.x % regionsX) * 32u + (wave & 3u) * 8u + (lane & 7u), py = (blockIdx.x / regionsX) * 32u + (wave >> 2) * 8u + (lane >> 3);
    const uint slot = (px < F.W && py < F.H) ? neeat_p0_pixel(F, px, py) : NONE;
    unsigned long long active = __builtin_amdgcn_ballot_w64(slot != NONE);
    while (active) {
        const uint leader = (uint)__builtin_ctzll(active);
        const uint v = (uint)__builtin_amdgcn_readlane((int)slot, (int)leader);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(slot == v);
        if (lane == leader) {
            const uint n = (uint)__popcll(same);
            uint h = (v * 2654435761u) >> 23; bool placed = false;                 // 9-bit multiplicative hash, linear probing
            for (uint probe = 0; probe < 16u && !placed; probe++, h = (h + 1u) & (NEEAT_P0_TABLE - 1u)) {
                const uint prev = atomicCAS(&hKey[h], NONE, v);
                if (prev == NONE || prev == v) { atomicAdd(&hCnt[h], n); placed = true; }
            }
            if (!placed) atomicAdd(&F.perLightCounters[v], n);
        }
        active &= ~same;
    }
    __syncthreads();
    for (uint k = threadIdx.x; k < NEEAT_P0_TABLE; k += 1024u) if (hKey[k] != NONE) atomicAdd(&F.perLightCounters[hKey[k]], hCnt[k]);
}
__global__ void __launch_bounds__(256) k_neeat_p1a(NeeAtFrame F) { uint i = blockIdx.x * 256u + threadIdx.x; if (i < F.BW * F.BH) neeat_p1a_pixel(F, i % F.BW, i / F.BW); }
__global__ void __launch_bounds__(256) k_neeat_p1b(NeeAtFrame F) { uint i = blockIdx.x * 256u + threadIdx.x; if (i < F.W * F.H) neeat_p1b_pixel(F, i % F.W, i / F.W); }
__global__ void __launch_bounds__(64) k_neeat_p2(NeeAtFrame F) { uint i = blockIdx.x * 64u + threadIdx.x; if (i < F.tilesX * F.tilesY) neeat_fill_tile(F, i % F.tilesX, i / F.tilesX); }
// P3: one 64-lane block per tile. The 128 light indices are sorted in LDS with a bitonic network (compare-exchange pairs as in MiniEngine's Bitonic32PreSortCS,
// which the reference cites: element `hi` = lane with a one inserted at bit j, partner = hi ^ (first step of a merge ? k - 1 : j)); then every entry finds the
// ends of its run.
__global__ void __launch_bounds__(64) k_neeat_p3(NeeAtFrame F) {
    __shared__ uint key[RTXPT_LIGHTING_LOCAL_PROXY_COUNT];
    const uint N = RTXPT_LIGHTING_LOCAL_PROXY_COUNT, t = threadIdx.x;
    uint* tile = F.local + (size_t)blockIdx.x * N;
    key[t] = UnpackMiniListLight(tile[t]); key[t + N / 2] = UnpackMiniListLight(tile[t + N / 2]);
    __syncthreads();
    for (uint k = 2; k <= N; k <<= 1) for (uint j = k / 2; j > 0; j >>= 1) {
        const uint mask = j - 1u, hi = ((t & ~mask) << 1) | (t & mask) | j, lo = hi ^ (k == 2u * j ? k - 1u : j);
        const uint a = key[lo], b = key[hi];
        if (a > b) { key[lo] = b; key[hi] = a; }
        __syncthreads();
    }
    for (uint e = t; e < N; e += N / 2) {
        const uint v = key[e]; uint l = e, r = e;
        while (l > 0u && key[l - 1u] == v) l--;
        while (r + 1u < N && key[r + 1u] == v) r++;
        tile[e] = PackMiniListLightAndCount(v, r - l + 1u);
    }
}
__global__ void __launch_bounds__(256) k_neeat_clear(NeeAtFrame F) { uint i = blockIdx.x * 256u + threadIdx.x; if (i < F.W * F.H) neeat_clear_pixel(F, i % F.W, i / F.W); }
// one thread per proxy slot: the light whose [offset, offset + count) range holds the slot (binary search over the scanned offsets)
__global__ void __launch_bounds__(256) k_light_proxy_fill(const uint* __restrict__ counts, const uint* __restrict__ offsets, uint n, uint* __restrict__ proxies, uint capacity) {
    const uint p = blockIdx.x * 256u + threadIdx.x;
    const uint total = offsets[n - 1u] + counts[n - 1u];
    if (p >= total || p >= capacity) return;
    // last light with offset <= p (lights without proxies share their successor's offset: skipped by taking the last)
    uint lo = 0u, hi = n;
    while (hi - lo > 1u) { uint mid = (lo + hi) >> 1; if (offsets[mid] <= p) lo = mid; else hi = mid; }
    proxies[p] = lo;
}
void launch_light_weights(const PolymorphicLightInfo* lights, const PolymorphicLightInfoEx* lightsEx, uint n, float* w, const LightFrustumBoost& boost, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_light_weights, dim3((n + 255) / 256), dim3(256), 0, st, lights, lightsEx, n, w, boost);
}
void launch_light_proxy_counts(const float* w, uint n, float* sum, uint budget, bool uniform, uint maxPerLight, uint* counts, const uint* usage, uint totalMaxFeedbackCount, float globalFeedbackUseWeight, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(k_light_weight_sum, dim3(1), dim3(256), 0, st, w, n, sum);
    hipLaunchKernelGGL(k_light_proxy_counts, dim3((n + 255) / 256), dim3(256), 0, st, w, n, sum, budget, uniform ? 1u : 0u, maxPerLight, counts, usage, totalMaxFeedbackCount, globalFeedbackUseWeight);
}
void launch_neeat_boost_weights(const float* base, const float* hist, uint nHist, uint n, float mul, float* cur, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_neeat_boost_weights, dim3((n + 255) / 256), dim3(256), 0, st, base, hist, nHist, n, mul, cur);
}
// UpdateBegin's feedback half: PreFilter from a snapshot of the reservoirs (snapW / snapC: W x H scratch), then P0's counts. The counters are expected zeroed
// (totalLightCount + 1 words).
void launch_neeat_begin(const NeeAtFrame& F, float* snapW, uint* snapC, bool preFilter, uint totalThreads, hipStream_t st) {
    const uint px = F.W * F.H;
    if (preFilter) {
        (void)hipMemcpyAsync(snapW, F.fbW, 4ull * px, hipMemcpyDeviceToDevice, st); (void)hipMemcpyAsync(snapC, F.fbC, 4ull * px, hipMemcpyDeviceToDevice, st);
        hipLaunchKernelGGL(k_neeat_prefilter, dim3((px + 255) / 256), dim3(256), 0, st, F, snapW, snapC);
        if (getenv("MI355PT_NEEAT_DEBUG")) fprintf(stderr, "[neeat] prefilter: %s\n", hipGetErrorString(hipStreamSynchronize(st)));
    }
    hipLaunchKernelGGL(k_neeat_p0, dim3(((F.W + 31) / 32) * ((F.H + 31) / 32)), dim3(1024), 0, st, F, totalThreads);
    if (getenv("MI355PT_NEEAT_DEBUG")) fprintf(stderr, "[neeat] p0: %s\n", hipGetErrorString(hipStreamSynchronize(st)));
}
// UpdateEnd: blended reservoirs, one candidate per pixel, the tiles (fill, sort + count), and the reservoirs cleared down to what the next frame keeps
void launch_neeat_end(const NeeAtFrame& F, hipStream_t st) {
    const uint px = F.W * F.H, bpx = F.BW * F.BH, tiles = F.tilesX * F.tilesY;
    const bool dbg = getenv("MI355PT_NEEAT_DEBUG") != nullptr;
#define NEEAT_DBG(what) do { if (dbg) { hipError_t e = hipStreamSynchronize(st); fprintf(stderr, "[neeat] %s: %s\n", what, hipGetErrorString(e)); } } while (0)
    hipLaunchKernelGGL(k_neeat_p1a, dim3((bpx + 255) / 256), dim3(256), 0, st, F); NEEAT_DBG("p1a");
    hipLaunchKernelGGL(k_neeat_p1b, dim3((px + 255) / 256), dim3(256), 0, st, F); NEEAT_DBG("p1b");
    hipLaunchKernelGGL(k_neeat_p2, dim3((tiles + 63) / 64), dim3(64), 0, st, F); NEEAT_DBG("p2");
    hipLaunchKernelGGL(k_neeat_p3, dim3(tiles), dim3(64), 0, st, F); NEEAT_DBG("p3");
    hipLaunchKernelGGL(k_neeat_clear, dim3((px + 255) / 256), dim3(256), 0, st, F); NEEAT_DBG("clear");
#undef NEEAT_DBG
}
void launch_light_proxy_fill(const uint* counts, const uint* offsets, uint n, uint* proxies, uint capacity, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(k_light_proxy_fill, dim3((capacity + 255) / 256), dim3(256), 0, st, counts, offsets, n, proxies, capacity);
}
void launch_bake_emissive(const DeviceScene& sc, const uint* subInstList, const uint* subInstTriOffset, uint numEmissiveSubInst, uint totalTris, uint lightBase,
                          PolymorphicLightInfo* lights, PolymorphicLightInfoEx* lightsEx, hipStream_t st) {
    if (!totalTris) return;
    hipLaunchKernelGGL(k_bake_emissive, dim3((totalTris + 255) / 256), dim3(256), 0, st, sc, subInstList, subInstTriOffset, numEmissiveSubInst, totalTris, lightBase, lights, lightsEx);
}
} // namespace ptk

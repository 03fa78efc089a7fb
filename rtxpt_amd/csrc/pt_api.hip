// mi355pt — C-ABI implementation (include/mi355pt.h): context, scene upload, BVH build/refit orchestration, light baking and
// read-back; the frame drivers (pt_render and the realtime passes) are in pt_frame.hip, the display tail (pt_tonemap, pt_average_luminance) in pt_display.hip. the tile shards and their exchanges in pt_shard.hip / pt_shard_host.cpp. Host side of the seam `Sample` implements in the reference
// (Rtxpt/Sample.cpp:1891-2313 Render, :2438-2559 PathTrace, :1464-1556 UpdatePathTracerConstants, :2770-2778 accumulation).
// There is NO CPU fallback: every entry point that needs the device fails with PT_ERROR_NO_DEVICE / PT_ERROR_HIP.
#include <cstring>
#include <rocprim/rocprim.hpp>      // before pt_context.h: its `using namespace ptk` makes rocprim's own uint2 / uint4 ambiguous
#include "pt_context.h"
#include "pt_denoiser.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <chrono>

using namespace ptk;

static_assert(sizeof(::PTMaterialData) == sizeof(ptk::PTMaterialData), "material ABI");
static_assert(sizeof(::PathTracerCameraData) == sizeof(ptk::PathTracerCameraData), "camera ABI");
static_assert(sizeof(::PtSettings) == sizeof(ptk::PtSettings), "settings ABI");
static_assert(sizeof(::PtGeometryDesc) == sizeof(ptk::GeometryDesc), "geometry ABI");
static_assert(sizeof(::PtInstanceDesc) == sizeof(ptk::InstanceDesc), "instance ABI");
static_assert(sizeof(::PolymorphicLightInfo) == sizeof(ptk::PolymorphicLightInfo), "light ABI");

namespace {

// the host path's chain and level 0: pt_texture_ingest.h's texel arithmetic, one texel at a time
void build_mips(HostTexture& t) {
    const uint lv = texi_level_count(t.w, t.h);
    t.mipLevels = lv; t.mips.resize(lv);
    for (uint l = 1; l < lv; l++) {
        const uint pw = texi_side(t.w, l - 1), ph = texi_side(t.h, l - 1), mw = texi_side(t.w, l), mh = texi_side(t.h, l);
        t.mips[l].resize((size_t)mw * mh);
        const ptk::float4* p = t.mips[l - 1].data();
        for (uint y = 0; y < mh; y++) for (uint x = 0; x < mw; x++) t.mips[l][(size_t)y * mw + x] = texi_mip_texel(p, pw, ph, x, y);
    }
}
void host_convert_texture(const PtTextureDesc& d, HostTexture& t) {
    t.w = d.width; t.h = d.height; t.mips.clear(); t.mips.resize(1); t.mips[0].resize((size_t)d.width * d.height);
    for (size_t k = 0; k < (size_t)d.width * d.height; k++) {
        if (d.format == PT_TEX_RGBA32F) { const float* p = (const float*)d.pixels + 4 * k; t.mips[0][k] = ptk::make_float4(p[0], p[1], p[2], p[3]); }
        else { const uint8_t* p = (const uint8_t*)d.pixels + 4 * k; t.mips[0][k] = texi_level0_rgba8((uint)p[0] | ((uint)p[1] << 8) | ((uint)p[2] << 16) | ((uint)p[3] << 24), d.format); }
    }
    build_mips(t);
}
size_t host_texture_bytes(const HostTexture& t) { size_t n = 0; for (auto& m : t.mips) n += m.size() * sizeof(ptk::float4); return n; }

// the accumulation starts again: no samples, uniform sample counts, and what was derived from the old one (the denoised picture) is gone. The callers clear dAccum.
void reset_accumulation(pt_context* c) { c->accumCount = 0; c->adaptive.perPixel = false; accum_denoise_drop(c); }

// the host path: the texels the setters converted (HostTexture::mips) pooled and uploaded, with the tables pt_texture_ingest.h lays out. With PT_DEVICE_TEXTURES_ON_DEVICE the
// material textures are on the device already (pt_texture_ingest.hip) and only the environment image is placed.
int upload_textures(pt_context* c) {
    if (c->deviceTextures) return tex_place_environment(c);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<ptk::float4> pool; c->texInfos.clear();
    auto add = [&](const HostTexture& t) {
        TexInfo ti; memset(&ti, 0, sizeof(ti)); ti.w = t.w; ti.h = t.h; ti.base = pool.size();
        if (t.mips.size() == 1) { ti.mipLevels = 1; pool.insert(pool.end(), t.mips[0].begin(), t.mips[0].end()); return ti; }      // (the environment image: level 0 only)
        texi_layout(t.w, t.h, &ti.mipLevels, ti.mipOffset);
        for (uint l = 0; l < t.mipLevels && l < 16; l++) pool.insert(pool.end(), t.mips[l].begin(), t.mips[l].end());
        return ti;
    };
    for (auto& t : c->textures) c->texInfos.push_back(add(t));
    c->matTexels = pool.size();
    memset(&c->envTexInfo, 0, sizeof(TexInfo));
    if (c->envEnabled && c->envTex.w) c->envTexInfo = add(c->envTex);      // (a procedural sky alone has no image)
    // alpha planes (pt_scene.h AlphaPlane): the opacity channel of every texture's mip 0 on its own, a byte per texel where every value is k / 255
    std::vector<uint> fmts(c->textures.size()); size_t poolBytes = 0;
    for (size_t ti = 0; ti < c->textures.size(); ti++) {
        const std::vector<ptk::float4>& m0 = c->textures[ti].mips[0];
        bool bytes = true;
        for (size_t k = 0; k < m0.size() && bytes; k++) bytes = texi_alpha_is_byte(m0[k].w);
        fmts[ti] = bytes ? 0u : 1u;
    }
    { int r = tex_plan_alpha_planes(c, fmts, &poolBytes); if (r != PT_OK) return r; }
    std::vector<unsigned char> apool(poolBytes, 0);
    for (size_t ti = 0; ti < c->textures.size(); ti++) {
        const std::vector<ptk::float4>& m0 = c->textures[ti].mips[0]; const size_t at = c->alphaPlanes[ti].offset;
        if (!fmts[ti]) for (size_t k = 0; k < m0.size(); k++) apool[at + k] = (unsigned char)texi_alpha_byte(m0[k].w);
        else for (size_t k = 0; k < m0.size(); k++) memcpy(&apool[at + 4u * k], &m0[k].w, 4);
    }
    PT_CHECK_HIP(c, c->dAlphaPlanes.upload(c->alphaPlanes, c->stream)); PT_CHECK_HIP(c, c->dAlphaPool.upload(apool, c->stream));
    PT_CHECK_HIP(c, c->dTexels.upload(pool, c->stream));
    PT_CHECK_HIP(c, c->dTexInfos.upload(c->texInfos, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    c->texDirty = false;
    // (pt_get_texture_ingest_stats) what this path did and what it keeps: the converted texels of every level stay on the host for the next upload
    PtTextureIngestStats& s = c->texStats; const double hostMs = c->texHostMs; memset(&s, 0, sizeof(s));
    for (size_t ti = 0; ti < c->textures.size(); ti++) {
        const HostTexture& t = c->textures[ti];
        s.level0Texels += (uint64_t)t.w * t.h; s.sourceBytes += (uint64_t)t.w * t.h * (c->texFormats[ti] == PT_TEX_RGBA32F ? 16u : 4u); s.hostBytesHeld += host_texture_bytes(t);
    }
    s.hostBytesHeld += host_texture_bytes(c->envTex); s.poolTexels = pool.size();
    s.uploadMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); s.totalMs = hostMs + s.uploadMs;
    return PT_OK;
}

void refresh_scene_view(pt_context* c) {
    DeviceScene& d = c->dsc;
    d.travSpill = c->dTravSpill.p;                           // allocated (and checked) by finalize_geometry
    d.indices = c->dIndices.p; d.positions = c->dPositions.p; d.uvs = c->dUvs.p; d.normals = c->dNormals.p; d.tangents = c->dTangents.p;
    d.geometries = c->dGeometries.p; d.instances = c->dInstances.p; d.subInstances = c->dSubInstances.p; d.subInstToInstGeom = c->dSubInstToInstGeom.p;
    const bool prevPose = c->motionHistory && c->dPrevPositions.p && c->dPrevInstances.p && c->dPrevPositions.n >= c->positions.size() && c->dPrevInstances.n >= c->instances.size();
    d.prevPositions = prevPose ? c->dPrevPositions.p : nullptr; d.prevInstances = prevPose ? c->dPrevInstances.p : nullptr;
    d.materials = c->dMaterials.p; d.materialCount = (uint)c->materials.size(); d.textures = c->dTexInfos.p; d.texels = c->dTexels.p;
    d.envCube = c->envCube; d.envCube.texels = c->dEnvCube.p;
    d.sky = c->skyEnabled ? c->dSky.p : nullptr; memset(&d.skyLowRes, 0, sizeof(d.skyLowRes)); d.skyLowRes.texels = c->dSkyLowRes.p; d.skyLowRes.dim = c->envCubeDim / 2u; d.skyLowRes.mipLevels = 1u;
    d.envCubeSource = d.envCube; if (c->envCompression && c->dEnvCubeSource.p) d.envCubeSource.texels = c->dEnvCubeSource.p;
    d.envImageCube = c->envImageCubeDim ? c->dEnvImageCube.p : nullptr; d.envImageCubeDim = c->envImageCubeDim; d._padEnvImageCube = 0u;
    d.envTex = c->envTexInfo; d.envEnabled = c->envEnabled ? 1u : 0u; d.envToWorld = c->envToWorld; d.envToLocal = c->envToLocal; d.envColorMultiplier = c->envColorMul;
    d.lights.Lights = c->dLights.p; d.lights.LightsEx = c->dLightsEx.p; d.lights.ProxyCounters = c->dProxyCounters.p; d.lights.ProxyIndices = c->dProxyIndices.p;
    d.lights.TotalLightCount = (uint)c->lights.size(); d.lights.SamplingProxyCount = c->numProxies;
    d.lights.EnvLookupMap = c->dEnvLookup.p; d.lights.EnvLookupDim = c->envLookupDim; d.lights.EnvToWorld = c->envToWorld; d.lights.WorldToEnv = c->envToLocal;
    d.lights.LocalSamplingBuffer = c->localResX ? (c->neeat.enabled ? c->neeat.local.p : c->dLocalTable.p) : nullptr; d.lights.LocalResX = c->localResX; d.lights.LocalResY = c->localResY; d.lights.LocalJitterX = c->localJitterX; d.lights.LocalJitterY = c->localJitterY;
    d.lights.DepthExport = (c->neeat.enabled && c->neeat.exportDepth && c->neeat.haveClip && c->neeat.W == c->width && c->neeat.H == c->height) ? c->neeat.depth.p : nullptr; d.lights.DepthWidth = c->width;
    memcpy(d.lights.ClipZ, c->neeat.clipZ, 16); memcpy(d.lights.ClipW, c->neeat.clipW, 16);
    d.lights.LocalToGlobalSampleRatio = c->localResX ? c->localRatio : 0.f; d.lights.ScreenSpaceVsWorldSpaceThreshold = c->sscThreshold; d.lights.TemporalFeedbackRequired = c->feedbackRequired ? 1u : 0u;
    d.nodes = c->bvh.bvh2Stale ? nullptr : c->bvh.nodes; d.nodes8 = c->bvh.nodes8; d.tris = c->bvh.triSorted; d.alphaRecs = c->bvh.alphaRecs; d.alphaPlanes = c->dAlphaPlanes.p; d.alphaPool = c->dAlphaPool.p; d.shadeTris = c->dShadeTris.p; d.primToSlot = c->bvh.primToSlot; d.primInfo = c->dPrimInfo.p; d.numTris = c->numTris; d.rootIsValid = c->numTris ? 1u : 0u;
}

// SubInstanceData fill (Rtxpt/Materials/MaterialsBaker.cpp:960-1017) + primitive table; then GPU LBVH build
// (pt_set_motion_history, below) previous pose <- current pose, on the device
static int32_t motion_history_sync(pt_context* c) {
    if (!c->motionHistory) return PT_OK;
    const bool fresh = c->dPrevPositions.n < c->positions.size() || c->dPrevInstances.n < c->instances.size() || !c->dPrevPositions.p || !c->dPrevInstances.p;
    PT_CHECK_HIP(c, c->dPrevPositions.resize(c->positions.size())); PT_CHECK_HIP(c, c->dPrevInstances.resize(c->instances.size()));
    if (c->instances.size()) PT_CHECK_HIP(c, hipMemcpyAsync(c->dPrevInstances.p, c->dInstances.p, sizeof(InstanceDesc) * c->instances.size(), hipMemcpyDeviceToDevice, c->stream));
    if (fresh || c->prevAllStale) { if (c->positions.size()) PT_CHECK_HIP(c, hipMemcpyAsync(c->dPrevPositions.p, c->dPositions.p, 4 * c->positions.size(), hipMemcpyDeviceToDevice, c->stream)); }
    else for (size_t r = 0; r + 1 < c->prevStaleRanges.size(); r += 2) {
        const size_t first = 3 * (size_t)c->prevStaleRanges[r], count = 3 * (size_t)c->prevStaleRanges[r + 1];
        if (count) PT_CHECK_HIP(c, hipMemcpyAsync(c->dPrevPositions.p + first, c->dPositions.p + first, 4 * count, hipMemcpyDeviceToDevice, c->stream));
    }
    c->prevAllStale = false; c->prevStaleRanges.clear();
    return PT_OK;
}
// (pt_set_skinning) the description leaves the device
static void skin_drop(pt_context* c) {
    if (c->skinSet) (void)hipSetDevice(c->device);
    c->skinSet = false; c->skinRanges.clear(); c->skinStale.clear(); c->skinMatrices = c->skinWeights = 0u; memset(&c->skinView, 0, sizeof(c->skinView));
    c->dSkinJoints.free(); c->dSkinWeights.free(); c->dSkinNormals.free(); c->dSkinTangents.free(); c->dSkinBind.free(); c->dSkinDeltaP.free(); c->dSkinDeltaN.free(); c->dSkinDeltaT.free();
    c->dSkinRanges.free(); c->dSkinRangeStart.free(); c->dSkinMatrices.free(); c->dSkinMorphWeights.free();
}
// (pt_animate_skinned) the host copies of the vertex streams <- the device's, over the ranges a device pose rewrote: paid by whoever reads the copies, not by every frame
static int32_t sync_mirrors(pt_context* c) {
    if (!c->mirrorsStale) return PT_OK;
    for (size_t r = 0; r + 1 < c->mirrorRanges.size(); r += 2) {
        const size_t first = c->mirrorRanges[r], count = c->mirrorRanges[r + 1];
        if (!count || first + count > c->normals.size()) continue;
        PT_CHECK_HIP(c, hipMemcpyAsync(c->positions.data() + 3 * first, c->dPositions.p + 3 * first, 12 * count, hipMemcpyDeviceToHost, c->stream));
        PT_CHECK_HIP(c, hipMemcpyAsync(c->normals.data() + first, c->dNormals.p + first, 4 * count, hipMemcpyDeviceToHost, c->stream));
        PT_CHECK_HIP(c, hipMemcpyAsync(c->tangents.data() + first, c->dTangents.p + first, 4 * count, hipMemcpyDeviceToHost, c->stream));
    }
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    c->mirrorsStale = false; c->mirrorRanges.clear();
    return PT_OK;
}
int finalize_geometry(pt_context* c) {
    c->subInstances.clear(); c->subInstToInstGeom.clear(); c->primInfo.clear(); c->subInstFirstPrim.clear();
    for (size_t i = 0; i < c->instances.size(); i++) {
        if (c->instances[i].meshIndex >= c->meshes.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "instance references a missing mesh");
        const MeshDesc& m = c->meshes[c->instances[i].meshIndex];
        for (uint g = 0; g < m.numGeometries; g++) {
            uint gi = m.firstGeometry + g;
            if (gi >= c->geometries.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "mesh references a missing geometry");
            const GeometryDesc& gd = c->geometries[gi];
            if (gd.materialIndex >= c->materials.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "geometry references a missing material");
            const ptk::PTMaterialData& mat = c->materials[gd.materialIndex];
            SubInstanceData si; memset(&si, 0, sizeof(si));
            bool alphaTested = (gd.geomFlags & GEOMF_ALPHA_TESTED) && (mat.Flags & PTMaterialFlags_UseBaseOrDiffuseTexture) && (gd.flags & GEOM_HAS_UV);
            if (alphaTested) {
                si.FlagsAndAlphaInfo |= SubInstanceData::Flags_AlphaTested;
                uint cutoff = (uint)(saturate(mat.AlphaCutoff) * 255.0f);
                si.FlagsAndAlphaInfo |= (cutoff & 0xFFu) << SubInstanceData::Flags_AlphaOffsetOffset;
                si.FlagsAndAlphaInfo |= (mat.BaseOrDiffuseTextureIndex & 0xFFFFu);
            }
            if (gd.geomFlags & GEOMF_EXCLUDE_FROM_NEE) si.FlagsAndAlphaInfo |= SubInstanceData::Flags_ExcludeFromNEE;
            si.GlobalGeometryIndex_PTMaterialDataIndex = (gi << 16) | (gd.materialIndex & 0xFFFFu);
            si.EmissiveLightMappingOffset = 0xFFFFFFFFu; si.AnalyticProxyLightIndex = 0xFFFFFFFFu;
            si.IndexOffset = gd.indexOffset; si.TexCoord1Offset = gd.vertexOffset;
            uint subInst = (uint)c->subInstances.size();
            c->subInstToInstGeom.push_back(ptk::make_uint2((uint)i, gi));
            c->subInstances.push_back(si); c->subInstFirstPrim.push_back((uint)c->primInfo.size());
            for (uint t = 0; t < gd.numIndices / 3; t++) c->primInfo.push_back(ptk::make_uint2(subInst, t));
        }
    }
    // traversal addresses triangles, and the alpha records parallel to them (alpha_test_slot), with 32-bit byte offsets (48 B records: slot * 48 < 2^32) and 28-bit leaf references
    if (c->primInfo.size() > 0x7FFFFFFull / 3ull * 2ull)
        return fail(c, PT_ERROR_UNSUPPORTED, "more than 89 M triangles per scene are not supported by the traversal kernels");
    c->numTris = (uint)c->primInfo.size();
    hipStream_t st = c->stream;
    PT_CHECK_HIP(c, c->dIndices.upload(c->indices, st)); PT_CHECK_HIP(c, c->dPositions.upload(c->positions, st)); PT_CHECK_HIP(c, c->dUvs.upload(c->uvs, st));
    PT_CHECK_HIP(c, c->dNormals.upload(c->normals, st)); PT_CHECK_HIP(c, c->dTangents.upload(c->tangents, st));
    PT_CHECK_HIP(c, c->dGeometries.upload(c->geometries, st)); PT_CHECK_HIP(c, c->dInstances.upload(c->instances, st));
    PT_CHECK_HIP(c, c->dSubInstances.upload(c->subInstances, st)); PT_CHECK_HIP(c, c->dSubInstToInstGeom.upload(c->subInstToInstGeom, st));
    PT_CHECK_HIP(c, c->dPrimInfo.upload(c->primInfo, st)); PT_CHECK_HIP(c, c->dMaterials.upload(c->materials, st));
    // a new scene: its history starts here (previous = current)
    if (c->motionHistory) { c->prevAllStale = true; c->prevStaleRanges.clear(); int r = motion_history_sync(c); if (r != PT_OK) return r; }
    if (c->bvhAllocated && c->bvh.capacity < c->numTris) { bvh_free(c->bvh); c->bvhAllocated = false; }
    if (!c->bvhAllocated) { PT_CHECK_HIP(c, bvh_alloc(c->bvh, c->numTris)); c->bvhAllocated = true; }
    c->bvh.builder = c->bvhBuilder; c->bvh.occlusionSlotOrder = c->occlusionSlotOrder ? 1u : 0u;
    // BVH_BUILDER_PLOC_OPT: parallel re-insertion passes (MI355X, C3: 8 passes = 1463 Mrays/s in 63 ms, 12 = 1477 in 81 ms, 16 = 1476 in 98 ms; host SAH +
    // re-insertion 1479 in 1824 ms — profiles/r03k_device_reinsertion_sweep.txt)
    { const char* e = getenv("MI355PT_REINSERT_PASSES"); c->bvh.riPasses = e ? (uint)atoi(e) : 12u; }
    PT_CHECK_HIP(c, c->dShadeTris.resize(c->numTris)); PT_CHECK_HIP(c, c->dInertBits.resize(inert_words(c->numTris)));
    // traversal stack tails, one region per pipelined batch (4 x 302 MB of 288 GB)
    if (!c->dTravSpill.p) PT_CHECK_HIP(c, c->dTravSpill.resize(PT_PIPELINE_BATCHES * (size_t)T8_MAX_BLOCKS * T8_GROUPS_PER_BLOCK * T8_SPILL_DEPTH));
    refresh_scene_view(c);
    hipEvent_t e0, e1; PT_CHECK_HIP(c, hipEventCreate(&e0)); PT_CHECK_HIP(c, hipEventCreate(&e1));
    PT_CHECK_HIP(c, hipEventRecord(e0, st));
    PT_CHECK_HIP(c, bvh_build(c->bvh, c->dsc, c->numTris, st));
    PT_CHECK_HIP(c, hipEventRecord(e1, st));
    launch_shade_tris(c->dsc, 0u, c->numTris, c->dShadeTris.p, st);
    launch_inert_bits(c->dsc, c->numTris, c->dInertBits.p, st);      // (every material edit comes through here: pt_set_materials marks the geometry dirty)
    PT_CHECK_HIP(c, hipStreamSynchronize(st));
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1); c->buildMs = ms; (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    c->geomDirty = false; c->lightsDirty = true;
    return PT_OK;
}

// ---- light baking. Order (Rtxpt/Lighting/LightsBaker.cpp:663-827): env quads, analytic lights, emissive triangles per sub-instance.
const uint RTXPT_LIGHTING_MAX_LIGHTS = 512 * 1024, RTXPT_LIGHTING_SAMPLING_PROXY_RATIO = 12, RTXPT_LIGHTING_MAX_SAMPLING_PROXIES_PER_LIGHT = 256 * 1024;
const float RTXPT_LIGHTING_MIN_WEIGHT_THRESHOLD = 1e-8f;
const uint QT_BASE_RES = 4, QT_SUBDIV = 24, QT_UNBOOSTED = QT_BASE_RES * QT_BASE_RES + 3 * QT_SUBDIV, QT_BOOST_DPT = 3, QT_BOOST_SUBDIV = 20,
           QT_BOOST_MULT = QT_BOOST_SUBDIV * 3 + 1, QT_TOTAL = QT_UNBOOSTED * QT_BOOST_MULT, EMISB_DIM = 1024;
struct EnvImportance { uint dim, mipCount; std::vector<std::vector<ptk::float4>> mips; };
uint firstbithigh(uint v) { uint r = 0; while (v >>= 1) r++; return r; }
// EnvironmentComputeWeightForQTBuild (LightsBaker.hlsl:181-198)
uint qt_weight(const EnvImportance& im, uint dim, uint x, uint y, uint lightIndex, uint depthLimit) {
    uint mipLevel = im.mipCount - firstbithigh(dim) - 1;
    float areaMul = (float)(1u << (mipLevel * 2));
    float radiance = im.mips[mipLevel][(size_t)y * dim + x].w;
    float ret = areaMul * radiance;
    ret = fmaxf_(sq(1.0f / 100.0f) * (float)mipLevel, ret);
    ret *= (mipLevel > depthLimit) ? 1.0f : 0.0f;
    uint v = (uint)(FastSqrt(ret) * 100 + 0.5f); if (v > 0x000FFFFFu) v = 0x000FFFFFu;
    return (v << 12) | lightIndex;
}
struct QTNode { uint dim, x, y; };
// EnvLightsSubdivideBase / EnvLightsSubdivideBoost (LightsBaker.hlsl:262-467): greedy split of the heaviest node
void qt_subdivide(const EnvImportance& im, std::vector<QTNode>& nodes, std::vector<uint>& packed, uint subdivisions, uint depthLimit) {
    for (uint si = 0; si < subdivisions; si++) {
        uint best = 0; for (size_t i = 0; i < packed.size(); i++) best = std::max(best, packed[i]);
        uint gi = best & 0xFFFu;
        QTNode n = nodes[gi];
        for (uint k = 0; k < 4; k++) {
            QTNode ch; ch.dim = n.dim * 2; ch.x = n.x * 2 + (k % 2); ch.y = n.y * 2 + (k / 2);
            uint ni = (k == 0) ? gi : (uint)nodes.size();
            if (k == 0) { nodes[gi] = ch; packed[gi] = qt_weight(im, ch.dim, ch.x, ch.y, ni, depthLimit); }
            else { nodes.push_back(ch); packed.push_back(qt_weight(im, ch.dim, ch.x, ch.y, ni, depthLimit)); }
        }
    }
}
int bake_env_quads(pt_context* c) {
    EnvImportance im; im.dim = EMISB_DIM; im.mipCount = 11; im.mips.resize(im.mipCount);
    PT_CHECK_HIP(c, c->dScratch4.resize((size_t)im.dim * im.dim));
    launch_env_importance(c->dsc, im.dim, 4, 4, c->dScratch4.p, c->stream);
    im.mips[0].resize((size_t)im.dim * im.dim);
    PT_CHECK_HIP(c, hipMemcpyAsync(im.mips[0].data(), c->dScratch4.p, sizeof(ptk::float4) * im.mips[0].size(), hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    for (uint l = 1; l < im.mipCount; l++) {
        uint pd = im.dim >> (l - 1), d = im.dim >> l;
        im.mips[l].resize((size_t)d * d);
        const std::vector<ptk::float4>& p = im.mips[l - 1];
        for (uint y = 0; y < d; y++) for (uint x = 0; x < d; x++) {
            ptk::float4 s = (p[(size_t)(2 * y) * pd + 2 * x] + p[(size_t)(2 * y) * pd + 2 * x + 1]) + (p[(size_t)(2 * y + 1) * pd + 2 * x] + p[(size_t)(2 * y + 1) * pd + 2 * x + 1]);
            // MipMapGenPass MODE_COLOR (Donut, not vendored: the 2x2 mean of the stored texels, stored as binary16)
            im.mips[l][(size_t)y * d + x] = ptk::env_round_rgba16f(s * 0.25f);
        }
    }
    std::vector<QTNode> base; std::vector<uint> packed;
    for (uint li = 0; li < QT_BASE_RES * QT_BASE_RES; li++) {
        QTNode n; n.dim = QT_BASE_RES; n.x = li / QT_BASE_RES; n.y = li % QT_BASE_RES;
        base.push_back(n); packed.push_back(qt_weight(im, n.dim, n.x, n.y, li, QT_BOOST_DPT));
    }
    qt_subdivide(im, base, packed, QT_SUBDIV, QT_BOOST_DPT);
    c->envLookupDim = im.dim; c->envLookup.assign((size_t)im.dim * im.dim, 0);
    const float distantVsLocal = 1.0f * 0.0002f;                                       // LightsBaker.cpp:1029-1030
    for (uint g = 0; g < QT_UNBOOSTED; g++) {
        std::vector<QTNode> nodes(1, base[g]); std::vector<uint> pk(1, qt_weight(im, base[g].dim, base[g].x, base[g].y, 0, 0));
        qt_subdivide(im, nodes, pk, QT_BOOST_SUBDIV, 0);
        for (uint li = 0; li < QT_BOOST_MULT; li++) {
            EnvironmentQuadLight e; e.NodeDim = nodes[li].dim; e.NodeX = nodes[li].x; e.NodeY = nodes[li].y;
            uint mipLevel = im.mipCount - firstbithigh(e.NodeDim) - 1;               // EnvironmentComputeRadianceAndWeight (LightsBaker.hlsl:167-175)
            float areaMul = (float)(1u << (mipLevel * 2));
            ptk::float4 value = im.mips[mipLevel][(size_t)e.NodeY * e.NodeDim + e.NodeX];
            e.Weight = areaMul * fmaxf_(0.f, value.w * Average(c->envColorMul) * distantVsLocal);
            e.Radiance = xyz(value) * c->envColorMul;
            PolymorphicLightInfoFull lf = e.Store(0);
            ptk::float2 sub = ptk::make_float2(((float)e.NodeX + 0.5f) / (float)e.NodeDim, ((float)e.NodeY + 0.5f) / (float)e.NodeDim);
            lf.Base.Center = mul_vec_mat3(oct_to_ndir_equal_area_unorm(sub), c->envToWorld) * DISTANT_LIGHT_DISTANCE;
            uint out = g * QT_BOOST_MULT + li;
            c->lights[out] = lf.Base; c->lightsEx[out] = lf.Extended;
            uint dimScale = im.dim / e.NodeDim;                                        // EnvLightsFillLookupMap (LightsBaker.hlsl:472-492)
            for (uint yy = 0; yy < dimScale; yy++) for (uint xx = 0; xx < dimScale; xx++)
                c->envLookup[(size_t)(e.NodeY * dimScale + yy) * im.dim + (e.NodeX * dimScale + xx)] = out;
        }
    }
    return PT_OK;
}
// geometryOnly: the instances / vertices moved but materials, environment, analytic lights and settings did not (pt_animate): the environment quad-tree lights
// are kept, only the emissive triangles are re-baked, and everything downstream (weights, proxy counts, proxy table) runs on the device. ComputeProxyCounts +
// the proxy fill (LightsBaker.hlsl:880-948, 1009-1060) from the weights in dWeights[0 .. N) (dWeights[N] receives their sum). usage != null: NEE-AT's feedback
// term. Leaves numProxies and the scene view current.
int build_light_proxies(pt_context* c, float* dWeights, const uint* dUsage, uint totalMaxFeedbackCount, float globalFeedbackUseWeight) {
    const uint N = (uint)c->lights.size(); if (!N) return PT_OK;
    const uint budget = RTXPT_LIGHTING_SAMPLING_PROXY_RATIO * std::max(N, RTXPT_LIGHTING_MAX_LIGHTS / 10);
    // sum of ceil((budget - N) w_i / W) <= budget - N + N (the feedback lerp keeps the weights' sum at W)
    const size_t proxyCapacity = (size_t)budget + N;
    PT_CHECK_HIP(c, c->dProxyCounters.resize(N)); PT_CHECK_HIP(c, c->dProxyOffsets.resize(N)); PT_CHECK_HIP(c, c->dProxyIndices.resize(proxyCapacity));
    launch_light_proxy_counts(dWeights, N, dWeights + N, budget, c->S.NEEType == 0, RTXPT_LIGHTING_MAX_SAMPLING_PROXIES_PER_LIGHT - 1, c->dProxyCounters.p, dUsage, totalMaxFeedbackCount, globalFeedbackUseWeight, c->stream);
    size_t need = 0;
    PT_CHECK_HIP(c, rocprim::exclusive_scan(nullptr, need, c->dProxyCounters.p, c->dProxyOffsets.p, 0u, (size_t)N, rocprim::plus<uint>(), c->stream));
    if (need > c->scanTempBytes) { if (c->dScanTemp) (void)hipFree(c->dScanTemp); c->dScanTemp = nullptr; PT_CHECK_HIP(c, hipMalloc(&c->dScanTemp, need)); c->scanTempBytes = need; }
    need = c->scanTempBytes;
    PT_CHECK_HIP(c, rocprim::exclusive_scan(c->dScanTemp, need, c->dProxyCounters.p, c->dProxyOffsets.p, 0u, (size_t)N, rocprim::plus<uint>(), c->stream));
    launch_light_proxy_fill(c->dProxyCounters.p, c->dProxyOffsets.p, N, c->dProxyIndices.p, (uint)proxyCapacity, c->stream);
    uint last[2] = {0u, 0u};                           // the proxy count is a field of the by-value scene view: one 8-byte read-back
    PT_CHECK_HIP(c, hipMemcpyAsync(&last[0], c->dProxyOffsets.p + (N - 1), 4, hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipMemcpyAsync(&last[1], c->dProxyCounters.p + (N - 1), 4, hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    c->numProxies = last[0] + last[1];
    if (c->numProxies > proxyCapacity) return fail(c, PT_ERROR_HIP, "light proxy table overflow");
    return PT_OK;
}
int bake_lights(pt_context* c, bool geometryOnly = false) {
    hipEvent_t e0, e1; PT_CHECK_HIP(c, hipEventCreate(&e0)); PT_CHECK_HIP(c, hipEventCreate(&e1));
    PT_CHECK_HIP(c, hipEventRecord(e0, c->stream));
    const bool keepEnv = geometryOnly && c->S.NEEEnabled && c->envEnabled && c->envLightsBaked == QT_TOTAL && c->lights.size() >= QT_TOTAL;
    if (!keepEnv) { c->lights.clear(); c->lightsEx.clear(); c->envLookup.clear(); c->envLookupDim = 0; c->envLightsBaked = 0; }
    else { c->lights.resize(QT_TOTAL); c->lightsEx.resize(QT_TOTAL); }
    c->numProxies = 0;
    for (auto& si : c->subInstances) { si.EmissiveLightMappingOffset = 0xFFFFFFFFu; si.AnalyticProxyLightIndex = 0xFFFFFFFFu; }
    if (c->S.NEEEnabled) {
        if (c->envEnabled && !keepEnv) { c->lights.resize(QT_TOTAL); c->lightsEx.resize(QT_TOTAL); int r = bake_env_quads(c); if (r != PT_OK) return r; c->envLightsBaked = QT_TOTAL; }
        const uint analyticBase = (uint)c->lights.size();
        for (auto& a : c->analyticLights) { c->lights.push_back(a.Base); c->lightsEx.push_back(a.Extended); }
        // analytic light proxies (LightsBaker.cpp:718-753): a mesh instance that stands in for an analytic light carries that light's index in its
        // sub-instances
        for (size_t s = 0; s < c->subInstances.size(); s++) {
            const uint proxy = c->instances[c->subInstToInstGeom[s].x].analyticProxyLight;
            if (proxy && proxy <= c->analyticLights.size() && (c->materials[c->subInstances[s].GlobalGeometryIndex_PTMaterialDataIndex & 0xFFFFu].Flags & PTMaterialFlags_EnableAsAnalyticLightProxy))
                c->subInstances[s].AnalyticProxyLightIndex = analyticBase + proxy - 1u;
        }
        // emissive triangles: host decides the layout (LightsBaker.cpp:663-827), the GPU bakes the records (LightsBaker.hlsl:544-716)
        std::vector<uint> list, offsets; uint total = 0; uint lightBase = (uint)c->lights.size();
        for (size_t s = 0; s < c->subInstances.size(); s++) {
            const GeometryDesc& g = c->geometries[c->subInstances[s].GlobalGeometryIndex_PTMaterialDataIndex >> 16];
            const ptk::PTMaterialData& mat = c->materials[g.materialIndex];
            bool isEmissive = any_gt0(mat.EmissiveColor);                            // PTMaterial::IsEmissive (MaterialsBaker.cpp:511-514)
            uint ntri = g.numIndices / 3;
            if (!isEmissive || (size_t)lightBase + total + ntri >= RTXPT_LIGHTING_MAX_LIGHTS) continue;
            c->subInstances[s].EmissiveLightMappingOffset = lightBase + total;
            list.push_back((uint)s); offsets.push_back(total); total += ntri;
        }
        // (the emissive part of the host mirror only holds the size)
        c->lights.resize((size_t)lightBase + total); c->lightsEx.resize((size_t)lightBase + total);
        const uint N = (uint)c->lights.size();
        PT_CHECK_HIP(c, c->dLights.resize(N)); PT_CHECK_HIP(c, c->dLightsEx.resize(N));
        if (lightBase && !keepEnv) {                       // environment quads + analytic lights: computed on the host, static under animation
            PT_CHECK_HIP(c, hipMemcpyAsync(c->dLights.p, c->lights.data(), sizeof(ptk::PolymorphicLightInfo) * lightBase, hipMemcpyHostToDevice, c->stream));
            PT_CHECK_HIP(c, hipMemcpyAsync(c->dLightsEx.p, c->lightsEx.data(), sizeof(ptk::PolymorphicLightInfoEx) * lightBase, hipMemcpyHostToDevice, c->stream));
        } else if (keepEnv && lightBase > QT_TOTAL) {
            PT_CHECK_HIP(c, hipMemcpyAsync(c->dLights.p + QT_TOTAL, c->lights.data() + QT_TOTAL, sizeof(ptk::PolymorphicLightInfo) * (lightBase - QT_TOTAL), hipMemcpyHostToDevice, c->stream));
            PT_CHECK_HIP(c, hipMemcpyAsync(c->dLightsEx.p + QT_TOTAL, c->lightsEx.data() + QT_TOTAL, sizeof(ptk::PolymorphicLightInfoEx) * (lightBase - QT_TOTAL), hipMemcpyHostToDevice, c->stream));
        }
        if (total) {
            // (a few KB; always: the list is not keyed on a capacity)
            PT_CHECK_HIP(c, c->dEmissiveList.upload(list, c->stream)); PT_CHECK_HIP(c, c->dEmissiveOffsets.upload(offsets, c->stream));
            launch_bake_emissive(c->dsc, c->dEmissiveList.p, c->dEmissiveOffsets.p, (uint)list.size(), total, lightBase, c->dLights.p, c->dLightsEx.p, c->stream);
        }
        // ComputeWeights + ComputeProxyCounts + proxy fill (LightsBaker.hlsl:738-751, 836-948) on the device; NEEType 0 = uniform (1 proxy per light)
        if (N) {
            const uint budget = RTXPT_LIGHTING_SAMPLING_PROXY_RATIO * std::max(N, RTXPT_LIGHTING_MAX_LIGHTS / 10);
            const size_t proxyCapacity = (size_t)budget + N;                       // sum of ceil((budget - N) w_i / W) <= budget - N + N
            (void)budget; (void)proxyCapacity;
            PT_CHECK_HIP(c, c->dLightW.resize(N + 1));
            launch_light_weights(c->dLights.p, c->dLightsEx.p, N, c->dLightW.p, c->lightBoost, c->stream);
            int pr = build_light_proxies(c, c->dLightW.p, nullptr, 0u, 0.f); if (pr != PT_OK) return pr;
        }
    } else { PT_CHECK_HIP(c, c->dLights.resize(1)); PT_CHECK_HIP(c, c->dLightsEx.resize(1)); }
    if (!keepEnv) PT_CHECK_HIP(c, c->dEnvLookup.upload(c->envLookup, c->stream));
    PT_CHECK_HIP(c, c->dSubInstances.upload(c->subInstances, c->stream));
    if (c->dInertBits.p) launch_inert_bits(c->dsc, c->numTris, c->dInertBits.p, c->stream);      // the light links were re-baked: the table follows them (pt_scene.h)
    PT_CHECK_HIP(c, hipEventRecord(e1, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1); c->lightBakeMs = ms; (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    refresh_scene_view(c);
    c->lightsDirty = false;
    return PT_OK;
}
// EnvMapBaker::Update (EnvMapBaker.cpp:425-620): lat-long source + directional lights -> the RGBA16F cube the path tracer and the light baker sample
int bake_env_cube(pt_context* c) {
    ptk::EnvCube& e = c->envCube; memset(&e, 0, sizeof(e)); e.dim = c->envCubeDim; e.mipLevels = ptk::env_cube_mip_levels(e.dim);
    size_t total = 0; for (uint l = 0; l < e.mipLevels; l++) { e.mipOffset[l] = (uint)total; total += 6ull * (e.dim >> l) * (e.dim >> l); }
    PT_CHECK_HIP(c, c->dEnvCube.resize(total));
    // the lights drawn into the cube: what the host handed over in the environment's frame (pt_set_environment_bake), then the loaded scene's own directional
    // lights, taken there by Sample::UpdateLighting's step (pt_env_bake_lights) with THIS bake's cube size and the environment's current orientation;
    // EMB_MAXDIRLIGHTS in all
    std::vector<ptk::EnvDirectionalLight> dirLights = c->envDirLights;
    if (!c->sceneDirLights.empty()) {
        PtEnvMapSceneParams prm; memset(&prm, 0, sizeof(prm)); memcpy(prm.Transform, c->envToWorld.m, 48); prm.Enabled = 1.f;
        std::vector<ptk::EnvDirectionalLight> conv(c->sceneDirLights.size());
        if (pt_env_bake_lights(reinterpret_cast<const PtEnvDirectionalLight*>(c->sceneDirLights.data()), (uint32_t)conv.size(), &prm, e.dim, reinterpret_cast<PtEnvDirectionalLight*>(conv.data())) != PT_OK) return fail(c, PT_ERROR_INVALID_ARGUMENT, "scene directional lights");
        for (auto& l : conv) if (dirLights.size() < 16u) dirLights.push_back(l);
    }
    PT_CHECK_HIP(c, c->dEnvDirLights.upload(dirLights, c->stream));
    if (c->skyEnabled) {          // constants + texture views for the kernels, and room for the half-resolution cloud pre-pass
        ptk::ProceduralSkyContext h = c->sky; h.Transmittance.texels = c->dSkyTex[0].p; h.Scatter.texels = c->dSkyTex[1].p; h.Irradiance.texels = c->dSkyTex[2].p; h.Clouds.texels = c->dSkyTex[3].p;
        PT_CHECK_HIP(c, c->dSky.resize(1)); PT_CHECK_HIP(c, hipMemcpyAsync(c->dSky.p, &h, sizeof(h), hipMemcpyHostToDevice, c->stream)); PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));      // (h is a local)
        PT_CHECK_HIP(c, c->dSkyLowRes.resize(6ull * (e.dim / 2u) * (e.dim / 2u)));
    }
    refresh_scene_view(c);
    launch_env_cube_bake(c->dsc, c->dEnvDirLights.p, (uint)dirLights.size(), c->dEnvCube.p, c->dsc.envCube, c->stream);
    if (c->envCompression) {          // EnvMapBaker.cpp:593-633: the path tracer samples the BC6H cube, the importance baker keeps the uncompressed one
        PT_CHECK_HIP(c, c->dEnvCubeSource.resize(total));
        PT_CHECK_HIP(c, hipMemcpyAsync(c->dEnvCubeSource.p, c->dEnvCube.p, sizeof(ptk::uint2) * total, hipMemcpyDeviceToDevice, c->stream));
        launch_env_cube_compress(c->dEnvCube.p, c->dsc.envCube, c->envCompression, c->stream);
    } else c->dEnvCubeSource.free();
    refresh_scene_view(c);
    PT_CHECK_HIP(c, hipGetLastError());
    c->envCubeDirty = false; c->lightsDirty = true;
    return PT_OK;
}
} // namespace

int prepare(pt_context* c) {
    if (c->texDirty) { int r = upload_textures(c); if (r != PT_OK) return r; refresh_scene_view(c); c->lightsDirty = true; c->envCubeDirty = true; }
    if (c->envEnabled && c->envCubeDirty) { int r = bake_env_cube(c); if (r != PT_OK) return r; }
    if (c->geomDirty) { int r = sync_mirrors(c); if (r != PT_OK) return r; r = finalize_geometry(c); if (r != PT_OK) return r; }      // (re-uploads the host copies of the streams)
    if (c->lightsDirty) { int r = bake_lights(c); if (r != PT_OK) return r; }
    // the camera moved under a frustum boost: weights and proxies only (the lights themselves do not depend on it)
    else if (c->weightsDirty && !c->lights.empty()) {
        launch_light_weights(c->dLights.p, c->dLightsEx.p, (uint)c->lights.size(), c->dLightW.p, c->lightBoost, c->stream);
        int r = build_light_proxies(c, c->dLightW.p, nullptr, 0u, 0.f); if (r != PT_OK) return r;
        refresh_scene_view(c);
    }
    c->weightsDirty = false;
    return PT_OK;
}

// One frame of LightsBaker::UpdateBegin + UpdateEnd for the NEE-AT layer (LightsBaker.cpp:943-962, 985-1075, 1186-1213, 1335-1420) ahead of the frame's path
// tracing; the order and the constants are spelled out in pt_neeat.h. The light set is the baked one; what changes per frame is the global proxy table, the
// tile tables and the jitter. phases: NEEAT_BEGIN = LightsBaker::UpdateBegin (before the frame's G-buffer), NEEAT_END = UpdateEnd (after it, on the frame's
// depth and motion vectors: Sample.cpp:2491-2494; pt_realtime_frame), NEEAT_BOTH = reference mode: nothing happens in between, UpdateEnd reads the depth the
// last traced frame exported (depth == nullptr) and the motion vectors are zero
int neeat_frame(pt_context* c, int phases, const float* depth, const ptk::uint2* motion) {
    pt_context::NeeAt& st = c->neeat;
    const uint N = (uint)c->lights.size();
    // nothing to sample (no lights, or all of them dark): NEE does not run (LightSampler::IsEmpty), the frame is traced without a local layer
    if (!N || !c->numProxies) {
        c->localResX = c->localResY = c->localJitterX = c->localJitterY = c->localMaxLight = 0; c->localRatio = 0.f; c->feedbackRequired = false; st.feedbackFilled = st.lastFeedbackAvailable = false; st.frameOpen = false;
        refresh_scene_view(c); return PT_OK;
    }
    NeeAtFrame F; memset(&F, 0, sizeof(F));
    F.W = c->width; F.H = c->height; F.BW = (F.W + 1) / 2; F.BH = (F.H + 1) / 2; F.tilesX = (F.W + 7) / 8 + 1; F.tilesY = (F.H + 7) / 8 + 1;
    const size_t px = (size_t)F.W * F.H, bpx = (size_t)F.BW * F.BH, tiles = (size_t)F.tilesX * F.tilesY;
    if (phases & NEEAT_BEGIN) {
        // another light set: its indices mean nothing to the old reservoirs and tiles
        if (st.historicTotalLightCount && st.historicTotalLightCount != N) st.feedbackFilled = st.lastFeedbackAvailable = false;
        if (st.W != F.W || st.H != F.H) {               // (re)create the textures: LightsBaker::CreateRenderPasses (LightsBaker.cpp:300-345)
            st.W = F.W; st.H = F.H; st.feedbackFilled = false; st.lastFeedbackAvailable = false;
            PT_CHECK_HIP(c, st.fbW.resize(px)); PT_CHECK_HIP(c, st.fbC.resize(px)); PT_CHECK_HIP(c, st.scW.resize(px)); PT_CHECK_HIP(c, st.scC.resize(px)); PT_CHECK_HIP(c, st.snapW.resize(px)); PT_CHECK_HIP(c, st.snapC.resize(px));
            PT_CHECK_HIP(c, st.blW.resize(bpx)); PT_CHECK_HIP(c, st.blC.resize(bpx)); PT_CHECK_HIP(c, st.local.resize(tiles * RTXPT_LIGHTING_LOCAL_PROXY_COUNT));
            PT_CHECK_HIP(c, hipMemsetAsync(st.fbW.p, 0, 4 * px, c->stream)); PT_CHECK_HIP(c, hipMemsetAsync(st.fbC.p, 0xFF, 4 * px, c->stream));
            PT_CHECK_HIP(c, st.depth.resize(px)); PT_CHECK_HIP(c, st.histDepth.resize(px));
            PT_CHECK_HIP(c, hipMemsetAsync(st.depth.p, 0, 4 * px, c->stream)); PT_CHECK_HIP(c, hipMemsetAsync(st.histDepth.p, 0, 4 * px, c->stream));
        }
        st.prevJitter[0] = st.jitter[0]; st.prevJitter[1] = st.jitter[1];
        neeat_advance_jitter(st.updateCounter, st.jitterF, st.jitter);
        st.updateCounter++;
        st.frameLocalAvailable = st.lastFeedbackAvailable; st.frameFeedbackAvailable = st.feedbackFilled;
        st.framePrevLightCount = st.historicTotalLightCount; st.historicTotalLightCount = N;
        st.frameOpen = true;
    }
    if (!st.frameOpen || st.W != F.W || st.H != F.H) return fail(c, PT_ERROR_NOT_READY, "NEE-AT: UpdateEnd without UpdateBegin of this frame size");
    const bool lastFrameLocalSamplesAvailable = st.frameLocalAvailable, lastFrameFeedbackAvailable = st.frameFeedbackAvailable;
    F.jitterX = st.jitter[0]; F.jitterY = st.jitter[1]; F.jitterPrevX = st.prevJitter[0]; F.jitterPrevY = st.prevJitter[1];
    F.updateCounter = st.updateCounter; F.dropoff = st.dropoff; F.totalLightCount = N; F.historicTotalLightCount = st.framePrevLightCount;
    F.lastFrameFeedbackAvailable = lastFrameFeedbackAvailable ? 1u : 0u; F.lastFrameLocalSamplesAvailable = (lastFrameLocalSamplesAvailable && lastFrameFeedbackAvailable) ? 1u : 0u;
    F.fbW = st.fbW.p; F.fbC = st.fbC.p; F.scW = st.scW.p; F.scC = st.scC.p; F.blW = st.blW.p; F.blC = st.blC.p; F.local = st.local.p;
    F.depth = depth ? depth : st.depth.p; F.motion = motion; F.historyDepth = st.histDepth.p; F.depthDisocclusionThreshold = 1.5f;
    const uint totalMaxFeedbackCount = lastFrameFeedbackAvailable ? ((F.W + 7) / 8) * ((F.H + 7) / 8) * 64u : 0u;
    if (phases & NEEAT_BEGIN) {
        PT_CHECK_HIP(c, st.counters.resize(N + 1)); PT_CHECK_HIP(c, hipMemsetAsync(st.counters.p, 0, 4 * (size_t)(N + 1), c->stream)); F.perLightCounters = st.counters.p;      // ResetLightProxyCounters
        if (lastFrameFeedbackAvailable) launch_neeat_begin(F, st.snapW.p, st.snapC.p, st.preFilter, totalMaxFeedbackCount, c->stream);
        PT_CHECK_HIP(c, st.curW.resize(N + 1)); PT_CHECK_HIP(c, st.histW.resize(N));
        launch_neeat_boost_weights(c->dLightW.p, (lastFrameFeedbackAvailable && st.intensityDeltaMul > 0) ? st.histW.p : nullptr, st.nHist, N, st.intensityDeltaMul, st.curW.p, c->stream);
        int r = build_light_proxies(c, st.curW.p, lastFrameFeedbackAvailable ? st.counters.p : nullptr, totalMaxFeedbackCount, lastFrameFeedbackAvailable ? st.globalFeedbackWeight : 0.f); if (r != PT_OK) return r;
        PT_CHECK_HIP(c, hipMemcpyAsync(st.histW.p, st.curW.p, 4 * (size_t)N, hipMemcpyDeviceToDevice, c->stream)); st.nHist = N;
        st.lastFeedbackAvailable = lastFrameFeedbackAvailable;
    }
    if (!(phases & NEEAT_END)) { PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); return PT_OK; }
    F.perLightCounters = st.counters.p;
    F.samplingProxyCount = c->numProxies; F.proxies = c->dProxyIndices.p;
    // ---- UpdateEnd
    launch_neeat_end(F, c->stream);
    // reference mode: Bridge::ExportSurfaceInit of every pixel of the frame about to be traced
    if (!depth) PT_CHECK_HIP(c, hipMemsetAsync(st.depth.p, 0, 4 * px, c->stream));
    // (the fill passes of realtime mode export nothing: the build pass wrote this frame's depth)
    st.exportDepth = depth == nullptr;
    st.feedbackFilled = true; st.frameOpen = false;
    // what the path tracer binds this frame (the local layer is sampled only once feedback exists: LightsBaker.cpp:1048)
    c->localResX = F.tilesX; c->localResY = F.tilesY; c->localJitterX = st.jitter[0]; c->localJitterY = st.jitter[1]; c->localMaxLight = 0;
    c->localRatio = lastFrameFeedbackAvailable ? st.localRatio : 0.f; c->sscThreshold = st.sscThreshold; c->feedbackRequired = true;
    refresh_scene_view(c);
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

extern "C" {

int32_t pt_create(const PtDeviceDesc* desc, pt_context** out) {
    if (!out) return PT_ERROR_INVALID_ARGUMENT;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PT_ERROR_NO_DEVICE;
    int dev = desc ? desc->deviceOrdinal : 0;
    if (dev < 0 || dev >= ndev) return PT_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(dev) != hipSuccess) return PT_ERROR_HIP;
    pt_context* c = new pt_context();
    c->device = dev; c->shardRank = desc ? desc->shardRank : 0; c->shardCount = (desc && desc->shardCount) ? desc->shardCount : 1;
    if (c->shardRank >= c->shardCount) { delete c; return PT_ERROR_INVALID_ARGUMENT; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return PT_ERROR_HIP; }
    c->streams[0] = c->stream;
    for (uint b = 1; b < PT_PIPELINE_BATCHES; b++) if (hipStreamCreateWithFlags(&c->streams[b], hipStreamNonBlocking) != hipSuccess) { delete c; return PT_ERROR_HIP; }
    if (hipHostMalloc(&c->hostCounters, PT_PIPELINE_BATCHES * sizeof(WaveCounters), hipHostMallocDefault) != hipSuccess) { delete c; return PT_ERROR_HIP; }
    c->serialKernels = desc && (desc->flags & PT_DEVICE_SERIAL_KERNELS);
    // scene builds prefer fast trace, as the reference asks of its driver (Sample.cpp:1093): PLOC + parallel re-insertion + cost-driven wide nodes, all on the
    // device (round 3; PT_DEVICE_HOST_SAH_BUILDER: round 2's host-side binned SAH + re-insertion) unless the host asks for fast builds; pt_animate's rebuilds
    // are always plain PLOC
    c->bvhBuilder = (desc && (desc->flags & PT_DEVICE_PREFER_FAST_BUILD)) ? BVH_BUILDER_PLOC : ((desc && (desc->flags & PT_DEVICE_HOST_SAH_BUILDER)) ? BVH_BUILDER_SAH : BVH_BUILDER_PLOC_OPT);
    { const char* e = getenv("MI355PT_BVH_BUILDER");        // developer A/B switch
      if (e && !strcmp(e, "karras")) c->bvhBuilder = BVH_BUILDER_KARRAS; else if (e && !strcmp(e, "ploc")) c->bvhBuilder = BVH_BUILDER_PLOC; else if (e && !strcmp(e, "sah")) c->bvhBuilder = BVH_BUILDER_SAH; else if (e && (!strcmp(e, "ploc_opt") || !strcmp(e, "device"))) c->bvhBuilder = BVH_BUILDER_PLOC_OPT; }
    { const char* e = getenv("MI355PT_TAIL_PATHS"); if (e) c->tailBelow = (uint)strtoul(e, nullptr, 10); }      // developer A/B switch (pt_set_tail_paths)
    // developer A/B switch (pt_set_fused_traversal)
    { const char* e = getenv("MI355PT_COMPACT_POOL"); if (e) c->compactPool = atoi(e) != 0; }      // developer A/B / test switch, read at pt_create like the others
    { const char* e = getenv("MI355PT_FIRST_VERTEX_IN_PLACE"); if (e) c->firstVertexInPlace = atoi(e) != 0; }      // (0: k_generate in front of every batch, as before)
    { const char* e = getenv("MI355PT_FIRST_VERTEX_PACKETS"); if (e) { const int v = atoi(e); c->firstVertexPackets = v <= 0 ? 0u : (v == 1 ? 1u : 2u); } }      // (0: k_extend_first, one ray per lane pair; 1: 32-ray pair packets; 2: 64-ray packets, one lane per ray)
    { const char* e = getenv("MI355PT_PACKET_PRECULL"); if (e) c->packetPrecull = atoi(e) != 0; }      // (0: the 64-ray packets test every child of a node for every ray)
    // test switches: the steps after which a packet goes to the per-ray kernel, and the entries of its stack (small values send most packets there)
    { const char* e = getenv("MI355PT_PACKET_STEP_CAP"); if (e) c->packetStepCap = (uint)strtoul(e, nullptr, 10); }
    { const char* e = getenv("MI355PT_PACKET_STACK"); if (e) c->packetStack = (uint)strtoul(e, nullptr, 10); }
    { const char* e = getenv("MI355PT_FUSED_TRAVERSAL"); if (e) c->fusedTraversal = (uint)strtoul(e, nullptr, 10); }
    { const char* e = getenv("MI355PT_OCCLUSION_SLOT_ORDER"); if (e) c->occlusionSlotOrder = atoi(e) != 0; }      // developer A/B / test switch (0: child slots in collapse order, as before)
    { const char* e = getenv("MI355PT_DROP_INERT_TERMINAL"); if (e) c->dropInertTerminal = atoi(e) != 0; }      // developer A/B / test switch (0: every terminal hit is shaded, as before)
    // test switch: iterations after which the tail kernel hands a ray back (0: T8_TAIL_DEFER); a small value sends most rays through the hand-back path
    { const char* e = getenv("MI355PT_TAIL_DEFER"); if (e) c->tailDefer = (uint)strtoul(e, nullptr, 10); }
    // PT_DEVICE_TEXTURES_ON_DEVICE: pt_set_materials converts the textures and builds their chains on the device (pt_texture_ingest.hip); the environment overrides the flag
    c->deviceTextures = desc && (desc->flags & PT_DEVICE_TEXTURES_ON_DEVICE);
    { const char* e = getenv("MI355PT_DEVICE_TEXTURES"); if (e) c->deviceTextures = atoi(e) != 0; }
    // test switch: the bytes of the pinned staging buffer (both halves together), so that chunk boundaries fall inside small textures
    { const char* e = getenv("MI355PT_TEXTURE_STAGING_BYTES"); if (e) c->texStagingBytes = std::max<size_t>(64u, (size_t)strtoull(e, nullptr, 10)); }
    memset(&c->dsc, 0, sizeof(c->dsc)); memset(&c->cam, 0, sizeof(c->cam)); memset(&c->bvh, 0, sizeof(c->bvh));
    pt_default_settings(reinterpret_cast<::PtSettings*>(&c->S));
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; memcpy(c->envToWorld.m, I, 48); memcpy(c->envToLocal.m, I, 48); c->envColorMul = ptk::make_float3(1.0f / ptk::kEnvMapRadianceScale);      // no params = tint 1, intensity 1: the cube holds radiance x 1/4
    if (c->dCounters.resize(PT_PIPELINE_BATCHES) != hipSuccess) { delete c; return PT_ERROR_HIP; }
    *out = c;
    return PT_OK;
}
int32_t pt_destroy(pt_context* c) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream);
    (void)pt_comm_destroy(c);
    c->dSpHeader.free(); c->dSpThroughput.free(); c->dSpPlanes.free(); c->dSpRadiance.free(); c->dSpMotion.free(); c->dSpDepth.free(); c->dSpHitT.free(); c->dSpMark.free(); c->dSpNewL.free(); c->dSpScratch.free();
    c->dDnRRDiff.free(); c->dDnRRSpec.free(); c->dDnRRSpecMV.free(); c->dDnRRNormal.free(); c->dDnMotion.free(); c->dDnViewZ.free(); c->dDnRoughness.free(); c->dDnNormal.free(); c->dDnDiff.free(); c->dDnSpec.free(); c->dDnDisocclusion.free(); c->dDnHistoryClamp.free();
    relax_free(c); taa_free(c); bloom_free(c); taau_free(c); adaptive_free(c); accum_denoise_free(c);
    skin_drop(c); for (int e = 0; e < 2; e++) if (c->skinEvents[e]) (void)hipEventDestroy(c->skinEvents[e]);
    c->neeat.free(); c->dLocalTable.free(); c->dFbWeight.free(); c->dFbCand.free(); c->dSq3.free();
    c->staging.free(); c->dLightW.free(); c->dProxyOffsets.free(); if (c->dScanTemp) (void)hipFree(c->dScanTemp);
    if (c->bvhAllocated) bvh_free(c->bvh);
    c->dIndices.free(); c->dNormals.free(); c->dTangents.free(); c->dProxyCounters.free(); c->dProxyIndices.free(); c->dEnvLookup.free(); c->dOwned.free(); c->dQueue[0].free(); c->dQueue[1].free();
    c->dPrevPositions.free(); c->dPrevInstances.free(); c->dEmissiveList.free(); c->dEmissiveOffsets.free(); c->dPositions.free(); c->dUvs.free(); c->dGeometries.free(); c->dInstances.free(); c->dSubInstances.free(); c->dSubInstToInstGeom.free();
    c->dPrimInfo.free(); c->dShadeTris.free(); c->dInertBits.free(); c->dAlphaPlanes.free(); c->dAlphaPool.free(); c->dMaterials.free(); c->dTexInfos.free(); c->dTexels.free(); c->dEnvCube.free(); c->dEnvCubeSource.free(); c->dEnvImageCube.free(); c->dEnvDirLights.free(); c->dLights.free(); c->dLightsEx.free(); c->dS0.free(); c->dS1.free(); c->dS2.free(); c->dS3.free(); c->dS4.free();
    c->dHit.free(); c->dS0b.free(); c->dS1b.free(); c->dS3b.free(); c->dS4b.free(); c->dHitb.free(); c->dSq0.free(); c->dSq1.free(); c->dSq2.free(); c->dAccum.free(); c->dScratch4.free(); c->dCounters.free(); c->dTravSpill.free(); c->dTaskQ.free(); c->dTravCounts.free(); c->dResolveList.free(); c->dFirstLeftover.free(); c->dBestKey.free(); c->dResolveListSh.free(); c->dBestKeySh.free(); c->dTaskQSh.free();
    for (uint b = 1; b < PT_PIPELINE_BATCHES; b++) (void)hipStreamDestroy(c->streams[b]);
    (void)hipStreamDestroy(c->stream); (void)hipHostFree(c->hostCounters);
    delete c;
    return PT_OK;
}
const char* pt_get_last_error(pt_context* c) { return c ? c->lastError.c_str() : "null context"; }

int32_t pt_set_geometry(pt_context* c, const PtGeometryBuffers* b, const PtGeometryDesc* geoms, uint32_t nGeoms, const PtMeshDesc* meshes, uint32_t nMeshes) {
    if (!c || !b || !geoms || !meshes) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (!b->indices || !b->positions) return fail(c, PT_ERROR_INVALID_ARGUMENT, "indices and positions are required");
    for (uint32_t g = 0; g < nGeoms; g++) {
        if ((size_t)geoms[g].indexOffset + geoms[g].numIndices > b->numIndices || (size_t)geoms[g].vertexOffset + geoms[g].numVertices > b->numVertices || geoms[g].numIndices % 3)
            return fail(c, PT_ERROR_INVALID_ARGUMENT, "geometry range outside the supplied streams");
        if ((geoms[g].flags & PT_GEOM_HAS_UV) && !b->uvs) return fail(c, PT_ERROR_INVALID_ARGUMENT, "geometry has uv flag but no uv stream");
        if ((geoms[g].flags & PT_GEOM_HAS_NORMAL) && !b->normals) return fail(c, PT_ERROR_INVALID_ARGUMENT, "geometry has normal flag but no normal stream");
        if ((geoms[g].flags & PT_GEOM_HAS_TANGENT) && !b->tangents) return fail(c, PT_ERROR_INVALID_ARGUMENT, "geometry has tangent flag but no tangent stream");
        const uint32_t* idx = b->indices + geoms[g].indexOffset;      // an out-of-range index would be an out-of-bounds read on the device
        for (uint32_t k = 0; k < geoms[g].numIndices; k++) if (idx[k] >= geoms[g].numVertices) return fail(c, PT_ERROR_INVALID_ARGUMENT, "index outside the geometry's vertex range");
    }
    for (uint32_t m = 0; m < nMeshes; m++)
        if ((size_t)meshes[m].firstGeometry + meshes[m].numGeometries > nGeoms) return fail(c, PT_ERROR_INVALID_ARGUMENT, "mesh references geometries outside the supplied array");
    uint nv = b->numVertices;
    c->indices.assign(b->indices, b->indices + b->numIndices);
    c->positions.assign(b->positions, b->positions + 3 * (size_t)nv);
    c->uvs.assign(nv, ptk::make_float2(0, 0)); if (b->uvs) memcpy(c->uvs.data(), b->uvs, 8 * (size_t)nv);
    c->normals.assign(nv, 0); if (b->normals) memcpy(c->normals.data(), b->normals, 4 * (size_t)nv);
    c->tangents.assign(nv, 0); if (b->tangents) memcpy(c->tangents.data(), b->tangents, 4 * (size_t)nv);
    c->geometries.resize(nGeoms); memcpy(c->geometries.data(), geoms, sizeof(GeometryDesc) * nGeoms);
    c->meshes.resize(nMeshes); memcpy(c->meshes.data(), meshes, sizeof(MeshDesc) * nMeshes);
    c->geomDirty = true;
    skin_drop(c); c->mirrorsStale = false; c->mirrorRanges.clear();      // a new scene: the skinning description was of another one, and the host copies above are the truth again
    relax_drop_history(c); taa_drop_history(c); taau_drop_history(c);      // a new scene: the denoiser's and the two resolves' histories are of another one
    return PT_OK;
}
int32_t pt_set_instances(pt_context* c, const PtInstanceDesc* inst, uint32_t n) {
    if (!c || (!inst && n)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    c->instances.resize(n); if (n) memcpy(c->instances.data(), inst, sizeof(InstanceDesc) * n);
    c->geomDirty = true;
    return PT_OK;
}
int32_t pt_set_materials(pt_context* c, const ::PTMaterialData* mats, uint32_t nMats, const PtTextureDesc* tex, uint32_t nTex) {
    if (!c || (!mats && nMats) || (!tex && nTex)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    c->materials.resize(nMats); if (nMats) memcpy(c->materials.data(), mats, 128 * (size_t)nMats);
    (void)hipSetDevice(c->device);
    const auto t0 = std::chrono::steady_clock::now();
    c->textures.clear(); c->texFormats.clear();
    for (uint32_t i = 0; i < nTex; i++) {
        const PtTextureDesc& d = tex[i];
        if (!d.pixels || !d.width || !d.height || d.format > 2) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bad texture descriptor");
        if (d.width > 32768u || d.height > 32768u) return fail(c, PT_ERROR_UNSUPPORTED, "textures above 32768 texels per side are not supported (16 mip levels)");
        HostTexture t;
        if (c->deviceTextures) { t.w = d.width; t.h = d.height; t.mipLevels = texi_level_count(t.w, t.h); }      // sizes only: the texels are made on the device, below
        else host_convert_texture(d, t);
        c->textures.push_back(std::move(t)); c->texFormats.push_back(d.format);
    }
    for (uint32_t m = 0; m < nMats; m++) {
        const ptk::PTMaterialData& mm = c->materials[m];
        auto chk = [&](uint flag, uint word) { return !(mm.Flags & flag) || (word & 0xFFFFu) < nTex; };
        if (!chk(PTMaterialFlags_UseBaseOrDiffuseTexture, mm.BaseOrDiffuseTextureIndex) || !chk(PTMaterialFlags_UseEmissiveTexture, mm.EmissiveTextureIndex) ||
            !chk(PTMaterialFlags_UseNormalTexture, mm.NormalTextureIndex) || !chk(PTMaterialFlags_UseMetalRoughOrSpecularTexture, mm.MetalRoughOrSpecularTextureIndex) ||
            !chk(PTMaterialFlags_UseTransmissionTexture, mm.TransmissionTextureIndex))
            return fail(c, PT_ERROR_INVALID_ARGUMENT, "material references a missing texture");
    }
    // the device path ingests here, while the caller's pixels are valid: no copy of them is kept (texDirty stays raised for the environment image's place in the new pool)
    if (c->deviceTextures) { int r = tex_ingest_all(c, tex, nTex); if (r != PT_OK) return r; }
    c->texHostMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->texDirty = true; c->geomDirty = true;
    return PT_OK;
}
int32_t pt_update_texture(pt_context* c, uint32_t texture, const PtTextureDesc* d) {
    if (!c || !d) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (texture >= c->textures.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_update_texture: no such texture in the last pt_set_materials");
    if (!d->pixels || d->width != c->textures[texture].w || d->height != c->textures[texture].h || d->format != c->texFormats[texture])
        return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_update_texture: the new pixels must have the texture's width, height and format");
    if (c->deviceTextures) {
        int r = tex_update_one(c, texture, d); if (r != PT_OK) return r;
        refresh_scene_view(c);                       // (the alpha pool may have been allocated again)
    } else {
        // correctness only: the one texture converted on the host, then everything pooled, uploaded and finalised again (a plane may change its format and move the others)
        (void)hipSetDevice(c->device);
        const auto t0 = std::chrono::steady_clock::now();
        host_convert_texture(*d, c->textures[texture]);
        c->texHostMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        c->texDirty = true; c->geomDirty = true;
    }
    c->lightsDirty = true;                           // the emissive bake may read the texture
    return PT_OK;
}
// orientation and colour multiplier of the environment (EnvMapSceneParams), shared by the two image setters
static void set_env_params(pt_context* c, const PtEnvMapSceneParams* params) {
    if (params) {
        memcpy(c->envToWorld.m, params->Transform, 48);
        memset(&c->envToLocal, 0, sizeof(float3x4));
        for (int r = 0; r < 3; r++) for (int k = 0; k < 3; k++) c->envToLocal.m[r * 4 + k] = c->envToWorld.m[k * 4 + r];   // rotation inverse = transpose
        c->envColorMul = ptk::make_float3(params->ColorMultiplier[0], params->ColorMultiplier[1], params->ColorMultiplier[2]);
    // no params: identity orientation, the supplied radiance as it is (ColorMultiplier = 1 / c_envMapRadianceScale undoes the cube's 1/4)
    } else {
        const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; memcpy(c->envToWorld.m, I, 48); memcpy(c->envToLocal.m, I, 48);
        c->envColorMul = ptk::make_float3(1.0f / ptk::kEnvMapRadianceScale);
    }
}
static bool env_has_image(const pt_context* c) { return c->envTex.w != 0u || c->envImageCubeDim != 0u; }
int32_t pt_set_environment(pt_context* c, const float* rgb, uint32_t w, uint32_t h, const PtEnvMapSceneParams* params) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    c->envImageCubeDim = 0; c->dEnvImageCube.free();          // one image source at a time: a lat-long image replaces a cube-map source
    c->envEnabled = (w != 0 && h != 0 && rgb && (!params || params->Enabled != 0.f));
    if (!c->envEnabled) { c->envTex.w = c->envTex.h = 0; c->envTex.mips.clear(); if (c->skyEnabled && (!params || params->Enabled != 0.f)) c->envEnabled = true; }      // (a procedural sky needs no image)
    else {
        HostTexture& t = c->envTex; t.w = w; t.h = h; t.mips.clear(); t.mips.resize(1); t.mips[0].resize((size_t)w * h);
        for (size_t i = 0; i < (size_t)w * h; i++) t.mips[0][i] = ptk::make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 1.f);
        t.mipLevels = 1;                                   // the bake reads mip 0 only (EnvMapBaker.hlsl:98-110: SampleLevel(.., 0))
    }
    set_env_params(c, params);
    c->texDirty = true; c->lightsDirty = true; c->envCubeDirty = true;
    return PT_OK;
}
int32_t pt_set_environment_cube(pt_context* c, const float* rgbaFaces, uint32_t dim, const PtEnvMapSceneParams* params) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (dim > 16384u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "cube-map source: at most 16384 texels per side");
    c->envTex.w = c->envTex.h = 0; c->envTex.mips.clear();    // one image source at a time
    c->envEnabled = (dim != 0 && rgbaFaces && (!params || params->Enabled != 0.f));
    if (!c->envEnabled) { c->envImageCubeDim = 0; c->dEnvImageCube.free(); if (c->skyEnabled && (!params || params->Enabled != 0.f)) c->envEnabled = true; }
    // stored as the RGBA16F texels a BC6H / RGBA16F cube file decodes to (a RGBA32F file is rounded to them)
    else {
        const size_t n = 6ull * dim * dim; std::vector<ptk::uint2> h(n);
        for (size_t i = 0; i < n; i++) h[i] = ptk::env_pack_rgba16f(ptk::make_float4(rgbaFaces[4 * i], rgbaFaces[4 * i + 1], rgbaFaces[4 * i + 2], rgbaFaces[4 * i + 3]));
        PT_CHECK_HIP(c, c->dEnvImageCube.resize(n)); PT_CHECK_HIP(c, hipMemcpy(c->dEnvImageCube.p, h.data(), n * sizeof(ptk::uint2), hipMemcpyHostToDevice));
        c->envImageCubeDim = dim;
    }
    set_env_params(c, params);
    c->texDirty = true; c->lightsDirty = true; c->envCubeDirty = true;
    return PT_OK;
}
int32_t pt_set_procedural_sky(pt_context* c, const PtProceduralSkyConstants* consts, const PtProceduralSkyTextures* tex) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    static_assert(sizeof(PtProceduralSkyConstants) == sizeof(ptk::ProceduralSkyConstants), "ProceduralSkyConstants layout");
    if (!consts) {
        if (c->skyEnabled) { c->skyEnabled = false; if (!env_has_image(c)) c->envEnabled = false; c->envCubeDirty = true; c->lightsDirty = true; c->texDirty = true; }
        return PT_OK;
    }
    if (tex) {
        const PtSkyTexture* t[4] = {&tex->transmittance, &tex->scattering, &tex->irradiance, &tex->clouds}; ptk::SkyTexture* dst[4] = {&c->sky.Transmittance, &c->sky.Scatter, &c->sky.Irradiance, &c->sky.Clouds};
        for (int i = 0; i < 4; i++) {
            if (!t[i]->rgba || !t[i]->width || !t[i]->height || !t[i]->depth || t[i]->width > 4096u || t[i]->height > 4096u || t[i]->depth > 4096u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "procedural sky: every look-up texture needs RGBA float texels and sizes in [1, 4096]");
            if ((i == 0 || i == 2) && t[i]->depth != 1u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "procedural sky: the transmittance and irradiance textures are 2-D (depth 1)");
        }
        for (int i = 0; i < 4; i++) {
            const size_t n = (size_t)t[i]->width * t[i]->height * t[i]->depth;
            PT_CHECK_HIP(c, c->dSkyTex[i].resize(n)); PT_CHECK_HIP(c, hipMemcpy(c->dSkyTex[i].p, t[i]->rgba, n * sizeof(ptk::float4), hipMemcpyHostToDevice));
            dst[i]->texels = nullptr; dst[i]->w = t[i]->width; dst[i]->h = t[i]->height; dst[i]->d = t[i]->depth; dst[i]->_pad = 0u;
        }
    } else if (!c->dSkyTex[0].p) return fail(c, PT_ERROR_INVALID_ARGUMENT, "procedural sky: no look-up textures have been set yet");
    memcpy(&c->sky.Consts, consts, sizeof(ptk::ProceduralSkyConstants));
    if (!c->envEnabled) {          // a sky without pt_set_environment: identity orientation, the baked radiance as it is
        if (!env_has_image(c)) { const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; memcpy(c->envToWorld.m, I, 48); memcpy(c->envToLocal.m, I, 48); c->envColorMul = ptk::make_float3(1.0f / ptk::kEnvMapRadianceScale); }
        c->envEnabled = true; c->texDirty = true;
    }
    c->skyEnabled = true; c->envCubeDirty = true; c->lightsDirty = true;
    return PT_OK;
}
int32_t pt_set_environment_bake(pt_context* c, uint32_t cubeDim, const PtEnvDirectionalLight* lights, uint32_t n) {
    if (!c || (!lights && n)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (cubeDim && (cubeDim < 16u || cubeDim > 8192u || (cubeDim & (cubeDim - 1u)))) return fail(c, PT_ERROR_INVALID_ARGUMENT, "cube resolution must be a power of two in [16, 8192]");
    if (n > 16u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "at most 16 directional lights are baked into the environment cube (EnvMapBaker.hlsl: EMB_MAXDIRLIGHTS)");
    if (cubeDim) c->envCubeDim = cubeDim;
    static_assert(sizeof(PtEnvDirectionalLight) == sizeof(ptk::EnvDirectionalLight), "EnvDirectionalLight layout");
    c->envDirLights.resize(n); if (n) memcpy(c->envDirLights.data(), lights, sizeof(ptk::EnvDirectionalLight) * n);
    c->envCubeDirty = true; c->lightsDirty = true;
    return PT_OK;
}
int32_t pt_set_scene_directional_lights(pt_context* c, const PtEnvDirectionalLight* worldLights, uint32_t n) {
    if (!c || (!worldLights && n)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (n > 16u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "at most 16 directional lights are baked into the environment cube (EnvMapBaker.hlsl: EMB_MAXDIRLIGHTS)");
    c->sceneDirLights.resize(n); if (n) memcpy(c->sceneDirLights.data(), worldLights, sizeof(ptk::EnvDirectionalLight) * n);
    c->envCubeDirty = true; c->lightsDirty = true;
    return PT_OK;
}
int32_t pt_set_environment_compression(pt_context* c, uint32_t quality) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (quality > 2u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "BC6U compression: 0 = off, 1 = fast (the reference's default on D3D12), 2 = quality (two-region modes)");
    if (c->envCompression != quality) { c->envCompression = quality; c->envCubeDirty = true; c->lightsDirty = true; }
    return PT_OK;
}
int32_t pt_set_local_light_sampling(pt_context* c, const uint32_t* table, uint32_t resX, uint32_t resY, uint32_t jitterX, uint32_t jitterY, float localToGlobalSampleRatio,
                                    float screenSpaceVsWorldSpaceThreshold, int32_t temporalFeedback) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (c->neeat.enabled) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_neeat is on: the baker in the loop writes the tile tables itself (pt_set_neeat(ctx, 0, ...) first)");
    (void)hipSetDevice(c->device);
    const uint N = ptk::RTXPT_LIGHTING_LOCAL_PROXY_COUNT, TILE_PX = ptk::RTXPT_LIGHTING_SAMPLING_BUFFER_TILE_SIZE;
    if (!(localToGlobalSampleRatio >= 0.f && localToGlobalSampleRatio <= 0.95f)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "LocalToGlobalSampleRatio: 0 .. 0.95 (SampleUI.cpp:750)");
    if (table) {
        if (!resX || !resY || jitterX >= TILE_PX || jitterY >= TILE_PX) return fail(c, PT_ERROR_INVALID_ARGUMENT, "local sampling table: resolution in tiles of 8 x 8 pixels, jitter below the tile size");
        uint maxLight = 0;
        // SampleLocalPDF searches the tile by light index (LightingAlgorithms.hlsli:654): the entries must be sorted
        for (size_t t = 0; t < (size_t)resX * resY; t++) for (uint k = 0; k < N; k++) {
            const uint light = table[t * N + k] >> 9;
            if (k && light < (table[t * N + k - 1] >> 9)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "local sampling table: a tile's entries must be sorted by light index");
            if (light > maxLight) maxLight = light;
        }
        PT_CHECK_HIP(c, c->dLocalTable.upload(table, (size_t)resX * resY * N, c->stream));
        PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
        c->localResX = resX; c->localResY = resY; c->localJitterX = jitterX; c->localJitterY = jitterY; c->localMaxLight = maxLight;
    } else { c->localResX = c->localResY = c->localJitterX = c->localJitterY = c->localMaxLight = 0; }
    c->localRatio = localToGlobalSampleRatio; c->sscThreshold = screenSpaceVsWorldSpaceThreshold; c->feedbackRequired = temporalFeedback != 0;
    refresh_scene_view(c);
    return PT_OK;
}
int32_t pt_get_light_feedback(pt_context* c, uint32_t sample, float* totalWeight, uint32_t* candidates) {
    if (!c || !totalWeight || !candidates) return PT_ERROR_INVALID_ARGUMENT;
    if (sample >= c->fbSamples) return fail(c, PT_ERROR_NOT_READY, "no feedback for that sample: pt_set_local_light_sampling(temporalFeedback = 1) or pt_set_neeat, then pt_render");
    if (c->neeat.enabled && (!c->neeat.fbW.p || c->neeat.W != c->width || c->neeat.H != c->height)) return fail(c, PT_ERROR_NOT_READY, "no NEE-AT frame of this size yet: pt_render first");
    (void)hipSetDevice(c->device);
    const size_t plane = (size_t)c->width * c->height;
    const float* w = c->neeat.enabled ? c->neeat.fbW.p : c->dFbWeight.p + plane * sample; const uint* cand = c->neeat.enabled ? c->neeat.fbC.p : c->dFbCand.p + plane * sample;
    PT_CHECK_HIP(c, hipMemcpy(totalWeight, w, 4 * plane, hipMemcpyDeviceToHost));
    PT_CHECK_HIP(c, hipMemcpy(candidates, cand, 4 * plane, hipMemcpyDeviceToHost));
    return PT_OK;
}
int32_t pt_set_neeat(pt_context* c, int32_t enable, float globalTemporalFeedbackWeight, float localToGlobalSampleRatio, float screenSpaceVsWorldSpaceThreshold, int32_t preFilter) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (enable && (!(globalTemporalFeedbackWeight >= 0.f && globalTemporalFeedbackWeight <= 0.95f) || !(localToGlobalSampleRatio >= 0.f && localToGlobalSampleRatio <= 0.95f)))
        return fail(c, PT_ERROR_INVALID_ARGUMENT, "global feedback weight and local-to-global ratio: 0 .. 0.95 (SampleUI.cpp:747-750)");
    (void)hipSetDevice(c->device);
    pt_context::NeeAt& st = c->neeat;
    if (st.enabled && !enable) {                 // back to the plain global sampler: no local layer, no feedback, the proxy table of the bake
        c->localResX = c->localResY = c->localJitterX = c->localJitterY = c->localMaxLight = 0; c->localRatio = 0.f; c->feedbackRequired = false; c->lightsDirty = true;
    }
    if (st.enabled != (enable != 0)) c->fbSamples = 0;      // the planes pt_get_light_feedback reads change hands: nothing is valid until the next pt_render
    st.enabled = enable != 0; st.globalFeedbackWeight = globalTemporalFeedbackWeight; st.localRatio = localToGlobalSampleRatio; st.sscThreshold = screenSpaceVsWorldSpaceThreshold; st.preFilter = preFilter != 0;
    refresh_scene_view(c);
    return PT_OK;
}
int32_t pt_set_view_projection(pt_context* c, const float* worldToClipRowMajor16) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    pt_context::NeeAt& st = c->neeat;
    if (worldToClipRowMajor16) { for (int r = 0; r < 4; r++) { st.clipZ[r] = worldToClipRowMajor16[4 * r + 2]; st.clipW[r] = worldToClipRowMajor16[4 * r + 3]; } st.haveClip = true; }
    else { memset(st.clipZ, 0, 16); memset(st.clipW, 0, 16); st.haveClip = false; }
    refresh_scene_view(c);
    return PT_OK;
}
int32_t pt_neeat_reset(pt_context* c) { if (!c) return PT_ERROR_INVALID_ARGUMENT; c->neeat.reset(); c->fbSamples = 0; return PT_OK; }
int32_t pt_get_neeat_tables(pt_context* c, uint32_t tilesXY[2], uint32_t jitterXY[2], uint32_t* table, uint32_t tableCapacityWords) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    const pt_context::NeeAt& st = c->neeat;
    if (!st.enabled || !st.W) return fail(c, PT_ERROR_NOT_READY, "no NEE-AT frame yet: pt_set_neeat, then pt_render");
    (void)hipSetDevice(c->device);
    const uint tx = (st.W + 7) / 8 + 1, ty = (st.H + 7) / 8 + 1;
    if (tilesXY) { tilesXY[0] = tx; tilesXY[1] = ty; }
    if (jitterXY) { jitterXY[0] = st.jitter[0]; jitterXY[1] = st.jitter[1]; }
    if (table) {
        if ((size_t)tableCapacityWords < (size_t)tx * ty * RTXPT_LIGHTING_LOCAL_PROXY_COUNT) return fail(c, PT_ERROR_INVALID_ARGUMENT, "table buffer too small");
        PT_CHECK_HIP(c, hipMemcpy(table, st.local.p, 4 * (size_t)tx * ty * RTXPT_LIGHTING_LOCAL_PROXY_COUNT, hipMemcpyDeviceToHost));
    }
    return PT_OK;
}
int32_t pt_set_light_importance_boost(pt_context* c, const float* viewProjRowMajor16, float frustumMul, float frustumFadeDistance) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (viewProjRowMajor16 && !(frustumMul >= 0.f && frustumFadeDistance >= 0.f)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "frustum boost: multiplier and fade distance must not be negative");
    ptk::LightFrustumBoost b; memset(&b, 0, sizeof(b));
    if (viewProjRowMajor16 && frustumMul > 0.f) { ptk::light_frustum_planes_from_viewproj(viewProjRowMajor16, b.planes); b.mul = frustumMul; b.fadeDistance = frustumFadeDistance; }
    if (memcmp(&b, &c->lightBoost, sizeof(b)) != 0) { c->lightBoost = b; c->weightsDirty = true; }
    return PT_OK;
}
int32_t pt_set_lights(pt_context* c, const ::PolymorphicLightInfo* lights, const ::PolymorphicLightInfoEx* ex, uint32_t n) {
    if (!c || (!lights && n)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    c->analyticLights.clear();
    for (uint32_t i = 0; i < n; i++) {
        PolymorphicLightInfoFull f; memcpy(&f.Base, &lights[i], 32);
        if (ex) memcpy(&f.Extended, &ex[i], 16); else memset(&f.Extended, 0, 16);
        uint type = DecodeLightType(f.Base);
        // sphere lights are the enabled analytic type; a point-type record (ConvertLight of a light without radius) has its type compiled out in the
        // reference (PolymorphicLightPTConfig.h:17-22) and is carried as the reference carries it: a slot in the buffer with no power and empty samples
        if (type != kSphere && type != kPoint) return fail(c, PT_ERROR_UNSUPPORTED, "only sphere (and inert point-type) analytic light records are accepted (PolymorphicLightPTConfig.h:17-22)");
        c->analyticLights.push_back(f);
    }
    c->lightsDirty = true;
    return PT_OK;
}

int32_t pt_bridge_camera(uint32_t w, uint32_t h, const float pos[3], const float dir[3], const float up[3], float fovY, float nearZ, float farZ, float focalDistance,
                         float apertureRadius, const float jitter[2], ::PathTracerCameraData* out) {
    if (!out || !pos || !dir || !up || !w || !h) return PT_ERROR_INVALID_ARGUMENT;
    // PathTracerShared.h:109-141 (donut::math normalize = v / length(v))
    auto nrm = [](ptk::float3 v) { float l = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); return ptk::make_float3(v.x / l, v.y / l, v.z / l); };
    ptk::PathTracerCameraData d; memset(&d, 0, sizeof(d));
    float aspect = (float)w / (float)h;
    d.FocalDistance = focalDistance; d.PosW = ptk::make_float3(pos[0], pos[1], pos[2]); d.NearZ = nearZ; d.FarZ = farZ; d.AspectRatio = aspect;
    d.ViewportSize = ptk::make_uint2(w, h);
    ptk::float3 camDir = ptk::make_float3(dir[0], dir[1], dir[2]), camUp = ptk::make_float3(up[0], up[1], up[2]);
    d.DirectionW = nrm(camDir);
    d.CameraW = nrm(camDir) * d.FocalDistance;
    d.CameraU = nrm(cross(d.CameraW, camUp));
    d.CameraV = nrm(cross(d.CameraU, d.CameraW));
    const float ulen = d.FocalDistance * std::tan(fovY * 0.5f) * d.AspectRatio;
    d.CameraU = d.CameraU * ulen;
    const float vlen = d.FocalDistance * std::tan(fovY * 0.5f);
    d.CameraV = d.CameraV * vlen;
    d.ApertureRadius = apertureRadius;
    d.PixelConeSpreadAngle = std::atan(2.0f * std::tan(fovY * 0.5f) / (float)h);
    d.Jitter = ptk::make_float2(jitter ? jitter[0] : 0.f, jitter ? -jitter[1] : 0.f);
    memcpy(out, &d, sizeof(d));
    return PT_OK;
}
int32_t pt_set_camera(pt_context* c, const ::PathTracerCameraData* cam) {
    if (!c || !cam) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    memcpy(&c->cam, cam, sizeof(c->cam));
    return PT_OK;
}
int32_t pt_default_settings(::PtSettings* s) {
    if (!s) return PT_ERROR_INVALID_ARGUMENT;
    memset(s, 0, sizeof(*s));
    s->bounceCount = 8; s->diffuseBounceCount = 8; s->perPixelJitterAAScale = 1.0f; s->texLODBias = -1.0f; s->fireflyFilterThreshold = 0.f; s->envMapDiffuseSampleMIPLevel = 0.f;
    s->NEEEnabled = 1; s->NEEType = 1; s->NEECandidateSamples = 5; s->NEEFullSamples = 1; s->enableRussianRoulette = 1; s->nestedDielectricsQuality = 1;
    s->enableLDSamplerForBSDF = 1; s->diffuseBrdf = 2; s->useFp16Types = 1;      // SampleUI.h:182: UseFp16Types = true
    return PT_OK;
}
int32_t pt_set_settings(pt_context* c, const ::PtSettings* s) {
    if (!c || !s) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    // NEEType 2 (NEE-AT): the global table is built as for type 1 (LightsBaker.hlsl:920-923 treats every type but 0 alike; the feedback-weighted boost of the
    // global proxies belongs to the baker's feedback passes, which the host does not have yet); the local layer and the feedback come from
    // pt_set_local_light_sampling
    if (s->NEEType > 2) return fail(c, PT_ERROR_INVALID_ARGUMENT, "NEEType: 0 (uniform), 1 (power) or 2 (NEE-AT)");
    if (s->NEECandidateSamples == 0 || s->NEECandidateSamples > 63) return fail(c, PT_ERROR_INVALID_ARGUMENT, "NEECandidateSamples must be in [1,63]");
    if (s->nestedDielectricsQuality > 2 || (s->diffuseBrdf != 0 && s->diffuseBrdf != 2) || s->bounceCount > 96 || s->useFp16Types > 1) return fail(c, PT_ERROR_INVALID_ARGUMENT, "setting out of range");
    if (c->S.NEEEnabled != s->NEEEnabled || c->S.NEEType != s->NEEType) c->lightsDirty = true;
    memcpy(&c->S, s, sizeof(c->S));
    ptk::stf_set_launch_filter(c->S, c->stf.enable != 0u, c->stf.filter);      // the pad word is the library's: the texture filter of the launches (pt_set_texture_filtering), whatever the caller left in it
    return PT_OK;
}
// RTXPT_STOCHASTIC_TEXTURE_FILTERING_ENABLE and the three STF settings of PathTracerConstants (PathTracerShared.h:88-90; defaults SampleUI.h:185-187)
int32_t pt_texture_filtering_default_params(PtTextureFiltering* p) {
    if (!p) return PT_ERROR_INVALID_ARGUMENT;
    p->enable = 0u; p->filter = PT_STF_FILTER_LINEAR; p->magnification = 0u; p->gaussianSigma = 0.3f;
    return PT_OK;
}
int32_t pt_set_texture_filtering(pt_context* c, const PtTextureFiltering* p) {
    if (!c || !p) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (p->enable > 1u || p->filter > PT_STF_FILTER_GAUSSIAN || p->magnification > 3u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "texture filtering: enable 0 / 1, filter 0 .. 3 (PT_STF_FILTER_*), magnification 0 .. 3");
    if (p->filter == PT_STF_FILTER_GAUSSIAN) return fail(c, PT_ERROR_UNSUPPORTED, "texture filtering: the Gaussian filter is not built (rtxpt_amd/csrc/pt_stf.h)");
    if (p->magnification != 0u) return fail(c, PT_ERROR_UNSUPPORTED, "texture filtering: only the Default magnification method (0) is built");
    (void)hipSetDevice(c->device);
    const bool changed = c->stf.enable != p->enable || (p->enable && c->stf.filter != p->filter);
    c->stf.enable = p->enable; c->stf.filter = p->filter; c->stf.magnification = p->magnification; c->stf.gaussianSigma = p->gaussianSigma;
    ptk::stf_set_launch_filter(c->S, c->stf.enable != 0u, c->stf.filter);
    if (changed && c->width) return pt_reset_accumulation(c);      // another estimator: what was accumulated is not its average
    return PT_OK;
}
int32_t pt_resize(pt_context* c, uint32_t w, uint32_t h) {
    if (!c || !w || !h || w > 65535 || h > 65535) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bad size");
    (void)hipSetDevice(c->device);
    if (w != c->width || h != c->height) { relax_drop_history(c); taa_drop_history(c); bloom_drop(c); taau_drop_history(c); }
    c->width = w; c->height = h; reset_accumulation(c); c->fbSamples = 0;
    build_shards(c); adaptive_drop(c);
    PT_CHECK_HIP(c, c->dAccum.resize((size_t)w * h));
    PT_CHECK_HIP(c, hipMemsetAsync(c->dAccum.p, 0, sizeof(ptk::float4) * (size_t)w * h, c->stream));
    PT_CHECK_HIP(c, c->dOwned.upload(c->owned, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}
int32_t pt_reset_accumulation(pt_context* c) {
    if (!c || !c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    (void)hipSetDevice(c->device);
    reset_accumulation(c);
    PT_CHECK_HIP(c, hipMemsetAsync(c->dAccum.p, 0, sizeof(ptk::float4) * (size_t)c->width * c->height, c->stream));
    return PT_OK;
}
int32_t pt_animate(pt_context* c, const PtInstanceDesc* inst, uint32_t nInst, const float* positions, uint32_t nVerts, int32_t rebuild) { return pt_animate_ranges(c, inst, nInst, positions, nVerts, nullptr, 0u, rebuild); }
// Motion history (Donut: SceneGraph::Refresh keeps every node's previous global transform, the skinning pass the previous positions of the meshes it rewrites;
// InstanceData.prevTransform, GeometryData.prevPositionOffset): with it on, every pt_animate / pt_animate_ranges call is one scene refresh — the pose it finds
// becomes the previous pose, the pose it brings the current one — and the stable-plane build pass's motion vectors carry the objects' motion
// (Bridge::loadSurface's prevPosW). A call without instances and positions only advances the history (a frame in which nothing moved: previous = current, no
// refit). Device-to-device copies of the instance table and of the vertex ranges that differ.
int32_t pt_set_motion_history(pt_context* c, int32_t enable) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    if (!enable) { c->motionHistory = false; c->dPrevPositions.free(); c->dPrevInstances.free(); c->prevStaleRanges.clear(); c->prevAllStale = false; refresh_scene_view(c); return PT_OK; }
    if (c->geomDirty || c->texDirty) { int r = prepare(c); if (r != PT_OK) return r; }
    // previous = current: nothing has moved yet
    if (!c->motionHistory) { c->motionHistory = true; c->prevAllStale = true; int r = motion_history_sync(c); if (r != PT_OK) return r; }
    refresh_scene_view(c);
    return PT_OK;
}
// the previous pose handed over directly (a host that keeps its own history, or a test): arrays shaped like the scene's; either may be NULL (= that part did
// not move). Turns the history on.
int32_t pt_set_previous_pose(pt_context* c, const PtInstanceDesc* inst, uint32_t nInst, const float* positions, uint32_t nVerts) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    if (c->geomDirty || c->texDirty) { int r = prepare(c); if (r != PT_OK) return r; }
    if (inst && nInst != c->instances.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_previous_pose: instance count differs from the scene's");
    if (positions && (size_t)nVerts * 3 != c->positions.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_previous_pose: vertex count differs from the scene's");
    c->motionHistory = true; c->prevAllStale = true;
    int r = motion_history_sync(c); if (r != PT_OK) return r;
    if (inst) { static_assert(sizeof(PtInstanceDesc) == sizeof(InstanceDesc), "instance layout"); PT_CHECK_HIP(c, hipMemcpyAsync(c->dPrevInstances.p, inst, sizeof(InstanceDesc) * nInst, hipMemcpyHostToDevice, c->stream)); }
    if (positions) { PT_CHECK_HIP(c, hipMemcpyAsync(c->dPrevPositions.p, positions, 12 * (size_t)nVerts, hipMemcpyHostToDevice, c->stream)); c->prevAllStale = true; }      // (differs anywhere: the next refresh copies everything)
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    refresh_scene_view(c);
    return PT_OK;
}

int32_t pt_animate_ranges(pt_context* c, const PtInstanceDesc* inst, uint32_t nInst, const float* positions, uint32_t nVerts, const uint32_t* vertexRanges, uint32_t nRanges, int32_t rebuild) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    if (c->geomDirty || c->texDirty) { int r = prepare(c); if (r != PT_OK) return r; }
    if (inst && nInst != c->instances.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate: instance count must not change");
    if (positions && (size_t)nVerts * 3 != c->positions.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate: vertex count must not change");
    if (positions && vertexRanges) for (uint32_t r = 0; r < nRanges; r++) if ((unsigned long long)vertexRanges[2 * r] + vertexRanges[2 * r + 1] > nVerts) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate_ranges: vertex range beyond the vertex count");
    if (inst) for (uint32_t i = 0; i < nInst; i++) if (inst[i].meshIndex != c->instances[i].meshIndex) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate: topology must not change");
    if (positions) { int r = sync_mirrors(c); if (r != PT_OK) return r; }      // (after pt_animate_skinned the host copy written below lags the device)
    // (every argument is validated by now: a rejected call must not advance the motion history — the next build pass would report zero object motion for what
    // moved last frame)
    if (c->motionHistory) {      // one scene refresh: what is current becomes previous (before the uploads below overwrite it)
        int r = motion_history_sync(c); if (r != PT_OK) return r;
        if (positions) { if (vertexRanges) c->prevStaleRanges.assign(vertexRanges, vertexRanges + 2 * (size_t)nRanges); else c->prevAllStale = true; }
        if (!inst && !positions) { PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); refresh_scene_view(c); return PT_OK; }
    }
    static const bool animLog = getenv("MI355PT_ANIMATE_LOG") != nullptr;      // developer probe: host-side time of every step of the call (stderr)
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tA = now(); double tB = tA, tC = tA, tD = tA, tE = tA;
    if (inst) {
        memcpy(c->instances.data(), inst, sizeof(InstanceDesc) * nInst);
        PT_CHECK_HIP(c, c->dInstances.upload(c->instances, c->stream));
    }
    if (positions) {
        if (vertexRanges) {
            for (uint32_t r = 0; r < nRanges; r++) {
                const size_t first = 3 * (size_t)vertexRanges[2 * r], count = 3 * (size_t)vertexRanges[2 * r + 1];
                if (!count) continue;
                memcpy(c->positions.data() + first, positions + first, 4 * count);
                PT_CHECK_HIP(c, hipMemcpyAsync(c->dPositions.p + first, c->positions.data() + first, 4 * count, hipMemcpyHostToDevice, c->stream));
            }
        } else {
            memcpy(c->positions.data(), positions, 12 * (size_t)nVerts);
            PT_CHECK_HIP(c, c->dPositions.upload(c->positions, c->stream));
        }
    }
    tB = now();
    refresh_scene_view(c);
    if (positions) {      // the shading records hold object-space vertices: deformed meshes rewrite them, rigid motion does not
        if (!vertexRanges) launch_shade_tris(c->dsc, 0u, c->numTris, c->dShadeTris.p, c->stream);
        else for (size_t s = 0; s < c->subInstToInstGeom.size(); s++) {      // sub-instances (= primitive ranges) of the geometries that hold a moved vertex
            const GeometryDesc& gd = c->geometries[c->subInstToInstGeom[s].y];
            bool touched = false;
            for (uint32_t r = 0; r < nRanges && !touched; r++) touched = vertexRanges[2 * r + 1] && vertexRanges[2 * r] < gd.vertexOffset + gd.numVertices && gd.vertexOffset < vertexRanges[2 * r] + vertexRanges[2 * r + 1];
            if (touched) launch_shade_tris(c->dsc, c->subInstFirstPrim[s], gd.numIndices / 3u, c->dShadeTris.p, c->stream);
        }
    }
    hipEvent_t e0, e1; PT_CHECK_HIP(c, hipEventCreate(&e0)); PT_CHECK_HIP(c, hipEventCreate(&e1));
    PT_CHECK_HIP(c, hipEventRecord(e0, c->stream));
    if (rebuild) {                                     // a rebuild between animated frames prefers a fast build: PLOC on the device (15 ms at 2.8 M triangles)
        if (c->bvh.builder == BVH_BUILDER_SAH || c->bvh.builder == BVH_BUILDER_PLOC_OPT) c->bvh.builder = BVH_BUILDER_PLOC;
        PT_CHECK_HIP(c, bvh_build(c->bvh, c->dsc, c->numTris, c->stream));
    } else PT_CHECK_HIP(c, bvh_refit(c->bvh, c->dsc, c->numTris, c->stream));
    // (a fast refit leaves the BVH2 behind: nothing may read it until the next full build, pt_build.h bvh2Stale)
    c->dsc.nodes = c->bvh.bvh2Stale ? nullptr : c->bvh.nodes;
    PT_CHECK_HIP(c, hipEventRecord(e1, c->stream));
    tC = now();
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    tD = now();
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1); if (rebuild) c->buildMs = ms; else c->refitMs = ms; (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    const bool lightsWereDirty = c->lightsDirty;      // something besides the geometry changed since the last bake (environment, analytic lights, NEE settings)
    c->lightsDirty = true;                    // emissive triangle lights move with the geometry (Sample.cpp:1170-1198)
    reset_accumulation(c);                        // any scene change resets accumulation in reference mode
    PT_CHECK_HIP(c, hipMemsetAsync(c->dAccum.p, 0, sizeof(ptk::float4) * (size_t)c->width * c->height, c->stream));
    // geometry moved, nothing else: environment lights kept, emissive re-bake + weights + proxy table on the device
    const int32_t rb = bake_lights(c, !lightsWereDirty);
    tE = now();
    if (animLog) fprintf(stderr, "[animate] copy + upload %.3f ms, launches %.3f ms, wait %.3f ms (refit %.3f ms on the device), light re-bake %.3f ms: %.3f ms\n", tB - tA, tC - tB, tD - tC, ms, tE - tD, tE - tA);
    return rb;
}

int32_t pt_animate_normals(pt_context* c, const uint32_t* normals, const uint32_t* tangents, uint32_t nVerts) {
    if (!c || (!normals && !tangents)) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    if (c->geomDirty || c->texDirty) { int r = prepare(c); if (r != PT_OK) return r; }
    if ((normals && nVerts != c->normals.size()) || (tangents && nVerts != c->tangents.size())) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate_normals: vertex count must not change");
    { int r = sync_mirrors(c); if (r != PT_OK) return r; }      // (after pt_animate_skinned the host copies written below lag the device)
    if (normals) { memcpy(c->normals.data(), normals, 4 * (size_t)nVerts); PT_CHECK_HIP(c, c->dNormals.upload(c->normals, c->stream)); }
    if (tangents) { memcpy(c->tangents.data(), tangents, 4 * (size_t)nVerts); PT_CHECK_HIP(c, c->dTangents.upload(c->tangents, c->stream)); }
    refresh_scene_view(c);
    launch_shade_tris(c->dsc, 0u, c->numTris, c->dShadeTris.p, c->stream);      // the shading records hold the packed vertex normals and tangents
    reset_accumulation(c);
    PT_CHECK_HIP(c, hipMemsetAsync(c->dAccum.p, 0, sizeof(ptk::float4) * (size_t)c->width * c->height, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

// ---- skins and morph targets on the device (pt_skin.h: the per-vertex text, shared with the host pose of pt_gltf.cpp; pt_skin.hip: k_skin)
int32_t pt_set_skinning(pt_context* c, const PtSkinningDesc* d) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    if (!d) { skin_drop(c); return PT_OK; }
    if (c->geomDirty || c->texDirty) { int r = prepare(c); if (r != PT_OK) return r; }
    const size_t nv = c->positions.size() / 3;
    if (d->numVertices != nv) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_skinning: vertex count differs from the scene's");
    if ((d->numRanges && !d->ranges) || (nv && (!d->joints || !d->weights || !d->normals || !d->tangents))) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_skinning: null array");
    std::vector<std::pair<uint64_t, uint64_t>> spans; std::vector<uint32_t> start(1, 0u), stale; bool morphs = false;
    for (uint32_t i = 0; i < d->numRanges; i++) {
        const PtSkinRange& r = d->ranges[i];
        if ((uint64_t)r.firstVertex + r.numVertices > nv) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_skinning: range beyond the vertex stream");
        if ((uint64_t)r.firstMatrix + r.numMatrices > d->numMatrices) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_skinning: a range's matrices lie beyond numMatrices");
        if (r.numTargets) {
            if ((uint64_t)r.firstWeight + r.numTargets > d->numMorphWeights) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_skinning: a range's morph weights lie beyond numMorphWeights");
            if ((uint64_t)r.firstMorphDelta + (uint64_t)r.numTargets * r.numVertices * 3ull > d->numMorphDeltaFloats) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_skinning: a range's morph displacements lie beyond numMorphDeltaFloats");
            morphs = true;
        }
        if (r.numVertices) spans.push_back({r.firstVertex, (uint64_t)r.firstVertex + r.numVertices});
        start.push_back(start.back() + r.numVertices); stale.push_back(r.firstVertex); stale.push_back(r.numVertices);      // (inside the stream and disjoint, checked below: the sum fits)
    }
    if (morphs && (!d->morphPositionDeltas || !d->morphNormalDeltas || !d->morphTangentDeltas)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_skinning: null morph displacement array");
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); i++) if (spans[i].first < spans[i - 1].second) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_set_skinning: ranges overlap");
    skin_drop(c);
    const size_t nd = morphs ? (size_t)d->numMorphDeltaFloats : 0; hipStream_t st = c->stream;
    PT_CHECK_HIP(c, c->dSkinJoints.upload(d->joints, 4 * nv, st)); PT_CHECK_HIP(c, c->dSkinWeights.upload(d->weights, 4 * nv, st));
    PT_CHECK_HIP(c, c->dSkinNormals.upload(d->normals, 3 * nv, st)); PT_CHECK_HIP(c, c->dSkinTangents.upload(d->tangents, 4 * nv, st));
    PT_CHECK_HIP(c, c->dSkinDeltaP.upload(d->morphPositionDeltas, nd, st)); PT_CHECK_HIP(c, c->dSkinDeltaN.upload(d->morphNormalDeltas, nd, st)); PT_CHECK_HIP(c, c->dSkinDeltaT.upload(d->morphTangentDeltas, nd, st));
    PT_CHECK_HIP(c, c->dSkinRanges.upload(d->ranges, d->numRanges, st)); PT_CHECK_HIP(c, c->dSkinRangeStart.upload(start, st));
    PT_CHECK_HIP(c, c->dSkinMatrices.resize(16 * (size_t)d->numMatrices)); PT_CHECK_HIP(c, c->dSkinMorphWeights.resize(d->numMorphWeights));
    // the bind pose: dPositions is overwritten by every pose
    PT_CHECK_HIP(c, c->dSkinBind.resize(3 * nv)); if (nv) PT_CHECK_HIP(c, hipMemcpyAsync(c->dSkinBind.p, c->dPositions.p, 12 * nv, hipMemcpyDeviceToDevice, st));
    PT_CHECK_HIP(c, hipStreamSynchronize(st));      // (the uploads read the caller's arrays)
    SkinView& v = c->skinView;
    v.joints = c->dSkinJoints.p; v.weights = c->dSkinWeights.p; v.normals = c->dSkinNormals.p; v.tangents = c->dSkinTangents.p; v.bindPositions = c->dSkinBind.p;
    v.deltasP = c->dSkinDeltaP.p; v.deltasN = c->dSkinDeltaN.p; v.deltasT = c->dSkinDeltaT.p; v.ranges = c->dSkinRanges.p; v.rangeStart = c->dSkinRangeStart.p;
    v.numRanges = d->numRanges; v.total = start.back();
    c->skinRanges.assign(d->ranges, d->ranges + d->numRanges); c->skinStale = stale; c->skinMatrices = d->numMatrices; c->skinWeights = d->numMorphWeights; c->skinSet = true;
    return PT_OK;
}
int32_t pt_animate_skinned(pt_context* c, const PtInstanceDesc* inst, uint32_t nInst, const double* matrices, uint32_t numMatrices, const double* morphWeights, uint32_t numWeights, int32_t rebuild) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    if (c->geomDirty || c->texDirty) { int r = prepare(c); if (r != PT_OK) return r; }
    if (!c->skinSet) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate_skinned: pt_set_skinning first");
    if (inst && nInst != c->instances.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate_skinned: instance count must not change");
    if (inst) for (uint32_t i = 0; i < nInst; i++) if (inst[i].meshIndex != c->instances[i].meshIndex) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate_skinned: topology must not change");
    if (numMatrices != c->skinMatrices || (numMatrices && !matrices)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate_skinned: the palette must hold the description's numMatrices matrices");
    if (numWeights != c->skinWeights || (numWeights && !morphWeights)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_animate_skinned: the morph weights must be the description's numMorphWeights");
    // (every argument is validated by now: a rejected call must not advance the motion history, pt_animate_ranges)
    if (c->motionHistory) {      // one scene refresh: what is current becomes previous, before k_skin overwrites it; the ranges are what differs afterwards
        int r = motion_history_sync(c); if (r != PT_OK) return r;
        c->prevStaleRanges = c->skinStale;
    }
    if (inst) { memcpy(c->instances.data(), inst, sizeof(InstanceDesc) * nInst); PT_CHECK_HIP(c, c->dInstances.upload(c->instances, c->stream)); }
    if (numMatrices) PT_CHECK_HIP(c, hipMemcpyAsync(c->dSkinMatrices.p, matrices, 128 * (size_t)numMatrices, hipMemcpyHostToDevice, c->stream));
    if (numWeights) PT_CHECK_HIP(c, hipMemcpyAsync(c->dSkinMorphWeights.p, morphWeights, 8 * (size_t)numWeights, hipMemcpyHostToDevice, c->stream));
    for (int e = 0; e < 2; e++) if (!c->skinEvents[e]) PT_CHECK_HIP(c, hipEventCreate(&c->skinEvents[e]));
    PT_CHECK_HIP(c, hipEventRecord(c->skinEvents[0], c->stream));
    launch_skin(c->skinView, c->dSkinMatrices.p, c->dSkinMorphWeights.p, c->dPositions.p, c->dNormals.p, c->dTangents.p, c->stream);
    PT_CHECK_HIP(c, hipEventRecord(c->skinEvents[1], c->stream));
    c->mirrorsStale = true; c->mirrorRanges = c->skinStale;
    refresh_scene_view(c);
    for (size_t s = 0; s < c->subInstToInstGeom.size(); s++) {      // the shading records of the sub-instances (= primitive ranges) of the geometries that hold a posed vertex
        const GeometryDesc& gd = c->geometries[c->subInstToInstGeom[s].y];
        bool touched = false;
        for (size_t r = 0; r < c->skinRanges.size() && !touched; r++) { const PtSkinRange& k = c->skinRanges[r]; touched = k.numVertices && k.firstVertex < gd.vertexOffset + gd.numVertices && gd.vertexOffset < k.firstVertex + k.numVertices; }
        if (touched) launch_shade_tris(c->dsc, c->subInstFirstPrim[s], gd.numIndices / 3u, c->dShadeTris.p, c->stream);
    }
    hipEvent_t e0, e1; PT_CHECK_HIP(c, hipEventCreate(&e0)); PT_CHECK_HIP(c, hipEventCreate(&e1));
    PT_CHECK_HIP(c, hipEventRecord(e0, c->stream));
    if (rebuild) {                                     // (pt_animate_ranges: a rebuild between animated frames is PLOC on the device)
        if (c->bvh.builder == BVH_BUILDER_SAH || c->bvh.builder == BVH_BUILDER_PLOC_OPT) c->bvh.builder = BVH_BUILDER_PLOC;
        PT_CHECK_HIP(c, bvh_build(c->bvh, c->dsc, c->numTris, c->stream));
    } else PT_CHECK_HIP(c, bvh_refit(c->bvh, c->dsc, c->numTris, c->stream));
    c->dsc.nodes = c->bvh.bvh2Stale ? nullptr : c->bvh.nodes;
    PT_CHECK_HIP(c, hipEventRecord(e1, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));      // the call's one wait (the palette and the instances are the caller's arrays)
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1); if (rebuild) c->buildMs = ms; else c->refitMs = ms; (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    ms = 0; (void)hipEventElapsedTime(&ms, c->skinEvents[0], c->skinEvents[1]); c->skinMs = ms;
    const bool lightsWereDirty = c->lightsDirty;
    c->lightsDirty = true;                    // emissive triangle lights move with the geometry
    reset_accumulation(c);
    PT_CHECK_HIP(c, hipMemsetAsync(c->dAccum.p, 0, sizeof(ptk::float4) * (size_t)c->width * c->height, c->stream));
    return bake_lights(c, !lightsWereDirty);
}
int32_t pt_get_skinning_time(pt_context* c, double* ms) { if (!c || !ms) return PT_ERROR_INVALID_ARGUMENT; *ms = c->skinMs; return PT_OK; }
int32_t pt_get_vertex_streams(pt_context* c, float* positions, float* prevPositions, uint32_t* normals, uint32_t* tangents, uint32_t capacityVertices) {
    if (!c) return -PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    if (c->geomDirty || c->texDirty) { int r = prepare(c); if (r != PT_OK) return -r; }
    const size_t nv = c->positions.size() / 3;
    if (capacityVertices < nv || !nv) return (int32_t)nv;
    if (prevPositions && !(c->motionHistory && c->dPrevPositions.p && c->dPrevPositions.n >= 3 * nv)) return -fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_get_vertex_streams: the previous positions exist only with the motion history on");
    auto back = [&](void* dst, const void* src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess; };
    hipError_t e = back(positions, c->dPositions.p, 12 * nv);
    if (e == hipSuccess) e = back(prevPositions, c->dPrevPositions.p, 12 * nv);
    if (e == hipSuccess) e = back(normals, c->dNormals.p, 4 * nv);
    if (e == hipSuccess) e = back(tangents, c->dTangents.p, 4 * nv);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return -fail(c, PT_ERROR_HIP, std::string("pt_get_vertex_streams: ") + hipGetErrorString(e));
    return (int32_t)nv;
}
static_assert(sizeof(::PtStablePlanesParams) == sizeof(ptk::StablePlanesParams) && sizeof(::PtStablePlane) == sizeof(ptk::StablePlane), "stable-plane ABI");
int32_t pt_stable_planes_plane_stride(uint32_t width, uint32_t height, uint32_t* stride) { if (!stride) return PT_ERROR_INVALID_ARGUMENT; *stride = ptk::GenericTSComputePlaneStride(width, height); return PT_OK; }
// The realtime mode's frame with everything coupled (Sample.cpp:2438-2516; pt_set_neeat on): LightsBaker::UpdateBegin -> build pass -> LightsBaker::UpdateEnd
// on THAT frame's depth and screen-space motion vectors -> the fill passes, which sample the tables just made and fill the reservoirs the next frame's
// UpdateBegin reads.
// On tile shards a frame has two exchanges (pt_shard.hip): the reservoirs before UpdateBegin (neeat_exchange_feedback) and the build pass's guides before UpdateEnd
// (sp_exchange_guides).
// LightsBaker::UpdateBegin / UpdateEnd as calls of their own (Rtxpt/Sample.cpp:1380-1412, 2491-2494): what pt_realtime_frame runs around the build pass, for a
// host that puts something of its own in between (a tile-sharded frame without a communicator: the exchanges above)
int32_t pt_neeat_update_begin(pt_context* c) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    if (!c->neeat.enabled) return fail(c, PT_ERROR_NOT_READY, "pt_set_neeat first");
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    return neeat_frame(c, NEEAT_BEGIN);
}
int32_t pt_neeat_update_end(pt_context* c) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->neeat.enabled) return fail(c, PT_ERROR_NOT_READY, "pt_set_neeat first");
    if (!c->spW || c->spW != c->width || c->spH != c->height) return fail(c, PT_ERROR_NOT_READY, "UpdateEnd reads the frame's depth and motion vectors: pt_build_stable_planes first");
    (void)hipSetDevice(c->device);
    int r = neeat_frame(c, NEEAT_END, c->dSpDepth.p, c->dSpMotion.p); if (r != PT_OK) return r;
    if (c->feedbackRequired) c->fbSamples = 1;
    return PT_OK;
}
int32_t pt_realtime_frame(pt_context* c, uint32_t sampleIndex, const PtStablePlanesParams* params, PtFrameStats* buildStats, PtFrameStats* fillStats) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    const bool baker = c->neeat.enabled && c->S.NEEEnabled && c->S.NEEFullSamples != 0u;
    if (baker && c->shardCount > 1 && !c->comm) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_realtime_frame on tile shards: the baker reads the whole frame's reservoirs, depth and motion vectors — pt_comm_init first, or drive the parts (pt_neeat_update_begin, pt_build_stable_planes, pt_pack / pt_unpack_stable_plane_guides, pt_neeat_update_end, pt_fill_stable_planes)");
    if (baker) { r = neeat_exchange_feedback(c); if (r != PT_OK) return r; r = neeat_frame(c, NEEAT_BEGIN); if (r != PT_OK) return r; }
    r = pt_build_stable_planes(c, sampleIndex, params, buildStats); if (r != PT_OK) return r;
    if (baker) { r = sp_exchange_guides(c); if (r != PT_OK) return r; r = neeat_frame(c, NEEAT_END, c->dSpDepth.p, c->dSpMotion.p); if (r != PT_OK) return r; }
    const uint32_t subSamples = params->subSampleCount ? params->subSampleCount : 1u;
    PtFrameStats total; memset(&total, 0, sizeof(total));
    for (uint32_t s = 0; s < subSamples; s++) { PtFrameStats one; r = pt_fill_stable_planes(c, sampleIndex + s, params, &one); if (r != PT_OK) return r; add_frame_stats(total, one); }
    if (fillStats) *fillStats = total;
    if (baker && c->feedbackRequired) c->fbSamples = 1;      // pt_get_light_feedback(0): the reservoirs as the fill passes left them
    return PT_OK;
}
int32_t pt_stable_planes_merge(pt_context* c) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->spW || c->spW != c->width || c->spH != c->height) return fail(c, PT_ERROR_NOT_READY, "no stable planes of this frame size yet: pt_build_stable_planes, pt_fill_stable_planes");
    (void)hipSetDevice(c->device);
    ptk::StablePlanesParams prm; memset(&prm, 0, sizeof(prm)); prm.activeStablePlaneCount = cStablePlaneCount;
    StablePlanesContext sp; sp.C = ptk::SP_make_consts(prm, c->width, c->height, c->S.bounceCount); memset(&sp.B, 0, sizeof(sp.B));
    sp.B.Header = c->dSpHeader.p; sp.B.Planes = c->dSpPlanes.p; sp.B.StableRadiance = c->dSpRadiance.p;
    const uint numOwned = (uint)c->owned.size();
    if (numOwned) launch_sp_merge(sp, c->dOwned.p, numOwned, c->dAccum.p, c->stream);
    // the buffer now holds one finished frame: pt_map_radiance / pt_tonemap / pt_gather read it, the next pt_render blends into it like into any first sample
    c->accumCount = 1;
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}
int32_t pt_denoise_spec_hit_t(pt_context* c) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->spW || c->spW != c->width || c->spH != c->height) return fail(c, PT_ERROR_NOT_READY, "no stable planes of this frame size yet: pt_build_stable_planes, pt_fill_stable_planes");
    if (c->shardCount > 1 && !c->spGathered) return fail(c, PT_ERROR_INVALID_ARGUMENT, "the fill-in reads 5 x 5 neighbourhoods: run it on the gathered planes (pt_gather_stable_planes / pt_unpack_stable_planes on rank 0), not on one rank's tiles");
    (void)hipSetDevice(c->device);
    PT_CHECK_HIP(c, c->dSpScratch.resize((size_t)c->width * c->height));
    launch_sp_denoise_spec_hit_t(c->dSpHitT.p, c->dSpDepth.p, c->dSpScratch.p, c->width, c->height, c->stream);
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}
int32_t pt_get_stable_planes(pt_context* c, uint32_t* header, PtStablePlane* planes, size_t planeCapacity, uint16_t* stableRadiance, float* depth, float* specularHitT, uint16_t* motionVectors, uint32_t* throughput) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->spW || c->spW != c->width || c->spH != c->height) return fail(c, PT_ERROR_NOT_READY, "no stable planes of this frame size yet: pt_build_stable_planes");
    (void)hipSetDevice(c->device);
    const size_t N = (size_t)c->width * c->height, nPlanes = (size_t)cStablePlaneCount * ptk::GenericTSComputePlaneStride(c->width, c->height);
    if (planes && planeCapacity < nPlanes) return fail(c, PT_ERROR_INVALID_ARGUMENT, "plane buffer smaller than 3 x the plane stride (pt_stable_planes_plane_stride)");
    if (header) PT_CHECK_HIP(c, hipMemcpy(header, c->dSpHeader.p, 16 * N, hipMemcpyDeviceToHost));
    if (planes) PT_CHECK_HIP(c, hipMemcpy(planes, c->dSpPlanes.p, sizeof(ptk::StablePlane) * nPlanes, hipMemcpyDeviceToHost));
    if (stableRadiance) PT_CHECK_HIP(c, hipMemcpy(stableRadiance, c->dSpRadiance.p, 8 * N, hipMemcpyDeviceToHost));
    if (depth) PT_CHECK_HIP(c, hipMemcpy(depth, c->dSpDepth.p, 4 * N, hipMemcpyDeviceToHost));
    if (specularHitT) PT_CHECK_HIP(c, hipMemcpy(specularHitT, c->dSpHitT.p, 4 * N, hipMemcpyDeviceToHost));
    if (motionVectors) PT_CHECK_HIP(c, hipMemcpy(motionVectors, c->dSpMotion.p, 8 * N, hipMemcpyDeviceToHost));
    if (throughput) PT_CHECK_HIP(c, hipMemcpy(throughput, c->dSpThroughput.p, 4 * N, hipMemcpyDeviceToHost));
    return PT_OK;
}
// ---- the denoiser passes of a realtime frame (pt_denoiser.h / pt_denoiser.hip; PostProcess.hlsl DENOISER_PREPARE_INPUTS, DENOISER_FINAL_MERGE)
static_assert(sizeof(::PtDenoiserParams) == sizeof(ptk::DenoiserParams), "denoiser ABI");
int32_t pt_denoiser_default_params(PtDenoiserParams* out) {
    if (!out) return PT_ERROR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    for (int i = 0; i < 4; i++) out->matWorldToView[i * 5] = 1.0f;
    out->preExposedGrayLuminance = 1.0f; out->denoiserRadianceClampK = 8.0f; out->DLSSRRBrightnessClampK = 4096.0f * out->preExposedGrayLuminance;
    out->stablePlanesSuppressPrimaryIndirectSpecularK = 0.6f;
    return PT_OK;
}
// (dn_ready, dn_buffers: pt_context.h — the device denoiser's entry points in pt_relax_api.hip use them too)
static int32_t dn_alloc(pt_context* c) {
    if (c->dnW == c->width && c->dnH == c->height) return PT_OK;
    const size_t N = (size_t)c->width * c->height;
    PT_CHECK_HIP(c, c->dDnRRDiff.resize(N)); PT_CHECK_HIP(c, c->dDnRRSpec.resize(N)); PT_CHECK_HIP(c, c->dDnRRSpecMV.resize(N)); PT_CHECK_HIP(c, c->dDnRRNormal.resize(N));
    PT_CHECK_HIP(c, c->dDnMotion.resize(N)); PT_CHECK_HIP(c, c->dDnViewZ.resize(N)); PT_CHECK_HIP(c, c->dDnRoughness.resize(N)); PT_CHECK_HIP(c, c->dDnNormal.resize(N));
    PT_CHECK_HIP(c, c->dDnDiff.resize(N)); PT_CHECK_HIP(c, c->dDnSpec.resize(N)); PT_CHECK_HIP(c, c->dDnDisocclusion.resize(N)); PT_CHECK_HIP(c, c->dDnHistoryClamp.resize(N));
    hipStream_t st = c->stream;
    PT_CHECK_HIP(c, hipMemsetAsync(c->dDnRRDiff.p, 0, 4 * N, st)); PT_CHECK_HIP(c, hipMemsetAsync(c->dDnRRSpec.p, 0, 4 * N, st)); PT_CHECK_HIP(c, hipMemsetAsync(c->dDnRRSpecMV.p, 0, 4 * N, st));
    PT_CHECK_HIP(c, hipMemsetAsync(c->dDnRRNormal.p, 0, 8 * N, st)); PT_CHECK_HIP(c, hipMemsetAsync(c->dDnMotion.p, 0, 8 * N, st)); PT_CHECK_HIP(c, hipMemsetAsync(c->dDnViewZ.p, 0, 4 * N, st));
    PT_CHECK_HIP(c, hipMemsetAsync(c->dDnRoughness.p, 0, 4 * N, st)); PT_CHECK_HIP(c, hipMemsetAsync(c->dDnNormal.p, 0, 16 * N, st)); PT_CHECK_HIP(c, hipMemsetAsync(c->dDnDiff.p, 0, 16 * N, st));
    PT_CHECK_HIP(c, hipMemsetAsync(c->dDnSpec.p, 0, 16 * N, st)); PT_CHECK_HIP(c, hipMemsetAsync(c->dDnDisocclusion.p, 0, N, st)); PT_CHECK_HIP(c, hipMemsetAsync(c->dDnHistoryClamp.p, 0, N, st));
    c->dnW = c->width; c->dnH = c->height;
    return PT_OK;
}
int32_t pt_denoiser_prepare_dlss_rr(pt_context* c, const PtStablePlanesParams* spParams, const PtDenoiserParams* params) {
    if (!c || !spParams || !params) return PT_ERROR_INVALID_ARGUMENT;
    int32_t r = dn_ready(c); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    r = dn_alloc(c); if (r != PT_OK) return r;
    ptk::DenoiserParams P; memcpy(&P, params, sizeof(P));
    launch_dn_prepare_dlss_rr(sp_context(c, spParams), P, dn_buffers(c), c->dAccum.p, c->stream);
    c->accumCount = 1;      // the radiance buffer holds one finished frame (as after pt_stable_planes_merge)
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}
int32_t pt_denoiser_prepare_nrd(pt_context* c, const PtStablePlanesParams* spParams, const PtDenoiserParams* params, uint32_t planeIndex, uint32_t initWithStableRadiance) {
    if (!c || !spParams || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (planeIndex >= cStablePlaneCount) return fail(c, PT_ERROR_INVALID_ARGUMENT, "plane index out of range (0..2)");
    int32_t r = dn_ready(c); if (r != PT_OK) return r;
    (void)hipSetDevice(c->device);
    r = dn_alloc(c); if (r != PT_OK) return r;
    ptk::DenoiserParams P; memcpy(&P, params, sizeof(P));
    PathKernelContext k; k.sc = c->dsc; k.S = c->S; k.cam = c->cam;
    launch_dn_prepare_nrd(k, sp_context(c, spParams), P, dn_buffers(c), planeIndex, initWithStableRadiance != 0u, c->spSampleBase, c->dAccum.p, c->stream);
    if (initWithStableRadiance) c->accumCount = 1;
    c->dnPreparedPlane = (int)planeIndex;      // what pt_denoise_plane may run on
    c->dnNrdSerial = c->spFrameSerial;         // (pt_taa_resolve reads the relax buffer of the current build pass only)
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}
int32_t pt_denoiser_merge_nrd(pt_context* c, uint32_t planeIndex, const float* diffDevice, const float* specDevice) {
    if (!c || !diffDevice || !specDevice) return PT_ERROR_INVALID_ARGUMENT;
    if (planeIndex >= cStablePlaneCount) return fail(c, PT_ERROR_INVALID_ARGUMENT, "plane index out of range (0..2)");
    int32_t r = dn_ready(c); if (r != PT_OK) return r;
    if (c->dnW != c->width || c->dnH != c->height) return fail(c, PT_ERROR_NOT_READY, "the merge reads the NRD prepare pass's viewZ: pt_denoiser_prepare_nrd first");
    (void)hipSetDevice(c->device);
    launch_dn_merge_nrd(sp_context(c, nullptr), dn_buffers(c), planeIndex, (const ptk::float4*)diffDevice, (const ptk::float4*)specDevice, c->dAccum.p, c->stream);
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}
int32_t pt_get_denoiser_inputs(pt_context* c, const PtDenoiserBuffers* host) {
    if (!c || !host) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->dnW || c->dnW != c->width || c->dnH != c->height) return fail(c, PT_ERROR_NOT_READY, "no denoiser inputs of this frame size yet: pt_denoiser_prepare_dlss_rr / pt_denoiser_prepare_nrd");
    (void)hipSetDevice(c->device);
    PtDenoiserBuffers dev; memset(&dev, 0, sizeof(dev)); (void)pt_denoiser_device_buffers(c, &dev);
    void* const* d = &dev.rrDiffuseAlbedo; void* const* h = &host->rrDiffuseAlbedo;
    for (int i = 0; i < 12; i++) if (h[i]) PT_CHECK_HIP(c, hipMemcpy(h[i], d[i], dev.pitch[i] * c->height, hipMemcpyDeviceToHost));
    return PT_OK;
}
int32_t pt_denoiser_device_buffers(pt_context* c, PtDenoiserBuffers* out) {
    if (!c || !out) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->dnW || c->dnW != c->width || c->dnH != c->height) return fail(c, PT_ERROR_NOT_READY, "no denoiser inputs of this frame size yet: pt_denoiser_prepare_dlss_rr / pt_denoiser_prepare_nrd");
    const ptk::DenoiserBuffers D = dn_buffers(c);
    void* p[12] = {D.RRDiffuseAlbedo, D.RRSpecAlbedo, D.RRNormalsAndRoughness, D.RRSpecMotionVectors, D.ViewZ, D.MotionVectors, D.NormalRoughness, D.DiffRadianceHitDist,
                   D.SpecRadianceHitDist, D.Roughness, D.DisocclusionThresholdMix, D.CombinedHistoryClampRelax};
    static const size_t bytes[12] = {4, 4, 8, 4, 4, 8, 16, 16, 16, 4, 1, 1};
    void** o = &out->rrDiffuseAlbedo;
    for (int i = 0; i < 12; i++) { o[i] = p[i]; out->pitch[i] = bytes[i] * c->width; }
    return PT_OK;
}
int32_t pt_map_radiance(pt_context* c, const float** rgba, size_t* pitch) {
    if (!c || !rgba) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    (void)hipSetDevice(c->device);
    c->hostRadiance.resize((size_t)c->width * c->height * 4);
    PT_CHECK_HIP(c, hipMemcpyAsync(c->hostRadiance.data(), c->dAccum.p, sizeof(float) * c->hostRadiance.size(), hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    *rgba = c->hostRadiance.data(); if (pitch) *pitch = (size_t)c->width * 16;
    return PT_OK;
}
int32_t pt_unmap_radiance(pt_context* c) { return c ? PT_OK : PT_ERROR_INVALID_ARGUMENT; }

int32_t pt_default_tonemap(PtToneMapParams* out, float exposureCompensation, float filmSpeed, float shutter, float fNumber) {
    if (!out || !(shutter > 0.f) || !(fNumber > 0.f)) return PT_ERROR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->whiteScale = 5.1f; out->whiteMaxLuminance = 1.0f; out->toneMapOperator = 5u; out->clamped = 1u; out->enabled = 1u;      // ToneMappingPasses.h:36-53
    // ToneMappingPasses.cpp:337-338
    out->autoExposure = 0u; out->avgLuminance = 1.0f; out->autoExposureLumValueMin = exp2f(-16.0f); out->autoExposureLumValueMax = exp2f(16.0f);
    // UpdateColorTransform (ToneMappingPasses.cpp:428-441), white balance off => identity * exposureScale * manualExposureScale
    float exposureScale = powf(2.f, exposureCompensation);
    float manualExposureScale = ((1.f / 100.f) * filmSpeed) / (shutter * fNumber * fNumber);
    float s = exposureScale * manualExposureScale;
    out->colorTransform[0] = s; out->colorTransform[4] = s; out->colorTransform[8] = s;
    return PT_OK;
}

static int trace_probe(pt_context* c, const float* rays, uint32_t n, float* outClosest, uint32_t* outVisible, double* kernelMs) {
    if (!c || !rays || !n) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bad argument");
    // TMin is non-negative (DXR's rule for TraceRay; every ray the renderer forms obeys it). The traversal relies on it: a node's entry distance is max(slab, tmin) >= +0, and
    // the front-to-back order of the children is taken from its BIT PATTERN (pt_traverse8p.h). A negative one (-0 included) orders behind "not hit", and the push that follows
    // indexes the stack with a wrapped count — a store far outside the stack's tail in global memory. Refused here (a NaN too), before anything reaches the device.
    for (uint32_t i = 0; i < n; i++) {
        const float tmin = rays[8 * (size_t)i + 3];
        if (!(tmin >= 0.0f) || std::signbit(tmin)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_trace_closest / pt_trace_visibility: ray " + std::to_string(i) + " has tmin < 0 (or -0, or NaN); tmin must be >= +0");
    }
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    DevBuf<ptk::float4> dr, dc; DevBuf<uint> dv;
    PT_CHECK_HIP(c, dr.upload((const ptk::float4*)rays, 2 * (size_t)n, c->stream));
    if (outClosest) PT_CHECK_HIP(c, dc.resize(n)); else PT_CHECK_HIP(c, dv.resize(n));
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, c->stream);
    launch_trace_probe(c->dsc, dr.p, n, outClosest ? dc.p : nullptr, outClosest ? nullptr : dv.p, &c->dCounters.p->overflow, c->stream);
    (void)hipEventRecord(e1, c->stream);
    if (outClosest) PT_CHECK_HIP(c, hipMemcpyAsync(outClosest, dc.p, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    else PT_CHECK_HIP(c, hipMemcpyAsync(outVisible, dv.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1); if (kernelMs) *kernelMs = ms; (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    dr.free(); dc.free(); dv.free();
    return PT_OK;
}
int32_t pt_trace_closest(pt_context* c, const float* rays, uint32_t n, float* out, double* ms) { if (!out) return PT_ERROR_INVALID_ARGUMENT; return trace_probe(c, rays, n, out, nullptr, ms); }
int32_t pt_trace_visibility(pt_context* c, const float* rays, uint32_t n, uint32_t* out, double* ms) { if (!out) return PT_ERROR_INVALID_ARGUMENT; return trace_probe(c, rays, n, nullptr, out, ms); }

int32_t pt_get_lights(pt_context* c, uint32_t* nLights, uint32_t* nProxies, void* lights, void* lightsEx, uint32_t* pc, uint32_t* pi, uint32_t* envLookup, uint32_t* envDim) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    if (nLights) *nLights = (uint32_t)c->lights.size(); if (nProxies) *nProxies = c->numProxies; if (envDim) *envDim = c->envLookupDim;
    // read back from the DEVICE copies: this is what the kernels sample from
    if (lights && c->lights.size()) PT_CHECK_HIP(c, hipMemcpy(lights, c->dLights.p, 32 * c->lights.size(), hipMemcpyDeviceToHost));
    if (lightsEx && c->lights.size()) PT_CHECK_HIP(c, hipMemcpy(lightsEx, c->dLightsEx.p, 16 * c->lights.size(), hipMemcpyDeviceToHost));
    if (pc && c->lights.size()) PT_CHECK_HIP(c, hipMemcpy(pc, c->dProxyCounters.p, 4 * c->lights.size(), hipMemcpyDeviceToHost));
    if (pi && c->numProxies) PT_CHECK_HIP(c, hipMemcpy(pi, c->dProxyIndices.p, 4 * (size_t)c->numProxies, hipMemcpyDeviceToHost));
    if (envLookup && c->envLookup.size()) PT_CHECK_HIP(c, hipMemcpy(envLookup, c->dEnvLookup.p, 4 * c->envLookup.size(), hipMemcpyDeviceToHost));
    return PT_OK;
}
int32_t pt_get_env_cube(pt_context* c, uint32_t* texelCount, uint32_t* dim, uint32_t* mipLevels, void* texels8B, uint32_t capacityTexels) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    size_t n = 0;
    if (c->envEnabled) { const uint last = c->envCube.mipLevels - 1u, d = c->envCube.dim >> last; n = (size_t)c->envCube.mipOffset[last] + 6ull * d * d; }
    if (texelCount) *texelCount = (uint32_t)n; if (dim) *dim = c->envEnabled ? c->envCube.dim : 0; if (mipLevels) *mipLevels = c->envEnabled ? c->envCube.mipLevels : 0;
    if (texels8B && n) {
        if (capacityTexels < n) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_get_env_cube: buffer too small");
        PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
        PT_CHECK_HIP(c, hipMemcpy(texels8B, c->dEnvCube.p, 8 * n, hipMemcpyDeviceToHost));
    }
    return PT_OK;
}
// (the texture read-backs) prepare()'s texture step alone: they need no geometry
static int32_t sync_textures(pt_context* c) {
    (void)hipSetDevice(c->device);
    if (c->texDirty) { int r = upload_textures(c); if (r != PT_OK) return r; refresh_scene_view(c); c->lightsDirty = true; c->envCubeDirty = true; }
    return PT_OK;
}
int32_t pt_get_texture_level(pt_context* c, uint32_t texture, uint32_t mip, uint32_t* w, uint32_t* h, float* rgba, uint32_t capacityTexels) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    int r = sync_textures(c); if (r != PT_OK) return r;
    if (texture >= c->texInfos.size() || mip >= c->texInfos[texture].mipLevels) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_get_texture_level: texture or mip out of range");
    const TexInfo& ti = c->texInfos[texture]; const uint mw = texi_side(ti.w, mip), mh = texi_side(ti.h, mip);
    if (w) *w = mw; if (h) *h = mh;
    if (rgba) {
        if (capacityTexels < (size_t)mw * mh) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_get_texture_level: buffer too small");
        PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
        PT_CHECK_HIP(c, hipMemcpy(rgba, c->dTexels.p + ti.base + ti.mipOffset[mip], sizeof(ptk::float4) * (size_t)mw * mh, hipMemcpyDeviceToHost));
    }
    return PT_OK;
}
int32_t pt_get_alpha_plane(pt_context* c, uint32_t texture, uint32_t* fmt, void* out, uint32_t capacityBytes, uint32_t* bytes) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    int r = sync_textures(c); if (r != PT_OK) return r;
    if (texture >= c->textures.size() || texture >= c->alphaPlanes.size()) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_get_alpha_plane: texture out of range");
    const ptk::AlphaPlane& ap = c->alphaPlanes[texture]; const size_t n = texi_alpha_plane_bytes(c->textures[texture].w, c->textures[texture].h, ap.fmt == 0u);
    if (fmt) *fmt = ap.fmt; if (bytes) *bytes = (uint32_t)n;
    if (out) {
        if (capacityBytes < n) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_get_alpha_plane: buffer too small");
        PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
        PT_CHECK_HIP(c, hipMemcpy(out, c->dAlphaPool.p + ap.offset, n, hipMemcpyDeviceToHost));
    }
    return PT_OK;
}
int32_t pt_get_texture_ingest_stats(pt_context* c, PtTextureIngestStats* out) {
    if (!c || !out) return PT_ERROR_INVALID_ARGUMENT;
    int r = sync_textures(c); if (r != PT_OK) return r;      // (the host path ingests at its upload)
    *out = c->texStats;
    return PT_OK;
}
int32_t pt_get_subinstances(pt_context* c, uint32_t* count, void* out) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    if (count) *count = (uint32_t)c->subInstances.size();
    if (out && c->subInstances.size()) PT_CHECK_HIP(c, hipMemcpy(out, c->dSubInstances.p, 32 * c->subInstances.size(), hipMemcpyDeviceToHost));
    return PT_OK;
}
int32_t pt_get_scene_info(pt_context* c, uint32_t* nTris, uint32_t* nNodes, uint32_t* nInst, uint32_t* nMat) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    if (nTris) *nTris = c->numTris; if (nNodes) *nNodes = c->numTris ? c->bvh.numNodes8 : 0;      /* BVH8 nodes */ if (nInst) *nInst = (uint32_t)c->instances.size(); if (nMat) *nMat = (uint32_t)c->materials.size();
    return PT_OK;
}
int32_t pt_get_build_stats(pt_context* c, double* b, double* r, double* l) { if (!c) return PT_ERROR_INVALID_ARGUMENT; if (b) *b = c->buildMs; if (r) *r = c->refitMs; if (l) *l = c->lightBakeMs; return PT_OK; }
int32_t pt_get_bvh_info(pt_context* c, PtBvhInfo* out) {
    if (!c || !out) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    memset(out, 0, sizeof(*out));
    out->builder = c->bvh.builder; out->builtOnDevice = (c->bvh.builder == BVH_BUILDER_SAH && c->bvh.hostBuildMs > 0.f) ? 0u : 1u; out->numTriangles = c->numTris;
    out->numWideNodes = c->numTris ? c->bvh.numNodes8 : 0u; out->collapseLevels = c->bvh.collapseLevels; out->optimiserPasses = c->bvh.optimiserPasses; out->hostMs = c->bvh.hostBuildMs; out->buildMs = (float)c->buildMs;
    return PT_OK;
}
int32_t pt_set_counters(pt_context* c, int32_t enable) { if (!c) return PT_ERROR_INVALID_ARGUMENT; c->countersEnabled = enable != 0; return PT_OK; }
int32_t pt_set_serial_kernels(pt_context* c, int32_t enable) { if (!c) return PT_ERROR_INVALID_ARGUMENT; c->serialKernels = enable != 0; return PT_OK; }
int32_t pt_set_tail_paths(pt_context* c, uint32_t maxPaths) { if (!c) return PT_ERROR_INVALID_ARGUMENT; c->tailBelow = maxPaths; return PT_OK; }
int32_t pt_set_fused_traversal(pt_context* c, uint32_t mode) { if (!c || mode > 2u) return PT_ERROR_INVALID_ARGUMENT; c->fusedTraversal = mode; return PT_OK; }

} // extern "C"

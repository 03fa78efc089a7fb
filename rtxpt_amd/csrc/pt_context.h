// mi355pt — what the translation units behind include/mi355pt.h share: the context, its device buffers, the error helpers, the tuning
// defines and the few functions of pt_api.hip and pt_shard.hip that the other translation units call. Private: nothing here is exported.
#pragma once
#include "../../include/mi355pt.h"
#include "pt_wavefront.h"
#include "pt_trace.h"
#include "pt_bake.h"
#include "pt_texture_ingest.h"
#include "pt_stableplanes_launch.h"
#include "pt_denoiser.h"
#include "pt_build.h"
#include "pt_adaptive.h"
#include "pt_shard.h"
#include <rccl/rccl.h>      // types only: the functions are bound at run time (dlopen), see pt_comm_init
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

using namespace ptk;

// what k_skin reads (pt_skin.hip): the device copies of a PtSkinningDesc's arrays, the bind-pose positions, the ranges and their prefix table (rangeStart[r]: the deformed
// vertices before range r; numRanges + 1 entries, the last one `total`)
struct SkinView {
    const uint16_t* joints; const float* weights; const float* normals; const float* tangents; const float* bindPositions;
    const float* deltasP; const float* deltasN; const float* deltasT; const PtSkinRange* ranges; const uint32_t* rangeStart; uint32_t numRanges, total;
};
template <typename T> struct DevBuf {
    T* p = nullptr; size_t n = 0;
    hipError_t resize(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
        hipError_t e = hipMalloc(&p, sizeof(T) * (count ? count : 1));
        if (e == hipSuccess) n = count ? count : 1;
        return e;
    }
    hipError_t upload(const T* src, size_t count, hipStream_t st) {
        hipError_t e = resize(count); if (e != hipSuccess) return e;
        if (!count) return hipSuccess;
        return hipMemcpyAsync(p, src, sizeof(T) * count, hipMemcpyHostToDevice, st);
    }
    hipError_t upload(const std::vector<T>& v, hipStream_t st) { return upload(v.data(), v.size(), st); }
    void free() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};
// the optional event timing of a pass (its gpuMs argument): two events, created by the first call that asks for its time; begin / end record them around the launches,
// read gives the time between them once the caller has waited for the stream. A call that does not ask creates and records nothing.
struct EventBracket {
    hipEvent_t ev[2] = {nullptr, nullptr}; bool on = false;
    hipError_t create() {      // (on its own: for a pass that wants every step that can fail on the host done before it gives its previous picture up)
        for (int s = 0; s < 2; s++) if (!ev[s]) { hipError_t e = hipEventCreate(&ev[s]); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    hipError_t begin(hipStream_t st, bool wanted) {
        on = wanted; if (!on) return hipSuccess;
        hipError_t e = create();
        return e != hipSuccess ? e : hipEventRecord(ev[0], st);
    }
    hipError_t end(hipStream_t st) { return on ? hipEventRecord(ev[1], st) : hipSuccess; }
    hipError_t read(float* ms) { return on ? hipEventElapsedTime(ms, ev[0], ev[1]) : hipSuccess; }
    void destroy() { for (int s = 0; s < 2; s++) if (ev[s]) { (void)hipEventDestroy(ev[s]); ev[s] = nullptr; } }
};
// a bloomed picture (pt_bloom_api.hip bloom_run): the result — a buffer of its own, the source is never written — and the two quarter-resolution images of the blur.
// ready: a bloomed picture of w x h is there.
struct BloomState {
    DevBuf<ptk::float4> out, q[2]; uint w = 0, h = 0; bool ready = false; EventBracket timer;
    void free() { out.free(); q[0].free(); q[1].free(); timer.destroy(); w = h = 0; ready = false; }
};

struct HostTexture { uint w, h, mipLevels; std::vector<std::vector<ptk::float4>> mips; };

// the staging of a shard exchange (pt_shard.hip shard_exchange), one for the four records: the packed records of the own pixels, the records received, and the pixel list the
// latter are unpacked by — every other rank's pixels in rank order, which serves both routes on every rank (a sender to rank 0 needs none). Grow-only, sized in words;
// w x h: the frame size `pixels` is of (0: none; build_shards drops it with the shard lists).
struct ShardStaging {
    DevBuf<uint> send, recv, pixels; uint w = 0, h = 0;
    void free() { send.free(); recv.free(); pixels.free(); w = h = 0; }
};

static const uint TASK_QUEUE_CAPACITY = 1u << 22;      // sub-tree tasks per queue (2 queues per pipelined batch, 16 B each)
#ifndef PT_PIPELINE_FULL_AT
// paths per pt_render call from which all PT_PIPELINE_BATCHES are used (one rank of an 8-way sharded 4K frame has 4.1 M)
#define PT_PIPELINE_FULL_AT (1u << 21)
#endif
#ifndef PT_PIPELINE_MID_BATCHES
#define PT_PIPELINE_MID_BATCHES 2      // batches between 1 M paths and PT_PIPELINE_FULL_AT
#endif
#ifndef PT_CLASSIFY_FROM
// passes with fewer paths skip k_classify (class-ordered shading pays through coherence, which a handful of waves do not have)
#define PT_CLASSIFY_FROM 65536u
#endif
#ifndef PT_SP_FILL_CLASSES
// the stable-plane fill pass shades in class order (k_classify), like reference mode; 0: queue order (A/B)
#define PT_SP_FILL_CLASSES 1
#endif
#ifndef PT_SP_FILL_RANGED
// the fill pass's first traversal launch uses FirstHitFromVBuffer's narrowed ray interval (pt_stableplanes.h firstHitInterval);
// 0: the whole ray (A/B) — same hits
#define PT_SP_FILL_RANGED 1
#endif
#ifndef PT_TAIL_PATHS
// a batch with at most this many live paths is finished by the tail kernel (pt_tail.hip, pt_set_tail_paths); 0: never. With fused traversal
// launches and free-running small passes a pass of tens of thousands of paths is cheaper as a wavefront pass than in the tail kernel's
// under-filled GPU (rank of eight 12.56 -> 12.11 ms without it; the threshold was 32768 before those two), while the chains of passes that
// hold a few hundred paths each — nested-dielectric re-traces: C5 runs 19 passes, twelve of them below 10 k paths at ~0.25 ms each — are
// what the kernel is for: 4096 takes C5's rank of eight 13.9 -> 13.2 ms, C3's 12.0 -> 11.8 (profiles/r06o_tail_small_ab.txt)
#define PT_TAIL_PATHS 4096u
#endif
#ifndef PT_FUSED_TRAVERSAL
// pt_set_fused_traversal (default: on — it pays at every size, profiles/r06b_fused_traversal_ab.txt): 0 = every bounce traces its
// visibility rays in a launch of their own, 1 = together with the closest-hit rays of the next bounce (k_trace_pair, pt_trace.hip),
// 2 = by the size of the call (PT_FUSED_BELOW)
#define PT_FUSED_TRAVERSAL 1u
#endif
#ifndef PT_FUSED_BELOW
// mode 2: calls of fewer paths than this fuse (one rank of a 4- or 8-way sharded 4K frame, 1080p frames); a full 4K x 4 spp frame (33 M)
// keeps its own launches
#define PT_FUSED_BELOW (12u << 20)
#endif
#ifndef PT_COMPACT_POOL
// pt_render keeps the live paths' state compacted by queue position (ptk::PathPool::home; environment MI355PT_COMPACT_POOL overrides)
#define PT_COMPACT_POOL 1
#endif
#ifndef PT_FIRST_VERTEX_IN_PLACE
// pt_render's compacted batches start without k_generate: the first pass's launches form the vertex-0 state where they use it (ptk::FirstVertex;
// environment MI355PT_FIRST_VERTEX_IN_PLACE overrides)
#define PT_FIRST_VERTEX_IN_PLACE 1
#endif
#ifndef PT_FIRST_VERTEX_PACKETS
// ... and that first pass traces its camera rays as packets on one shared stack per wave (pt_traverse8k.h; environment MI355PT_FIRST_VERTEX_PACKETS overrides):
// 0: k_extend_first, one ray per lane pair; 1: 32-ray packets in the lane-pair layout; 2: 64-ray packets, one lane per ray
#define PT_FIRST_VERTEX_PACKETS 2
#endif
#ifndef PT_PACKET_PRECULL
// ... and a node step of the 64-ray packets culls the node's children against the packet as a whole before the per-ray slab tests (pt_packet_precull.h; environment
// MI355PT_PACKET_PRECULL overrides; 0: every child is tested for every ray)
#define PT_PACKET_PRECULL 1
#endif
#ifndef PT_DROP_INERT_TERMINAL
// pt_render: k_classify leaves out the hits of terminating paths (PF_terminateAtNextBounce) on primitives that can neither emit nor stand in for an analytic light — their
// vertex would change nothing anybody reads (pt_wavefront.hip k_classify; environment MI355PT_DROP_INERT_TERMINAL overrides)
#define PT_DROP_INERT_TERMINAL 1
#endif
#ifndef PT_FREE_RUN_BELOW
// pt_render: once every live batch holds fewer paths than this, the batches stop advancing in lockstep (0: lockstep to the end)
#define PT_FREE_RUN_BELOW (1u << 22)
#endif
#ifndef PT_TEXTURE_STAGING_BYTES
// the pinned staging buffer a device texture ingest streams the source pixels through, both halves together (pt_texture_ingest.hip; MI355PT_TEXTURE_STAGING_BYTES: tests)
#define PT_TEXTURE_STAGING_BYTES (64u << 20)
#endif
#ifndef PT_PIPELINE_BATCHES
// independent sub-frame batches pt_render keeps in flight on separate streams (A/B on C3 in DESIGN.md)
#define PT_PIPELINE_BATCHES 4
#endif
// a full task queue is reported as an error (pt_render), it does not silently disable splitting

#pragma GCC visibility pop
struct pt_context {      // (the type include/mi355pt.h names: default visibility, like its declaration there)
    int device = 0; hipStream_t stream = nullptr; uint shardRank = 0, shardCount = 1;
    // streams / hostCounters: one stream and one pinned counter block per pipelined batch (pt_render, pt_fill_stable_planes)
    hipStream_t streams[PT_PIPELINE_BATCHES] = {}; WaveCounters* hostCounters = nullptr; bool serialKernels = false;
    struct { uint enable = 0u, filter = 1u, magnification = 0u; float gaussianSigma = 0.3f; } stf;      // pt_set_texture_filtering (defaults: SampleUI.h:185-187); S._pad carries enable + filter to the launchers (pt_path.h stf_set_launch_filter)
    uint tailBelow = PT_TAIL_PATHS, tailDefer = 0, fusedTraversal = PT_FUSED_TRAVERSAL; bool occlusionSlotOrder = true, compactPool = PT_COMPACT_POOL != 0, firstVertexInPlace = PT_FIRST_VERTEX_IN_PLACE != 0;
    // vertex 0 as packets (ptk::FirstPackets): the switch (0 / 1 / 2, as above), the step cap and stack bound of a packet (0: T8_PACKET_STEP_CAP or T8_PACKET64_STEP_CAP / T8_PACKET_STACK), the leftover list (one word per path)
    uint firstVertexPackets = PT_FIRST_VERTEX_PACKETS; uint packetStepCap = 0, packetStack = 0; DevBuf<uint> dFirstLeftover;
    bool packetPrecull = PT_PACKET_PRECULL != 0;      // the 64-ray packets' interval test of a node's children (FirstPackets::precull)
    // pt_render's classified passes drop the terminal hits that can add nothing (k_classify, pt_wavefront.hip); droppedTerminal: how many the last pt_render call dropped
    bool dropInertTerminal = PT_DROP_INERT_TERMINAL != 0; unsigned long long droppedTerminal = 0;
    std::string lastError;
    // host copies of the scene (kept for re-bake / animation)
    std::vector<uint> indices; std::vector<float> positions; std::vector<ptk::float2> uvs; std::vector<uint> normals, tangents;
    std::vector<GeometryDesc> geometries; std::vector<MeshDesc> meshes; std::vector<InstanceDesc> instances;
    std::vector<ptk::PTMaterialData> materials; std::vector<HostTexture> textures; HostTexture envTex; bool envEnabled = false;
    float3x4 envToWorld, envToLocal; ptk::float3 envColorMul;
    // sceneDirLights: world-space lights of the loaded scene (pt_set_scene_directional_lights), converted at bake time
    uint envCubeDim = 2048; std::vector<ptk::EnvDirectionalLight> envDirLights, sceneDirLights; bool envCubeDirty = true;
    ptk::EnvCube envCube;      // EnvMapBaker state (pt_set_environment_bake)
    std::vector<PolymorphicLightInfoFull> analyticLights;
    std::vector<SubInstanceData> subInstances; std::vector<ptk::uint2> subInstToInstGeom; std::vector<ptk::uint2> primInfo;
    std::vector<uint> subInstFirstPrim;
    // (light weights / proxy table live on the device only)
    std::vector<ptk::PolymorphicLightInfo> lights; std::vector<ptk::PolymorphicLightInfoEx> lightsEx; std::vector<uint> envLookup;
    uint envLookupDim = 0; uint numProxies = 0, envLightsBaked = 0;
    DevBuf<float> dLightW; DevBuf<uint> dProxyOffsets; void* dScanTemp = nullptr; size_t scanTempBytes = 0;
    // device
    DevBuf<uint> dIndices, dNormals, dTangents, dProxyCounters, dProxyIndices, dEnvLookup, dOwned, dQueue[2], dEmissiveList, dEmissiveOffsets;
    // pt_set_motion_history: the previous frame's pose; the (first, count) vertex ranges in which it differs from the current one
    DevBuf<float> dPrevPositions; DevBuf<InstanceDesc> dPrevInstances; bool motionHistory = false, prevAllStale = false;
    std::vector<uint32_t> prevStaleRanges;
    // pt_set_skinning: the description on the device (skinRanges: the host's copy of its ranges; skinStale: the (first, count) pairs of the ranges, what a device pose makes
    // stale in the previous pose and in the host copies above). mirrorsStale: a device pose has rewritten dPositions / dNormals / dTangents since `positions` / `normals` /
    // `tangents` were last equal to them (sync_mirrors brings mirrorRanges back before anything reads the host copies). skinMs: k_skin's device time in the last pt_animate_skinned
    bool skinSet = false, mirrorsStale = false; std::vector<PtSkinRange> skinRanges; std::vector<uint32_t> skinStale, mirrorRanges; uint32_t skinMatrices = 0, skinWeights = 0; double skinMs = 0;
    DevBuf<uint16_t> dSkinJoints; DevBuf<float> dSkinWeights, dSkinNormals, dSkinTangents, dSkinBind, dSkinDeltaP, dSkinDeltaN, dSkinDeltaT; DevBuf<PtSkinRange> dSkinRanges;
    DevBuf<uint32_t> dSkinRangeStart; DevBuf<double> dSkinMatrices, dSkinMorphWeights; SkinView skinView = {}; hipEvent_t skinEvents[2] = {nullptr, nullptr};
    DevBuf<float> dPositions; DevBuf<ptk::float2> dUvs; DevBuf<GeometryDesc> dGeometries; DevBuf<InstanceDesc> dInstances;
    DevBuf<SubInstanceData> dSubInstances;
    DevBuf<ptk::AlphaPlane> dAlphaPlanes; DevBuf<unsigned char> dAlphaPool; DevBuf<ptk::ShadeTri> dShadeTris;
    DevBuf<uint> dInertBits;      // two bits per global primitive: "inert when terminal" (pt_scene.h inert_bits_of, pt_build.hip k_inert_bits)
    DevBuf<ptk::uint2> dSubInstToInstGeom, dPrimInfo; DevBuf<ptk::PTMaterialData> dMaterials; DevBuf<TexInfo> dTexInfos; DevBuf<ptk::float4> dTexels;
    // pt_set_procedural_sky
    bool skyEnabled = false; ptk::ProceduralSkyContext sky; DevBuf<ptk::float4> dSkyTex[4]; DevBuf<ptk::ProceduralSkyContext> dSky;
    DevBuf<ptk::uint2> dSkyLowRes;
    // pt_set_environment_cube: the environment image as a cube map (RGBA16F), uploaded by the setter
    DevBuf<ptk::uint2> dEnvImageCube; uint envImageCubeDim = 0;
    // envCompression: EnvMapBaker's BC6U compression (0 off, 1 fast)
    DevBuf<ptk::uint2> dEnvCube, dEnvCubeSource; DevBuf<ptk::EnvDirectionalLight> dEnvDirLights; uint envCompression = 0;
    DevBuf<ptk::PolymorphicLightInfo> dLights; DevBuf<ptk::PolymorphicLightInfoEx> dLightsEx;
    // NEE-AT (pt_set_local_light_sampling): the screen-tile local samplers as the host hands them in, and the feedback reservoirs of the
    // last pt_render call (one plane per sample)
    DevBuf<uint> dLocalTable; uint localResX = 0, localResY = 0, localJitterX = 0, localJitterY = 0, localMaxLight = 0;
    float localRatio = 0.f, sscThreshold = 0.f; bool feedbackRequired = false;
    DevBuf<float> dFbWeight; DevBuf<uint> dFbCand; DevBuf<ptk::float4> dSq3; uint fbSamples = 0;
    // pt_set_light_importance_boost: ImportanceBooster's frustum term (mul 0: off)
    ptk::LightFrustumBoost lightBoost = {}; bool weightsDirty = false;
    // NEE-AT with the baker in the loop (pt_set_neeat): what LightsBaker keeps between frames (LightsBaker.h:225-260) and the textures /
    // buffers its feedback passes bind
    struct NeeAt {
        bool enabled = false; float globalFeedbackWeight = 0.75f, localRatio = 0.65f, sscThreshold = 0.3f, dropoff = 0.005f, intensityDeltaMul = 64.0f;
        bool preFilter = true;
        uint updateCounter = 0; float jitterF[2] = {0, 0}; uint jitter[2] = {0, 0}, prevJitter[2] = {0, 0};
        bool feedbackFilled = false, lastFeedbackAvailable = false; uint historicTotalLightCount = 0, W = 0, H = 0, nHist = 0;
        // between UpdateBegin and UpdateEnd of a frame (realtime mode: the build pass runs in between)
        bool frameOpen = false, frameFeedbackAvailable = false, frameLocalAvailable = false, exportDepth = true; uint framePrevLightCount = 0;
        DevBuf<float> fbW, scW, blW, snapW, curW, histW; DevBuf<uint> fbC, scC, blC, snapC, local, counters;
        // the exported depth of the last traced frame / of the one before; columns 2 and 3 of pt_set_view_projection's matrix
        DevBuf<float> depth, histDepth; bool haveClip = false; float clipZ[4] = {0, 0, 0, 0}, clipW[4] = {0, 0, 0, 0};
        void reset() {
            W = H = 0; updateCounter = 0; jitterF[0] = jitterF[1] = 0; jitter[0] = jitter[1] = prevJitter[0] = prevJitter[1] = 0;
            feedbackFilled = lastFeedbackAvailable = false; frameOpen = false; exportDepth = true; historicTotalLightCount = 0; nHist = 0;
        }
        void free() {
            fbW.free(); scW.free(); blW.free(); snapW.free(); curW.free(); histW.free(); fbC.free(); scC.free(); blC.free(); snapC.free();
            local.free(); counters.free(); depth.free(); histDepth.free();
        }
    } neeat;
    // the path pool (ensure_pool). ...b: the second array set of a compacted pool (pt_render)
    DevBuf<ptk::uint4> dS0, dS1, dS2, dS3, dS4, dHit, dS0b, dS1b, dS3b, dS4b, dHitb; DevBuf<ptk::float4> dSq0, dSq1, dSq2, dAccum, dScratch4;
    DevBuf<WaveCounters> dCounters; DevBuf<ptk::uint2> dTravSpill; DevBuf<ptk::TravTask> dTaskQ; DevBuf<uint> dTravCounts, dResolveList;
    DevBuf<unsigned long long> dBestKey;
    // ...Sh: the visibility rays' own straggler state in a frame of fused traversal launches
    DevBuf<ptk::TravTask> dTaskQSh; DevBuf<uint> dResolveListSh; DevBuf<unsigned long long> dBestKeySh;
    std::vector<TexInfo> texInfos; TexInfo envTexInfo;
    // textures (pt_texture_ingest.hip). deviceTextures: PT_DEVICE_TEXTURES_ON_DEVICE — `textures` then holds sizes only. texFormats: the source format of every texture;
    // alphaPlanes: the host's copy of the plane table; matTexels: the texels of the material textures in the pool, where the environment image starts; texStagingBytes: the
    // pinned staging buffer of an ingest, both halves; texStats: of the last ingest or update; texHostMs: the host time of the last pt_set_materials
    bool deviceTextures = false; std::vector<uint> texFormats; std::vector<ptk::AlphaPlane> alphaPlanes; size_t matTexels = 0, texStagingBytes = PT_TEXTURE_STAGING_BYTES;
    PtTextureIngestStats texStats = {}; double texHostMs = 0;
    BvhBuildBuffers bvh; bool bvhAllocated = false; uint numTris = 0; uint bvhBuilder = BVH_BUILDER_SAH;
    DeviceScene dsc;
    // frame state
    ptk::PtSettings S; ptk::PathTracerCameraData cam; uint width = 0, height = 0, accumCount = 0; std::vector<uint> owned;
    std::vector<std::vector<uint>> shardPixels;
    std::vector<float> hostRadiance; bool countersEnabled = false;
    bool geomDirty = true, lightsDirty = true, texDirty = true;
    double buildMs = 0, refitMs = 0, lightBakeMs = 0;
    uint poolCapacity = 0; size_t shadowCapacity = 0;
    // stable planes (pt_build_stable_planes): the realtime mode's per-frame buffers (RenderTargets.cpp:60-141, 340-352) of the last pre-pass
    DevBuf<uint> dSpHeader, dSpThroughput; DevBuf<ptk::StablePlane> dSpPlanes; DevBuf<ptk::uint2> dSpRadiance, dSpMotion;
    DevBuf<float> dSpDepth, dSpHitT; uint spW = 0, spH = 0; bool spGathered = false;
    DevBuf<ptk::uint4> dSpMark; DevBuf<ptk::float4> dSpNewL;      // scratch of the fill passes
    DevBuf<float> dSpScratch;
    // the denoiser buffers (pt_denoiser_prepare_dlss_rr / _nrd, pt_denoiser.h), allocated zeroed for a frame size by the first prepare call
    DevBuf<uint> dDnRRDiff, dDnRRSpec, dDnRRSpecMV; DevBuf<ptk::uint2> dDnRRNormal, dDnMotion; DevBuf<float> dDnViewZ, dDnRoughness;
    DevBuf<ptk::float4> dDnNormal, dDnDiff, dDnSpec;
    DevBuf<unsigned char> dDnDisocclusion, dDnHistoryClamp; uint dnW = 0, dnH = 0;
    // the sample index of the last build pass: Bridge::getSampleIndex's sampleBaseIndex for the NRD pass's camera rays
    uint spSampleBase = 0;
    // the device denoiser (pt_denoise_plane; pt_relax.h). Per plane: the history of the previous and of the current frame, five records a pixel each (ptk::RelaxHistory), and the
    // two denoised buffers; shared by the planes: the guide records and the a-trous ping-pong pairs. dnPreparedPlane: the plane the last pt_denoiser_prepare_nrd of this frame
    // left in the NRD buffers (-1: none, or already denoised). rxSide: which of the two histories is the previous frame's. spFrameSerial counts the build passes; rxFrameSerial:
    // the build pass a plane's history is of — a history older than the previous build pass (a plane that was not denoised in between) is not used.
    DevBuf<ptk::float4> dRxHist[3][2][5], dRxOut[3][2], dRxGuide, dRxPing[2], dRxPong[2];
    uint rxW = 0, rxH = 0, rxSide[3] = {0, 0, 0}; bool rxHistory[3] = {false, false, false}, rxDenoised[3] = {false, false, false}; int dnPreparedPlane = -1;
    uint spFrameSerial = 0, rxFrameSerial[3] = {0, 0, 0};
    // diagnostic only (pt_denoise_pass_times, for tools/denoise_probe.py): off unless asked for; when off pt_denoise_plane records no event
    bool rxTiming = false; std::vector<float> rxPassMs; std::vector<hipEvent_t> rxEvents;
    // the temporal anti-aliasing resolve (pt_taa_resolve; pt_taa.h): the reference's two feedback buffers; taaSide: the one written last (the resolved picture), the other one
    // is its history. taaFrameSerial: the build pass the resolved picture is of (rxFrameSerial's rule). dnNrdSerial: the build pass of the last pt_denoiser_prepare_nrd — the
    // relax buffer is read only when it is the current one.
    DevBuf<ptk::float4> dTaa[2]; uint taaW = 0, taaH = 0, taaSide = 0, taaFrameSerial = 0, dnNrdSerial = 0; bool taaHistory = false, taaResolved = false;
    EventBracket taaEvents;
    // the bloom pass (pt_bloom; pt_bloom.h) at the frame size: the source (the radiance buffer, dTaa[taaSide] or the denoised accumulation) is never written
    BloomState bloom;
    // the temporal upscaling resolve (pt_taa_upscale; pt_taau.h): two display-size buffers that swap as dTaa's do (taauSide: the upscaled picture, the other one its history),
    // of taauW x taauH pixels, resolved from a frame of taauRenderW x taauRenderH; a serial of its own under taaFrameSerial's rule. taauBloom: the display tail's bloomed
    // picture (pt_bloom_upscaled), of the display size: separate from `bloom`.
    DevBuf<ptk::float4> dTaau[2]; uint taauW = 0, taauH = 0, taauRenderW = 0, taauRenderH = 0, taauSide = 0, taauFrameSerial = 0;
    bool taauHistory = false, taauResolved = false;
    EventBracket taauEvents; BloomState taauBloom;
    // adaptive sampling (pt_render_adaptive; pt_adaptive.h). perPixel: the accumulation buffer holds per-pixel sample counts — pt_render refuses until the accumulation is reset.
    // tableValid: ownedBlocks / dBlkOwned describe the current owned list (its 8 x 8 blocks as runs of the list; built at first use, dropped by pt_resize). stateValid: dHalf,
    // dCounts, dBlockError and the active lists are the last adaptive render's, of this frame size. The active lists: the owned list and its block table before the first
    // evaluation that retires something, then one of the two list pairs (activePix / activeBlk point at the current one). hostTotals: pinned, two words.
    struct Adaptive {
        bool perPixel = false, tableValid = false, stateValid = false;
        std::vector<ptk::AdaptiveBlock> ownedBlocks; DevBuf<ptk::AdaptiveBlock> dBlkOwned, dBlk[2]; DevBuf<uint> dPix[2], dCounts, dTotals; DevBuf<ptk::float4> dHalf;
        DevBuf<float> dBlockError; DevBuf<ptk::uint2> dFlags, dChunks; uint* hostTotals = nullptr;
        const uint* activePix = nullptr; const ptk::AdaptiveBlock* activeBlk = nullptr; uint activeCount = 0, activeBlocks = 0;
    } adaptive;
    // the reference-mode denoiser (pt_accum_denoise; pt_accum_denoise.h): the denoised picture and the prepare launch's three outputs (H' with valid(p) in .w, O', V), of
    // w x h pixels; ready: they are a call's, of this frame size, and the accumulation has not been reset since. dInA / dInH: pt_accum_denoise_host_inputs' copies of the
    // caller's pictures (dAccum and adaptive.dHalf are never written).
    struct AccumDenoise {
        DevBuf<ptk::float4> dOut, dStageH, dStageO, dVar, dInA, dInH; uint w = 0, h = 0; bool ready = false;
        EventBracket events;
    } accumDenoise;
    // the exchanges of tile shards (pt_shard.hip): the communicator of pt_comm_init, of shardRank / shardCount
    ncclComm_t comm = nullptr; ShardStaging staging;
};

#pragma GCC visibility push(hidden)

inline int fail(pt_context* c, int code, const std::string& msg) { if (c) c->lastError = msg; return code; }
#define PT_CHECK_HIP(c, expr) \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(c, PT_ERROR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
// the packets of the context's settings (ptk::FirstPackets): the traverser of c->firstVertexPackets (2: 64-ray packets) with or without the interval test; stepCap / stackBound 0: that traverser's default
inline FirstPackets first_packets(const pt_context* c, uint* leftover, uint* leftoverCount, uint capacity, uint stepCap, uint stackBound) {
    const bool wide = c->firstVertexPackets == 2u;
    return FirstPackets{leftover, leftoverCount, capacity, stepCap ? stepCap : (wide ? (uint)T8_PACKET64_STEP_CAP : (uint)T8_PACKET_STEP_CAP), stackBound ? stackBound : (uint)T8_PACKET_STACK, wide ? 1u : 0u, c->packetPrecull ? 1u : 0u}; }

// ---- pt_shard.hip
void build_shards(pt_context* c);                    // the shard lists of the frame size (pt_resize)
int neeat_exchange_feedback(pt_context* c);          // tile shards with a communicator: the other ranks' reservoirs and depth, before UpdateBegin
int sp_exchange_guides(pt_context* c);               // ... and the build pass's depth and motion vectors, before UpdateEnd
// ---- pt_api.hip, for the frame drivers
int prepare(pt_context* c);                          // whatever is dirty — textures, environment cube, geometry, lights — brought up to date
// One frame of LightsBaker::UpdateBegin (NEEAT_BEGIN) / UpdateEnd (NEEAT_END) for the NEE-AT layer; see the definition
enum { NEEAT_BEGIN = 1, NEEAT_END = 2, NEEAT_BOTH = 3 };
int neeat_frame(pt_context* c, int phases = NEEAT_BOTH, const float* depth = nullptr, const ptk::uint2* motion = nullptr);
// the planes of the whole frame must be here: an unsharded context, or a sharded one after pt_gather_stable_planes / pt_unpack_stable_planes (the NRD pass reads neighbours)
inline int32_t dn_ready(pt_context* c) {
    if (!c->spW || c->spW != c->width || c->spH != c->height) return fail(c, PT_ERROR_NOT_READY, "no stable planes of this frame size yet: pt_build_stable_planes, pt_fill_stable_planes");
    if (c->shardCount > 1 && !c->spGathered) return fail(c, PT_ERROR_NOT_READY, "the denoiser passes read the whole frame's planes: pt_gather_stable_planes / pt_unpack_stable_planes first");
    return PT_OK;
}
inline ptk::DenoiserBuffers dn_buffers(pt_context* c) {
    ptk::DenoiserBuffers D;
    D.RRDiffuseAlbedo = c->dDnRRDiff.p; D.RRSpecAlbedo = c->dDnRRSpec.p; D.RRNormalsAndRoughness = c->dDnRRNormal.p; D.RRSpecMotionVectors = c->dDnRRSpecMV.p;
    D.ViewZ = c->dDnViewZ.p; D.MotionVectors = c->dDnMotion.p; D.NormalRoughness = c->dDnNormal.p; D.DiffRadianceHitDist = c->dDnDiff.p; D.SpecRadianceHitDist = c->dDnSpec.p;
    D.Roughness = c->dDnRoughness.p; D.DisocclusionThresholdMix = c->dDnDisocclusion.p; D.CombinedHistoryClampRelax = c->dDnHistoryClamp.p;
    return D;
}
// ---- pt_skin.hip: the device skinning pass over the ranges of `s`, in place on the scene's streams
void launch_skin(const SkinView& s, const double* matrices, const double* morphWeights, float* positions, uint* normals, uint* tangents, hipStream_t st);
// ---- pt_texture_ingest.hip: the texture pool made on the device (PT_DEVICE_TEXTURES_ON_DEVICE). tex_plan_alpha_planes: the plane table of `textures` for the given plane
// formats (0 = bytes, 1 = floats) into c->alphaPlanes, and the bytes of the alpha pool — both paths' layout; tex_ingest_all: pt_set_materials' textures, from the caller's
// pixels to the pool, the chains and the planes; tex_update_one: pt_update_texture's fast path; tex_place_environment: the lat-long image behind the material textures
int tex_plan_alpha_planes(pt_context* c, const std::vector<uint>& fmts, size_t* poolBytes);
int tex_ingest_all(pt_context* c, const PtTextureDesc* tex, uint32_t n);
int tex_update_one(pt_context* c, uint32_t index, const PtTextureDesc* desc);
int tex_place_environment(pt_context* c);
// ---- pt_relax_api.hip: the device denoiser's history is dropped (resize to another size, new scene) / its buffers freed
void relax_drop_history(pt_context* c);
void relax_free(pt_context* c);
// ---- pt_taa_api.hip: the same two hooks for the temporal anti-aliasing resolve
void taa_drop_history(pt_context* c);
void taa_free(pt_context* c);
// ---- pt_bloom_api.hip: the frame-size bloomed picture is dropped (resize to another size) / the pass's buffers freed
void bloom_drop(pt_context* c);
void bloom_free(pt_context* c);
// ---- pt_taau_api.hip: the upscaling resolve's history, picture and bloomed picture are dropped (resize to another size, new scene) / its buffers freed
void taau_drop_history(pt_context* c);
void taau_free(pt_context* c);
// ---- pt_adaptive_api.hip: the adaptive state is dropped (resize, new shard lists) / its buffers freed
void adaptive_drop(pt_context* c);
void adaptive_free(pt_context* c);
// ---- pt_accum_denoise_api.hip: the denoised picture is dropped (resize, every reset of the accumulation) / the pass's buffers freed
void accum_denoise_drop(pt_context* c);
void accum_denoise_free(pt_context* c);
// ---- pt_frame.hip
// pt_render's frame over `numPixels` entries of a device pixel list (x << 16 | y) whose pixels all hold accumBase samples: samples [first, first + count) traced and folded in.
// pt_render passes the owned list and no round (and the call advances c->accumCount); pt_render_adaptive passes the active list and the round's AdaptiveRound.
int32_t render_pixel_list(pt_context* c, const uint* pixels, uint numPixels, uint32_t first, uint32_t count, uint accumBase, ptk::AdaptiveRound* round, PtFrameStats* stats);
// the stable-plane buffers of the context with a frame's constants; params == nullptr: zeroed params with all planes active (what the
// passes that only address the buffers need: pack / unpack, merge, read-back)
StablePlanesContext sp_context(pt_context* c, const PtStablePlanesParams* params);
// t += o for every additive field of PtFrameStats (the batches of a call, the samples of a call that traces them one frame at a time;
// maxima stay maxima)
void add_frame_stats(PtFrameStats& t, const PtFrameStats& o);

#pragma GCC visibility pop

// ORACLE pin (test infrastructure only): the driver around the reference's integrator text (PathTracer.hlsli, PathTracerNEE.hlsli,
// PathTracerNestedDielectrics.hlsli, LightSampler.hlsli, PolymorphicLight.hlsli, EnvMap.hlsli, PathState.hlsli, BxDF.hlsli ... compiled above).
//
// The reference leaves three things to its host: the `Bridge` (scene access: PathTracerBridgeDonut.hlsli, needs Donut + DXR), the raygen loop
// (PathTracerSample.hlsl:200-250) and the resource bindings. Here the Bridge is served by the ORACLE's scene services (its BVH, its loadSurface,
// its light table, its environment lookup: oracle/ptref/*), the loop is the dozen lines of refpt_render_rect below, and the bindings are the
// pointer-carrying stubs of hlsl_pt_stubs.h. Everything between "a ray hit something" and "the pixel's radiance" is the reference's own text —
// HandleHit, HandleMiss, nested dielectrics, NEE with its reservoir, MIS, Russian roulette, the packed PathState. tests compare the image this
// produces with the oracle's own integrator, bit for bit.

namespace hl {
struct PtDriver { const ptref::PathTracer* svc = nullptr; };        // per-thread oracle services (BVH queries and their counters)
static thread_local const PtDriver* g_drv = nullptr;
static inline ptref::float3 toP(float3 v) { return ptref::make_float3(v.x, v.y, v.z); }
static inline float3 toH(ptref::float3 v) { return float3(v.x, v.y, v.z); }
static float4 env_fetch(const void* ctx, float3 localDir, float lod) {          // no environment: the reference binds a black texture
    const ptref::EnvMap* e = (const ptref::EnvMap*)ctx; if (!e->enabled) return float4(0, 0, 0, 1);
    ptref::float3 c = e->EvalLocal(toP(localDir), lod); return float4(c.x, c.y, c.z, 1.0f); }

// The bindings of one frame (Sample.cpp:2315-2427), built from the oracle's scene: Donut-style instance / geometry records over two byte-address
// buffers (indices; positions | texcoords | normals | tangents), the material and sub-instance tables, the light tables, the environment.
struct FrameBindings {
    std::vector<InstanceData> instances; std::vector<GeometryData> geometries; std::vector<GeometryDebugData> geometryDebug; std::vector<unsigned char> vertexBytes;
    std::vector<SubInstanceData> subInstances;
    ByteAddressBuffer buffers[2]; std::vector<Texture2D<float4> > textures; LightingControlData control; ptref::EnvMap envRaw;
    void bind(const ::Context* c, uint sampleIndex) {
        const ptref::Scene& sc = c->sc;
        const size_t nv = sc.positions.size();
        const uint posBase = 0, uvBase = (uint)(nv * 12), nBase = uvBase + (uint)(sc.uvs.size() * 8), tBase = nBase + (uint)(sc.normals.size() * 4);
        const bool havePrevPos = sc.prevPositions.size() == nv && nv, havePrevInst = sc.prevInstances.size() == sc.instances.size();      // ptref_set_previous_pose
        const uint prevBase = tBase + (uint)(sc.tangents.size() * 4);
        vertexBytes.resize((size_t)prevBase + (havePrevPos ? nv * 12 : 0) + 16);
        if (havePrevPos) memcpy(&vertexBytes[prevBase], sc.prevPositions.data(), nv * 12);
        if (nv) memcpy(&vertexBytes[posBase], sc.positions.data(), nv * 12);
        if (sc.uvs.size()) memcpy(&vertexBytes[uvBase], sc.uvs.data(), sc.uvs.size() * 8);
        if (sc.normals.size()) memcpy(&vertexBytes[nBase], sc.normals.data(), sc.normals.size() * 4);
        if (sc.tangents.size()) memcpy(&vertexBytes[tBase], sc.tangents.data(), sc.tangents.size() * 4);
        buffers[0].p = (const unsigned char*)sc.indices.data(); buffers[1].p = vertexBytes.data();
        geometries.resize(sc.geometries.size()); geometryDebug.assign(sc.geometries.size(), GeometryDebugData{-1, 0xFFFFFFFFu});
        for (size_t g = 0; g < sc.geometries.size(); g++) {
            const ptref::GeometryDesc& d = sc.geometries[g]; GeometryData& o = geometries[g];
            o.indexBufferIndex = 0; o.vertexBufferIndex = 1; o.indexOffset = d.indexOffset * 4; o.positionOffset = posBase + d.vertexOffset * 12; o.prevPositionOffset = havePrevPos ? prevBase + d.vertexOffset * 12 : 0xFFFFFFFFu;      // (Donut: skinned meshes only; a copy of unmoved vertices interpolates to the same point)
            o.texCoord1Offset = (d.flags & ptref::GEOM_HAS_UV) ? uvBase + d.vertexOffset * 8 : ~0u;
            o.normalOffset = (d.flags & ptref::GEOM_HAS_NORMAL) ? nBase + d.vertexOffset * 4 : ~0u;
            o.tangentOffset = (d.flags & ptref::GEOM_HAS_TANGENT) ? tBase + d.vertexOffset * 4 : ~0u;
            o.materialIndex = d.materialIndex;
        }
        instances.resize(sc.instances.size());
        for (size_t i = 0; i < sc.instances.size(); i++) {
            const ptref::InstanceDesc& d = sc.instances[i]; InstanceData& o = instances[i];
            for (int r = 0; r < 3; r++) o.transform.r[r] = o.prevTransform.r[r] = float4(d.transform.m[4 * r], d.transform.m[4 * r + 1], d.transform.m[4 * r + 2], d.transform.m[4 * r + 3]);
            if (havePrevInst) { const ptref::InstanceDesc& q = sc.prevInstances[i]; for (int r = 0; r < 3; r++) o.prevTransform.r[r] = float4(q.transform.m[4 * r], q.transform.m[4 * r + 1], q.transform.m[4 * r + 2], q.transform.m[4 * r + 3]); }
            o.firstGeometryIndex = sc.meshes[d.meshIndex].firstGeometry; o.firstGeometryInstanceIndex = sc.instFirstSubInstance[i]; o.numGeometries = sc.meshes[d.meshIndex].numGeometries; o.flags = 0;
        }
        textures.resize(sc.textures.size());
        for (size_t t = 0; t < sc.textures.size(); t++) textures[t].tex = &sc.textures[t];
        t_InstanceData.p = instances.data(); t_GeometryData.p = geometries.data(); t_GeometryDebugData.p = geometryDebug.data();
        static_assert(sizeof(SubInstanceData) == sizeof(ptref::SubInstanceData) && sizeof(PTMaterialData) == sizeof(ptref::PTMaterialData), "table layouts");
        subInstances.resize(sc.subInstances.size());          // SUBINSTANCEDATA_EXTENDED: the alpha test reads its buffer indices / offsets from here (SubInstanceData.h:37-42)
        for (size_t k = 0; k < sc.subInstances.size(); k++) {
            memcpy(&subInstances[k], &sc.subInstances[k], sizeof(SubInstanceData));
            const GeometryData& g = geometries[sc.subInstances[k].GlobalGeometryIndex_PTMaterialDataIndex >> 16];
            subInstances[k].IndexBufferIndex_VertexBufferIndex = (g.indexBufferIndex << 16) | g.vertexBufferIndex; subInstances[k].IndexOffset = g.indexOffset; subInstances[k].TexCoord1Offset = g.texCoord1Offset;
        }
        t_SubInstanceData.p = subInstances.data(); t_PTMaterialData.p = (const PTMaterialData*)sc.materials.data();
        t_BindlessBuffers.b = buffers; t_BindlessTextures.t = textures.data();
        // constants (UpdatePathTracerConstants, Sample.cpp:1464-1556)
        memset(&g_Const, 0, sizeof(g_Const)); memset(&g_MiniConst, 0, sizeof(g_MiniConst));
        static_assert(sizeof(PathTracerCameraData) == sizeof(ptref::PathTracerCameraData), "camera layout");
        PathTracerConstants& k = g_Const.ptConsts;
        memcpy(&k.camera, &c->cam, sizeof(k.camera));
        k.imageWidth = c->w; k.imageHeight = c->h; k.sampleBaseIndex = sampleIndex; k.perPixelJitterAAScale = c->S.perPixelJitterAAScale;
        k.bounceCount = c->S.bounceCount; k.diffuseBounceCount = c->S.diffuseBounceCount; k.EnvironmentMapDiffuseSampleMIPLevel = c->S.envMapDiffuseSampleMIPLevel;
        k.texLODBias = c->S.texLODBias; k.invSubSampleCount = 1.0f; k.fireflyFilterThreshold = c->S.fireflyFilterThreshold;
        k.NEEEnabled = c->S.NEEEnabled; k.NEEType = c->S.NEEType; k.NEECandidateSamples = c->S.NEECandidateSamples; k.NEEFullSamples = c->S.NEEFullSamples;
        g_Const.MaterialCount = (uint)sc.materials.size();
        for (int r = 0; r < 3; r++) { g_Const.envMapSceneParams.Transform.r[r] = float4(sc.env.toWorld.m[4 * r], sc.env.toWorld.m[4 * r + 1], sc.env.toWorld.m[4 * r + 2], sc.env.toWorld.m[4 * r + 3]);
                                      g_Const.envMapSceneParams.InvTransform.r[r] = float4(sc.env.toLocal.m[4 * r], sc.env.toLocal.m[4 * r + 1], sc.env.toLocal.m[4 * r + 2], sc.env.toLocal.m[4 * r + 3]); }
        g_Const.envMapSceneParams.ColorMultiplier = toH(sc.env.colorMultiplier); g_Const.envMapSceneParams.Enabled = sc.env.enabled ? 1.0f : 0.0f;
        envRaw = sc.env; envRaw.colorMultiplier = ptref::make_float3(1.f);
        t_EnvironmentMap.fetch = env_fetch; t_EnvironmentMap.ctx = &envRaw;
        // the guide-buffer dump of reference mode (Bridge::ExportSurface / ExportNonSurface, compiled above): depth only, and only when the host gave its world-to-clip matrix
        for (int r = 0; r < 4; r++) g_Const.view.matWorldToClip.r[r] = float4(sc.worldToClip[4 * r], sc.worldToClip[4 * r + 1], sc.worldToClip[4 * r + 2], sc.worldToClip[4 * r + 3]);
        u_Depth.p = sc.depthExport; u_Depth.w = c->w; u_Depth.h = c->h;
        // light tables (LightsBaker output). NEEType 0/1: no local layer, no temporal feedback (SampleUI.h:127, LightsBaker.cpp:998-1004); NEE-AT: the
        // tile tables and the control values come from ptref_set_local_light_sampling, the feedback textures are the context's planes (render_rect binds them per sample)
        const ptref::LightTable& T = sc.lightTable;
        memset(&control, 0, sizeof(control));
        control.TotalLightCount = T.TotalLightCount; control.SamplingProxyCount = T.SamplingProxyCount; control.ImportanceSamplingType = c->S.NEEType;
        control.LocalToGlobalSampleRatio = T.LocalToGlobalSampleRatio; control.ScreenSpaceVsWorldSpaceThreshold = T.ScreenSpaceVsWorldSpaceThreshold; control.TemporalFeedbackRequired = T.TemporalFeedbackRequired;
        control.LocalSamplingResolution = T.LocalSamplingBuffer ? uint2(T.LocalResX, T.LocalResY) : uint2(1, 1); control.LocalSamplingTileJitter = uint2(T.LocalJitterX, T.LocalJitterY);
        t_LightLocalSamplingBuffer.p = T.LocalSamplingBuffer; t_LightLocalSamplingBuffer.n = T.LocalResX * T.LocalResY * RTXPT_LIGHTING_LOCAL_PROXY_COUNT;      // (SampleLocalPDF's binary search can leave the buffer)
        static_assert(sizeof(PolymorphicLightInfo) == sizeof(ptref::PolymorphicLightInfo) && sizeof(PolymorphicLightInfoEx) == sizeof(ptref::PolymorphicLightInfoEx), "light record layout");
        t_LightsCB.p = &control; t_Lights.p = (const PolymorphicLightInfo*)T.Lights; t_LightsEx.p = (const PolymorphicLightInfoEx*)T.LightsEx;
        t_LightProxyCounters.p = T.ProxyCounters; t_LightProxyIndices.p = T.ProxyIndices; t_EnvLookupMap.p = T.EnvLookupMap; t_EnvLookupMap.w = t_EnvLookupMap.h = T.EnvLookupDim;
    }
};

// ---- Bridge: everything that is RTXPT's own text in PathTracerBridgeDonut.hlsli was compiled above (sample index, bounce limits, computeCameraRay,
// createTextureSampler, loadSurface, updateOutsideIoR, loadIoR, loadHomogeneousVolumeData, CreateEnvMap, CreateLightSampler, ...). What is left
// for the driver are the functions built on DXR ray queries (served by the oracle's BVH) and the G-buffer / motion-vector exports (no-ops here).
float3 Bridge::computeSkyMotionVector(uint2) { return float3(0, 0, 0); }
bool Bridge::traceVisibilityRay(RayDesc ray, RayCone, int, DebugContext) {                             // :993-1027: visible iff nothing committed (alpha test + ExcludeFromNEE inside)
    const ptref::PathTracer* t = g_drv->svc;
    if (t->counters) t->counters->shadowRays++;
    return ptref::trace_visibility(t->sc, toP(ray.Origin), toP(ray.Direction), ray.TMin, ray.TMax, t->counters ? &t->counters->nodeVisitsSh : 0, t->counters ? &t->counters->triTestsSh : 0);
}
void Bridge::traceScatterRay(PathState, RayQuery<RAY_FLAG_NONE, RTXPT_FLAG_ALLOW_OPACITY_MICROMAPS>&, float2, DebugContext) {}
} // namespace hl

namespace hl {
// ---- LightsBaker.hlsl: the NEE-AT feedback passes as the reference's own text, behind the interface ptref_api.cpp's neeat_frame drives (OracleNeeAtPasses is the other
// implementation). The host side of a frame — constants, order of the passes, jitter (LightsBaker.cpp) — is neeat_frame's restatement; the bindings below are what
// FillBindings + the control buffer hold for the pass at hand. History is read at the same pixel (EnableMotionReprojection 0), the light remap is the identity, and
// PreFilter's loads see the feedback as it was before the pass (its groups race in the reference; see rtxpt_amd/csrc/pt_neeat.h).
struct ReferenceNeeAtPasses {
    std::vector<uint> identity; std::vector<float> snapW; std::vector<uint> snapC;
    void bind(const ptref::NeeAtFrame& F) {
        LightingControlData& c = lbfb::g_ctrl; memset(&c, 0, sizeof(c)); LightsBakerConstants& b = lbfb::g_bakerConstants; memset(&b, 0, sizeof(b));
        c.TotalLightCount = F.totalLightCount; c.HistoricTotalLightCount = F.historicTotalLightCount; c.SamplingProxyCount = F.samplingProxyCount;
        c.LastFrameTemporalFeedbackAvailable = F.lastFrameFeedbackAvailable; c.LastFrameLocalSamplesAvailable = F.lastFrameLocalSamplesAvailable;
        c.LocalSamplingResolution = uint2(F.tilesX, F.tilesY); c.LocalSamplingTileJitter = uint2(F.jitterX, F.jitterY); c.LocalSamplingTileJitterPrev = uint2(F.jitterPrevX, F.jitterPrevY);
        b.FeedbackResolution = uint2(F.W, F.H); b.BlendedFeedbackResolution = uint2(F.BW, F.BH); b.UpdateCounter = F.updateCounter; b.ReservoirHistoryDropoff = F.dropoff;
        b.EnableMotionReprojection = 1; b.PrevOverCurrentViewportSize = float2(1, 1); b.DepthDisocclusionThreshold = F.depthDisocclusionThreshold;      // LightsBaker.cpp:1011-1018; the motion vectors are zero in reference mode
        b.MouseCursorPos = uint2(0x7FFFFFFF, 0x7FFFFFFF);
        lbfb::t_motionVectors.p = (const uint*)F.motion; lbfb::t_motionVectors.w = F.W;
        lbfb::t_depthBuffer.p = (float*)F.depth; lbfb::t_depthBuffer.w = F.W; lbfb::t_depthBuffer.h = F.H; lbfb::u_historyDepth.p = F.historyDepth; lbfb::u_historyDepth.w = F.W; lbfb::u_historyDepth.h = F.H;
        auto tex = [](auto& t, auto* p, uint w, uint h) { t.p = p; t.w = w; t.h = h; };
        tex(lbfb::u_feedbackTotalWeight, F.fbW, F.W, F.H); tex(lbfb::u_feedbackCandidates, F.fbC, F.W, F.H);
        tex(lbfb::u_feedbackTotalWeightScratch, F.scW, F.W, F.H); tex(lbfb::u_feedbackCandidatesScratch, F.scC, F.W, F.H);
        tex(lbfb::u_feedbackTotalWeightBlended, F.blW, F.BW, F.BH); tex(lbfb::u_feedbackCandidatesBlended, F.blC, F.BW, F.BH);
        lbfb::u_localSamplingBuffer.p = F.local; lbfb::u_lightSamplingProxies.p = (uint*)F.proxies; lbfb::u_perLightProxyCounters.p = F.perLightCounters;
        const uint n = F.historicTotalLightCount > F.totalLightCount ? F.historicTotalLightCount : F.totalLightCount;
        identity.resize(n + 1); for (uint i = 0; i <= n; i++) identity[i] = i; lbfb::u_historyRemapPastToCurrent.p = identity.data();
    }
    static uint div_ceil(uint a, uint b) { return (a + b - 1) / b; }
    template <class K> static void dispatch2d(uint gx, uint gy, uint t, K kernel) {      // kernels without barriers: every thread of every group, in dispatch order
        for (uint y = 0; y < gy * t; y++) for (uint x = 0; x < gx * t; x++) kernel(uint2(x, y));
    }
    void prefilter(const ptref::NeeAtFrame& F) {
        bind(F);
        snapW.assign(F.fbW, F.fbW + (size_t)F.W * F.H); snapC.assign(F.fbC, F.fbC + (size_t)F.W * F.H);
        const uint T = LLB_PREPROCESS_BLOCK_SIZE_OUTER;
        for (uint gy = 0; gy < div_ceil(F.H, LLB_PREPROCESS_BLOCK_SIZE_INNER); gy++) for (uint gx = 0; gx < div_ceil(F.W, LLB_PREPROCESS_BLOCK_SIZE_INNER); gx++) {
            lbfb::u_feedbackTotalWeight.p = snapW.data(); lbfb::u_feedbackCandidates.p = snapC.data();                  // the group's loads: the frame as it was before the pass
            lbfb::run_group(T * T, [&](uint t) { lbfb::ProcessFeedbackHistoryPreFilter(uint3(gx, gy, 0), uint3(t % T, t / T, 0)); },
                            [&](uint) { lbfb::u_feedbackTotalWeight.p = F.fbW; lbfb::u_feedbackCandidates.p = F.fbC; });     // after the barrier the stores go to the textures
        }
        lbfb::u_feedbackTotalWeight.p = F.fbW; lbfb::u_feedbackCandidates.p = F.fbC;
    }
    void p0(const ptref::NeeAtFrame& F, uint totalThreads) {
        bind(F); lbfb::g_ctrl.TotalMaxFeedbackCount = totalThreads;
        dispatch2d(div_ceil(F.W, LLB_NUM_COMPUTE_THREADS_2D), div_ceil(F.H, LLB_NUM_COMPUTE_THREADS_2D), LLB_NUM_COMPUTE_THREADS_2D, [](uint2 id) { lbfb::ProcessFeedbackHistoryP0(id); });
    }
    void p1a(const ptref::NeeAtFrame& F) { bind(F); dispatch2d(div_ceil(F.BW, 8), div_ceil(F.BH, 8), 8, [](uint2 id) { lbfb::ProcessFeedbackHistoryP1a(id); }); }
    void p1b(const ptref::NeeAtFrame& F) { bind(F); dispatch2d(div_ceil(F.W, 8), div_ceil(F.H, 8), 8, [](uint2 id) { lbfb::ProcessFeedbackHistoryP1b(id); }); }
    void p2(const ptref::NeeAtFrame& F) { bind(F); dispatch2d(div_ceil(F.tilesX, 8), div_ceil(F.tilesY, 8), 8, [](uint2 id) { lbfb::ProcessFeedbackHistoryP2(id); }); }
    void p3(const ptref::NeeAtFrame& F) {
        bind(F);
        for (uint ty = 0; ty < F.tilesY; ty++) for (uint tx = 0; tx < F.tilesX; tx++)
            lbfb::run_group(RTXPT_LIGHTING_LOCAL_PROXY_COUNT / 2, [&](uint t) { lbfb::ProcessFeedbackHistoryP3(uint3(tx, ty, 0), uint3(t, 0, 0)); });
    }
    void clear(const ptref::NeeAtFrame& F) { bind(F); dispatch2d(div_ceil(F.W, 8), div_ceil(F.H, 8), 8, [](uint2 id) { lbfb::ClearFeedbackHistory(id); }); }
};

// Renders pixels [x0,x1) x [y0,y1) of samples [first, first+n) into the context's accumulation buffer, like ptref_render_rect, but with the
// reference's integrator text between the hits. (Same accumulation: AccumulationPass.hlsl:36-66.)
static void render_rect(::Context* c, uint32_t first, uint32_t n, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) {
    ::prepare(c);
    const ptref::Scene& sc = c->sc;
    if (c->neeat.enabled) c->sc.feedbackRequired = true;
    c->beginFeedback(n);
    for (uint32_t s = 0; s < n; s++) {
        if (c->neeat.enabled) { ReferenceNeeAtPasses passes; ::neeat_frame(c, passes); }      // every sample is a frame: the reference's baker passes, then its path tracer
        FrameBindings frame; frame.bind(c, first + s);
        u_LightFeedbackTotalWeight.p = c->neeat.enabled ? c->neeat.fbW.data() : (c->fbSamples ? c->fbWeight.data() + (size_t)c->w * c->h * s : nullptr); u_LightFeedbackTotalWeight.w = c->w; u_LightFeedbackTotalWeight.h = 0;
        u_LightFeedbackCandidates.p = c->neeat.enabled ? c->neeat.fbC.data() : (c->fbSamples ? c->fbCand.data() + (size_t)c->w * c->h * s : nullptr); u_LightFeedbackCandidates.w = c->w; u_LightFeedbackCandidates.h = 0;
        const PathTracerConstants consts = g_Const.ptConsts;
        const float blend = 1.0f / (float)(c->accumCount + 1u);
#pragma omp parallel for schedule(dynamic, 4)
        for (int y = (int)y0; y < (int)y1; y++) {
            ptref::RayCounters rowCounters; memset(&rowCounters, 0, sizeof(rowCounters));
            ptref::PathTracer rowSvc(sc, c->S, c->cam, first + s, &rowCounters);      // per-row services: the counters are not shared between threads
            PtDriver rowDriver; rowDriver.svc = &rowSvc;
            g_drv = &rowDriver;
            std::vector<float4> row(c->w);
            PathTracer::WorkingContext workingContext;
            workingContext.PtConsts = consts; workingContext.OutputColor.p = row.data(); workingContext.OutputColor.w = 0;     // one row: index = x
            for (uint32_t x = x0; x < x1; x++) {
                // RAYGEN_ENTRY (PathTracerSample.hlsl:200-250)
                uint2 pixelPos = uint2(x, 0);
                PathState path = PathTracer::EmptyPathInitialize(uint2(x, (uint)y), consts.camera.PixelConeSpreadAngle);
                PathTracer::SetupPathPrimaryRay(path, Bridge::computeCameraRay(uint2(x, (uint)y)));
                PathTracer::StartPixel(path, workingContext);
                while (path.isActive()) {
                    // nextHit: TraceRay with RAY_FLAG_NONE, tMin 0, tMax kMaxRayTravel -> closest-hit / miss shader (PathTracerMaterialSpecializations.hlsl:27, PathTracerSample.hlsl:276-281)
                    Ray ray = path.getScatterRay();
                    rowCounters.extendRays++;
                    ptref::HitInfo hit = ptref::trace_closest(sc, toP(ray.origin), toP(ray.dir), 0.0f, kMaxRayTravel, &rowCounters.nodeVisitsExt, &rowCounters.triTestsExt);
                    if (hit.prim == 0xFFFFFFFFu) PathTracer::HandleMiss(path, ray.origin, ray.dir, kMaxRayTravel, workingContext);
                    else {      // closest-hit shader: InstanceIndex() / GeometryIndex() / PrimitiveIndex() identify the triangle (BridgeDonut:612-631)
                        const ptref::Triangle& tr = sc.tris[hit.prim];
                        g_hitInstanceIndex = sc.subInstToInstGeom[tr.subInstance].x; g_hitGeometryIndex = tr.subInstance - sc.instFirstSubInstance[g_hitInstanceIndex]; g_hitPrimitiveIndex = tr.triIndex;
                        PathTracer::HandleHit(path, ray.origin, ray.dir, hit.t, float2(hit.u, hit.v), workingContext);
                    }
                }
                // CommitPixel writes OutputColor[pixelPos]; PathState carries the real pixel id, the row buffer is indexed by x only
                workingContext.OutputColor.w = 0;
                PathTracer::CommitPixel(path, workingContext);
                (void)pixelPos;
            }
#pragma omp critical
            { uint64_t* dst = (uint64_t*)&c->ctr; const uint64_t* src = (const uint64_t*)&rowCounters; for (size_t k = 0; k < sizeof(rowCounters) / 8; k++) dst[k] += src[k]; }
            for (uint32_t x = x0; x < x1; x++) {
                ptref::float4& acc = c->accum[(size_t)y * c->w + x];
                ptref::float4 col = ptref::make_float4(row[x].x, row[x].y, row[x].z, row[x].w);
                acc = (blend < 1.f) ? ptref::lerp4(acc, col, blend) : col;
            }
        }
        c->accumCount++;
        if (c->neeat.enabled && c->fbSamples && c->neeat.fbW.size() == (size_t)c->w * c->h) { const size_t plane = (size_t)c->w * c->h;
            memcpy(c->fbWeight.data() + plane * s, c->neeat.fbW.data(), 4 * plane); memcpy(c->fbCand.data() + plane * s, c->neeat.fbC.data(), 4 * plane); }
    }
}
// the constants of the stable-plane passes (Sample.cpp:1509-1540) and the views of the frame, over what FrameBindings::bind set
static void bind_stable_plane_constants(::Context* c, const ptref::StablePlanesParams* prm) {
    const ptref::StablePlanesConsts K = ptref::SP_make_consts(*prm, c->w, c->h, c->S.bounceCount);
    PathTracerConstants& k = g_Const.ptConsts;
    k._activeStablePlaneCount = K.activeStablePlaneCount; k.maxStablePlaneVertexDepth = K.maxStablePlaneVertexDepth; k.allowPrimarySurfaceReplacement = K.allowPrimarySurfaceReplacement;
    k.genericTSLineStride = K.genericTSLineStride; k.genericTSPlaneStride = K.genericTSPlaneStride; k.invSubSampleCount = K.invSubSampleCount;
    auto mat = [](float4x4& M, const float* m) { for (int r = 0; r < 4; r++) M.r[r] = float4(m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]); };
    mat(g_Const.view.matWorldToClip, K.matWorldToClip); mat(g_Const.view.matWorldToClipNoOffset, K.matWorldToClipNoOffset); mat(g_Const.previousView.matWorldToClipNoOffset, K.prevMatWorldToClipNoOffset);
    g_Const.view.clipToWindowScale = float2(K.clipToWindowScale[0], K.clipToWindowScale[1]); g_Const.previousView.clipToWindowScale = g_Const.view.clipToWindowScale;
}
#if PATH_TRACER_MODE == PATH_TRACER_MODE_FILL_STABLE_PLANES
// One sub-sample of the realtime mode's noisy pass as the reference's own text runs it (RAYGEN_ENTRY with PATH_TRACER_MODE_FILL_STABLE_PLANES: FirstHitFromVBuffer, nextHit with its ray interval,
// CommitPixel -> CommitDenoiserRadiance), over the header / planes a build pass left; the planes' noisy radiance and the specular hit distance are updated in place.
static void fill_stable_planes(::Context* c, uint32_t sampleIndex, const ptref::StablePlanesParams* prm, uint32_t* header, void* planes, float* specHitT) {
    ::prepare(c);
    const ptref::Scene& sc = c->sc;
    FrameBindings frame; frame.bind(c, sampleIndex);
    bind_stable_plane_constants(c, prm);
    u_SpecularHitT.p = specHitT; u_SpecularHitT.w = c->w; u_SpecularHitT.h = c->h;
    // realtime mode with the baker in the loop (refpt_neeat_update_begin / _end around the build pass): the visible light samples of this pass fill the run's reservoirs
    u_LightFeedbackTotalWeight.p = c->neeat.enabled ? c->neeat.fbW.data() : nullptr; u_LightFeedbackTotalWeight.w = c->w; u_LightFeedbackTotalWeight.h = 0;
    u_LightFeedbackCandidates.p = c->neeat.enabled ? c->neeat.fbC.data() : nullptr; u_LightFeedbackCandidates.w = c->w; u_LightFeedbackCandidates.h = 0;
    RWTexture2DArray<uint> hdr; hdr.p = header; hdr.w = c->w; hdr.h = c->h;
    RWStructuredBuffer<StablePlane> planeBuf; planeBuf.p = (StablePlane*)planes;
    RWTexture2D<float4> srTex;      // the stable radiance is not touched by this pass
    const PathTracerConstants consts = g_Const.ptConsts;
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < (int)c->h; y++) {
        ptref::RayCounters rowCounters; memset(&rowCounters, 0, sizeof(rowCounters));
        ptref::PathTracer rowSvc(sc, c->S, c->cam, sampleIndex, &rowCounters);
        PtDriver rowDriver; rowDriver.svc = &rowSvc; g_drv = &rowDriver;
        PathTracer::WorkingContext workingContext;
        workingContext.PtConsts = consts; workingContext.StablePlanes = StablePlanesContext::make(hdr, planeBuf, srTex, consts);
        for (uint32_t x = 0; x < c->w; x++) {
            PathState path = PathTracer::EmptyPathInitialize(uint2(x, (uint)y), consts.camera.PixelConeSpreadAngle);
            PathTracer::SetupPathPrimaryRay(path, Bridge::computeCameraRay(uint2(x, (uint)y)));
            PathTracer::StartPixel(path, workingContext);
            float2 tMinMax = FirstHitFromVBuffer(path, 0, workingContext);
            while (path.isActive()) {
                Ray ray = path.getScatterRay();
                rowCounters.extendRays++;
                ptref::HitInfo hit = ptref::trace_closest(sc, toP(ray.origin), toP(ray.dir), tMinMax.x, tMinMax.y, &rowCounters.nodeVisitsExt, &rowCounters.triTestsExt);
                if (hit.prim == 0xFFFFFFFFu) PathTracer::HandleMiss(path, ray.origin, ray.dir, kMaxRayTravel, workingContext);
                else {
                    const ptref::Triangle& tr = sc.tris[hit.prim]; rowCounters.hits++;
                    g_hitInstanceIndex = sc.subInstToInstGeom[tr.subInstance].x; g_hitGeometryIndex = tr.subInstance - sc.instFirstSubInstance[g_hitInstanceIndex]; g_hitPrimitiveIndex = tr.triIndex;
                    PathTracer::HandleHit(path, ray.origin, ray.dir, hit.t, float2(hit.u, hit.v), workingContext);
                }
                tMinMax = float2(0, kMaxRayTravel);
            }
            PathTracer::CommitPixel(path, workingContext);
        }
#pragma omp critical
        { uint64_t* dst = (uint64_t*)&c->ctr; const uint64_t* src = (const uint64_t*)&rowCounters; for (size_t q = 0; q < sizeof(rowCounters) / 8; q++) dst[q] += src[q]; }
    }
    u_SpecularHitT.p = nullptr;
}
#endif
#if PATH_TRACER_MODE == PATH_TRACER_MODE_BUILD_STABLE_PLANES
// The realtime mode's pre-pass as the reference's own text runs it (RAYGEN_ENTRY with PATH_TRACER_MODE_BUILD_STABLE_PLANES, PathTracerSample.hlsl:200-250; nextHit / postProcessHit :96-169):
// same arguments and output arrays as ptref_build_stable_planes. The RGBA16F render targets (stable radiance, motion vectors) are float4 images here that are rounded to binary16 after every
// shader invocation that can write them — each writes a pixel at most once, so this is what a store through the UAV does.
static void round_half4(float4& t) { t = float4(ptref::f16tof32(ptref::f32tof16(t.x)), ptref::f16tof32(ptref::f32tof16(t.y)), ptref::f16tof32(ptref::f32tof16(t.z)), ptref::f16tof32(ptref::f32tof16(t.w))); }
static void build_stable_planes(::Context* c, uint32_t sampleIndex, const ptref::StablePlanesParams* prm, uint32_t* header, void* planes, uint32_t* stableRadiance, float* depth, float* specHitT, uint32_t* motionVectors, uint32_t* throughput) {
    ::prepare(c);
    const ptref::Scene& sc = c->sc;
    FrameBindings frame; frame.bind(c, sampleIndex);
    bind_stable_plane_constants(c, prm);
    const size_t N = (size_t)c->w * c->h;
    std::vector<float4> sr(N), mv(N);
    u_Depth.p = depth; u_Depth.w = c->w; u_Depth.h = c->h; u_SpecularHitT.p = specHitT; u_SpecularHitT.w = c->w; u_SpecularHitT.h = c->h;
    u_MotionVectors.p = mv.data(); u_MotionVectors.w = c->w; u_MotionVectors.h = c->h; u_Throughput.p = throughput; u_Throughput.w = c->w; u_Throughput.h = c->h;
    static_assert(sizeof(StablePlane) == 80, "StablePlane layout");
    RWTexture2DArray<uint> hdr; hdr.p = header; hdr.w = c->w; hdr.h = c->h;
    RWStructuredBuffer<StablePlane> planeBuf; planeBuf.p = (StablePlane*)planes;
    RWTexture2D<float4> srTex; srTex.p = sr.data(); srTex.w = c->w; srTex.h = c->h;
    const PathTracerConstants consts = g_Const.ptConsts;
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < (int)c->h; y++) {
        ptref::RayCounters rowCounters; memset(&rowCounters, 0, sizeof(rowCounters));
        ptref::PathTracer rowSvc(sc, c->S, c->cam, sampleIndex, &rowCounters);
        PtDriver rowDriver; rowDriver.svc = &rowSvc; g_drv = &rowDriver;
        PathTracer::WorkingContext workingContext;
        workingContext.PtConsts = consts; workingContext.StablePlanes = StablePlanesContext::make(hdr, planeBuf, srTex, consts);
        for (uint32_t x = 0; x < c->w; x++) {
            float4& srPixel = sr[(size_t)y * c->w + x];
            PathState path = PathTracer::EmptyPathInitialize(uint2(x, (uint)y), consts.camera.PixelConeSpreadAngle);
            PathTracer::SetupPathPrimaryRay(path, Bridge::computeCameraRay(uint2(x, (uint)y)));
            PathTracer::StartPixel(path, workingContext); round_half4(srPixel);
            while (path.isActive()) {
                Ray ray = path.getScatterRay();
                rowCounters.extendRays++;
                ptref::HitInfo hit = ptref::trace_closest(sc, toP(ray.origin), toP(ray.dir), 0.0f, kMaxRayTravel, &rowCounters.nodeVisitsExt, &rowCounters.triTestsExt);
                if (hit.prim == 0xFFFFFFFFu) PathTracer::HandleMiss(path, ray.origin, ray.dir, kMaxRayTravel, workingContext);
                else {
                    const ptref::Triangle& tr = sc.tris[hit.prim]; rowCounters.hits++;
                    g_hitInstanceIndex = sc.subInstToInstGeom[tr.subInstance].x; g_hitGeometryIndex = tr.subInstance - sc.instFirstSubInstance[g_hitInstanceIndex]; g_hitPrimitiveIndex = tr.triIndex;
                    PathTracer::HandleHit(path, ray.origin, ray.dir, hit.t, float2(hit.u, hit.v), workingContext);
                }
                round_half4(srPixel);
                postProcessHit(path, workingContext);
            }
            PathTracer::CommitPixel(path, workingContext);
        }
#pragma omp critical
        { uint64_t* dst = (uint64_t*)&c->ctr; const uint64_t* src = (const uint64_t*)&rowCounters; for (size_t q = 0; q < sizeof(rowCounters) / 8; q++) dst[q] += src[q]; }
    }
    auto pack = [](uint32_t* dst, const float4& v) { dst[0] = (ptref::f32tof16(v.y) << 16) | ptref::f32tof16(v.x); dst[1] = (ptref::f32tof16(v.w) << 16) | ptref::f32tof16(v.z); };
    for (size_t i = 0; i < N; i++) { pack(stableRadiance + 2 * i, sr[i]); pack(motionVectors + 2 * i, mv[i]); }
    u_Depth.p = nullptr; u_SpecularHitT.p = nullptr; u_MotionVectors.p = nullptr; u_Throughput.p = nullptr;
}
#endif
// Surface probe: Bridge::loadSurface of the reference text next to the oracle's loadSurface for the same hits (45 words per surface, floats as bits).
static void put3(uint32_t*& o, float3 v) { *o++ = asuint(v.x); *o++ = asuint(v.y); *o++ = asuint(v.z); }
static void surface_probe(::Context* c, uint32_t n, const uint32_t* prims, const float* uvDirCone, uint32_t* outRef, uint32_t* outOracle) {
    ::prepare(c);
    const ptref::Scene& sc = c->sc;
    FrameBindings frame; frame.bind(c, 0);
    ptref::PathTracer svc(sc, c->S, c->cam, 0, nullptr);
    for (uint32_t k = 0; k < n; k++) {
        const float* a = uvDirCone + 7 * k; const ptref::Triangle& tr = sc.tris[prims[k]];
        RayCone rc = RayCone::make(a[5], a[6]); ptref::RayCone prc; prc.widthSpreadAngleFP16 = rc.widthSpreadAngleFP16;
        uint inst = sc.subInstToInstGeom[tr.subInstance].x;
        PathTracer::SurfaceData r = Bridge::loadSurface(inst, tr.subInstance - sc.instFirstSubInstance[inst], tr.triIndex, float2(a[0], a[1]), float3(a[2], a[3], a[4]), rc, 2, uint2(0, 0), DebugContext());
        ptref::SurfaceData q = svc.loadSurface(prims[k], a[0], a[1], ptref::make_float3(a[2], a[3], a[4]), prc);
        uint32_t* o = outRef + 45 * k;
        put3(o, r.shadingData.posW); put3(o, r.shadingData.faceNCorrected); put3(o, r.shadingData.V); put3(o, r.shadingData.N); put3(o, r.shadingData.T); put3(o, r.shadingData.B); put3(o, r.shadingData.vertexN);
        *o++ = r.shadingData.frontFacing; *o++ = r.shadingData.mtl.packedData; *o++ = r.shadingData.materialID; *o++ = asuint((float)r.shadingData.IoR); *o++ = asuint((float)r.shadingData.shadowNoLFadeout); put3(o, float3(r.shadingData.emission));
        put3(o, float3(r.bsdf.data.Diffuse())); *o++ = asuint((float)r.bsdf.data.Roughness()); put3(o, float3(r.bsdf.data.Specular())); *o++ = asuint((float)r.bsdf.data.Metallic()); put3(o, float3(r.bsdf.data.Transmission()));
        *o++ = asuint((float)r.bsdf.data.DiffuseTransmission()); *o++ = asuint((float)r.bsdf.data.SpecularTransmission()); *o++ = asuint((float)r.bsdf.data.Eta()); *o++ = asuint((float)r.interiorIoR); *o++ = r.neeTriangleLightIndex;
        o = outOracle + 45 * k; const ptref::ShadingData& s = q.shadingData; const ptref::StandardBSDFData& b = q.bsdf.data;
        put3(o, toH(s.posW)); put3(o, toH(s.faceNCorrected)); put3(o, toH(s.V)); put3(o, toH(s.N)); put3(o, toH(s.T)); put3(o, toH(s.B)); put3(o, toH(s.vertexN));
        *o++ = s.frontFacing; *o++ = s.mtl.packedData; *o++ = s.materialID; *o++ = asuint(s.IoR); *o++ = asuint(s.shadowNoLFadeout); put3(o, toH(s.emission));
        put3(o, toH(b.diffuse)); *o++ = asuint(b.roughness); put3(o, toH(b.specular)); *o++ = asuint(b.metallic); put3(o, toH(b.transmission));
        *o++ = asuint(b.diffuseTransmission); *o++ = asuint(b.specularTransmission); *o++ = asuint(b.eta); *o++ = asuint(q.interiorIoR); *o++ = q.neeTriangleLightIndex;
    }
}
// Alpha probe: the reference's candidate tests for non-opaque triangles (AlphaTestImpl, Bridge::AlphaTest / AlphaTestVisibilityRay, BridgeDonut:929-989)
// next to what the oracle's traversal applies to the same candidates. out: [ref accept (closest), ref accept (visibility), oracle closest, oracle visibility]
static void alpha_probe(::Context* c, uint32_t n, const uint32_t* prims, const float* uv, uint32_t* out) {
    ::prepare(c);
    const ptref::Scene& sc = c->sc;
    FrameBindings frame; frame.bind(c, 0);
    for (uint32_t k = 0; k < n; k++) {
        const ptref::Triangle& tr = sc.tris[prims[k]];
        uint inst = sc.subInstToInstGeom[tr.subInstance].x, instanceID = sc.instFirstSubInstance[inst], geom = tr.subInstance - instanceID;      // InstanceID() = instanceContributionToHitGroupIndex (Sample.cpp:1200-1240)
        float2 b(uv[2 * k], uv[2 * k + 1]);
        out[4 * k + 0] = Bridge::AlphaTest(instanceID, inst, geom, tr.triIndex, b); out[4 * k + 1] = Bridge::AlphaTestVisibilityRay(instanceID, inst, geom, tr.triIndex, b);
        bool opaque = (tr.flags & 1u) == 0;
        out[4 * k + 2] = opaque || ptref::AlphaTest(sc, tr, b.x, b.y);
        out[4 * k + 3] = opaque || (!(tr.flags & 2u) && ptref::AlphaTest(sc, tr, b.x, b.y));
    }
}

// ---- EnvMapBaker.hlsl: the reference's BaseLayerCS and MIPReduceCS text, dispatched over the context's environment source, directional lights and cube
// resolution (EnvMapBaker::Update, EnvMapBaker.cpp:425-620: ScaleColor = EnvMapRadianceScale, BackgroundSourceType 1 = equirectangular image, 2 = cube-map image).
// out: 2 words per texel, laid out like the oracle's EnvCube (mips one after the other, face-major within a mip). Returns the texel count.
// the QUALITY 1 tail of BC6UCompress.hlsl's CSMain (:790-808): the best-scoring two-region partition, encoded over the one-region block where its estimate is lower
static void bc6u_encode_p2(uint4& block, float& blockMSLE, float3 texels[16]) {
    float bestScore = bc6u::EvaluateP2Pattern(0, texels); uint bestPattern = 0;
    for (uint patternIndex = 1; patternIndex < 32; ++patternIndex) { float score = bc6u::EvaluateP2Pattern(patternIndex, texels); if (score < bestScore) { bestPattern = patternIndex; bestScore = score; } }
    bc6u::EncodeP2Pattern(block, blockMSLE, bestPattern, texels);
}
static uint32_t env_bake(const ::Context* c, uint32_t* out, uint32_t capacity) {
    const ptref::EnvMap& e = c->sc.env;
    const uint dim = e.cubeDim, levels = ptref::env_cube_mip_levels(dim);
    size_t total = 0; std::vector<size_t> off(levels);
    for (uint l = 0; l < levels; l++) { off[l] = total; total += 6ull * (dim >> l) * (dim >> l); }
    if (!out || capacity < total) return (uint32_t)total;
    ptref::uint2* T = (ptref::uint2*)out;
    memset(&embake::g_Const, 0, sizeof(embake::g_Const));
    embake::g_Const.ScaleColor = float3(ptref::kEnvMapRadianceScale); embake::g_Const.CubeDim = dim; embake::g_Const.CubeDimLowRes = dim / 2; embake::g_Const.BackgroundSourceType = e.imageCubeDim ? 2 : (e.tex.w ? 1 : 0); embake::g_Const.ProcSkyEnabled = e.skyEnabled ? 1 : 0;
    embake::g_Const.DirectionalLightCount = (uint)e.dirLights.size();
    for (size_t i = 0; i < e.dirLights.size(); i++) {
        const ptref::EnvDirectionalLight& d = e.dirLights[i];
        embake::g_Const.DirectionalLights[i].ColorIntensity = float4(d.ColorIntensity.x, d.ColorIntensity.y, d.ColorIntensity.z, d.ColorIntensity.w);
        embake::g_Const.DirectionalLights[i].Direction = toH(d.Direction); embake::g_Const.DirectionalLights[i].AngularSize = d.AngularSize;
    }
    embake::t_SrcEquirectangularEnvMap.tex = &e.tex;
    static ptref::EnvCube imageCube; imageCube = e.imageCubeView();      // EnvMapBaker.cpp:483-486: the loaded cube map bound as t_SrcCubemapEnvMap
    embake::t_SrcCubemapEnvMap.ctx = &imageCube;
    embake::t_SrcCubemapEnvMap.fetch = [](const void* ctx, float3 dir, float lod) { ptref::float4 c = ptref::env_cube_sample_level(*(const ptref::EnvCube*)ctx, ptref::make_float3(dir.x, dir.y, dir.z), lod); return float4(c.x, c.y, c.z, c.w); };
    std::vector<ptref::uint2> lowRes; ptref::EnvCube lowCube;
    if (e.skyEnabled) {          // EnvMapBaker.cpp:454-470, 516-533: the constants, the four look-up textures, the half-resolution pre-pass into m_cubemapLowRes (RGBA16F), which the base layer then samples
        static_assert(sizeof(ProceduralSkyConstants) == sizeof(ptref::ProceduralSkyConstants), "ProceduralSkyConstants layout");
        memcpy(&embake::g_Const.ProcSkyConsts, &e.sky.Consts, sizeof(ProceduralSkyConstants));
        static ptref::SkyTexture lut[4]; lut[0] = e.sky.Transmittance; lut[1] = e.sky.Scatter; lut[2] = e.sky.Irradiance; lut[3] = e.sky.Clouds;
        for (int i = 0; i < 4; i++) lut[i].texels = e.skyTex[i].data();
        embake::t_ProcSkyTransmittance.lut = &lut[0]; embake::t_ProcSkyScatter.lut = &lut[1]; embake::t_ProcSkyIrradiance.lut = &lut[2]; embake::t_ProcSkyClouds.lut = &lut[3];
        const uint h = dim / 2; lowRes.assign(6ull * h * h, ptref::make_uint2(0, 0));
        embake::u_EnvMapCubeFacesDst0.texels = lowRes.data(); embake::u_EnvMapCubeFacesDst0.dim = h;
        for (uint f = 0; f < 6; f++) for (uint y = 0; y < h; y++) for (uint x = 0; x < h; x++) embake::LowResPrePassLayerCS(uint3(x, y, f));
        memset(&lowCube, 0, sizeof(lowCube)); lowCube.texels = lowRes.data(); lowCube.dim = h; lowCube.mipLevels = 1;
        embake::t_LowResPrePassCube.ctx = &lowCube;
        embake::t_LowResPrePassCube.fetch = [](const void* ctx, float3 dir, float lod) { ptref::float4 c = ptref::env_cube_sample_level(*(const ptref::EnvCube*)ctx, ptref::make_float3(dir.x, dir.y, dir.z), lod); return float4(c.x, c.y, c.z, c.w); };
    }
    embake::u_EnvMapCubeFacesDst0.texels = T + off[0]; embake::u_EnvMapCubeFacesDst0.dim = dim;
    embake::u_EnvMapCubeFacesDst1.texels = T + off[1]; embake::u_EnvMapCubeFacesDst1.dim = dim / 2;
    for (uint f = 0; f < 6; f++) for (uint y = 0; y < dim / 2; y++) for (uint x = 0; x < dim / 2; x++) embake::BaseLayerCS(uint3(x, y, f));      // one thread per mip-1 texel (EnvMapBaker.cpp:560-575)
    for (uint l = 2; l < levels; l++) {
        const uint d = dim >> l;
        embake::u_EnvMapCubeFacesSrc.texels = T + off[l - 1]; embake::u_EnvMapCubeFacesSrc.dim = d * 2; embake::u_EnvMapCubeFacesDst.texels = T + off[l]; embake::u_EnvMapCubeFacesDst.dim = d;
        for (uint f = 0; f < 6; f++) for (uint y = 0; y < d; y++) for (uint x = 0; x < d; x++) embake::MIPReduceCS(uint3(x, y, f));
    }
    if (e.cubeCompression) {          // BC6UCompress.hlsl (QUALITY 0) over every level, texel order of CSMain's gathers; what the texture unit then returns is the BC6H_UF16 decode (ptref::bc6_decode_mode11)
        for (uint l = 0; l < levels; l++) {
            const uint d = dim >> l; ptref::uint2* L = T + off[l];
            for (uint f = 0; f < 6; f++) for (uint by = 0; by < d / 4; by++) for (uint bx = 0; bx < d / 4; bx++) {
                float3 t[16];
                for (uint i = 0; i < 16; i++) { ptref::float4 v = ptref::env_unpack_rgba16f(L[((size_t)f * d + (by * 4 + i / 4)) * d + (bx * 4 + i % 4)]); t[i] = float3(v.x, v.y, v.z); }
                uint4 b = uint4(0, 0, 0, 0); float msle = 0.f; bc6u::EncodeP1(b, msle, t);
                if (e.cubeCompression >= 2) bc6u_encode_p2(b, msle, t);          // QUALITY 1 (CSMain, BC6UCompress.hlsl:790-808)
                const ptref::uint blk[4] = {b.x, b.y, b.z, b.w}; ptref::uint hb[16][3]; ptref::bc6_decode(blk, hb);
                for (uint i = 0; i < 16; i++) L[((size_t)f * d + (by * 4 + i / 4)) * d + (bx * 4 + i % 4)] = ptref::make_uint2(hb[i][0] | (hb[i][1] << 16), hb[i][2] | (0x3C00u << 16));
            }
        }
    }
    return (uint32_t)total;
}
// ---- EnvMapImportanceSamplingBaker.hlsl: BuildMIPDescentImportanceMapCS of the reference text over the context's baked cube (constants as
// EnvMapImportanceSamplingBaker::FillBakerConsts, .cpp:178-194: 1024^2 texels, 4 x 4 samples each). out: dim x dim float4 (rgb mean radiance, w importance).
static void env_importance(::Context* c, uint32_t dim, float* out) {
    ptref::EnvMap& e = c->sc.env;
    if (e.cubeDirty) { bake_env_cube(e); c->lightsDirty = true; }
    const uint samples = 16, sx = 4, sy = samples / sx;
    emisb::g_BuilderConsts.SourceCubeDim = e.cube.dim; emisb::g_BuilderConsts.SourceCubeMIPCount = e.cube.mipLevels; emisb::g_BuilderConsts.SampleIndex = 0;
    emisb::g_BuilderConsts.ImportanceMapDim = uint2(dim, dim); emisb::g_BuilderConsts.ImportanceMapDimInSamples = uint2(dim * sx, dim * sy);
    emisb::g_BuilderConsts.ImportanceMapNumSamples = uint2(sx, sy); emisb::g_BuilderConsts.ImportanceMapInvSamples = 1.f / (float)(sx * sy); emisb::g_BuilderConsts.ImportanceMapBaseMip = 0;
    std::vector<float> imp((size_t)dim * dim);
    emisb::t_EnvMapCube.cube = &e.cubeSource;      // (EnvMapBaker.cpp:635: the importance baker is handed the uncompressed cube)
    emisb::u_ImportanceMap.p = imp.data(); emisb::u_ImportanceMap.w = dim; emisb::u_RadianceMap.p = (ptref::float4*)out; emisb::u_RadianceMap.w = dim;
#pragma omp parallel for schedule(dynamic, 8)
    for (int y = 0; y < (int)dim; y++) for (uint x = 0; x < dim; x++) emisb::BuildMIPDescentImportanceMapCS(uint3(x, (uint)y, 0));
}
} // namespace hl
extern "C" {
// BC6UCompress.hlsl EncodeP1 on n blocks of 16 RGB texels (48 floats each) -> 4 words each
void refpt_bc6_encode_quality(const float* texels, uint32_t n, uint32_t* out) {
    for (uint32_t k = 0; k < n; k++) { hl::float3 t[16]; for (int i = 0; i < 16; i++) t[i] = hl::float3(texels[48 * k + 3 * i], texels[48 * k + 3 * i + 1], texels[48 * k + 3 * i + 2]);
        hl::uint4 b = hl::uint4(0, 0, 0, 0); float msle = 0.f; hl::bc6u::EncodeP1(b, msle, t); hl::bc6u_encode_p2(b, msle, t); out[4 * k] = b.x; out[4 * k + 1] = b.y; out[4 * k + 2] = b.z; out[4 * k + 3] = b.w; }
}
void refpt_bc6_encode(const float* texels, uint32_t n, uint32_t* out) {
    for (uint32_t k = 0; k < n; k++) { hl::float3 t[16]; for (int i = 0; i < 16; i++) t[i] = hl::float3(texels[48 * k + 3 * i], texels[48 * k + 3 * i + 1], texels[48 * k + 3 * i + 2]);
        hl::uint4 b = hl::uint4(0, 0, 0, 0); float msle = 0.f; hl::bc6u::EncodeP1(b, msle, t); out[4 * k] = b.x; out[4 * k + 1] = b.y; out[4 * k + 2] = b.z; out[4 * k + 3] = b.w; }
}
// LightsBaker.hlsl ImportanceBooster (with DistanceFromFrustum) on n lights: 12 words each (PolymorphicLightInfo + Ex), planes = 5 x 4 floats, hist: last frame's weights or null
void refpt_importance_boost(uint32_t n, const uint32_t* lights12, const float* planes20, float mul, float fade, float intensityDeltaMul, const float* hist, const float* unboosted, float* out) {
    memset(&hl::lbfb::g_ctrl, 0, sizeof(hl::lbfb::g_ctrl)); memset(&hl::lbfb::g_bakerConstants, 0, sizeof(hl::lbfb::g_bakerConstants));
    for (int i = 0; i < 5; i++) hl::lbfb::g_bakerConstants.FrustumPlanes[i] = hl::float4(planes20[4 * i], planes20[4 * i + 1], planes20[4 * i + 2], planes20[4 * i + 3]);
    hl::lbfb::g_bakerConstants.ImportanceBoostFrustumMul = mul; hl::lbfb::g_bakerConstants.ImportanceBoostFrustumFadeDistance = fade; hl::lbfb::g_bakerConstants.ImportanceBoostIntensityDelta = hist ? intensityDeltaMul : 0.0f;
    hl::lbfb::g_ctrl.LastFrameTemporalFeedbackAvailable = hist ? 1 : 0; hl::lbfb::g_bakerConstants.HistoricWeightsBufferOffset = 0;
    std::vector<hl::uint> identity(n); for (uint32_t i = 0; i < n; i++) identity[i] = i;
    hl::lbfb::u_historyRemapCurrentToPast.p = identity.data(); hl::lbfb::u_lightWeights.p = (float*)hist;
    for (uint32_t i = 0; i < n; i++) {
        hl::PolymorphicLightInfoFull lf; memcpy(&lf.Base, lights12 + 12 * i, 32); memcpy(&lf.Extended, lights12 + 12 * i + 8, 16);
        out[i] = hl::lbfb::ImportanceBooster(lf, i, unboosted[i]);
    }
}
// LightsBaker.hlsl ComputeProxyCounts on n lights, dispatched as the reference does (groups of 128 threads, the barrier honoured): weights + their sum in, the per-light
// proxy counts and SamplingProxyCount out. usage: n + 1 counts of last frame's feedback (P0) or null.
uint32_t refpt_proxy_counts(uint32_t n, const float* weights, float weightSum, const uint32_t* usage, uint32_t totalMaxFeedbackCount, float globalFeedbackUseWeight, uint32_t importanceSamplingType, uint32_t* counts) {
    memset(&hl::lbfb::g_ctrl, 0, sizeof(hl::lbfb::g_ctrl)); memset(&hl::lbfb::g_bakerConstants, 0, sizeof(hl::lbfb::g_bakerConstants));
    hl::LightingControlData& c = hl::lbfb::g_ctrl;
    c.TotalLightCount = n; c.ImportanceSamplingType = importanceSamplingType; memcpy(&c.WeightsSumUINT, &weightSum, 4);
    c.LastFrameTemporalFeedbackAvailable = usage ? 1 : 0; c.TotalMaxFeedbackCount = totalMaxFeedbackCount; c.GlobalFeedbackUseWeight = globalFeedbackUseWeight;
    std::vector<hl::uint> counters(n + 1, 0u), scratch(n + 256, 0u), proxies(n / 128 + 8, 0u);
    if (usage) memcpy(counters.data(), usage, 4 * (size_t)(n + 1));
    hl::lbfb::u_lightWeights.p = (float*)weights; hl::lbfb::u_perLightProxyCounters.p = counters.data(); hl::lbfb::u_scratchList.p = scratch.data(); hl::lbfb::u_lightSamplingProxies.p = proxies.data();
    for (uint32_t g = 0; g < (n + 127) / 128; g++) hl::lbfb::run_group(128, [&](hl::uint t) { hl::lbfb::ComputeProxyCounts(g * 128 + t, t); });
    memcpy(counts, counters.data(), 4 * (size_t)n);
    return c.SamplingProxyCount;
}
void refpt_env_importance(void* h, uint32_t dim, float* out) { hl::env_importance((Context*)h, dim, out); }
uint32_t refpt_env_bake(void* h, uint32_t* out, uint32_t capacity) { return hl::env_bake((Context*)h, out, capacity); }
void refpt_alpha_probe(void* h, uint32_t n, const uint32_t* prims, const float* uv, uint32_t* out) { hl::alpha_probe((Context*)h, n, prims, uv, out); }
void refpt_surface_probe(void* h, uint32_t n, const uint32_t* prims, const float* uvDirCone, uint32_t* outRef, uint32_t* outOracle) { hl::surface_probe((Context*)h, n, prims, uvDirCone, outRef, outOracle); }
#if PATH_TRACER_MODE == PATH_TRACER_MODE_FILL_STABLE_PLANES
void refpt_fill_stable_planes(void* h, uint32_t sampleIndex, const ptref::StablePlanesParams* prm, uint32_t* header, void* planes, float* specHitT) { hl::fill_stable_planes((Context*)h, sampleIndex, prm, header, planes, specHitT); }
#endif
#if PATH_TRACER_MODE == PATH_TRACER_MODE_BUILD_STABLE_PLANES
void refpt_build_stable_planes(void* h, uint32_t sampleIndex, const ptref::StablePlanesParams* prm, uint32_t* header, void* planes, uint32_t* stableRadiance, float* depth, float* specHitT, uint32_t* motionVectors, uint32_t* throughput) {
    hl::build_stable_planes((Context*)h, sampleIndex, prm, header, planes, stableRadiance, depth, specHitT, motionVectors, throughput); }
#endif
// PostProcess.hlsl NO_DENOISER_FINAL_MERGE: u_OutputColor[pixelPos] = float4(stablePlanes.GetAllRadiance(pixelPos), 1) with the reference's StablePlanesContext (StablePlanes.hlsli)
namespace hl { static void stable_planes_merge(uint32_t w, uint32_t hgt, const uint32_t* header, const void* planes, const uint32_t* stableRadiance, float* rgba) {
    std::vector<float4> sr((size_t)w * hgt);
    for (size_t i = 0; i < sr.size(); i++) sr[i] = float4(ptref::f16tof32(stableRadiance[2 * i] & 0xffffu), ptref::f16tof32(stableRadiance[2 * i] >> 16), ptref::f16tof32(stableRadiance[2 * i + 1] & 0xffffu), ptref::f16tof32(stableRadiance[2 * i + 1] >> 16));
    RWTexture2DArray<uint> hdr; hdr.p = (uint*)header; hdr.w = w; hdr.h = hgt;
    RWStructuredBuffer<StablePlane> planeBuf; planeBuf.p = (StablePlane*)planes;
    RWTexture2D<float4> srTex; srTex.p = sr.data(); srTex.w = w; srTex.h = hgt;
    PathTracerConstants consts; memset(&consts, 0, sizeof(consts)); consts.imageWidth = w; consts.imageHeight = hgt;
    consts.genericTSLineStride = GenericTSComputeLineStride(w, hgt); consts.genericTSPlaneStride = GenericTSComputePlaneStride(w, hgt);
    StablePlanesContext stablePlanes = StablePlanesContext::make(hdr, planeBuf, srTex, consts);
    for (uint32_t y = 0; y < hgt; y++) for (uint32_t x = 0; x < w; x++) { const float3 c = stablePlanes.GetAllRadiance(uint2(x, y)); float* o = rgba + 4 * ((size_t)y * w + x); o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = 1.0f; }
} }
void refpt_stable_planes_merge(uint32_t w, uint32_t hgt, const uint32_t* header, const void* planes, const uint32_t* stableRadiance, float* rgba) { hl::stable_planes_merge(w, hgt, header, planes, stableRadiance, rgba); }
} // extern "C" (the helpers below are templates)
// ---- PostProcess.hlsl: the denoiser passes as the reference's own text (hl::pp, over hlsl_postprocess_stubs.h). One frame's inputs and constants travel in a PpFrame; the
// outputs and the state that one pass leaves for the next are the caller's arrays, so a sequence of calls runs over what the previous call left, as Sample::Denoise's
// dispatches do (Sample.cpp:2561-2619, 2712-2719). Every `main` runs over every thread of whole 8 x 8 groups; the shader rejects the threads beyond the frame.
struct PpFrame {
    uint32_t width, height, sampleBaseIndex; float perPixelJitterAAScale;
    const ptref::StablePlanesParams* prm; const float* dn;          // dn: matWorldToView[16], preExposedGrayLuminance, denoiserRadianceClampK, DLSSRRBrightnessClampK, stablePlanesSuppressPrimaryIndirectSpecularK
    const float* hitParams; const ptref::PathTracerCameraData* cam;  // hitParams: g_Const.denoisingHitParamConsts (REBLUR's hit-distance parameters; the recorder ignores them)
    const uint32_t* header; const void* planes; const uint32_t* stableRadiance; const float* specHitT; const uint32_t* motionVectors;
};
struct PpNrdState { float* viewZ; uint16_t* motionVectors; float* normalRoughness; float* diffRadianceHitDist; float* specRadianceHitDist; float* roughness; unsigned char* disocclusionThresholdMix; unsigned char* combinedHistoryClampRelax;
                    float* normHitDistCalls; };      // normHitDistCalls: [h][w][2][2] the (hitDist, roughness) arguments of REBLUR_FrontEnd_GetNormHitDist's two calls, or null
namespace hl {
struct PpBound { std::vector<float4> stableRadiance, motionVectors; };
static void pp_bind(const PpFrame* f, uint32_t p0, uint32_t p1, PpBound& B) {
    using namespace pp;
    const uint32_t w = f->width, h = f->height; const size_t N = (size_t)w * h;
    memset(&g_Const, 0, sizeof(g_Const)); memset(&g_MiniConst, 0, sizeof(g_MiniConst));
    const ptref::StablePlanesConsts K = ptref::SP_make_consts(*f->prm, w, h, 0);
    PathTracerConstants& k = g_Const.ptConsts;
    static_assert(sizeof(PathTracerCameraData) == sizeof(ptref::PathTracerCameraData), "camera layout");
    memcpy(&k.camera, f->cam, sizeof(k.camera));
    k.imageWidth = w; k.imageHeight = h; k.sampleBaseIndex = f->sampleBaseIndex; k.perPixelJitterAAScale = f->perPixelJitterAAScale;
    k._activeStablePlaneCount = K.activeStablePlaneCount; k.genericTSLineStride = K.genericTSLineStride; k.genericTSPlaneStride = K.genericTSPlaneStride;
    k.preExposedGrayLuminance = f->dn[16]; k.denoiserRadianceClampK = f->dn[17]; k.DLSSRRBrightnessClampK = f->dn[18]; k.stablePlanesSuppressPrimaryIndirectSpecularK = f->dn[19];
    auto mat = [](float4x4& M, const float* m) { for (int r = 0; r < 4; r++) M.r[r] = float4(m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]); };
    mat(g_Const.view.matWorldToClip, K.matWorldToClip); mat(g_Const.view.matWorldToClipNoOffset, K.matWorldToClipNoOffset); mat(g_Const.previousView.matWorldToClipNoOffset, K.prevMatWorldToClipNoOffset);
    mat(g_Const.view.matWorldToView, f->dn);
    g_Const.view.clipToWindowScale = float2(K.clipToWindowScale[0], K.clipToWindowScale[1]); g_Const.previousView.clipToWindowScale = g_Const.view.clipToWindowScale;
    if (f->hitParams) g_Const.denoisingHitParamConsts = float4(f->hitParams[0], f->hitParams[1], f->hitParams[2], f->hitParams[3]);
    g_MiniConst.params = uint4(p0, p1, 0, 0);          // Sample::Denoise: (plane, initWithStableRadiance, 0, 0); the DLSS-RR pass: zeros
    auto half4 = [](const uint32_t* q) { return float4(ptref::f16tof32(q[0] & 0xffffu), ptref::f16tof32(q[0] >> 16), ptref::f16tof32(q[1] & 0xffffu), ptref::f16tof32(q[1] >> 16)); };
    B.stableRadiance.resize(N); B.motionVectors.resize(N);
    for (size_t i = 0; i < N; i++) { B.stableRadiance[i] = half4(f->stableRadiance + 2 * i); B.motionVectors[i] = f->motionVectors ? half4(f->motionVectors + 2 * i) : float4(); }
    u_StablePlanesHeader.p = (uint*)f->header; u_StablePlanesHeader.w = w; u_StablePlanesHeader.h = h; u_StablePlanesBuffer.p = (StablePlane*)f->planes; t_StablePlanesBuffer.p = (const StablePlane*)f->planes;
    u_StableRadiance.p = B.stableRadiance.data(); u_StableRadiance.w = w; u_StableRadiance.h = h;
    hl::u_MotionVectors.p = B.motionVectors.data(); hl::u_MotionVectors.w = w; hl::u_MotionVectors.h = h; hl::u_SpecularHitT.p = (float*)f->specHitT; hl::u_SpecularHitT.w = w; hl::u_SpecularHitT.h = h;
}
static void pp_unbind() { hl::u_MotionVectors.p = nullptr; hl::u_SpecularHitT.p = nullptr; pp::g_nrdCalls = nullptr; }
template <class M> static void pp_dispatch(uint32_t w, uint32_t h, M entry) {
    for (uint32_t y = 0; y < (h + 7) / 8 * 8; y++) for (uint32_t x = 0; x < (w + 7) / 8 * 8; x++) { pp::g_nrdPixel = (size_t)(y < h ? y : 0) * w + (x < w ? x : 0); pp::g_nrdCallCount = 0; entry(uint3(x, y, 0)); }
}
template <class T, class P> static void pp_target(T& t, P* p, uint32_t w, uint32_t h) { t.p = p; t.w = w; t.h = h; }
}
extern "C" {
void refpt_denoiser_prepare_dlss_rr(const PpFrame* f, float* outputColor, uint32_t* rrDiffuseAlbedo, uint32_t* rrSpecAlbedo, uint16_t* rrNormalsAndRoughness, uint16_t* rrSpecMotionVectors) {
    using namespace hl::pp; hl::PpBound B; hl::pp_bind(f, 0, 0, B); const uint32_t w = f->width, h = f->height;
    hl::pp_target(u_OutputColor, (hl::float4*)outputColor, w, h); hl::pp_target(u_RRDiffuseAlbedo, rrDiffuseAlbedo, w, h); hl::pp_target(u_RRSpecAlbedo, rrSpecAlbedo, w, h);
    hl::pp_target(u_RRNormalsAndRoughness, (Half4*)rrNormalsAndRoughness, w, h); hl::pp_target(u_RRSpecMotionVectors, (Half2*)rrSpecMotionVectors, w, h);
    hl::pp_dispatch(w, h, [](hl::uint3 id) { rr::main(id); });
    hl::pp_unbind();
}
// init: g_MiniConst.params[1], and the host's per-frame clear of CombinedHistoryClampRelax (RenderTargets::Clear, RenderTargets.cpp:380) before the frame's first plane
void refpt_denoiser_prepare_nrd(const PpFrame* f, uint32_t plane, uint32_t init, uint32_t useRelax, float* outputColor, const PpNrdState* s) {
    using namespace hl::pp; hl::PpBound B; hl::pp_bind(f, plane, init ? 1u : 0u, B); const uint32_t w = f->width, h = f->height;
    if (init) memset(s->combinedHistoryClampRelax, 0, (size_t)w * h);
    hl::pp_target(u_OutputColor, (hl::float4*)outputColor, w, h); hl::pp_target(u_DenoiserViewspaceZ, s->viewZ, w, h); hl::pp_target(u_DenoiserMotionVectors, (Half4*)s->motionVectors, w, h);
    hl::pp_target(u_DenoiserNormalRoughness, (hl::float4*)s->normalRoughness, w, h); hl::pp_target(u_DenoiserDiffRadianceHitDist, (hl::float4*)s->diffRadianceHitDist, w, h);
    hl::pp_target(u_DenoiserSpecRadianceHitDist, (hl::float4*)s->specRadianceHitDist, w, h);
    hl::pp_target(u_DenoiserDisocclusionThresholdMix, s->disocclusionThresholdMix, w, h); hl::pp_target(u_CombinedHistoryClampRelax, s->combinedHistoryClampRelax, w, h);
    std::vector<float> calls((size_t)w * h * 4, 0.0f); std::vector<unsigned char> called((size_t)w * h, 0);
    g_nrdCalls = useRelax ? nullptr : calls.data();
    if (useRelax) hl::pp_dispatch(w, h, [](hl::uint3 id) { relax::prepare::main(id); });
    else hl::pp_dispatch(w, h, [&](hl::uint3 id) { reblur::prepare::main(id); if (id.x < w && id.y < h && g_nrdCallCount) called[g_nrdPixel] = 1; });
    // REBLUR hands the plane's raw roughness to NRD through its second GetNormHitDist call (RELAX has no such argument): the pixels that made the call record it
    if (!useRelax) for (size_t i = 0; i < (size_t)w * h; i++) if (called[i]) { s->roughness[i] = calls[4 * i + 3]; if (s->normHitDistCalls) memcpy(s->normHitDistCalls + 4 * i, &calls[4 * i], 16); }
    hl::pp_unbind();
}
void refpt_denoiser_merge_nrd(const PpFrame* f, uint32_t plane, uint32_t useRelax, const float* diff, const float* spec, const float* viewZ, const unsigned char* disocclusionThresholdMix, float* outputColor) {
    using namespace hl::pp; hl::PpBound B; hl::pp_bind(f, plane, 0, B); const uint32_t w = f->width, h = f->height;
    hl::pp_target(u_InputOutput, (hl::float4*)outputColor, w, h); hl::pp_target(t_DiffRadiance, (const hl::float4*)diff, w, h); hl::pp_target(t_SpecRadiance, (const hl::float4*)spec, w, h);
    hl::pp_target(t_DenoiserViewspaceZ, viewZ, w, h); hl::pp_target(t_DenoiserDisocclusionThresholdMix, (unsigned char*)disocclusionThresholdMix, w, h);
    if (useRelax) hl::pp_dispatch(w, h, [](hl::uint3 id) { relax::merge::main(id); }); else hl::pp_dispatch(w, h, [](hl::uint3 id) { reblur::merge::main(id); });
    hl::pp_unbind();
}
}
extern "C" {
// DenoisingGuidesBaker::DenoiseSpecHitT: the reference's compute shader, thread by thread, ping then pong (DenoisingGuidesBaker.cpp:62-84)
void refpt_denoise_spec_hit_t(uint32_t w, uint32_t hgt, const float* depth, float* specHitT) {
    using namespace hl::dgb;
    std::vector<float> scratch((size_t)w * hgt);
    u_Depth.p = (float*)depth; u_Depth.w = w; u_Depth.h = hgt; u_SpecularHitT.p = specHitT; u_SpecularHitT.w = w; u_SpecularHitT.h = hgt; u_ScratchFloat1.p = scratch.data(); u_ScratchFloat1.w = w; u_ScratchFloat1.h = hgt;
    memset(&g_denoisingConstants, 0, sizeof(g_denoisingConstants)); g_denoisingConstants.RenderResolution = hl::uint2(w, hgt); g_denoisingConstants.DisplayResolution = hl::uint2(w, hgt);
    for (uint ping = 1; ping != (uint)-1; ping--) {
        g_denoisingConstants.Ping = ping;
        for (uint32_t gy = 0; gy < (hgt + 7) / 8 * 8; gy++) for (uint32_t gx = 0; gx < (w + 7) / 8 * 8; gx++) DenoiseSpecHitT(hl::uint2(gx, gy));      // whole groups: the shader rejects the threads beyond the frame
    }
}
// realtime mode: the reference's baker passes around the build pass (ptref_neeat_update_begin / _end with the LightsBaker.hlsl text)
void refpt_neeat_update_begin(void* h) { Context* c = (Context*)h; ::prepare(c); hl::ReferenceNeeAtPasses passes; ::neeat_frame(c, passes, NEEAT_BEGIN); }
void refpt_neeat_update_end(void* h, const float* depth, const uint32_t* motionVectors) { Context* c = (Context*)h; ::prepare(c); hl::ReferenceNeeAtPasses passes; ::neeat_frame(c, passes, NEEAT_END, depth, motionVectors); }
void refpt_render_rect(void* h, uint32_t first, uint32_t n, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) { hl::render_rect((Context*)h, first, n, x0, y0, x1, y1); }
void refpt_render(void* h, uint32_t first, uint32_t n) { Context* c = (Context*)h; hl::render_rect(c, first, n, 0, 0, c->w, c->h); }
}

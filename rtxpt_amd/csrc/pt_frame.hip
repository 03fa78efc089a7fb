// mi355pt — the frame drivers: pt_render (reference mode) and the realtime mode's build and fill passes (pt_build_stable_planes,
// pt_fill_stable_planes). Host code only: each composes a frame out of the launches pt_wavefront.h, pt_trace.h and pt_stableplanes_launch.h declare.
// What the three share — the slicing of the owned pixels into batches, the frame's events, the harvest of the counters, the checks at the
// end of a frame — exists once, at the top of the file.
#include "pt_context.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

StablePlanesContext sp_context(pt_context* c, const PtStablePlanesParams* params) {
    ptk::StablePlanesParams prm;
    if (params) memcpy(&prm, params, sizeof(prm));
    else { memset(&prm, 0, sizeof(prm)); prm.activeStablePlaneCount = cStablePlaneCount; }
    StablePlanesContext sp; sp.C = ptk::SP_make_consts(prm, c->width, c->height, c->S.bounceCount);
    sp.B.Header = c->dSpHeader.p; sp.B.Planes = c->dSpPlanes.p; sp.B.StableRadiance = c->dSpRadiance.p; sp.B.Depth = c->dSpDepth.p;
    sp.B.SpecularHitT = c->dSpHitT.p; sp.B.MotionVectors = c->dSpMotion.p; sp.B.Throughput = c->dSpThroughput.p;
    return sp;
}

void add_frame_stats(PtFrameStats& t, const PtFrameStats& o) {
    t.extendRays += o.extendRays; t.shadowRays += o.shadowRays; t.hits += o.hits;
    t.nodeVisitsExtend += o.nodeVisitsExtend; t.triTestsExtend += o.triTestsExtend; t.nodeVisitsShadow += o.nodeVisitsShadow;
    t.triTestsShadow += o.triTestsShadow; t.leafVisitsExtend += o.leafVisitsExtend; t.waveItersExtend += o.waveItersExtend;
    t.leafVisitsShadow += o.leafVisitsShadow; t.waveItersShadow += o.waveItersShadow;
    for (int q = 0; q < 4; q++) t.extendPhaseCycles[q] += o.extendPhaseCycles[q];
    t.leafBlocksExtend += o.leafBlocksExtend; if (o.waveItersMaxExtend > t.waveItersMaxExtend) t.waveItersMaxExtend = o.waveItersMaxExtend;
    for (int q = 0; q < 16; q++) t.extendRayIterHist[q] += o.extendRayIterHist[q];
    for (uint q = 0; q < o.longRayCount && q < 32u && t.longRayCount < 32u; q++) { memcpy(t.longRays[t.longRayCount], o.longRays[q], 32); t.longRayCount++; }
    for (int q = 0; q < 8; q++) t.extendEvents[q] += o.extendEvents[q];
    t.gpuMilliseconds += o.gpuMilliseconds; t.extendKernelMs += o.extendKernelMs; t.shadeKernelMs += o.shadeKernelMs; t.shadowKernelMs += o.shadowKernelMs;
    t.extendLaunches += o.extendLaunches; if (o.iterations > t.iterations) t.iterations = o.iterations;
    t.pathsTraced += o.pathsTraced; t.tailLaunches += o.tailLaunches;
}

namespace {

// ---------------------------------------------------------------- what the three drivers share

int ensure_pool(pt_context* c, uint n, uint shadowPerPath) {      // shadowPerPath: shadow-queue entries a path vertex may emit (NEEFullSamples)
    if (n <= c->poolCapacity && (size_t)n * shadowPerPath <= c->shadowCapacity) return PT_OK;
    if (n < c->poolCapacity) n = c->poolCapacity;
    const size_t ns = (size_t)n * shadowPerPath;
    if (ns > 0xF0000000ull) return fail(c, PT_ERROR_INVALID_ARGUMENT, "too many shadow-queue entries in one pt_render call (paths x NEEFullSamples)");
    PT_CHECK_HIP(c, c->dS0.resize(n)); PT_CHECK_HIP(c, c->dS1.resize(n)); PT_CHECK_HIP(c, c->dS2.resize(n)); PT_CHECK_HIP(c, c->dS3.resize(n));
    PT_CHECK_HIP(c, c->dS4.resize(n)); PT_CHECK_HIP(c, c->dHit.resize(n)); PT_CHECK_HIP(c, c->dQueue[0].resize(n)); PT_CHECK_HIP(c, c->dQueue[1].resize(n));
    PT_CHECK_HIP(c, c->dSq0.resize(ns)); PT_CHECK_HIP(c, c->dSq1.resize(ns)); PT_CHECK_HIP(c, c->dSq2.resize(ns));
    PT_CHECK_HIP(c, c->dBestKey.resize(ns)); PT_CHECK_HIP(c, c->dResolveList.resize(ns));
    PT_CHECK_HIP(c, c->dTaskQ.resize((size_t)PT_PIPELINE_BATCHES * 2 * TASK_QUEUE_CAPACITY));
    PT_CHECK_HIP(c, c->dTravCounts.resize(PT_PIPELINE_BATCHES * PASS_COUNTERS));
    c->poolCapacity = n; c->shadowCapacity = ns;
    return PT_OK;
}

// HIP events that are destroyed whichever way a driver returns: the pair around a frame, and the marks around single launches of a batch.
// Those only when somebody reads them (serial-kernel steps, counter frames, the pass log) — ten API calls per pass and batch otherwise.
struct Events {
    std::vector<hipEvent_t> ev;
    Events() = default; Events(const Events&) = delete; Events& operator=(const Events&) = delete;
    ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t record(hipStream_t st) {
        hipEvent_t e = nullptr; const hipError_t r = hipEventCreate(&e); ev.push_back(e);
        return r != hipSuccess ? r : hipEventRecord(e, st);
    }
    size_t mark(hipStream_t st) { (void)record(st); return ev.size() - 1; }
    float ms(size_t a = 0, size_t b = 1) const { float m = 0; (void)hipEventElapsedTime(&m, ev[a], ev[b]); return m; }
};

// The owned pixels are traced as up to PT_PIPELINE_BATCHES independent sub-frame batches, each on its own stream with its own queues,
// counters, task queues and slice of the pool. Paths never interact, so this changes nothing in the result; it lets the k_shade of one batch
// (3 waves per SIMD, mostly waiting on memory) overlap the traversal of the others and hides the ~0.5 ms drain at the end of every launch
// (C3: 241 ms with one batch, 199 ms with four). Small frames use fewer batches, serial-kernel frames one.
struct Batch {
    uint pixFirst = 0, numPix = 0, total = 0, base = 0;      // owned pixels [pixFirst, + numPix); its paths: `total` from slot `base` of the pool
    hipStream_t st = nullptr; WaveCounters* wc = nullptr; WaveCounters* hwc = nullptr;
    PathPool pool; ShadowQueue sq; uint* queue[2] = {nullptr, nullptr}; DeviceScene sc; PathKernelContext k; TravAux aux;
    uint cur = 0, active = 0, iterations = 0; unsigned long long extendRays = 0, shadowRays = 0; bool waiting = false;
};
uint batch_count(const pt_context* c, uint paths) {
    if (c->serialKernels || paths < (1u << 20)) return 1u;
    return paths < PT_PIPELINE_FULL_AT ? (uint)PT_PIPELINE_MID_BATCHES : (uint)PT_PIPELINE_BATCHES;
}
// Batch b of numBatches with all its slices. numPixels: the entries of the pixel list the frame is traced over (the owned list, or pt_render_adaptive's active list);
// pathsPerPixel: pt_render's sample count, 1 in the realtime passes; frameSq: the shadow queue of
// the whole frame (shadowPerPath entries per path); maxBlocks: the grid bound of the batch's traversal launches (0: T8_MAX_BLOCKS). The
// host's copy of the batch's counters is left zeroed.
void slice_batch(pt_context* c, const PathKernelContext& k, uint numPixels, uint b, uint numBatches, uint pathsPerPixel, uint shadowPerPath,
                 const ShadowQueue& frameSq, uint maxBlocks, Batch& t) {
    const unsigned long long numOwned = numPixels;
    t.pixFirst = (uint)(numOwned * b / numBatches); t.numPix = (uint)(numOwned * (b + 1) / numBatches) - t.pixFirst;
    t.total = t.numPix * pathsPerPixel; t.base = t.pixFirst * pathsPerPixel;
    t.st = c->streams[b]; t.wc = c->dCounters.p + b; t.hwc = c->hostCounters + b;
    t.pool = PathPool{c->dS0.p + t.base, c->dS1.p + t.base, c->dS2.p + t.base, c->dS3.p + t.base, c->dS4.p + t.base, c->dHit.p + t.base};
    const size_t sbase = (size_t)t.base * shadowPerPath;
    t.sq = frameSq; t.sq.q0 += sbase; t.sq.q1 += sbase; t.sq.q2 += sbase; if (t.sq.q3) t.sq.q3 += sbase;
    t.queue[0] = c->dQueue[0].p + t.base; t.queue[1] = c->dQueue[1].p + t.base;
    // (finalize_geometry allocates a stack-tail slice of this size for each of PT_PIPELINE_BATCHES batches)
    t.sc = c->dsc; t.sc.travSpill = c->dsc.travSpill + (size_t)b * T8_MAX_BLOCKS * T8_GROUPS_PER_BLOCK * T8_SPILL_DEPTH;
    t.k = k; t.k.sc = t.sc;
    t.aux.taskQ[0] = c->dTaskQ.p + (size_t)(2 * b) * TASK_QUEUE_CAPACITY; t.aux.taskQ[1] = t.aux.taskQ[0] + TASK_QUEUE_CAPACITY;
    t.aux.counts = c->dTravCounts.p + PASS_COUNTERS * b; t.aux.taskCap = TASK_QUEUE_CAPACITY; t.aux.maxBlocks = maxBlocks;
    t.aux.bestKey = c->dBestKey.p + sbase; t.aux.resolveList = c->dResolveList.p + sbase; t.aux.primToSlot = c->bvh.primToSlot;
    memset(t.hwc, 0, sizeof(WaveCounters));
}
PathKernelContext kernel_context(const pt_context* c) { PathKernelContext k; k.sc = c->dsc; k.S = c->S; k.cam = c->cam; return k; }
ShadowQueue frame_shadow_queue(const pt_context* c, uint group) {
    return ShadowQueue{c->dSq0.p, c->dSq1.p, c->dSq2.p, group, nullptr, nullptr, nullptr, 0u, 0u, 0u};
}
// the straggler state of a batch's visibility launches: the batch's own, with the shadow launch's block of pass counters
TravAux shadow_aux(const Batch& t) { TravAux a = t.aux; a.counts = t.aux.counts + PASS_SHADOW_OFFSET; return a; }

// the rejected hits a path may meet in nested dielectrics, each of which costs one more pass (PathTracerNestedDielectrics.hlsli)
uint nested_dielectric_allowance(const ptk::PtSettings& S) { return S.nestedDielectricsQuality == 2 ? 16u : (S.nestedDielectricsQuality == 1 ? 4u : 0u); }

// "A composed frame": one whose passes pt_render may compose freely — tail kernel, fused traversal launches, compacted pool. Not serial-kernel
// and counter frames (their per-kernel attribution is the point), not grouped NEE samples (NEEFullSamples > 1 folds a vertex's samples in
// k_resolve_nee) and not without a tree (the traversal's empty-scene path is per launch, not per wave).
bool composed_frame(const pt_context* c, uint shadowGroup) { return !c->serialKernels && !c->countersEnabled && !shadowGroup && c->dsc.rootIsValid; }

// one finished batch as frame statistics: the host's counts and the batch's WaveCounters, read back whole. The times are not a batch's.
PtFrameStats batch_stats(const Batch& t, uint shadowGroup) {
    const WaveCounters& h = *t.hwc;
    PtFrameStats s; memset(&s, 0, sizeof(s));
    s.extendRays = t.extendRays + h.tailExtendRays; s.shadowRays = shadowGroup ? h.shadowValid : t.shadowRays + h.tailShadowRays; s.hits = h.hits;
    s.nodeVisitsExtend = h.nodeVisitsExt; s.triTestsExtend = h.triTestsExt; s.nodeVisitsShadow = h.nodeVisitsSh; s.triTestsShadow = h.triTestsSh;
    s.leafVisitsExtend = h.leafVisitsExt; s.waveItersExtend = h.itersExt; s.leafVisitsShadow = h.leafVisitsSh; s.waveItersShadow = h.itersSh;
    for (int q = 0; q < 4; q++) s.extendPhaseCycles[q] = h.phaseCycExt[q];
    s.leafBlocksExtend = h.leafBlocksExt; s.waveItersMaxExtend = h.itersMaxExt;
    for (int q = 0; q < 8; q++) s.extendEvents[q] = h.eventsExt[q];
    for (int q = 0; q < 16; q++) s.extendRayIterHist[q] = h.rayIterHistExt[q];
    s.longRayCount = h.longRayCount < 32u ? h.longRayCount : 32u; memcpy(s.longRays, h.longRays, 32 * (size_t)s.longRayCount);
    s.extendLaunches = s.iterations = t.iterations; s.pathsTraced = t.total;
    return s;
}

// The end of every frame, once its streams are drained and the batches' counters are back: a traversal that ran out of room, and paths that
// outlived the pass bound. That bound is a safety net, never what ends a path: a path ends by its own bounce / rejected-hit counters
// (PathTracer.hlsli:40-45, PathTracerNestedDielectrics.hlsli). Were a path still alive here, the set of dropped paths — the image — would
// depend on how the passes were composed (tail threshold): reported, not swallowed.
template <typename B> int32_t check_frame_end(pt_context* c, const B* batches, uint numBatches, const char* stillAlive) {
    for (uint b = 0; b < numBatches; b++)
        if (batches[b].hwc->overflow)
            return fail(c, PT_ERROR_HIP, "BVH8 traversal: stack tail or straggler task queue overflow (raise T8_SPILL_DEPTH / TASK_QUEUE_CAPACITY)");
    for (uint b = 0; b < numBatches; b++) if (batches[b].active) return fail(c, PT_ERROR_HIP, stillAlive);
    return PT_OK;
}
// every batch's counters back to the host, the batch streams and then the main stream drained, the frame's end recorded in between
template <typename B> int32_t drain_frame(pt_context* c, B* batches, uint numBatches, Events& frame) {
    for (uint b = 0; b < numBatches; b++)
        PT_CHECK_HIP(c, hipMemcpyAsync(batches[b].hwc, batches[b].wc, sizeof(WaveCounters), hipMemcpyDeviceToHost, batches[b].st));
    for (uint b = 0; b < numBatches; b++) PT_CHECK_HIP(c, hipStreamSynchronize(batches[b].st));
    PT_CHECK_HIP(c, frame.record(c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}

// ---------------------------------------------------------------- pt_render

struct RenderBatch : Batch {
    uint bound = 0;                       // wavefront passes so far (what maxIter limits; a tail launch is followed by one, so the loop ends)
    uint tailLaunches = 0; bool afterTail = false, inTail = false;
    uint pendingShadow = 0; TravAux auxSh;                          // fused traversal launches (enable_fused)
    PathPool poolSet[2]; uint set = 0; bool compact = false;        // the compacted pool (enable_compact_pool)
    bool firstInPlace = false;                                      // no k_generate: the first pass forms the vertex-0 state itself (enable_first_vertex_in_place)
    FirstPackets packets = {nullptr, nullptr, 0u, 0u, 0u, 0u, 0u};         // ... and traces its camera rays as packets (leftover == nullptr: one by one)
    bool timed = false; Events marks; size_t t0 = 0, t1 = 0;
    struct Span { size_t a, b; int kind; uint items; }; std::vector<Span> spans;      // kind: 0 extend, 1 shade, 2 shadow, 3 tail
    size_t mark() { return timed ? marks.mark(st) : 0; }
    void span(size_t a, size_t b, int kind, uint items) { if (timed) spans.push_back({a, b, kind, items}); }
};

// One frame of render_pixel_list (a pt_render call, a round of pt_render_adaptive): the batches and what every pass of every batch needs to know. pixels / numPixels: the
// device pixel list the frame is traced over, whose pixels all hold accumBase samples; round: pt_render_adaptive's (nullptr: pt_render).
struct RenderFrame {
    pt_context* c; uint first, count, total, shadowGroup, shadowPerPath; bool feedback;
    const uint* pixels; uint numPixels, accumBase; AdaptiveRound* round;
    uint numBatches = 0; RenderBatch B[PT_PIPELINE_BATCHES];
    uint maxIter = 0, tailBelow = 0, wavefrontPasses = 0; bool fused = false, passLog = false;

    bool live(const RenderBatch& t) const { return t.active && t.bound < maxIter; }
    int32_t setup(const PathKernelContext& k) {
        numBatches = batch_count(c, total);
        // developer A/B switches
        static const uint batchesOverride = []() { const char* e = getenv("MI355PT_BATCHES"); return e ? (uint)strtoul(e, nullptr, 10) : 0u; }();
        static const uint blocksOverride = []() { const char* e = getenv("MI355PT_MAX_BLOCKS"); return e ? (uint)strtoul(e, nullptr, 10) : 0u; }();
        if (batchesOverride && !c->serialKernels) numBatches = batchesOverride < (uint)PT_PIPELINE_BATCHES ? batchesOverride : (uint)PT_PIPELINE_BATCHES;
        // pipelined batches: one GPU-full of blocks per traversal launch (pt_scene.h PT_T8_MAX_BLOCKS) — and fewer for the launches of a small
        // frame (one rank of a sharded frame): every wave then works through more chunks before it runs dry and fewer of its rays are cut into
        // sub-trees; the other batches keep the GPU full. profiles/r05q_grid_cap_ab.txt: a rank of eight (4.1 M paths) 896 blocks -1 ... -3 %, a
        // rank of four / two 1120 blocks -1 %, the full frame (33 M paths) +1 % with either: hence by size.
        uint maxBlocks = (numBatches >= 3u) ? (total < (6u << 20) ? 256u * 7u / 2u : (total < (24u << 20) ? 256u * 35u / 8u : 256u * 7u)) : 0u;
        // (clamped: a batch's stack-tail slice is sized for T8_MAX_BLOCKS blocks, and launch_trace_pair splits its grid in two)
        if (blocksOverride) maxBlocks = blocksOverride < 2u ? 2u : (blocksOverride < T8_MAX_BLOCKS ? blocksOverride : (uint)T8_MAX_BLOCKS);
        ShadowQueue sq = frame_shadow_queue(c, shadowGroup);
        if (feedback) {
            sq.q3 = c->dSq3.p; sq.fbTotalWeight = c->neeat.enabled ? c->neeat.fbW.p : c->dFbWeight.p;
            sq.fbCandidates = c->neeat.enabled ? c->neeat.fbC.p : c->dFbCand.p;
            sq.fbWidth = c->width; sq.fbPlane = c->width * c->height; sq.fbSampleFirst = first;
        }
        passLog = getenv("MI355PT_PASS_LOG") != nullptr;
        for (uint b = 0; b < numBatches; b++) {
            RenderBatch& t = B[b];
            slice_batch(c, k, numPixels, b, numBatches, count, shadowPerPath, sq, maxBlocks, t);
            t.timed = c->serialKernels || c->countersEnabled || passLog;
            t.hwc->extendCount[0] = t.active = t.total;
        }
        // upper bound on extend passes: bounceCount + 1 vertices plus rejected (nested dielectric) re-traces
        maxIter = c->S.bounceCount + 2 + nested_dielectric_allowance(c->S);
        // the tail kernel takes over a batch once it holds at most this many paths (0: never)
        const bool composed = composed_frame(c, shadowGroup);
        tailBelow = composed ? c->tailBelow : 0u;
        const bool fuse = composed && (c->fusedTraversal == 1u || (c->fusedTraversal == 2u && total < PT_FUSED_BELOW));
        if (fuse) { int32_t r = enable_fused(); if (r != PT_OK) return r; }
        // (the compacted pool is not for NEE-AT either: its visibility resolve patches the path's flags)
        const bool neeatShade = c->dsc.lights.LocalSamplingBuffer != nullptr || c->dsc.lights.TemporalFeedbackRequired != 0u;
        if (composed && c->compactPool && !neeatShade && !feedback) {
            int32_t r = enable_compact_pool(); if (r != PT_OK) return r;
            if (c->firstVertexInPlace) { enable_first_vertex_in_place(); if (c->firstVertexPackets) { r = enable_first_vertex_packets(); if (r != PT_OK) return r; } }
        }
        return PT_OK;
    }
    // Fused traversal launches (pt_set_fused_traversal, k_trace_pair): the visibility rays a bounce's shading leaves in the shadow queue are not
    // traced in a launch of their own but wait (RenderBatch::pendingShadow) for the next bounce's closest-hit launch and share it — and its task
    // rounds and resolve pass — block by block. Nothing of vertex k + 1 needs the visibility of vertex k before vertex k + 1 is shaded (the order
    // of the fp16 additions into a path's L), and that is exactly where the fused launch sits, so the image cannot change; the visibility rays
    // need their own task queues, merge keys and resolve list (auxSh). A batch whose paths have ended, or which goes to the tail kernel, traces
    // what is pending in a plain visibility launch first. Composed frames only.
    int32_t enable_fused() {
        PT_CHECK_HIP(c, c->dBestKeySh.resize(c->shadowCapacity)); PT_CHECK_HIP(c, c->dResolveListSh.resize(c->shadowCapacity));
        PT_CHECK_HIP(c, c->dTaskQSh.resize((size_t)PT_PIPELINE_BATCHES * 2 * TASK_QUEUE_CAPACITY));
        for (uint b = 0; b < numBatches; b++) {
            RenderBatch& t = B[b]; const size_t sbase = (size_t)t.base * shadowPerPath;
            t.auxSh = shadow_aux(t);
            t.auxSh.taskQ[0] = c->dTaskQSh.p + (size_t)(2 * b) * TASK_QUEUE_CAPACITY; t.auxSh.taskQ[1] = t.auxSh.taskQ[0] + TASK_QUEUE_CAPACITY;
            t.auxSh.bestKey = c->dBestKeySh.p + sbase; t.auxSh.resolveList = c->dResolveListSh.p + sbase;
        }
        fused = true;
        return PT_OK;
    }
    // Compacted pool (ptk::PathPool::home). A path's state lives at its home slot (owned pixel x sample) for the whole frame in the plain layout,
    // and from the second bounce on the survivors are scattered over the pool: a wave's 64 paths touch up to 64 lines per word group where the
    // first bounce touches 8. Here k_shade writes a survivor's origin, direction, interior list | counters | ray cone and {firefly K, MIS info,
    // flags, sample index} at the POSITION it appends the path to, into the other of two array sets; the next bounce's traversal reads rays, and
    // writes hits, by position (the extend queue is the identity), k_classify and k_shade read dense arrays. Only throughput | radiance — what
    // the visibility resolve and k_accumulate address by path — stays at the home slot, which the extend queue keeps carrying (and the shadow
    // queue names). Same values, another place: the image cannot change. A batch that goes to the tail kernel is scattered back to its home slots
    // first (k_uncompact) and continues in the home-slot layout. Composed frames without NEE-AT only. Costs five more uint4 arrays per path.
    int32_t enable_compact_pool() {
        PT_CHECK_HIP(c, c->dS0b.resize(c->poolCapacity)); PT_CHECK_HIP(c, c->dS1b.resize(c->poolCapacity)); PT_CHECK_HIP(c, c->dS3b.resize(c->poolCapacity));
        PT_CHECK_HIP(c, c->dS4b.resize(c->poolCapacity)); PT_CHECK_HIP(c, c->dHitb.resize(c->poolCapacity));
        for (uint b = 0; b < numBatches; b++) {
            RenderBatch& t = B[b]; t.compact = true; t.set = 0; t.poolSet[0] = t.pool;
            t.poolSet[1] = PathPool{c->dS0b.p + t.base, c->dS1b.p + t.base, t.pool.s2, c->dS3b.p + t.base, c->dS4b.p + t.base, c->dHitb.p + t.base, nullptr};
        }
        return PT_OK;
    }
    // Vertex 0 in place (ptk::FirstVertex). k_generate writes 80 bytes of state and a queue word per path, and the first pass reads them back: the
    // ray in k_extend, the flags word in k_classify, everything in k_shade — none of which holds information: at vertex 0 a path's state is its
    // camera ray, its pixel id and sample index, and constants of the frame. A compacted batch whose first pass is a wavefront pass therefore
    // starts without k_generate, and that pass launches k_extend_first, k_classify<UNIFORM> and k_shade<..., FIRST>, which form what they
    // need. Who else reads vertex-0 state, and why each is covered:
    //  - the task rounds and the resolve pass behind k_extend_first read s0 / s1 of rays cut into sub-trees: k_extend_first writes those;
    //  - k_shade's survivors and every s2 go where PathCompactIO's go, so pass 1 and the visibility resolve find what they always found;
    //  - k_accumulate reads s2 at the home slots: every path is shaded at vertex 0, alive or not, and k_shade writes its s2 there;
    //  - the tail kernel and k_uncompact read the pool: a batch small enough to START in the tail kernel keeps k_generate (below); a batch
    //    that gets there later is past vertex 0;
    //  - the extend queue (pool.home) of pass 0 would be the identity: the three launches use the position instead.
    // Serial-kernel and counter frames, grouped NEE samples, NEE-AT and feedback frames are not compacted and keep k_generate as well.
    void enable_first_vertex_in_place() {
        for (uint b = 0; b < numBatches; b++) {
            RenderBatch& t = B[b]; t.firstInPlace = t.compact && !(tailBelow && t.total <= tailBelow);
            t.hwc->firstCamera.cam = t.k.cam; t.hwc->firstCamera.perPixelJitterAAScale = t.k.S.perPixelJitterAAScale;      // (uploaded with the block by start())
        }
    }
    // Vertex 0 as packets (ptk::FirstPackets, pt_traverse8k.h). The camera rays of 32 consecutive paths — 8 x 1 pixels x 4 samples of an 8 x 8 block of the owned-pixel list at
    // 4 spp — walk almost the same nodes, and one ray per lane pair repeats the per-ray bookkeeping 32 times over. k_extend_first_packets walks them on one stack per wave;
    // the packets over the step cap leave their rays on the batch's slice of dFirstLeftover (count: word PASS_LEFTOVER of the pass's counter block, zeroed with it), and
    // k_extend_first's loop traces those behind it, straggler machinery included. Same hits at the same positions: nothing else of the pass knows.
    // c->firstVertexPackets == 2 (the default): 64-ray packets, one lane per ray — two rows of the block — through k_extend_first_packets64 (traverse8_packets64), step cap
    // T8_PACKET64_STEP_CAP; 1: the 32-ray packets above.
    int32_t enable_first_vertex_packets() {
        PT_CHECK_HIP(c, c->dFirstLeftover.resize(c->poolCapacity));
        for (uint b = 0; b < numBatches; b++) {
            RenderBatch& t = B[b]; if (!t.firstInPlace) continue;
            t.packets = first_packets(c, c->dFirstLeftover.p + t.base, t.aux.counts + PASS_LEFTOVER, t.total, c->packetStepCap, c->packetStack);
        }
        return PT_OK;
    }
    int32_t start() {
        for (uint b = 0; b < numBatches; b++) {
            RenderBatch& t = B[b];
            t.t0 = t.mark();
            PT_CHECK_HIP(c, hipMemcpyAsync(t.wc, t.hwc, sizeof(WaveCounters), hipMemcpyHostToDevice, t.st));
            if (!t.firstInPlace) launch_generate(t.k, t.pool, pixels + t.pixFirst, t.numPix, first, count, 0u, t.total, t.queue[0], nullptr, t.st);
        }
        return PT_OK;
    }
    // One pass of a batch is queued by queue_pass (counter reset, traversal — fused with the pending visibility rays — classify + shade,
    // read-back of the two queue counts) and finished by finish_pass once those counts have arrived (the visibility rays become pending, or are
    // traced if the batch ends here).
    int32_t queue_pass(RenderBatch& t) {
        const uint nxt = t.cur ^ 1u;
        // the pass's traversal / class counters and the two queue counters it refills: one launch (fused: the shadow queue's counter still counts
        // the pending rays; k_resolve_pair zeroes it)
        launch_pass_reset(t.aux.counts, &t.wc->extendCount[nxt], fused ? nullptr : &t.wc->shadowCount, t.st);
        if (tailBelow && t.active <= tailBelow && !t.afterTail) return queue_tail(t);
        t.afterTail = false; t.bound++; wavefrontPasses++;
        const size_t e0 = t.mark();
        PathPool pin = t.pool, pout = PathPool{};
        if (t.compact) { pin = t.poolSet[t.set]; pin.home = t.queue[t.cur]; pout = t.poolSet[t.set ^ 1u]; t.set ^= 1u; }
        const uint* countIn = &t.wc->extendCount[t.cur];
        // (pass 0 of a batch has no visibility rays pending)
        const bool vertex0 = t.firstInPlace && t.iterations == 0u;
        const FirstVertex fv{pixels + t.pixFirst, t.numPix, first, count};
        if (vertex0) launch_extend_first(t.k, pin, fv, countIn, t.active, t.wc, t.aux, t.packets, t.st);
        else if (t.pendingShadow) {
            launch_trace_pair(t.sc, pin, t.queue[t.cur], countIn, t.active, t.sq, &t.wc->shadowCount, t.pendingShadow, t.wc, t.aux, t.auxSh, t.st);
            t.pendingShadow = 0;
        } else launch_extend(t.sc, pin, t.queue[t.cur], countIn, t.active, t.wc, c->countersEnabled, t.aux, t.st);
        const size_t e1 = t.mark(); t.span(e0, e1, 0, t.active);
        // the straggler keys are idle between k_resolve_extend and the shadow launch: k_classify's scratch. A few thousand paths are shaded in
        // queue order: one launch fewer
        uint* classScratch = t.active >= PT_CLASSIFY_FROM ? reinterpret_cast<uint*>(t.aux.bestKey) : nullptr;
        launch_shade(t.k, pin, t.queue[t.cur], countIn, t.active, t.queue[nxt], &t.wc->extendCount[nxt], t.sq, t.wc, classScratch,
                     t.aux.counts + PASS_CLASS_OFFSET, t.st, pout, vertex0 ? &fv : nullptr, c->dropInertTerminal ? c->dInertBits.p : nullptr);
        const size_t e2 = t.mark(); t.span(e1, e2, 1, t.active);
        t.extendRays += t.active;
        PT_CHECK_HIP(c, hipMemcpyAsync(t.hwc, t.wc, 16, hipMemcpyDeviceToHost, t.st));
        t.waiting = true;
        return PT_OK;
    }
    // few paths left: one launch runs them to their end, wave by wave (pt_tail.hip); stragglers come back through queue[nxt] / the shadow queue
    int32_t queue_tail(RenderBatch& t) {
        const uint nxt = t.cur ^ 1u;
        if (t.compact) {      // the tail kernel works on home slots: scatter the live paths back, into the array set that is not being read
            PathPool in = t.poolSet[t.set]; in.home = t.queue[t.cur];
            launch_uncompact(in, t.poolSet[t.set ^ 1u], &t.wc->extendCount[t.cur], t.active, t.st);
            t.pool = t.poolSet[t.set ^ 1u]; t.compact = false;
        }
        if (t.pendingShadow) {      // (the tail kernel adds to the paths' radiance itself: what is pending lands first)
            launch_shadow(t.sc, t.pool, t.sq, &t.wc->shadowCount, t.pendingShadow, t.wc, false, t.auxSh, t.st);
            PT_CHECK_HIP(c, hipMemsetAsync(&t.wc->shadowCount, 0, 4, t.st));
            t.pendingShadow = 0;
        }
        const size_t e0 = t.mark();
        launch_tail(t.k, t.pool, t.queue[t.cur], &t.wc->extendCount[t.cur], t.active, t.queue[nxt], &t.wc->extendCount[nxt], t.sq, t.wc, maxIter - t.bound,
                    c->tailDefer, t.aux.maxBlocks, t.st);
        const size_t e1 = t.mark(); t.span(e0, e1, 3, t.active);
        // what comes back — stragglers — is traced by a wavefront pass (task rounds included) before the tail kernel gets another turn
        t.tailLaunches++; t.afterTail = true; t.inTail = true;
        PT_CHECK_HIP(c, hipMemcpyAsync(t.hwc, t.wc, 16, hipMemcpyDeviceToHost, t.st));
        t.waiting = true;
        return PT_OK;
    }
    int32_t finish_pass(RenderBatch& t, uint b) {
        t.waiting = false; t.inTail = false;
        const uint nxt = t.cur ^ 1u, nShadow = t.hwc->shadowCount;
        // the pass's straggler counters: sub-trees split off by k_extend and by task rounds 0..2, rays sent to the resolve pass (the previous
        // pass's shadow launch is reported with the next line)
        if (passLog) {
            uint pc[PASS_COUNTERS]; PT_CHECK_HIP(c, hipMemcpy(pc, t.aux.counts, sizeof(pc), hipMemcpyDeviceToHost));
            fprintf(stderr, "[pass log]   b%u pass %u: %u paths -> extend splits %u / %u / %u / %u sub-trees, %u rays resolved; %u visibility rays next\n",
                    b, t.iterations, t.active, pc[0], pc[1], pc[2], pc[3], pc[TRAV_RESOLVE], nShadow);
            if (t.packets.leftover && t.iterations == 0u)
                fprintf(stderr, "[pass log]   b%u pass 0: %u of %u camera rays left over by the packets (step cap %u, stack %u)\n", b, pc[PASS_LEFTOVER], t.active, t.packets.stepCap, t.packets.stackBound);
            if (t.active >= PT_CLASSIFY_FROM)
                fprintf(stderr, "[pass log]   b%u pass %u: classes %u continuing / %u terminating / %u misses, %u inert terminating hits dropped\n",
                        b, t.iterations, pc[PASS_CLASS_OFFSET], pc[PASS_CLASS_OFFSET + 1], pc[PASS_CLASS_OFFSET + 2], pc[PASS_CLASS_OFFSET + 3]);
        }
        t.active = t.hwc->extendCount[nxt];
        if (fused && nShadow && live(t)) { t.pendingShadow = nShadow; t.shadowRays += nShadow; }      // they ride with the next closest-hit launch
        else if (nShadow) {
            const size_t s0 = t.mark();
            launch_shadow(t.sc, t.pool, t.sq, &t.wc->shadowCount, nShadow, t.wc, c->countersEnabled, fused ? t.auxSh : shadow_aux(t), t.st);
            const size_t s1 = t.mark(); t.span(s0, s1, 2, nShadow);
            if (!shadowGroup) t.shadowRays += nShadow;
            if (fused) PT_CHECK_HIP(c, hipMemsetAsync(&t.wc->shadowCount, 0, 4, t.st));
        }
        t.cur = nxt; t.iterations++;
        return PT_OK;
    }
    // Batches run in lockstep: a batch's next pass is queued when ALL batches have delivered their counts (queue all, then service each as its
    // counts arrive), which keeps one batch's shading next to the others' traversal. Free-running streams drift into running the same kernel at
    // the same time: 7 % slower on the full frame and no gain on a rank of a sharded frame (profiles/r04i_event_loop_ab.txt).
    // Small passes are another matter. The lockstep pays while every pass fills the GPU; at the end of a frame — and for the whole of a small
    // frame — a pass is a chain of a dozen short launches, the batches no longer take equally long, and in lockstep three streams sit idle until
    // the slowest has delivered its counts (0.7 - 1 ms per late pass of the 4K frame, profiles/r06i_*). So once every live batch holds fewer
    // than `freeRunBelow` paths, lockstep() queues that round's passes and returns with them in flight: free_run() takes over. Otherwise it
    // returns when every batch has ended.
    int32_t lockstep() {
        static const uint freeRunBelow = []() {
            const char* e = getenv("MI355PT_FREE_RUN_BELOW"); return e ? (uint)strtoul(e, nullptr, 10) : (uint)PT_FREE_RUN_BELOW;
        }();
        for (;;) {
            bool freeRun = freeRunBelow != 0u && numBatches > 1u;
            for (uint b = 0; b < numBatches; b++) if (live(B[b]) && B[b].active >= freeRunBelow) freeRun = false;
            // phase 1: every live batch queues extend + shade and the read-back of its queue counts
            wavefrontPasses = 0;
            for (uint b = 0; b < numBatches; b++) {
                RenderBatch& t = B[b];
                if (t.waiting || !live(t)) continue;      // waiting: a tail launch still in flight (below); the batch rejoins the lockstep when it is done
                int32_t r = queue_pass(t); if (r != PT_OK) return r;
            }
            if (freeRun) return PT_OK;
            // phase 2: as each batch's counts arrive, its visibility rays become pending (or are traced, if the batch ends); the other batches
            // keep the GPU busy meanwhile
            bool any = false;
            for (uint b = 0; b < numBatches; b++) {
                RenderBatch& t = B[b];
                if (!t.waiting) continue;
                // a tail launch runs for about a millisecond — several of the other batches' passes: while those have wavefront passes to queue, it
                // is only polled
                if (t.inTail && wavefrontPasses && hipStreamQuery(t.st) == hipErrorNotReady) { any = true; continue; }
                PT_CHECK_HIP(c, hipStreamSynchronize(t.st));
                int32_t r = finish_pass(t, b); if (r != PT_OK) return r;
                if (live(t)) any = true;
            }
            if (!any) return PT_OK;
        }
    }
    // event-driven until every batch has ended: whichever batch's counts arrive first is finished and its next pass queued at once (nothing is in
    // flight, and nothing happens here, when lockstep() ran the frame to its end)
    int32_t free_run() {
        uint waiting = 0; for (uint b = 0; b < numBatches; b++) waiting += B[b].waiting ? 1u : 0u;
        while (waiting) {
            for (uint b = 0; b < numBatches; b++) {
                RenderBatch& t = B[b];
                if (!t.waiting || hipStreamQuery(t.st) == hipErrorNotReady) continue;
                PT_CHECK_HIP(c, hipStreamSynchronize(t.st));
                int32_t r = finish_pass(t, b); if (r != PT_OK) return r;
                waiting--;
                if (live(t)) { r = queue_pass(t); if (r != PT_OK) return r; waiting++; }
            }
        }
        return PT_OK;
    }
    void accumulate() {
        for (uint b = 0; b < numBatches; b++) {
            RenderBatch& t = B[b];
            if (round) launch_adaptive_accumulate(t.pool, pixels + t.pixFirst, t.numPix, count, c->dAccum.p, round->half, round->counts, accumBase, c->width, t.st);
            else launch_accumulate(t.pool, pixels + t.pixFirst, t.numPix, count, c->dAccum.p, accumBase, c->width, t.st);
            t.t1 = t.mark();
        }
    }
    // pt_render_adaptive's evaluation behind the round's accumulation: the main stream waits for every batch's, runs the error and compaction launches between two events of
    // `ev` (returned through a / b) and sends the new lists' sizes to the host. drain_frame's synchronisation of the main stream is what the host waits on: no point of its own.
    int32_t evaluate(Events& ev, size_t& a, size_t& b) {
        for (uint q = 0; q < numBatches; q++) {
            if (B[q].st == c->stream) continue;
            PT_CHECK_HIP(c, ev.record(B[q].st)); PT_CHECK_HIP(c, hipStreamWaitEvent(c->stream, ev.ev.back(), 0));
        }
        PT_CHECK_HIP(c, ev.record(c->stream)); a = ev.ev.size() - 1;
        launch_adaptive_evaluate(round->eval, c->stream);
        PT_CHECK_HIP(c, ev.record(c->stream)); b = ev.ev.size() - 1;
        PT_CHECK_HIP(c, hipMemcpyAsync(round->hostTotals, round->eval.totals, 2 * sizeof(uint), hipMemcpyDeviceToHost, c->stream));
        return PT_OK;
    }
    // frameMs: from the first batch's start to the last batch's end (all streams were idle before and are drained now)
    void harvest(PtFrameStats& stats, float frameMs) const {
        for (uint b = 0; b < numBatches; b++) {
            const RenderBatch& t = B[b];
            PtFrameStats s = batch_stats(t, shadowGroup);
            s.tailLaunches = t.tailLaunches;
            for (const RenderBatch::Span& sp : t.spans) {      // (none in pipelined frames: no per-launch events there)
                const float m = t.marks.ms(sp.a, sp.b);
                if (sp.kind == 0) s.extendKernelMs += m; else if (sp.kind == 1) s.shadeKernelMs += m; else if (sp.kind == 2) s.shadowKernelMs += m;
            }
            add_frame_stats(stats, s);
        }
        stats.gpuMilliseconds = frameMs;
    }
    // developer probe (MI355PT_PASS_LOG): the launch sequence of every batch with item counts and HIP-event durations (stderr)
    void log_passes() const {
        static const char* const kinds[4] = {"extend", "shade", "shadow", "tail"};
        for (uint b = 0; b < numBatches; b++) {
            const RenderBatch& t = B[b]; const WaveCounters& h = *t.hwc;
            if (t.tailLaunches)
                fprintf(stderr, "[pass log] batch %u: %u tail launches traced %llu + %llu rays, handed back %llu extend stragglers, "
                        "%llu visibility stragglers, %llu paths at the bounce bound\n", b, t.tailLaunches, (unsigned long long)h.tailExtendRays,
                        (unsigned long long)h.tailShadowRays, (unsigned long long)h.tailHandedBack[0], (unsigned long long)h.tailHandedBack[1],
                        (unsigned long long)h.tailHandedBack[2]);
            if (!t.timed) continue;
            fprintf(stderr, "[pass log] batch %u of %u: %u paths, %u passes, %.3f ms from first to last event\n", b, numBatches, t.total, t.iterations,
                    t.marks.ms(t.t0, t.t1));
            for (const RenderBatch::Span& sp : t.spans)
                fprintf(stderr, "[pass log]   b%u %-6s %9u items  start %8.3f ms  %7.3f ms\n", b, kinds[sp.kind], sp.items, t.marks.ms(t.t0, sp.a),
                        t.marks.ms(sp.a, sp.b));
        }
    }
};

// NEE-AT with the baker in the loop: every sample is a frame — baker passes, then the path tracer
int32_t render_sample_by_sample(pt_context* c, uint32_t first, uint32_t count, PtFrameStats* stats) {
    PtFrameStats total; memset(&total, 0, sizeof(total));
    int32_t r = PT_OK;
    for (uint32_t s = 0; s < count && r == PT_OK; s++) {
        PtFrameStats one; r = pt_render(c, first + s, 1, &one);
        if (r == PT_OK) add_frame_stats(total, one);
    }
    if (stats) *stats = total;      // (the samples before a failing one were accumulated: their counts are reported)
    return r;
}
// NEE-AT's inputs and outputs of a pt_render call: the local layer must cover the frame, the feedback planes are cleared
int32_t prepare_neeat_layers(pt_context* c, uint32_t count, bool feedback, uint shadowGroup) {
    if (c->localResX) {      // every pixel's (jittered) tile must exist, and a table can only name lights that were baked
        const uint TILE_PX = ptk::RTXPT_LIGHTING_SAMPLING_BUFFER_TILE_SIZE;
        if ((c->width - 1u + c->localJitterX) / TILE_PX >= c->localResX || (c->height - 1u + c->localJitterY) / TILE_PX >= c->localResY)
            return fail(c, PT_ERROR_INVALID_ARGUMENT, "local sampling table smaller than the frame");
        if (c->localMaxLight >= c->lights.size())
            return fail(c, PT_ERROR_INVALID_ARGUMENT, "local sampling table names a light index beyond the baked light table");
    }
    c->fbSamples = 0;
    if (!feedback) return PT_OK;
    if (shadowGroup)
        return fail(c, PT_ERROR_INVALID_ARGUMENT, "NEE-AT temporal feedback needs NEEFullSamples 1 (the reference's default): the feedback draw of one light "
                                                  "sample shifts the random numbers of the next");
    const size_t plane = (size_t)c->width * c->height;
    PT_CHECK_HIP(c, c->dSq3.resize(c->shadowCapacity));
    if (!c->neeat.enabled) {      // (with the baker in the loop the run's own reservoirs are the target: they carry what the Clear pass kept)
        PT_CHECK_HIP(c, c->dFbWeight.resize(plane * count)); PT_CHECK_HIP(c, c->dFbCand.resize(plane * count));
        PT_CHECK_HIP(c, hipMemsetAsync(c->dFbWeight.p, 0, 4 * plane * count, c->stream));
        PT_CHECK_HIP(c, hipMemsetAsync(c->dFbCand.p, 0xFF, 4 * plane * count, c->stream));      // LightFeedbackReservoir::Clear
    }
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

// ---------------------------------------------------------------- pt_fill_stable_planes

struct FillBatch : Batch { PathPool markPool; ptk::float4* newL = nullptr; };

// One fill pass. Batches as in pt_render, advancing in lockstep to the end. The loop is the fill pass's own: its passes are other launches
// (k_sp_fill_shade, the resolve after every visibility launch) and it has neither tail launches to poll nor a free-running end, so sharing
// lockstep would put the question "which caller am I" into every phase of it. What is shared is the batch.
struct FillFrame {
    pt_context* c; StablePlanesContext sp; uint sampleIndex; bool feedback;
    uint numBatches = 0, maxIter = 0; FillBatch B[PT_PIPELINE_BATCHES];

    bool live(const FillBatch& t) const { return t.active && t.iterations < maxIter; }
    void commit() { for (uint b = 0; b < numBatches; b++) launch_sp_fill_commit(B[b].k, sp, B[b].pool, B[b].numPix, sampleIndex, B[b].st); }
    void setup(const PathKernelContext& k) {
        numBatches = batch_count(c, (uint)c->owned.size());
        ShadowQueue sq = frame_shadow_queue(c, 0u);
        // feedback: the fourth word group of an entry and the reservoir planes; the reference mode's shadow kernels then apply the reservoir update
        // and the roulette fix-up of a visible entry themselves (pt_trace.hip shadow_visible; one slot per pixel: plane stride 0)
        if (feedback) {
            sq.q3 = c->dSq3.p; sq.fbTotalWeight = c->neeat.fbW.p; sq.fbCandidates = c->neeat.fbC.p;
            sq.fbWidth = c->width; sq.fbPlane = 0u; sq.fbSampleFirst = 0u;
        }
        for (uint b = 0; b < numBatches; b++) {
            FillBatch& t = B[b];
            slice_batch(c, k, (uint)c->owned.size(), b, numBatches, 1u, 1u, sq, (numBatches >= 3u) ? 256u * 7u : 0u, t);
            t.markPool = t.pool; t.markPool.s2 = c->dSpMark.p + t.base; t.newL = c->dSpNewL.p + t.base;
        }
        maxIter = c->S.bounceCount + 2 + nested_dielectric_allowance(c->S) * (c->S.bounceCount + 1u);
    }
    // the pixels that have something to fill: k_sp_fill_generate counts them on the device
    int32_t start() {
        for (uint b = 0; b < numBatches; b++) {
            FillBatch& t = B[b];
            PT_CHECK_HIP(c, hipMemcpyAsync(t.wc, t.hwc, sizeof(WaveCounters), hipMemcpyHostToDevice, t.st));
            launch_sp_fill_generate(t.k, sp, t.pool, c->dOwned.p + t.pixFirst, t.numPix, sampleIndex, t.queue[0], &t.wc->extendCount[0], t.st);
            PT_CHECK_HIP(c, hipMemcpyAsync(t.hwc, t.wc, 16, hipMemcpyDeviceToHost, t.st));
        }
        for (uint b = 0; b < numBatches; b++) { PT_CHECK_HIP(c, hipStreamSynchronize(B[b].st)); B[b].active = B[b].hwc->extendCount[0]; }
        return PT_OK;
    }
    int32_t queue_pass(FillBatch& t) {
        const uint nxt = t.cur ^ 1u;
        launch_pass_reset(t.aux.counts, &t.wc->extendCount[nxt], &t.wc->shadowCount, t.st);
        launch_extend(t.sc, t.pool, t.queue[t.cur], &t.wc->extendCount[t.cur], t.active, t.wc, c->countersEnabled, t.aux, t.st,
                      /*ranged*/ t.iterations == 0u && PT_SP_FILL_RANGED);
        // (the straggler keys are idle between k_resolve_extend and the shadow launch, as in pt_render)
        uint* classScratch = (PT_SP_FILL_CLASSES && t.active >= PT_CLASSIFY_FROM) ? reinterpret_cast<uint*>(t.aux.bestKey) : nullptr;
        launch_sp_fill_shade(t.k, sp, t.pool, t.queue[t.cur], &t.wc->extendCount[t.cur], t.active, t.queue[nxt], &t.wc->extendCount[nxt], t.sq, t.newL,
                             sampleIndex, t.wc, classScratch, t.aux.counts + PASS_CLASS_OFFSET, t.st);
        t.extendRays += t.active;
        PT_CHECK_HIP(c, hipMemcpyAsync(t.hwc, t.wc, 16, hipMemcpyDeviceToHost, t.st));
        t.waiting = true;
        return PT_OK;
    }
    int32_t finish_pass(FillBatch& t) {
        t.waiting = false;
        const uint nxt = t.cur ^ 1u, nShadow = t.hwc->shadowCount;
        if (nShadow) {
            launch_shadow(t.sc, t.markPool, t.sq, &t.wc->shadowCount, nShadow, t.wc, c->countersEnabled, shadow_aux(t), t.st);
            launch_sp_fill_resolve(t.pool, t.markPool.s2, t.sq, t.newL, &t.wc->shadowCount, nShadow, t.st);
            t.shadowRays += nShadow;
        }
        t.active = t.hwc->extendCount[nxt]; t.cur = nxt; t.iterations++;
        return PT_OK;
    }
    int32_t lockstep() {
        for (bool any = true; any;) {
            // phase 1: every live batch queues extend + shade and the read-back of its queue counts
            for (uint b = 0; b < numBatches; b++) if (live(B[b])) { int32_t r = queue_pass(B[b]); if (r != PT_OK) return r; }
            // phase 2: as each batch's counts arrive, its visibility rays and their resolve; the other batches keep the GPU busy meanwhile
            any = false;
            for (uint b = 0; b < numBatches; b++) {
                FillBatch& t = B[b];
                if (!t.waiting) continue;
                PT_CHECK_HIP(c, hipStreamSynchronize(t.st));
                int32_t r = finish_pass(t); if (r != PT_OK) return r;
                if (live(t)) any = true;
            }
        }
        return PT_OK;
    }
};

// ---------------------------------------------------------------- pt_build_stable_planes

// the realtime mode's per-frame buffers for the context's frame size; a new size: nothing of the old frame is meaningful (pixels of other
// ranks' tiles and the records of planes that do not exist stay zero)
int32_t ensure_stable_planes(pt_context* c, uint planeStride) {
    const size_t N = (size_t)c->width * c->height, planes = (size_t)cStablePlaneCount * planeStride;
    PT_CHECK_HIP(c, c->dSpHeader.resize(4 * N)); PT_CHECK_HIP(c, c->dSpPlanes.resize(planes)); PT_CHECK_HIP(c, c->dSpRadiance.resize(N));
    PT_CHECK_HIP(c, c->dSpMotion.resize(N)); PT_CHECK_HIP(c, c->dSpDepth.resize(N)); PT_CHECK_HIP(c, c->dSpHitT.resize(N));
    PT_CHECK_HIP(c, c->dSpThroughput.resize(N));
    if (c->spW == c->width && c->spH == c->height) return PT_OK;
    PT_CHECK_HIP(c, hipMemsetAsync(c->dSpHeader.p, 0xFF, 16 * N, c->stream));
    PT_CHECK_HIP(c, hipMemsetAsync(c->dSpPlanes.p, 0, sizeof(ptk::StablePlane) * planes, c->stream));
    PT_CHECK_HIP(c, hipMemsetAsync(c->dSpRadiance.p, 0, 8 * N, c->stream)); PT_CHECK_HIP(c, hipMemsetAsync(c->dSpMotion.p, 0, 8 * N, c->stream));
    PT_CHECK_HIP(c, hipMemsetAsync(c->dSpDepth.p, 0, 4 * N, c->stream)); PT_CHECK_HIP(c, hipMemsetAsync(c->dSpHitT.p, 0, 4 * N, c->stream));
    PT_CHECK_HIP(c, hipMemsetAsync(c->dSpThroughput.p, 0, 4 * N, c->stream));
    c->spW = c->width; c->spH = c->height;
    return PT_OK;
}
// the build pass's loop: one batch on the context's main stream, every pass awaited before the next is queued
int32_t build_passes(pt_context* c, const StablePlanesContext& sp, uint sampleIndex, uint maxIter, Batch& t) {
    while (t.active && t.iterations < maxIter) {
        const uint nxt = t.cur ^ 1u;
        launch_pass_reset(t.aux.counts, &t.wc->extendCount[nxt], &t.wc->shadowCount, t.st);
        launch_extend(t.sc, t.pool, t.queue[t.cur], &t.wc->extendCount[t.cur], t.active, t.wc, c->countersEnabled, t.aux, t.st);
        launch_sp_build_shade(t.k, sp, t.pool, t.queue[t.cur], &t.wc->extendCount[t.cur], t.active, t.queue[nxt], &t.wc->extendCount[nxt], sampleIndex, t.wc,
                              t.st);
        t.extendRays += t.active;
        PT_CHECK_HIP(c, hipMemcpyAsync(t.hwc, t.wc, 16, hipMemcpyDeviceToHost, t.st));
        PT_CHECK_HIP(c, hipStreamSynchronize(t.st));
        t.active = t.hwc->extendCount[nxt]; t.cur = nxt; t.iterations++;
    }
    return PT_OK;
}

} // namespace

extern "C" {

int32_t pt_render(pt_context* c, uint32_t first, uint32_t count, PtFrameStats* stats) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    if (c->adaptive.perPixel)
        return fail(c, PT_ERROR_NOT_READY, "the accumulation buffer holds an adaptive render (per-pixel sample counts): pt_reset_accumulation first");
    if (!count) return PT_OK;
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    if (c->neeat.enabled && c->S.NEEEnabled && c->S.NEEFullSamples != 0u) {
        if (count > 1) return render_sample_by_sample(c, first, count, stats);
        // (tile shards with a communicator; a host without one exchanges through pt_neeat_pack / unpack_feedback)
        r = neeat_exchange_feedback(c); if (r != PT_OK) return r;
        r = neeat_frame(c); if (r != PT_OK) return r;
    }
    return render_pixel_list(c, c->dOwned.p, (uint)c->owned.size(), first, count, c->accumCount, nullptr, stats);
}

} // extern "C"

// The frame both reference-mode entry points share: everything of it — pool, batches, vertex-0 packets, compacted pool, fused traversal, tail kernel — runs on whatever
// count the list has. With a round, k_adaptive_accumulate replaces k_accumulate and the round's evaluation follows it.
int32_t render_pixel_list(pt_context* c, const uint* pixels, uint numPixels, uint32_t first, uint32_t count, uint accumBase, AdaptiveRound* round, PtFrameStats* stats) {
    int r = PT_OK;
    if ((unsigned long long)numPixels * count > 0xF0000000ull) return fail(c, PT_ERROR_INVALID_ARGUMENT, "too many paths in one pt_render call");
    const uint total = numPixels * count;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (total == 0) { if (!round) c->accumCount += count; return PT_OK; }
    // min(RTXPT_LIGHTING_MAX_SAMPLE_COUNT, NEEFullSamples), PathTracerNEE.hlsli:312
    const uint neeSamples = c->S.NEEFullSamples < 63u ? c->S.NEEFullSamples : 63u;
    // 0: one shadow-queue entry per path vertex, written by k_shade itself
    const uint shadowGroup = (c->S.NEEEnabled && neeSamples > 1u) ? neeSamples : 0u;
    const uint shadowPerPath = shadowGroup ? shadowGroup : 1u;
    r = ensure_pool(c, total, shadowPerPath); if (r != PT_OK) return r;
    const bool feedback = c->feedbackRequired && c->S.NEEEnabled && neeSamples != 0u;
    r = prepare_neeat_layers(c, count, feedback, shadowGroup); if (r != PT_OK) return r;
    PathKernelContext k = kernel_context(c);
    // `applyNEE &= fullSamples > 0` (PathTracerNEE.hlsli:322): the vertices behave as without NEE; the light tables stay as baked
    if (neeSamples == 0u) k.S.NEEEnabled = 0;

    RenderFrame f{c, first, count, total, shadowGroup, shadowPerPath, feedback, pixels, numPixels, accumBase, round};
    r = f.setup(k); if (r != PT_OK) return r;
    // uploads issued on the main stream (prepare) must be visible to the other streams
    if (f.numBatches > 1) PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    Events frame; PT_CHECK_HIP(c, frame.record(c->stream));
    r = f.start(); if (r != PT_OK) return r;
    r = f.lockstep(); if (r != PT_OK) return r;
    r = f.free_run(); if (r != PT_OK) return r;
    f.accumulate();
    Events evalMarks; size_t e0 = 0, e1 = 0;
    if (round && round->evaluate) { r = f.evaluate(evalMarks, e0, e1); if (r != PT_OK) return r; }
    r = drain_frame(c, f.B, f.numBatches, frame); if (r != PT_OK) return r;
    if (round) round->errorPassMs = round->evaluate ? evalMarks.ms(e0, e1) : 0.0f;
    else c->accumCount += count;
    if (feedback) c->fbSamples = count;
    if (stats) f.harvest(*stats, frame.ms());
    c->droppedTerminal = 0; for (uint b = 0; b < f.numBatches; b++) c->droppedTerminal += f.B[b].hwc->droppedTerminal;
    if (f.passLog) f.log_passes();
    return check_frame_end(c, f.B, f.numBatches,
                           "pt_render: paths still alive at the pass bound (bounceCount + 2 + the nested-dielectric allowance): the bound must be raised");
}

extern "C" {

int32_t pt_build_stable_planes(pt_context* c, uint32_t sampleIndex, const PtStablePlanesParams* params, PtFrameStats* stats) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    if (stats) memset(stats, 0, sizeof(*stats));
    const uint numOwned = (uint)c->owned.size();
    r = ensure_pool(c, numOwned ? numOwned : 1u, 1u); if (r != PT_OK) return r;
    r = ensure_stable_planes(c, ptk::GenericTSComputePlaneStride(c->width, c->height)); if (r != PT_OK) return r;
    const StablePlanesContext sp = sp_context(c, params);
    c->spGathered = false; c->spSampleBase = sampleIndex; c->dnPreparedPlane = -1; c->spFrameSerial++;      // a new frame: no plane of it is prepared for the denoiser yet
    if (!numOwned) return PT_OK;
    PathKernelContext k = kernel_context(c);
    // a batch of one, but on the context's main stream: what later calls synchronise with
    Batch t; slice_batch(c, k, numOwned, 0u, 1u, 1u, 1u, frame_shadow_queue(c, 0u), 0u, t);
    t.st = c->stream; t.hwc->extendCount[0] = t.active = t.total;
    Events frame; PT_CHECK_HIP(c, frame.record(t.st));
    PT_CHECK_HIP(c, hipMemcpyAsync(t.wc, t.hwc, sizeof(WaveCounters), hipMemcpyHostToDevice, t.st));
    launch_sp_generate(k, sp, t.pool, c->dOwned.p, numOwned, sampleIndex, t.queue[0], t.st);
    // every pass is one vertex of every pixel that still explores: at most three planes of at most maxStablePlaneVertexDepth + 1 vertices,
    // plus the false hits nested dielectrics reject (quality 1: its four at every vertex; quality 2: sixteen per plane)
    const uint depth = sp.C.maxStablePlaneVertexDepth, rejects = nested_dielectric_allowance(c->S);
    const uint maxIter = cStablePlaneCount * (depth + 2u + (c->S.nestedDielectricsQuality == 1 ? rejects * (depth + 1u) : rejects));
    r = build_passes(c, sp, sampleIndex, maxIter, t); if (r != PT_OK) return r;
    PT_CHECK_HIP(c, frame.record(t.st));
    PT_CHECK_HIP(c, hipMemcpyAsync(t.hwc, t.wc, sizeof(WaveCounters), hipMemcpyDeviceToHost, t.st));
    PT_CHECK_HIP(c, hipStreamSynchronize(t.st));
    PT_CHECK_HIP(c, hipGetLastError());
    if (stats) { *stats = batch_stats(t, 0u); stats->gpuMilliseconds = frame.ms(); }
    return check_frame_end(c, &t, 1u, "stable-plane build pass: paths still exploring after the iteration bound");
}

int32_t pt_fill_stable_planes(pt_context* c, uint32_t sampleIndex, const PtStablePlanesParams* params, PtFrameStats* stats) {
    if (!c || !params) return PT_ERROR_INVALID_ARGUMENT;
    if (!c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    if (!c->spW || c->spW != c->width || c->spH != c->height)
        return fail(c, PT_ERROR_NOT_READY, "no stable planes of this frame size yet: pt_build_stable_planes first");
    if (c->S.NEEEnabled && c->S.NEEFullSamples > 1u)
        return fail(c, PT_ERROR_INVALID_ARGUMENT, "the fill pass traces one full NEE sample per vertex (NEEFullSamples 0 or 1, the reference's default)");
    // temporal feedback: with the baker in the loop (pt_set_neeat + pt_realtime_frame) the pass's visible light samples fill the run's
    // reservoirs; a host that runs its own baker (pt_set_local_light_sampling with temporalFeedback) gets its per-sample planes from pt_render
    // only
    const bool feedback = c->neeat.enabled && c->feedbackRequired && c->S.NEEEnabled && c->S.NEEFullSamples != 0u;
    if (c->feedbackRequired && !c->neeat.enabled)
        return fail(c, PT_ERROR_INVALID_ARGUMENT, "the fill pass feeds NEE-AT's reservoirs only with the baker in the loop (pt_set_neeat, pt_realtime_frame): "
                                                  "switch the temporal feedback of pt_set_local_light_sampling off");
    if (feedback && (!c->neeat.fbW.p || c->neeat.W != c->width || c->neeat.H != c->height))
        return fail(c, PT_ERROR_NOT_READY, "NEE-AT: no baker frame of this size yet (pt_realtime_frame runs it)");
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    if (stats) memset(stats, 0, sizeof(*stats));
    const uint numOwned = (uint)c->owned.size();
    if (!numOwned) return PT_OK;
    r = ensure_pool(c, numOwned, 1u); if (r != PT_OK) return r;
    const bool freshMark = c->dSpMark.n < numOwned;
    PT_CHECK_HIP(c, c->dSpMark.resize(numOwned)); PT_CHECK_HIP(c, c->dSpNewL.resize(numOwned));
    if (feedback) PT_CHECK_HIP(c, c->dSq3.resize(c->shadowCapacity));
    // (k_sp_fill_resolve clears what a pass marked)
    if (freshMark) PT_CHECK_HIP(c, hipMemsetAsync(c->dSpMark.p, 0, sizeof(ptk::uint4) * c->dSpMark.n, c->stream));
    PathKernelContext k = kernel_context(c);
    FillFrame f{c, sp_context(c, params), sampleIndex, feedback};
    f.setup(k);
    // uploads / memsets issued on the main stream (prepare, the marks) must be visible to the batch streams
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    Events frame; PT_CHECK_HIP(c, frame.record(c->stream));
    r = f.start(); if (r != PT_OK) return r;
    r = f.lockstep(); if (r != PT_OK) return r;
    f.commit();
    r = drain_frame(c, f.B, f.numBatches, frame); if (r != PT_OK) return r;
    if (stats) {
        for (uint b = 0; b < f.numBatches; b++) add_frame_stats(*stats, batch_stats(f.B[b], 0u));
        stats->gpuMilliseconds = frame.ms();
    }
    return check_frame_end(c, f.B, f.numBatches, "stable-plane fill pass: paths still alive after the iteration bound");
}

} // extern "C"

// mi355pt — wavefront kernels, the path-state half: generate / classify / shade / uncompact / accumulate (the traversal launches: pt_trace.hip; the bake passes: pt_bake.hip).
// The reference runs all of this as ONE DXR dispatch, one thread per pixel looping over bounces
// (Rtxpt/Shaders/PathTracerSample.hlsl:200-250) and relies on SER to re-sort threads (:136-148). Here each stage is its own
// kernel over a compacted queue, so every wave starts full regardless of how many paths died in the previous bounce.
#include "pt_wavefront.h"
#include "pt_wavefront_device.h"
#include <type_traits>

namespace ptk {

// Paths [first, first + n) of the batch's pool region (slot i = sample i % spp of owned pixel i / spp) are generated and their indices written to queue[0 ..
// n).
__global__ void __launch_bounds__(256) k_generate(PathKernelContext k, PathPool pool, const uint* __restrict__ ownedPixels, uint numOwned, uint sampleFirst, uint spp, uint first, uint n, uint* __restrict__ queue, uint* countPtr) {
    const uint t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const uint i = first + t;
    uint px, sample; first_vertex_of(FirstVertex{ownedPixels, numOwned, sampleFirst, spp}, i, px, sample);
    PathState p = k.generate(px >> 16, px & 0xFFFFu, sample);
    store_path(pool, i, p);
    queue[t] = i;
    if (countPtr && t == 0u) atomicAdd(countPtr, n);
}

#ifndef PT_SHADE_BLOCK
#define PT_SHADE_BLOCK 256       // threads per k_shade block (the queue appends meet per block: one atomic per block and counter)
#endif
#ifndef PT_SHADE_MIN_BLOCKS
#define PT_SHADE_MIN_BLOCKS 1
#endif
#ifndef PT_SHADE_PROBE
#define PT_SHADE_PROBE 0
#endif
#ifndef PT_SHADE_CLASSES
#define PT_SHADE_CLASSES 1      // 1: k_classify sorts the bounce's paths into {hit that goes on, hit that terminates after its emission, miss} before k_shade
#endif

// Path classes for k_shade. A shading wave lives ~90 us, nearly all of it waiting on dependent loads, and as long as ONE lane runs the whole of HandleHit
// (surface, scatter, light sampling) the wave stays for all of it — while 13 % of a bounce's paths are misses and ~20 % are hits that terminate right after
// their emission term (PF_terminateAtNextBounce). k_classify makes the classes contiguous (continuing hits from the front of one array, terminating hits from
// its back, misses in a second one; one atomic per class per 1024 paths), so all but two waves of a launch are of one class and the short classes leave early.
// Radiance, queues and counters do not depend on the order in which paths are shaded.
// paths per thread: 4096 per block, one atomic per class and block (with 1024 per block the 32 000 blocks of a 4K bounce spent 0.3 ms queueing on three L2
// lines)
// UNIFORM: every path of the launch carries the flags word `uniformFlags` — vertex 0, where it follows from the settings alone (PathKernelContextT::generateState) and pool.s4
// may not have been written (FirstVertex): only the hit's primitive is read
// DROP (pt_render, not vertex 0): the fourth outcome — a terminating hit that is INERT is written into no class and counted in classCount[3]. Such a vertex exists for its
// emission term alone (HandleHit, pt_path.h: loadSurface<LEAN>, the nested-dielectric check, the emission and the analytic-light-proxy terms, path.terminate()), and on a
// primitive whose material can neither emit nor stand in for a light, and whose hit the nested-dielectric check cannot reject (inert_when_terminal, pt_scene.h: quality 0
// or a thin surface), it adds no radiance and ends the path. Why the image cannot change when k_shade never sees it:
//  - the only stores the vertex would make are the path's own state, which nothing reads again — the path is not appended to the next queue, and the tail kernel, k_uncompact
//    and the next pass read the pool through that queue — and s2[home], whose radiance words would be rewritten with the value they hold (k_accumulate and the visibility
//    resolve read those; the throughput words, which volumeTransmittance may scale, die with the path like the ray cone and the scene length);
//  - no random number is drawn, no queue entry is made, and no counter but the hit count depends on it: k_shade adds classCount[3] to WaveCounters::hits.
// The launcher asks for it only where nothing else observes a terminal hit: no NEE-AT instantiation (ExportSurface writes a depth for every hit) and not the stable-plane
// fill pass, which has its own shading kernel. The lane reads the table only once it knows it is a terminating hit: both words it needs for that are loaded anyway.
#define PT_CLASSIFY_ITEMS 4u
template <bool UNIFORM = false, bool DROP = false>
__global__ void __launch_bounds__(1024) k_classify(PathPool pool, const uint* __restrict__ queueIn, const uint* __restrict__ countInPtr, uint* __restrict__ classQ, uint* __restrict__ classCount, uint uniformFlags,
                                                   const uint* __restrict__ inertBits, uint nestedDielectricsQuality) {
    static_assert(!(UNIFORM && DROP), "vertex 0 has no terminating paths");
    __shared__ uint waveCnt[PT_CLASSIFY_ITEMS][16][4]; __shared__ uint blockBase[3];
    const uint count = *countInPtr, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    // cls: 0 continuing hit, 1 terminating hit, 2 miss, 3 terminating hit that is dropped, 4 out of range
    uint p[PT_CLASSIFY_ITEMS], cls[PT_CLASSIFY_ITEMS]; unsigned long long mine[PT_CLASSIFY_ITEMS];
#pragma unroll
    for (uint j = 0; j < PT_CLASSIFY_ITEMS; j++) {
        const uint i = (blockIdx.x * PT_CLASSIFY_ITEMS + j) * 1024u + threadIdx.x;
        p[j] = 0u; cls[j] = 4u;
        if (i < count) {
            p[j] = pool.home ? i : queueIn[i];
            const uint prim = reinterpret_cast<const uint*>(pool.hit)[4u * (size_t)p[j] + 1u], flags = UNIFORM ? uniformFlags : reinterpret_cast<const uint*>(pool.s4)[4u * (size_t)p[j] + 2u];
            cls[j] = (prim == 0xFFFFFFFFu) ? 2u : (((flags >> kVertexIndexBitCount) & PF_terminateAtNextBounce) ? 1u : 0u);
            if (DROP && cls[j] == 1u && inert_when_terminal(inert_bits_at(inertBits, prim), nestedDielectricsQuality)) cls[j] = 3u;
        }
        const unsigned long long m0 = __builtin_amdgcn_ballot_w64(cls[j] == 0u), m1 = __builtin_amdgcn_ballot_w64(cls[j] == 1u), m2 = __builtin_amdgcn_ballot_w64(cls[j] == 2u);
        if (lane == 0u) { waveCnt[j][wave][0] = (uint)__popcll(m0); waveCnt[j][wave][1] = (uint)__popcll(m1); waveCnt[j][wave][2] = (uint)__popcll(m2); }
        if (DROP) { const unsigned long long m3 = __builtin_amdgcn_ballot_w64(cls[j] == 3u); if (lane == 0u) waveCnt[j][wave][3] = (uint)__popcll(m3); }
        mine[j] = cls[j] == 0u ? m0 : (cls[j] == 1u ? m1 : m2);
    }
    __syncthreads();
    if (threadIdx.x < 3u) {      // exclusive prefix over (item, wave) in queue order, then the block's base
        uint tot = 0;
        for (uint j = 0; j < PT_CLASSIFY_ITEMS; j++) for (uint w = 0; w < 16u; w++) { const uint c = waveCnt[j][w][threadIdx.x]; waveCnt[j][w][threadIdx.x] = tot; tot += c; }
        blockBase[threadIdx.x] = tot ? atomicAdd(&classCount[threadIdx.x], tot) : 0u;
    } else if (DROP && threadIdx.x == 3u) {      // the dropped hits: a count, no place
        uint tot = 0;
        for (uint j = 0; j < PT_CLASSIFY_ITEMS; j++) for (uint w = 0; w < 16u; w++) tot += waveCnt[j][w][3];
        if (tot) atomicAdd(&classCount[3], tot);
    }
    __syncthreads();
#pragma unroll
    for (uint j = 0; j < PT_CLASSIFY_ITEMS; j++) {
        if (cls[j] > 2u) continue;
        const uint rank = blockBase[cls[j]] + waveCnt[j][wave][cls[j]] + (uint)__popcll(mine[j] & ((1ull << lane) - 1ull));
        // continuing hits from the front of [0, count), terminating hits from its back (they cannot meet: together they are at most count), misses in [count, 2
        // count)
        classQ[cls[j] == 0u ? rank : (cls[j] == 1u ? count - 1u - rank : count + rank)] = p[j];
    }
}

// PKC: PathKernelContextT<false> (lp types in fp32) or PathKernelContextT<true> (the reference's default build, lp types in binary16)
// COMPACT: the pool is compacted (PathPool::home): the path at position p of this bounce's array set is written, if it survives, to the position it is appended at in `outPool`'s set;
// its throughput | radiance word group stays at its home slot, which is also what the extend queue keeps and the shadow queue names
// FIRST (with COMPACT): vertex 0 of paths that were not generated (FirstVertex fv): the state is formed, not loaded (PathFirstVertexIO); position == home slot, pool.home is not read
template <bool MULTI, class PKC, bool NEEAT, bool COMPACT = false, bool FIRST = false>
__global__ void __launch_bounds__(PT_SHADE_BLOCK, PT_SHADE_MIN_BLOCKS) k_shade(PKC k, PathPool pool, const uint* __restrict__ queueIn, const uint* __restrict__ countInPtr,
                                               uint* __restrict__ queueOut, uint* countOutPtr, ShadowQueue sq, WaveCounters* wc, const uint* __restrict__ classCount, PathPool outPool, FirstVertex fv) {
    static_assert(!FIRST || (COMPACT && !MULTI && !NEEAT), "vertex 0 in place: the compacted pool of a composed frame");
    static_assert(!COMPACT || !PT_SHADE_PROBE, "the PT_SHADE_PROBE timing builds do not know the compacted pool: take the COMPACT launch out of launch_shade and run with MI355PT_COMPACT_POOL=0");
    const uint count = *countInPtr;
    uint i = blockIdx.x * (uint)PT_SHADE_BLOCK + threadIdx.x;
    bool inRange = i < count;
    bool alive = false; bool isHit = false; uint p = 0, hp = 0;
    ShadowRequest req; req.valid = false;
    PathState cpath;      // COMPACT: the shaded path, kept until its position is known
    if (COMPACT) __builtin_memset(&cpath, 0, sizeof(cpath));
    if (inRange) {
        // queueIn = k_classify's arrays: thread i takes the i-th path of the order {continuing, terminating, miss}
        if (classCount) {
            const uint nGo = classCount[0], nEnd = classCount[1];
            inRange = i < nGo + nEnd + classCount[2];      // fewer than `count` where k_classify dropped inert terminal hits: those threads leave here
            p = inRange ? queueIn[i < nGo ? i : (i < nGo + nEnd ? count - 1u - (i - nGo) : count + (i - nGo - nEnd))] : 0u;
        } else p = COMPACT ? i : queueIn[i];
    }
    if (inRange) {
        hp = (COMPACT && !FIRST) ? pool.home[p] : p;
        uint4 hr = pool.hit[p];
        HitInfo h; h.t = asfloat(hr.x); h.prim = hr.y; h.u = asfloat(hr.z); h.v = asfloat(hr.w);
#if PT_SHADE_PROBE
        PathState path = load_path(pool, p);
#if PT_SHADE_PROBE == 1          // timing probes (developer builds only, the image is wrong by design): 1 = stream the path state through, nothing else
        if (h.prim != 0xFFFFFFFFu) { isHit = true; path.sceneLength += h.t; } path.terminate();
#elif PT_SHADE_PROBE == 2        // 2 = the surface gather (record, instance, material, textures) and nothing after it
        if (h.prim != 0xFFFFFFFFu) { isHit = true; SurfaceData sfd = k.loadSurface(h.prim, h.u, h.v, path.dir, path.rayCone); path.origin = sfd.shadingData.posW + sfd.shadingData.N * sfd.bsdf.data.roughness + sfd.bsdf.data.diffuse + sfd.shadingData.T; } path.terminate();
#endif
        store_path(pool, p, path);
        alive = path.isActive();
#else
        if (COMPACT && FIRST) {
            uint px, sample; first_vertex_of(fv, p, px, sample);
            const PathFirstVertexIO<PKC> io{k, px, sample};
            if (h.prim == 0xFFFFFFFFu) { cpath = io.load_all(); k.template HandleMiss<NEEAT>(cpath, cpath.dir, kMaxRayTravel); }
            else { isHit = true; cpath = io.load_first(); k.template HandleHit<false, NEEAT>(cpath, h, req, nullptr, io); }
            alive = cpath.isActive();
            pool.s2[hp] = make_uint4(cpath.pack23[0], cpath.pack23[1], cpath.pack45[0], cpath.pack45[1]);      // every home slot's throughput | radiance is written here before anything reads it
        }
        else if (COMPACT) {
            const PathCompactIO io{pool, p, hp};
            if (h.prim == 0xFFFFFFFFu) { cpath = io.load_all(); k.template HandleMiss<NEEAT>(cpath, cpath.dir, kMaxRayTravel); }
            else { isHit = true; cpath = io.load_first(); k.template HandleHit<false, NEEAT>(cpath, h, req, nullptr, io); }
            alive = cpath.isActive();
            pool.s2[hp] = make_uint4(cpath.pack23[0], cpath.pack23[1], cpath.pack45[0], cpath.pack45[1]);      // throughput | radiance: at home, alive or not
        }
        else if (h.prim == 0xFFFFFFFFu) { PathState path = load_path(pool, p); k.template HandleMiss<NEEAT>(path, path.dir, kMaxRayTravel); store_path(pool, p, path); alive = path.isActive(); }
        else {
            isHit = true;
            const PathPoolIO io{pool, p};      // the path streams through HandleHit: late loads, early stores (pt_wavefront_device.h)
            PathState path = io.load_first();
            if (MULTI) { ShadowSink sink{sq.q0, sq.q1, sq.q2, &wc->shadowCount, &wc->shadowValid, p}; k.template HandleHit<true, NEEAT>(path, h, req, &sink, io); }
            else k.template HandleHit<false, NEEAT>(path, h, req, nullptr, io);
            alive = path.isActive();
#ifdef PT_SHADE_PHASE_PROBE
            for (int q = 1; q < 6; q++) wave_add64(io.tk[q] ? (unsigned long long)(uint)(io.tk[q] - io.tk[q - 1 - (io.tk[q - 1] ? 0 : 1)]) : 0ull, &wc->eventsExt[q - 1]);      // (a vertex that returns early leaves later stamps at 0)
#endif
        }
#endif
    }
    // Queue appends, one atomic per BLOCK and counter: the four waves' counts meet in LDS, thread 0 reserves both ranges. A launch of 33 M paths has 518 k
    // waves; one returning atomic per wave on each of three words — all waves of the GPU on the same three addresses — is what the kernel waited for
    // (same-address atomics serialise in the L2: ~10^8 per second and address). The hit count needs no atomic at all when the paths were classified: it is the
    // size of two classes.
    __shared__ uint sCnt[PT_SHADE_BLOCK / 64][2]; __shared__ uint sBase[2];
    const uint wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const unsigned long long mAlive = __builtin_amdgcn_ballot_w64(alive), mReq = __builtin_amdgcn_ballot_w64(!MULTI && req.valid);
    if (lane == 0u) { sCnt[wave][0] = (uint)__popcll(mAlive); sCnt[wave][1] = (uint)__popcll(mReq); }
    __syncthreads();
    if (threadIdx.x < 2u) {
        uint tot = 0; for (uint w = 0; w < (uint)(PT_SHADE_BLOCK / 64); w++) { const uint c = sCnt[w][threadIdx.x]; sCnt[w][threadIdx.x] = tot; tot += c; }
        sBase[threadIdx.x] = tot ? atomicAdd(threadIdx.x == 0u ? countOutPtr : &wc->shadowCount, tot) : 0u;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    if (alive) {
        const uint slot = sBase[0] + sCnt[wave][0] + (uint)__popcll(mAlive & below);
        queueOut[slot] = hp;
        if (COMPACT) {      // the survivor's state at its new position, in the other array set
            outPool.s0[slot] = make_uint4(asuint(cpath.origin.x), asuint(cpath.origin.y), asuint(cpath.origin.z), cpath.id);
            outPool.s1[slot] = make_uint4(asuint(cpath.dir.x), asuint(cpath.dir.y), asuint(cpath.dir.z), asuint(cpath.sceneLength));
            outPool.s3[slot] = make_uint4(cpath.interiorList.slots[0], cpath.interiorList.slots[1], cpath.packedCounters, cpath.rayCone.widthSpreadAngleFP16);
            outPool.s4[slot] = make_uint4(cpath.pack0, cpath.pack1, cpath.flagsAndVertexIndex, cpath.sampleIndex);
        }
    }
    if (!MULTI && req.valid) {
        const uint sslot = sBase[1] + sCnt[wave][1] + (uint)__popcll(mReq & below);
        sq.q0[sslot] = make_float4(req.origin.x, req.origin.y, req.origin.z, req.tmax);
        sq.q1[sslot] = make_float4(req.dir.x, req.dir.y, req.dir.z, asfloat(hp));
        sq.q2[sslot] = make_float4(req.radiance.x, req.radiance.y, req.radiance.z, 0.f);
        if (NEEAT && sq.q3) sq.q3[sslot] = make_float4(req.fbWeight, req.fbRandom, asfloat(req.fbLight), asfloat(req.rrFix));
    }
    if (classCount) {      // (classCount[3]: the terminating hits k_classify dropped — hits all the same)
        if (blockIdx.x == 0u && threadIdx.x == 0u) { const uint nDropped = classCount[3]; atomicAdd(&wc->hits, ((unsigned long long)classCount[0] + classCount[1]) + nDropped); if (nDropped) atomicAdd(&wc->droppedTerminal, (unsigned long long)nDropped); }
    }
    else wave_add64(isHit ? 1ull : 0ull, &wc->hits);
}

__global__ void __launch_bounds__(256) k_accumulate(PathPool pool, const uint* __restrict__ ownedPixels, uint numOwned, uint spp, float4* __restrict__ accum, uint accumCountBase, uint width) {
    uint kpx = blockIdx.x * 256u + threadIdx.x;
    if (kpx >= numOwned) return;
    uint px = ownedPixels[kpx];
    uint addr = (px & 0xFFFFu) * width + (px >> 16);
    float4 acc = accum[addr];
    for (uint s = 0; s < spp; s++) {
        uint4 c = pool.s2[PT_SAMPLE_MINOR ? kpx * spp + s : s * numOwned + kpx];
        float2 l0 = Fp16ToFp32(c.z), l1 = Fp16ToFp32(c.w);
        float4 col = make_float4(l0.x, l0.y, l1.x, 1.0f);
        float blend = 1.0f / (float)(accumCountBase + s + 1u);
        acc = (blend < 1.f) ? lerp4(acc, col, blend) : col;
    }
    accum[addr] = acc;
}

void launch_generate(const PathKernelContext& k, PathPool pool, const uint* ownedPixels, uint numOwned, uint sampleFirst, uint spp, uint first, uint n, uint* queue, uint* countPtr, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_generate, dim3((n + 255) / 256), dim3(256), 0, st, k, pool, ownedPixels, numOwned, sampleFirst, spp, first, n, queue, countPtr);
}
// k_classify for a caller in another translation unit (the stable-plane fill pass): classScratch 2 x countIn words, classCount 3 words (zero on entry)
void launch_classify(PathPool pool, const uint* queueIn, const uint* countInPtr, uint countIn, uint* classScratch, uint* classCount, hipStream_t st) {
    hipLaunchKernelGGL((k_classify<false>), dim3((countIn + 1024u * PT_CLASSIFY_ITEMS - 1u) / (1024u * PT_CLASSIFY_ITEMS)), dim3(1024), 0, st, pool, queueIn, countInPtr, classScratch, classCount, 0u, (const uint*)nullptr, 0u);
}
void launch_shade(const PathKernelContext& k, PathPool pool, const uint* queueIn, const uint* countInPtr, uint countIn, uint* queueOut, uint* countOutPtr, ShadowQueue sq, WaveCounters* wc,
                  uint* classScratch, uint* classCount, hipStream_t st, PathPool outPool, const FirstVertex* fv, const uint* inertBits) {
    const FirstVertex fv0 = fv ? *fv : FirstVertex{nullptr, 0u, 0u, 0u};
    const dim3 g((countIn + PT_SHADE_BLOCK - 1) / PT_SHADE_BLOCK), b(PT_SHADE_BLOCK);
    // NEE-AT (a local sampling table and / or temporal feedback, pt_set_local_light_sampling) runs its own instantiations: the frames without it keep their
    // kernels unchanged
    const bool neeat = k.sc.lights.LocalSamplingBuffer != nullptr || k.sc.lights.TemporalFeedbackRequired != 0u;
    // (scratch: 2 x countIn words, free between the extend and the shadow launches; classCount: 3 words, zeroed with the pass's traversal counters)
    if (PT_SHADE_CLASSES && classScratch) {
        const dim3 cg((countIn + 1024u * PT_CLASSIFY_ITEMS - 1u) / (1024u * PT_CLASSIFY_ITEMS));
        // (vertex 0 in place: the flags word every path would have been generated with)
        // (inert terminal hits are dropped only where nothing else observes a hit: the NEE-AT instantiations export a depth per hit)
        const bool drop = inertBits && !neeat && k.sc.lights.DepthExport == nullptr;
        if (fv) hipLaunchKernelGGL((k_classify<true>), cg, dim3(1024), 0, st, pool, queueIn, countInPtr, classScratch, classCount, k.generateState(0u, 0u, 0u).flagsAndVertexIndex, (const uint*)nullptr, 0u);
        else if (drop) hipLaunchKernelGGL((k_classify<false, true>), cg, dim3(1024), 0, st, pool, queueIn, countInPtr, classScratch, classCount, 0u, inertBits, (uint)k.S.nestedDielectricsQuality);
        else hipLaunchKernelGGL((k_classify<false>), cg, dim3(1024), 0, st, pool, queueIn, countInPtr, classScratch, classCount, 0u, (const uint*)nullptr, 0u);
        queueIn = classScratch;
    } else classCount = nullptr;
#define PT_LAUNCH_SHADE(MULTI, PKC, CTX) do { if (neeat) hipLaunchKernelGGL((k_shade<MULTI, PKC, true>), g, b, 0, st, CTX, pool, queueIn, countInPtr, queueOut, countOutPtr, sq, wc, classCount, outPool, fv0); \
                                              else if (pool.home && !MULTI && fv) hipLaunchKernelGGL((k_shade<false, PKC, false, true, true>), g, b, 0, st, CTX, pool, queueIn, countInPtr, queueOut, countOutPtr, sq, wc, classCount, outPool, fv0); \
                                              else if (pool.home && !MULTI) hipLaunchKernelGGL((k_shade<false, PKC, false, true>), g, b, 0, st, CTX, pool, queueIn, countInPtr, queueOut, countOutPtr, sq, wc, classCount, outPool, fv0); \
                                              else hipLaunchKernelGGL((k_shade<MULTI, PKC, false>), g, b, 0, st, CTX, pool, queueIn, countInPtr, queueOut, countOutPtr, sq, wc, classCount, outPool, fv0); } while (0)
    if (stf_launch_filter(k.S) != STF_OFF) {      // a stochastic texture filter (pt_set_texture_filtering): the same launches over that context's instantiations
        dispatch_stf(k, [&](const auto& c) { typedef typename std::decay<decltype(c)>::type PKC; if (sq.group) PT_LAUNCH_SHADE(true, PKC, c); else PT_LAUNCH_SHADE(false, PKC, c); });
    } else if (k.S.useFp16Types) {          // the reference's default build of its lp types (binary16): same context data, the other instantiation of the shading code
        static_assert(sizeof(PathKernelContextT<true>) == sizeof(PathKernelContext), "the two lp builds share one context layout");
        PathKernelContextT<true> k16; __builtin_memcpy(&k16, &k, sizeof(k16));
        if (sq.group) PT_LAUNCH_SHADE(true, PathKernelContextT<true>, k16); else PT_LAUNCH_SHADE(false, PathKernelContextT<true>, k16);
    } else {
        if (sq.group) PT_LAUNCH_SHADE(true, PathKernelContext, k); else PT_LAUNCH_SHADE(false, PathKernelContext, k);
    }
#undef PT_LAUNCH_SHADE
}
// start of a pass: the batch's PASS_COUNTERS words and the two queue counters the pass refills, zeroed by one launch (three memsets were three launches)
__global__ void __launch_bounds__(64) k_pass_begin(uint* __restrict__ passCounters, uint* __restrict__ nextCount, uint* __restrict__ shadowCount) {
    if (threadIdx.x < PASS_COUNTERS) passCounters[threadIdx.x] = 0u;
    if (threadIdx.x == 32u) *nextCount = 0u;
    if (threadIdx.x == 33u && shadowCount) *shadowCount = 0u;      // (null: a frame of fused traversal launches, whose k_resolve_pair zeroes it)
}
void launch_pass_reset(uint* passCounters, uint* nextCount, uint* shadowCount, hipStream_t st) { static_assert(PASS_COUNTERS <= 32u, "k_pass_begin"); hipLaunchKernelGGL(k_pass_begin, dim3(1), dim3(64), 0, st, passCounters, nextCount, shadowCount); }
__global__ void __launch_bounds__(256) k_uncompact(PathPool in, PathPool out, const uint* __restrict__ countPtr) {
    const uint i = blockIdx.x * 256u + threadIdx.x;
    if (i >= *countPtr) return;
    const uint hp = in.home[i];
    out.s0[hp] = in.s0[i]; out.s1[hp] = in.s1[i]; out.s3[hp] = in.s3[i]; out.s4[hp] = in.s4[i];
}
void launch_uncompact(PathPool in, PathPool out, const uint* countPtr, uint count, hipStream_t st) {
    if (count) hipLaunchKernelGGL(k_uncompact, dim3((count + 255u) / 256u), dim3(256), 0, st, in, out, countPtr);
}
void launch_accumulate(PathPool pool, const uint* ownedPixels, uint numOwned, uint spp, float4* accum, uint accumCountBase, uint width, hipStream_t st) {
    hipLaunchKernelGGL(k_accumulate, dim3((numOwned + 255) / 256), dim3(256), 0, st, pool, ownedPixels, numOwned, spp, accum, accumCountBase, width);
}

} // namespace ptk

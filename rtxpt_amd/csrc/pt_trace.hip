// mi355pt — the BVH8 traversal launches: extend / shadow / the fused pair, vertex 0 in place and as packets, the task rounds and resolve passes behind them, the trace probe.
// Every kernel here is an instantiation of traverse8_pairs, traverse8_packets or traverse8_packets64 (pt_traverse8*.h) or reads what one left; the launchers take their grids
// from pt_trace_plan.h.
#include "pt_trace_device.h"
#include <type_traits>

namespace ptk {
// The closest-hit launch of a bounce (Bridge::traceScatterRay for every path of the extend queue) as a device function, so that two kernels can run it:
// k_extend, and k_trace_pair next to the visibility rays of the previous vertex. vBlock / vGrid: this block's place among the blocks that work on the extend
// queue (traverse8_pairs).
// FIRST: the first pass of a batch whose paths were not generated (FirstVertex, pt_wavefront.h): ray i is the camera ray of path i, formed at the chunk refill from the owned
// pixel and the sample index — no queue, no stored ray. The rays that end up cut into sub-trees (thousands of a launch, not millions) are on the resolve list: k_first_split_rays
// writes their origin | id and direction | length to pool.s0 / s1 behind the launch, where the task rounds and the resolve pass read them as in every other pass.
// LISTED (with FIRST): ray i of the launch is the camera ray of path queue[i] — the rays the packet launch left over (k_extend_first_packets).
template <bool COUNT, bool RANGED, bool FIRST = false, bool LISTED = false>
__device__ __forceinline__ void t8_extend_body(const DeviceScene& sc, const PathPool& pool, const uint* __restrict__ queue, const uint count, WaveCounters* wc, const TravAux& aux, const uint rpc,
                                               uint2* stack, uint* rayBuf, float2* mineUV, const uint vBlock, const uint vGrid, const FirstVertex* fv = nullptr) {
    static_assert(!FIRST || (!COUNT && !RANGED), "vertex 0 in place: composed frames only");
    static_assert(!LISTED || FIRST, "an index list: vertex 0 in place only");
    // RANGED: every ray brings its own interval in the first two words of its (not yet written) hit record — the stable-plane fill pass's first launch,
    // FirstHitFromVBuffer (pt_stableplanes.h firstHitInterval). A ray of such a launch that is cut into sub-trees continues over [0, best hit so far]: the
    // lower bound is a hint, not part of the query.
    Traverse8Counters ctr; t8_counters_init(ctr);
    auto fetch = [&](uint i, float3& o, float3& d, float& tmin, float& tmax, uint& startRef, float& bestT0, uint& bestPrim0) -> uint {
        if (FIRST) {
            if (LISTED) i = queue[i];
            t8_camera_ray(wc, *fv, i, o, d);
            tmin = 0.0f; tmax = kMaxRayTravel; startRef = 0u; bestT0 = kMaxRayTravel; bestPrim0 = 0xFFFFFFFFu;
            return i;
        }
        uint p = pool.home ? i : queue[i];      // (a compacted pool's ray i is the path at position i)
        t8_stored_ray(pool, p, o, d);
        tmin = 0.0f; tmax = kMaxRayTravel; startRef = 0u; bestT0 = kMaxRayTravel; bestPrim0 = 0xFFFFFFFFu;
        if (RANGED) { const uint4 r = pool.hit[p]; tmin = asfloat(r.x); tmax = asfloat(r.y); bestT0 = tmax; }
        return p;
    };
    auto commit = [&](uint p, const HitInfo& h) { t8_store_hit(pool, p, h); };
    // a split ray: its best hit so far seeds the merge key, the resolve pass will write pool.hit (k_resolve_extend)
    auto publish = [&](uint p, float bestT, uint bestPrim) { aux.bestKey[p] = t8_hit_key(bestT, bestPrim); aux.resolveList[atomicAdd(&aux.counts[TRAV_RESOLVE], 1u)] = p; };
    if (COUNT) { ctr.rayIterHist = wc->rayIterHistExt; ctr.longRayCount = &wc->longRayCount; ctr.longRays = &wc->longRays[0][0]; }
    traverse8_pairs<false, COUNT, !RANGED, false, true>(sc, count, rpc, stack, rayBuf, mineUV, fetch, commit, publish, TravTaskOut{aux.taskQ[0], &aux.counts[0], aux.taskCap}, ctr, &wc->overflow, vBlock, vGrid);
    if (COUNT) { wave_add64(ctr.nodeVisits, &wc->nodeVisitsExt); wave_add64(ctr.triTests, &wc->triTestsExt); wave_add64(ctr.leafVisits, &wc->leafVisitsExt); wave_add64(ctr.iters, &wc->itersExt); wave_add64(ctr.leafBlocks, &wc->leafBlocksExt); if ((threadIdx.x & 63u) == 0u) atomicMax(&wc->itersMaxExt, (unsigned long long)ctr.iters);
                 if ((threadIdx.x & 63u) == 0u) for (int q = 0; q < 4; q++) atomicAdd(&wc->phaseCycExt[q], ctr.cyc[q]);
                 for (int q = 0; q < 8; q++) wave_add64(ctr.ev[q], &wc->eventsExt[q]); }
}
template <bool COUNT, bool RANGED = false>
__global__ void __launch_bounds__(T8_BLOCK, T8_EXTEND_MIN_BLOCKS) k_extend(DeviceScene sc, PathPool pool, const uint* __restrict__ queue, const uint* __restrict__ countPtr, WaveCounters* wc, TravAux aux, uint rpc) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_RAYBUF_WORDS];
    __shared__ float2 mineUV[T8_BLOCK];
    t8_extend_body<COUNT, RANGED>(sc, pool, queue, *countPtr, wc, aux, rpc, stack, rayBuf, mineUV, blockIdx.x, gridDim.x);
}

// k_extend<false> for vertex 0 in place: the batch's pixels instead of a queue
__global__ void __launch_bounds__(T8_BLOCK, T8_EXTEND_MIN_BLOCKS) k_extend_first(DeviceScene sc, PathPool pool, FirstVertex fv, const uint* __restrict__ countPtr, WaveCounters* wc, TravAux aux, uint rpc) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_RAYBUF_WORDS];
    __shared__ float2 mineUV[T8_BLOCK];
    t8_extend_body<false, false, true>(sc, pool, nullptr, *countPtr, wc, aux, rpc, stack, rayBuf, mineUV, blockIdx.x, gridDim.x, &fv);
}

// Vertex 0 as packets (pt_traverse8k.h): the 32 camera rays of a wave's packet — 32 consecutive paths: 8 x 1 pixels x 4 samples of an 8 x 8 block at 4 spp — walk the tree on one
// shared stack. Hits are committed by position like k_extend_first's; a packet over its step cap or stack bound commits nothing and leaves its rays on pk.leftover. No task queue,
// no resolve list: a wave walks its strided range of packets and ends.
__global__ void __launch_bounds__(T8_BLOCK, T8_EXTEND_MIN_BLOCKS) k_extend_first_packets(DeviceScene sc, PathPool pool, FirstVertex fv, const uint* __restrict__ countPtr, WaveCounters* wc, FirstPackets pk) {
    __shared__ uint2 stack[(T8_BLOCK / 64u) * T8_PACKET_STACK];
    __shared__ float2 mineUV[T8_BLOCK];
    traverse8_packets(sc, *countPtr, stack, mineUV, [&](uint i, float3& o, float3& d) { t8_camera_ray(wc, fv, i, o, d); }, [&](uint p, const HitInfo& h) { t8_store_hit(pool, p, h); }, pk, &wc->overflow);
}
// The same as 64-ray packets, one lane per ray (traverse8_packets64): 64 consecutive paths — two rows of an 8 x 8 block x 4 samples at 4 spp. The lane that holds a ray reports
// its hit, so there is no barycentrics parking lot; the wave's stack is all the LDS the kernel has.
// PRECULL: the node step culls its children against the packet's interval first (pk.precull; the wave's interval is sixteen more words of LDS)
template <bool PRECULL>
__global__ void __launch_bounds__(T8_BLOCK, T8_PACKET64_MIN_BLOCKS) k_extend_first_packets64(DeviceScene sc, PathPool pool, FirstVertex fv, const uint* __restrict__ countPtr, WaveCounters* wc, FirstPackets pk) {
    __shared__ uint2 stack[(T8_BLOCK / 64u) * T8_PACKET_STACK];
    __shared__ __attribute__((aligned(16))) float interval[PRECULL ? (T8_BLOCK / 64u) * T8_PACKET_INTERVAL_WORDS : 4u];
    traverse8_packets64<PRECULL>(sc, *countPtr, stack, interval, [&](uint i, float3& o, float3& d) { t8_camera_ray(wc, fv, i, o, d); }, [&](uint p, const HitInfo& h) { t8_store_hit(pool, p, h); }, pk, &wc->overflow);
}
// ... and the per-ray kernel over the rays the packets left over: k_extend_first reading i through the list (its count: what the packet launch appended)
__global__ void __launch_bounds__(T8_BLOCK, T8_EXTEND_MIN_BLOCKS) k_extend_first_listed(DeviceScene sc, PathPool pool, FirstVertex fv, FirstPackets pk, WaveCounters* wc, TravAux aux, uint rpc) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_RAYBUF_WORDS];
    __shared__ float2 mineUV[T8_BLOCK];
    uint n = *pk.leftoverCount; if (n > pk.capacity) n = pk.capacity;
    t8_extend_body<false, false, true, true>(sc, pool, pk.leftover, n, wc, aux, rpc, stack, rayBuf, mineUV, blockIdx.x, gridDim.x, &fv);
}

// ... and behind it, before the task rounds: the stored ray (origin | id, direction | length, as k_generate writes them) of every ray k_extend_first cut into sub-trees — the
// launch's resolve list. Kept out of k_extend_first's publish: the two array pointers it needs there are two more scalar pairs across the traversal loop
__global__ void __launch_bounds__(256) k_first_split_rays(PathKernelContext k, PathPool pool, FirstVertex fv, TravAux aux) {
    const uint n = aux.counts[TRAV_RESOLVE];
    for (uint i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint p = aux.resolveList[i];
        uint px, sample; first_vertex_of(fv, p, px, sample);
        float3 o, d; k.computeCameraRay(px >> 16, px & 0xFFFFu, sample, o, d);
        pool.s0[p] = make_uint4(asuint(o.x), asuint(o.y), asuint(o.z), px); pool.s1[p] = make_uint4(asuint(d.x), asuint(d.y), asuint(d.z), asuint(0.0f));
    }
}

// Task rounds hold hundreds to thousands of sub-trees, far fewer than the launch has quads. A 64-item chunk would put them on count/64 waves (one rank of
// an 8-way sharded frame: ~90 us per round on a handful of waves, 40 % on top of k_extend itself); with few tasks a chunk carries only 16 real ones —
// one per quad — and 48 empty slots that cost an iteration each, so the sub-trees spread over 4x as many waves.
#ifndef T8_TASK_SPREAD
#define T8_TASK_SPREAD 1
#endif
__device__ __forceinline__ uint t8_tasks_per_chunk(uint count) { return (!T8_TASK_SPREAD || count > T8_GROUPS_PER_WAVE * 4u * T8_TASK_BLOCKS_N || T8_GROUPS_PER_WAVE > T8_CHUNK) ? T8_CHUNK : T8_GROUPS_PER_WAVE; }
// sub-trees of split extend rays, round STAGE (0..3) of a traversal launch: reads queue STAGE & 1 (count: counts[STAGE]); unless it is the final round,
// stragglers among the sub-trees are split again into the other queue (count: counts[STAGE + 1]). One counter per round: the whole block is zeroed once per
// pass (pt_wavefront.h TravAux). Task i of the launch is queue entry (i % 64) * ceil(count / 64) + i / 64: the sub-trees of one ray sit next to each other in
// the queue and would otherwise land in one 64-item chunk, i.e. on one wave.
template <int STAGE, bool FINAL>
__device__ __forceinline__ void t8_extend_tasks_body(const DeviceScene& sc, const PathPool& pool, WaveCounters* wc, const TravAux& aux, uint2* stack, uint* rayBuf, const uint vBlock, const uint vGrid) {
    constexpr int IN = STAGE & 1;
    // A count above the capacity: the producer ran out of room (it has set the overflow word, and the frame fails at its end). Such a queue is not read at all: a ray's
    // reservation that straddles the end is not written (pt_traverse8p.h: all of a ray's sub-trees or none), so the entries from there to the capacity hold whatever the
    // memory held — stale tasks of an earlier launch, or nothing ever written — and a tag or a node reference taken from there indexes the pool and the tree out of bounds.
    const uint count = aux.counts[STAGE];
    if (count == 0u || count > aux.taskCap) return;
    const TravTask* tasks = aux.taskQ[IN];
    const uint real = t8_tasks_per_chunk(count), per = (count + real - 1u) / real;
    Traverse8Counters ctr; t8_counters_init(ctr);
    auto fetch = [&](uint i, float3& o, float3& d, float& tmin, float& tmax, uint& startRef, float& bestT0, uint& bestPrim0) -> uint {
        const uint lane = i % T8_CHUNK, j = lane * per + i / T8_CHUNK;
        const bool pad = lane >= real || j >= count;                                  // padding of the transposed index space: an empty task
        TravTask t = tasks[pad ? 0u : j];
        if (pad) t.tbits = 0x7F800000u;
        t8_stored_ray(pool, t.tag, o, d);
        unsigned long long key = aux.bestKey[t.tag];
        tmin = 0.0f; tmax = kMaxRayTravel; bestT0 = __uint_as_float((uint)(key >> 32)); bestPrim0 = (uint)key;
        startRef = (__uint_as_float(t.tbits) <= bestT0) ? t.ref : BVH_EMPTY;            // a sub-tree behind the current best hit is dropped here
        return t.tag;
    };
    auto commit = [&](uint p, const HitInfo& h) { atomicMin(&aux.bestKey[p], t8_hit_key(h.t, h.prim)); };
    auto publish = [&](uint p, float bestT, uint bestPrim) { if (bestPrim != 0xFFFFFFFFu) atomicMin(&aux.bestKey[p], t8_hit_key(bestT, bestPrim)); };
    traverse8_pairs<false, false, true, true, !FINAL>(sc, per * T8_CHUNK, T8_CHUNK, stack, rayBuf, nullptr, fetch, commit, publish, TravTaskOut{aux.taskQ[IN ^ 1], &aux.counts[FINAL ? STAGE : STAGE + 1], FINAL ? 0u : aux.taskCap}, ctr, &wc->overflow, vBlock, vGrid);
}
template <int STAGE, bool FINAL = (STAGE == 3)>
__global__ void __launch_bounds__(T8_BLOCK, T8_EXTEND_MIN_BLOCKS) k_extend_tasks(DeviceScene sc, PathPool pool, WaveCounters* wc, TravAux aux) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_TASKBUF_WORDS];
    t8_extend_tasks_body<STAGE, FINAL>(sc, pool, wc, aux, stack, rayBuf, blockIdx.x, gridDim.x);
}

// split extend rays: the merged key -> hit record; the barycentrics come from re-intersecting the winning triangle (same arithmetic, same operands)
__device__ __forceinline__ void t8_resolve_extend_body(const DeviceScene& sc, const PathPool& pool, const TravAux& aux, const uint vBlock, const uint vGrid) {
    const uint n = aux.counts[TRAV_RESOLVE];
    for (uint i = vBlock * 256u + threadIdx.x; i < n; i += vGrid * 256u) {
        uint p = aux.resolveList[i];
        unsigned long long key = aux.bestKey[p];
        uint prim = (uint)key;
        uint4 out = make_uint4((uint)(key >> 32), prim, 0u, 0u);
        if (prim != 0xFFFFFFFFu) {
            float3 o, d; t8_stored_ray(pool, p, o, d);
            float t, u = 0.f, v = 0.f;
            // the winner was accepted by the traversal; only (u, v) are needed
            const TriRecord tr = sc.tris[aux.primToSlot[prim]]; (void)intersect_tri_wt(tri_v0(tr), tri_v1(tr), tri_v2(tr), o, d, 0.0f, kMaxRayTravel, t, u, v);
            out.z = asuint(u); out.w = asuint(v);
        }
        pool.hit[p] = out;
    }
}
__global__ void __launch_bounds__(256) k_resolve_extend(DeviceScene sc, PathPool pool, TravAux aux) { t8_resolve_extend_body(sc, pool, aux, blockIdx.x, gridDim.x); }

// A visibility ray that ends visible leaves only this mark in the traversal loop (every writer of q2 leaves .w = 0): what the contribution does to its path is
// not needed before the path's next vertex is shaded, and a read-modify-write of the path's radiance — two dependent round trips, the second a scattered one —
// under a divergent branch between the stack pop and the next node loads holds the whole wave up. The resolve pass behind the launch applies the marks
// (t8_resolve_shadow_body); the grouped queue's are folded by k_resolve_nee in sample order.
__device__ __forceinline__ void shadow_mark_visible(ShadowQueue sq, uint i) { reinterpret_cast<float*>(sq.q2 + i)[3] = 1.0f; }
template <bool GROUPED>
// visible == the deferred NEE contribution lands (BridgeDonut:1026)
__device__ __forceinline__ void shadow_visible(PathPool pool, ShadowQueue sq, uint i) {
    if (GROUPED) { shadow_mark_visible(sq, i); return; }
    float4 r = sq.q2[i];
    uint p = asuint(sq.q1[i].w);
    uint4 c = pool.s2[p];
    uint pack45[2] = {c.z, c.w};
    PathKernelContext::ResolveShadow(pack45, make_float3(r.x, r.y, r.z));
    c.z = pack45[0]; c.w = pack45[1];
    pool.s2[p] = c;
    // NEE-AT: the visible light feeds the pixel's reservoir (LightSampler.hlsli:184-200), and the path continues as k_shade worked out for this case
    if (sq.q3) {
        const float4 f = sq.q3[i];
        const uint light = asuint(f.z), fix = asuint(f.w);
        if (light != RTXPT_INVALID_LIGHT_INDEX) {
            uint4 e = pool.s4[p];
            const uint id = pool.s0[p].w, slot = (e.w - sq.fbSampleFirst) * sq.fbPlane + (id & 0xFFFFu) * sq.fbWidth + (id >> 16);
            float total = sq.fbTotalWeight[slot]; uint cand = sq.fbCandidates[slot];
            LightFeedbackReservoir_Add(total, cand, f.y, light & ~LFR_SCREEN_SPACE_COHERENT_FLAG, f.x, (light & LFR_SCREEN_SPACE_COHERENT_FLAG) != 0u);
            sq.fbTotalWeight[slot] = total; sq.fbCandidates[slot] = cand;
            if (fix & 1u) {
                const uint bit = (uint)PF_terminateAtNextBounce << kVertexIndexBitCount;
                if (fix & 2u) e.z |= bit; else { e.z &= ~bit; e.y = (e.y & 0xFFFF0000u) | (fix >> 16); }
                pool.s4[p] = e;
            }
        }
    }
}

// The visibility launch of a path vertex (Bridge::traceVisibilityRay for every entry of the shadow queue) as a device function: k_shadow, and k_trace_pair next
// to the closest-hit rays of the next vertex.
template <bool COUNT>
__device__ __forceinline__ void t8_shadow_body(const DeviceScene& sc, const ShadowQueue& sq, const uint count, WaveCounters* wc, const TravAux& aux, const uint rpc,
                                               uint2* stack, uint* rayBuf, const uint vBlock, const uint vGrid) {
    Traverse8Counters ctr; t8_counters_init(ctr);
    auto fetch = [&](uint i, float3& o, float3& d, float& tmin, float& tmax, uint& startRef, float& bestT0, uint& bestPrim0) -> uint {
        float4 a = sq.q0[i], b = sq.q1[i];
        o = make_float3(a.x, a.y, a.z); d = make_float3(b.x, b.y, b.z); tmin = 0.0f; tmax = a.w; startRef = 0u; bestT0 = a.w; bestPrim0 = 0xFFFFFFFFu;
        return i;
    };
    auto commit = [&](uint i, const HitInfo& h) { if (h.prim == 0xFFFFFFFFu) shadow_mark_visible(sq, i); };      // visible: a mark, one store; occluded: nothing is committed
    // a split shadow ray: "visible so far"; its sub-trees may set the flag, k_resolve_shadow applies the contribution if none did
    auto publish = [&](uint i, float, uint) { aux.bestKey[i] = 0ull; aux.resolveList[atomicAdd(&aux.counts[TRAV_RESOLVE], 1u)] = i; };
    traverse8_pairs<true, COUNT, false, false, true>(sc, count, rpc, stack, rayBuf, nullptr, fetch, commit, publish, TravTaskOut{aux.taskQ[0], &aux.counts[0], aux.taskCap}, ctr, &wc->overflow, vBlock, vGrid);
    if (COUNT) { wave_add64(ctr.nodeVisits, &wc->nodeVisitsSh); wave_add64(ctr.triTests, &wc->triTestsSh); wave_add64(ctr.leafVisits, &wc->leafVisitsSh); wave_add64(ctr.iters, &wc->itersSh); }
}
template <bool COUNT>
__global__ void __launch_bounds__(T8_BLOCK, COUNT ? 1 : T8_SHADOW_MIN_WAVES) k_shadow(DeviceScene sc, ShadowQueue sq, const uint* __restrict__ countPtr, WaveCounters* wc, TravAux aux, uint rpc) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_RAYBUF_WORDS];
    t8_shadow_body<COUNT>(sc, sq, *countPtr, wc, aux, rpc, stack, rayBuf, blockIdx.x, gridDim.x);
}

template <int STAGE, bool FINAL>
__device__ __forceinline__ void t8_shadow_tasks_body(const DeviceScene& sc, const ShadowQueue& sq, WaveCounters* wc, const TravAux& aux, uint2* stack, uint* rayBuf, const uint vBlock, const uint vGrid) {
    constexpr int IN = STAGE & 1;
    const uint count = aux.counts[STAGE];
    if (count == 0u || count > aux.taskCap) return;      // (an overflowed queue is not read: t8_extend_tasks_body)
    const TravTask* tasks = aux.taskQ[IN];
    const uint real = t8_tasks_per_chunk(count), per = (count + real - 1u) / real;
    Traverse8Counters ctr; t8_counters_init(ctr);
    auto fetch = [&](uint i, float3& o, float3& d, float& tmin, float& tmax, uint& startRef, float& bestT0, uint& bestPrim0) -> uint {
        const uint lane = i % T8_CHUNK, j = lane * per + i / T8_CHUNK;
        const bool pad = lane >= real || j >= count;
        TravTask t = tasks[pad ? 0u : j];
        float4 a = sq.q0[t.tag], b = sq.q1[t.tag];
        o = make_float3(a.x, a.y, a.z); d = make_float3(b.x, b.y, b.z); tmin = 0.0f; tmax = a.w; bestT0 = a.w; bestPrim0 = 0xFFFFFFFFu;
        startRef = (!pad && aux.bestKey[t.tag] == 0ull) ? t.ref : BVH_EMPTY;              // padding, or another sub-tree already found an occluder
        return t.tag;
    };
    auto commit = [&](uint i, const HitInfo& h) { if (h.prim != 0xFFFFFFFFu) aux.bestKey[i] = 1ull; };
    auto publish = [&](uint, float, uint) {};
    traverse8_pairs<true, false, false, true, !FINAL>(sc, per * T8_CHUNK, T8_CHUNK, stack, rayBuf, nullptr, fetch, commit, publish, TravTaskOut{aux.taskQ[IN ^ 1], &aux.counts[FINAL ? STAGE : STAGE + 1], FINAL ? 0u : aux.taskCap}, ctr, &wc->overflow, vBlock, vGrid);
}
template <int STAGE, bool FINAL = (STAGE == 3)>
__global__ void __launch_bounds__(T8_BLOCK) k_shadow_tasks(DeviceScene sc, ShadowQueue sq, WaveCounters* wc, TravAux aux) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_TASKBUF_WORDS];
    t8_shadow_tasks_body<STAGE, FINAL>(sc, sq, wc, aux, stack, rayBuf, blockIdx.x, gridDim.x);
}

// The resolve pass of a visibility launch: the rays that were cut into sub-trees (resolve list) land if no sub-tree found an occluder, and — not GROUPED — a
// sweep over the launch's `count` queue entries lands the contributions of the rays the traversal loop marked visible. Order: a later launch of the stream than
// k_shadow / k_trace_pair and the task rounds (every mark is written), an earlier one than everything that reads or adds to a path's radiance or rewrites the
// queue: the k_classify / k_shade of the next vertex, launch_sp_fill_resolve, k_accumulate, the tail kernel. A ray that was cut into sub-trees is published and
// never committed, so the list and the marked set are disjoint; an entry names one path and a path has at most one pending entry, so no two threads touch one
// slot. The sum is the fp16 addition the loop made, on the same operands: the image cannot change. `count` is the host's (k_resolve_pair zeroes the device's
// word in this very launch); 0 is fine.
template <bool GROUPED>
__device__ __forceinline__ void t8_resolve_shadow_body(const PathPool& pool, const ShadowQueue& sq, const TravAux& aux, const uint count, const uint vBlock, const uint vGrid) {
    const uint n = aux.counts[TRAV_RESOLVE];
    for (uint k = vBlock * 256u + threadIdx.x; k < n; k += vGrid * 256u) {
        uint i = aux.resolveList[k];
        if (aux.bestKey[i] == 0ull) shadow_visible<GROUPED>(pool, sq, i);
    }
    if (GROUPED) return;
    for (uint i = vBlock * 256u + threadIdx.x; i < count; i += vGrid * 256u)
        if (reinterpret_cast<const float*>(sq.q2 + i)[3] == 1.0f) shadow_visible<false>(pool, sq, i);
}
template <bool GROUPED>
__global__ void __launch_bounds__(256) k_resolve_shadow(PathPool pool, ShadowQueue sq, TravAux aux, uint count) { t8_resolve_shadow_body<GROUPED>(pool, sq, aux, count, blockIdx.x, gridDim.x); }

// ---- Fused traversal launches (round 6). The visibility rays of path vertex k and the closest-hit rays of vertex k + 1 are independent of each other — the
// visibility results only have to be in the paths' radiance before vertex k + 1 is SHADED (the order of the fp16 additions into PathState::L: the light sample
// of vertex k, then the emission found at vertex k + 1; PathTracer.hlsli:505-762, PathTracerNEE.hlsli:185-275) — so one launch traces both: blocks [0, blocksE)
// work through the extend queue, the others through the shadow queue; every block is of one kind, the traversal loops themselves are the ones k_extend /
// k_shadow run (no per-ray kind, not one instruction more in the loop). What it buys a small frame (one rank of a tile-sharded frame): half the traversal
// launches of a pass and half the straggler rounds behind them — the two kinds' task rounds and resolve passes share their launches too (k_tasks_pair,
// k_resolve_pair) — and each kind's dry tail runs beside the other kind's work instead of in a launch of its own.
__global__ void __launch_bounds__(T8_BLOCK, T8_EXTEND_MIN_BLOCKS) k_trace_pair(DeviceScene sc, PathPool pool, const uint* __restrict__ queue, const uint* __restrict__ extCountPtr, ShadowQueue sq, const uint* __restrict__ shCountPtr,
                                                                              WaveCounters* wc, TravAux auxE, TravAux auxS, uint rpcE, uint rpcS, uint blocksE) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_RAYBUF_WORDS];
    __shared__ float2 mineUV[T8_BLOCK];
    if (blockIdx.x < blocksE) t8_extend_body<false, false>(sc, pool, queue, *extCountPtr, wc, auxE, rpcE, stack, rayBuf, mineUV, blockIdx.x, blocksE);
    else t8_shadow_body<false>(sc, sq, *shCountPtr, wc, auxS, rpcS, stack, rayBuf, blockIdx.x - blocksE, gridDim.x - blocksE);
}
template <int STAGE, bool FINAL = (STAGE == 3)>
__global__ void __launch_bounds__(T8_BLOCK, T8_EXTEND_MIN_BLOCKS) k_tasks_pair(DeviceScene sc, PathPool pool, ShadowQueue sq, WaveCounters* wc, TravAux auxE, TravAux auxS) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_TASKBUF_WORDS];
    const uint half = gridDim.x >> 1;
    if (blockIdx.x < half) t8_extend_tasks_body<STAGE, FINAL>(sc, pool, wc, auxE, stack, rayBuf, blockIdx.x, half);
    else t8_shadow_tasks_body<STAGE, FINAL>(sc, sq, wc, auxS, stack, rayBuf, blockIdx.x - half, gridDim.x - half);
}
// ... and the two resolve passes; the shadow queue's counter is zeroed here for the k_shade that follows (every reader of it — k_trace_pair — is an earlier
// launch of the stream)
__global__ void __launch_bounds__(256) k_resolve_pair(DeviceScene sc, PathPool pool, ShadowQueue sq, TravAux auxE, TravAux auxS, uint* shadowCount, uint shCount, uint blocksE) {
    if (blockIdx.x < blocksE) t8_resolve_extend_body(sc, pool, auxE, blockIdx.x, blocksE);
    else { t8_resolve_shadow_body<false>(pool, sq, auxS, shCount, blockIdx.x - blocksE, gridDim.x - blocksE); if (blockIdx.x == blocksE && threadIdx.x == 0u) *shadowCount = 0u; }
}

// NEEFullSamples != 1: NEEResult accumulates the visible samples of a path vertex in sample order (fp16, PathTracerTypes.hlsli:170-207), then the
// vertex adds the sum to the path once (PathTracer.hlsli:722-746). One thread per group of the shadow queue.
__global__ void __launch_bounds__(256) k_resolve_nee(PathPool pool, ShadowQueue sq, const uint* __restrict__ countPtr) {
    const uint groups = *countPtr / sq.group;
    for (uint g = blockIdx.x * 256u + threadIdx.x; g < groups; g += gridDim.x * 256u) {
        const uint first = g * sq.group;
        uint nee[2] = {0u, 0u};
        for (uint s = 0; s < sq.group; s++) {
            float4 r = sq.q2[first + s];
            if (r.w != 0.f) PathKernelContext::NeeAccumulate(nee, make_float3(r.x, r.y, r.z));
        }
        uint p = asuint(sq.q1[first].w);
        uint4 c = pool.s2[p];
        uint pack45[2] = {c.z, c.w};
        PathKernelContext::NeeCommit(pack45, nee);
        c.z = pack45[0]; c.w = pack45[1];
        pool.s2[p] = c;
    }
}

__global__ void __launch_bounds__(T8_BLOCK) k_trace_probe(DeviceScene sc, const float4* __restrict__ rays, uint n, float4* __restrict__ outClosest, uint* __restrict__ outVisible, uint* overflow) {
    __shared__ uint2 stack[T8_GROUPS_PER_BLOCK * BVH8_STACK_STRIDE];
    __shared__ uint rayBuf[T8_RAYBUF_WORDS];
    __shared__ float2 mineUV[T8_BLOCK];
    Traverse8Counters ctr; t8_counters_init(ctr);
    auto fetch = [&](uint i, float3& o, float3& d, float& tmin, float& tmax, uint& startRef, float& bestT0, uint& bestPrim0) -> uint {
        float4 a = rays[2 * i], b = rays[2 * i + 1];
        o = make_float3(a.x, a.y, a.z); d = make_float3(b.x, b.y, b.z); tmin = a.w; tmax = b.w; startRef = 0u; bestT0 = b.w; bestPrim0 = 0xFFFFFFFFu;
        return i;
    };
    auto publish = [&](uint, float, uint) {};
    if (outClosest) {
        auto commit = [&](uint i, const HitInfo& h) { outClosest[i] = make_float4(h.t, asfloat(h.prim), h.u, h.v); };
        traverse8_pairs<false, false, false, false, false>(sc, n, T8_CHUNK, stack, rayBuf, mineUV, fetch, commit, publish, TravTaskOut{nullptr, nullptr, 0u}, ctr, overflow, blockIdx.x, gridDim.x);
    } else {
        auto commit = [&](uint i, const HitInfo& h) { outVisible[i] = (h.prim == 0xFFFFFFFFu) ? 1u : 0u; };
        traverse8_pairs<true, false, false, false, false>(sc, n, T8_CHUNK, stack, rayBuf, mineUV, fetch, commit, publish, TravTaskOut{nullptr, nullptr, 0u}, ctr, overflow, blockIdx.x, gridDim.x);
    }
}

// The task rounds and the resolve pass behind a traversal launch, for every kind of launch. round(stage, last) launches task round `stage`: two rounds behind a small launch
// (split once more, then finish), else four (queue 0 -> 1, 1 -> 0, 0 -> 1, queue 1 to the end; pt_trace_plan.h t8_task_rounds). resolve() launches the pass that lands the
// split rays' results.
template <class Round, class Resolve>
static void launch_stragglers(uint rounds, Round round, Resolve resolve) {
    using std::integral_constant;
    round(integral_constant<int, 0>{}, std::false_type{});
    if (rounds == 2u) round(integral_constant<int, 1>{}, std::true_type{});
    else { round(integral_constant<int, 1>{}, std::false_type{}); round(integral_constant<int, 2>{}, std::false_type{}); round(integral_constant<int, 3>{}, std::true_type{}); }
    resolve();
}
static void launch_extend_stragglers(const DeviceScene& sc, PathPool pool, uint count, WaveCounters* wc, TravAux aux, hipStream_t st) {
    launch_stragglers(t8_task_rounds(count),
        [&](auto stage, auto last) { hipLaunchKernelGGL((k_extend_tasks<decltype(stage)::value, decltype(last)::value>), dim3(T8_TASK_BLOCKS), dim3(T8_BLOCK), 0, st, sc, pool, wc, aux); },
        [&] { hipLaunchKernelGGL(k_resolve_extend, dim3(T8_RESOLVE_BLOCKS), dim3(256), 0, st, sc, pool, aux); });
}
void launch_extend_first(const PathKernelContext& k, PathPool pool, FirstVertex fv, const uint* countPtr, uint count, WaveCounters* wc, TravAux aux, FirstPackets pk, hipStream_t st) {
    const uint rpc = rays_per_chunk(count);
    const uint g = t8_ray_grid(count, rpc, t8_grid_bound(aux.maxBlocks));
    if (pk.leftover) {
        // the packets, then the per-ray kernel over what they left (its count is on the device: the grid that would hold all of it, and the waves without a chunk end at once)
        const uint gp = t8_packet_grid(count, pk.wide != 0u, aux.maxBlocks);
        if (pk.wide && pk.precull) hipLaunchKernelGGL(k_extend_first_packets64<true>, dim3(gp), dim3(T8_BLOCK), 0, st, k.sc, pool, fv, countPtr, wc, pk);
        else if (pk.wide) hipLaunchKernelGGL(k_extend_first_packets64<false>, dim3(gp), dim3(T8_BLOCK), 0, st, k.sc, pool, fv, countPtr, wc, pk);
        else hipLaunchKernelGGL(k_extend_first_packets, dim3(gp), dim3(T8_BLOCK), 0, st, k.sc, pool, fv, countPtr, wc, pk);
        hipLaunchKernelGGL(k_extend_first_listed, dim3(g), dim3(T8_BLOCK), 0, st, k.sc, pool, fv, pk, wc, aux, rpc);
    } else
    hipLaunchKernelGGL(k_extend_first, dim3(g), dim3(T8_BLOCK), 0, st, k.sc, pool, fv, countPtr, wc, aux, rpc);
    hipLaunchKernelGGL(k_first_split_rays, dim3(T8_RESOLVE_BLOCKS), dim3(256), 0, st, k, pool, fv, aux);
    launch_extend_stragglers(k.sc, pool, count, wc, aux, st);
}
void launch_extend(const DeviceScene& sc, PathPool pool, const uint* queue, const uint* countPtr, uint count, WaveCounters* wc, bool counters, TravAux aux, hipStream_t st, bool ranged) {
    const uint rpc = rays_per_chunk(count);
    const uint g = t8_ray_grid(count, rpc, t8_grid_bound(aux.maxBlocks));
    if (ranged) { if (counters) hipLaunchKernelGGL((k_extend<true, true>), dim3(g), dim3(T8_BLOCK), 0, st, sc, pool, queue, countPtr, wc, aux, rpc);
                  else hipLaunchKernelGGL((k_extend<false, true>), dim3(g), dim3(T8_BLOCK), 0, st, sc, pool, queue, countPtr, wc, aux, rpc); }
    else if (counters) hipLaunchKernelGGL((k_extend<true>), dim3(g), dim3(T8_BLOCK), 0, st, sc, pool, queue, countPtr, wc, aux, rpc);
    else hipLaunchKernelGGL((k_extend<false>), dim3(g), dim3(T8_BLOCK), 0, st, sc, pool, queue, countPtr, wc, aux, rpc);
    launch_extend_stragglers(sc, pool, count, wc, aux, st);
}
// One launch for the closest-hit rays of the extend queue AND the visibility rays the previous vertex left in the shadow queue (k_trace_pair), then the task
// rounds and resolve passes of both. auxE / auxS: separate task queues, counters, merge keys and resolve lists. The grid and its split: t8_pair_grid (pt_trace_plan.h), whose
// precondition is the caller's: the bound (auxE.maxBlocks, where set) is >= 2. Zeroes *shCountPtr at its end.
void launch_trace_pair(const DeviceScene& sc, PathPool pool, const uint* queue, const uint* extCountPtr, uint extCount, ShadowQueue sq, uint* shCountPtr, uint shCount, WaveCounters* wc, TravAux auxE, TravAux auxS, hipStream_t st) {
    const uint rpc = rays_per_chunk(extCount + shCount);
    const T8PairGrid g = t8_pair_grid(extCount, shCount, rpc, t8_grid_bound(auxE.maxBlocks));
    hipLaunchKernelGGL(k_trace_pair, dim3(g.gE + g.gS), dim3(T8_BLOCK), 0, st, sc, pool, queue, extCountPtr, sq, shCountPtr, wc, auxE, auxS, rpc, rpc, g.gE);
    launch_stragglers(t8_task_rounds_pair(extCount, shCount),
        [&](auto stage, auto last) { hipLaunchKernelGGL((k_tasks_pair<decltype(stage)::value, decltype(last)::value>), dim3(2u * T8_TASK_BLOCKS), dim3(T8_BLOCK), 0, st, sc, pool, sq, wc, auxE, auxS); },
        [&] { hipLaunchKernelGGL(k_resolve_pair, dim3(T8_RESOLVE_BLOCKS + shadow_resolve_grid(shCount)), dim3(256), 0, st, sc, pool, sq, auxE, auxS, shCountPtr, shCount, T8_RESOLVE_BLOCKS); });
}
void launch_shadow(const DeviceScene& sc, PathPool pool, ShadowQueue sq, const uint* countPtr, uint count, WaveCounters* wc, bool counters, TravAux aux, hipStream_t st) {
    const uint rpc = rays_per_chunk(count);
    const uint g = t8_ray_grid(count, rpc, t8_grid_bound(aux.maxBlocks));
    // (one loop for both queue layouts: it only marks. No traversal counters in the grouped mode)
    if (counters && !sq.group) hipLaunchKernelGGL((k_shadow<true>), dim3(g), dim3(T8_BLOCK), 0, st, sc, sq, countPtr, wc, aux, rpc);
    else hipLaunchKernelGGL((k_shadow<false>), dim3(g), dim3(T8_BLOCK), 0, st, sc, sq, countPtr, wc, aux, rpc);
    launch_stragglers(t8_task_rounds(count),
        [&](auto stage, auto last) { hipLaunchKernelGGL((k_shadow_tasks<decltype(stage)::value, decltype(last)::value>), dim3(T8_TASK_BLOCKS), dim3(T8_BLOCK), 0, st, sc, sq, wc, aux); },
        [&] { if (sq.group) hipLaunchKernelGGL((k_resolve_shadow<true>), dim3(T8_RESOLVE_BLOCKS), dim3(256), 0, st, pool, sq, aux, 0u);      // (marks only; k_resolve_nee folds them)
              else hipLaunchKernelGGL((k_resolve_shadow<false>), dim3(shadow_resolve_grid(count)), dim3(256), 0, st, pool, sq, aux, count); });
    if (sq.group) hipLaunchKernelGGL(k_resolve_nee, dim3(grid_for(count / sq.group, 256, 4096)), dim3(256), 0, st, pool, sq, countPtr);
}
void launch_trace_probe(const DeviceScene& sc, const float4* rays, uint n, float4* outClosest, uint* outVisible, uint* overflow, hipStream_t st) {
    hipLaunchKernelGGL(k_trace_probe, dim3(grid_for(n, T8_BLOCK, T8_MAX_BLOCKS)), dim3(T8_BLOCK), 0, st, sc, rays, n, outClosest, outVisible, overflow);
}
} // namespace ptk

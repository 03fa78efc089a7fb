// mi355pt — cooperative BVH8 traversal for wave64, two lanes per ray: a wave carries 32 rays, each owned by a PAIR of lanes; lane h of a pair tests
// children 4h .. 4h + 3 of the current 128-byte node (48 contiguous bytes: three 16-byte loads) and triangle h of a leaf.
//
// Why pairs (round 3): with four lanes per ray (the kernel of rounds 1-3, in the history) the loop is VALU-issue bound at 8 waves per SIMD — extra v_nop slots
// lengthen k_extend one for one (profiles/r03i_valu_bound_probe.txt) — and a wave64 VALU instruction costs its four cycles whatever the lanes do. Of the ~325
// VALU instructions of an average wave iteration only the slab tests (~50) and the triangle tests (~110 when the leaf block runs) are work that belongs to a
// child or a triangle; the rest — refill, child ranking, stack, slot bookkeeping, the alpha test's addressing, the hit reduction — is per-RAY work that every
// lane of the ray's group repeats. Two lanes per ray halve the replicated share per ray: per lane the slab and triangle work doubles (four children, two
// triangle rounds), per wave iteration the instruction count rises by about a third, and the iteration advances 32 rays instead of 16. The closest hit is
// traversal-order free (min t, ties to the lower primitive id); an occlusion query reports whether any accepted hit exists. Straggler splitting, Src / Dst /
// Pub and the template flags: pt_traverse8.h — and so are the slab test and the hit definition (ray frame, leaf block, pair minimum, closest-hit report), which this
// traverser calls like every other: what is written here is policy — refill, child ranking, the stack, postponed leaves, splitting.
#pragma once
#include "pt_traverse8.h"

namespace ptk {

#define DPP_PAIR_LO 0xA0      // quad_perm [0,0,2,2]: lane 0 of the pair
__device__ __forceinline__ uint pair_bits(unsigned long long m, uint pl) { return (uint)(m >> pl) & 0x3u; }

// Measured and removed (history: commit af4c2b2 has the code; numbers in DESIGN.md §4): a dense leaf block (profiles/r04y_dense_leaf_ab.txt, +13 %), batched
// refills (r04y_refill_batch_ab.txt), one pop trip per iteration (r04v_pop_once_ab.txt), two entries per pop trip, octant-ordered child slots
// (r04u_octant_order_ab.txt, +25 %); round 5: a ray with nothing left but postponed leaves waiting one or three iterations (or for a second / fourth such ray)
// before it forces the leaf block — the block then runs in 0.50 instead of 0.65 of the iterations and the rays take 0.63 instead of 0.58 iterations: k_extend
// unchanged (profiles/r05s_leaf_patience_ab.txt). DEFER (with CAN_SPLIT): a dry wave keeps going for taskOut.capacity iterations (instead of T8_TAIL_ITERS),
// and the rays then still in flight are not cut into sub-trees, only reported through publish() — the caller has them traced again elsewhere (the tail kernel,
// pt_tail.hip, hands their paths back to the host loop). No task queue is touched.
template <bool ANYHIT, bool COUNT, bool FIXED_RANGE, bool TASKS, bool CAN_SPLIT, bool DEFER = false, class Src, class Dst, class Pub>
__device__ __forceinline__ void traverse8_pairs(const DeviceScene& sc, uint count, uint raysPerChunk, uint2* stackBase, uint* rayBufBase, float2* mineUV, Src fetch, Dst commit, Pub publish, TravTaskOut taskOut,
                                                Traverse8Counters& ctr, uint* overflowFlag, const uint vBlock, const uint vGrid) {
    // vBlock / vGrid: the block's index among, and the number of, the blocks that work on THIS launch's items — blockIdx.x / gridDim.x for a kernel of one
    // kind; a fused launch (k_trace_pair: closest-hit blocks next to visibility blocks, pt_wavefront.hip) hands each kind its own range. The stack tails are
    // addressed by the physical block index.
    static_assert(T8_LANES == 2u, "traverse8_pairs is the two-lanes-per-ray build");
    const uint RAY_STRIDE = TASKS ? T8_TASK_STRIDE : T8_RAY_STRIDE;
    const uint lane = threadIdx.x & 63u, h = lane & 1u, pl = lane & ~1u;
    const uint grp = threadIdx.x >> 1;
    uint2* stack = stackBase + grp * BVH8_STACK_STRIDE;
    const uint wavesPerBlock = T8_BLOCK / 64u;
    const uint waveId = vBlock * wavesPerBlock + (threadIdx.x >> 6), numWaves = vGrid * wavesPerBlock;
    const char* nodesBase = reinterpret_cast<const char*>(sc.nodes8);
    const char* trisBase = reinterpret_cast<const char*>(sc.tris);
    const uint laneChildOff = 16u + 48u * h;
    const uint INF_BITS = 0x7F800000u;

    const uint numWavesU = (uint)__builtin_amdgcn_readfirstlane((int)numWaves);
    uint chunk = (uint)__builtin_amdgcn_readfirstlane((int)(waveId - numWaves)), chunkPos = 0u, chunkEnd = 0u;
    const uint rpc = (uint)__builtin_amdgcn_readfirstlane((int)raysPerChunk);
    bool exhausted = (waveId * rpc >= count) || !sc.rootIsValid;
    uint* rayBuf = rayBufBase + (threadIdx.x >> 6) * (T8_CHUNK * RAY_STRIDE);
    uint tailIters = 0u, waveDry = 0u;      // wave-uniform, kept as scalars: the number of iterations since the wave found its queue empty
    if (!sc.rootIsValid && waveId == 0 && count) {            // empty scene: every ray misses
        for (uint i = lane; i < count; i += 64u) { float3 o, d; float a, b, bt; uint sr, bp; uint tag = fetch(i, o, d, a, b, sr, bt, bp); HitInfo hh; hh.t = b; hh.prim = 0xFFFFFFFFu; hh.u = hh.v = 0.f; commit(tag, hh); }
    }
    bool active = false;
    float3 o = make_float3(0.f);
    // the ray's shear (d[kx] / d[kz], d[ky] / d[kz]) and the byte offsets of the record groups of its axes kx | ky << 8 | kz << 16 (leaf block)
    float Sx = 0.f, Sy = 0.f; uint axes = 0u;
    float ix = 0.f, iy = 0.f, iz = 0.f;
    uint selN = 0u, selF = 0u;
    float tmin = 0.f, tmax = FIXED_RANGE ? kMaxRayTravel : 0.f;
    float bestT = 0.f; uint bestPrim = 0xFFFFFFFFu;
    uint minePrim = 0xFFFFFFFFu;
    uint cur = BVH_EMPTY, pend = BVH_EMPTY, sp = 0, tag = 0;
    uint rayIters = 0;
    float taskT0 = 0.f; uint taskPrim0 = 0xFFFFFFFFu;
    uint pend1 = BVH_EMPTY, pend2 = BVH_EMPTY;
#ifdef T8_PROBE_INSTANCE_SWITCHES
    uint lastInst_ = 0xFFFFFFFFu;
#endif

    // sb: the pair's stack base. The caller forms it anew for every node that pushes (stack_base(): two instructions) instead of keeping it across the loop:
    // the loop is one register short since the watertight leaf block, and the allocator's choice was to spill exactly this value — a scratch load and a full
    // vmcnt(0) wait at every push.
    auto stack_base = [&]() -> uint2* { uint g_ = threadIdx.x >> 1; asm volatile("" : "+v"(g_)); return stackBase + g_ * BVH8_STACK_STRIDE; };
    // the pair's stack tail in global memory (entries BVH8_STACK and up: rare). Formed where it is used, for the same reason: hoisted out of the loop, the
    // address is the value the allocator spills.
    auto spill_slot = [&](uint idx) -> uint2* { uint g_ = threadIdx.x >> 1; asm volatile("" : "+v"(g_)); return sc.travSpill + ((size_t)(blockIdx.x * T8_GROUPS_PER_BLOCK + g_) * T8_SPILL_DEPTH + (idx - BVH8_STACK)); };
    auto stackStore = [&](uint2* sb, uint idx, uint ref, uint tbits) {
        if (idx < BVH8_STACK) sb[idx] = make_uint2(ref, tbits);
        else {
            unsigned long long* tail = reinterpret_cast<unsigned long long*>(spill_slot(idx));
            __builtin_nontemporal_store(((unsigned long long)tbits << 32) | ref, tail);
        }
    };

    bool splitNow = false, stop = false;
    while (!stop) {
        unsigned long long tc0 = 0, tc1 = 0, tc2 = 0, tc3 = 0;
        if (COUNT) tc0 = __builtin_readcyclecounter();
        // ---- refill idle pairs from the wave's current chunk
        bool need = !active && !exhausted;
        unsigned long long needMask = t8_ballot(need && h == 0u);
        if (needMask) {
            T8_EVENT(0, true);
            if (chunkPos >= chunkEnd) {
                T8_EVENT(1, true);
                chunk += numWavesU;
                chunkPos = chunk * rpc; chunkEnd = (chunkPos + rpc < count) ? chunkPos + rpc : count;
                if (chunkPos >= count) { chunkPos = chunkEnd = count; }
                if (chunkPos + lane < chunkEnd) {
                    float3 ro, rd; float rtmin, rtmax, rbestT; uint rstart, rbestPrim;
                    uint rtag = fetch(chunkPos + lane, ro, rd, rtmin, rtmax, rstart, rbestT, rbestPrim);
                    uint* slot = rayBuf + lane * RAY_STRIDE;
                    slot[0] = __float_as_uint(ro.x); slot[1] = __float_as_uint(ro.y); slot[2] = __float_as_uint(ro.z);
                    float rix, riy, riz, rSx, rSy; uint raxes; t8_ray_frame(rd, rix, riy, riz, rSx, rSy, raxes);      // (formed once, by the fetching lane)
                    slot[3] = __float_as_uint(rSx); slot[4] = __float_as_uint(rSy); slot[5] = raxes;
                    slot[6] = rtag;
                    // the interval's two words are free (every ray of the launch has [0, kMaxRayTravel]): they carry the byte selectors of the slab test
                    if (FIXED_RANGE && !TASKS) {
                        uint rselN, rselF; t8_slab_selectors(rix, riy, riz, rselN, rselF); slot[7] = rselN; slot[8] = rselF;
                    } else { slot[7] = __float_as_uint(TASKS ? rtmax : rtmin); slot[8] = TASKS ? __float_as_uint(rbestT) : __float_as_uint(rtmax); }
                    if (TASKS) { slot[9] = rbestPrim; slot[10] = rstart; }
                    slot[RAY_STRIDE - 3u] = __float_as_uint(rix); slot[RAY_STRIDE - 2u] = __float_as_uint(riy); slot[RAY_STRIDE - 1u] = __float_as_uint(riz);
                }
            }
            uint avail = chunkEnd - chunkPos;
            // Two statements, not if / else: with "queue empty -> flags, else -> take a ray" every loop-carried value of the ray is a three-way phi at the
            // join, which the compiler lowers as a copy of the loop's registers out to temporaries and back on every pass through this block (38 v_mov). An
            // empty queue simply makes the take condition below false (rank < 0) and the cursor advance zero (profiles/r05t_refill_flat_ab.txt: k_extend 46.2
            // -> 45.1 ms).
            if (avail == 0u) { if (need) exhausted = true; waveDry = 1u; }
            {
                uint rank = (uint)__popcll(needMask & ((1ull << pl) - 1ull));
                uint n = (uint)__popcll(needMask);
                if (need && rank < avail) {
                    const uint* slot = rayBuf + (((chunkPos - chunk * rpc) + rank) * RAY_STRIDE);
                    o = make_float3(__uint_as_float(slot[0]), __uint_as_float(slot[1]), __uint_as_float(slot[2]));
                    Sx = __uint_as_float(slot[3]); Sy = __uint_as_float(slot[4]); axes = slot[5];
                    tag = slot[6];
                    ix = __uint_as_float(slot[RAY_STRIDE - 3u]); iy = __uint_as_float(slot[RAY_STRIDE - 2u]); iz = __uint_as_float(slot[RAY_STRIDE - 1u]);
                    if (FIXED_RANGE && !TASKS) { selN = slot[7]; selF = slot[8]; }
                    else t8_slab_selectors(ix, iy, iz, selN, selF);
                    if (TASKS) {
                        if (!FIXED_RANGE) tmax = __uint_as_float(slot[7]);
                        bestT = taskT0 = __uint_as_float(slot[8]); bestPrim = taskPrim0 = slot[9]; cur = slot[10];
                    } else {
                        if (!FIXED_RANGE) { tmin = __uint_as_float(slot[7]); tmax = __uint_as_float(slot[8]); }
                        bestT = tmax; bestPrim = 0xFFFFFFFFu; cur = 0u;
                    }
                    minePrim = 0xFFFFFFFFu; rayIters = 0u;
#ifdef T8_PROBE_INSTANCE_SWITCHES
                    lastInst_ = 0xFFFFFFFFu;
#endif
                    pend = BVH_EMPTY; pend1 = BVH_EMPTY; pend2 = BVH_EMPTY; sp = 0u; active = true;
                }
                chunkPos = (uint)__builtin_amdgcn_readfirstlane((int)(chunkPos + ((n < avail) ? n : avail)));
            }
        }
        bool run = t8_ballot(active) != 0ull;
        if (!run) { if (t8_ballot(!exhausted) == 0ull) stop = true; }
        else if (CAN_SPLIT) {
            tailIters += waveDry;
            if (tailIters > (DEFER ? taskOut.capacity : (uint)(TASKS ? T8_TAIL_ITERS_TASKS : T8_TAIL_ITERS))) { splitNow = true; stop = true; run = false; }
        }
        if (run) {
#ifdef T8_PROBE_VNOPS
#pragma unroll
        for (int k_ = 0; k_ < T8_PROBE_VNOPS; k_++) asm volatile("v_nop");
#endif
// issue-slot probes (developer builds; tools/valu_ceiling): T8_PROBE_FILL_N independent filler instructions per wave iteration — 1: of the class that issues
// every
#ifdef T8_PROBE_FILL
        // 2 cycles per SIMD (v_add_u32), 2: of the class that issues every 4 (v_max_f32), 3: v_cndmask_b32_e64, 4: scalar (s_and_b64 of the exec mask into a dead
        // SGPR pair, no memory operand). Outputs are dead; no register lives across the loop.
        {
            uint f0_, f1_;
#pragma unroll
            for (int k_ = 0; k_ < T8_PROBE_FILL_N / 2; k_++) {
                if (T8_PROBE_FILL == 4) { unsigned long long s0_, s1_; asm volatile("s_and_b64 %0, exec, exec\n s_and_b64 %1, exec, exec" : "=s"(s0_), "=s"(s1_) : : "scc"); }
                else if (T8_PROBE_FILL == 1) asm volatile("v_add_u32 %0, %2, %2\n v_add_u32 %1, %2, %2" : "=v"(f0_), "=v"(f1_) : "v"(lane));
                else if (T8_PROBE_FILL == 2) asm volatile("v_max_f32 %0, %2, %2\n v_max_f32 %1, %2, %2" : "=v"(f0_), "=v"(f1_) : "v"(lane));
                else asm volatile("v_cndmask_b32_e64 %0, %2, %2, s[0:1]\n v_cndmask_b32_e64 %1, %2, %2, s[0:1]" : "=v"(f0_), "=v"(f1_) : "v"(lane));
            }
        }
#endif
        if (COUNT && lane == 0u) ctr.iters++;
        if (COUNT && active) rayIters++;
        if (COUNT) tc1 = __builtin_readcyclecounter();
        const bool inner = active && !(cur & BVH_LEAF_BIT);
        const bool leafReady = active && (pend != BVH_EMPTY);
        const bool queueFull = (T8_LEAF_QUEUE == 1) ? true : ((T8_LEAF_QUEUE == 2) ? (pend1 != BVH_EMPTY) : (pend2 != BVH_EMPTY));
        const bool leafBlocked = leafReady && (cur & BVH_LEAF_BIT) && (cur == BVH_EMPTY || queueFull);
        // (a second trigger — "n pairs hold a postponed leaf" — never paid: profiles/r05o_leaf_batch_ab.txt, r05t_refill_flat_ab.txt)
        const bool runLeaves = t8_ballot(leafBlocked) != 0ull;
        const bool leaf = leafReady && runLeaves;
        if (COUNT && leaf && h == 0u) ctr.leafVisits++;
// developer probe (counter builds): how often would a two-level traversal have to enter an instance? Counted per ray as the visited leaves whose
#ifdef T8_PROBE_INSTANCE_SWITCHES
        // instance differs from the previous visited leaf's (event slot 4 — the alpha-test count — carries it in such a build)
        if (COUNT && leaf && h == 0u) {
            const uint prim_ = *reinterpret_cast<const uint*>(trisBase + (((pend & 0x7FFFFFFFu) >> 3) * 48u + 12u));
            const uint inst_ = *reinterpret_cast<const uint*>(reinterpret_cast<const char*>(sc.shadeTris) + (size_t)prim_ * 128u);
            if (inst_ != lastInst_) ctr.ev[4]++;
            lastInst_ = inst_;
        }
#endif
        T8_EVENT(2, inner); T8_EVENT(3, leaf);

        // ---- inner node: lane h tests children 4h .. 4h + 3
        if (inner) {
            const uint nodeOff = cur * 128u;
            const u32x4 hdr = *reinterpret_cast<const u32x4*>(nodesBase + nodeOff);
            const u32x4 c0 = *reinterpret_cast<const u32x4*>(nodesBase + (nodeOff + laneChildOff));
            const u32x4 c1 = *reinterpret_cast<const u32x4*>(nodesBase + (nodeOff + laneChildOff + 16u));
            const u32x4 c2 = *reinterpret_cast<const u32x4*>(nodesBase + (nodeOff + laneChildOff + 32u));
            const f32x4 scl = *reinterpret_cast<const f32x4*>(nodesBase + (nodeOff + 112u));
            if (COUNT && h == 0u) ctr.nodeVisits++;
            const float nx = __uint_as_float(hdr.x), ny = __uint_as_float(hdr.y), nz = __uint_as_float(hdr.z);
            const float sx = scl.x, sy = scl.y, sz = scl.z;
            auto slab = [&](uint q0, uint q1, float& tn, float& tf) { t8_slab(q0, q1, selN, selF, nx, ny, nz, sx, sy, sz, o.x, o.y, o.z, ix, iy, iz, tmin, bestT, tn, tf); };
            uint ref[4] = {c0.x, c0.w, c1.z, c2.y};
            // integer sort keys: tn >= 0 so its bits order like the value; the low 3 mantissa bits carry the child index (unique keys, ties to the lower
            // child); a child that is not hit gets +inf. The stack entry's distance is the key without its index bits.
            uint key[4]; bool hit[4];
            {   float tn, tf;
                slab(c0.y, c0.z, tn, tf); hit[0] = T8_HIT(ref[0], tn, tf); key[0] = (hit[0] ? (__float_as_uint(tn) & ~7u) : INF_BITS) | (4u * h);
                slab(c1.x, c1.y, tn, tf); hit[1] = T8_HIT(ref[1], tn, tf); key[1] = (hit[1] ? (__float_as_uint(tn) & ~7u) : INF_BITS) | (4u * h + 1u);
                slab(c1.w, c2.x, tn, tf); hit[2] = T8_HIT(ref[2], tn, tf); key[2] = (hit[2] ? (__float_as_uint(tn) & ~7u) : INF_BITS) | (4u * h + 2u);
                slab(c2.z, c2.w, tn, tf); hit[3] = T8_HIT(ref[3], tn, tf); key[3] = (hit[3] ? (__float_as_uint(tn) & ~7u) : INF_BITS) | (4u * h + 3u);
            }
            uint nhit, rank[4];
            if (ANYHIT && T8_ANYHIT_UNORDERED) {
                // an occlusion query has no use for a front-to-back order: the hit children are numbered by child index
                const uint own = (hit[0] ? 1u : 0u) | (hit[1] ? 2u : 0u) | (hit[2] ? 4u : 0u) | (hit[3] ? 8u : 0u);
                const uint oth = dpp_u<DPP_QP_XOR1>(own);
                const uint all = h ? (oth | (own << 4)) : (own | (oth << 4));
                nhit = (uint)__popc(all);
                const uint below = (1u << (4u * h)) - 1u;            // children of the other lane that come first
#pragma unroll
                for (int k = 0; k < 4; k++) rank[k] = (uint)__popc(all & (below | (((1u << k) - 1u) << (4u * h))));
            } else {
                nhit = (hit[0] ? 1u : 0u) + (hit[1] ? 1u : 0u) + (hit[2] ? 1u : 0u) + (hit[3] ? 1u : 0u);
                nhit += dpp_u<DPP_QP_XOR1>(nhit);
                // rank = number of keys below mine: six compares among my own four (each decides two ranks), sixteen against the other lane's
                rank[0] = 3u; rank[1] = 2u; rank[2] = 1u; rank[3] = 0u;
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = i + 1; j < 4; j++) { const uint c = (key[i] < key[j]) ? 1u : 0u; rank[j] += c; rank[i] -= c; }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint ok = dpp_u<DPP_QP_XOR1>(key[j]);
#pragma unroll
                    for (int k = 0; k < 4; k++) rank[k] += (ok < key[k]) ? 1u : 0u;
                }
            }
            uint next = BVH_EMPTY;
#pragma unroll
            for (int k = 0; k < 4; k++) next = (hit[k] && rank[k] == 0u) ? ref[k] : next;
            next &= dpp_u<DPP_QP_XOR1>(next);
            // The pushes, far to near (nearest on top). One ballot chooses between two texts. Common: no ray of the wave leaves the LDS part of its stack with this
            // node — every child slot is ONE unconditional store: a child that is not pushed (not hit, or the nearest: rank 0) writes to entry BVH8_STACK of the pair's
            // own row, the spare entry behind the BVH8_STACK that are used (BVH8_STACK_STRIDE = BVH8_STACK + 1; no pop, no split and no store of the other text touches
            // it: each of them tests its index < BVH8_STACK first). A compare, a select, a shift-add and the store per slot, no exec-mask change; as four guarded
            // stores the same region was four mask save / branch / restore groups. Rare: some ray goes into, or over, its tail in global memory — the guarded text.
            const bool deep = nhit > 1u && sp + nhit - 1u > BVH8_STACK;
            if (t8_ballot(deep) == 0ull) {
                uint2* sb = stack_base();
                const uint top = sp + nhit - 1u;
#pragma unroll
                for (int k = 0; k < 4; k++) sb[(hit[k] && rank[k] > 0u) ? top - rank[k] : BVH8_STACK] = make_uint2(ref[k], key[k] & ~7u);
                sp = (nhit > 1u) ? top : sp;
            } else if (nhit > 1u) {
                if (sp + nhit - 1u > BVH8_STACK + T8_SPILL_DEPTH) { if (h == 0u) atomicOr(overflowFlag, 1u); }
                else {      // far to near: nearest on top
                    uint2* sb = stack_base();
#pragma unroll
                    for (int k = 0; k < 4; k++) if (hit[k] && rank[k] > 0u) stackStore(sb, sp + (nhit - 1u - rank[k]), ref[k], key[k] & ~7u);
                    sp += nhit - 1u;
                }
            }
            cur = next;
        }

        if (COUNT) { tc2 = __builtin_readcyclecounter(); if (t8_ballot(leaf) != 0ull && lane == 0u) ctr.leafBlocks++; }
        // ---- postponed leaf: the shared leaf block (pt_traverse8.h t8_leaf_block), every lane of the wave that holds a ray with a postponed leaf
        if (leaf) {
            const T8LeafHit lh = t8_leaf_block<ANYHIT, COUNT>(sc, trisBase, pend, h, true, o.x, o.y, o.z, ix, iy, iz, Sx, Sy, axes, tmin, tmax, bestT, bestPrim, &ctr);
            const bool cand = (lh.prim != 0xFFFFFFFFu);
            pend = pend1; pend1 = pend2; pend2 = BVH_EMPTY;
            uint candBits = pair_bits(t8_ballot(cand), pl);
#ifndef T8_PROBE_INSTANCE_SWITCHES
            T8_EVENT(4, lh.alphaRan);
#endif
            T8_EVENT(5, candBits != 0u);
            if (candBits) {
                if (ANYHIT) {
                    if (h == (uint)__ffs((int)candBits) - 1u) { HitInfo hh; hh.t = lh.t; hh.prim = lh.prim; hh.u = hh.v = 0.f; commit(tag, hh); }
                    active = false;
                } else {
                    if (cand && !TASKS) { minePrim = lh.prim; mineUV[threadIdx.x] = make_float2(lh.u, lh.v); }
                    float tk = lh.t; uint pk = lh.prim; t8_pair_min(tk, pk);
                    bestT = tk; bestPrim = pk;
                }
            }
        }

        if (COUNT) tc3 = __builtin_readcyclecounter();
        // ---- slot bookkeeping: a leaf reached by the descent moves to the free leaf slot; an empty node slot pops the stack
        if (active) {
            {   // the first free leaf slot takes the leaf: compares and selects, no branches (profiles/r05u_queue_select_ab.txt)
                const bool isLeaf = (cur & BVH_LEAF_BIT) && cur != BVH_EMPTY;
                const bool e0 = pend == BVH_EMPTY, e1 = (T8_LEAF_QUEUE > 1) && pend1 == BVH_EMPTY, e2 = (T8_LEAF_QUEUE > 2) && pend2 == BVH_EMPTY;
                const bool to0 = isLeaf && e0, to1 = isLeaf && !e0 && e1, to2 = isLeaf && !e0 && !e1 && e2;
                pend = to0 ? cur : pend; pend1 = to1 ? cur : pend1; pend2 = to2 ? cur : pend2;
                cur = (to0 || to1 || to2) ? BVH_EMPTY : cur;
            }
            if (cur == BVH_EMPTY) {
                T8_EVENT(6, true);
                while (sp > 0u) {
                    T8_EVENT(7, true);
                    sp--;
                    uint2 e;
                    if (sp < BVH8_STACK) e = stack[sp];
                    else {
                        unsigned long long w = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long*>(spill_slot(sp)));
                        e = make_uint2((uint)w, (uint)(w >> 32));
                    }
                    if (ANYHIT || __uint_as_float(e.y) <= bestT) { cur = e.x; break; }
                }
                if (cur == BVH_EMPTY && pend == BVH_EMPTY) {          // nothing left: report
                    if (COUNT && h == 0u && ctr.rayIterHist) {
                        if (rayIters > 2048u) { uint k = atomicAdd(ctr.longRayCount, 1u); if (k < 32u) { float* r = ctr.longRays + 8u * k; r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = Sx; r[4] = Sy; r[5] = __uint_as_float(axes); r[6] = (float)rayIters; r[7] = __uint_as_float(tag); } }
                        if (rayIters >= 128u) { uint bin = 31u - (uint)__clz((int)rayIters); atomicAdd(&ctr.rayIterHist[bin < 15u ? bin : 15u], 1ull); }
                    }
                    if (TASKS) {
                        if (ANYHIT) { /* visible sub-tree: nothing to report */ }
                        else if (h == 0u && (bestPrim != taskPrim0 || bestT != taskT0)) { HitInfo hh; hh.t = bestT; hh.prim = bestPrim; hh.u = hh.v = 0.f; commit(tag, hh); }
                    }
                    else if (ANYHIT) { if (h == 0u) { HitInfo hh; hh.t = tmax; hh.prim = 0xFFFFFFFFu; hh.u = hh.v = 0.f; commit(tag, hh); } }
                    else t8_report_closest(tag, h, bestT, bestPrim, minePrim, mineUV, commit);
                    active = false;
                }
            }
        }
        if (COUNT) { unsigned long long tc4 = __builtin_readcyclecounter(); ctr.cyc[0] += tc1 - tc0; ctr.cyc[1] += tc2 - tc1; ctr.cyc[2] += tc3 - tc2; ctr.cyc[3] += tc4 - tc3; }
        }       // run
    }
    if (CAN_SPLIT && splitNow)
    // ---- every ray still in flight becomes a list of sub-tree tasks: node slot, postponed leaves, stack entries
    {
        const uint nSlots = (cur != BVH_EMPTY ? 1u : 0u) + (pend != BVH_EMPTY ? 1u : 0u) + (pend1 != BVH_EMPTY ? 1u : 0u) + (pend2 != BVH_EMPTY ? 1u : 0u);
        const uint n = active ? nSlots + sp : 0u;
        if (DEFER) { if (active && h == 0u) publish(tag, bestT, bestPrim); return; }
        uint base = 0u;
        if (h == 0u && n) base = atomicAdd(taskOut.count, n);
        base = dpp_u<DPP_PAIR_LO>(base);
        const bool fits = n && (base + n <= taskOut.capacity);
        if (active && !fits && h == 0u) atomicOr(overflowFlag, 2u);
        if (active && fits) {
            uint* tq = reinterpret_cast<uint*>(taskOut.tasks);
            if (h == 0u) {
                uint k = base;
                if (cur != BVH_EMPTY) { tq[4u * k] = tag; tq[4u * k + 1u] = cur; tq[4u * k + 2u] = 0u; k++; }
                if (pend != BVH_EMPTY) { tq[4u * k] = tag; tq[4u * k + 1u] = pend; tq[4u * k + 2u] = 0u; k++; }
                if (pend1 != BVH_EMPTY) { tq[4u * k] = tag; tq[4u * k + 1u] = pend1; tq[4u * k + 2u] = 0u; k++; }
                if (pend2 != BVH_EMPTY) { tq[4u * k] = tag; tq[4u * k + 1u] = pend2; tq[4u * k + 2u] = 0u; k++; }
                publish(tag, bestT, bestPrim);
            }
            for (uint i = h; i < sp; i += T8_LANES) {
                uint2 e;
                if (i < BVH8_STACK) e = stack[i];
                else { unsigned long long w = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long*>(sc.travSpill + ((size_t)(blockIdx.x * T8_GROUPS_PER_BLOCK + grp) * T8_SPILL_DEPTH + (i - BVH8_STACK)))); e = make_uint2((uint)w, (uint)(w >> 32)); }
                const uint k = base + nSlots + i;
                tq[4u * k] = tag; tq[4u * k + 1u] = e.x; tq[4u * k + 2u] = e.y;
            }
        }
    }
}

} // namespace ptk

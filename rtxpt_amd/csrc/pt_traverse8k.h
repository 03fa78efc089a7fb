// mi355pt — BVH8 traversal of camera rays as PACKETS: the 32 rays of a wave walk the tree together on ONE stack. The lane-pair layout of pt_traverse8p.h stays — lane h of
// a pair tests children 4h .. 4h + 3 of the current node and triangle h of a leaf, for the pair's own ray — but the current node, the stack and the stack pointer are
// wave-uniform, so a step has no child ranking per ray, no per-ray stack, no pop loop and no refill.
//
// Why the result is the single-ray kernel's, bit for bit: the closest hit is the minimum of (t, primitive) over the triangles a ray ACCEPTS, and acceptance is a property of
// the ray and the triangle alone (the watertight test, tri_box_accepts, the alpha test: pt_scene.h) — the tree only decides which triangles are looked at. What decides
// acceptance (t8_leaf_block), and the slab test that decides what a ray enters (t8_slab on t8_ray_frame's and t8_slab_selectors' values), are the functions of
// pt_traverse8.h that traverse8_pairs calls, on the same operands: the same function, not the same expression restated. A packet looks at a SUPERSET of what each of its
// rays would look at alone:
//  - a child is visited if ANY ray's own slab test (against its own best t) enters it;
//  - a stack entry carries the MINIMUM entry distance over the rays that entered it, and is dropped unvisited only if that exceeds the LARGEST best t of the packet — then
//    every ray that entered it would have dropped it (its own entry distance is no smaller, its own best t no larger);
//  - a leaf's triangles are tested by every ray of the packet.
// Order and pruning change cost, never results.
//
// A packet that needs more than `stepCap` steps, or a deeper stack than `stackBound`, commits nothing: its rays go to a leftover list (one atomic per packet) that the
// per-ray kernel traces from scratch behind this launch (pt_wavefront.hip launch_extend_first).
//
// Two traversers: traverse8_packets (32 rays, the lane-pair layout described above) and, further down, traverse8_packets64 (64 rays, one lane per ray, the uniform part
// of a step in scalar registers), which the frame uses by default (MI355PT_FIRST_VERTEX_PACKETS, pt_context.h) — with a test of each child against the packet as a whole in
// front of the per-ray slab tests (MI355PT_PACKET_PRECULL, pt_packet_precull.h).
#pragma once
#include "pt_traverse8p.h"
#include "pt_wavefront.h"
#include "pt_packet_precull.h"

namespace ptk {

#define DPP_ROW_ROR(n) (0x120 + (n))
__device__ __forceinline__ uint t8k_min(uint a, uint b) { return a < b ? a : b; }
__device__ __forceinline__ uint t8k_max(uint a, uint b) { return a > b ? a : b; }
__device__ __forceinline__ uint t8k_uniform(uint v) { return (uint)__builtin_amdgcn_readfirstlane((int)v); }

// Ray: void form(uint i, float3& o, float3& d) — ray i of the launch (every lane of a pair forms its pair's ray). Dst: void commit(uint i, const HitInfo&), one lane per ray.
template <class Ray, class Dst>
__device__ __forceinline__ void traverse8_packets(const DeviceScene& sc, const uint count, uint2* stackBase, float2* mineUV, Ray form, Dst commit, const FirstPackets pk, uint* overflowFlag) {
    static_assert(T8_LANES == 2u, "traverse8_packets keeps the lane-pair layout");
    const uint lane = threadIdx.x & 63u, h = lane & 1u;
    const uint wavesPerBlock = T8_BLOCK / 64u;
    const uint waveId = t8k_uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), numWaves = t8k_uniform(gridDim.x * wavesPerBlock);
    uint2* stack = stackBase + t8k_uniform(threadIdx.x >> 6) * T8_PACKET_STACK;
    const char* nodesBase = reinterpret_cast<const char*>(sc.nodes8);
    const char* trisBase = reinterpret_cast<const char*>(sc.tris);
    const uint laneChildOff = 16u + 48u * h;
    const uint INF_BITS = 0x7F800000u;
    const float tmin = 0.f, tmax = kMaxRayTravel;
    // after the reduction over the packet, lane L answers for ONE child: 4h + kSel (a row of sixteen lanes holds every child twice)
    const uint kSel = (lane >> 1) & 3u, myChild = 4u * h + kSel;
    const uint stepCap = t8k_uniform(pk.stepCap), stackBound = t8k_uniform(pk.stackBound < T8_PACKET_STACK ? pk.stackBound : T8_PACKET_STACK);
    const uint numPackets = (count + T8_PACKET_RAYS - 1u) / T8_PACKET_RAYS;

    for (uint p = waveId; p < numPackets; p += numWaves) {
        const uint i0 = p * T8_PACKET_RAYS, i = i0 + (lane >> 1);
        const bool valid = i < count;      // (the launch's last packet may be short: its idle pairs form the last ray and enter nothing)
        float3 o; float Sx, Sy, ix, iy, iz; uint axes, selN, selF;
        {   float3 rd; form(valid ? i : count - 1u, o, rd); t8_ray_frame(rd, ix, iy, iz, Sx, Sy, axes); t8_slab_selectors(ix, iy, iz, selN, selF); }
        // (an idle pair's best t is negative: its slab intervals are empty, it enters nothing, and no triangle is tested for it)
        float bestT = valid ? tmax : -1.0f; uint bestPrim = 0xFFFFFFFFu, minePrim = 0xFFFFFFFFu;
        // wave-uniform: the node in hand, the stack pointer, the steps so far, the largest best t of the packet (as bits: t > 0)
        uint cur = sc.rootIsValid ? 0u : BVH_EMPTY, sp = 0u, steps = 0u, maxBest = __float_as_uint(tmax);
        bool handOff = false;

        for (;;) {
            if (cur == BVH_EMPTY) {
                while (sp > 0u) {
                    sp--;
                    const uint2 e = stack[sp];
                    const uint er = t8k_uniform(e.x), et = t8k_uniform(e.y);
                    if (__uint_as_float(et) <= __uint_as_float(maxBest)) { cur = er; break; }
                }
                if (cur == BVH_EMPTY) break;
            }
            if (++steps > stepCap) { handOff = true; break; }

            if (!(cur & BVH_LEAF_BIT)) {
                // ---- inner node: lane h tests children 4h .. 4h + 3 for its pair's ray
                const uint nodeOff = cur * 128u;
                const u32x4 hdr = *reinterpret_cast<const u32x4*>(nodesBase + nodeOff);
                const u32x4 c0 = *reinterpret_cast<const u32x4*>(nodesBase + (nodeOff + laneChildOff));
                const u32x4 c1 = *reinterpret_cast<const u32x4*>(nodesBase + (nodeOff + laneChildOff + 16u));
                const u32x4 c2 = *reinterpret_cast<const u32x4*>(nodesBase + (nodeOff + laneChildOff + 32u));
                const f32x4 scl = *reinterpret_cast<const f32x4*>(nodesBase + (nodeOff + 112u));
                const float nx = __uint_as_float(hdr.x), ny = __uint_as_float(hdr.y), nz = __uint_as_float(hdr.z);
                const float sx = scl.x, sy = scl.y, sz = scl.z;
                auto slab = [&](uint q0, uint q1, float& tn, float& tf) { t8_slab(q0, q1, selN, selF, nx, ny, nz, sx, sy, sz, o.x, o.y, o.z, ix, iy, iz, tmin, bestT, tn, tf); };
                const uint ref[4] = {c0.x, c0.w, c1.z, c2.y};
                // a ray's key for a child: its entry distance (tn >= 0: the bits order like the value; the sign is cleared with the index bits, so a -0 is a 0), +inf
                // where the ray does not enter
                uint key[4];
                {   float tn, tf;
                    slab(c0.y, c0.z, tn, tf); key[0] = T8_HIT(ref[0], tn, tf) ? (__float_as_uint(tn) & 0x7FFFFFF8u) : INF_BITS;
                    slab(c1.x, c1.y, tn, tf); key[1] = T8_HIT(ref[1], tn, tf) ? (__float_as_uint(tn) & 0x7FFFFFF8u) : INF_BITS;
                    slab(c1.w, c2.x, tn, tf); key[2] = T8_HIT(ref[2], tn, tf) ? (__float_as_uint(tn) & 0x7FFFFFF8u) : INF_BITS;
                    slab(c2.z, c2.w, tn, tf); key[3] = T8_HIT(ref[3], tn, tf) ? (__float_as_uint(tn) & 0x7FFFFFF8u) : INF_BITS;
                }
                // the minimum over the eight pairs of a row of sixteen lanes; every exchange keeps the lane's parity, so a lane goes on holding children 4h .. 4h + 3
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    key[k] = t8k_min(key[k], dpp_u<DPP_QP_XOR2>(key[k]));
                    key[k] = t8k_min(key[k], dpp_u<DPP_ROW_ROR(4)>(key[k]));
                    key[k] = t8k_min(key[k], dpp_u<DPP_ROW_ROR(8)>(key[k]));
                }
                // my child's, then over the four rows (lane positions are kept: v_permlane16_swap, v_permlane32_swap)
                uint mk = kSel == 0u ? key[0] : (kSel == 1u ? key[1] : (kSel == 2u ? key[2] : key[3]));
                const uint mref = kSel == 0u ? ref[0] : (kSel == 1u ? ref[1] : (kSel == 2u ? ref[2] : ref[3]));
                {   auto r = __builtin_amdgcn_permlane16_swap(mk, mk, false, false); mk = t8k_min(r[0], r[1]); }
                {   auto r = __builtin_amdgcn_permlane32_swap(mk, mk, false, false); mk = t8k_min(r[0], r[1]); }
                const bool hitC = mk < INF_BITS && mref != BVH_EMPTY;      // (an empty slot is an inverted box, which nothing enters: pt_traverse8.h T8_EMPTY_SLOT_CHECK)
                mk |= myChild;      // unique keys: ties to the lower child
                // rank = children with a smaller key: rotations by 1 .. 7 within the row bring each of the other seven once
                uint rank = 0u;
                rank += (dpp_u<DPP_ROW_ROR(1)>(mk) < mk) ? 1u : 0u; rank += (dpp_u<DPP_ROW_ROR(2)>(mk) < mk) ? 1u : 0u; rank += (dpp_u<DPP_ROW_ROR(3)>(mk) < mk) ? 1u : 0u;
                rank += (dpp_u<DPP_ROW_ROR(4)>(mk) < mk) ? 1u : 0u; rank += (dpp_u<DPP_ROW_ROR(5)>(mk) < mk) ? 1u : 0u; rank += (dpp_u<DPP_ROW_ROR(6)>(mk) < mk) ? 1u : 0u;
                rank += (dpp_u<DPP_ROW_ROR(7)>(mk) < mk) ? 1u : 0u;
                const uint hitMask = (uint)t8_ballot(hitC) & 0xFFu;
                uint next = BVH_EMPTY;
                if (hitMask) {
                    const uint nhit = (uint)__popc(hitMask);
                    const uint nearMask = (uint)t8_ballot(hitC && rank == 0u) & 0xFFu;
                    next = (uint)__builtin_amdgcn_readlane((int)mref, (int)(__ffs((int)nearMask) - 1));
                    if (nhit > 1u) {
                        if (sp + nhit - 1u > stackBound) { handOff = true; break; }
                        if (lane < 8u && hitC && rank > 0u) stack[sp + (nhit - 1u - rank)] = make_uint2(mref, mk & ~7u);      // far to near: nearest on top
                        sp += nhit - 1u;
                    }
                }
                cur = next;
            } else {
                // ---- leaf: every ray of the packet tests its triangles — the shared leaf block (pt_traverse8.h t8_leaf_block), closest hit, no counters
                const T8LeafHit lh = t8_leaf_block<false, false>(sc, trisBase, cur, h, valid, o.x, o.y, o.z, ix, iy, iz, Sx, Sy, axes, tmin, tmax, bestT, bestPrim, nullptr);
                const bool cand = (lh.prim != 0xFFFFFFFFu);
                if (t8_ballot(cand) != 0ull) {
                    if (cand) { minePrim = lh.prim; mineUV[threadIdx.x] = make_float2(lh.u, lh.v); }
                    float tk = lh.t; uint pkk = lh.prim; t8_pair_min(tk, pkk);
                    if (pkk != 0xFFFFFFFFu) { bestT = tk; bestPrim = pkk; }
                    // the packet's largest best t (both lanes of a pair hold their ray's)
                    uint m = valid ? __float_as_uint(bestT) : 0u;
                    m = t8k_max(m, dpp_u<DPP_QP_XOR2>(m)); m = t8k_max(m, dpp_u<DPP_ROW_ROR(4)>(m)); m = t8k_max(m, dpp_u<DPP_ROW_ROR(8)>(m));
                    maxBest = t8k_max(t8k_max((uint)__builtin_amdgcn_readlane((int)m, 0), (uint)__builtin_amdgcn_readlane((int)m, 16)),
                                      t8k_max((uint)__builtin_amdgcn_readlane((int)m, 32), (uint)__builtin_amdgcn_readlane((int)m, 48)));
                }
                cur = BVH_EMPTY;
            }
        }

        if (handOff) {
            // nothing is committed: the packet's rays are traced again, one by one
            const uint n = (count - i0 < T8_PACKET_RAYS) ? count - i0 : T8_PACKET_RAYS;
            uint base = 0u;
            if (lane == 0u) base = atomicAdd(pk.leftoverCount, n);
            base = t8k_uniform(base);
            if (base + n <= pk.capacity) { if (valid && h == 0u) pk.leftover[base + (lane >> 1)] = i; }
            else if (lane == 0u) atomicOr(overflowFlag, 2u);
        } else if (valid) {
            t8_report_closest(i, h, bestT, bestPrim, minePrim, mineUV, commit);
        }
    }
}

// ---- 64-ray packets, ONE LANE PER RAY: lane L of a wave holds ray 64 p + L of packet p (at 4 spp: two rows of an 8 x 8 block of the owned-pixel list), forms it once, tests
// all eight children of the node in hand and both triangles of a leaf for it, and reports its own hit — no pair, no hand-off of barycentrics through LDS. What is wave-uniform
// lives in scalar registers: the node's 128 bytes (scalar loads; T8_PACKET64_VECTOR_NODE: vector loads at a uniform address, the A/B partner), the per-child minimum of the
// entry-distance keys (reduced over the wave only for a child whose ballot of "some ray enters" is non-zero), the order of the entered children (a sorting network of scalar
// min / max on the unique keys distance | child), the stack pointer, the step count, the packet's largest best t.
//
// The three invariants above hold as they do for traverse8_packets, and the result is bit for bit the single-ray kernel's for the same reason:
//  - a child is visited if ANY ray's own slab test enters it: its bit of the hit mask is the ballot of T8_HIT over the lanes, each on its own t8_slab interval;
//  - a stack entry carries a value no larger than any entering ray's entry distance: the wave minimum of the entering lanes' keys with the three index bits cleared;
//  - an entry is dropped unvisited only when that value exceeds the largest best t over the packet's valid rays (maxBest, taken over the valid lanes after every leaf that
//    produced a candidate).
// The slab test, the ray frame, the selectors and the leaf block are pt_traverse8.h's functions on the same operands; the leaf block runs once as lane h = 0 and once as lane
// h = 1 of a pair, and the second call's candidate has to beat the first's in the order (t, primitive): the pair's minimum.
#ifndef T8_PACKET64_MIN_BLOCKS
#define T8_PACKET64_MIN_BLOCKS 7   // waves per SIMD the register allocator leaves room for in the 64-ray packet kernels (72 VGPRs; at 8 / 64 VGPRs it spills eight registers, some inside the leaf step)
#endif
#ifndef T8_PACKET64_VECTOR_NODE
#define T8_PACKET64_VECTOR_NODE 0
#endif
typedef uint u32x16 __attribute__((ext_vector_type(16)));
#if T8_PACKET64_VECTOR_NODE
typedef const u32x16* T8kNodeHalf;
#else
typedef const __attribute__((address_space(4))) u32x16* T8kNodeHalf;      // constant address space: s_load_dwordx16 (the tree is not written while a frame is traced)
#endif
// the minimum / maximum of v over the wave, as a scalar: four exchanges within a row of sixteen lanes (every lane then holds its row's value), lane 15 of rows 0 and 2 to
// rows 1 and 3 (row_bcast:15), lane 31 to rows 2 and 3 (row_bcast:31) — lane 63 holds the wave's. The rows a broadcast does not write get the operation's identity.
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143
template <int CTRL, int ROWS> __device__ __forceinline__ uint t8k_dpp_rows(uint v, uint identity) { return (uint)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROWS, 0xF, false); }
__device__ __forceinline__ uint t8k_wave_min(uint v) {
    v = t8k_min(v, dpp_u<DPP_QP_XOR1>(v)); v = t8k_min(v, dpp_u<DPP_QP_XOR2>(v)); v = t8k_min(v, dpp_u<DPP_ROW_ROR(4)>(v)); v = t8k_min(v, dpp_u<DPP_ROW_ROR(8)>(v));
    v = t8k_min(v, t8k_dpp_rows<DPP_ROW_BCAST15, 0xA>(v, 0xFFFFFFFFu)); v = t8k_min(v, t8k_dpp_rows<DPP_ROW_BCAST31, 0xC>(v, 0xFFFFFFFFu));
    return (uint)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint t8k_wave_max(uint v) {
    v = t8k_max(v, dpp_u<DPP_QP_XOR1>(v)); v = t8k_max(v, dpp_u<DPP_QP_XOR2>(v)); v = t8k_max(v, dpp_u<DPP_ROW_ROR(4)>(v)); v = t8k_max(v, dpp_u<DPP_ROW_ROR(8)>(v));
    v = t8k_max(v, t8k_dpp_rows<DPP_ROW_BCAST15, 0xA>(v, 0u)); v = t8k_max(v, t8k_dpp_rows<DPP_ROW_BCAST31, 0xC>(v, 0u));
    return (uint)__builtin_amdgcn_readlane((int)v, 63);
}
// eight wave-uniform keys into ascending order: the 19 compare-exchanges of the optimal 8-input network, each a scalar min and a scalar max
__device__ __forceinline__ void t8k_sort8(uint (&s)[8]) {
#define T8K_CE(a, b) { const uint lo_ = t8k_min(s[a], s[b]), hi_ = t8k_max(s[a], s[b]); s[a] = lo_; s[b] = hi_; }
    T8K_CE(0, 2) T8K_CE(1, 3) T8K_CE(4, 6) T8K_CE(5, 7)
    T8K_CE(0, 4) T8K_CE(1, 5) T8K_CE(2, 6) T8K_CE(3, 7)
    T8K_CE(0, 1) T8K_CE(2, 3) T8K_CE(4, 5) T8K_CE(6, 7)
    T8K_CE(2, 4) T8K_CE(3, 5)
    T8K_CE(1, 4) T8K_CE(3, 6)
    T8K_CE(1, 2) T8K_CE(3, 4) T8K_CE(5, 6)
#undef T8K_CE
}

// a float as a uint that orders like it (negative values below positive ones), and back: the wave minimum / maximum of floats through t8k_wave_min / t8k_wave_max
__device__ __forceinline__ uint t8k_float_key(float f) { const uint b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float t8k_key_float(uint k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ float t8k_wave_fmin(float v) { return t8k_key_float(t8k_wave_min(t8k_float_key(v))); }
__device__ __forceinline__ float t8k_wave_fmax(float v) { return t8k_key_float(t8k_wave_max(t8k_float_key(v))); }

// PRECULL (MI355PT_PACKET_PRECULL, FirstPackets::precull): before the eight per-ray slab tests of a node step, lane c < 8 tests child c against the packet as a whole
// (pt_packet_precull.h: the intervals of the rays' origins and reciprocals, formed once per packet and kept in the wave's sixteen words of LDS at `intervalBase`), and the
// per-ray test of a child runs only under a scalar branch on its bit of the ballot. The interval test drops a child only if NO ray's own T8_HIT can be true, so the hit mask,
// the keys, the order and the pushes — and with them the three invariants above — are what they are without it. A packet whose rays' reciprocals have both signs on an axis has
// no test: every child is kept.
// Ray: void form(uint i, float3& o, float3& d) — ray i of the launch, formed once, by the lane that holds it. Dst: void commit(uint i, const HitInfo&), by the same lane.
template <bool PRECULL, class Ray, class Dst>
__device__ __forceinline__ void traverse8_packets64(const DeviceScene& sc, const uint count, uint2* stackBase, float* intervalBase, Ray form, Dst commit, const FirstPackets pk, uint* overflowFlag) {
    const uint lane = threadIdx.x & 63u;
    const uint wavesPerBlock = T8_BLOCK / 64u;
    const uint waveId = t8k_uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), numWaves = t8k_uniform(gridDim.x * wavesPerBlock);
    uint2* stack = stackBase + t8k_uniform(threadIdx.x >> 6) * T8_PACKET_STACK;
    float* interval = PRECULL ? intervalBase + t8k_uniform(threadIdx.x >> 6) * T8_PACKET_INTERVAL_WORDS : nullptr;
    const char* nodesBase = reinterpret_cast<const char*>(sc.nodes8);
    const char* trisBase = reinterpret_cast<const char*>(sc.tris);
    const uint INF_BITS = 0x7F800000u;
    const float tmin = 0.f, tmax = kMaxRayTravel;
    // lane k < 8 fetches child k's reference (a child is twelve bytes from byte 16 of the node: reference, six plane bytes, two spare); v_readlane picks one by child index
    const uint refOff = 16u + 12u * (lane & 7u);
    const uint stepCap = t8k_uniform(pk.stepCap), stackBound = t8k_uniform(pk.stackBound < T8_PACKET_STACK ? pk.stackBound : T8_PACKET_STACK);
    const uint numPackets = (count + T8_PACKET64_RAYS - 1u) / T8_PACKET64_RAYS;

    for (uint p = waveId; p < numPackets; p += numWaves) {
        const uint i0 = p * T8_PACKET64_RAYS, i = i0 + lane;
        const bool valid = i < count;      // (the launch's last packet may be short: its idle lanes form the last ray and enter nothing)
        float3 o; float Sx, Sy, ix, iy, iz; uint axes, selN, selF;
        {   float3 rd; form(valid ? i : count - 1u, o, rd); t8_ray_frame(rd, ix, iy, iz, Sx, Sy, axes); t8_slab_selectors(ix, iy, iz, selN, selF); }
        // (an idle lane's best t is negative: its slab intervals are empty, it enters nothing, and no triangle is tested for it)
        float bestT = valid ? tmax : -1.0f, bestU = 0.f, bestV = 0.f; uint bestPrim = 0xFFFFFFFFu;
        // wave-uniform: the node in hand, the stack pointer, the steps so far, the largest best t of the packet (as bits: t > 0)
        uint cur = sc.rootIsValid ? 0u : BVH_EMPTY, sp = 0u, steps = 0u, maxBest = __float_as_uint(tmax);
        bool handOff = false;
        // the packet's interval: every lane holds a ray of THIS packet (an idle lane the launch's last ray, which the last packet holds), so the extremes are taken over all
        // lanes, and when the signs are definite every lane's selectors are the packet's
        bool culls = false;
        if (PRECULL) {
            T8PacketInterval pi;
            culls = t8_packet_interval(t8k_wave_fmin(o.x), t8k_wave_fmin(o.y), t8k_wave_fmin(o.z), t8k_wave_fmax(o.x), t8k_wave_fmax(o.y), t8k_wave_fmax(o.z),
                                       t8k_wave_fmin(ix), t8k_wave_fmin(iy), t8k_wave_fmin(iz), t8k_wave_fmax(ix), t8k_wave_fmax(iy), t8k_wave_fmax(iz), pi);
            if (lane == 0u) {
                f32x4* dst = reinterpret_cast<f32x4*>(interval);
                dst[0] = (f32x4){pi.oNx, pi.oNy, pi.oNz, pi.oFx}; dst[1] = (f32x4){pi.oFy, pi.oFz, pi.iLox, pi.iLoy}; dst[2] = (f32x4){pi.iLoz, pi.iHix, pi.iHiy, pi.iHiz};
            }
        }

        for (;;) {
            if (cur == BVH_EMPTY) {
                while (sp > 0u) {
                    sp--;
                    const uint2 e = stack[sp];
                    const uint er = t8k_uniform(e.x), et = t8k_uniform(e.y);
                    if (et <= maxBest && er != BVH_EMPTY) { cur = er; break; }      // (both are the bits of floats >= +0: they order like the values; an empty slot's reference is skipped)
                }
                if (cur == BVH_EMPTY) break;
            }
            if (++steps > stepCap) { handOff = true; break; }
            cur = t8k_uniform(cur);      // (wave-uniform by construction; said once per step, so that the node's address and the leaf's slot are formed in scalar registers)

            if (!(cur & BVH_LEAF_BIT)) {
                // ---- inner node: every lane tests all eight children for its ray
                const uint nodeOff = cur * 128u;
                const uint vref = *reinterpret_cast<const uint*>(nodesBase + nodeOff + refOff);
                const T8kNodeHalf np = (T8kNodeHalf)(unsigned long long)(nodesBase + nodeOff);
                const u32x16 w0 = np[0], w1 = np[1];
                // (the node's origin in vector registers, once: as scalars each of the eight slab tests copies the three pairs again)
                float nx = __uint_as_float(w0[0]), ny = __uint_as_float(w0[1]), nz = __uint_as_float(w0[2]);
                asm volatile("" : "+v"(nx), "+v"(ny), "+v"(nz));
                const float sx = __uint_as_float(w1[12]), sy = __uint_as_float(w1[13]), sz = __uint_as_float(w1[14]);
                // child k's plane bytes: words 5 + 3k and 6 + 3k of the node
                const uint q0[8] = {w0[5], w0[8], w0[11], w0[14], w1[1], w1[4], w1[7], w1[10]};
                const uint q1[8] = {w0[6], w0[9], w0[12], w0[15], w1[2], w1[5], w1[8], w1[11]};
                const uint ref[8] = {w0[4], w0[7], w0[10], w0[13], w1[0], w1[3], w1[6], w1[9]};
                // the children some ray may enter: lane c < 8 holds child c's plane bytes (the two words behind its reference) and tests its box against the packet's interval,
                // read at a uniform LDS address; t8_slab_planes on the lane's own selectors, which are the packet's
                uint keep = 0xFFu;
                if (PRECULL && culls) {
                    const uint vq0 = *reinterpret_cast<const uint*>(nodesBase + nodeOff + refOff + 4u), vq1 = *reinterpret_cast<const uint*>(nodesBase + nodeOff + refOff + 8u);
                    const f32x4* src = reinterpret_cast<const f32x4*>(interval);
                    const f32x4 a = src[0], b = src[1], c = src[2];
                    const T8PacketInterval pi = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
                    f32x2 px, py, pz; t8_slab_planes(vq0, vq1, selN, selF, nx, ny, nz, sx, sy, sz, px, py, pz);
                    keep = (uint)t8_ballot(t8_packet_keeps(px.x, px.y, py.x, py.y, pz.x, pz.y, pi, tmin, __uint_as_float(maxBest))) & 0xFFu;
                }
                // a child's key: the minimum over the rays that enter it of the entry distance (tn >= 0: the bits order like the value; the sign is cleared with the index
                // bits, so a -0 is a 0), then the child index in the low bits (unique keys, ties to the lower child); +inf for a child that nothing enters
                uint sk[8]; uint nhit = 0u;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    uint mk = INF_BITS;
                    if (!PRECULL || ((keep >> k) & 1u)) {
                        float tn, tf;
                        t8_slab(q0[k], q1[k], selN, selF, nx, ny, nz, sx, sy, sz, o.x, o.y, o.z, ix, iy, iz, tmin, bestT, tn, tf);
                        const bool hit = T8_HIT(ref[k], tn, tf);      // (an empty slot is an inverted box, which nothing enters: pt_traverse8.h T8_EMPTY_SLOT_CHECK)
                        if (t8_ballot(hit) != 0ull) { mk = t8k_wave_min(hit ? (__float_as_uint(tn) & 0x7FFFFFF8u) : INF_BITS); nhit++; }
                    }
                    sk[k] = mk | (uint)k;
                }
                uint next = BVH_EMPTY;
                if (nhit == 1u) {
                    const uint m = t8k_min(t8k_min(t8k_min(sk[0], sk[1]), t8k_min(sk[2], sk[3])), t8k_min(t8k_min(sk[4], sk[5]), t8k_min(sk[6], sk[7])));
                    next = (uint)__builtin_amdgcn_readlane((int)vref, (int)(m & 7u));
                } else if (nhit > 1u) {
                    if (sp + nhit - 1u > stackBound) { handOff = true; break; }
                    t8k_sort8(sk);
                    next = (uint)__builtin_amdgcn_readlane((int)vref, (int)(sk[0] & 7u));
                    // far to near: nearest on top. One lane writes; the entries are wave-uniform
#pragma unroll
                    for (int r = 1; r < 8; r++) {
                        if ((uint)r < nhit) { const uint ref = (uint)__builtin_amdgcn_readlane((int)vref, (int)(sk[r] & 7u)); if (lane == 0u) stack[sp + (nhit - 1u - (uint)r)] = make_uint2(ref, sk[r] & ~7u); }
                    }
                    sp += nhit - 1u;
                }
                cur = next;      // (a reference of BVH_EMPTY — a node of zero extent "entering" an empty slot — pops; the pop loop skips such an entry)
            } else {
                // ---- leaf: every ray of the packet tests both triangles — the shared leaf block (pt_traverse8.h t8_leaf_block), once as each lane of a pair
                bool cand = false;
#pragma unroll 1
                for (uint h = 0; h < 2u; h++) {
                    const T8LeafHit lh = t8_leaf_block<false, false>(sc, trisBase, cur, h, valid, o.x, o.y, o.z, ix, iy, iz, Sx, Sy, axes, tmin, tmax, bestT, bestPrim, nullptr);
                    if (lh.prim != 0xFFFFFFFFu) { bestT = lh.t; bestPrim = lh.prim; bestU = lh.u; bestV = lh.v; cand = true; }
                }
                if (t8_ballot(cand) != 0ull) maxBest = t8k_wave_max(valid ? __float_as_uint(bestT) : 0u);
                cur = BVH_EMPTY;
            }
        }

        if (handOff) {
            // nothing is committed: the packet's rays are traced again, one by one
            const uint n = (count - i0 < T8_PACKET64_RAYS) ? count - i0 : T8_PACKET64_RAYS;
            uint base = 0u;
            if (lane == 0u) base = atomicAdd(pk.leftoverCount, n);
            base = t8k_uniform(base);
            if (base + n <= pk.capacity) { if (valid) pk.leftover[base + lane] = i; }
            else if (lane == 0u) atomicOr(overflowFlag, 2u);
        } else if (valid) {
            HitInfo hh; hh.t = bestT; hh.prim = bestPrim; hh.u = bestU; hh.v = bestV; commit(i, hh);
        }
    }
}

} // namespace ptk

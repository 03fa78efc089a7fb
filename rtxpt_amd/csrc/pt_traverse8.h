// mi355pt — cooperative BVH8 traversal for wave64: what the traversers (pt_traverse8p.h: two lanes per ray, 32 rays per wave; pt_traverse8k.h: the same 32 rays as a packet on one
// stack) share with each other and with their callers — counters, tuning constants, DPP helpers, the description of the template interface, and the ONE text of the slab test
// and of the hit definition (ray frame, leaf block with the watertight test, the candidate's box test and the alpha test, the pair's minimum, the closest-hit report): a
// traverser gets them by calling them. Replaces RayQuery::TraceRayInline / the DXR any-hit visibility query (PathTracerBridgeDonut.hlsli:993-1055). Results are
// traversal-order free (min t, ties to the lower primitive id).
//
// How the shape was arrived at on MI355X (profiles/r01a_*, r01b_*, r03s_*):
//  * one ray per lane over BVH2 was bound by divergent 16-byte gathers through the per-CU texture-address path (33 % L2 misses but only
//    ~0.4 TB/s of HBM traffic): 4 line lookups per lane per node. Cooperative 128 B nodes cut line lookups per ray by ~6-9x.
//  * 8 lanes per ray / 1 child per lane then turned out VALU-issue bound: every per-ray scalar (addresses, stack, control) is replicated over the lanes of its
//    group, so the cure is fewer lanes per ray: 4 lanes x 2 children per lane (rounds 1-3), then 2 lanes x 4 children (round 3 on; the four-lane kernel is in the history).
#pragma once
#include <hip/hip_runtime.h>
#include "pt_scene.h"

namespace ptk {

struct Traverse8Counters { uint nodeVisits, triTests, leafVisits, iters, leafBlocks; uint ev[8]; unsigned long long cyc[4]; unsigned long long* rayIterHist; uint* longRayCount; float* longRays; };

#define T8_EVENT(k, cond) do { if (COUNT) { unsigned long long m_ = t8_ballot(cond); if (m_ && lane == (uint)__ffsll((long long)m_) - 1u) ctr.ev[k]++; } } while (0)
static const uint T8_RAY_STRIDE = 13, T8_TASK_STRIDE = 15;      // origin, shear + axes, tag, interval (fixed-range launches: the slab test's byte selectors) | best hit, (task: best primitive, start node,) the three reciprocals                                              // per-wave LDS parking lot for a chunk's rays / tasks (odd strides)
static const uint T8_RAYBUF_WORDS = (T8_BLOCK / 64u) * T8_CHUNK * T8_RAY_STRIDE, T8_TASKBUF_WORDS = (T8_BLOCK / 64u) * T8_CHUNK * T8_TASK_STRIDE;
static const uint T8_LEAF_ROUNDS = (BVH_MAX_LEAF + T8_LANES - 1u) / T8_LANES;

#ifndef T8_EXTEND_MIN_BLOCKS
#define T8_EXTEND_MIN_BLOCKS 7   // waves per SIMD the register allocator must leave room for in k_extend (64 VGPRs, 2 spilled outside the loop): 6 -> 7 -> 8 waves were
                                  // 1161 -> 1187 -> 1239 Mrays/s in round 2 (profiles/r02n_occupancy_ab.txt). At 8 waves the loop is VALU-issue bound (round 3: extra v_nop
                                  // slots lengthen it one for one, profiles/r03i_valu_bound_probe.txt): from here on instructions per ray count, not waves in flight
#endif
#ifndef T8_SHADOW_MIN_WAVES
#define T8_SHADOW_MIN_WAVES 7    // the same for k_shadow
#endif
#ifndef T8_TAIL_ITERS
#define T8_TAIL_ITERS 32         // loop iterations a wave keeps going after its last chunk before it splits what is still in flight into tasks
#endif
#ifndef T8_TAIL_ITERS_TASKS
#define T8_TAIL_ITERS_TASKS 8    // the same for task rounds: sub-trees are short, and every round of every launch pays this tail once
#endif
#ifndef T8_ANYHIT_UNORDERED
#define T8_ANYHIT_UNORDERED 1     // 1: occlusion queries number a node's hit children by child index instead of ranking them by entry distance
#endif
#ifndef T8_LEAF_QUEUE
#define T8_LEAF_QUEUE 3        // postponed leaves a ray may hold (1..3) before it has to wait for the wave's next leaf block (A/B: within noise on extend, -4 % on shadow)
#endif

// the ray's reciprocal direction is the correctly rounded one of the hit definition (pt_scene.h tri_box_accepts): inner nodes and the triangle's own
// box are then tested with the same arithmetic, which is what makes the closest hit independent of the tree (three divisions per ray, not per node)
__device__ __forceinline__ float t8_rcp_dir(float d) { return ray_safe_rcp(d); }
// tri_box_accepts (pt_scene.h) with the hardware's min/max (v_min3/v_max3 instead of compare + select pairs), on the leaf block's operands: g0 / g1 / g2 are the record's 16-byte
// groups of the axes x / y / z (three coordinates each, one per vertex), o* and i* the ray's origin and reciprocal direction. The operands are finite here —
// the triangle test has already accepted the triangle, so neither the ray nor the vertices hold a NaN — and on finite operands minNum / maxNum differ from `(a < b) ? a : b` only
// in the sign of a zero, which no comparison below can see; the maximum / minimum over the three axes does not depend on their order: same boolean as tri_box_accepts, bit for bit.
__device__ __forceinline__ bool t8_tri_box_accepts(f32x4 g0, f32x4 g1, f32x4 g2, float pad, float okx, float oky, float okz, float ikx, float iky, float ikz, float t) {
    const float mnx = fminf(g0.x, fminf(g0.y, g0.z)) - pad, mny = fminf(g1.x, fminf(g1.y, g1.z)) - pad, mnz = fminf(g2.x, fminf(g2.y, g2.z)) - pad;
    const float mxx = fmaxf(g0.x, fmaxf(g0.y, g0.z)) + pad, mxy = fmaxf(g1.x, fmaxf(g1.y, g1.z)) + pad, mxz = fmaxf(g2.x, fmaxf(g2.y, g2.z)) + pad;
    const float ax = (mnx - okx) * ikx, bx = (mxx - okx) * ikx, ay = (mny - oky) * iky, by = (mxy - oky) * iky, az = (mnz - okz) * ikz, bz = (mxz - okz) * ikz;
    const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    return (tn <= t) && (t <= tf);
}
__device__ __forceinline__ unsigned long long t8_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }   // v_cmp straight into an SGPR pair
// In-quad data exchange with DPP quad permutes only — no LDS crossbar (ds_bpermute) latency on the critical path.
#define DPP_QP_XOR1 0xB1
#define DPP_QP_XOR2 0x4E
template <int CTRL> __device__ __forceinline__ uint dpp_u(uint v) { return (uint)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) { return __uint_as_float(dpp_u<CTRL>(__float_as_uint(v))); }

// ---- The hit definition and the slab test, written once: every traverser of the BVH8 (traverse8_pairs, pt_traverse8p.h; traverse8_packets, pt_traverse8k.h) calls the functions
// below, so what a ray enters and which triangles it accepts cannot differ between them. What stays with a traverser is policy: refill, ranking, stacks, postponed leaves,
// splitting, hand-off, reductions over a packet — and a node's five loads with the four T8_HIT lines that turn a child's slab interval into the traverser's sort key: wrapped in
// a function (out-arrays, or a callable per child) they cost k_extend, k_trace_pair and the task kernels a spilled register (profiles/r17a_traversal_shared_text_ab.txt).
// The ray's origin travels as three floats: a float3 by reference costs every kernel a 16-byte stack object.

// What the leaf block needs of the direction (intersect_tri_wt, pt_scene.h), formed once per ray: ix / iy / iz = the reciprocals; kz = the axis of the largest |d| (ties to the
// lower axis), kx / ky the next two in cyclic order; Sz = the reciprocal of d[kz], Sx = d[kx] * Sz, Sy = d[ky] * Sz; axes = the byte offsets of the record groups of the ray's
// axes, kx | ky << 8 | kz << 16. The direction itself is not kept.
__device__ __forceinline__ void t8_ray_frame(const float3 rd, float& ix, float& iy, float& iz, float& Sx, float& Sy, uint& axes) {
    ix = t8_rcp_dir(rd.x); iy = t8_rcp_dir(rd.y); iz = t8_rcp_dir(rd.z);
    const float adx = fabsf(rd.x), ady = fabsf(rd.y), adz = fabsf(rd.z);
    const bool rk2 = adz > adx && adz > ady, rk1 = !rk2 && ady > adx;
    const float rSz = rk2 ? iz : (rk1 ? iy : ix);
    Sx = (rk2 ? rd.x : (rk1 ? rd.z : rd.y)) * rSz; Sy = (rk2 ? rd.y : (rk1 ? rd.x : rd.z)) * rSz;
    axes = rk2 ? (0u | (16u << 8) | (32u << 16)) : (rk1 ? (32u | (0u << 8) | (16u << 16)) : (16u | (32u << 8) | (0u << 16)));
}
// the slab test's byte selectors (v_perm_b32) for a child's near and far planes. Child bytes: q0 = lo.x lo.y lo.z hi.x (selector values 0..3), q1 = hi.y hi.z (4, 5)
__device__ __forceinline__ void t8_slab_selectors(float ix, float iy, float iz, uint& selN, uint& selF) {
    const uint nxb = ix < 0.f ? 3u : 0u, fxb = ix < 0.f ? 0u : 3u, nyb = iy < 0.f ? 4u : 1u, fyb = iy < 0.f ? 1u : 4u, nzb = iz < 0.f ? 5u : 2u, fzb = iz < 0.f ? 2u : 5u;
    selN = nxb | (nyb << 8) | (nzb << 16) | (fxb << 24); selF = fyb | (fzb << 8);
}

#ifndef T8_EMPTY_SLOT_CHECK
// 0: an empty child slot needs no test of its own — the builder writes it as an inverted box (lo = 255, hi = 0 on every axis: pt_build.hip k_collapse8),
#define T8_EMPTY_SLOT_CHECK 0
// which no ray's slab interval enters; were it ever "hit" (a node of zero extent), its reference is BVH_EMPTY, which the slot bookkeeping skips
#endif
#if T8_EMPTY_SLOT_CHECK
#define T8_HIT(ref, tn, tf) (((ref) != BVH_EMPTY) && ((tn) <= (tf) * 1.0000012f))
#else
#define T8_HIT(ref, tn, tf) ((tn) <= (tf) * 1.0000012f)
#endif
// a child's six planes in world space, (near, far) per axis by the selectors: they depend on the ray through the selectors alone, so rays with the same signs see the same
// values (what the packet's interval test, pt_packet_precull.h, relies on)
__device__ __forceinline__ void t8_slab_planes(uint q0, uint q1, uint selN, uint selF, float nx, float ny, float nz, float sx, float sy, float sz, f32x2& px, f32x2& py, f32x2& pz) {
    const uint N = __builtin_amdgcn_perm(q1, q0, selN), F = __builtin_amdgcn_perm(q1, q0, selF);
    px = __builtin_elementwise_fma((f32x2){(float)(N & 0xFFu), (float)(N >> 24)}, (f32x2){sx, sx}, (f32x2){nx, nx});
    py = __builtin_elementwise_fma((f32x2){(float)((N >> 8) & 0xFFu), (float)(F & 0xFFu)}, (f32x2){sy, sy}, (f32x2){ny, ny});
    pz = __builtin_elementwise_fma((f32x2){(float)((N >> 16) & 0xFFu), (float)((F >> 8) & 0xFFu)}, (f32x2){sz, sz}, (f32x2){nz, nz});
}
// one child's slab test: the quantised planes (q0, q1: the child's six bytes) against the ray, clipped to [tmin, bestT]; n* / s* are the node's origin and scales
__device__ __forceinline__ void t8_slab(uint q0, uint q1, uint selN, uint selF, float nx, float ny, float nz, float sx, float sy, float sz, float ox, float oy, float oz, float ix, float iy, float iz,
                                        float tmin, float bestT, float& tn, float& tf) {
    f32x2 px, py, pz; t8_slab_planes(q0, q1, selN, selF, nx, ny, nz, sx, sy, sz, px, py, pz);
    f32x2 tx = (px - (f32x2){ox, ox}) * (f32x2){ix, ix}, ty = (py - (f32x2){oy, oy}) * (f32x2){iy, iy}, tz = (pz - (f32x2){oz, oz}) * (f32x2){iz, iz};
    tn = fmaxf(fmaxf(tx.x, ty.x), fmaxf(tz.x, tmin));
    tf = fminf(fminf(tx.y, ty.y), fminf(tz.y, bestT));
}

// A lane's candidate of a leaf block: the nearest triangle it accepted (prim == ~0: none). alphaRan: counter builds only
struct T8LeafHit { float t; uint prim; float u, v; bool alphaRan; };
// ---- the leaf block: lane h of a pair tests triangle h (h + 2, ... when leaves hold more than two) of leaf `leaf` for its ray. The watertight test of pt_scene.h
// (intersect_tri_wt) on the same operands: the axis permutation (kx, ky, kz) is the ORDER in which the record's three 16-byte groups are loaded; the ray's own quantities are
// selected once per leaf block. valid: false for a lane that holds no ray (the idle pairs of a short packet): nothing is tested for it. Closest hit: a triangle is a candidate
// if it beats (bestT, bestPrim) and the lane's candidate so far in the order (t, prim); ANYHIT: any accepted triangle. ctr is used only when COUNT (else it may be null).
template <bool ANYHIT, bool COUNT>
__device__ __forceinline__ T8LeafHit t8_leaf_block(const DeviceScene& sc, const char* trisBase, const uint leaf, const uint h, const bool valid, const float ox, const float oy, const float oz,
                                                   const float ix, const float iy, const float iz, const float Sx, const float Sy, const uint axes, const float tmin, const float tmax,
                                                   const float bestT, const uint bestPrim, Traverse8Counters* ctr) {
    const uint cnt = (leaf & 7u) + 1u;
    const uint slot0 = (leaf & 0x7FFFFFFFu) >> 3;
    const uint triOff0 = slot0 * 48u + 48u * h;
    float lt = __uint_as_float(0x7F800000u), lu = 0.f, lv = 0.f; uint lp = 0xFFFFFFFFu;
    bool alphaRan = false;
    const uint gx = axes & 0xFFu, gy = (axes >> 8) & 0xFFu, gz = axes >> 16;          // byte offsets of the groups of axes kx, ky, kz
    const bool k2 = gz == 32u, k1 = gz == 16u;                                      // kz = 2 / 1 / 0
    const float okx = k2 ? ox : (k1 ? oz : oy), oky = k2 ? oy : (k1 ? ox : oz), okz = k2 ? oz : (k1 ? oy : ox);
    const float Sz = k2 ? iz : (k1 ? iy : ix);                                       // ix / iy / iz = ray_safe_rcp of the direction's components
#pragma unroll 1
    for (uint r = 0; r < T8_LEAF_ROUNDS; r++) {
        const bool doit = valid && (h + T8_LANES * r) < cnt;
        if (r > 0u && t8_ballot(doit) == 0ull) break;
        if (doit) {
            const uint toff = triOff0 + (T8_LANES * 48u) * r;      // (32-bit byte offsets from the SGPR base: global_load ... saddr)
            // twelve bytes per group (global_load_dwordx3): the fourth word is not needed here, and a 16-byte destination whose last register the
            // allocator then reuses for the next load's address makes that load wait for this one — two memory latencies in a row instead of one (seen
            // in the ISA, measured: +10 % on k_extend)
            struct __attribute__((packed, aligned(4))) f32x3p { float x, y, z; };
            const f32x3p g0 = *reinterpret_cast<const f32x3p*>(trisBase + (toff + gx)), g1 = *reinterpret_cast<const f32x3p*>(trisBase + (toff + gy)), g2 = *reinterpret_cast<const f32x3p*>(trisBase + (toff + gz));
            if (COUNT) ctr->triTests++;
            // intersect_tri_wt's arithmetic, two values per instruction where the operands already sit in neighbouring registers (vertices 0 and 1 of a
            // loaded group): packed fp32 operations round each half like the scalar ones
            const f32x2 ABkz = (f32x2){g2.x, g2.y} - (f32x2){okz, okz}; const float Ckz = g2.z - okz;
            const f32x2 ABx = __builtin_elementwise_fma((f32x2){-Sx, -Sx}, ABkz, (f32x2){g0.x, g0.y} - (f32x2){okx, okx}), ABy = __builtin_elementwise_fma((f32x2){-Sy, -Sy}, ABkz, (f32x2){g1.x, g1.y} - (f32x2){oky, oky});
            const float Cx = fmaf(-Sx, Ckz, g0.z - okx), Cy = fmaf(-Sy, Ckz, g1.z - oky);
            const float Ax = ABx.x, Bx = ABx.y, Ay = ABy.x, By = ABy.y, Akz = ABkz.x, Bkz = ABkz.y;
            const f32x2 m1 = ABx * (f32x2){Cy, Cy}, m2 = ABy * (f32x2){Cx, Cx};      // (Ax Cy, Bx Cy), (Ay Cx, By Cx)
            float V = m1.x - m2.x, U = m2.y - m1.y, W = Bx * Ay - By * Ax;            // U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax
            // on an edge or a vertex (or a degenerate triangle): the exact sign from the products' rounding errors (wt_edge)
            if (U == 0.0f || V == 0.0f || W == 0.0f) {
                if (U == 0.0f) U = fmaf(Cx, By, -(Cx * By)) - fmaf(Cy, Bx, -(Cy * Bx));
                if (V == 0.0f) V = fmaf(Ax, Cy, -(Ax * Cy)) - fmaf(Ay, Cx, -(Ay * Cx));
                if (W == 0.0f) W = fmaf(Bx, Ay, -(Bx * Ay)) - fmaf(By, Ax, -(By * Ax));
            }
            const float det = (U + V) + W;
            // no edge function negative, or none positive (pt_scene.h writes it as !((U < 0 || V < 0 || W < 0) && (U > 0 || V > 0 || W > 0)): the same
            // boolean for numbers; a NaN ends as "no hit" either way, through t); without short-circuits: v_min3, v_max3 and three compares, no branch
            const bool inside = (bool)(((int)(fminf(U, fminf(V, W)) >= 0.0f) | (int)(fmaxf(U, fmaxf(V, W)) <= 0.0f)) & (int)(det != 0.0f));
            if (inside) {
                const float T = fmaf(W, Sz * Ckz, fmaf(V, Sz * Bkz, U * (Sz * Akz)));
                const float inv = 1.0f / det;
                const float t = T * inv, u = V * inv, v = W * inv;
                if (t > tmin && t < tmax) {
                    // a candidate (about one test in six): the record again, in its own order this time — prim rides with the x group, flags with y,
                    // pad with z. Reloaded (the line is in the L1) instead of kept: twelve registers that the loop does not have — with them live
                    // across the test the kernels spill inside the loop.
                    uint off2 = toff; asm volatile("" : "+v"(off2));      // (an address the compiler cannot match with the loads above)
                    const f32x4 rx = *reinterpret_cast<const f32x4*>(trisBase + off2), ry = *reinterpret_cast<const f32x4*>(trisBase + (off2 + 16u)), rz = *reinterpret_cast<const f32x4*>(trisBase + (off2 + 32u));
                    const uint prim = __float_as_uint(rx.w), flags = __float_as_uint(ry.w);
                    bool c;
                    if (ANYHIT) {
                        c = t8_tri_box_accepts(rx, ry, rz, rz.w, ox, oy, oz, ix, iy, iz, t);
                        if (c && (flags & 1u)) { if (COUNT && !(flags & 2u)) alphaRan = true; c = !(flags & 2u) && alpha_test_slot(sc, slot0 + h + T8_LANES * r, u, v); }      // AlphaTestVisibilityRay (BridgeDonut:981-989)
                    } else {
                        c = ((t < bestT) || (t == bestT && prim < bestPrim)) && ((t < lt) || (t == lt && prim < lp));
                        if (c) c = t8_tri_box_accepts(rx, ry, rz, rz.w, ox, oy, oz, ix, iy, iz, t);
                        if (c && (flags & 1u)) { if (COUNT) alphaRan = true; c = alpha_test_slot(sc, slot0 + h + T8_LANES * r, u, v); }
                    }
                    if (c) { lt = t; lp = prim; lu = u; lv = v; }
                }
            }
        }
    }
    return T8LeafHit{lt, lp, lu, lv, alphaRan};
}
// the lexicographic minimum of (t, prim) over the two lanes of a pair: both lanes end with it
__device__ __forceinline__ void t8_pair_min(float& t, uint& prim) {
    const float ot = dpp_f<DPP_QP_XOR1>(t); const uint op = dpp_u<DPP_QP_XOR1>(prim);
    const bool take = (ot < t) || (ot == t && op < prim); t = take ? ot : t; prim = take ? op : prim;
}
// a finished ray's closest hit: a miss is reported by lane 0 of the pair, a hit by the lane that found the winning primitive (minePrim: the last candidate of this lane,
// its barycentrics parked in mineUV) — Dst::commit is called by ONE lane
template <class Dst>
__device__ __forceinline__ void t8_report_closest(uint tag, uint h, float bestT, uint bestPrim, uint minePrim, const float2* mineUV, Dst& commit) {
    if (bestPrim == 0xFFFFFFFFu) { if (h == 0u) { HitInfo hh; hh.t = bestT; hh.prim = 0xFFFFFFFFu; hh.u = hh.v = 0.f; commit(tag, hh); } }
    else if (minePrim == bestPrim) { const float2 uv = mineUV[threadIdx.x]; HitInfo hh; hh.t = bestT; hh.prim = bestPrim; hh.u = uv.x; hh.v = uv.y; commit(tag, hh); }
}

// FIXED_RANGE: every ray of the launch has tmin = 0, tmax = kMaxRayTravel (extend rays), whatever fetch() reports.
// TASKS: the work items are sub-trees of rays (TravTask) instead of whole rays: fetch() also reports the start node and the ray's best hit so far.
// CAN_SPLIT: straggler handling. One ray is a serial chain on one quad, and C3 has ~300 rays (of 10^8) that need 10^3..10^4 iterations (rays
//   running along the street inside the tree crowns): alone they kept a launch alive for up to 20 ms and cost 15-25 % of the frame and half of
//   the 8-GPU scaling. So a wave that has been out of fresh rays for T8_TAIL_ITERS iterations stops: every ray still in flight is cut into its
//   pending sub-trees (node slot, postponed leaves, stack entries), which go to a task queue together with the best hit so far (publish()),
//   and a follow-up launch spreads them over the whole GPU. The result is the minimum over all sub-trees, so nothing changes in the image.
// Src: uint fetch(uint i, float3& o, float3& d, float& tmin, float& tmax, uint& startRef, float& bestT0, uint& bestPrim0) -> user tag (e.g. path
//        index); called once per item by one lane; tmin >= 0. Rays: startRef = 0, bestT0 = tmax, bestPrim0 = ~0.
// Dst: void commit(uint tag, const HitInfo& h) ; called by ONE lane of the quad (closest: best hit or prim == ~0; any-hit: prim != ~0 when occluded)
// Pub: void publish(uint tag, float bestT, uint bestPrim) ; called by one lane for every ray that is split (CAN_SPLIT only)
// (the traversal itself: pt_traverse8p.h, two lanes per ray; the four-lane kernel of rounds 1-3 is in the history: commit af4c2b2)

} // namespace ptk

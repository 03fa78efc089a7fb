// mi355pt — the launch plan of the BVH8 traversal launches (pt_trace.hip): the launch geometry, how many blocks a launch gets, how many task rounds follow it, and how a
// fused launch splits its grid between its two kinds of ray. Integer arithmetic in plain C++ without a dependency: the launchers call it, nothing else computes a traversal
// grid, and tests/trace_plan_check.cpp holds it to its invariants on the host.
#pragma once

namespace ptk {
typedef unsigned int uint;

#define PT_T8_LANES 2             // lanes per ray in the traversal kernels (pt_traverse8p.h; the four-lane kernel of rounds 1-3 is in the history)
#ifndef PT_T8_CHUNK
#define PT_T8_CHUNK 32      // rays a wave parks in LDS per chunk fetch (one per lane pair)
#endif
// traversal launch geometry (pt_traverse8p.h): 256-thread blocks, 2 lanes per ray -> 128 rays in flight per block, each with an LDS stack of
// BVH8_STACK entries (odd stride: quads land on different banks) and a T8_SPILL_DEPTH-entry tail in global memory (DeviceScene::travSpill)
static const uint T8_BLOCK = 256, T8_CHUNK = PT_T8_CHUNK, T8_LANES = PT_T8_LANES, T8_GROUPS_PER_WAVE = 64 / PT_T8_LANES, T8_GROUPS_PER_BLOCK = T8_BLOCK / T8_LANES, T8_SPILL_DEPTH = 96;
#ifndef PT_T8_MAX_BLOCKS
#define PT_T8_MAX_BLOCKS (256 * 7 * 3)  // upper bound of a traversal grid (sizes the stack-tail memory). The GPU holds 256 x 7 blocks (LDS). A frame
                                                                          // of several pipelined batches launches exactly that many per batch — 2x / 3x / 4x were 0.2 / 1.7 / 3.7 % slower on the full frame and
                                                                          // 4-7 % on one rank of an 8-way shard (profiles/r03w_maxblocks_ab.txt): the other batches fill the gaps —, a launch that has the GPU to
                                                                          // itself three times that: the blocks that finish early are replaced (TravAux::maxBlocks)
#endif
static const uint T8_MAX_BLOCKS = PT_T8_MAX_BLOCKS;     // persistent waves stride over 64-ray chunks
static const uint T8_PACKET_RAYS = 32, T8_PACKET64_RAYS = 64;

#ifndef T8_CHUNKS_PER_WAVE_MIN
#define T8_CHUNKS_PER_WAVE_MIN 1     // small launches: fewer waves, each working through this many 64-ray chunks (idle quads refill from the next chunk)
#endif
#ifndef T8_SHORT_TAIL_BELOW
#define T8_SHORT_TAIL_BELOW 32768u    // traversal launches of at most this many rays run two task rounds instead of four (launch_extend)
#endif
#ifndef T8_TASK_BLOCKS_N
#define T8_TASK_BLOCKS_N 512        // blocks of a task-round launch: task rounds hold thousands of sub-trees, not millions
#endif
#ifndef T8_ADAPTIVE_CHUNKS
#define T8_ADAPTIVE_CHUNKS 1        // 1: launches below (resident waves x 64) rays use shorter chunks (see traverse8_pairs), 0: always 64 rays per chunk
#endif
// rays per chunk of a traversal launch: the waves the GPU can hold (256 CUs x 4 SIMDs x 8 waves) should cover the launch in one go, 16 .. 64 rays each, in
// steps of 16
static inline uint rays_per_chunk(uint count) {
    if (!T8_ADAPTIVE_CHUNKS) return T8_CHUNK;
    const uint resident = 256u * 4u * 8u;
    const uint step = T8_GROUPS_PER_WAVE;                   // one ray per lane group
    uint r = ((count + resident - 1u) / resident + step - 1u) / step * step;
    return r < step ? (step > T8_CHUNK ? T8_CHUNK : step) : (r > T8_CHUNK ? T8_CHUNK : r);
}
static inline uint grid_for(uint count, uint block, uint maxBlocks) { uint g = (count + block - 1) / block; if (g < 1) g = 1; if (g > maxBlocks) g = maxBlocks; return g; }
// the grid bound of a traversal launch (TravAux::maxBlocks; 0: T8_MAX_BLOCKS), the grid of `count` rays in chunks of rpc, and the grid of the packet launches (a packet per wave)
static inline uint t8_grid_bound(uint maxBlocks) { return (maxBlocks && maxBlocks < T8_MAX_BLOCKS) ? maxBlocks : T8_MAX_BLOCKS; }
static inline uint t8_ray_grid(uint count, uint rpc, uint bound) { return grid_for(count, (T8_BLOCK / 64u) * rpc * T8_CHUNKS_PER_WAVE_MIN, bound); }
static inline uint t8_packet_grid(uint count, bool wide, uint maxBlocks) { return grid_for(count, (T8_BLOCK / 64u) * (wide ? T8_PACKET64_RAYS : T8_PACKET_RAYS), t8_grid_bound(maxBlocks)); }
// task rounds + resolve pass of one traversal launch; all counts live on the device, so the grids are fixed (empty rounds return at once)
static const uint T8_TASK_BLOCKS = T8_TASK_BLOCKS_N, T8_RESOLVE_BLOCKS = 256;
// ... except the visibility resolve's: its sweep over the launch's queue entries (t8_resolve_shadow_body) is sized by the host's count — one entry per thread
// up to 2048 blocks (the 2048 threads a CU holds, on 256 CUs: chosen by that count, not by an A/B — all sweeps of a 4K step together take 0.34 ms), never
// fewer blocks than the resolve list wants, and a zero count is a valid launch
static const uint T8_SWEEP_BLOCKS = 2048;
static inline uint shadow_resolve_grid(uint count) { const uint g = grid_for(count, 256u, T8_SWEEP_BLOCKS); return g < T8_RESOLVE_BLOCKS ? T8_RESOLVE_BLOCKS : g; }
// a small launch holds few stragglers and short ones: two task rounds (split once more, then finish) instead of four — late bounces are
// bound by the host's launch rate, not by the GPU. A fused launch: two only when both of its kinds are small
static inline uint t8_task_rounds(uint count) { return count <= T8_SHORT_TAIL_BELOW ? 2u : 4u; }
static inline uint t8_task_rounds_pair(uint extCount, uint shCount) { return t8_task_rounds(extCount > shCount ? extCount : shCount); }
// The grid of a fused launch: what the two launches would use if it fits the bound, else the bound split by ray count (a visibility ray costs about what a closest-hit ray
// costs: 0.47 against 0.44 ns on C3, its launch's sweep included — 11.70 ms for 25.00 M against 44.41 ms for 101.73 M rays of a serial-kernel step, table 2 of
// profiles/r11a_deferred_visibility_ab.txt; within 10 %: no weights). Precondition: bound >= 2 — each half needs a block, and with a bound of 1 the visibility half
// would get none while its count is zeroed all the same; pt_render clamps the only way in (MI355PT_MAX_BLOCKS).
struct T8PairGrid { uint gE, gS; };
static inline T8PairGrid t8_pair_grid(uint extCount, uint shCount, uint rpc, uint bound) {
    uint gE = t8_ray_grid(extCount, rpc, bound), gS = t8_ray_grid(shCount, rpc, bound);
    if (gE + gS > bound) {
        uint s = (uint)(((unsigned long long)bound * shCount + (extCount + shCount) / 2u) / (extCount + shCount)); if (s < 1u) s = 1u; if (s > bound - 1u) s = bound - 1u;
        if (s > gS) s = gS;
        uint e = bound - s; if (e > gE) { e = gE; s = (bound - e < gS) ? bound - e : gS; }
        gE = e; gS = s;
    }
    return T8PairGrid{gE, gS};
}
} // namespace ptk

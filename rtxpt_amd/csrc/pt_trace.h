// mi355pt — the BVH8 traversal launches (pt_trace.hip): everything that runs traverse8_pairs, traverse8_packets or traverse8_packets64 for the product, their task rounds and
// resolve passes. The grids come from pt_trace_plan.h; the device functions the kernels share with the tests' packet route are in pt_trace_device.h.
#pragma once
#include "pt_wavefront.h"

namespace ptk {
// straggler splitting (pt_traverse8.h): per pipelined batch, two task queues (ping-pong), the per-ray merge keys and the list of rays to resolve.
// bestKey: closest hit = float bits of t << 32 | primitive (atomicMin = min t, ties to the
// lower primitive id); occlusion = 0 visible so far / 1 occluded.
// counts: TRAV_COUNTERS words per traversal launch, one counter per producer so that nothing has to be reset between the launches of a pass —
//   [0] sub-trees split off by k_extend / k_shadow (task queue 0), [1..3] by task rounds 0..2 (queues 1, 0, 1), [TRAV_RESOLVE] rays to resolve.
struct TravAux { TravTask* taskQ[2]; uint* counts; uint taskCap; unsigned long long* bestKey; uint* resolveList; const uint* primToSlot; uint maxBlocks; };      // maxBlocks: grid bound of the traversal launches (0: T8_MAX_BLOCKS)

void launch_extend(const DeviceScene& sc, PathPool pool, const uint* queue, const uint* countPtr, uint count, WaveCounters* wc, bool counters, TravAux aux, hipStream_t st, bool ranged = false);      // ranged: the rays' intervals wait in pool.hit[p].xy (k_extend)
// launch_extend for the first pass of a batch whose paths were NOT generated: ray i is the camera ray of path i of `fv` (no queue, no read of pool.s0 / s1). The rays that are cut into
// sub-trees get their origin | id and direction | length written to pool.s0 / s1 [i] by a launch over the resolve list (k_first_split_rays), for the task rounds and the resolve pass behind it. The camera: wc->firstCamera. Composed frames only (no counters).
// pk.leftover != null: the rays are traced as packets on one shared stack per wave (pt_traverse8k.h: k_extend_first_packets64, 64 rays, or k_extend_first_packets, 32); the packets that exceed pk.stepCap steps or
// pk.stackBound stack entries leave their rays on pk.leftover (count: *pk.leftoverCount, zero on entry; capacity >= count), which the per-ray kernel traces behind them. Same hits.
#ifndef T8_PACKET_STACK
#define T8_PACKET_STACK 64        // entries of a wave's stack in LDS (a node pushes at most seven)
#endif
#ifndef T8_PACKET_STEP_CAP
#define T8_PACKET_STEP_CAP 128    // node + leaf steps after which a packet is handed to the per-ray kernel (environment MI355PT_PACKET_STEP_CAP overrides)
#endif
#ifndef T8_PACKET64_STEP_CAP
#define T8_PACKET64_STEP_CAP 192  // the same for the 64-ray packets, which take a few more steps: the first launch of a 4K step alone on the GPU 7.05 / 6.68 / 6.71 ms at 128 / 192 / 256 (profiles/r21a_packet64_ab.txt)
#endif
// wide != 0: 64-ray packets, one lane per ray (k_extend_first_packets64, traverse8_packets64); 0: the 32-ray pair packets
// precull != 0 (64-ray packets only): a node step first tests each child against the packet's interval of origins and reciprocals, and runs the per-ray slab tests only for
// the children that test keeps (pt_packet_precull.h; environment MI355PT_PACKET_PRECULL)
struct FirstPackets { uint* leftover; uint* leftoverCount; uint capacity, stepCap, stackBound, wide, precull; };
static const uint T8_PACKET_INTERVAL_WORDS = 16;      // a wave's LDS words for its packet's interval (twelve floats, read as three 16-byte groups)
void launch_extend_first(const PathKernelContext& k, PathPool pool, FirstVertex fv, const uint* countPtr, uint count, WaveCounters* wc, TravAux aux, FirstPackets pk, hipStream_t st);
void launch_shadow(const DeviceScene& sc, PathPool pool, ShadowQueue sq, const uint* countPtr, uint count, WaveCounters* wc, bool counters, TravAux aux, hipStream_t st);
// the closest-hit rays of the extend queue and the visibility rays of the previous vertex (shadow queue) in ONE traversal launch, their task rounds and resolve passes in shared launches
// too (k_trace_pair; sq.group == 0 only). auxE / auxS must not share task queues, counters, keys or resolve lists; *shCountPtr is zero afterwards
void launch_trace_pair(const DeviceScene& sc, PathPool pool, const uint* queue, const uint* extCountPtr, uint extCount, ShadowQueue sq, uint* shCountPtr, uint shCount, WaveCounters* wc, TravAux auxE, TravAux auxS, hipStream_t st);
void launch_trace_probe(const DeviceScene& sc, const float4* rays, uint n, float4* outClosest, uint* outVisible, uint* overflow, hipStream_t st);
} // namespace ptk

// mi355pt — wavefront kernels (declarations + HBM stream layout of the path pool and queues).
//
// Path pool (N = owned pixels x samples in flight; ALL samples of a pt_render call are resident at once — HBM is 288 GB):
//   s0[N] uint4  origin.xyz | pixel id (x<<16|y)          s1[N] uint4  dir.xyz | sceneLength
//   s2[N] uint4  thp fp16x4 (2 words) | L fp16x4 (2 words) s3[N] uint4  interiorList[2] | packedCounters | rayCone(fp16x2)
//   s4[N] uint4  {fireflyK,bsdfPdf} | {MISinfo,RRcorr} | flags+vertexIndex | sampleIndex
//   = 80 B per path, the reference's PathPayload size (Rtxpt/Shaders/PathTracer/PathTracerShared.h:21).
//   hit[N] uint4 t | global primitive | bary u | bary v   (written by k_extend, read by k_shade)
// Queues: extend queue = compacted u32 path indices (ping-pong); shadow queue = 3 x float4 per entry
//   q0 origin.xyz|tmax, q1 dir.xyz|path index, q2 radiance.rgb (already multiplied by throughput, MIS, BSDF).
// Queue appends use one atomic per wave64: ballot -> popcount prefix -> lane-0 atomicAdd -> broadcast.
#pragma once
#include "pt_path.h"
#include "pt_neeat.h"
#include "pt_tonemap.h"
#include <hip/hip_runtime.h>

namespace ptk {

struct PathPool { uint4* s0; uint4* s1; uint4* s2; uint4* s3; uint4* s4; uint4* hit;
    // Compacted pool (round 6, pt_render): home == nullptr — every array is indexed by the path's home slot (owned pixel x sample), the extend queue holds home slots. home != nullptr —
    // s0, s1, s3, s4 and hit are indexed by the path's POSITION in the extend queue (k_shade writes a surviving path's state at the position it appends it to, into the other of two
    // array sets), home[position] is its home slot, and s2 — throughput and radiance, what the visibility resolve and k_accumulate address — stays at the home slot.
    const uint* home; };
struct ShadowQueue { float4* q0; float4* q1; float4* q2; uint group;           // group: 0 = one entry per path vertex (NEEFullSamples 1), else entries come in groups of `group` (pt_path.h ShadowSink)
    // NEE-AT feedback (null: off): q3 = {weight, random, light | SSC flag, roulette fix-up} per entry (pt_path.h ShadowRequest); the sub-frame's feedback reservoirs, one slot per pixel
    float4* q3; float* fbTotalWeight; uint* fbCandidates; uint fbWidth, fbPlane, fbSampleFirst; };      // slot = (sample - fbSampleFirst) * fbPlane + y * fbWidth + x
// Vertex 0 in place (pt_render's compacted batches, pt_frame.hip): the launches of a batch's first pass form a path's vertex-0 state where they use it instead of reading what
// k_generate would have stored. Path i of the batch is sample sampleFirst + i % spp of owned pixel ownedPixels[i / spp] — k_generate's map (first_vertex_of,
// pt_wavefront_device.h) — and everything else of the state follows from the frame's settings and camera (PathKernelContextT::generateState, computeCameraRay).
struct FirstVertex { const uint* ownedPixels; uint numOwned, sampleFirst, spp; };
// what a camera ray is a function of besides the pixel and the sample, in memory (WaveCounters::firstCamera) for k_extend_first
struct FirstVertexCamera { PathTracerCameraData cam; float perPixelJitterAAScale, _pad[3]; };
struct WaveCounters {           // device-resident counters / stats (one 256 B block)
    uint extendCount[2]; uint shadowCount; uint overflow;
    unsigned long long hits, nodeVisitsExt, triTestsExt, nodeVisitsSh, triTestsSh, leafVisitsExt, itersExt, leafVisitsSh, itersSh, phaseCycExt[4], leafBlocksExt, eventsExt[8], itersMaxExt, rayIterHistExt[16]; uint longRayCount, _padLong; float longRays[32][8];
    unsigned long long shadowValid;     // grouped shadow queue: entries that carry a light sample (= shadow rays in the reference's sense)
    unsigned long long tailExtendRays, tailShadowRays;      // rays the tail kernel traced itself (pt_tail.hip); what it hands back is counted by the launches that trace it
    unsigned long long tailHandedBack[3];                   // paths the tail kernel handed back: extend stragglers, visibility stragglers, still alive at the bounce bound
    unsigned long long droppedTerminal;                     // terminating hits k_classify dropped as inert (counted in `hits` too)
    // not a counter — the frame's camera for k_extend_first, which reads it where it forms a ray instead of holding twenty more scalars across the traversal loop (it has none to
    // spare): set by the host, it rides with the block's upload at the start of a frame
    FirstVertexCamera firstCamera;
};

// pt_render keeps one PASS_COUNTERS block per batch — {extend launch, shadow launch, k_classify's three class counts and its count of dropped hits} — and zeroes it once per pass.
static const uint TRAV_COUNTERS = 5, TRAV_RESOLVE = 4, PASS_COUNTERS = 16, PASS_SHADOW_OFFSET = 5, PASS_CLASS_OFFSET = 10, PASS_LEFTOVER = 14;      // PASS_LEFTOVER: the rays the vertex-0 packets left to the per-ray kernel (FirstPackets)

// paths [first, first + n) of the pool region -> queue[0 .. n); countPtr (may be null): the counter of the queue `queue` is the end of, incremented by n (k_generate)
void launch_generate(const PathKernelContext& k, PathPool pool, const uint* ownedPixels, uint numOwned, uint sampleFirst, uint spp, uint first, uint n, uint* queue, uint* countPtr, hipStream_t st);
// classScratch (2 x countIn words: memory that is free between the extend and the shadow launches of a bounce) + classCount (4 words, zero on entry: three classes and the dropped hits): k_classify's output; null = shade in queue order
// launch_extend / launch_shade / launch_shadow expect the pass's counter block zeroed by the caller (launch_pass_reset)
void launch_shade(const PathKernelContext& k, PathPool pool, const uint* queueIn, const uint* countInPtr, uint countIn, uint* queueOut, uint* countOutPtr,
                  ShadowQueue sq, WaveCounters* wc, uint* classScratch, uint* classCount, hipStream_t st, PathPool outPool = PathPool{},      // outPool: a compacted pool's other array set (pool.home != nullptr)
                  const FirstVertex* fv = nullptr, const uint* inertBits = nullptr);      // inertBits: pt_scene.h's two bits per primitive — k_classify drops the terminating hits that are inert (null: none; never with NEE-AT or at vertex 0). fv: vertex 0 of paths that were not generated — k_classify and k_shade form the state (pool.home is not read: position == home slot). Compacted pool, sq.group == 0, no NEE-AT
// a compacted pool's live paths back to their home slots: out.s0 / s1 / s3 / s4 [home[i]] = in...[i] for the *countPtr positions (out: another array set than in's); the queue `in.home` is then an ordinary extend queue
void launch_uncompact(PathPool in, PathPool out, const uint* countPtr, uint count, hipStream_t st);
void launch_classify(PathPool pool, const uint* queueIn, const uint* countInPtr, uint countIn, uint* classScratch, uint* classCount, hipStream_t st);      // k_classify: {continuing hit, terminating hit, miss} made contiguous
// the late bounces of a batch in one launch: every wave runs 32 paths of queueIn to their end (at most maxBounces bounces each); stragglers and paths beyond the bound come back through
// queueOut / countOutPtr (and, for visibility rays, the shadow queue / wc->shadowCount). NEEFullSamples 1 only (sq.group == 0); the pass's counters zeroed by the caller as for launch_shade
void launch_tail(const PathKernelContext& k, PathPool pool, const uint* queueIn, const uint* countInPtr, uint countIn, uint* queueOut, uint* countOutPtr, ShadowQueue sq, WaveCounters* wc, uint maxBounces, uint deferIters /* 0: T8_TAIL_DEFER */, uint maxBlocks, hipStream_t st);
void launch_pass_reset(uint* passCounters, uint* nextCount, uint* shadowCount, hipStream_t st);      // one launch: the batch's PASS_COUNTERS words and the two queue counters the pass refills
void launch_accumulate(PathPool pool, const uint* ownedPixels, uint numOwned, uint spp, float4* accum, uint accumCountBase, uint width, hipStream_t st);

} // namespace ptk

/* mi355pt — evaluation hooks for the known-answer tests. NOT part of the product's ABI: the shipped rtxpt_amd/libmi355pt.so does not export anything declared here.
 * `make -C rtxpt_amd/csrc` also builds rtxpt_amd/libmi355pt_testhooks.so — the same sources with -DMI355PT_TEST_HOOKS — which exports everything include/mi355pt.h
 * declares plus the entry point below; tests/ load that variant where they need it (rtxpt_amd.PathTracer(test_hooks=True)). */
#ifndef MI355PT_TESTHOOKS_H
#define MI355PT_TESTHOOKS_H
#include "mi355pt.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Device-side evaluation of the product's own leaf functions, one thread per row, so that a test can compare them bit for bit with the outputs of the reference's text
 * (tests/golden/refpin_hlsl_golden.npz) or of the oracle. kind (rtxpt_amd/csrc/pt_wavefront.hip k_probe): 0 deterministic math (fn, x, y); 1 binary16 round trip;
 * 2 sample streams (pixel, vertex, sample, seed, generator, count); 3 whole-BSDF eval / sample / pdf; 4 camera rays; 5 leaf functions pinned to the reference text
 * (Fresnel, microfacet, octahedral maps, disk / hemisphere sampling, ComputeRayOrigin, firefly filter ...); 6 polymorphic lights; 7 the half-typed operators of the lp16 build;
 * 8 Bridge::loadSurface (45 words per hit); 9 EnvMap::EvalLocal on the baked cube; 10 the traversal's alpha test; 11 the texture samplers; 12 stochastic texture filtering. `n` rows in, `n` rows out; the row
 * layouts are the probe's.
 * Kind 11, eight 32-bit words in, one float4 out: word 0 the mode, word 1 the texture, words 2-3 uv (floats), words 4-7 by mode —
 *   mode 0  PathKernelContext::sampleTexture: word 1 = the packed texture word of a material (baseLOD << 24 | mipLevels << 16 | index), word 4 = lambdaNoDims (float)
 *   mode 1  sample_bilinear at one level:     word 1 = the texture index, word 4 = the mip (integer, below the texture's mipLevels)
 *   mode 2  sample_grad_anisotropic:          word 1 = the texture index, words 4-5 = gx, words 6-7 = gy (floats)
 * pt_probe refuses rows whose mode, texture or mip the scene does not have. uv, lambda and the gradients must be finite: the samplers' data contract.
 * Kind 12, stochastic texture filtering (rtxpt_amd/csrc/pt_stf.h), twelve words in, eight words out: word 0 the mode, word 1 the packed texture word of a material, words 2-3 uv,
 * word 4 lambdaNoDims, word 5 the filter (PT_STF_FILTER_POINT / LINEAR / CUBIC), words 6-9 by mode, words 10-11 unused —
 *   mode 0  one lookup with the four random numbers of words 6-9 (floats in [0, 1)): words 0-3 out = the texel, words 4-6 = the level, x and y it was taken from, word 7 = 0
 *   mode 1  words 6-8 = packed pixel (x << 16 | y), path vertex index, sample index: words 0-3 out = the four numbers Bridge::loadSurface draws for that call, words 4-7 = 0
 * pt_probe refuses rows whose mode, texture (mode 0) or filter (mode 0) the scene or the library does not have. */
int32_t pt_probe(pt_context* ctx, int32_t kind, const void* in, size_t inBytes, void* out, size_t outBytes, uint32_t n);
/* The "inert when terminal" table of the prepared scene (rtxpt_amd/csrc/pt_scene.h inert_bits_of; built on the device by k_inert_bits) and what the last pt_render call did with
 * it. Two bits per global primitive, sixteen primitives a word, primitive p in bits 2 (p % 16) and 2 (p % 16) + 1 of word p / 16: bit 0 = the material can neither emit (all three
 * components of EmissiveColor exactly zero) nor stand in for an analytic light, bit 1 = thin surface. numPrims (may be null): the scene's primitives; words (may be null):
 * capacityWords >= (numPrims + 15) / 16 words; lastDropped (may be null): the terminating hits the last pt_render call left unshaded (0 with MI355PT_DROP_INERT_TERMINAL=0, with
 * NEE-AT, and in frames whose passes are all below the classification threshold). */
int32_t pt_get_inert_terminal(pt_context* ctx, uint32_t* numPrims, uint32_t* words, uint32_t capacityWords, uint64_t* lastDropped);
/* The wide tree of the prepared scene as the traversal reads it, for tests/bvh_ref.py (the checker of the tree's invariants). Synchronises the context's stream and copies
 *   nodes           numNodes 128-byte records (rtxpt_amd/csrc/pt_scene.h Bvh8Node: origin, exps, eight 12-byte child slots, the three scales as floats), capacityNodes records
 *   tris            numTris 48-byte leaf-order records (pt_scene.h TriRecord: x[3] prim y[3] flags z[3] pad — the stored pad included), capacityTris records
 *   bounds          six floats, min xyz then max xyz: the scene bounds the pads were formed from
 *   wideLevelStart  min(collapseLevels, 64) + 1 words: the wide nodes of collapse level L are [wideLevelStart[L], wideLevelStart[L + 1]); capacityLevels words
 * Every pointer may be null: the counts alone come back, so a caller sizes its buffers with a first call. A non-null buffer whose capacity is below its count is
 * PT_ERROR_INVALID_ARGUMENT and nothing is written to any buffer. A scene without triangles gives 0 nodes, 0 triangles, 0 levels and zero bounds. Only what the traversal reads is
 * read: after a refit (pt_animate without rebuild) the binary tree, the primitive-order triangles and the range tables of the last full build hold an older pose and stay out. */
int32_t pt_get_bvh8(pt_context* ctx, uint32_t* numNodes, void* nodes, uint32_t capacityNodes, uint32_t* numTris, void* tris, uint32_t capacityTris, float* bounds,
                    uint32_t* collapseLevels, uint32_t* wideLevelStart, uint32_t capacityLevels);
/* A caller's rays through the traversal launches a FRAME runs, for tests/test_gpu_traversal_routes.py: pt_trace_closest / pt_trace_visibility run a probe kernel whose
 * instantiation of the traverser (no fixed interval, no sub-tree tasks, no splitting) no frame uses. rays: n x 8 floats, origin | tmin | direction | tmax, as pt_trace_closest
 * takes them. Everything the launches write is owned by the call: the context's pool, queues and counters are untouched.
 *   PT_ROUTE_EXTEND         the rays stand in a path pool as k_generate stores them (origin | id, direction | length), behind an identity queue; launch_extend: k_extend, the
 *                           sub-tree task rounds of that count, k_resolve_extend. The interval is [0, kMaxRayTravel] whatever a ray says, so rays that say anything else
 *                           (tmin != 0, tmax != 1e15f) are refused. out: n x 4 words, t | primitive | u | v — the pool's hit records.
 *   PT_ROUTE_EXTEND_RANGED  the same with launch_extend(..., ranged): every ray's (tmin, tmax) waits in the first two words of its hit record (the stable-plane fill pass's first launch).
 *   PT_ROUTE_SHADOW         the rays stand in a shadow queue of the grouped layout, one entry per group (origin | tmax, direction | entry, radiance zero); tmin must be 0.
 *                           launch_shadow: k_shadow, its task rounds, the marking resolve pass (and the fold of the marks into a path pool of the call's own). out: n words,
 *                           1 = visible (the entry's mark), 0 = occluded.
 *   PT_ROUTE_PACKETS        64 or 32 rays per wave on one stack (traverse8_packets64 / traverse8_packets, by the context's packet mode), read from the same pool; the packets over the step cap or the stack bound leave their rays on a
 *                           list that launch_extend then traces one by one, task rounds included — what launch_extend_first does for camera rays. Fixed interval, as EXTEND.
 * options (may be null; a zero field is the product's value): taskCap = entries of a task queue (TASK_QUEUE_CAPACITY); maxBlocks = TravAux::maxBlocks, the grid bound of the
 * traversal launches; stepCap / stackBound = FirstPackets' (T8_PACKET_STEP_CAP or, for the 64-ray packets, T8_PACKET64_STEP_CAP; T8_PACKET_STACK). The packet route runs the traverser of the context's MI355PT_FIRST_VERTEX_PACKETS mode, the 64-ray one with or without the packet's interval test (MI355PT_PACKET_PRECULL).
 * stats (may be null), written whenever the launches ran: splitRays = the resolve list's length (rays cut into sub-trees); taskCounts[r] = sub-trees fed to task round r;
 * packetRays = rays the packets committed themselves, leftoverRays = rays they left over (both 0 on the other routes); overflow = WaveCounters::overflow after the launches
 * (1: a stack tail, 2: a task queue or the leftover list ran out of room). A set overflow word is PT_ERROR_HIP, as at the end of pt_render — `out` is then not the answer.
 * A ray whose tmin is negative, -0 or NaN is refused before anything reaches the device (pt_trace_closest's rule), an unknown route too. */
enum { PT_ROUTE_EXTEND = 0, PT_ROUTE_EXTEND_RANGED = 1, PT_ROUTE_SHADOW = 2, PT_ROUTE_PACKETS = 3 };
typedef struct PtRouteOptions { uint32_t taskCap, maxBlocks, stepCap, stackBound; } PtRouteOptions;
typedef struct PtRouteStats { uint32_t splitRays, taskCounts[4], packetRays, leftoverRays, overflow; } PtRouteStats;
int32_t pt_trace_route(pt_context* ctx, int32_t route, const float* rays, uint32_t n, const PtRouteOptions* options, void* out, PtRouteStats* stats);
#ifdef __cplusplus
}
#endif
#endif

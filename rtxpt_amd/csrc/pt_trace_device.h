// mi355pt — device functions of the traversal launches (pt_trace.hip) that the tests' packet route (pt_hooks.hip) runs too: one statement of each ray source and sink. A packet
// kernel says where its rays come from and what a commit does, and hands both to its traverser (pt_traverse8k.h).
#pragma once
#include "pt_trace.h"          // (FirstPackets, before pt_traverse8k.h names it)
#include "pt_traverse8.h"
#include "pt_traverse8p.h"
#include "pt_traverse8k.h"
#include "pt_wavefront_device.h"

namespace ptk {
// The camera ray of path i of a batch whose paths were not generated (FirstVertex). The camera comes from memory (WaveCounters::firstCamera) each time a ray is formed, behind a
// compiler barrier: as kernel arguments its twenty scalars, and what the compiler hoists of the ray's arithmetic, would be live across the traversal loop, which runs at its
// register bound
__device__ __forceinline__ void t8_camera_ray(const WaveCounters* wc, const FirstVertex& fv, uint i, float3& o, float3& d) {
    asm volatile("" ::: "memory");
    const FirstVertexCamera fc = wc->firstCamera;
    uint px, sample; first_vertex_of(fv, i, px, sample);
    PathKernelContext::cameraRay(fc.cam, fc.perPixelJitterAAScale, px >> 16, px & 0xFFFFu, sample, o, d);
}
// the stored ray of pool position p: origin | id, direction | length, as k_generate, k_shade and k_first_split_rays write them
__device__ __forceinline__ void t8_stored_ray(const PathPool& pool, uint p, float3& o, float3& d) {
    uint4 a = pool.s0[p], b = pool.s1[p];
    o = make_float3(asfloat(a.x), asfloat(a.y), asfloat(a.z)); d = make_float3(asfloat(b.x), asfloat(b.y), asfloat(b.z));
}
// the hit record k_classify and k_shade read: t | global primitive | bary u | bary v
__device__ __forceinline__ void t8_store_hit(const PathPool& pool, uint p, const HitInfo& h) { pool.hit[p] = make_uint4(asuint(h.t), h.prim, asuint(h.u), asuint(h.v)); }
} // namespace ptk

// mi355pt — adaptive sampling on the device (pt_adaptive.h holds the per-pixel text; this file maps it onto waves). Blocks of 256 threads:
//   k_adaptive_accumulate   k_accumulate's loop over a slice of the active list: a lane is one pixel, its `spp` samples are neighbours in the pool. Besides the accumulation
//                           buffer (the same values by the same expressions) it keeps the mean of the even-indexed samples and the pixel's count: 32 more bytes read and
//                           36 written a pixel and round.
//   k_adaptive_error        one wave per 8 x 8 block, four blocks a workgroup. Lane i holds the error of the block's i-th pixel (two 16-byte loads; an 8 x 8 block is eight
//                           128-byte lines of each buffer), the lanes past the block's count hold 0. The sum is a cross-lane tree in registers, v[i] += v[i + off] for
//                           off = 32 .. 1 (__shfl_down: ds_bpermute_b32, no LDS allocation, no barrier); lane 0 holds the tree's value — the order of the additions is part of the
//                           interface — and writes E to the frame's block map and the block's flag: {the pixels it keeps, 1} or {0, 0}.
//   k_adaptive_scan_chunks  exclusive prefix sums of the flags, both words, over chunks of 256 blocks: a block a lane, a wave scan by __shfl_up, the four wave totals through
//                           LDS (one barrier). A flag becomes {pixels kept before it in the chunk, blocks kept before it | kept << 31}; the chunk's sums go to `chunks`.
//   k_adaptive_scan_totals  one wave turns the chunk sums into exclusive prefixes, 64 a step with the carry in a register (507 chunks, eight steps, for the 129 600 blocks of
//                           a 4K rank), and leaves the totals — the new lists' sizes — in device memory for the host's read-back.
//   k_adaptive_copy         one wave per block again: a kept block's pixels go to chunk prefix + local prefix of the new pixel list, lane 0 writes the new block record. The
//                           new lists are the old ones without the retired blocks, in the same order: nothing is placed by an atomic.
// No scratch. The error pass reads 32 bytes a pixel.
#include "pt_adaptive.h"
#include "pt_wavefront_device.h"

namespace ptk {

__global__ void __launch_bounds__(256)
k_adaptive_accumulate(PathPool pool, const uint* __restrict__ pixels, uint numPix, uint spp, float4* __restrict__ accum, float4* __restrict__ half, uint* __restrict__ counts,
                      uint accumCountBase, uint width) {
    const uint kpx = blockIdx.x * 256u + threadIdx.x;
    if (kpx >= numPix) return;
    const uint px = pixels[kpx];
    const uint addr = (px & 0xFFFFu) * width + (px >> 16);
    float4 acc = accum[addr], hf = half[addr];
    for (uint s = 0; s < spp; s++) {
        const uint4 c = pool.s2[PT_SAMPLE_MINOR ? kpx * spp + s : s * numPix + kpx];
        const float2 l0 = Fp16ToFp32(c.z), l1 = Fp16ToFp32(c.w);
        const float4 col = make_float4(l0.x, l0.y, l1.x, 1.0f);
        const uint index = accumCountBase + s;
        acc = Adaptive_Fold(acc, col, index);
        if (!(index & 1u)) hf = Adaptive_Fold(hf, col, index >> 1);
    }
    accum[addr] = acc; half[addr] = hf; counts[addr] += spp;
}

__global__ void __launch_bounds__(256) k_adaptive_error(AdaptiveEval e) {
    const uint b = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (b >= e.numBlocks) return;      // (the whole wave)
    const AdaptiveBlock blk = e.blkIn[b];
    float v = 0.0f;
    if (lane < blk.count) {
        const uint px = e.pixIn[blk.first + lane];
        const uint addr = (px & 0xFFFFu) * e.width + (px >> 16);
        v = Adaptive_PixelError(e.accum[addr], e.half[addr], e.darkFloor);
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, (unsigned)off);      // lane i < off: v[i] + v[i + off]
    if (lane == 0u) {
        const float E = v / (float)blk.count;
        const uint px = e.pixIn[blk.first];
        e.blockError[((px & 0xFFFFu) >> 3) * e.blocksX + (px >> 19)] = E;
        e.flags[b] = (E < e.threshold) ? make_uint2(0u, 0u) : make_uint2(blk.count, 1u);
    }
}

// inclusive prefix sum over the 64 lanes of a wave
static __device__ __forceinline__ uint wave_scan(uint v, uint lane) {
    #pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint t = __shfl_up(v, (unsigned)o); if (lane >= (uint)o) v += t; }
    return v;
}
static __device__ __forceinline__ uint2 wave_scan(uint2 v, uint lane) { return make_uint2(wave_scan(v.x, lane), wave_scan(v.y, lane)); }

__global__ void __launch_bounds__(256) k_adaptive_scan_chunks(uint2* __restrict__ flags, uint numBlocks, uint2* __restrict__ chunks) {
    __shared__ uint2 sums[4];
    const uint i = blockIdx.x * kAdaptiveScanChunk + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint2 f = i < numBlocks ? flags[i] : make_uint2(0u, 0u);
    uint2 incl = wave_scan(f, lane);
    if (lane == 63u) sums[wave] = incl;
    __syncthreads();
    for (uint w = 0; w < wave; w++) { incl.x += sums[w].x; incl.y += sums[w].y; }
    if (i < numBlocks) flags[i] = make_uint2(incl.x - f.x, (incl.y - f.y) | (f.y << 31));
    if (threadIdx.x == 255u) chunks[blockIdx.x] = incl;
}

// one wave: 64 chunk sums a step, the carry in a register
__global__ void __launch_bounds__(64) k_adaptive_scan_totals(uint2* __restrict__ chunks, uint numChunks, uint* __restrict__ totals) {
    const uint lane = threadIdx.x;
    uint2 carry = make_uint2(0u, 0u);
    for (uint base = 0; base < numChunks; base += 64u) {
        const uint i = base + lane;
        const uint2 v = i < numChunks ? chunks[i] : make_uint2(0u, 0u);
        const uint2 incl = wave_scan(v, lane);
        if (i < numChunks) chunks[i] = make_uint2(carry.x + incl.x - v.x, carry.y + incl.y - v.y);
        carry.x += __shfl(incl.x, 63); carry.y += __shfl(incl.y, 63);
    }
    if (lane == 0u) { totals[0] = carry.x; totals[1] = carry.y; }
}

__global__ void __launch_bounds__(256) k_adaptive_copy(AdaptiveEval e) {
    const uint b = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (b >= e.numBlocks) return;
    const uint2 f = e.flags[b];
    if (!(f.y >> 31)) return;      // retired
    const uint2 chunk = e.chunks[b / kAdaptiveScanChunk];
    const AdaptiveBlock blk = e.blkIn[b];
    const uint dst = chunk.x + f.x;
    if (lane < blk.count) e.pixOut[dst + lane] = e.pixIn[blk.first + lane];
    if (lane == 0u) e.blkOut[chunk.y + (f.y & 0x7FFFFFFFu)] = AdaptiveBlock{dst, blk.count};
}

void launch_adaptive_accumulate(PathPool pool, const uint* pixels, uint numPix, uint spp, float4* accum, float4* half, uint* counts, uint accumCountBase, uint width, hipStream_t st) {
    hipLaunchKernelGGL(k_adaptive_accumulate, dim3((numPix + 255) / 256), dim3(256), 0, st, pool, pixels, numPix, spp, accum, half, counts, accumCountBase, width);
}
void launch_adaptive_evaluate(const AdaptiveEval& e, hipStream_t st) {
    const uint waves = (e.numBlocks + 3u) / 4u, numChunks = adaptive_chunks(e.numBlocks);
    hipLaunchKernelGGL(k_adaptive_error, dim3(waves), dim3(256), 0, st, e);
    hipLaunchKernelGGL(k_adaptive_scan_chunks, dim3(numChunks), dim3(256), 0, st, e.flags, e.numBlocks, e.chunks);
    hipLaunchKernelGGL(k_adaptive_scan_totals, dim3(1), dim3(64), 0, st, e.chunks, numChunks, e.totals);
    hipLaunchKernelGGL(k_adaptive_copy, dim3(waves), dim3(256), 0, st, e);
}

} // namespace ptk

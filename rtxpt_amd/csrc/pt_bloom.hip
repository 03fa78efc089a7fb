// mi355pt — the bloom pass on the device (pt_bloom.h holds the per-texel text; this file maps it onto waves). Four kernels per call, blocks of 256 threads:
//   k_bloom_reduce     a lane is one quarter-resolution texel, a wave 64 consecutive ones of a row: the lane's four 16-byte loads of a source row are 64 contiguous bytes and the
//                      wave's 4 KB, four rows each. Sanitises as it sums. (Alpha is not used, so the compiler issues these loads, and the composite's, as
//                      global_load_dwordx3: 12 of a texel's 16 bytes. The lines fetched are the same.)
//   k_bloom_blur_x     a block is a 64 x 4 tile of quarter-resolution texels, a wave one row of it. The row plus a halo of R texels on each side (R <= 48, the halo that is
//                      staged is the call's R, not 48) goes to LDS as 16-byte records at consecutive slots, coordinates clamped to the image (an edge texel repeats); a
//                      lane's tap i is the slot i to each side of its own, so every ds_read_b128 of a wave covers 64 consecutive slots: no bank conflict.
//   k_bloom_blur_y     a block is an 8 x 32 tile, a wave 8 consecutive rows of it; the tile plus R rows above and below in LDS, rows of 8 records (128 bytes: one cache line of
//                      the global image a row). Lane (lx, ly) is slot ly x 8 + lx = its lane number plus a constant, tap i is 8 i slots away: again 64 consecutive slots a read.
//                      The tile shapes: the x pass holds (64 + 96) x 4 records = 10 KB, the y pass (32 + 96) x 8 = 16 KB; 160 KB of LDS a CU take ten such blocks and the
//                      wave slots take eight (8 waves a SIMD x 4 SIMDs / 4 waves a block), so the y pass's footprint does not cap occupancy below the x pass's. A 64 x 4 tile
//                      turned on its side (4 x 64) would be as small as the x pass's, but its global rows would be 64 bytes: half a line.
//                      The taps g[0 .. R] and their sum G are a kernel argument (BloomTaps, 204 bytes): uniform, read by scalar loads inside the tap loop; nothing is
//                      pre-divided — the result is acc / G as the formulas state.
//   k_bloom_composite  a lane is one full-resolution pixel, a wave 64 consecutive ones of a row: one load of the source texel (rgb, see the reduce; sanitised again, so no full-resolution
//                      intermediate exists), four cached taps of the blurred image, one 16-byte store.
// The quarter-resolution images (8.3 MB at 3840 x 2160) are meant to stay in the cache between the passes. No scratch.
#include "pt_bloom.h"

namespace ptk {

static const int BLOOM_XW = 64, BLOOM_XH = 4;       // k_bloom_blur_x's tile; also the thread shape of the reduce and the composite
static const int BLOOM_YW = 8, BLOOM_YH = 32;       // k_bloom_blur_y's tile

// the LDS record: a 16-byte vector (ptk::float4 is a plain struct of alignment 4), so a record is written and read whole, by one ds_write_b128 / ds_read_b128
typedef float BloomRecord __attribute__((ext_vector_type(4)));
static __device__ inline BloomRecord bloom_record(float4 v) { BloomRecord r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w; return r; }
static __device__ inline float3 bloom_rgb(BloomRecord r) { return make_float3(r.x, r.y, r.z); }

__global__ void __launch_bounds__(256)
k_bloom_reduce(const float4* __restrict__ src, float4* __restrict__ q, float maxRadiance, uint width, uint height, uint qw, uint qh) {
    const uint X = blockIdx.x * BLOOM_XW + (threadIdx.x & 63u), Y = blockIdx.y * BLOOM_XH + (threadIdx.x >> 6);
    if (X >= qw || Y >= qh) return;
    q[(size_t)Y * qw + X] = make_float4(Bloom_Reduce(src, (int)X, (int)Y, width, height, maxRadiance), 0.0f);
}

__global__ void __launch_bounds__(256)
k_bloom_blur_x(const float4* __restrict__ in, float4* __restrict__ out, BloomTaps K, uint qw, uint qh) {
    constexpr int LW = BLOOM_XW + 2 * kBloomMaxTaps;
    __shared__ BloomRecord sT[BLOOM_XH][LW];
    const int R = (int)K.R, tx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);
    const int bx = (int)blockIdx.x * BLOOM_XW, y = (int)blockIdx.y * BLOOM_XH + ly;
    const float4* __restrict__ row = in + (size_t)TAA_ClampCoord(y, (int)qh) * qw;
    for (int lx = tx; lx < BLOOM_XW + 2 * R; lx += 64) sT[ly][lx] = bloom_record(row[TAA_ClampCoord(bx + lx - R, (int)qw)]);
    __syncthreads();
    const int x = bx + tx;
    if (x >= (int)qw || y >= (int)qh) return;
    out[(size_t)y * qw + x] = make_float4(Bloom_Blur([&](int i) { return bloom_rgb(sT[ly][tx + R + i]); }, K), 0.0f);
}

__global__ void __launch_bounds__(256)
k_bloom_blur_y(const float4* __restrict__ in, float4* __restrict__ out, BloomTaps K, uint qw, uint qh) {
    constexpr int LH = BLOOM_YH + 2 * kBloomMaxTaps;
    __shared__ BloomRecord sT[LH][BLOOM_YW];
    const int R = (int)K.R, lx = (int)(threadIdx.x & 7u), ty = (int)(threadIdx.x >> 3);
    const int by = (int)blockIdx.y * BLOOM_YH, x = (int)blockIdx.x * BLOOM_YW + lx;
    const int cx = TAA_ClampCoord(x, (int)qw);
    for (int ly = ty; ly < BLOOM_YH + 2 * R; ly += BLOOM_YH) sT[ly][lx] = bloom_record(in[(size_t)TAA_ClampCoord(by + ly - R, (int)qh) * qw + cx]);
    __syncthreads();
    const int y = by + ty;
    if (x >= (int)qw || y >= (int)qh) return;
    out[(size_t)y * qw + x] = make_float4(Bloom_Blur([&](int i) { return bloom_rgb(sT[ty + R + i][lx]); }, K), 0.0f);
}

__global__ void __launch_bounds__(256)
k_bloom_composite(const float4* __restrict__ src, const float4* __restrict__ B, float4* __restrict__ out, float intensity, float maxRadiance, uint width, uint height, uint qw, uint qh) {
    const uint x = blockIdx.x * BLOOM_XW + (threadIdx.x & 63u), y = blockIdx.y * BLOOM_XH + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const size_t pix = (size_t)y * width + x;
    const float3 s = Bloom_Sanitise(src[pix], maxRadiance);
    out[pix] = make_float4(Bloom_Composite(s, Bloom_Upsample(B, (int)x, (int)y, (int)qw, (int)qh), intensity), 1.0f);
}

void launch_bloom(const float4* src, float4* q0, float4* q1, float4* out, const BloomTaps& K, float intensity, float maxRadiance, uint width, uint height, hipStream_t st) {
    const uint qw = bloom_reduced(width), qh = bloom_reduced(height);
    const auto blocks = [](uint n, int tile) { return (n + (uint)tile - 1u) / (uint)tile; };
    const dim3 gq(blocks(qw, BLOOM_XW), blocks(qh, BLOOM_XH)), gy(blocks(qw, BLOOM_YW), blocks(qh, BLOOM_YH)), gf(blocks(width, BLOOM_XW), blocks(height, BLOOM_XH));
    hipLaunchKernelGGL(k_bloom_reduce, gq, dim3(256), 0, st, src, q0, maxRadiance, width, height, qw, qh);
    hipLaunchKernelGGL(k_bloom_blur_x, gq, dim3(256), 0, st, (const float4*)q0, q1, K, qw, qh);
    hipLaunchKernelGGL(k_bloom_blur_y, gy, dim3(256), 0, st, (const float4*)q1, q0, K, qw, qh);
    hipLaunchKernelGGL(k_bloom_composite, gf, dim3(256), 0, st, src, (const float4*)q0, out, intensity, maxRadiance, width, height, qw, qh);
}

} // namespace ptk

// mi355pt — the temporal anti-aliasing resolve on the device (pt_taa.h holds the per-pixel text; this file maps it onto waves). One kernel per frame, shaped like the denoiser's
// history clamp (pt_relax.hip k_relax_clamp): a block of 256 threads is a 32 x 8 pixel tile, a lane one pixel. The tile plus a 1-pixel halo is staged in LDS as two arrays of
// 16-byte records — the sanitised colour with its luminance, and the motion vector with its squared length — so a pixel is sanitised and its motion unpacked once, not nine
// times; halo coordinates are clamped to the frame (an edge pixel repeats). A row of lanes reads consecutive 16-byte slots: no bank conflict at any row length. The history taps
// (16 for Catmull-Rom, 4 for bilinear) are 16-byte global loads: their footprint follows the motion vector, not the tile. 10.6 KB of LDS a block, no scratch.
#include "pt_taa.h"

namespace ptk {

static const int TAA_TW = 32, TAA_TH = 8;

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_taa_resolve(const float4* __restrict__ colour, const uint2* __restrict__ motion, const unsigned char* __restrict__ relax, const float4* __restrict__ history, float4* __restrict__ out,
              TaaParams P, uint width, uint height) {
    constexpr int HALO = 1, LW = TAA_TW + 2 * HALO, LH = TAA_TH + 2 * HALO;
    __shared__ __attribute__((aligned(16))) float4 sC[LH][LW], sM[LH][LW];
    const int bx = (int)blockIdx.x * TAA_TW, by = (int)blockIdx.y * TAA_TH;
    for (int i = (int)threadIdx.x; i < LW * LH; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const size_t q = (size_t)TAA_ClampCoord(by + ly - HALO, (int)height) * width + TAA_ClampCoord(bx + lx - HALO, (int)width);
        sC[ly][lx] = TAA_Colour(colour[q], P.maxRadiance); sM[ly][lx] = TAA_Motion(motion[q]);
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & 31u) + HALO, ly = (int)(threadIdx.x >> 5) + HALO, x = bx + lx - HALO, y = by + ly - HALO;
    if (x >= (int)width || y >= (int)height) return;
    const size_t pix = (size_t)y * width + x;
    const float4 c = sC[ly][lx];
    // the 3 x 3 in scan-line order: colour moments per channel, and the longest motion vector (the first of equals)
    float3 sum = make_float3(0.0f), sum2 = make_float3(0.0f); float4 mv = sM[ly - 1][lx - 1];
    #pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        #pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const float4 t = sC[ly + dy][lx + dx], m = sM[ly + dy][lx + dx];
            sum = sum + xyz(t); sum2 = sum2 + xyz(t) * xyz(t);
            if (m.z > mv.z) mv = m;
        }
    }
    float px, py; float3 r = xyz(c);
    if (history && TAA_PreviousPosition(x, y, mv.x, mv.y, width, height, px, py)) {
        float3 hst = TAA_SampleHistory(history, px, py, width, height, P.useCatmullRomFilter != 0u);
        if (P.enableHistoryClamping) hst = TAA_ClampHistory(hst, sum, sum2, P.clampingFactor, relax ? DN_LoadUnorm8(relax[pix]) : 0.0f);
        r = TAA_Blend(xyz(c), c.w, hst, P);
    }
    out[pix] = make_float4(r, 1.0f);
}

void launch_taa_resolve(const float4* colour, const uint2* motion, const unsigned char* relax, const float4* history, float4* out, const TaaParams& P, uint width, uint height, hipStream_t st) {
    const dim3 grid((width + TAA_TW - 1) / TAA_TW, (height + TAA_TH - 1) / TAA_TH);
    hipLaunchKernelGGL(k_taa_resolve, grid, dim3(256), 0, st, colour, motion, relax, history, out, P, width, height);
}

} // namespace ptk

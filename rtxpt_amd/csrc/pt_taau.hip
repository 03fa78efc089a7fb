// mi355pt — the temporal upscaling resolve on the device (pt_taau.h holds the per-pixel text; this file maps it onto waves). One kernel per frame, built on k_taa_resolve's
// shape (pt_taa.hip) but output-driven: a block of 256 threads is a 32 x 8 tile of DISPLAY pixels, a lane one display pixel. The block stages the tile's render-space
// footprint — the nearest samples of its pixels plus a 1-pixel halo — in LDS as the same two arrays of 16-byte records (the sanitised colour with its luminance, the motion
// vector with its squared length): a render pixel is sanitised and its motion unpacked once per block; coordinates are clamped on load (an edge pixel repeats). Neighbouring
// lanes read the same or the next 16-byte record (at ratio 2 a pair of lanes shares one, which LDS serves as a broadcast; at ratio 1 a row of lanes reads consecutive
// records as k_taa_resolve does): no bank conflict beyond the four passes a 16-byte read of 64 lanes takes anyway. The history taps (16 for Catmull-Rom, 4 for bilinear) are
// 16-byte global loads at display resolution. 12.0 KB of LDS a block, no scratch.
//
// The staged extent. u(X) = ((float)X + 0.5f) x rx with rx = (float)w / (float)W <= 1 (the host refuses W < w), and i0(X) = clamp(floor(u(X) + jx)). Every step — the
// product, the sum, floor, the clamp — is monotone in X, so the tile's first pixel X0 has the smallest i0. In exact arithmetic u(X0 + 31) - u(X0) = 31 rx <= 31; the four
// roundings on the way (two products, two sums) move a value by half an ulp each, below 2^-4 in all for coordinates below 2^18 (frames are below 2^16 pixels wide and the
// display at most four times that), so the rounded difference stays below 32 and floor differs by at most 32: i0(X) is in [i0(X0), i0(X0) + 32] for the whole tile, 33 columns,
// and 35 with the halo. Likewise 8 rows give j0 in [j0(Y0), j0(Y0) + 8]: 9 rows, 11 with the halo. Only the part the tile's last pixel needs is loaded.
#include "pt_taau.h"

namespace ptk {

static const int TAAU_TW = 32, TAAU_TH = 8;

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_taa_upscale(const float4* __restrict__ colour, const uint2* __restrict__ motion, const unsigned char* __restrict__ relax, const float4* __restrict__ history, float4* __restrict__ out,
              TaauParams P, TaauFrame F) {
    constexpr int HALO = 1, LW = TAAU_TW + 1 + 2 * HALO, LH = TAAU_TH + 1 + 2 * HALO;
    __shared__ __attribute__((aligned(16))) float4 sC[LH][LW], sM[LH][LW];
    const int w = (int)F.width, h = (int)F.height;
    const int bx = (int)blockIdx.x * TAAU_TW, by = (int)blockIdx.y * TAAU_TH;
    // the footprint's origin: the nearest sample of the tile's first pixel, less the halo; its extent: up to the nearest sample of the tile's last pixel, plus the halo
    const int ox = TAAU_Nearest(TAAU_Centre(bx, F.rx), F.jx, w) - HALO, oy = TAAU_Nearest(TAAU_Centre(by, F.ry), F.jy, h) - HALO;
    const int nx = min(TAAU_Nearest(TAAU_Centre(bx + TAAU_TW - 1, F.rx), F.jx, w) - ox + 1 + HALO, LW);
    const int ny = min(TAAU_Nearest(TAAU_Centre(by + TAAU_TH - 1, F.ry), F.jy, h) - oy + 1 + HALO, LH);
    for (int i = (int)threadIdx.x; i < nx * ny; i += 256) {
        const int ly = i / nx, lx = i - ly * nx;
        const size_t q = (size_t)TAA_ClampCoord(oy + ly, h) * F.width + TAA_ClampCoord(ox + lx, w);
        sC[ly][lx] = TAA_Colour(colour[q], P.taa.maxRadiance); sM[ly][lx] = TAA_Motion(motion[q]);
    }
    __syncthreads();
    const int X = bx + (int)(threadIdx.x & 31u), Y = by + (int)(threadIdx.x >> 5);
    if (X >= (int)F.displayWidth || Y >= (int)F.displayHeight) return;
    const float u = TAAU_Centre(X, F.rx), v = TAAU_Centre(Y, F.ry);
    const int i0 = TAAU_Nearest(u, F.jx, w), j0 = TAAU_Nearest(v, F.jy, h);
    const int lx = i0 - ox, ly = j0 - oy;      // in [1, nx - 2] x [1, ny - 2]
    TaauTaps T; T.begin(sM[ly - 1][lx - 1]);
    #pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const float ddy = TAAU_Distance(j0 + dy, F.jy, v);
        #pragma unroll
        for (int dx = -1; dx <= 1; dx++)
            T.tap(sC[ly + dy][lx + dx], sM[ly + dy][lx + dx], TAAU_Weight(TAAU_Distance(i0 + dx, F.jx, u), ddy, F.invR2));
    }
    const bool clampRelaxed = history && P.taa.enableHistoryClamping && relax;
    const float3 r = TAAU_Resolve(T, X, Y, history, clampRelaxed ? DN_LoadUnorm8(relax[(size_t)j0 * F.width + i0]) : 0.0f, P, F);
    out[(size_t)Y * F.displayWidth + X] = make_float4(r, 1.0f);
}

void launch_taa_upscale(const float4* colour, const uint2* motion, const unsigned char* relax, const float4* history, float4* out, const TaauParams& P, const TaauFrame& F, hipStream_t st) {
    const dim3 grid((F.displayWidth + TAAU_TW - 1) / TAAU_TW, (F.displayHeight + TAAU_TH - 1) / TAAU_TH);
    hipLaunchKernelGGL(k_taa_upscale, grid, dim3(256), 0, st, colour, motion, relax, history, out, P, F);
}

} // namespace ptk

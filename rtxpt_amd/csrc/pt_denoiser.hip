// mi355pt — the denoiser passes of a realtime stable-plane frame on the device (pt_denoiser.h holds the per-pixel text; this file maps it onto waves).
// One wave of 64 lanes is one 8 x 8 tile of the frame, lane = the Morton index inside the tile (GenericTSPixelToAddress, Utils.hlsli:335-341): a plane's 80-byte records of a wave
// are 5 KB in one piece, and the scan-line buffers are 8-pixel runs per row. One thread per pixel; the NRD pass's neighbour reads are read-only, so nothing needs an atomic.
#include "pt_denoiser.h"

namespace ptk {

// the pixel of this lane: tile = blockIdx.x * 4 + wave (256 threads = four tiles), Morton decode of the lane (x in the even bits, y in the odd bits: Morton16BitEncode)
__device__ __forceinline__ bool dn_pixel(const StablePlanesContext& sp, uint& px, uint& py) {
    const uint tilesX = (sp.C.imageWidth + 7u) / 8u;
    const uint tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint lx = (lane & 1u) | ((lane >> 1) & 2u) | ((lane >> 2) & 4u), ly = ((lane >> 1) & 1u) | ((lane >> 2) & 2u) | ((lane >> 3) & 4u);
    px = (tile % tilesX) * 8u + lx; py = (tile / tilesX) * 8u + ly;
    return px < sp.C.imageWidth && py < sp.C.imageHeight;
}
static dim3 dn_grid(const StablePlanesContext& sp) { const uint tiles = ((sp.C.imageWidth + 7u) / 8u) * ((sp.C.imageHeight + 7u) / 8u); return dim3((tiles + 3u) / 4u); }

__global__ void __launch_bounds__(256) k_dn_prepare_dlss_rr(StablePlanesContext sp, DenoiserParams P, DenoiserBuffers D, float4* __restrict__ out) {
    uint px, py; if (!dn_pixel(sp, px, py)) return;
    DN_PrepareDLSSRR(sp, P, D, px, py, out);
}
__global__ void __launch_bounds__(256) k_dn_prepare_nrd(PathKernelContext k, StablePlanesContext sp, DenoiserParams P, DenoiserBuffers D, uint planeIndex, uint init, uint sampleIndex, float4* __restrict__ out) {
    uint px, py; if (!dn_pixel(sp, px, py)) return;
    float3 o = make_float3(0.0f), d = make_float3(0.0f);
    const uint bid = sp.GetBranchID(px, py, planeIndex);
    if (bid != cStablePlaneInvalidBranchID) k.computeCameraRay(px, py, sampleIndex, o, d);      // (only a plane that hit a surface uses it)
    DN_PrepareNRD(sp, P, D, px, py, planeIndex, init != 0u, o, d, out);
}
__global__ void __launch_bounds__(256) k_dn_merge_nrd(StablePlanesContext sp, DenoiserBuffers D, uint planeIndex, const float4* __restrict__ diff, const float4* __restrict__ spec, float4* __restrict__ out) {
    uint px, py; if (!dn_pixel(sp, px, py)) return;
    DN_MergeNRD(sp, D, px, py, planeIndex, diff, spec, out);
}

void launch_dn_prepare_dlss_rr(const StablePlanesContext& sp, const DenoiserParams& P, const DenoiserBuffers& D, float4* outputColor, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_prepare_dlss_rr, dn_grid(sp), dim3(256), 0, st, sp, P, D, outputColor);
}
void launch_dn_prepare_nrd(const PathKernelContext& k, const StablePlanesContext& sp, const DenoiserParams& P, const DenoiserBuffers& D, uint planeIndex, bool init, uint sampleBaseIndex,
                           float4* outputColor, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_prepare_nrd, dn_grid(sp), dim3(256), 0, st, k, sp, P, D, planeIndex, init ? 1u : 0u, sampleBaseIndex + planeIndex, outputColor);
}
void launch_dn_merge_nrd(const StablePlanesContext& sp, const DenoiserBuffers& D, uint planeIndex, const float4* diff, const float4* spec, float4* outputColor, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_merge_nrd, dn_grid(sp), dim3(256), 0, st, sp, D, planeIndex, diff, spec, outputColor);
}

} // namespace ptk

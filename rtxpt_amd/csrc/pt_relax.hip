// mi355pt — the device denoiser's passes on the device (pt_relax.h holds the per-pixel text; this file maps it onto waves).
// Streaming stencil work. A block of 256 threads is a 32 x 8 pixel tile, a lane one pixel, a wave two rows of 32: every tile read is a 16-byte lane load over 512 contiguous bytes
// per row. The temporal pass packs a pixel's guides once into one 16-byte record; later taps cost that record plus the radiance loads. The 3 x 3 and 5 x 5 work and the a-trous
// steps 1 and 2 stage the tile plus its halo in LDS as separate arrays of 16-byte records (a row of lanes reads consecutive 16-byte slots: no bank conflict at any row length; the
// guide is staged decoded, so a normal is decoded once per staged pixel, not once per tap). Steps 4 to 16 read global memory: their halo would be larger than the tile.
// At most 4 blocks per CU (the largest LDS image, step 2, is 30 KB a block), no scratch.
#include "pt_relax.h"

namespace ptk {

static const int RX_TW = 32, RX_TH = 8;
#define RX_KERNEL __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4)))
static dim3 rx_grid(uint w, uint h) { return dim3((w + RX_TW - 1) / RX_TW, (h + RX_TH - 1) / RX_TH); }
__device__ __forceinline__ bool rx_inside(int x, int y, uint w, uint h) { return x >= 0 && y >= 0 && x < (int)w && y < (int)h; }
__device__ __forceinline__ float4 rx_sky() { return make_float4(kDenoiserViewZSkyMarker, 0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ float4 rx_zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// ---- temporal pass: anti-firefly over the staged 3 x 3, reprojection with a bilinear 2 x 2 of the plane's history, accumulation of radiance, moments and the fast history
RX_KERNEL k_relax_temporal(DenoiserBuffers D, RelaxSettings S, RelaxHistory prev, RelaxHistory cur, float4* __restrict__ guide, uint width, uint height, uint hasHistory) {
    constexpr int HALO = 1, LW = RX_TW + 2 * HALO, LH = RX_TH + 2 * HALO;
    __shared__ __attribute__((aligned(16))) float4 sG[LH][LW], sD[LH][LW], sS[LH][LW];      // viewZ + decoded normal; sanitised radiance + its luminance, diffuse and specular
    const int bx = (int)blockIdx.x * RX_TW, by = (int)blockIdx.y * RX_TH;
    for (int i = (int)threadIdx.x; i < LW * LH; i += 256) {
        const int ly = i / LW, lx = i - ly * LW, x = bx + lx - HALO, y = by + ly - HALO;
        float4 g = rx_sky(), d = rx_zero(), s = rx_zero();
        if (rx_inside(x, y, width, height)) {
            const size_t q = (size_t)y * width + x;
            const float z = D.ViewZ[q];
            if (z != kDenoiserViewZSkyMarker) {
                g = RX_zn(z, OctToNDirUnorm32(NDirToOctUnorm32(xyz(D.NormalRoughness[q]))));
                const float3 cd = RX_finite0(D.DiffRadianceHitDist[q]), cs = RX_finite0(D.SpecRadianceHitDist[q]);
                d = make_float4(cd, Luminance(cd)); s = make_float4(cs, Luminance(cs));
            }
        }
        sG[ly][lx] = g; sD[ly][lx] = d; sS[ly][lx] = s;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & 31u) + HALO, ly = (int)(threadIdx.x >> 5) + HALO, x = bx + lx - HALO, y = by + ly - HALO;
    if (!rx_inside(x, y, width, height)) return;
    const size_t pix = (size_t)y * width + x;
    const float4 g = sG[ly][lx];
    if (g.x == kDenoiserViewZSkyMarker) {
        guide[pix] = RX_PackGuide(kDenoiserViewZSkyMarker, 0u, 0.0f, 0.0f);
        cur.DiffLen[pix] = rx_zero(); cur.SpecLen[pix] = rx_zero(); cur.FastDiffM1[pix] = rx_zero(); cur.FastSpecM1[pix] = rx_zero();
        cur.M2Guide[pix] = make_float4(0.0f, 0.0f, kDenoiserViewZSkyMarker, 0.0f);
        return;
    }
    const float absZ = fabsf(g.x); const float3 n = RX_yzw(g);
    const float thr = RX_DisocclusionThreshold(S, D.DisocclusionThresholdMix[pix]);
    const float coneCos = 1.0f - S.lobeAngleFraction;
    float3 cd = xyz(sD[ly][lx]), cs = xyz(sS[ly][lx]); float ld = sD[ly][lx].w, ls = sS[ly][lx].w;
    if (S.enableAntiFirefly) {
        float maxD = 0.0f, maxS = 0.0f; bool any = false;
        for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
            if (!dx && !dy) continue;
            const float4 t = sG[ly + dy][lx + dx];
            if (t.x == kDenoiserViewZSkyMarker || !RX_SameSurface(absZ, n, fabsf(t.x), RX_yzw(t), thr, coneCos)) continue;
            any = true; maxD = fmaxf_(maxD, sD[ly + dy][lx + dx].w); maxS = fmaxf_(maxS, sS[ly + dy][lx + dx].w);
        }
        if (any) { cd = RX_ClampLuminance(cd, ld, maxD); ld = Luminance(cd); cs = RX_ClampLuminance(cs, ls, maxS); ls = Luminance(cs); }
    }
    // the previous position is pixel + 0.5 + mv.xy; the bilinear 2 x 2 around it, taps in the order (0, 0) (1, 0) (0, 1) (1, 1)
    const float4 mv = SP_UnpackHalf4(D.MotionVectors[pix]);
    const float fx = (((float)x + 0.5f) + mv.x) - 0.5f, fy = (((float)y + 0.5f) + mv.y) - 0.5f;
    float wsum = 0.0f; float4 h0 = rx_zero(), h1 = rx_zero(), h2 = rx_zero(), h3 = rx_zero(); float m2d = 0.0f, m2s = 0.0f;
    if (hasHistory && fabsf(fx) < kRelaxMaxReprojection && fabsf(fy) < kRelaxMaxReprojection) {
        const float flx = floorf(fx), fly = floorf(fy), tx = fx - flx, ty = fy - fly;
        const int ix = (int)flx, iy = (int)fly;
        const float expected = absZ + mv.z;
        const float bw[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            const int qx = ix + (k & 1), qy = iy + (k >> 1);
            if (!rx_inside(qx, qy, width, height) || !(bw[k] > 0.0f)) continue;
            const size_t q = (size_t)qy * width + qx;
            const float4 m = prev.M2Guide[q];
            if (m.z == kDenoiserViewZSkyMarker || !RX_SameSurface(expected, n, fabsf(m.z), OctToNDirUnorm32(asuint(m.w)), thr, coneCos)) continue;
            wsum = wsum + bw[k];
            h0 = RX_madd(h0, prev.DiffLen[q], bw[k]); h1 = RX_madd(h1, prev.SpecLen[q], bw[k]); h2 = RX_madd(h2, prev.FastDiffM1[q], bw[k]); h3 = RX_madd(h3, prev.FastSpecM1[q], bw[k]);
            m2d = m2d + m.x * bw[k]; m2s = m2s + m.y * bw[k];
        }
    }
    const bool valid = wsum > 0.0f;
    if (valid) { h0 = RX_div(h0, wsum); h1 = RX_div(h1, wsum); h2 = RX_div(h2, wsum); h3 = RX_div(h3, wsum); m2d = m2d / wsum; m2s = m2s / wsum; }
    const RelaxAccum ad = RX_Accumulate(valid, cd, ld, h0, h2, m2d, S.diffuseMaxAccumulatedFrameNum, S.diffuseMaxFastAccumulatedFrameNum);
    const RelaxAccum as = RX_Accumulate(valid, cs, ls, h1, h3, m2s, S.specularMaxAccumulatedFrameNum, S.specularMaxFastAccumulatedFrameNum);
    const float4 nr = D.NormalRoughness[pix]; const uint oct = NDirToOctUnorm32(xyz(nr));
    cur.DiffLen[pix] = make_float4(ad.acc, ad.len); cur.SpecLen[pix] = make_float4(as.acc, as.len);
    cur.FastDiffM1[pix] = make_float4(ad.fast, ad.m1); cur.FastSpecM1[pix] = make_float4(as.fast, as.m1);
    cur.M2Guide[pix] = make_float4(ad.m2, as.m2, g.x, asfloat(oct));
    guide[pix] = RX_PackGuide(g.x, oct, nr.w, fminf_(ad.len, as.len));
}

// ---- history clamp: the accumulated radiance into the fast history's 3 x 3 mean +- k sigma (where the two histories differ: length beyond the fast cap); writes the clamped
// radiance back as the stored history and, with the temporal variance, as the first a-trous input
RX_KERNEL k_relax_clamp(DenoiserBuffers D, RelaxSettings S, RelaxHistory cur, const float4* __restrict__ guide, float4* __restrict__ outDiff, float4* __restrict__ outSpec, uint width, uint height) {
    constexpr int HALO = 1, LW = RX_TW + 2 * HALO, LH = RX_TH + 2 * HALO;
    __shared__ __attribute__((aligned(16))) float4 sD[LH][LW], sS[LH][LW];      // the fast histories; .w: 1 where the pixel is a tap (inside the frame, not sky), else 0
    const int bx = (int)blockIdx.x * RX_TW, by = (int)blockIdx.y * RX_TH;
    for (int i = (int)threadIdx.x; i < LW * LH; i += 256) {
        const int ly = i / LW, lx = i - ly * LW, x = bx + lx - HALO, y = by + ly - HALO;
        float4 d = rx_zero(), s = rx_zero();
        if (rx_inside(x, y, width, height)) {
            const size_t q = (size_t)y * width + x;
            if (guide[q].x != kDenoiserViewZSkyMarker) { d = cur.FastDiffM1[q]; s = cur.FastSpecM1[q]; d.w = 1.0f; s.w = 1.0f; }
        }
        sD[ly][lx] = d; sS[ly][lx] = s;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & 31u) + HALO, ly = (int)(threadIdx.x >> 5) + HALO, x = bx + lx - HALO, y = by + ly - HALO;
    if (!rx_inside(x, y, width, height)) return;
    const size_t pix = (size_t)y * width + x;
    if (sD[ly][lx].w == 0.0f) { outDiff[pix] = rx_zero(); outSpec[pix] = rx_zero(); return; }
    float4 hd = cur.DiffLen[pix], hs = cur.SpecLen[pix];
    const float m1d = cur.FastDiffM1[pix].w, m1s = cur.FastSpecM1[pix].w; const float4 m2 = cur.M2Guide[pix];
    const bool clampD = hd.w > (float)S.diffuseMaxFastAccumulatedFrameNum, clampS = hs.w > (float)S.specularMaxFastAccumulatedFrameNum;
    if (clampD || clampS) {
        float3 sd = make_float3(0.0f), sd2 = make_float3(0.0f), ss = make_float3(0.0f), ss2 = make_float3(0.0f); float cnt = 0.0f;
        for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
            const float4 d = sD[ly + dy][lx + dx], s = sS[ly + dy][lx + dx];
            if (d.w == 0.0f) continue;
            cnt = cnt + 1.0f; sd = sd + xyz(d); sd2 = sd2 + xyz(d) * xyz(d); ss = ss + xyz(s); ss2 = ss2 + xyz(s) * xyz(s);
        }
        const float relax = DN_LoadUnorm8(D.CombinedHistoryClampRelax[pix]);
        if (clampD) { hd = make_float4(RX_ClampToFast(xyz(hd), sd, sd2, cnt, relax), hd.w); cur.DiffLen[pix] = hd; }
        if (clampS) { hs = make_float4(RX_ClampToFast(xyz(hs), ss, ss2, cnt, relax), hs.w); cur.SpecLen[pix] = hs; }
    }
    outDiff[pix] = make_float4(xyz(hd), fmaxf_(m2.x - m1d * m1d, 0.0f));
    outSpec[pix] = make_float4(xyz(hs), fmaxf_(m2.y - m1s * m1s, 0.0f));
}

// ---- a-trous: 5 x 5 taps at step `step`, diffuse and specular in one kernel, taps in scan-line order. STEP 1 / 2: the tile and its halo from LDS; STEP 0: taps from global memory
template <int STEP, bool FIRST>
RX_KERNEL k_relax_atrous(DenoiserBuffers D, RelaxSettings S, const float4* __restrict__ guide, const float4* __restrict__ inDiff, const float4* __restrict__ inSpec,
                         float4* __restrict__ outDiff, float4* __restrict__ outSpec, uint step, uint last, uint width, uint height) {
    constexpr int HALO = 2 * (STEP ? STEP : 1), LW = STEP ? RX_TW + 2 * HALO : 1, LH = STEP ? RX_TH + 2 * HALO : 1;
    __shared__ __attribute__((aligned(16))) float4 sG[LH][LW], sD[LH][LW], sS[LH][LW];
    const int bx = (int)blockIdx.x * RX_TW, by = (int)blockIdx.y * RX_TH;
    if (STEP) {
        for (int i = (int)threadIdx.x; i < LW * LH; i += 256) {
            const int ly = i / LW, lx = i - ly * LW, x = bx + lx - HALO, y = by + ly - HALO;
            float4 g = rx_sky(), d = rx_zero(), s = rx_zero();
            if (rx_inside(x, y, width, height)) {
                const size_t q = (size_t)y * width + x;
                g = RX_DecodeGuide(guide[q]);
                if (g.x != kDenoiserViewZSkyMarker) { d = inDiff[q]; s = inSpec[q]; }
            }
            sG[ly][lx] = g; sD[ly][lx] = d; sS[ly][lx] = s;
        }
        __syncthreads();
    }
    const int tx = (int)(threadIdx.x & 31u), ty = (int)(threadIdx.x >> 5), x = bx + tx, y = by + ty;
    if (!rx_inside(x, y, width, height)) return;
    const size_t pix = (size_t)y * width + x;
    const float4 gRaw = guide[pix];
    if (gRaw.x == kDenoiserViewZSkyMarker) { outDiff[pix] = rx_zero(); outSpec[pix] = rx_zero(); return; }
    const int st = STEP ? STEP : (int)step;
    const float4 gC = STEP ? sG[ty + HALO][tx + HALO] : RX_DecodeGuide(gRaw);
    const float4 dC = STEP ? sD[ty + HALO][tx + HALO] : inDiff[pix], sC = STEP ? sS[ty + HALO][tx + HALO] : inSpec[pix];
    RelaxCentre C = RX_Centre(S, gC, gRaw.z, dC, sC);
    if (FIRST && gRaw.w < kRelaxSpatialVarianceBelow) {
        RelaxEstimate E = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int dy = -2; dy <= 2; dy++) for (int dx = -2; dx <= 2; dx++) {
            const float4 gT = sG[ty + HALO + dy * st][tx + HALO + dx * st];
            if (gT.x == kDenoiserViewZSkyMarker) continue;
            RX_EstimateTap(C, RX_B3(dx) * RX_B3(dy), !dx && !dy, gT, sD[ty + HALO + dy * st][tx + HALO + dx * st], sS[ty + HALO + dy * st][tx + HALO + dx * st], E);
        }
        RX_EstimateResolve(E, C);
    }
    RX_CentreSigma(S, C);
    RelaxSums A; A.d = make_float3(0.0f); A.s = make_float3(0.0f); A.vd = A.vs = A.wd = A.ws = 0.0f;
    for (int dy = -2; dy <= 2; dy++) for (int dx = -2; dx <= 2; dx++) {
        float4 gT, dT, sT;
        if (STEP) {
            gT = sG[ty + HALO + dy * st][tx + HALO + dx * st];
            if (gT.x == kDenoiserViewZSkyMarker) continue;      // (outside the frame is staged as sky)
            dT = sD[ty + HALO + dy * st][tx + HALO + dx * st]; sT = sS[ty + HALO + dy * st][tx + HALO + dx * st];
        } else {
            const int qx = x + dx * st, qy = y + dy * st;
            if (!rx_inside(qx, qy, width, height)) continue;
            const size_t q = (size_t)qy * width + qx;
            gT = RX_DecodeGuide(guide[q]);
            if (gT.x == kDenoiserViewZSkyMarker) continue;
            dT = inDiff[q]; sT = inSpec[q];
        }
        RX_FilterTap(C, RX_B3(dx) * RX_B3(dy), !dx && !dy, gT, dT, sT, A);
    }
    float4 od = RX_FilterResolve(A.d, A.vd, A.wd), os = RX_FilterResolve(A.s, A.vs, A.ws);
    if (last) { od.w = 0.0f; os.w = D.SpecRadianceHitDist[pix].w; }
    outDiff[pix] = od; outSpec[pix] = os;
}

void launch_relax_temporal(const DenoiserBuffers& D, const RelaxSettings& S, const RelaxHistory& prev, const RelaxHistory& cur, float4* guide, uint width, uint height, bool hasHistory, hipStream_t st) {
    hipLaunchKernelGGL(k_relax_temporal, rx_grid(width, height), dim3(256), 0, st, D, S, prev, cur, guide, width, height, hasHistory ? 1u : 0u);
}
void launch_relax_clamp(const DenoiserBuffers& D, const RelaxSettings& S, const RelaxHistory& cur, const float4* guide, float4* outDiff, float4* outSpec, uint width, uint height, hipStream_t st) {
    hipLaunchKernelGGL(k_relax_clamp, rx_grid(width, height), dim3(256), 0, st, D, S, cur, guide, outDiff, outSpec, width, height);
}
void launch_relax_atrous(const DenoiserBuffers& D, const RelaxSettings& S, const float4* guide, const float4* inDiff, const float4* inSpec, float4* outDiff, float4* outSpec, uint iteration, bool last,
                         uint width, uint height, hipStream_t st) {
    const dim3 grid = rx_grid(width, height); const uint step = 1u << iteration, l = last ? 1u : 0u;
    if (iteration == 0) hipLaunchKernelGGL((k_relax_atrous<1, true>), grid, dim3(256), 0, st, D, S, guide, inDiff, inSpec, outDiff, outSpec, step, l, width, height);
    else if (iteration == 1) hipLaunchKernelGGL((k_relax_atrous<2, false>), grid, dim3(256), 0, st, D, S, guide, inDiff, inSpec, outDiff, outSpec, step, l, width, height);
    else hipLaunchKernelGGL((k_relax_atrous<0, false>), grid, dim3(256), 0, st, D, S, guide, inDiff, inSpec, outDiff, outSpec, step, l, width, height);
}

} // namespace ptk

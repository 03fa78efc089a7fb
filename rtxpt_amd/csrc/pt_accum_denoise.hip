// mi355pt — the reference-mode denoiser on the device (pt_accum_denoise.h holds the per-pixel text; this file maps it onto waves). Two kernels per call, blocks of 256 threads:
//   k_accum_denoise_prepare  a lane is one pixel, a wave 64 consecutive ones of a row. Writes the staged halves H' (valid(p) in .w) and O' and the variance V; V's 3 x 3 box
//                            re-derives s of the nine neighbours from A and H (cached lines), so the pass is one launch and no intermediate s exists.
//   k_accum_denoise_filter   a workgroup owns a 16 x 16 tile, a lane one pixel of it. With g = r + f and T = 16 + 2 g, the tile plus a halo of g goes to dynamic LDS as nine
//                            planes of T x T floats (H', O', V by channel; coordinates clamped to the frame, an edge pixel repeats) and one plane of T x T bytes (1 where the
//                            position is inside the frame and valid: the only pixels that may receive weight). Then, per search offset o, oy outer and ox inner:
//                              1. e of both directions over the extended tile of E x E positions, E = 16 + 2 f (at most 484: two a lane). A position outside the frame stands for
//                                 the clamped pixel q, and e(q) pairs q with clamp(q + o) — not with the position's own neighbour — so a lane keeps q's slot and q's nine
//                                 values in registers from before the loop and reads only the nine values at q + o: the loop has no bounds test;
//                              2. row sums, left to right, 16 x E of them for each direction;
//                              3. column sums, top to bottom, by the pixel's lane; weight; w = 0 by the byte plane; the four accumulators in registers.
//                            Two barriers an offset (after 1 and after 2): step 1 of the next offset writes e only after every lane has passed barrier 2, behind the reads of
//                            step 2, and step 2 writes the row sums only after barrier 1, behind the reads of step 3. e costs six divisions per position and offset, not per tap.
//                            LDS: 36 T^2 + T^2 + 8 E^2 + 128 E bytes — 39 060 at r 5, f 2 (four workgroups a CU by LDS, sixteen waves), 60 116 at r 8, f 3 (two workgroups).
//                            All LDS traffic is ds_read_b32 / ds_write_b32 (32 banks, lanes in two groups of 32): a group is two tile rows of 16, T floats apart, so for
//                            T mod 32 != 16 part of a group's reads of the staged planes take a second cycle; the e and row-sum planes are read and written at consecutive
//                            addresses. No atomics, no scratch.
#include "pt_accum_denoise.h"

namespace ptk {

static const int AD_TILE = kAccumDenoiseTile, AD_THREADS = AD_TILE * AD_TILE;

size_t accum_denoise_lds_bytes(int r, int f) {
    const size_t T = (size_t)(AD_TILE + 2 * (r + f)), E = (size_t)(AD_TILE + 2 * f);
    return 9u * T * T * sizeof(float) + 2u * E * E * sizeof(float) + 2u * E * AD_TILE * sizeof(float) + T * T;
}

__global__ void __launch_bounds__(256)
k_accum_denoise_prepare(AccumDenoiseArgs a) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= a.width || y >= a.height) return;
    const size_t pix = (size_t)y * (size_t)a.width + (size_t)x;
    float3 Hs, Os;
    const bool valid = AD_Stage(a.A[pix], a.H[pix], a.maxRadiance, Hs, Os);
    a.stageH[pix] = make_float4(Hs, valid ? 1.0f : 0.0f);
    a.stageO[pix] = make_float4(Os, 0.0f);
    a.var[pix] = make_float4(AD_Variance(a.A, a.H, x, y, a.width, a.height, a.maxRadiance), 0.0f);
}

__global__ void __launch_bounds__(256)
k_accum_denoise_filter(AccumDenoiseArgs a) {
    extern __shared__ float adLds[];
    const int r = a.r, f = a.f, g = r + f, T = AD_TILE + 2 * g, TT = T * T, E = AD_TILE + 2 * f, EE = E * E, patch = 2 * f + 1;
    float* __restrict__ sU = adLds;                       // nine planes: H'.x H'.y H'.z O'.x O'.y O'.z V.x V.y V.z
    float* __restrict__ sE = sU + 9 * TT;                 // e: [2][E x E]
    float* __restrict__ sR = sE + 2 * EE;                 // row sums: [2][E rows x 16]
    unsigned char* __restrict__ sM = (unsigned char*)(sR + 2 * E * AD_TILE);
    const int tid = (int)threadIdx.x, lx = tid & (AD_TILE - 1), ly = tid >> 4;
    const int x0 = (int)blockIdx.x * AD_TILE, y0 = (int)blockIdx.y * AD_TILE;

    for (int i = tid; i < TT; i += AD_THREADS) {
        const int sy = i / T, sx = i - sy * T, gx = x0 - g + sx, gy = y0 - g + sy;
        const size_t p = (size_t)TAA_ClampCoord(gy, a.height) * (size_t)a.width + (size_t)TAA_ClampCoord(gx, a.width);
        const float4 h = a.stageH[p], o = a.stageO[p], v = a.var[p];
        sU[i] = h.x; sU[TT + i] = h.y; sU[2 * TT + i] = h.z; sU[3 * TT + i] = o.x; sU[4 * TT + i] = o.y; sU[5 * TT + i] = o.z;
        sU[6 * TT + i] = v.x; sU[7 * TT + i] = v.y; sU[8 * TT + i] = v.z;
        sM[i] = (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height && h.w != 0.0f) ? 1 : 0;
    }
    __syncthreads();

    // step 1's positions of this lane: tid and tid + 256 of the E x E extended tile; slot: the staged slot of the clamped pixel
    int slot[2]; float c[2][9]; bool has[2];
    #pragma unroll
    for (int t = 0; t < 2; t++) {
        const int i = tid + t * AD_THREADS;
        has[t] = i < EE;
        const int ey = has[t] ? i / E : 0, ex = has[t] ? i - ey * E : 0;
        const int qx = TAA_ClampCoord(x0 - f + ex, a.width), qy = TAA_ClampCoord(y0 - f + ey, a.height);
        slot[t] = (qy - y0 + g) * T + (qx - x0 + g);
        #pragma unroll
        for (int k = 0; k < 9; k++) c[t][k] = sU[k * TT + slot[t]];
    }
    // step 2's sums of this lane: tid and tid + 256 of the 16 x E row sums
    const int rows = E * AD_TILE;
    int rsrc[2]; bool rhas[2];
    #pragma unroll
    for (int t = 0; t < 2; t++) {
        const int j = tid + t * AD_THREADS;
        rhas[t] = j < rows;
        const int ry = rhas[t] ? j >> 4 : 0, rx = j & (AD_TILE - 1);
        rsrc[t] = ry * E + rx;
    }
    const int centre = (ly + g) * T + (lx + g);
    const float norm = AD_PatchNorm(f);
    float sumWH = 0.0f, sumWO = 0.0f;
    float3 sumCH = make_float3(0.0f), sumCO = make_float3(0.0f);

    for (int oy = -r; oy <= r; oy++) {
        for (int ox = -r; ox <= r; ox++) {
            const int off = oy * T + ox;
            #pragma unroll
            for (int t = 0; t < 2; t++) {
                if (!has[t]) continue;
                const int n = slot[t] + off;
                const float vx = sU[6 * TT + n], vy = sU[7 * TT + n], vz = sU[8 * TT + n];
                const float eH = (AD_Distance(c[t][0], sU[n], c[t][6], vx, a.alpha, a.epsilon, a.kk) + AD_Distance(c[t][1], sU[TT + n], c[t][7], vy, a.alpha, a.epsilon, a.kk)) +
                                 AD_Distance(c[t][2], sU[2 * TT + n], c[t][8], vz, a.alpha, a.epsilon, a.kk);
                const float eO = (AD_Distance(c[t][3], sU[3 * TT + n], c[t][6], vx, a.alpha, a.epsilon, a.kk) + AD_Distance(c[t][4], sU[4 * TT + n], c[t][7], vy, a.alpha, a.epsilon, a.kk)) +
                                 AD_Distance(c[t][5], sU[5 * TT + n], c[t][8], vz, a.alpha, a.epsilon, a.kk);
                sE[tid + t * AD_THREADS] = eH; sE[EE + tid + t * AD_THREADS] = eO;
            }
            __syncthreads();
            #pragma unroll
            for (int t = 0; t < 2; t++) {
                if (!rhas[t]) continue;
                float sH = sE[rsrc[t]], sO = sE[EE + rsrc[t]];
                for (int i = 1; i < patch; i++) { sH = sH + sE[rsrc[t] + i]; sO = sO + sE[EE + rsrc[t] + i]; }
                sR[tid + t * AD_THREADS] = sH; sR[rows + tid + t * AD_THREADS] = sO;
            }
            __syncthreads();
            float SH = sR[tid], SO = sR[rows + tid];
            for (int j = 1; j < patch; j++) { SH = SH + sR[tid + j * AD_TILE]; SO = SO + sR[rows + tid + j * AD_TILE]; }
            const int n = centre + off;
            const bool take = sM[n] != 0;
            const float wH = take ? AD_Weight(SH, norm) : 0.0f, wO = take ? AD_Weight(SO, norm) : 0.0f;
            // weights from H' average O', weights from O' average H'
            sumWH = sumWH + wH; sumCH = sumCH + make_float3(sU[3 * TT + n], sU[4 * TT + n], sU[5 * TT + n]) * wH;
            sumWO = sumWO + wO; sumCO = sumCO + make_float3(sU[n], sU[TT + n], sU[2 * TT + n]) * wO;
        }
    }

    const int x = x0 + lx, y = y0 + ly;
    if (x >= a.width || y >= a.height) return;
    const size_t pix = (size_t)y * (size_t)a.width + (size_t)x;
    const float4 A = a.A[pix];
    float4 D = A;      // an invalid pixel keeps A's bytes; alpha is always A's
    if (sM[centre]) {
        const float3 FO = make_float3(sumCH.x / sumWH, sumCH.y / sumWH, sumCH.z / sumWH), FH = make_float3(sumCO.x / sumWO, sumCO.y / sumWO, sumCO.z / sumWO);
        const float3 d = (FO + FH) * 0.5f;
        D.x = d.x; D.y = d.y; D.z = d.z;
    }
    a.out[pix] = D;
}

hipError_t launch_accum_denoise(const AccumDenoiseArgs& a, hipStream_t st) {
    const size_t lds = accum_denoise_lds_bytes(a.r, a.f);
    const dim3 gp(((uint)a.width + 63u) / 64u, ((uint)a.height + 3u) / 4u), gf(((uint)a.width + AD_TILE - 1u) / AD_TILE, ((uint)a.height + AD_TILE - 1u) / AD_TILE);
    if (lds > 64u * 1024u) return hipErrorInvalidValue;      // (not reached: r <= 8 and f <= 3 give 60 116 bytes)
    hipLaunchKernelGGL(k_accum_denoise_prepare, gp, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_accum_denoise_filter, gf, dim3(AD_THREADS), lds, st, a);
    return hipGetLastError();
}

} // namespace ptk

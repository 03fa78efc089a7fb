// mi355pt — the bloom pass between the temporal anti-aliasing resolve and the tone mapper (pt_bloom): the seam of Sample::PostProcessPreToneMapping (Sample.cpp:1827-1837), which
// runs BloomPass::Render in place on ProcessedOutputColor unless !(EnableBloom && BloomIntensity > 0 && BloomRadius > 0). The pass itself is Donut's and is not in the reference
// tree: the filter is our own (docs/WIDENING.md N7), not Donut's text, and is not compared with Donut's output; the three defaults, the slider ranges and the skip condition that
// have a citation in include/mi355pt.h are the reference's. One separable Gaussian over a quarter-resolution copy, blended back by a constant factor.
// This file holds the per-texel text; pt_bloom.hip maps it onto waves.
// Part of the PRODUCT path (libmi355pt.so). Arithmetic contract of pt_vec.h, as pt_taa.h: one binary32 operation at a time in the written order, no contraction; only + - x /,
// floorf, min / max / compare on the device (the taps' exp is evaluated on the host, in double), so that tests/bloom_ref.py restates every value bit for bit.
#pragma once
#include "pt_taa.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

static const int kBloomMaxTaps = 48;      // R <= ceil(3 x 0.25 x 64)
static const int kBloomReduce = 4;        // the blur runs on ceil(w / 4) x ceil(h / 4) texels

// the blur's taps (pt_bloom_kernel): g[0 .. R] and their float sum G = 1 + 2 g[1] + ... A kernel argument: uniform, so the tap loop reads it through scalar loads.
struct BloomTaps { float g[kBloomMaxTaps + 1]; float G; uint R; };

static inline float3 Bloom_Sanitise(float4 v, float maxRadiance) { return make_float3(TAA_Sanitise(v.x, maxRadiance), TAA_Sanitise(v.y, maxRadiance), TAA_Sanitise(v.z, maxRadiance)); }

// Q(X, Y): the 4 x 4 block's sanitised texels summed from 0 in scan-line order, then x 0.0625; source coordinates clamped to the frame (an edge texel repeats)
static inline float3 Bloom_Reduce(const float4* __restrict__ src, int X, int Y, uint width, uint height, float maxRadiance) {
    float3 acc = make_float3(0.0f);
    #pragma unroll
    for (int j = 0; j < kBloomReduce; j++) {
        const float4* __restrict__ row = src + (size_t)TAA_ClampCoord(Y * kBloomReduce + j, (int)height) * width;
        float4 t[kBloomReduce];
        #pragma unroll
        for (int i = 0; i < kBloomReduce; i++) t[i] = row[TAA_ClampCoord(X * kBloomReduce + i, (int)width)];
        #pragma unroll
        for (int i = 0; i < kBloomReduce; i++) acc = acc + Bloom_Sanitise(t[i], maxRadiance);
    }
    return acc * 0.0625f;
}

// one axis of the blur: at(0) is the centre, at(-i) and at(i) the texels i steps to each side (coordinates already clamped by whoever staged them).
// acc = c x g[0]; acc = acc + (l_i + r_i) x g[i], i = 1 .. R; the result is acc / G
template <class Fetch> static inline float3 Bloom_Blur(Fetch at, const BloomTaps& K) {
    float3 acc = at(0) * K.g[0];
    #pragma unroll 2
    for (int i = 1; i <= (int)K.R; i++) acc = acc + (at(-i) + at(i)) * K.g[i];
    return make_float3(acc.x / K.G, acc.y / K.G, acc.z / K.G);
}

// the fraction and the first tap of full-resolution coordinate x in the quarter-resolution image: u = (x + 0.5) x 0.25 - 0.5 (t is one of 0.125, 0.375, 0.625, 0.875, exact)
static inline float Bloom_Tap(int x, int& i) { const float u = ((float)x + 0.5f) * 0.25f - 0.5f, fl = floorf(u); i = (int)fl; return u - fl; }

// the blurred image B [qh][qw] at full-resolution pixel (x, y): bilinear, the 2 x 2 in the order (0, 0) (1, 0) (0, 1) (1, 1) summed from 0, coordinates clamped
static inline float3 Bloom_Upsample(const float4* __restrict__ B, int x, int y, int qw, int qh) {
    int ix, iy; const float tx = Bloom_Tap(x, ix), ty = Bloom_Tap(y, iy);
    const float bw[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
    float3 r = make_float3(0.0f);
    #pragma unroll
    for (int k = 0; k < 4; k++) r = TAA_madd(r, B[(size_t)TAA_ClampCoord(iy + (k >> 1), qh) * qw + TAA_ClampCoord(ix + (k & 1), qw)], bw[k]);
    return r;
}

// out = s + (b - s) x intensity
static inline float3 Bloom_Composite(float3 s, float3 b, float intensity) { return s + (b - s) * intensity; }

#pragma clang force_cuda_host_device end

static inline uint bloom_reduced(uint n) { return (n + (uint)kBloomReduce - 1u) / (uint)kBloomReduce; }

// src: the full-resolution picture [height][width]; q0, q1: two quarter-resolution buffers of bloom_reduced(width) x bloom_reduced(height) texels (Q and B in q0, T in q1);
// out: the bloomed picture. Four kernels on st.
void launch_bloom(const float4* src, float4* q0, float4* q1, float4* out, const BloomTaps& K, float intensity, float maxRadiance, uint width, uint height, hipStream_t st);
} // namespace ptk

// mi355pt device/host leaf library — stochastic texture filtering: ONE stored texel per material lookup, chosen at random so that its expectation is the filtered value.
// The seam is the reference's (Bridge::loadSurface builds one STF_SamplerState per call from four random numbers and hands it to every lookup of the surface,
// PathTracerBridgeDonut.hlsli:637-664, TextureSampler.hlsli:57-72, 96-116; the settings STFFilterMode / STFMagnificationMethod / STFGaussianSigma, PathTracerShared.h:88-90,
// SampleUI.h:185-187). The sampler itself is the project's own: the library the reference calls (External/Rtxtf) is not part of its tree, so nothing here is compared with it.
// Host-and-device text like pt_scene.h, and written with what pt_scene.h has.
//
// The definition (lambda = the level sampleTexture forms, pt_path.h; u = four numbers in [0, 1)):
//   level   l, l0, m0, m1, f exactly as sample_trilinear forms them (m1 clamped to the last level).
//           LINEAR, CUBIC: m = (u.z < f) ? m1 : m0 — f == 0 never reads m1, and P(m1) = f: the blend of the two levels in expectation.
//           POINT:         m = (f < 0.5f) ? m0 : m1, u is not read.
//   texel   at level m, sides mw, mh as sample_bilinear forms them; per axis (y the same with uv.y, mh, u.y):
//           POINT   x = floorf(uv.x * mw)                                  (no half-texel shift: the texel whose area holds the coordinate)
//           LINEAR  fx = uv.x * mw - 0.5f, flx = floorf(fx), ax = fx - flx,  x = flx + (u.x < ax ? 1 : 0)           P(flx + 1) = ax: the bilinear value in expectation
//           CUBIC   the same flx, ax; the uniform cubic B-spline's weights of the taps flx - 1 .. flx + 2 (stf_bspline_weights: all four >= 0 on [0, 1)), then
//                   c0 = w0, c1 = c0 + w1, c2 = c1 + w2, k = (u.x >= c0) + (u.x >= c1) + (u.x >= c2), x = flx - 1 + k   (the last tap takes what is left of [0, 1))
//   wrap    applied to the FINAL integer-valued coordinate, by sample_bilinear's two routes: the exact power-of-two scaling where both sides are powers of two, wrap_texel_npot
//           otherwise. Both give the exact remainder for |x| up to 2^30, so the far range of the deterministic samplers carries over and nothing leans on tex_texel's
//           one-period conditional for the taps at -1 and +2.
//   value   the stored float4 at (m, x, y), returned as it is: no arithmetic touches the texel, so "bit for bit" is a statement about which texel was picked.
// uv and lambda must be finite (the samplers' data contract); the last clamp only keeps the fetch of a NaN coordinate in bounds.
//
// NOT HERE (pt_set_texture_filtering answers PT_ERROR_UNSUPPORTED): the GAUSSIAN filter — it needs a Box-Muller transform through the dm_* polynomials (pt_dmath.h) and a
// restatement of those for the tests; left for later — and every magnification method but Default (the 2x2 / 3x3 / 4x4 quad-sharing methods).
#pragma once
#include "pt_scene.h"
#include "pt_rng.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

// StfFilterMode's values (include/mi355pt.h PT_STF_FILTER_*); STF_OFF: the deterministic trilinear sampler
enum : int { STF_OFF = -1, STF_POINT = 0, STF_LINEAR = 1, STF_CUBIC = 2, STF_GAUSSIAN = 3 };

// the key of one loadSurface call's random numbers: pixel, path vertex and sample — never a pool slot or a queue position
struct StfKey { uint pixel, vertex, sample; };
struct StfNoKey {};      // (the deterministic instantiations pass this: no data)
struct StfPick { uint mip; int x, y; };

// BridgeDonut:648-650: SampleGeneratorVertexBase::make(pixelPos, pathVertexIndex, sampleIndex), the SampleGenerator on it with its default arguments (effect seed Base, uniform
// mode), sampleNext4D = four sampleNext1D in a row
static inline float4 stf_draw(uint packedPixel, uint vertexIndex, uint sampleIndex) {
    SampleGeneratorVertexBase vb = SampleGeneratorVertexBase::make(packedPixel, vertexIndex, sampleIndex);
    SampleSequenceGenerator sg = SampleSequenceGenerator::make(vb);
    float4 u; u.x = sampleNext1D(sg); u.y = sampleNext1D(sg); u.z = sampleNext1D(sg); u.w = sampleNext1D(sg);
    return u;
}

// the uniform cubic B-spline at fraction t in [0, 1), taps -1 .. +2, in float32 and in THIS order of operations (tests/stf_ref.py restates it):
//   s = 1 - t
//   w0 = ((s * s) * s) * (1/6)
//   w1 = ((((3 t) - 6) * t) * t + 4) * (1/6)
//   w2 = (((((-3 t) + 3) * t + 3) * t) + 1) * (1/6)
//   w3 = ((t * t) * t) * (1/6)
// w0, w3 are cubes of non-negative numbers; the polynomials of w1 and w2 stay in [1, 4] on [0, 1]: every weight is >= 0 in float32 too
static inline void stf_bspline_weights(float t, float w[4]) {
    const float sixth = 1.0f / 6.0f, s = 1.0f - t;
    w[0] = ((s * s) * s) * sixth;
    w[1] = ((((3.0f * t) - 6.0f) * t) * t + 4.0f) * sixth;
    w[2] = (((((-3.0f * t) + 3.0f) * t + 3.0f) * t) + 1.0f) * sixth;
    w[3] = ((t * t) * t) * sixth;
}
// one axis: the integer-valued coordinate before the wrap
template <int FILTER> static inline float stf_axis(float coord, float side, float u) {
    if (FILTER == STF_POINT) return floorf(coord * side);
    const float fx = coord * side - 0.5f, flx = floorf(fx), ax = fx - flx;
    if (FILTER == STF_LINEAR) return flx + (u < ax ? 1.0f : 0.0f);
    float w[4]; stf_bspline_weights(ax, w);
    const float c0 = w[0], c1 = c0 + w[1], c2 = c1 + w[2];
    const float k = (u >= c0 ? 1.0f : 0.0f) + (u >= c1 ? 1.0f : 0.0f) + (u >= c2 ? 1.0f : 0.0f);
    return (flx - 1.0f) + k;
}
template <int FILTER> static inline StfPick stf_pick(const TexInfo& t, float2 uv, float lambda, float4 u) {
    static_assert(FILTER == STF_POINT || FILTER == STF_LINEAR || FILTER == STF_CUBIC, "POINT, LINEAR or CUBIC");
    float maxl = (float)(t.mipLevels - 1);
    float l = clampf(lambda, 0.0f, maxl);
    float l0 = floorf(l);
    uint m0 = (uint)l0, m1 = m0 + 1; if (m1 > t.mipLevels - 1) m1 = t.mipLevels - 1;
    float f = l - l0;
    const uint mip = (FILTER == STF_POINT) ? ((f < 0.5f) ? m0 : m1) : ((u.z < f) ? m1 : m0);
    uint mw = t.w >> mip; if (mw < 1u) mw = 1u;
    uint mh = t.h >> mip; if (mh < 1u) mh = 1u;
    const float fmw = (float)mw, fmh = (float)mh;
    float x = stf_axis<FILTER>(uv.x, fmw, u.x), y = stf_axis<FILTER>(uv.y, fmh, u.y);
    // the wrap of the final coordinate: sample_bilinear's two routes (pt_scene.h)
    if (((mw & (mw - 1u)) | (mh & (mh - 1u))) == 0u) { x = x - floorf(x * asfloat(0x7F000000u - asuint(fmw))) * fmw; y = y - floorf(y * asfloat(0x7F000000u - asuint(fmh))) * fmh; }
    else { x = wrap_texel_npot(x, fmw); y = wrap_texel_npot(y, fmh); }
    int xi = (int)x, yi = (int)y;
    xi = xi < 0 ? 0 : (xi >= (int)mw ? (int)mw - 1 : xi);
    yi = yi < 0 ? 0 : (yi >= (int)mh ? (int)mh - 1 : yi);
    StfPick p; p.mip = mip; p.x = xi; p.y = yi;
    return p;
}
static inline const float4& stf_texel(const DeviceScene& sc, const TexInfo& t, const StfPick& p) {
    uint mw = t.w >> p.mip; if (mw < 1u) mw = 1u;
    return sc.texels[t.base + t.mipOffset[p.mip] + (unsigned long long)p.y * mw + (uint)p.x];
}
// the lookup: one 16-byte load
template <int FILTER> static inline float4 sample_stochastic(const DeviceScene& sc, const TexInfo& t, float2 uv, float lambda, float4 u) {
    return stf_texel(sc, t, stf_pick<FILTER>(t, uv, lambda, u));
}
// the filter as a run-time value (the probe, the host check); `filter` must be POINT, LINEAR or CUBIC
static inline StfPick stf_pick_filter(int filter, const TexInfo& t, float2 uv, float lambda, float4 u) {
    return filter == STF_POINT ? stf_pick<STF_POINT>(t, uv, lambda, u) : (filter == STF_CUBIC ? stf_pick<STF_CUBIC>(t, uv, lambda, u) : stf_pick<STF_LINEAR>(t, uv, lambda, u));
}

#pragma clang force_cuda_host_device end
} // namespace ptk

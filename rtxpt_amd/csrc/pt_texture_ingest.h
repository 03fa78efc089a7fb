// mi355pt — what a texture upload makes of its source, as one text for the host path (pt_api.hip: pt_set_materials, upload_textures) and the device path
// (pt_texture_ingest.hip): the level-0 texel of a source texel, one texel of a mip level from the level above, the opacity rule of the alpha planes, and the layout of a
// texture's levels in the texel pool and of the planes in the alpha pool. Both paths produce the same TexInfo / AlphaPlane tables and the same bits in both pools.
// Arithmetic contract (pt_vec.h): single fp32 operations in the written order, dm_pow for pow().
#pragma once
#include "pt_vec.h"
#include "pt_dmath.h"

namespace ptk {
#pragma clang force_cuda_host_device begin

// the formats of PtTextureDesc (include/mi355pt.h)
enum : uint { TEXI_RGBA8_UNORM = 0u, TEXI_RGBA8_SRGB = 1u, TEXI_RGBA32F = 2u };

// ---- level 0
static inline float texi_srgb_to_linear(float c) { return (c <= 0.04045f) ? c / 12.92f : dm_pow((c + 0.055f) / 1.055f, 2.4f); }
static inline float texi_unorm(uint byte) { return (float)byte / 255.0f; }
// one channel of an 8-bit source: colour channels of an sRGB source go through the transfer function, everything else is k / 255
static inline float texi_channel(uint byte, bool srgbColour) { const float c = texi_unorm(byte); return srgbColour ? texi_srgb_to_linear(c) : c; }
// the level-0 texel of four source bytes (r, g, b, a from the low byte up: the little-endian word of an RGBA8 texel)
static inline float4 texi_level0_rgba8(uint word, uint format) {
    const bool s = format == TEXI_RGBA8_SRGB;
    return make_float4(texi_channel(word & 0xFFu, s), texi_channel((word >> 8) & 0xFFu, s), texi_channel((word >> 16) & 0xFFu, s), texi_channel(word >> 24, false));
}
// (a float source passes through unchanged)

// ---- the chain: sides max(1, side >> l); texel (x, y) of a level of mw texels a row from the level above (pw x ph), source indices clamped to an odd side's last texel
static inline uint texi_side(uint side, uint level) { const uint s = side >> level; return s ? s : 1u; }
static inline uint texi_level_count(uint w, uint h) { uint lv = 1u, m = w > h ? w : h; while (m > 1u) { m >>= 1; lv++; } return lv; }
static inline float4 texi_mip_texel(const float4* p, uint pw, uint ph, uint x, uint y) {
    const uint x0 = (2u * x < pw - 1u) ? 2u * x : pw - 1u, x1 = (2u * x + 1u < pw - 1u) ? 2u * x + 1u : pw - 1u;
    const uint y0 = (2u * y < ph - 1u) ? 2u * y : ph - 1u, y1 = (2u * y + 1u < ph - 1u) ? 2u * y + 1u : ph - 1u;
    const float4 s = (p[(size_t)y0 * pw + x0] + p[(size_t)y0 * pw + x1]) + (p[(size_t)y1 * pw + x0] + p[(size_t)y1 * pw + x1]);
    return s * 0.25f;
}

// ---- the opacity rule. A texture's alpha plane holds one byte per texel where every opacity of level 0 is k / 255 — in [0, 1] and returned by the quotient of its own
// rounded byte — and one float per texel otherwise. Every 8-bit source is a byte plane by construction: its opacity is (float)k / 255.0f, k * (1 / 255) * 255 + 0.5 lies
// within 2^-15 of k + 0.5, so the truncation gives k back for all 256 values (tests/test_texture_ingest_host.py runs all of them through this function).
static inline int texi_alpha_byte(float a) { return (int)(a * 255.0f + 0.5f); }
static inline bool texi_alpha_is_byte(float a) { const int q = (a >= 0.f && a <= 1.f) ? texi_alpha_byte(a) : -1; return q >= 0 && (float)q / 255.0f == a; }

// ---- the layout. A texture's levels follow each other in the texel pool, level 0 first: mipOffset[l] in texels from the texture's base, at most 16 levels.
// Returns the texels of the whole chain.
static inline size_t texi_layout(uint w, uint h, uint* mipLevels, uint mipOffset[16]) {
    const uint lv = texi_level_count(w, h); size_t off = 0;
    for (uint l = 0; l < 16u; l++) mipOffset[l] = 0u;
    for (uint l = 0; l < lv && l < 16u; l++) { mipOffset[l] = (uint)off; off += (size_t)texi_side(w, l) * texi_side(h, l); }
    *mipLevels = lv;
    return off;
}
// the alpha pool: every plane starts on a 16-byte boundary (zero bytes in between), the pool ends on one and is never empty
static inline size_t texi_alpha_align(size_t bytes) { return (bytes + 15u) & ~(size_t)15u; }
static inline size_t texi_alpha_plane_bytes(uint w, uint h, bool bytes) { return (size_t)w * h * (bytes ? 1u : 4u); }
static inline size_t texi_alpha_pool_end(size_t bytes) { const size_t e = texi_alpha_align(bytes); return e ? e : 16u; }

#pragma clang force_cuda_host_device end
} // namespace ptk

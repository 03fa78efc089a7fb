// The stochastic texture filter's text (rtxpt_amd/csrc/pt_stf.h is host-and-device text) run on the HOST: a stand-alone program that tests/test_stf_reference.py builds
// twice — plainly, and with -fsanitize=address,undefined — and holds to tests/stf_ref.py bit for bit in level, x, y and texel. Each texture's texels and its TexInfo stand in
// host allocations of exactly their size: a fetch one texel outside is a sanitizer report, so is a float-to-int conversion out of range. Mips are built as pt_api.hip builds
// them (tests/texture_host_check.hip has the same lines).
//   stf_host_check <in> <out>
//   in : u32 nTextures, u32 nRows; per texture u32 w, u32 h, w * h float4 texels of level 0; nRows x 12 u32 probe rows (include/mi355pt_testhooks.h kind 12)
//   out: per row 8 u32 — mode 0: the texel, level, x, y, 0; mode 1: the four numbers stf_draw forms for (packed pixel, vertex, sample), 0 0 0 0
//   stdout: "ok"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "pt_stf.h"

namespace ptk {      // (inside the product's namespace: its float2 / float4 / uint are not HIP's)

struct HostTex { TexInfo* info; float4* texels; DeviceScene sc; };

static void build(HostTex& t, uint w, uint h, const float4* level0) {
    std::vector<std::vector<float4>> mips(1); mips[0].assign(level0, level0 + (size_t)w * h);
    uint lv = 1; { uint m = std::max(w, h); while (m > 1) { m >>= 1; lv++; } }
    mips.resize(lv);
    for (uint l = 1; l < lv; l++) {
        uint pw = std::max(1u, w >> (l - 1)), ph = std::max(1u, h >> (l - 1)), mw = std::max(1u, w >> l), mh = std::max(1u, h >> l);
        mips[l].resize((size_t)mw * mh); const std::vector<float4>& p = mips[l - 1];
        for (uint y = 0; y < mh; y++) for (uint x = 0; x < mw; x++) {
            uint x0 = std::min(2 * x, pw - 1), x1 = std::min(2 * x + 1, pw - 1), y0 = std::min(2 * y, ph - 1), y1 = std::min(2 * y + 1, ph - 1);
            float4 s = (p[(size_t)y0 * pw + x0] + p[(size_t)y0 * pw + x1]) + (p[(size_t)y1 * pw + x0] + p[(size_t)y1 * pw + x1]);
            mips[l][(size_t)y * mw + x] = s * 0.25f;
        }
    }
    t.info = (TexInfo*)malloc(sizeof(TexInfo)); memset(t.info, 0, sizeof(TexInfo)); t.info->w = w; t.info->h = h; t.info->mipLevels = lv; t.info->base = 0;
    std::vector<float4> pool; for (uint l = 0; l < lv; l++) { t.info->mipOffset[l] = (uint)pool.size(); pool.insert(pool.end(), mips[l].begin(), mips[l].end()); }
    t.texels = (float4*)malloc(pool.size() * sizeof(float4)); memcpy(t.texels, pool.data(), pool.size() * sizeof(float4));
    memset(&t.sc, 0, sizeof(t.sc));
    t.sc.textures = t.info; t.sc.texels = t.texels;
}

int run(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    uint hdr[2]; if (fread(hdr, 4, 2, f) != 2) return 2;
    std::vector<HostTex> tex(hdr[0]);
    for (uint i = 0; i < hdr[0]; i++) {
        uint wh[2]; if (fread(wh, 4, 2, f) != 2) return 2;
        std::vector<float4> l0((size_t)wh[0] * wh[1]); if (fread(l0.data(), sizeof(float4), l0.size(), f) != l0.size()) return 2;
        build(tex[i], wh[0], wh[1], l0.data());
    }
    std::vector<uint> rows((size_t)hdr[1] * 12); if (fread(rows.data(), 4, rows.size(), f) != rows.size()) return 2;
    fclose(f);
    std::vector<uint> out((size_t)hdr[1] * 8, 0u);
    for (uint i = 0; i < hdr[1]; i++) {
        const uint* a = &rows[(size_t)i * 12]; uint* o = &out[(size_t)i * 8];
        if (a[0] == 1u) { const float4 u = stf_draw(a[6], a[7], a[8]); o[0] = asuint(u.x); o[1] = asuint(u.y); o[2] = asuint(u.z); o[3] = asuint(u.w); continue; }
        const uint ti = a[1] & 0xFFFFu;
        if (a[0] != 0u || ti >= hdr[0] || a[5] > 2u) { printf("row %u out of range\n", i); return 1; }
        const HostTex& t = tex[ti];
        const uint baseLOD = a[1] >> 24, mipLevels = (a[1] >> 16) & 0xFFu;      // PathKernelContext::sampleTexture's two lines (pt_path.h)
        float lambda = 0.5f * (float)baseLOD + asfloat(a[4]);
        lambda = fminf_(lambda, fmaxf_((float)mipLevels - 5.0f, 0.0f));
        const float2 uv = make_float2(asfloat(a[2]), asfloat(a[3])); const float4 u = make_float4(asfloat(a[6]), asfloat(a[7]), asfloat(a[8]), asfloat(a[9]));
        const StfPick p = stf_pick_filter((int)a[5], *t.info, uv, lambda, u);
        // the compile-time form the kernels use returns the same texel
        const float4 r = a[5] == 0u ? sample_stochastic<STF_POINT>(t.sc, *t.info, uv, lambda, u) : (a[5] == 2u ? sample_stochastic<STF_CUBIC>(t.sc, *t.info, uv, lambda, u) : sample_stochastic<STF_LINEAR>(t.sc, *t.info, uv, lambda, u));
        const float4 q = stf_texel(t.sc, *t.info, p);
        if (asuint(q.x) != asuint(r.x) || asuint(q.y) != asuint(r.y) || asuint(q.z) != asuint(r.z) || asuint(q.w) != asuint(r.w)) { printf("row %u: the two forms differ\n", i); return 1; }
        o[0] = asuint(r.x); o[1] = asuint(r.y); o[2] = asuint(r.z); o[3] = asuint(r.w); o[4] = p.mip; o[5] = (uint)p.x; o[6] = (uint)p.y;
    }
    f = fopen(argv[2], "wb"); if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2; fclose(f);
    for (uint i = 0; i < hdr[0]; i++) { free(tex[i].info); free(tex[i].texels); }
    printf("ok\n");
    return 0;
}
} // namespace ptk

int main(int argc, char** argv) { return ptk::run(argc, argv); }

// The product's own sampler text (rtxpt_amd/csrc/pt_scene.h is host-and-device text) run on the HOST, for a build with -fsanitize=address,undefined
// (tests/test_texture_sampling.py): sample_bilinear, sample_trilinear, sample_grad_anisotropic and alpha_test_slot over probe rows, each texture's texels, its alpha plane,
// its TexInfo and its AlphaRec in host allocations of exactly their size — a fetch one texel or one opacity outside is a sanitizer report, so is a float-to-int
// conversion out of range. Mips and alpha planes are built as pt_api.hip builds them (build_mips, upload_textures).
//   texture_host_check <in> <out>
//   in : u32 nTextures, u32 nRows; per texture u32 w, u32 h, w * h float4 texels of level 0; nRows x 8 u32 probe rows (include/mi355pt_testhooks.h kind 11; mode 0 = the
//        lambda arithmetic of PathKernelContext::sampleTexture followed by sample_trilinear)
//   out: per row 4 floats (the sampler's value) + u32 (alpha_test_slot of that texture at the row's uv: cutoff 0.5, texture coordinates t0 = (0, 0), t1 = (1, 0), t2 = (0, 1))
//   stdout: "ok" and the plane format chosen per texture (0 bytes, 1 floats)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include "pt_scene.h"

namespace ptk {      // (inside the product's namespace: its float2 / float4 / uint are not HIP's)

struct HostTex {
    TexInfo* info; float4* texels; unsigned char* plane; AlphaRec* rec; uint fmt;
    DeviceScene sc;
};

static float4* exact_copy(const std::vector<float4>& v) { float4* p = (float4*)malloc(v.size() * sizeof(float4)); memcpy(p, v.data(), v.size() * sizeof(float4)); return p; }

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
    t.texels = exact_copy(pool);
    const std::vector<float4>& m0 = mips[0];
    bool bytes = true;
    for (size_t k = 0; k < m0.size() && bytes; k++) { const float a = m0[k].w; const int q = (a >= 0.f && a <= 1.f) ? (int)(a * 255.0f + 0.5f) : -1; bytes = q >= 0 && (float)q / 255.0f == a; }
    t.fmt = bytes ? 0u : 1u;
    t.plane = (unsigned char*)malloc(m0.size() * (bytes ? 1u : 4u));
    if (bytes) for (size_t k = 0; k < m0.size(); k++) t.plane[k] = (unsigned char)(int)(m0[k].w * 255.0f + 0.5f);
    else for (size_t k = 0; k < m0.size(); k++) memcpy(t.plane + 4u * k, &m0[k].w, 4);
    t.rec = (AlphaRec*)malloc(sizeof(AlphaRec)); memset(t.rec, 0, sizeof(AlphaRec));
    t.rec->t0 = make_float2(0.f, 0.f); t.rec->t1 = make_float2(1.f, 0.f); t.rec->t2 = make_float2(0.f, 1.f);
    t.rec->tex = 0u; t.rec->cutoff = 0.5f; t.rec->wh = (w & 0xFFFFu) | (h << 16); t.rec->plane = 0u; t.rec->fmt = t.fmt;
    memset(&t.sc, 0, sizeof(t.sc));
    t.sc.textures = t.info; t.sc.texels = t.texels; t.sc.alphaRecs = t.rec; t.sc.alphaPool = t.plane;
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
    std::vector<uint> rows((size_t)hdr[1] * 8); if (fread(rows.data(), 4, rows.size(), f) != rows.size()) return 2;
    fclose(f);
    std::vector<uint> out((size_t)hdr[1] * 5);
    for (uint i = 0; i < hdr[1]; i++) {
        const uint* a = &rows[(size_t)i * 8]; const uint ti = a[0] == 0u ? (a[1] & 0xFFFFu) : a[1];
        if (a[0] > 2u || ti >= hdr[0] || (a[0] == 1u && a[4] >= tex[ti].info->mipLevels)) { printf("row %u out of range\n", i); return 1; }
        const HostTex& t = tex[ti]; const float2 uv = make_float2(asfloat(a[2]), asfloat(a[3])); float4 r;
        if (a[0] == 0u) {                          // PathKernelContext::sampleTexture (pt_path.h)
            const uint baseLOD = a[1] >> 24, mipLevels = (a[1] >> 16) & 0xFFu;
            float lambda = 0.5f * (float)baseLOD + asfloat(a[4]);
            lambda = fminf_(lambda, fmaxf_((float)mipLevels - 5.0f, 0.0f));
            r = sample_trilinear(t.sc, *t.info, uv, lambda);
        }
        else if (a[0] == 1u) r = sample_bilinear(t.sc, *t.info, a[4], uv);
        else r = sample_grad_anisotropic(t.sc, *t.info, uv, make_float2(asfloat(a[4]), asfloat(a[5])), make_float2(asfloat(a[6]), asfloat(a[7])));
        uint* o = &out[(size_t)i * 5]; o[0] = asuint(r.x); o[1] = asuint(r.y); o[2] = asuint(r.z); o[3] = asuint(r.w);
        o[4] = alpha_test_slot(t.sc, 0u, uv.x, uv.y) ? 1u : 0u;
    }
    f = fopen(argv[2], "wb"); if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 2; fclose(f);
    printf("ok");
    for (uint i = 0; i < hdr[0]; i++) { printf(" %u", tex[i].fmt); free(tex[i].info); free(tex[i].texels); free(tex[i].plane); free(tex[i].rec); }
    printf("\n");
    return 0;
}
} // namespace ptk

int main(int argc, char** argv) { return ptk::run(argc, argv); }

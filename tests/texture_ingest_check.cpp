// tests/test_texture_ingest_host.py: rtxpt_amd/csrc/pt_texture_ingest.h on the host, one texel at a time — level 0, the chain, the plane rule and the layout of both pools
// for the textures of the input file — printed as digests the numpy restatement (tests/texture_ingest_ref.py) must reproduce. Also the claim the device path leans on:
// every 8-bit opacity is a byte-plane opacity.
// input:  uint32 count, then per texture uint32 w, h, format and the source pixels (4 or 16 bytes a texel)
// output: "ok <all 256 bytes pass: 0 / 1> <material texels> <alpha pool bytes>", then per texture "base levels planeOffset planeFmt crc(levels) crc(plane) crc(level offsets)"
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "pt_texture_ingest.h"

using namespace ptk;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    uint32_t count = 0; if (fread(&count, 4, 1, f) != 1) return 2;
    bool all256 = true;
    for (uint k = 0; k < 256u; k++) { const float a = texi_channel(k, false); all256 = all256 && texi_alpha_is_byte(a) && texi_alpha_byte(a) == (int)k; }
    struct Line { size_t base; uint levels; size_t plane; uint fmt; unsigned long crcLevels, crcPlane, crcOffsets; };
    std::vector<Line> lines; size_t base = 0, at = 0;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t hdr[3]; if (fread(hdr, 4, 3, f) != 3) return 2;
        const uint w = hdr[0], h = hdr[1], format = hdr[2]; const size_t texels = (size_t)w * h;
        std::vector<unsigned char> src(texels * (format == TEXI_RGBA32F ? 16u : 4u));
        if (fread(src.data(), 1, src.size(), f) != src.size()) return 2;
        uint levels = 0, offs[16]; const size_t total = texi_layout(w, h, &levels, offs);
        std::vector<ptk::float4> pool(total);          // exactly sized: one texel past a level is a sanitizer report
        for (size_t k = 0; k < texels; k++) {
            if (format == TEXI_RGBA32F) memcpy(&pool[k], &src[16 * k], 16);
            else { uint word; memcpy(&word, &src[4 * k], 4); pool[k] = texi_level0_rgba8(word, format); }
        }
        for (uint l = 1; l < levels; l++) {
            const uint pw = texi_side(w, l - 1), ph = texi_side(h, l - 1), mw = texi_side(w, l), mh = texi_side(h, l);
            std::vector<ptk::float4> prev(pool.begin() + offs[l - 1], pool.begin() + offs[l - 1] + (size_t)pw * ph);      // a copy of its own size, for the same reason
            for (uint y = 0; y < mh; y++) for (uint x = 0; x < mw; x++) pool[offs[l] + (size_t)y * mw + x] = texi_mip_texel(prev.data(), pw, ph, x, y);
        }
        bool bytes = true; for (size_t k = 0; k < texels && bytes; k++) bytes = texi_alpha_is_byte(pool[k].w);
        std::vector<unsigned char> plane(texi_alpha_plane_bytes(w, h, bytes));
        for (size_t k = 0; k < texels; k++) { if (bytes) plane[k] = (unsigned char)texi_alpha_byte(pool[k].w); else memcpy(&plane[4 * k], &pool[k].w, 4); }
        at = texi_alpha_align(at);
        Line ln; ln.base = base; ln.levels = levels; ln.plane = at; ln.fmt = bytes ? 0u : 1u;
        ln.crcLevels = crc32(0L, (const Bytef*)pool.data(), (uInt)(pool.size() * 16u)); ln.crcPlane = crc32(0L, plane.data(), (uInt)plane.size());
        ln.crcOffsets = crc32(0L, (const Bytef*)offs, (uInt)(4u * levels));
        lines.push_back(ln); base += total; at += plane.size();
    }
    fclose(f);
    printf("ok %d %zu %zu\n", all256 ? 1 : 0, base, texi_alpha_pool_end(at));
    for (const Line& l : lines) printf("%zu %u %zu %u %lu %lu %lu\n", l.base, l.levels, l.plane, l.fmt, l.crcLevels, l.crcPlane, l.crcOffsets);
    return 0;
}

// The product's "inert when terminal" text (rtxpt_amd/csrc/pt_scene.h is host-and-device text: inert_bits_of, inert_word, inert_bits_at, inert_when_terminal) run on the
// HOST, for a build with -fsanitize=address,undefined (tests/test_inert_terminal.py). The table is built as k_inert_bits builds it — inert_word per word, into an allocation
// of exactly inert_words(n) words — and read back as k_classify reads it (inert_bits_at), so a word or a material one past the end is a sanitizer report.
//   inert_terminal_check <in> <out>
//   in : u32 nMaterials, u32 nPrims; nMaterials x 128 B PTMaterialData; nPrims x u32 material index of the primitive
//   out: per primitive 4 bytes: the two bits, then inert_when_terminal at nestedDielectricsQuality 0, 1, 2
//   stdout: "ok <words>"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pt_scene.h"

int main(int argc, char** argv) {
    using namespace ptk;
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb"); if (!f) return 3;
    uint hdr[2]; if (fread(hdr, 4, 2, f) != 2) return 4;
    const uint nMat = hdr[0], nPrim = hdr[1];
    PTMaterialData* mats = (PTMaterialData*)malloc(sizeof(PTMaterialData) * (size_t)nMat); uint* matOf = (uint*)malloc(4 * (size_t)nPrim);
    if ((nMat && fread(mats, sizeof(PTMaterialData), nMat, f) != nMat) || (nPrim && fread(matOf, 4, nPrim, f) != nPrim)) return 4;
    fclose(f);
    const uint words = inert_words(nPrim);
    uint* table = (uint*)malloc(4 * (size_t)words);
    for (uint w = 0; w < words; w++) table[w] = inert_word(w, nPrim, [&](uint p) -> const PTMaterialData& { return mats[matOf[p]]; });
    std::vector<unsigned char> out(4 * (size_t)nPrim);
    for (uint p = 0; p < nPrim; p++) {
        const uint b = inert_bits_at(table, p);
        out[4 * (size_t)p] = (unsigned char)b;
        for (uint q = 0; q < 3; q++) out[4 * (size_t)p + 1 + q] = inert_when_terminal(b, q) ? 1 : 0;
    }
    FILE* g = fopen(argv[2], "wb"); if (!g) return 5;
    if (nPrim && fwrite(out.data(), 1, out.size(), g) != out.size()) return 6;
    fclose(g);
    free(table); free(mats); free(matOf);
    printf("ok %u\n", words);
    return 0;
}

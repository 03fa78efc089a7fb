// CPU check of pt_scene.h's unorm8_to_float (tests/test_unorm8_exact.py): the opacity k / 255 of a byte of an alpha plane, formed without a division and without a
// table, must be the float the correctly rounded division gives — the quotient the texture upload and the oracle form — for every byte, bit for bit. The header's own
// text is compiled (for the host), not a copy; fmaf is the C library's (correctly rounded, single rounding).
#include <cmath>
#include <cstdio>
#include <cstring>
using std::fmaf;
#include "pt_scene.h"

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

int main() {
    int bad = 0, plainBad = 0;
    for (int k = 0; k < 256; k++) {
        const volatile float kf = (float)k;      // (volatile: the reference quotient is a run-time division, not a folded constant)
        const float want = kf / 255.0f, got = ptk::unorm8_to_float((unsigned char)k);
        if (bits(got) != bits(want)) { std::printf("k = %d: unorm8_to_float %.9g (%08x), k / 255 %.9g (%08x)\n", k, got, bits(got), want, bits(want)); bad++; }
        float r; const unsigned rb = 0x3B808081u; std::memcpy(&r, &rb, 4);
        const volatile float plain = kf * r;
        if (bits(plain) != bits(want)) plainBad++;
    }
    // the plain product with the rounded reciprocal is NOT the quotient (126 of 256 bytes differ): the correction step is what the function is for
    if (plainBad != 126) { std::printf("the plain product differs for %d bytes, expected 126\n", plainBad); bad++; }
    if (ptk::unorm8_to_float(0) != 0.0f || ptk::unorm8_to_float(255) != 1.0f) { std::printf("end points\n"); bad++; }
    if (bad) return 1;
    std::printf("ok bytes 256 plain_product_wrong %d\n", plainBad);
    return 0;
}

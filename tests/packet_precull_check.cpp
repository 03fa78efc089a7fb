// Host check of the packet's interval test (rtxpt_amd/csrc/pt_packet_precull.h) against a plain restatement of the per-ray slab test of the BVH8 traversers (t8_slab + T8_HIT,
// rtxpt_amd/csrc/pt_traverse8.h): whenever the interval test DROPS a child, no ray of the packet may enter it. Stand-alone: built with -fsanitize=address,undefined and
// -ffp-contract=off (the device's arithmetic: fma only where t8_slab says fma) and run as a program by tests/test_packet_precull_host.py.
// usage: packet_precull_check [cases] [seed]   — prints one line per family and a summary; exit status 1 on a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../rtxpt_amd/csrc/pt_packet_precull.h"

static const float kMaxRayTravel = 1e15f;      // pt_path.h
static const int MAX_RAYS = 64;

// pt_scene.h ray_safe_rcp
static inline float ray_safe_rcp(float d) {
    float a = fabsf(d);
    float s = (a < 7.888609e-31f) ? 7.888609e-31f : a;
    return 1.0f / ((d < 0.0f) ? -s : s);
}

struct Rng {
    uint64_t s;
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 32); }
    float unit() { return (next() >> 8) * (1.0f / 16777216.0f); }                  // [0, 1)
    float sym() { return unit() * 2.0f - 1.0f; }                                   // [-1, 1)
    uint32_t below(uint32_t n) { return next() % n; }
};

struct Ray { float o[3], i[3], bestT; };
struct Node { float n[3], s[3]; };
struct Child { uint8_t lo[3], hi[3]; };

// the planes a ray with reciprocal sign `neg` sees on an axis: t8_slab's v_perm selection (near = hi where the reciprocal is negative), cvt, fma
static inline void planes(const Node& nd, const Child& c, int a, bool neg, float& pN, float& pF) {
    const float lo = fmaf((float)c.lo[a], nd.s[a], nd.n[a]), hi = fmaf((float)c.hi[a], nd.s[a], nd.n[a]);
    pN = neg ? hi : lo; pF = neg ? lo : hi;
}
// t8_slab + T8_HIT for one ray, tmin = 0
static inline bool ray_enters(const Node& nd, const Child& c, const Ray& r) {
    float tN[3], tF[3];
    for (int a = 0; a < 3; a++) { float pN, pF; planes(nd, c, a, r.i[a] < 0.0f, pN, pF); tN[a] = (pN - r.o[a]) * r.i[a]; tF[a] = (pF - r.o[a]) * r.i[a]; }
    const float tn = fmaxf(fmaxf(tN[0], tN[1]), fmaxf(tN[2], 0.0f));
    const float tf = fminf(fminf(tF[0], tF[1]), fminf(tF[2], r.bestT));
    return tn <= tf * 1.0000012f;
}

enum Family { GENERAL = 0, WIDE_LENS, STRADDLE, CLAMP, ON_PLANE, INVERTED, ONE_RAY, FAMILIES };
static const char* const FAMILY_NAME[FAMILIES] = {"general", "wide origin box", "reciprocals straddle zero", "reciprocals at the clamp", "origins on a plane", "inverted (empty-slot) boxes", "one valid ray"};

struct Tally { uint64_t cases = 0, noTest = 0, kept = 0, keptEntered = 0, dropped = 0, violations = 0; };

int main(int argc, char** argv) {
    const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 12000000ull;
    Rng g{argc > 2 ? strtoull(argv[2], nullptr, 10) : 0x9E3779B97F4A7C15ull};
    if (!g.s) g.s = 1;
    Tally tally[FAMILIES];
    Ray rays[MAX_RAYS]; int R = 0; Node nd{}; int family = GENERAL; T8PacketInterval pi{}; bool tests = false; float maxBest = 0.f; bool negs[3] = {false, false, false};

    for (uint64_t n = 0; n < cases; n++) {
        if ((n & 7u) == 0u) {
            // ---- a node and a packet: eight children are tested against each
            family = (int)g.below(FAMILIES);
            const float scale = ldexpf(1.0f, (int)g.below(41) - 20);                 // 2^-20 .. 2^20
            for (int a = 0; a < 3; a++) { nd.s[a] = scale * (0.25f + g.unit()); nd.n[a] = g.sym() * (g.below(4) ? 100.0f * scale : 1.0e6f); }
            const float ext = 255.0f * scale;
            R = family == ONE_RAY ? 1 : (g.below(32) ? 1 + (int)g.below(8) : MAX_RAYS);
            // the packet's central origin: around the node, up to a few extents away, or far (|o| up to 1e6)
            float oc[3], dc[3];
            for (int a = 0; a < 3; a++) oc[a] = g.below(8) ? nd.n[a] + ext * (0.5f + 3.0f * g.sym()) : 1.0e6f * g.sym();
            // the central direction: towards a point of the node's box (so that children are entered), or anywhere
            float len = 0.f;
            for (int a = 0; a < 3; a++) { dc[a] = g.below(4) ? (nd.n[a] + ext * g.unit()) - oc[a] : g.sym(); len += dc[a] * dc[a]; }
            len = sqrtf(len); if (!(len > 0.f) || !std::isfinite(len)) { dc[0] = 1.f; dc[1] = dc[2] = 0.f; len = 1.f; }
            for (int a = 0; a < 3; a++) dc[a] /= len;
            const float spread = ldexpf(1.0f, -(int)g.below(16));                   // the cone: 1 .. 2^-15
            const float lens = family == WIDE_LENS ? ext * g.unit() * 2.0f : (g.below(2) ? 0.f : ext * 1.0e-3f * g.unit());
            const int special = 1 + (int)g.below(3);                                // axes the STRADDLE / CLAMP / ON_PLANE families act on
            const float bestScale = g.below(3) ? ext * 4.0f * g.unit() : kMaxRayTravel;
            for (int r = 0; r < R; r++) {
                Ray& q = rays[r];
                for (int a = 0; a < 3; a++) {
                    float d = dc[a] + spread * g.sym();
                    if (family == STRADDLE && a < special) d = (g.below(3) ? spread * 1.0e-3f : 1.0e-33f) * g.sym() * (g.below(4) ? 1.0f : 0.0f);      // both signs, zeros, values under the clamp
                    if (family == CLAMP && a < special) d = dc[a] < 0.f ? -(1.0e-38f + 7.888609e-31f * g.unit() * 2.0f) : (g.below(2) ? 0.0f : 7.888609e-31f * g.unit() * 2.0f);      // one sign (a zero counts as positive), |d| around or under the clamp
                    q.i[a] = ray_safe_rcp(d);
                    q.o[a] = oc[a] + lens * g.sym();
                    if (family == ON_PLANE && a < special) q.o[a] = fmaf((float)g.below(256), nd.s[a], nd.n[a]);      // exactly a quantised plane's position
                }
                const uint32_t k = g.below(8);
                q.bestT = k == 0 ? kMaxRayTravel : (k == 1 ? 0.0f : bestScale * g.unit());
            }
            float oMin[3], oMax[3], iLo[3], iHi[3];
            for (int a = 0; a < 3; a++) { oMin[a] = oMax[a] = rays[0].o[a]; iLo[a] = iHi[a] = rays[0].i[a]; }
            maxBest = rays[0].bestT;
            for (int r = 1; r < R; r++) { for (int a = 0; a < 3; a++) { oMin[a] = fminf(oMin[a], rays[r].o[a]); oMax[a] = fmaxf(oMax[a], rays[r].o[a]); iLo[a] = fminf(iLo[a], rays[r].i[a]); iHi[a] = fmaxf(iHi[a], rays[r].i[a]); }
                                          maxBest = fmaxf(maxBest, rays[r].bestT); }
            tests = t8_packet_interval(oMin[0], oMin[1], oMin[2], oMax[0], oMax[1], oMax[2], iLo[0], iLo[1], iLo[2], iHi[0], iHi[1], iHi[2], pi);
            for (int a = 0; a < 3; a++) negs[a] = rays[0].i[a] < 0.0f;              // (with definite signs: every ray's selectors)
        }
        // ---- a child: a random quantised box, sometimes thin or flat, sometimes inverted
        Child c;
        for (int a = 0; a < 3; a++) {
            uint32_t p = g.below(256), q = g.below(4) ? g.below(256) : p + g.below(3);
            if (q > 255u) q = 255u;
            c.lo[a] = (uint8_t)(p < q ? p : q); c.hi[a] = (uint8_t)(p < q ? q : p);
        }
        if (family == INVERTED) { for (int a = 0; a < 3; a++) { if (g.below(4) == 0u) continue; c.lo[a] = 255; c.hi[a] = 0; } if (g.below(2)) { c.lo[0] = c.lo[1] = c.lo[2] = 255; c.hi[0] = c.hi[1] = c.hi[2] = 0; } }

        Tally& t = tally[family]; t.cases++;
        bool entered = false;
        for (int r = 0; r < R && !entered; r++) entered = ray_enters(nd, c, rays[r]);
        if (!tests) { t.noTest++; continue; }
        float pN[3], pF[3];
        for (int a = 0; a < 3; a++) planes(nd, c, a, negs[a], pN[a], pF[a]);
        const bool keeps = t8_packet_keeps(pN[0], pF[0], pN[1], pF[1], pN[2], pF[2], pi, 0.0f, maxBest);
        if (keeps) { t.kept++; if (entered) t.keptEntered++; }
        else { t.dropped++; if (entered) { if (t.violations++ < 5) printf("VIOLATION family %s case %llu\n", FAMILY_NAME[family], (unsigned long long)n); } }
    }

    Tally all;
    for (int f = 0; f < FAMILIES; f++) {
        const Tally& t = tally[f];
        printf("%-30s cases %10llu  no test %9llu  kept %9llu (entered by a ray %9llu)  dropped %9llu  violations %llu\n", FAMILY_NAME[f], (unsigned long long)t.cases, (unsigned long long)t.noTest,
               (unsigned long long)t.kept, (unsigned long long)t.keptEntered, (unsigned long long)t.dropped, (unsigned long long)t.violations);
        all.cases += t.cases; all.noTest += t.noTest; all.kept += t.kept; all.keptEntered += t.keptEntered; all.dropped += t.dropped; all.violations += t.violations;
    }
    const uint64_t tested = all.kept + all.dropped;
    printf("cases %llu tested %llu dropped %llu violations %llu share_kept %.4f share_kept_that_a_ray_enters %.4f\n", (unsigned long long)all.cases, (unsigned long long)tested, (unsigned long long)all.dropped,
           (unsigned long long)all.violations, tested ? (double)all.kept / (double)tested : 1.0, all.kept ? (double)all.keptEntered / (double)all.kept : 0.0);
    return all.violations ? 1 : 0;
}

// Host check of the traversal launch plan (rtxpt_amd/csrc/pt_trace_plan.h: what launch_extend, launch_shadow and launch_trace_pair size their launches with), stand-alone:
// the header is plain C++, so this is the arithmetic the launchers run. Over every combination of the extend counts, shadow counts and grid bounds below it holds
//   - the fused launch's split: each half has a block, the two fit the bound, neither exceeds the grid a launch of its own would get, two grids that fit the bound together
//     are left as they are, and a split uses the whole bound;
//   - rays_per_chunk: a multiple of T8_GROUPS_PER_WAVE within [T8_GROUPS_PER_WAVE, T8_CHUNK] (T8_CHUNK where a wave's groups exceed it);
//   - the task rounds: two at or below 32768 rays, four above; for the pair two only when both counts are at or below 32768;
//   - every grid: at least one block, at most its bound, and enough blocks for the count where the bound allows.
// Built by tests/test_trace_plan.py, once plainly and once with -fsanitize=address,undefined. Prints "ok combos N"; exit status 1 with one line per violation.
#include <cstdio>
#include "../rtxpt_amd/csrc/pt_trace_plan.h"

using namespace ptk;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main() {
    const uint counts[] = {0u, 1u, 2u, 31u, 32u, 33u, 64u, 127u, 128u, 129u, 1000u, 4096u, 32768u, 32769u, 100000u, 1000000u, 8294400u, 33177600u, 40000000u};
    const uint bounds[] = {2u, 3u, 4u, 7u, 64u, 1000u, T8_MAX_BLOCKS, 0u};      // (0: unset)
    const uint nCounts = sizeof(counts) / sizeof(counts[0]), nBounds = sizeof(bounds) / sizeof(bounds[0]);
    auto check_rpc = [&](uint count) {
        const uint rpc = rays_per_chunk(count);
        if (T8_GROUPS_PER_WAVE > T8_CHUNK) { CHECK(rpc == T8_CHUNK, "count %u rpc %u", count, rpc); return; }
        CHECK(rpc % T8_GROUPS_PER_WAVE == 0u && rpc >= T8_GROUPS_PER_WAVE && rpc <= T8_CHUNK, "count %u rpc %u", count, rpc);
    };
    auto check_grid = [&](uint g, uint count, uint perBlock, uint bound) {
        CHECK(g >= 1u && g <= bound, "grid %u count %u bound %u", g, count, bound);
        CHECK(g == bound || (unsigned long long)g * perBlock >= count, "grid %u x %u below count %u (bound %u)", g, perBlock, count, bound);
    };
    unsigned combos = 0;
    for (uint ie = 0; ie < nCounts; ie++) for (uint is = 0; is < nCounts; is++) for (uint ib = 0; ib < nBounds; ib++) {
        const uint e = counts[ie], s = counts[is], mb = bounds[ib];
        const uint bound = t8_grid_bound(mb);
        CHECK(bound == ((mb == 0u || mb > T8_MAX_BLOCKS) ? T8_MAX_BLOCKS : mb), "maxBlocks %u bound %u", mb, bound);
        check_rpc(e); check_rpc(s); check_rpc(e + s);
        // a launch of one kind, and its task rounds
        const uint perBlockE = (T8_BLOCK / 64u) * rays_per_chunk(e) * T8_CHUNKS_PER_WAVE_MIN, perBlockS = (T8_BLOCK / 64u) * rays_per_chunk(s) * T8_CHUNKS_PER_WAVE_MIN;
        const uint aloneE = t8_ray_grid(e, rays_per_chunk(e), bound), aloneS = t8_ray_grid(s, rays_per_chunk(s), bound);
        check_grid(aloneE, e, perBlockE, bound); check_grid(aloneS, s, perBlockS, bound);
        check_grid(t8_packet_grid(e, false, mb), e, (T8_BLOCK / 64u) * T8_PACKET_RAYS, bound); check_grid(t8_packet_grid(e, true, mb), e, (T8_BLOCK / 64u) * T8_PACKET64_RAYS, bound);
        const uint sweep = shadow_resolve_grid(s);
        CHECK(sweep >= T8_RESOLVE_BLOCKS && sweep <= T8_SWEEP_BLOCKS && (sweep == T8_SWEEP_BLOCKS || (unsigned long long)sweep * 256u >= s), "count %u sweep %u", s, sweep);
        CHECK(t8_task_rounds(e) == (e <= 32768u ? 2u : 4u), "count %u rounds %u", e, t8_task_rounds(e));
        CHECK(t8_task_rounds_pair(e, s) == ((e <= 32768u && s <= 32768u) ? 2u : 4u), "counts %u %u rounds %u", e, s, t8_task_rounds_pair(e, s));
        // the fused launch
        const uint rpc = rays_per_chunk(e + s);
        const uint ownE = t8_ray_grid(e, rpc, bound), ownS = t8_ray_grid(s, rpc, bound);
        const T8PairGrid g = t8_pair_grid(e, s, rpc, bound);
        CHECK(g.gE >= 1u && g.gS >= 1u, "e %u s %u bound %u: gE %u gS %u", e, s, bound, g.gE, g.gS);
        CHECK(g.gE + g.gS <= bound, "e %u s %u bound %u: gE %u gS %u", e, s, bound, g.gE, g.gS);
        CHECK(g.gE <= ownE && g.gS <= ownS, "e %u s %u bound %u: gE %u of %u, gS %u of %u", e, s, bound, g.gE, ownE, g.gS, ownS);
        CHECK(g.gE <= aloneE && g.gS <= aloneS, "e %u s %u bound %u: gE %u of %u alone, gS %u of %u alone", e, s, bound, g.gE, aloneE, g.gS, aloneS);      // (a launch alone has chunks no longer than the pair's)
        if (ownE + ownS <= bound) CHECK(g.gE == ownE && g.gS == ownS, "e %u s %u bound %u: gE %u gS %u changed from %u %u", e, s, bound, g.gE, g.gS, ownE, ownS);
        else CHECK(g.gE + g.gS == bound, "e %u s %u bound %u: gE %u gS %u leave blocks unused", e, s, bound, g.gE, g.gS);
        combos++;
    }
    if (failures) { printf("violations %d over combos %u\n", failures, combos); return 1; }
    printf("ok combos %u\n", combos);
    return 0;
}

// The host form of the shard exchange (rtxpt_amd/csrc/pt_shard_host.cpp) with ranks as threads over a RENDEZVOUS transport: a send returns only when the matching
// receive has taken the bytes, so "pairs meet in rank order, the lower rank sends first: blocking transports cannot deadlock" is held to its word (a buffering transport
// proves nothing about it). A watchdog ends a stuck run after a fixed wall time. Usage: shard_exchange_check <width> <height> <world>; prints "ok ..." and exits 0, or
// says what is wrong and exits 1 (2: stuck).
#include "../include/mi355pt.h"
#include "../rtxpt_amd/csrc/pt_shard.h"
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <utility>
#include <vector>

namespace {

const int kWatchdogSeconds = 20;
uint32_t W, H, WORLD;
std::mutex g_mx; std::condition_variable g_cv;
int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::lock_guard<std::mutex> lk_(g_mx); g_failures++; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// one slot per (sender, receiver): the sender posts its buffer and waits until the receiver has copied it
struct Slot { const void* buf = nullptr; size_t bytes = 0; bool posted = false, taken = false; };
std::vector<Slot> g_slots;
struct Rank {
    uint32_t rank = 0; std::vector<std::pair<uint32_t, size_t>> sent; int begins = 0, ends = 0, callsInsideGroup = 0, callsOutsideGroup = 0; bool inGroup = false;
    void count() { if (inGroup) callsInsideGroup++; else callsOutsideGroup++; }
};
int32_t t_send(void* user, const void* buf, size_t bytes, uint32_t peer) {
    Rank* me = (Rank*)user; me->sent.push_back({peer, bytes}); me->count();
    std::unique_lock<std::mutex> lk(g_mx);
    Slot& s = g_slots[me->rank * WORLD + peer];
    g_cv.wait(lk, [&] { return !s.posted; });
    s.buf = buf; s.bytes = bytes; s.posted = true; s.taken = false; g_cv.notify_all();
    g_cv.wait(lk, [&] { return s.taken; });
    s.posted = false; g_cv.notify_all();
    return 0;
}
int32_t t_recv(void* user, void* buf, size_t bytes, uint32_t peer) {
    Rank* me = (Rank*)user; me->count();
    std::unique_lock<std::mutex> lk(g_mx);
    Slot& s = g_slots[peer * WORLD + me->rank];
    g_cv.wait(lk, [&] { return s.posted && !s.taken; });
    const bool sameSize = s.bytes == bytes;
    if (sameSize) memcpy(buf, s.buf, bytes);
    s.taken = true; g_cv.notify_all();
    return sameSize ? 0 : 1;      // a transfer is un-padded: both sides name the same size
}
int32_t t_begin(void* user) { Rank* me = (Rank*)user; me->begins++; me->inGroup = true; return 0; }
int32_t t_end(void* user) { Rank* me = (Rank*)user; me->ends++; me->inGroup = false; return 0; }

unsigned char value(uint32_t plane, size_t pixel, uint32_t byte) { uint32_t h = (uint32_t)pixel * 2654435761u + plane * 40503u + byte * 97u; return (unsigned char)(h >> 13); }

std::vector<std::vector<uint32_t>> layout() {
    std::vector<std::vector<uint32_t>> lists(WORLD);
    for (uint32_t r = 0; r < WORLD; r++) {
        uint32_t n = 0; if (pt_shard_layout(W, H, r, WORLD, nullptr, 0, &n) != PT_OK) { fprintf(stderr, "pt_shard_layout failed\n"); exit(1); }
        lists[r].resize(n); if (pt_shard_layout(W, H, r, WORLD, lists[r].data(), n, nullptr) != PT_OK) { fprintf(stderr, "pt_shard_layout failed\n"); exit(1); }
    }
    return lists;
}

// the schedule: the offsets are the prefix sums over the other ranks in rank order, and every (sender, receiver) pair of the route appears once on each side, with equal counts
void check_schedule(const std::vector<std::vector<uint32_t>>& lists, ShardRoute route) {
    std::vector<size_t> counts; for (auto& l : lists) counts.push_back(l.size());
    std::map<std::pair<uint32_t, uint32_t>, std::vector<size_t>> sends, recvs;      // (sender, receiver) -> the counts named
    for (uint32_t r = 0; r < WORLD; r++) {
        uint32_t last = 0; bool first = true;
        for (const ShardStep& s : shard_schedule(counts, r, route)) {
            CHECK(s.peer < WORLD && s.peer != r, "route %d rank %u: peer %u", (int)route, r, s.peer);
            CHECK(first || s.peer > last, "route %d rank %u: peers not in rank order", (int)route, r); first = false; last = s.peer;
            size_t prefix = 0; for (uint32_t q = 0; q < s.peer; q++) if (q != r) prefix += counts[q];
            CHECK(s.offset == prefix, "route %d rank %u peer %u: offset %zu, prefix sum %zu", (int)route, r, s.peer, s.offset, prefix);
            const bool iSend = route == SHARD_ALL_TO_ALL || s.peer == 0u, iRecv = route == SHARD_ALL_TO_ALL || r == 0u;
            CHECK(iSend || iRecv, "route %d rank %u: a step with peer %u", (int)route, r, s.peer);
            CHECK(s.send == (iSend ? counts[r] : 0) && s.recv == (iRecv ? counts[s.peer] : 0), "route %d rank %u peer %u: send %zu recv %zu", (int)route, r, s.peer, s.send, s.recv);
            if (iSend) sends[std::make_pair(r, s.peer)].push_back(s.send);
            if (iRecv) recvs[std::make_pair(s.peer, r)].push_back(s.recv);
        }
    }
    size_t pairs = 0;
    for (uint32_t a = 0; a < WORLD; a++) for (uint32_t b = 0; b < WORLD; b++) {
        const std::pair<uint32_t, uint32_t> ab(a, b);
        if (a == b || (route == SHARD_TO_ROOT && b != 0u)) { CHECK(!sends.count(ab) && !recvs.count(ab), "route %d: pair %u -> %u", (int)route, a, b); continue; }
        pairs++;
        const std::vector<size_t> s = sends[ab], r = recvs[ab];
        CHECK(s.size() == 1 && r.size() == 1, "route %d: pair %u -> %u appears %zu / %zu times", (int)route, a, b, s.size(), r.size());
        if (s.size() == 1 && r.size() == 1) CHECK(s[0] == r[0] && s[0] == counts[a], "route %d: pair %u -> %u counts", (int)route, a, b);
    }
    CHECK(sends.size() == pairs && recvs.size() == pairs, "route %d: %zu / %zu pairs, expected %zu", (int)route, sends.size(), recvs.size(), pairs);
}

void run_exchange(const std::vector<std::vector<uint32_t>>& lists, const std::vector<uint32_t>& bpp, ShardRoute route) {
    const size_t N = (size_t)W * H; size_t rec = 0; for (uint32_t b : bpp) rec += b;
    std::vector<std::vector<unsigned char>> full(bpp.size());
    for (uint32_t k = 0; k < bpp.size(); k++) { full[k].resize(N * bpp[k]); for (size_t p = 0; p < N; p++) for (uint32_t j = 0; j < bpp[k]; j++) full[k][p * bpp[k] + j] = value(k, p, j); }
    // every rank: its own pixels valid, poison elsewhere
    auto own = [&](uint32_t r) {
        std::vector<std::vector<unsigned char>> mine(bpp.size());
        for (uint32_t k = 0; k < bpp.size(); k++) {
            mine[k].assign(N * bpp[k], 0xEE);
            for (uint32_t px : lists[r]) { const size_t slot = (size_t)(px & 0xFFFFu) * W + (px >> 16); memcpy(&mine[k][slot * bpp[k]], &full[k][slot * bpp[k]], bpp[k]); }
        }
        return mine;
    };
    std::vector<std::vector<std::vector<unsigned char>>> planes(WORLD); std::vector<Rank> ranks(WORLD); std::vector<int32_t> result(WORLD, -99);
    for (uint32_t r = 0; r < WORLD; r++) { planes[r] = own(r); ranks[r].rank = r; }
    g_slots.assign((size_t)WORLD * WORLD, Slot());
    uint32_t finished = 0;
    std::vector<std::thread> threads;
    for (uint32_t r = 0; r < WORLD; r++) threads.emplace_back([&, r] {
        std::vector<void*> ptrs; for (auto& p : planes[r]) ptrs.push_back(p.data());
        PtTransport t = {&ranks[r], t_send, t_recv, t_begin, t_end};
        result[r] = pt_exchange_planes_host(W, H, r, WORLD, ptrs.data(), bpp.data(), (uint32_t)bpp.size(), route == SHARD_TO_ROOT ? 1 : 0, &t);
        std::lock_guard<std::mutex> lk(g_mx); finished++; g_cv.notify_all();
    });
    {   // the watchdog: a deadlock is a failure, not a hang
        std::unique_lock<std::mutex> lk(g_mx);
        if (!g_cv.wait_until(lk, std::chrono::system_clock::now() + std::chrono::seconds(kWatchdogSeconds), [&] { return finished == WORLD; })) {
            fprintf(stderr, "FAILED: stuck after %d s (route %d, %zu planes, %u of %u ranks finished)\n", kWatchdogSeconds, (int)route, bpp.size(), finished, WORLD); fflush(stderr); _exit(2);
        }
    }
    for (auto& t : threads) t.join();
    for (uint32_t r = 0; r < WORLD; r++) {
        CHECK(result[r] == PT_OK, "route %d rank %u: returned %d", (int)route, r, result[r]);
        // the planes: all-to-all leaves every rank with the full planes; to rank 0 leaves rank 0 with them and a sender with what it had
        const bool whole = route == SHARD_ALL_TO_ALL || r == 0u;
        const std::vector<std::vector<unsigned char>> want = whole ? full : own(r);
        for (uint32_t k = 0; k < bpp.size(); k++) CHECK(planes[r][k] == want[k], "route %d rank %u plane %u (%u bytes per pixel): wrong bytes", (int)route, r, k, bpp[k]);
        // the sends: exactly the rank's own bytes, once per receiver, in rank order
        std::vector<std::pair<uint32_t, size_t>> expect;
        if (WORLD > 1 && !lists[r].empty()) for (uint32_t p = 0; p < WORLD; p++) if (p != r && (route == SHARD_ALL_TO_ALL || p == 0u)) expect.push_back({p, rec * lists[r].size()});
        CHECK(ranks[r].sent == expect, "route %d rank %u: %zu sends, expected %zu", (int)route, r, ranks[r].sent.size(), expect.size());
        // the group calls: rank 0 of a gather brackets its receives with one pair; nobody else makes any
        const int pairs = (route == SHARD_TO_ROOT && r == 0u && WORLD > 1) ? 1 : 0;
        CHECK(ranks[r].begins == pairs && ranks[r].ends == pairs, "route %d rank %u: %d group_begin / %d group_end, expected %d", (int)route, r, ranks[r].begins, ranks[r].ends, pairs);
        CHECK(!ranks[r].inGroup && (pairs ? ranks[r].callsOutsideGroup : ranks[r].callsInsideGroup) == 0, "route %d rank %u: transfers on the wrong side of the group", (int)route, r);
    }
}

} // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s width height world\n", argv[0]); return 1; }
    W = (uint32_t)atoi(argv[1]); H = (uint32_t)atoi(argv[2]); WORLD = (uint32_t)atoi(argv[3]);
    const std::vector<std::vector<uint32_t>> lists = layout();
    size_t total = 0, empty = 0; for (auto& l : lists) { total += l.size(); empty += l.empty(); }
    CHECK(total == (size_t)W * H, "the shards hold %zu pixels of %zu", total, (size_t)W * H);
    const std::vector<std::vector<uint32_t>> planeSets = {{4}, {8}, {16}, {4, 8, 16}};
    for (ShardRoute route : {SHARD_ALL_TO_ALL, SHARD_TO_ROOT}) {
        check_schedule(lists, route);
        for (const std::vector<uint32_t>& bpp : planeSets) run_exchange(lists, bpp, route);
    }
    if (g_failures) { fprintf(stderr, "%d checks failed\n", g_failures); return 1; }
    printf("ok %ux%u world %u, %zu ranks own nothing\n", W, H, WORLD, empty);
    return 0;
}

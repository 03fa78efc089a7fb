// mi355pt — tile shards on the host (pt_shard.h): the shard layout, the schedule of an exchange, and the exchange itself over HOST memory and the caller's point-to-point
// transport (include/mi355pt.h PtTransport): pt_gather_host, pt_neeat_exchange_host and pt_exchange_planes_host are one core. No HIP: this file compiles with a plain C++ compiler.
#include "../../include/mi355pt.h"
#include "pt_shard.h"
#include <algorithm>
#include <cstring>
#include <utility>

uint32_t morton2(uint32_t x, uint32_t y) {
    auto part = [](uint32_t v) { v &= 0xFFFF; v = (v | (v << 8)) & 0x00FF00FF; v = (v | (v << 4)) & 0x0F0F0F0F; v = (v | (v << 2)) & 0x33333333; v = (v | (v << 1)) & 0x55555555; return v; };
    return part(x) | (part(y) << 1);
}
void shard_pixel_lists(uint32_t width, uint32_t height, uint32_t world, std::vector<std::vector<uint32_t>>& out) {
    out.assign(world, std::vector<uint32_t>());
    uint32_t tx = (width + TILE - 1) / TILE, ty = (height + TILE - 1) / TILE;
    std::vector<std::pair<uint32_t, uint32_t>> tiles;
    for (uint32_t y = 0; y < ty; y++) for (uint32_t x = 0; x < tx; x++) tiles.push_back({morton2(x, y), y * tx + x});
    std::sort(tiles.begin(), tiles.end());
    uint32_t order = 0;
    for (auto& t : tiles) {
        uint32_t tX = t.second % tx, tY = t.second / tx;
        std::vector<uint32_t>& dst = out[(order / PT_SHARD_TILE_GROUP) % world];
        order++;
        for (uint32_t by = 0; by < TILE; by += 8) for (uint32_t bx = 0; bx < TILE; bx += 8)
            for (uint32_t y = 0; y < 8; y++) for (uint32_t x = 0; x < 8; x++) {
                uint32_t px = tX * TILE + bx + x, py = tY * TILE + by + y;
                if (px < width && py < height) dst.push_back((px << 16) | py);
            }
    }
}

std::vector<ShardStep> shard_schedule(const std::vector<size_t>& counts, uint32_t rank, ShardRoute route) {
    std::vector<ShardStep> steps;
    size_t offset = 0;
    for (uint32_t p = 0; p < (uint32_t)counts.size(); p++) {
        if (p == rank) continue;
        const bool iSend = route == SHARD_ALL_TO_ALL || p == 0u, iRecv = route == SHARD_ALL_TO_ALL || rank == 0u;
        if (iSend || iRecv) steps.push_back({p, iSend ? counts[rank] : 0, iRecv ? counts[p] : 0, offset});
        offset += counts[p];
    }
    return steps;
}

namespace {

// The exchange over numPlanes row-major width x height planes of bytesPerPixel[k] bytes per pixel. A record = the planes' bytes of one pixel back to back, in the owner's pixel
// order; transfers are un-padded, a rank sends exactly its own bytes. The pairs of a rank meet in rank order and the lower rank of a pair sends first, so blocking transports
// cannot deadlock. Rank 0 of a gather only receives: it brackets its receives with the transport's group calls (a transport may queue until group_end) and unpacks after them.
// The arguments are the exports' to check.
int32_t exchange_host(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, void* const* planes, const uint32_t* bytesPerPixel, uint32_t numPlanes, ShardRoute route, const PtTransport* t) {
    if (world == 1) return PT_OK;
    try {
        std::vector<std::vector<uint32_t>> lists; shard_pixel_lists(width, height, world, lists);
        std::vector<size_t> counts(world); size_t rec = 0, recvEnd = 0;
        for (uint32_t r = 0; r < world; r++) counts[r] = lists[r].size();
        for (uint32_t k = 0; k < numPlanes; k++) rec += bytesPerPixel[k];
        const std::vector<ShardStep> steps = shard_schedule(counts, rank, route);
        for (const ShardStep& s : steps) if (s.recv) recvEnd = s.offset + s.recv;      // (a rank that only sends stages nothing)
        // one pixel's record <-> its place in the planes
        auto copy = [&](uint32_t px, unsigned char* buf, bool unpack) {
            const size_t slot = (size_t)(px & 0xFFFFu) * width + (px >> 16);
            for (uint32_t k = 0; k < numPlanes; k++) {
                unsigned char* at = (unsigned char*)planes[k] + slot * bytesPerPixel[k];
                if (unpack) memcpy(at, buf, bytesPerPixel[k]); else memcpy(buf, at, bytesPerPixel[k]);
                buf += bytesPerPixel[k];
            }
        };
        const std::vector<uint32_t>& mine = lists[rank];
        std::vector<unsigned char> sendbuf(rec * mine.size()), recvbuf(rec * recvEnd);
        for (size_t i = 0; i < mine.size(); i++) copy(mine[i], &sendbuf[rec * i], false);
        const bool grouped = route == SHARD_TO_ROOT && rank == 0u;
        if (grouped && t->group_begin && t->group_begin(t->user) != 0) return PT_ERROR_IO;
        for (const ShardStep& s : steps)
            for (int half = 0; half < 2; half++) {
                const bool sendNow = (rank < s.peer) == (half == 0);
                if (sendNow) { if (s.send && t->send(t->user, sendbuf.data(), sendbuf.size(), s.peer) != 0) return PT_ERROR_IO; }
                else if (s.recv && t->recv(t->user, &recvbuf[rec * s.offset], rec * s.recv, s.peer) != 0) return PT_ERROR_IO;
            }
        if (grouped && t->group_end && t->group_end(t->user) != 0) return PT_ERROR_IO;
        for (const ShardStep& s : steps) for (size_t i = 0; i < s.recv; i++) copy(lists[s.peer][i], &recvbuf[rec * (s.offset + i)], true);
        return PT_OK;
    } catch (...) { return PT_ERROR_IO; }
}

} // namespace

extern "C" {

// ---- the frame gather (include/mi355pt.h "the frame gather itself")
int32_t pt_shard_layout(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, uint32_t* pixels, uint32_t capacity, uint32_t* count) {
    if (!width || !height || width > 65535 || height > 65535 || !world || rank >= world) return PT_ERROR_INVALID_ARGUMENT;
    std::vector<std::vector<uint32_t>> lists; shard_pixel_lists(width, height, world, lists);
    const std::vector<uint32_t>& mine = lists[rank];
    if (count) *count = (uint32_t)mine.size();
    if (pixels) { if (capacity < mine.size()) return PT_ERROR_INVALID_ARGUMENT; if (!mine.empty()) memcpy(pixels, mine.data(), 4 * mine.size()); }
    return PT_OK;
}
// pt_gather's protocol over host memory: one 16-byte plane, to rank 0
int32_t pt_gather_host(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, float* rgba, const PtTransport* t) {
    if (!rgba || !t || !t->send || !t->recv || !width || !height || width > 65535 || height > 65535 || !world || rank >= world) return PT_ERROR_INVALID_ARGUMENT;
    void* const planes[1] = {rgba}; const uint32_t bytes[1] = {16};
    return exchange_host(width, height, rank, world, planes, bytes, 1, SHARD_TO_ROOT, t);
}
// The NEE-AT feedback exchange of tile-sharded frames (neeat_exchange_feedback, pt_shard.hip) over host memory: every rank sends the reservoirs and the exported depth of its
// own pixels (12 bytes each: three 4-byte planes) to every other rank and receives theirs
int32_t pt_neeat_exchange_host(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, float* totalWeight, uint32_t* candidates, float* depth, const PtTransport* t) {
    if (!totalWeight || !candidates || !depth || !t || !t->send || !t->recv || !width || !height || width > 65535 || height > 65535 || !world || rank >= world) return PT_ERROR_INVALID_ARGUMENT;
    void* const planes[3] = {totalWeight, candidates, depth}; const uint32_t bytes[3] = {4, 4, 4};
    return exchange_host(width, height, rank, world, planes, bytes, 3, SHARD_ALL_TO_ALL, t);
}
// The general form: any planes (depth: 4 bytes per pixel, motion vectors: 8, a header plane: 4 ...). toRoot = 0: all-to-all (the guide exchange of a tile-sharded realtime
// frame); toRoot = 1: to rank 0 only (the plane-buffer gather)
int32_t pt_exchange_planes_host(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, void* const* planes, const uint32_t* bytesPerPixel, uint32_t numPlanes, int32_t toRoot, const PtTransport* t) {
    if (!planes || !bytesPerPixel || !numPlanes || !t || !t->send || !t->recv || !width || !height || width > 65535 || height > 65535 || !world || rank >= world) return PT_ERROR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < numPlanes; k++) if (!planes[k] || !bytesPerPixel[k]) return PT_ERROR_INVALID_ARGUMENT;
    return exchange_host(width, height, rank, world, planes, bytesPerPixel, numPlanes, toRoot ? SHARD_TO_ROOT : SHARD_ALL_TO_ALL, t);
}

} // extern "C"

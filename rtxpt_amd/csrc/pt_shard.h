// mi355pt — tile shards, the host-only part (no HIP header: pt_shard_host.cpp compiles with a plain C++ compiler, tests/shard_exchange_check.cpp links it): which rank owns
// which pixel, and who sends what to whom when the ranks exchange a per-pixel record. The device form of the exchange (RCCL, pt_shard.hip) and the host form (PtTransport,
// pt_shard_host.cpp) both walk the one schedule below. Private: nothing here is exported.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)

static const uint32_t TILE = 32;
#ifndef PT_SHARD_TILE_GROUP
#define PT_SHARD_TILE_GROUP 1      // consecutive Morton-ordered 32x32 tiles dealt to the same rank (locality vs load balance)
#endif

uint32_t morton2(uint32_t x, uint32_t y);
// pixel ownership: 32x32 tiles, tile t -> rank morton(t) % world; inside a tile pixels are listed in 8x8 blocks so that the 64 lanes of a wave start as an 8x8 screen
// block (coherent primary rays). A pixel is x << 16 | y; out[r]: rank r's pixels in its pack order.
void shard_pixel_lists(uint32_t width, uint32_t height, uint32_t world, std::vector<std::vector<uint32_t>>& out);

// The routes of an exchange: every rank's own pixels to every other rank, or to rank 0 only (a gather).
enum ShardRoute { SHARD_ALL_TO_ALL = 0, SHARD_TO_ROOT = 1 };
// One peer of a rank's part in an exchange, counts in pixels: `send` of the rank's own pixels go to `peer` (always all of them or none), `recv` pixels — all of the peer's —
// come from it, into the receive buffer at pixel `offset`. The receive buffer is laid out as "every other rank's pixels in rank order" on every rank and for both routes, so
// `offset` is the prefix sum of the counts over the other ranks below `peer` whether or not anything arrives from them: one pixel list per rank serves both routes.
struct ShardStep { uint32_t peer; size_t send, recv, offset; };
// rank's steps, peers in rank order; a pair that exchanges nothing on this route has no step. counts[r]: the pixels rank r owns.
std::vector<ShardStep> shard_schedule(const std::vector<size_t>& counts, uint32_t rank, ShardRoute route);

#pragma GCC visibility pop

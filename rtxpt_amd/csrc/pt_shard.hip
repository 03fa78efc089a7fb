// mi355pt — tile shards on the device (include/mi355pt.h "the frame gather itself"; the layout and the schedule: pt_shard.h). A tile-sharded frame moves four kinds of
// per-pixel record between ranks — the radiance, the NEE-AT reservoirs with exported depth, the build pass's guides and the whole stable-plane record — and all four go the
// same way: the own pixels packed into flat records, RCCL point-to-point inside one group (un-padded, on the library's stream), the received records unpacked by the peers'
// pixel list; or, without a communicator, packed and unpacked by the host, which moves the buffers itself (the eight pack / unpack exports).
#include "pt_context.h"
#include <dlfcn.h>
#include <cstring>

using namespace ptk;

namespace ptk {

__global__ void __launch_bounds__(256) k_pack(const float4* __restrict__ accum, const uint* __restrict__ pixels, uint num, uint width, float4* __restrict__ dst) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= num) return;
    uint px = pixels[i]; dst[i] = accum[(px & 0xFFFFu) * width + (px >> 16)];
}
__global__ void __launch_bounds__(256) k_unpack(float4* __restrict__ accum, const uint* __restrict__ pixels, uint num, uint width, const float4* __restrict__ src) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= num) return;
    uint px = pixels[i]; accum[(px & 0xFFFFu) * width + (px >> 16)] = src[i];
}
// the NEE-AT feedback of a list of pixels as (weight bits, candidate, exported depth bits) triples, 12 bytes per pixel: what the ranks of a tile-sharded frame
// exchange between frames — the reservoirs AND the depth the baker's reprojection tests (neeat_reproject): a neighbourhood crosses shard borders, so every rank
// needs every pixel's depth
__global__ void __launch_bounds__(256) k_pack_feedback(const float* __restrict__ fbW, const uint* __restrict__ fbC, const float* __restrict__ depth, const uint* __restrict__ pixels, uint num, uint width, uint* __restrict__ dst) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= num) return;
    const uint px = pixels[i], slot = (px & 0xFFFFu) * width + (px >> 16);
    dst[3u * i] = __float_as_uint(fbW[slot]); dst[3u * i + 1u] = fbC[slot]; dst[3u * i + 2u] = depth ? __float_as_uint(depth[slot]) : 0u;
}
__global__ void __launch_bounds__(256) k_unpack_feedback(float* __restrict__ fbW, uint* __restrict__ fbC, float* __restrict__ depth, const uint* __restrict__ pixels, uint num, uint width, const uint* __restrict__ src) {
    uint i = blockIdx.x * 256u + threadIdx.x; if (i >= num) return;
    const uint px = pixels[i], slot = (px & 0xFFFFu) * width + (px >> 16);
    fbW[slot] = __uint_as_float(src[3u * i]); fbC[slot] = src[3u * i + 1u]; if (depth) depth[slot] = __uint_as_float(src[3u * i + 2u]);
}
void launch_pack_feedback(const float* fbW, const uint* fbC, const float* depth, const uint* pixels, uint num, uint width, uint* dst, hipStream_t st) {
    if (num) hipLaunchKernelGGL(k_pack_feedback, dim3((num + 255) / 256), dim3(256), 0, st, fbW, fbC, depth, pixels, num, width, dst);
}
void launch_unpack_feedback(float* fbW, uint* fbC, float* depth, const uint* pixels, uint num, uint width, const uint* src, hipStream_t st) {
    if (num) hipLaunchKernelGGL(k_unpack_feedback, dim3((num + 255) / 256), dim3(256), 0, st, fbW, fbC, depth, pixels, num, width, src);
}
void launch_pack(const float4* accum, const uint* pixels, uint num, uint width, float4* dst, hipStream_t st) {
    hipLaunchKernelGGL(k_pack, dim3((num + 255) / 256), dim3(256), 0, st, accum, pixels, num, width, dst);
}
void launch_unpack(float4* accum, const uint* pixels, uint num, uint width, const float4* src, hipStream_t st) {
    hipLaunchKernelGGL(k_unpack, dim3((num + 255) / 256), dim3(256), 0, st, accum, pixels, num, width, src);
}

} // namespace ptk

namespace {

// ---- RCCL, bound at run time. One process may already hold a librccl.so (PyTorch ships its own): RTLD_NOLOAD finds that copy first, so that a single
// RCCL runs on the single HIP runtime of the process; a plain C++ host gets the system library.
struct RcclApi {
    void* lib = nullptr; bool tried = false; std::string error;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load() {
        if (tried) return lib != nullptr;
        tried = true;
        const char* env = getenv("MI355PT_RCCL_LIB");
        if (env && *env) lib = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { const char* e = dlerror(); error = std::string("librccl.so not found: ") + (e ? e : ""); return false; }
#define PT_RCCL_SYM(field, name) field = reinterpret_cast<decltype(field)>(dlsym(lib, name)); if (!field) { error = std::string("librccl.so lacks ") + name; lib = nullptr; return false; }
        PT_RCCL_SYM(GetUniqueId, "ncclGetUniqueId") PT_RCCL_SYM(CommInitRank, "ncclCommInitRank") PT_RCCL_SYM(CommDestroy, "ncclCommDestroy") PT_RCCL_SYM(Send, "ncclSend")
        PT_RCCL_SYM(Recv, "ncclRecv") PT_RCCL_SYM(GroupStart, "ncclGroupStart") PT_RCCL_SYM(GroupEnd, "ncclGroupEnd") PT_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef PT_RCCL_SYM
        return true;
    }
};
RcclApi g_rccl;
#define PT_CHECK_NCCL(c, expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) return fail(c, PT_ERROR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); } while (0)

// ---- the four records. words: 4-byte words per pixel of the flat form; ready / notReady: whether the context holds the record, and what a caller that asks too early is
// told; destSmall / sourceSmall: the pack / unpack exports' refusals of a short buffer; rccl: what a failing transfer's text starts with.
enum ShardRecordKind { REC_RADIANCE, REC_FEEDBACK, REC_GUIDES, REC_PLANES };
struct ShardRecord { ShardRecordKind kind; uint words; bool (*ready)(const pt_context*); const char* notReady, * destSmall, * sourceSmall, * rccl; };
bool sp_there(const pt_context* c) { return c->spW && c->spW == c->width && c->spH == c->height; }
const ShardRecord RADIANCE = {REC_RADIANCE, 4u, [](const pt_context* c) { return c->width != 0u; }, "pt_resize first", "destination too small", "source too small", "pt_gather"};
const ShardRecord FEEDBACK = {REC_FEEDBACK, 3u, [](const pt_context* c) { return c->neeat.enabled && c->neeat.W && c->neeat.W == c->width && c->neeat.H == c->height; },
    "no NEE-AT frame yet: pt_set_neeat, then pt_render", "destination too small (12 bytes per owned pixel)", "source too small (12 bytes per pixel of that rank)", "NEE-AT feedback exchange"};
const ShardRecord GUIDES = {REC_GUIDES, SP_GUIDE_WORDS, sp_there, "no stable planes of this frame size yet: pt_build_stable_planes", "destination too small (16 bytes per owned pixel)",
    "source too small (16 bytes per pixel of that rank)", "stable-plane guide exchange"};
const ShardRecord PLANES = {REC_PLANES, SP_SHARD_WORDS, sp_there, "no stable planes of this frame size yet: pt_build_stable_planes", "destination too small (pt_stable_planes_shard_bytes)",
    "source too small (pt_stable_planes_shard_bytes)", "pt_gather_stable_planes"};
// (the two stable-plane unpack exports say why the build pass has to come first even on a rank that only receives)
std::string unpack_not_ready(const ShardRecord& R) { return std::string(R.notReady) + " (it allocates the buffers)"; }

// `num` pixels of a device pixel list between the context's buffers and flat records at `buf`, either way
void record_copy(pt_context* c, const ShardRecord& R, const uint* pixels, size_t num, uint* buf, bool unpack, hipStream_t st) {
    if (!num) return;
    pt_context::NeeAt& fb = c->neeat;
    switch (R.kind) {
    case REC_RADIANCE:
        if (unpack) launch_unpack(c->dAccum.p, pixels, (uint)num, c->width, (const ptk::float4*)buf, st); else launch_pack(c->dAccum.p, pixels, (uint)num, c->width, (ptk::float4*)buf, st);
        break;
    case REC_FEEDBACK:
        if (unpack) launch_unpack_feedback(fb.fbW.p, fb.fbC.p, fb.depth.p, pixels, (uint)num, c->width, buf, st); else launch_pack_feedback(fb.fbW.p, fb.fbC.p, fb.depth.p, pixels, (uint)num, c->width, buf, st);
        break;
    case REC_GUIDES: launch_sp_pack(sp_context(c, nullptr), pixels, (uint)num, buf, unpack, st, SP_GUIDE_FIRST, SP_GUIDE_WORDS); break;
    case REC_PLANES: launch_sp_pack(sp_context(c, nullptr), pixels, (uint)num, buf, unpack, st); break;
    }
}
// the context's buffers of a record overwritten (the loop-back of the two gathers): what is read afterwards has been through the transfer
hipError_t record_poison(pt_context* c, const ShardRecord& R, hipStream_t st) {
    const size_t N = (size_t)c->width * c->height;
    if (R.kind == REC_RADIANCE) return hipMemsetAsync(c->dAccum.p, 0xFF, sizeof(ptk::float4) * N, st);
    if (R.kind != REC_PLANES) return hipSuccess;
    struct { void* p; size_t bytes; } const all[] = {{c->dSpHeader.p, 16 * N}, {c->dSpPlanes.p, sizeof(ptk::StablePlane) * cStablePlaneCount * sp_context(c, nullptr).C.genericTSPlaneStride},
        {c->dSpRadiance.p, 8 * N}, {c->dSpDepth.p, 4 * N}, {c->dSpHitT.p, 4 * N}, {c->dSpMotion.p, 8 * N}, {c->dSpThroughput.p, 4 * N}};
    for (const auto& b : all) { hipError_t e = hipMemsetAsync(b.p, 0xEE, b.bytes, st); if (e != hipSuccess) return e; }
    return hipSuccess;
}

// One record of the owned pixels to the other ranks along `route`, on the library's stream and without waiting for it: staging, pack, one RCCL group with the schedule's
// sends and receives, unpack. A world of one (WITH a communicator: the two gathers) runs the whole protocol as a loop-back — pack, ncclSend to self + ncclRecv from self
// inside the group, unpack — so that the run-time-bound RCCL path can be exercised (and checked) on a one-GPU box; the context's buffers are poisoned between pack and unpack.
int shard_exchange(pt_context* c, const ShardRecord& R, ShardRoute route) {
    hipStream_t st = c->stream;
    ShardStaging& X = c->staging;
    const size_t W = R.words;
    const bool loopBack = c->shardCount == 1;
    std::vector<ShardStep> steps;
    if (loopBack) steps.push_back({0u, c->owned.size(), c->owned.size(), 0});
    else { std::vector<size_t> counts; for (const std::vector<uint>& px : c->shardPixels) counts.push_back(px.size()); steps = shard_schedule(counts, c->shardRank, route); }
    size_t sendPixels = 0, recvPixels = 0;
    for (const ShardStep& s : steps) { if (s.send) sendPixels = s.send; if (s.recv) recvPixels = s.offset + s.recv; }
    if (!sendPixels && !recvPixels) return PT_OK;
    PT_CHECK_HIP(c, X.send.resize(sendPixels * W)); PT_CHECK_HIP(c, X.recv.resize(recvPixels * W));
    // whose pixels the receive buffer holds, in its order: the loop-back's own; otherwise every other rank's in rank order — uploaded once per shard layout
    const uint* received = c->dOwned.p;
    if (!loopBack && recvPixels) {
        if (X.w != c->width || X.h != c->height) {
            std::vector<uint> others; for (uint r = 0; r < c->shardCount; r++) if (r != c->shardRank) others.insert(others.end(), c->shardPixels[r].begin(), c->shardPixels[r].end());
            PT_CHECK_HIP(c, X.pixels.upload(others, st)); PT_CHECK_HIP(c, hipStreamSynchronize(st));
            X.w = c->width; X.h = c->height;
        }
        received = X.pixels.p;
    }
    record_copy(c, R, c->dOwned.p, sendPixels, X.send.p, false, st);
    if (loopBack) PT_CHECK_HIP(c, record_poison(c, R, st));
    PT_CHECK_NCCL(c, g_rccl.GroupStart());
    ncclResult_t bad = ncclSuccess;
    for (const ShardStep& s : steps) {
        if (s.send && bad == ncclSuccess) bad = g_rccl.Send(X.send.p, s.send * W, ncclFloat, (int)s.peer, c->comm, st);
        if (s.recv && bad == ncclSuccess) bad = g_rccl.Recv(X.recv.p + s.offset * W, s.recv * W, ncclFloat, (int)s.peer, c->comm, st);
    }
    const ncclResult_t ge = g_rccl.GroupEnd();      // (on every path: a group left open would swallow the next call's transfers)
    if (bad != ncclSuccess || ge != ncclSuccess) return fail(c, PT_ERROR_HIP, std::string(R.rccl) + (loopBack ? " loop-back: " : ": ") + g_rccl.GetErrorString(bad != ncclSuccess ? bad : ge));
    record_copy(c, R, received, recvPixels, X.recv.p, true, st);
    return PT_OK;
}

// ---- behind the eight pack / unpack exports (device pointers; the caller has checked its arguments and that the record is there): the owned pixels' records in the order of
// the rank's pixel list (pt_shard_layout) / the records of rank `rank`'s pixels into the context's buffers
int pack_owned(pt_context* c, const ShardRecord& R, void* dst, size_t bytes) {
    if (bytes < c->owned.size() * (size_t)R.words * 4u) return fail(c, PT_ERROR_INVALID_ARGUMENT, R.destSmall);
    (void)hipSetDevice(c->device);
    record_copy(c, R, c->dOwned.p, c->owned.size(), (uint*)dst, false, c->stream);
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}
int unpack_rank(pt_context* c, const ShardRecord& R, const void* src, size_t bytes, uint32_t rank) {
    const std::vector<uint>& px = c->shardPixels[rank];
    if (bytes < px.size() * (size_t)R.words * 4u) return fail(c, PT_ERROR_INVALID_ARGUMENT, R.sourceSmall);
    (void)hipSetDevice(c->device);
    DevBuf<uint> list; PT_CHECK_HIP(c, list.upload(px, c->stream));
    record_copy(c, R, list.p, px.size(), (uint*)src, true, c->stream);      // (unpack: `src` is only read)
    const hipError_t e = hipStreamSynchronize(c->stream);
    list.free();
    PT_CHECK_HIP(c, e); PT_CHECK_HIP(c, hipGetLastError());
    return PT_OK;
}

} // namespace

void build_shards(pt_context* c) {
    shard_pixel_lists(c->width, c->height, c->shardCount, c->shardPixels);
    c->owned = c->shardPixels[c->shardRank];
    c->staging.w = c->staging.h = 0;      // the peers' pixel list follows the shard lists
}

// Tile-sharded frames (pt_create with shardCount > 1): a rank traces, and feeds back for, its own pixels only, but the baker's passes read whole
// neighbourhoods. Between two frames every rank therefore receives the other ranks' reservoirs and exported depth (12 bytes per pixel: 100 MB for a 4K frame;
// the depth is what the reprojection tests — a pixel another rank traced would otherwise read as depth 0, "valid" by NaN compare, whatever its owner sees) and
// then runs the same deterministic passes on the same planes as everybody else: identical tables and proxy counts on all ranks, identical to the unsharded run.
// Without a communicator the host moves the packed buffers (pt_neeat_pack_feedback / pt_neeat_unpack_feedback).
int neeat_exchange_feedback(pt_context* c) {
    if (c->shardCount == 1 || !c->comm || !c->neeat.feedbackFilled || c->neeat.W != c->width || c->neeat.H != c->height) return PT_OK;
    return shard_exchange(c, FEEDBACK, SHARD_ALL_TO_ALL);
}
// ---- the realtime frame on tile shards (no reference analogue). The baker's passes read whole neighbourhoods of three things a rank only has for its own
// tiles: last frame's reservoirs (UpdateBegin resolves them into the history), and this frame's depth and motion vectors (UpdateEnd reprojects through them).
// So a sharded frame has two exchanges: the reservoirs before UpdateBegin (neeat_exchange_feedback, as between two reference-mode frames) and the build pass's
// guides — depth and motion vectors, 16 bytes per pixel with the hit-distance word that lies between them — before UpdateEnd; every rank then runs the same
// deterministic baker passes on the same planes. With a communicator pt_realtime_frame does both itself; without one the host drives the parts and moves the
// packed buffers: pt_neeat_pack / unpack_feedback -> pt_neeat_update_begin -> pt_build_stable_planes -> pt_pack / unpack_stable_plane_guides ->
// pt_neeat_update_end -> pt_fill_stable_planes
int sp_exchange_guides(pt_context* c) {
    if (c->shardCount == 1 || !c->comm) return PT_OK;
    return shard_exchange(c, GUIDES, SHARD_ALL_TO_ALL);
}

extern "C" {

int32_t pt_comm_unique_id(void* id128) {
    if (!id128) return PT_ERROR_INVALID_ARGUMENT;
    if (!g_rccl.load()) return PT_ERROR_HIP;
    static_assert(sizeof(ncclUniqueId) == PT_COMM_ID_BYTES, "unique id size");
    ncclUniqueId id; if (g_rccl.GetUniqueId(&id) != ncclSuccess) return PT_ERROR_HIP;
    memcpy(id128, &id, sizeof(id));
    return PT_OK;
}
int32_t pt_comm_init(pt_context* c, const void* id128, uint32_t rank, uint32_t world) {
    if (!c || !id128) return fail(c, PT_ERROR_INVALID_ARGUMENT, "null argument");
    if (rank != c->shardRank || world != c->shardCount) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_comm_init: rank / world must equal the context's shardRank / shardCount");
    if (!g_rccl.load()) return fail(c, PT_ERROR_HIP, g_rccl.error);
    (void)hipSetDevice(c->device);
    if (c->comm) { (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
    ncclUniqueId id; memcpy(&id, id128, sizeof(id));
    PT_CHECK_NCCL(c, g_rccl.CommInitRank(&c->comm, (int)world, id, (int)rank));
    return PT_OK;
}
int32_t pt_comm_destroy(pt_context* c) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (c->comm && g_rccl.lib) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); (void)g_rccl.CommDestroy(c->comm); }
    c->comm = nullptr;
    return PT_OK;
}

// ---- the radiance (16 bytes per pixel)
int32_t pt_shard_info(pt_context* c, uint32_t* numOwned, size_t* bytes) {
    if (!c || !c->width) return fail(c, PT_ERROR_NOT_READY, "pt_resize first");
    if (numOwned) *numOwned = (uint32_t)c->owned.size(); if (bytes) *bytes = c->owned.size() * 16;
    return PT_OK;
}
int32_t pt_device_radiance(pt_context* c, void** p) { if (!c || !p || !c->width) return PT_ERROR_INVALID_ARGUMENT; *p = c->dAccum.p; return PT_OK; }
int32_t pt_pack_shard(pt_context* c, void* dst, size_t bytes) {
    if (!c || !dst || !c->width) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bad argument");
    return pack_owned(c, RADIANCE, dst, bytes);
}
int32_t pt_unpack_shard(pt_context* c, const void* src, size_t bytes, uint32_t rank) {
    if (!c || !src || !c->width || rank >= c->shardCount) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bad argument");
    return unpack_rank(c, RADIANCE, src, bytes, rank);
}
// every rank's tiles to rank 0's accumulation buffer; asynchronous (pt_map_radiance waits for the stream)
int32_t pt_gather(pt_context* c) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!RADIANCE.ready(c)) return fail(c, PT_ERROR_NOT_READY, RADIANCE.notReady);
    if (c->shardCount == 1 && !c->comm) return PT_OK;                           // nothing to gather
    if (!c->comm) return fail(c, PT_ERROR_NOT_READY, "pt_comm_init first");
    (void)hipSetDevice(c->device);
    return shard_exchange(c, RADIANCE, SHARD_TO_ROOT);
}

// ---- the NEE-AT reservoirs and exported depth as (weight bits, candidate, depth bits) triples (12 bytes per pixel)
int32_t pt_neeat_pack_feedback(pt_context* c, void* dst, size_t bytes) {
    if (!c || !dst) return PT_ERROR_INVALID_ARGUMENT;
    if (!FEEDBACK.ready(c)) return fail(c, PT_ERROR_NOT_READY, FEEDBACK.notReady);
    return pack_owned(c, FEEDBACK, dst, bytes);
}
int32_t pt_neeat_unpack_feedback(pt_context* c, const void* src, size_t bytes, uint32_t rank) {
    if (!c || !src || rank >= c->shardCount) return PT_ERROR_INVALID_ARGUMENT;
    if (!FEEDBACK.ready(c)) return fail(c, PT_ERROR_NOT_READY, FEEDBACK.notReady);
    return unpack_rank(c, FEEDBACK, src, bytes, rank);
}

// ---- the build pass's guides: depth, specular hit distance, motion vectors (16 bytes per pixel)
int32_t pt_pack_stable_plane_guides(pt_context* c, void* dst, size_t bytes) {
    if (!c || !dst) return PT_ERROR_INVALID_ARGUMENT;
    if (!GUIDES.ready(c)) return fail(c, PT_ERROR_NOT_READY, GUIDES.notReady);
    return pack_owned(c, GUIDES, dst, bytes);
}
int32_t pt_unpack_stable_plane_guides(pt_context* c, const void* src, size_t bytes, uint32_t rank) {
    if (!c || !src || rank >= c->shardCount) return PT_ERROR_INVALID_ARGUMENT;
    if (!GUIDES.ready(c)) return fail(c, PT_ERROR_NOT_READY, unpack_not_ready(GUIDES));
    return unpack_rank(c, GUIDES, src, bytes, rank);
}

// ---- the plane buffers (no reference analogue): every rank builds and fills the planes of its own tiles; the rank that denoises or shows the frame needs them all.
// 284 bytes per pixel (SP_SHARD_WORDS): header, three plane records, stable radiance, depth, specular hit distance, motion vectors, throughput.
int32_t pt_stable_planes_shard_bytes(pt_context* c, uint32_t rank, size_t* bytes) {
    if (!c || !bytes || rank >= c->shardCount || !c->width) return PT_ERROR_INVALID_ARGUMENT;
    *bytes = c->shardPixels[rank].size() * (size_t)SP_SHARD_WORDS * 4u; return PT_OK;
}
int32_t pt_pack_stable_planes(pt_context* c, void* dst, size_t bytes) {
    if (!c || !dst) return PT_ERROR_INVALID_ARGUMENT;
    if (!PLANES.ready(c)) return fail(c, PT_ERROR_NOT_READY, PLANES.notReady);
    return pack_owned(c, PLANES, dst, bytes);
}
int32_t pt_unpack_stable_planes(pt_context* c, const void* src, size_t bytes, uint32_t rank) {
    if (!c || !src || rank >= c->shardCount) return PT_ERROR_INVALID_ARGUMENT;
    if (!PLANES.ready(c)) return fail(c, PT_ERROR_NOT_READY, unpack_not_ready(PLANES));
    int r = unpack_rank(c, PLANES, src, bytes, rank); if (r != PT_OK) return r;
    c->spGathered = true;      // (the host says when all ranks are in: pt_denoise_spec_hit_t trusts it from here on)
    return PT_OK;
}
// pt_gather for the plane buffers; waits for the stream, and rank 0 then holds the whole frame's planes
int32_t pt_gather_stable_planes(pt_context* c) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    if (!PLANES.ready(c)) return fail(c, PT_ERROR_NOT_READY, PLANES.notReady);
    if (c->shardCount == 1 && !c->comm) return PT_OK;
    if (!c->comm) return fail(c, PT_ERROR_NOT_READY, "pt_comm_init first");
    (void)hipSetDevice(c->device);
    int r = shard_exchange(c, PLANES, SHARD_TO_ROOT); if (r != PT_OK) return r;
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    if (c->shardCount > 1 && c->shardRank == 0) c->spGathered = true;
    return PT_OK;
}

} // extern "C"

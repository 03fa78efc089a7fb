// mi355pt — the texture pool made on the device (PT_DEVICE_TEXTURES_ON_DEVICE; include/mi355pt.h): pt_set_materials' source pixels stream through a pinned staging buffer
// of two halves (PT_TEXTURE_STAGING_BYTES) — while k_tex_level0 converts one half on the context's stream, the host fills the other and a copy stream brings it over — then
// k_tex_mip makes level l of every texture that has one in one launch (at most 15 launches a scene), k_tex_alpha_scan decides per RGBA32F texture whether its opacities are
// all k / 255, and k_tex_alpha_fill writes every alpha plane from the .w of its level 0. The arithmetic and the layout are pt_texture_ingest.h's, the text the host path
// runs: the same bits in the same TexInfo / AlphaPlane tables. The number of launches depends on the levels and the staging chunks, never on the number of textures: every
// kernel reads a row table (one row per texture or per piece of one, with the work items before it) and each work item finds its row by bisection.
// All four kernels stream: a texel is read once and written once, 16 bytes a lane where a row's alignment allows (always for the float texels; four RGBA8 texels per lane
// as one 16-byte load; four opacities per lane as one 4- or 16-byte store), blocks of 256, no LDS beyond k_tex_level0's two 256-entry decode tables, no scratch.
#include "pt_context.h"
#include <algorithm>
#include <chrono>
#include <cstring>

using namespace ptk;

namespace {

// k_tex_level0: a piece of one texture's source in a staging half. src: byte offset in the half (a multiple of 16); dst: the pool index of its first texel; itemStart: the
// work items of the rows before it (an item: four texels of an 8-bit source, one texel of a float source)
struct TexSeg { unsigned long long dst; uint src, count, format, itemStart; };
// k_tex_mip: one texture's level l. src / dst: pool indices of levels l - 1 and l; start: the texels of the rows before it
struct TexMipRow { unsigned long long src, dst, start; uint pw, ph, mw, mh; };
// k_tex_alpha_scan / k_tex_alpha_fill: one texture's level 0. src: its pool index; start: the work items before it (scan: a texel; fill: four texels); plane: the byte offset
// of its alpha plane; fmt: 0 = bytes, 1 = floats
struct TexAlphaRow { unsigned long long src, start; uint count, plane, fmt, tex; };
const uint TEX_MAX_SEGS = 4096u;      // rows of one staging chunk (a chunk closes when either its bytes or its rows are full)

template <typename Row, typename Start> __device__ inline uint tex_find_row(const Row* rows, uint n, Start i, Start Row::*start) {
    uint lo = 0u, hi = n;                                     // the last row that starts at or before i (the first row starts at 0)
    while (hi - lo > 1u) { const uint mid = (lo + hi) >> 1; if (rows[mid].*start <= i) lo = mid; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(256) void k_tex_level0(const unsigned char* __restrict__ stage, const TexSeg* __restrict__ segs, uint numSegs, uint totalItems, ptk::float4* __restrict__ pool) {
    // the 256 values a byte decodes to, made by the function the host path calls per channel: a table of the same function returns the same floats
    __shared__ float lutU[256], lutS[256];
    lutU[threadIdx.x] = texi_channel(threadIdx.x, false); lutS[threadIdx.x] = texi_channel(threadIdx.x, true);
    __syncthreads();
    for (uint i = blockIdx.x * 256u + threadIdx.x; i < totalItems; i += gridDim.x * 256u) {
        const TexSeg s = segs[tex_find_row(segs, numSegs, i, &TexSeg::itemStart)];
        const uint k = i - s.itemStart;
        if (s.format == TEXI_RGBA32F) { pool[s.dst + k] = reinterpret_cast<const ptk::float4*>(stage + s.src)[k]; continue; }
        const uint t0 = 4u * k, n = (s.count - t0 < 4u) ? s.count - t0 : 4u;
        uint w[4] = {0u, 0u, 0u, 0u};
        if (n == 4u) { const ptk::uint4 v = *reinterpret_cast<const ptk::uint4*>(stage + s.src + 16u * (size_t)k); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
        else for (uint j = 0; j < n; j++) w[j] = reinterpret_cast<const uint*>(stage + s.src)[t0 + j];
        const float* lut = s.format == TEXI_RGBA8_SRGB ? lutS : lutU;
        for (uint j = 0; j < n; j++) pool[s.dst + t0 + j] = ptk::make_float4(lut[w[j] & 0xFFu], lut[(w[j] >> 8) & 0xFFu], lut[(w[j] >> 16) & 0xFFu], lutU[w[j] >> 24]);
    }
}

__global__ __launch_bounds__(256) void k_tex_mip(const ptk::float4* src, ptk::float4* dst, const TexMipRow* __restrict__ rows, uint numRows, unsigned long long total) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const TexMipRow r = rows[tex_find_row(rows, numRows, i, &TexMipRow::start)];
    const uint k = (uint)(i - r.start), y = k / r.mw, x = k - y * r.mw;
    dst[r.dst + k] = texi_mip_texel(src + r.src, r.pw, r.ph, x, y);
}

// one word per texture, raised when an opacity of its level 0 is no k / 255: a wave votes, and one lane per texture the wave's counter-examples belong to writes
__global__ __launch_bounds__(256) void k_tex_alpha_scan(const ptk::float4* __restrict__ pool, const TexAlphaRow* __restrict__ rows, uint numRows, unsigned long long total, uint* __restrict__ words) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    bool bad = false; uint tex = 0xFFFFFFFFu;
    if (i < total) {
        const TexAlphaRow r = rows[tex_find_row(rows, numRows, i, &TexAlphaRow::start)];
        bad = !texi_alpha_is_byte(pool[r.src + (i - r.start)].w); tex = r.tex;
    }
    unsigned long long m = __ballot(bad);
    const uint lane = threadIdx.x & 63u;
    while (m) {
        const uint leader = (uint)__ffsll((long long)m) - 1u;
        const uint lt = __shfl(tex, (int)leader);
        const unsigned long long same = __ballot(bad && tex == lt);
        if (lane == leader) atomicOr(&words[lt], 1u);
        m &= ~same;
    }
}

__global__ __launch_bounds__(256) void k_tex_alpha_fill(const ptk::float4* __restrict__ pool, const TexAlphaRow* __restrict__ rows, uint numRows, unsigned long long total, unsigned char* __restrict__ apool) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const TexAlphaRow r = rows[tex_find_row(rows, numRows, i, &TexAlphaRow::start)];
    const uint t0 = 4u * (uint)(i - r.start), n = (r.count - t0 < 4u) ? r.count - t0 : 4u;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (uint j = 0; j < n; j++) a[j] = pool[r.src + t0 + j].w;
    if (r.fmt == 0u) {                      // (planes start on 16-byte boundaries and t0 is a multiple of four: the word store is aligned)
        unsigned char* p = apool + r.plane + t0;
        if (n == 4u) *reinterpret_cast<uint*>(p) = (uint)texi_alpha_byte(a[0]) | ((uint)texi_alpha_byte(a[1]) << 8) | ((uint)texi_alpha_byte(a[2]) << 16) | ((uint)texi_alpha_byte(a[3]) << 24);
        else for (uint j = 0; j < n; j++) p[j] = (unsigned char)texi_alpha_byte(a[j]);
    } else {
        float* p = reinterpret_cast<float*>(apool + r.plane) + t0;
        if (n == 4u) *reinterpret_cast<ptk::float4*>(p) = ptk::make_float4(a[0], a[1], a[2], a[3]);
        else for (uint j = 0; j < n; j++) p[j] = a[j];
    }
}

struct Events {          // HIP events of one ingest, destroyed with it
    std::vector<hipEvent_t> ev;
    hipError_t make(size_t n) { ev.assign(n, nullptr); for (auto& e : ev) { hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; } return hipSuccess; }
    ~Events() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
    double ms(size_t a, size_t b) const { float t = 0.f; return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : 0.0; }
};

// The staging buffer of one ingest: pinned host memory of two halves, its twin on the device, a row table per half. add() cuts a texture's source into pieces that fit
// what is left of the open half; flush() sends the half over on the copy stream and launches k_tex_level0 behind it on the context's stream; the other half opens once the
// kernel that read it last has finished.
struct Stager {
    pt_context* c = nullptr; unsigned char* pinned = nullptr; unsigned char* dStage = nullptr; TexSeg* pinnedSegs = nullptr; TexSeg* dSegs = nullptr;
    size_t half = 0; hipStream_t copy = nullptr; Events ev; bool used[2] = {false, false};
    uint cur = 0, nSegs = 0, items = 0; size_t fill = 0;
    uint chunks = 0, launches = 0; double uploadMs = 0, level0Ms = 0;

    int init(pt_context* ctx, size_t sourceBytes) {
        c = ctx;
        // no larger than the sources need (every piece starts on a 16-byte boundary: 16 bytes of slack a texture), two halves of a multiple of 16 bytes, one float texel at least
        const size_t want = std::min<size_t>(c->texStagingBytes, 2u * (sourceBytes + 16u * (c->textures.size() + 1u)));
        half = std::max<size_t>(16u, (want / 2u) & ~(size_t)15u);
        PT_CHECK_HIP(c, hipHostMalloc((void**)&pinned, 2u * half, hipHostMallocDefault)); PT_CHECK_HIP(c, hipHostMalloc((void**)&pinnedSegs, 2u * TEX_MAX_SEGS * sizeof(TexSeg), hipHostMallocDefault));
        PT_CHECK_HIP(c, hipMalloc((void**)&dStage, 2u * half)); PT_CHECK_HIP(c, hipMalloc((void**)&dSegs, 2u * TEX_MAX_SEGS * sizeof(TexSeg)));
        PT_CHECK_HIP(c, hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        PT_CHECK_HIP(c, ev.make(8));          // per half: copy begins, copy done, kernel begins, kernel done
        return PT_OK;
    }
    ~Stager() {
        if (copy) { (void)hipStreamSynchronize(copy); (void)hipStreamDestroy(copy); }
        if (pinned) (void)hipHostFree(pinned); if (pinnedSegs) (void)hipHostFree(pinnedSegs); if (dStage) (void)hipFree(dStage); if (dSegs) (void)hipFree(dSegs);
    }
    int retire(uint h) {                  // the half's last chunk has been converted: its times are read, the half may be written again
        if (!used[h]) return PT_OK;
        PT_CHECK_HIP(c, hipEventSynchronize(ev.ev[4 * h + 3]));
        uploadMs += ev.ms(4 * h, 4 * h + 1); level0Ms += ev.ms(4 * h + 2, 4 * h + 3); used[h] = false;
        return PT_OK;
    }
    int flush() {
        if (!nSegs) return PT_OK;
        const uint h = cur;
        PT_CHECK_HIP(c, hipEventRecord(ev.ev[4 * h], copy));
        PT_CHECK_HIP(c, hipMemcpyAsync(dStage + h * half, pinned + h * half, fill, hipMemcpyHostToDevice, copy));
        PT_CHECK_HIP(c, hipMemcpyAsync(dSegs + h * TEX_MAX_SEGS, pinnedSegs + h * TEX_MAX_SEGS, nSegs * sizeof(TexSeg), hipMemcpyHostToDevice, copy));
        PT_CHECK_HIP(c, hipEventRecord(ev.ev[4 * h + 1], copy));
        PT_CHECK_HIP(c, hipStreamWaitEvent(c->stream, ev.ev[4 * h + 1], 0));
        PT_CHECK_HIP(c, hipEventRecord(ev.ev[4 * h + 2], c->stream));
        const uint blocks = std::min<uint>((items + 255u) / 256u, 2048u);
        hipLaunchKernelGGL(k_tex_level0, dim3(blocks), dim3(256), 0, c->stream, dStage + h * half, dSegs + h * TEX_MAX_SEGS, nSegs, items, c->dTexels.p);
        PT_CHECK_HIP(c, hipEventRecord(ev.ev[4 * h + 3], c->stream));
        used[h] = true; chunks++; launches++;
        cur ^= 1u; nSegs = 0; items = 0; fill = 0;
        return retire(cur);
    }
    int add(const void* pixels, size_t texels, uint format, unsigned long long dst) {
        const size_t bpt = format == TEXI_RGBA32F ? 16u : 4u; const unsigned char* src = (const unsigned char*)pixels;
        while (texels) {
            fill = (fill + 15u) & ~(size_t)15u;
            size_t room = fill < half ? (half - fill) / bpt : 0u;
            if (!room || nSegs == TEX_MAX_SEGS) { int r = flush(); if (r != PT_OK) return r; continue; }
            const size_t n = std::min(texels, room);
            memcpy(pinned + cur * half + fill, src, n * bpt);
            TexSeg& s = pinnedSegs[cur * TEX_MAX_SEGS + nSegs++]; s.dst = dst; s.src = (uint)fill; s.count = (uint)n; s.format = format; s.itemStart = items;
            items += format == TEXI_RGBA32F ? (uint)n : (uint)((n + 3u) / 4u);
            fill += n * bpt; src += n * bpt; dst += n; texels -= n;
        }
        return PT_OK;
    }
    int finish() { int r = flush(); if (r != PT_OK) return r; r = retire(0); if (r != PT_OK) return r; return retire(1); }
};

template <typename T> struct Scratch {      // a device buffer of one ingest
    T* p = nullptr;
    hipError_t upload(const std::vector<T>& v, hipStream_t st) {
        hipError_t e = hipMalloc((void**)&p, sizeof(T) * std::max<size_t>(1, v.size())); if (e != hipSuccess || v.empty()) return e;
        return hipMemcpyAsync(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st);
    }
    ~Scratch() { if (p) (void)hipFree(p); }
};

size_t source_bytes(const pt_context* c, uint i) { return (size_t)c->textures[i].w * c->textures[i].h * (c->texFormats[i] == TEXI_RGBA32F ? 16u : 4u); }
size_t env_texels(const pt_context* c) { return (c->envEnabled && c->envTex.w) ? (size_t)c->envTex.w * c->envTex.h : 0u; }
size_t env_host_bytes(const pt_context* c) { size_t n = 0; for (auto& m : c->envTex.mips) n += m.size() * sizeof(ptk::float4); return n; }

// the chains of the textures `which`: level l of all of them in one launch. `rows` must outlive the stream's work (the caller synchronises).
int run_mips(pt_context* c, const std::vector<uint>& which, std::vector<TexMipRow>& rows, Scratch<TexMipRow>& dRows, uint* launches) {
    uint first[17] = {0}; unsigned long long total[16] = {0};
    for (uint l = 1; l < 16u; l++) {
        first[l] = (uint)rows.size();
        for (uint i : which) {
            const TexInfo& ti = c->texInfos[i];
            if (ti.mipLevels <= l) continue;
            TexMipRow r; r.src = ti.base + ti.mipOffset[l - 1]; r.dst = ti.base + ti.mipOffset[l]; r.start = total[l];
            r.pw = texi_side(ti.w, l - 1); r.ph = texi_side(ti.h, l - 1); r.mw = texi_side(ti.w, l); r.mh = texi_side(ti.h, l);
            total[l] += (unsigned long long)r.mw * r.mh; rows.push_back(r);
        }
    }
    first[16] = (uint)rows.size();
    PT_CHECK_HIP(c, dRows.upload(rows, c->stream));
    for (uint l = 1; l < 16u; l++) {
        if (!total[l]) break;
        const unsigned long long blocks = (total[l] + 255u) / 256u;
        if (blocks > 0x7FFFFFFFull) return fail(c, PT_ERROR_UNSUPPORTED, "texture ingest: more than 2^39 texels in one mip level of a scene");
        hipLaunchKernelGGL(k_tex_mip, dim3((uint)blocks), dim3(256), 0, c->stream, c->dTexels.p, c->dTexels.p, dRows.p + first[l], first[l + 1] - first[l], total[l]);
        (*launches)++;
    }
    return PT_OK;
}
// rows of the textures `which` for the scan (per texel, RGBA32F sources only) or the fill (per four texels)
unsigned long long alpha_rows(const pt_context* c, const std::vector<uint>& which, bool scan, std::vector<TexAlphaRow>& rows) {
    unsigned long long total = 0; rows.clear();
    for (uint i : which) {
        if (scan && c->texFormats[i] != TEXI_RGBA32F) continue;
        const TexInfo& ti = c->texInfos[i];
        TexAlphaRow r; r.src = ti.base; r.start = total; r.count = ti.w * ti.h; r.tex = i; r.plane = scan ? 0u : c->alphaPlanes[i].offset; r.fmt = scan ? 0u : c->alphaPlanes[i].fmt;
        total += scan ? r.count : (r.count + 3u) / 4u; rows.push_back(r);
    }
    return total;
}
int launch_alpha(pt_context* c, bool scan, const std::vector<TexAlphaRow>& rows, Scratch<TexAlphaRow>& dRows, unsigned long long total, uint* words, uint* launches) {
    if (!total) return PT_OK;
    const unsigned long long blocks = (total + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return fail(c, PT_ERROR_UNSUPPORTED, "texture ingest: more than 2^39 level-0 texels in a scene");
    PT_CHECK_HIP(c, dRows.upload(rows, c->stream));
    if (scan) hipLaunchKernelGGL(k_tex_alpha_scan, dim3((uint)blocks), dim3(256), 0, c->stream, c->dTexels.p, dRows.p, (uint)rows.size(), total, words);
    else hipLaunchKernelGGL(k_tex_alpha_fill, dim3((uint)blocks), dim3(256), 0, c->stream, c->dTexels.p, dRows.p, (uint)rows.size(), total, c->dAlphaPool.p);
    (*launches)++;
    return PT_OK;
}
// the plane table and the alpha pool for `fmts`, zeroed (the padding between planes is zero bytes, as the host path's), and every plane filled
int rebuild_alpha_pool(pt_context* c, const std::vector<uint>& fmts, const std::vector<uint>& all, uint* launches) {
    size_t poolBytes = 0;
    { int r = tex_plan_alpha_planes(c, fmts, &poolBytes); if (r != PT_OK) return r; }
    PT_CHECK_HIP(c, c->dAlphaPool.resize(poolBytes)); PT_CHECK_HIP(c, hipMemsetAsync(c->dAlphaPool.p, 0, poolBytes, c->stream));
    PT_CHECK_HIP(c, c->dAlphaPlanes.upload(c->alphaPlanes, c->stream));
    std::vector<TexAlphaRow> rows; Scratch<TexAlphaRow> dRows; const unsigned long long total = alpha_rows(c, all, false, rows);
    { int r = launch_alpha(c, false, rows, dRows, total, nullptr, launches); if (r != PT_OK) return r; }
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));      // (rows and dRows end here)
    return PT_OK;
}

} // namespace

int tex_plan_alpha_planes(pt_context* c, const std::vector<uint>& fmts, size_t* poolBytes) {
    c->alphaPlanes.assign(std::max<size_t>(1, c->textures.size()), ptk::AlphaPlane{0u, 0u, 0u, 0u});
    size_t at = 0;
    for (size_t ti = 0; ti < c->textures.size(); ti++) {
        const HostTexture& t = c->textures[ti]; const bool bytes = fmts[ti] == 0u;
        at = texi_alpha_align(at);
        if (at + texi_alpha_plane_bytes(t.w, t.h, bytes) > 0xFFFFFFF0ull) return fail(c, PT_ERROR_UNSUPPORTED, "alpha planes above 4 GB are not supported");
        if (t.w > 0xFFFFu || t.h > 0xFFFFu) return fail(c, PT_ERROR_UNSUPPORTED, "textures larger than 65535 texels on a side are not supported (the traversal's alpha test packs the size into 16 + 16 bits)");
        ptk::AlphaPlane& ap = c->alphaPlanes[ti]; ap.wh = (t.w & 0xFFFFu) | (t.h << 16); ap.offset = (uint)at; ap.fmt = bytes ? 0u : 1u;
        at += texi_alpha_plane_bytes(t.w, t.h, bytes);
    }
    *poolBytes = texi_alpha_pool_end(at);
    return PT_OK;
}

int tex_ingest_all(pt_context* c, const PtTextureDesc* tex, uint32_t n) {
    const auto t0 = std::chrono::steady_clock::now();
    (void)hipSetDevice(c->device);
    PtTextureIngestStats s; memset(&s, 0, sizeof(s)); s.onDevice = 1u;
    // the layout, from the sizes alone
    c->texInfos.clear(); size_t base = 0;
    for (uint32_t i = 0; i < n; i++) {
        TexInfo ti; memset(&ti, 0, sizeof(ti)); ti.w = tex[i].width; ti.h = tex[i].height; ti.base = base;
        base += texi_layout(ti.w, ti.h, &ti.mipLevels, ti.mipOffset);
        c->texInfos.push_back(ti); s.sourceBytes += source_bytes(c, i); s.level0Texels += (uint64_t)ti.w * ti.h;
    }
    c->matTexels = base;
    PT_CHECK_HIP(c, c->dTexels.resize(base + env_texels(c)));          // (room for the environment image as it is now: tex_place_environment)
    PT_CHECK_HIP(c, c->dTexInfos.upload(c->texInfos, c->stream));
    Events ev; PT_CHECK_HIP(c, ev.make(6));
    std::vector<uint> all(n); for (uint32_t i = 0; i < n; i++) all[i] = i;
    std::vector<TexMipRow> mipRows; Scratch<TexMipRow> dMipRows; std::vector<TexAlphaRow> scanRows; Scratch<TexAlphaRow> dScanRows; Scratch<uint> dWords;
    if (n) {
        Stager st; { int r = st.init(c, (size_t)s.sourceBytes); if (r != PT_OK) return r; }
        for (uint32_t i = 0; i < n; i++) { int r = st.add(tex[i].pixels, (size_t)tex[i].width * tex[i].height, tex[i].format, c->texInfos[i].base); if (r != PT_OK) return r; }
        { int r = st.finish(); if (r != PT_OK) return r; }
        s.stagingChunks = st.chunks; s.launches = st.launches; s.uploadMs = st.uploadMs; s.level0Ms = st.level0Ms;
    }
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[0], c->stream));
    { int r = run_mips(c, all, mipRows, dMipRows, &s.launches); if (r != PT_OK) return r; }
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[1], c->stream));
    // which RGBA32F textures hold opacities other than k / 255 (8-bit sources never do: pt_texture_ingest.h)
    std::vector<uint> words(std::max<uint32_t>(1u, n), 0u);
    PT_CHECK_HIP(c, dWords.upload(words, c->stream));
    const unsigned long long scanTotal = alpha_rows(c, all, true, scanRows);
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[2], c->stream));
    { int r = launch_alpha(c, true, scanRows, dScanRows, scanTotal, dWords.p, &s.launches); if (r != PT_OK) return r; }
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[3], c->stream));
    PT_CHECK_HIP(c, hipMemcpyAsync(words.data(), dWords.p, 4u * words.size(), hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<uint> fmts(n); for (uint32_t i = 0; i < n; i++) fmts[i] = words[i] ? 1u : 0u;
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[4], c->stream));
    { int r = rebuild_alpha_pool(c, fmts, all, &s.launches); if (r != PT_OK) return r; }
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[5], c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); PT_CHECK_HIP(c, hipGetLastError());
    s.mipMs = ev.ms(0, 1); s.alphaMs = ev.ms(2, 3) + ev.ms(4, 5);
    s.poolTexels = c->dTexels.n; s.hostBytesHeld = env_host_bytes(c);          // (the staging buffer has been freed; the environment image is the host's to convert)
    s.totalMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->texStats = s;
    return PT_OK;
}

int tex_update_one(pt_context* c, uint32_t index, const PtTextureDesc* desc) {
    const auto t0 = std::chrono::steady_clock::now();
    (void)hipSetDevice(c->device);
    PtTextureIngestStats s; memset(&s, 0, sizeof(s)); s.onDevice = 1u;
    const TexInfo& ti = c->texInfos[index];
    s.sourceBytes = source_bytes(c, index); s.level0Texels = (uint64_t)ti.w * ti.h;
    Events ev; PT_CHECK_HIP(c, ev.make(6));
    const std::vector<uint> one(1, index);
    std::vector<TexMipRow> mipRows; Scratch<TexMipRow> dMipRows; std::vector<TexAlphaRow> scanRows, fillRows; Scratch<TexAlphaRow> dScanRows, dFillRows; Scratch<uint> dWords;
    {
        Stager st; { int r = st.init(c, (size_t)s.sourceBytes); if (r != PT_OK) return r; }
        { int r = st.add(desc->pixels, (size_t)ti.w * ti.h, desc->format, ti.base); if (r != PT_OK) return r; }
        { int r = st.finish(); if (r != PT_OK) return r; }
        s.stagingChunks = st.chunks; s.launches = st.launches; s.uploadMs = st.uploadMs; s.level0Ms = st.level0Ms;
    }
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[0], c->stream));
    { int r = run_mips(c, one, mipRows, dMipRows, &s.launches); if (r != PT_OK) return r; }
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[1], c->stream));
    std::vector<uint> words(c->textures.size(), 0u);
    PT_CHECK_HIP(c, dWords.upload(words, c->stream));
    const unsigned long long scanTotal = alpha_rows(c, one, true, scanRows);
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[2], c->stream));
    { int r = launch_alpha(c, true, scanRows, dScanRows, scanTotal, dWords.p, &s.launches); if (r != PT_OK) return r; }
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[3], c->stream));
    PT_CHECK_HIP(c, hipMemcpyAsync(words.data(), dWords.p, 4u * words.size(), hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[4], c->stream));
    if (c->alphaPlanes[index].fmt == 0u && words[index]) {
        // a byte plane receives opacities that are no k / 255: it becomes a float plane, the planes behind it move, and the alpha records of the geometry with them
        std::vector<uint> fmts(c->textures.size()), all(c->textures.size());
        for (size_t i = 0; i < fmts.size(); i++) { fmts[i] = c->alphaPlanes[i].fmt; all[i] = (uint)i; }
        fmts[index] = 1u;
        { int r = rebuild_alpha_pool(c, fmts, all, &s.launches); if (r != PT_OK) return r; }
        c->geomDirty = true;
    } else {
        const unsigned long long total = alpha_rows(c, one, false, fillRows);
        { int r = launch_alpha(c, false, fillRows, dFillRows, total, nullptr, &s.launches); if (r != PT_OK) return r; }
    }
    PT_CHECK_HIP(c, hipEventRecord(ev.ev[5], c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream)); PT_CHECK_HIP(c, hipGetLastError());
    s.mipMs = ev.ms(0, 1); s.alphaMs = ev.ms(2, 3) + ev.ms(4, 5);
    s.poolTexels = c->dTexels.n; s.hostBytesHeld = env_host_bytes(c);
    s.totalMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->texStats = s;
    return PT_OK;
}

// The lat-long environment image keeps its place behind the material textures (TexInfo envTex, read by the cube bake only), converted on the host as one image. When the
// pool has no room for it, a larger pool is allocated and the material textures are copied over on the device: they are not ingested again.
int tex_place_environment(pt_context* c) {
    (void)hipSetDevice(c->device);
    if (!c->dAlphaPool.p || !c->dTexels.p) { int r = tex_ingest_all(c, nullptr, 0u); if (r != PT_OK) return r; }      // no pt_set_materials yet: the empty tables
    memset(&c->envTexInfo, 0, sizeof(TexInfo));
    const size_t n = env_texels(c);
    if (n) {
        if (c->dTexels.n < c->matTexels + n) {
            DevBuf<ptk::float4> grown; PT_CHECK_HIP(c, grown.resize(c->matTexels + n));
            if (c->matTexels) PT_CHECK_HIP(c, hipMemcpyAsync(grown.p, c->dTexels.p, sizeof(ptk::float4) * c->matTexels, hipMemcpyDeviceToDevice, c->stream));
            PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
            c->dTexels.free(); c->dTexels = grown;
        }
        PT_CHECK_HIP(c, hipMemcpyAsync(c->dTexels.p + c->matTexels, c->envTex.mips[0].data(), sizeof(ptk::float4) * n, hipMemcpyHostToDevice, c->stream));
        TexInfo& ti = c->envTexInfo; ti.w = c->envTex.w; ti.h = c->envTex.h; ti.mipLevels = 1u; ti.base = c->matTexels;
    }
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    c->texDirty = false;
    return PT_OK;
}

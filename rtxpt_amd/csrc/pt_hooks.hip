// mi355pt — the evaluation hooks of include/mi355pt_testhooks.h: pt_probe, pt_get_inert_terminal, pt_get_bvh8 and pt_trace_route, with their kernels. This file is linked into
// libmi355pt_testhooks.so only, on top of the very objects the shipped library is made of: the shipped library carries no evaluation hooks.
#include <cstring>
#include "pt_context.h"
#include "../../include/mi355pt_testhooks.h"
#include "pt_trace_device.h"
#include <cmath>

namespace ptk {
// known-answer probes for the tests: the device evaluates leaf functions so they can be compared bit-for-bit with the oracle
__global__ void __launch_bounds__(64) k_probe(PathKernelContext k, int kind, const float* __restrict__ in, float* __restrict__ out, uint n) {
    uint i = blockIdx.x * 64u + threadIdx.x; if (i >= n) return;
    switch (kind) {
    case 0: { const float* p = in + 3 * i; int fn = (int)p[0]; float x = p[1], y = p[2]; float r;      // dmath: (fn, x, y)
        switch (fn) { case 0: r = dm_sin(x); break; case 1: r = dm_cos(x); break; case 2: r = dm_exp2(x); break; case 3: r = dm_log2(x); break;
                      case 4: r = dm_atan2(y, x); break; case 5: r = dm_pow(x, y); break; case 6: r = FastACos(x); break; default: r = FastSqrt(x); break; }
        out[i] = r; } break;
    case 1: { float x = in[i]; uint hbits = f32tof16(x); out[2 * i] = asfloat(hbits); out[2 * i + 1] = f16tof32(hbits); } break;          // fp16 round trip
    // sample stream: pixel, vertex, sample, seed, kind, count(<=8)
    case 2: { const uint* p = reinterpret_cast<const uint*>(in) + 6 * i;
        SampleGeneratorVertexBase vb = SampleGeneratorVertexBase::make(p[0], p[1], p[2]);
        uint cnt = p[5] > 8 ? 8 : p[5];
        if (p[4] == 0) { float4 v = SampleSequenceGenerator::Generate(cnt, vb, p[3]); out[8 * i] = v.x; out[8 * i + 1] = v.y; out[8 * i + 2] = v.z; out[8 * i + 3] = v.w; }
        else if (p[4] == 1) { float4 v = UniformSampleSequenceGenerator::Generate(cnt, vb, p[3]); out[8 * i] = v.x; out[8 * i + 1] = v.y; out[8 * i + 2] = v.z; out[8 * i + 3] = v.w; }
        else if (p[4] == 2) { UniformSampleSequenceGenerator g = UniformSampleSequenceGenerator::make(vb, p[3]); for (uint j = 0; j < cnt; j++) out[8 * i + j] = sampleNext1D(g); }
        else { SampleSequenceGenerator g = SampleSequenceGenerator::make(vb, p[3], p[4] == 4); for (uint j = 0; j < cnt; j++) out[8 * i + j] = sampleNext1D(g); } } break;
    // bsdf probe: params[14], thin, model, wi[3], w[3], mode
    case 3: { const float* p = in + 24 * i;
        ShadingData sd; __builtin_memset(&sd, 0, sizeof(sd));
        sd.N = make_float3(0, 0, 1); sd.T = make_float3(1, 0, 0); sd.B = make_float3(0, 1, 0); sd.V = make_float3(p[16], p[17], p[18]);
        sd.faceNCorrected = sd.N; sd.vertexN = sd.N; sd.frontFacing = true; sd.mtl = MaterialHeader::make(); sd.mtl.setActiveLobes(Lobe_All); sd.mtl.setThinSurface(p[14] != 0.f);
        StandardBSDF b; b.diffuseModel = (int)p[15];
        b.data.diffuse = make_float3(p[0], p[1], p[2]); b.data.specular = make_float3(p[3], p[4], p[5]); b.data.roughness = p[6]; b.data.metallic = p[7];
        b.data.transmission = make_float3(p[8], p[9], p[10]); b.data.diffuseTransmission = p[11]; b.data.specularTransmission = p[12]; b.data.eta = p[13];
        float* o = out + 10 * i;
        if (p[22] == 0.f) { float3 wo = make_float3(p[19], p[20], p[21]); float4 e = b.eval(sd, wo); o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w; o[4] = b.evalPdf(sd, wo); o[5] = (float)b.getLobes(); o[6] = o[7] = o[8] = o[9] = 0.f; }
        else { BSDFSample s; __builtin_memset(&s, 0, sizeof(s)); bool v = b.sample(sd, make_float4(p[19], p[20], p[21], 0), s);
               o[0] = s.wo.x; o[1] = s.wo.y; o[2] = s.wo.z; o[3] = s.pdf; o[4] = s.weight.x; o[5] = s.weight.y; o[6] = s.weight.z; o[7] = (float)s.lobe; o[8] = s.lobeP; o[9] = v ? 1.f : 0.f; } } break;
    case 4: { const uint* p = reinterpret_cast<const uint*>(in) + 3 * i;                                   // camera ray: px, py, sampleIndex
        PathState ps = k.generate(p[0], p[1], p[2]);
        out[6 * i] = ps.origin.x; out[6 * i + 1] = ps.origin.y; out[6 * i + 2] = ps.origin.z; out[6 * i + 3] = ps.dir.x; out[6 * i + 4] = ps.dir.y; out[6 * i + 5] = ps.dir.z; } break;
    // leaf functions pinned to the reference text (tests/golden/refpin_hlsl_golden.npz): (fn, 8 args) -> 4 results
    case 5: { const float* a = in + 9 * i + 1; int fn = (int)in[9 * i]; float* o = out + 4 * i; o[0] = o[1] = o[2] = o[3] = 0.f;
        switch (fn) {
        case 0: o[0] = evalFresnelSchlick(a[0], a[1], a[2]); break;
        case 1: { float3 r = evalFresnelSchlick(make_float3(a[0], a[1], a[2]), a[3], a[4]); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
        case 2: { float ct = 0.f; o[0] = evalFresnelDielectric(a[0], a[1], ct); o[1] = ct; } break;
        case 3: o[0] = evalNdfGGX(a[0], a[1]); break;
        case 4: o[0] = evalPdfGGX_BVNDF(a[0], make_float3(a[1], a[2], a[3]), make_float3(a[4], a[5], a[6])); break;
        case 5: { float3 r = sampleGGX_BVNDF(a[0], make_float3(a[1], a[2], a[3]), make_float2(a[4], a[5])); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
        case 6: o[0] = evalLambdaGGX(a[0], a[1]); break;
        case 7: o[0] = evalMaskingSmithGGXCorrelated(a[0], a[1], a[2]); break;
        case 8: { float2 r = ndir_to_oct_equal_area_unorm(make_float3(a[0], a[1], a[2])); o[0] = r.x; o[1] = r.y; } break;
        case 9: { float3 r = oct_to_ndir_equal_area_unorm(make_float2(a[0], a[1])); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
        case 10: { float2 r = sample_disk(make_float2(a[0], a[1])); o[0] = r.x; o[1] = r.y; } break;
        case 11: { float2 r = sample_disk_concentric(make_float2(a[0], a[1])); o[0] = r.x; o[1] = r.y; } break;
        case 12: { float pdf = 0.f; float3 r = sample_cosine_hemisphere_concentric(make_float2(a[0], a[1]), pdf); o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = pdf; } break;
        case 13: { float3 r = perp_stark(make_float3(a[0], a[1], a[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
        case 14: { float3 r = ComputeRayOrigin(make_float3(a[0], a[1], a[2]), make_float3(a[3], a[4], a[5])); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
        case 15: o[0] = FastSqrt(a[0]); break;
        case 16: o[0] = FastACos(a[0]); break;
        case 17: o[0] = ComputeRayConeSpreadAngleExpansionByScatterPDF(a[0], a[1]); break;
        case 18: o[0] = ComputeNewScatterFireflyFilterK<LPOps<false>>(a[0], a[1], a[2]); break;
        case 19: { float3 r = FireflyFilter<LPOps<false>>(make_float3(a[0], a[1], a[2]), a[3], a[4]); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
        case 20: o[0] = FireflyFilterShort(a[0], a[1], a[2]); break;
        case 21: o[0] = ComputeLowGrazingAngleFalloff(make_float3(a[0], a[1], a[2]), make_float3(a[3], a[4], a[5]), a[6], a[7]); break;
        default: break;
        } } break;
    case 6: { const uint* a = reinterpret_cast<const uint*>(in) + 19 * i + 1; const uint lk = reinterpret_cast<const uint*>(in)[19 * i]; uint* o = reinterpret_cast<uint*>(out) + 12 * i;      // polymorphic lights: (kind, 18 words) -> 12 words
        for (int q = 0; q < 12; q++) o[q] = 0u;
        const float3x4 I = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
        auto info = [&](const uint* w) { PolymorphicLightInfoFull li; __builtin_memset(&li, 0, sizeof(li));
            li.Base.Center = make_float3(asfloat(w[0]), asfloat(w[1]), asfloat(w[2])); li.Base.ColorTypeAndFlags = w[3]; li.Base.Direction1 = w[4]; li.Base.Direction2 = w[5]; li.Base.Scalars = w[6]; li.Base.LogRadiance = w[7];
            li.Extended.IesProfileIndex = w[8]; li.Extended.PrimaryAxis = w[9]; li.Extended.CosConeAngleAndSoftness = w[10]; li.Extended.UniqueID = w[11]; return li; };
        if (lk == 0u) { PolymorphicLightInfo b; __builtin_memset(&b, 0, sizeof(b)); PackLightColor(make_float3(asfloat(a[0]), asfloat(a[1]), asfloat(a[2])), b); float3 c = UnpackLightColor(b);
            o[0] = b.ColorTypeAndFlags; o[1] = b.LogRadiance; o[2] = asuint(c.x); o[3] = asuint(c.y); o[4] = asuint(c.z); }
        else if (lk == 1u) { TriangleLight t; t.base = make_float3(asfloat(a[0]), asfloat(a[1]), asfloat(a[2])); t.edge1 = make_float3(asfloat(a[3]), asfloat(a[4]), asfloat(a[5])); t.edge2 = make_float3(asfloat(a[6]), asfloat(a[7]), asfloat(a[8]));
            t.radiance = make_float3(asfloat(a[9]), asfloat(a[10]), asfloat(a[11])); t.normal = make_float3(0.f); t.surfaceArea = 0;
            PolymorphicLightInfoFull li = t.Store(7u);
            o[0] = asuint(li.Base.Center.x); o[1] = asuint(li.Base.Center.y); o[2] = asuint(li.Base.Center.z); o[3] = li.Base.ColorTypeAndFlags; o[4] = li.Base.Direction1; o[5] = li.Base.Direction2; o[6] = li.Base.Scalars; o[7] = li.Base.LogRadiance;
            o[8] = li.Extended.IesProfileIndex; o[9] = li.Extended.PrimaryAxis; o[10] = li.Extended.CosConeAngleAndSoftness; o[11] = li.Extended.UniqueID; }
        else if (lk == 2u) { PolymorphicLightInfoFull li = info(a);
            PolymorphicLightSample sm = PolymorphicLight_CalcSample(li, make_float2(asfloat(a[12]), asfloat(a[13])), make_float3(asfloat(a[14]), asfloat(a[15]), asfloat(a[16])), I);
            o[0] = asuint(sm.Position.x); o[1] = asuint(sm.Position.y); o[2] = asuint(sm.Position.z); o[3] = asuint(sm.Normal.x); o[4] = asuint(sm.Normal.y); o[5] = asuint(sm.Normal.z);
            o[6] = asuint(sm.Radiance.x); o[7] = asuint(sm.Radiance.y); o[8] = asuint(sm.Radiance.z); o[9] = asuint(sm.SolidAnglePdf); o[10] = sm.LightSampleableByBSDF ? 1u : 0u; o[11] = asuint(PolymorphicLight_GetPower(li)); }
        else if (lk == 3u) { TriangleLight t = TriangleLight::Create(info(a));
            o[0] = asuint(t.CalcSolidAnglePdfForMIS(make_float3(asfloat(a[12]), asfloat(a[13]), asfloat(a[14])), make_float3(asfloat(a[15]), asfloat(a[16]), asfloat(a[17])))); }
        else { uint pk = NDirToOctUnorm32(make_float3(asfloat(a[0]), asfloat(a[1]), asfloat(a[2]))); float3 d = OctToNDirUnorm32(pk); o[0] = pk; o[1] = asuint(d.x); o[2] = asuint(d.y); o[3] = asuint(d.z); }
        } break;
    // loadSurface: (prim bits, u, v, dir.xyz, coneWidth, coneSpread) -> 45 words (layout of the oracle's surface probe)
    case 8: { const float* a = in + 8 * i; uint* o = reinterpret_cast<uint*>(out) + 45 * i;
        RayCone rc = RayCone::make(a[6], a[7]);
        auto emit = [&](const SurfaceData& q) {
            const ShadingData& s = q.shadingData; const StandardBSDFData& b = q.bsdf.data;
            auto put3 = [&](float3 v) { *o++ = asuint(v.x); *o++ = asuint(v.y); *o++ = asuint(v.z); };
            put3(s.posW); put3(s.faceNCorrected); put3(s.V); put3(s.N); put3(s.T); put3(s.B); put3(s.vertexN);
            *o++ = s.frontFacing ? 1u : 0u; *o++ = s.mtl.packedData; *o++ = s.materialID; *o++ = asuint(s.IoR); *o++ = asuint(s.shadowNoLFadeout); put3(s.emission);
            put3(b.diffuse); *o++ = asuint(b.roughness); put3(b.specular); *o++ = asuint(b.metallic); put3(b.transmission);
            *o++ = asuint(b.diffuseTransmission); *o++ = asuint(b.specularTransmission); *o++ = asuint(b.eta); *o++ = asuint(q.interiorIoR); *o++ = q.neeTriangleLightIndex; };
        if (k.S.useFp16Types) { PathKernelContextT<true> k16; __builtin_memcpy(&k16, &k, sizeof(k16)); emit(k16.loadSurface(asuint(a[0]), a[1], a[2], make_float3(a[3], a[4], a[5]), rc)); }
        else emit(k.loadSurface(asuint(a[0]), a[1], a[2], make_float3(a[3], a[4], a[5]), rc));
        } break;
    // the half-typed operators of the lp16 build: (op, a, b, c) -> result
    case 7: { const float* a = in + 4 * i; const int op = (int)a[0]; typedef LPOps<true> H; float r = 0.f;
        switch (op) { case 0: r = H::r(a[1]); break; case 1: r = H::add(H::r(a[1]), H::r(a[2])); break; case 2: r = H::sub(H::r(a[1]), H::r(a[2])); break; case 3: r = H::mul(H::r(a[1]), H::r(a[2])); break;
                      case 4: r = H::div(H::r(a[1]), H::r(a[2])); break; case 5: r = H::lerp(H::r(a[1]), H::r(a[2]), H::r(a[3])); break;
                      case 7: r = H::r(a[1] * a[2]); break; case 8: r = H::r(H::r(a[1]) * a[2]); break; case 9: r = H::r(a[1] + a[2]); break; case 10: r = H::r(a[1] / a[2]); break;      // lpfloat(float expression)
                      default: r = H::average3(make_float3(H::r(a[1]), H::r(a[2]), H::r(a[3]))); break; }
        out[i] = r; } break;
    // the traversal's alpha test: (primitive, u, v) -> (scatter ray accepts, visibility ray accepts)
    case 10: { const uint* a = reinterpret_cast<const uint*>(in) + 3 * i; uint* o = reinterpret_cast<uint*>(out) + 2 * i;
        // AlphaTestImpl / Bridge::AlphaTest / AlphaTestVisibilityRay (BridgeDonut:929-989) as the leaf block applies them
        const uint slot = k.sc.primToSlot[a[0]]; const TriRecord tr = k.sc.tris[slot];
        const bool solid = !(tr.flags & 1u) || alpha_test_slot(k.sc, slot, asfloat(a[1]), asfloat(a[2]));
        o[0] = solid ? 1u : 0u; o[1] = (!(tr.flags & 1u) || (!(tr.flags & 2u) && solid)) ? 1u : 0u; } break;
    // EnvMap::EvalLocal on the baked cube: (localDir.xyz, lod)
    case 9: { const float* a = in + 4 * i; float* o = out + 3 * i;
        float3 r = k.sc.envEnabled ? env_eval_local(k.sc, make_float3(a[0], a[1], a[2]), a[3]) : make_float3(0.f);
        o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
    // the texture samplers: (mode, texture, u, v, four mode words) -> float4 (include/mi355pt_testhooks.h; pt_probe has checked texture and mip against the scene)
    case 11: { const uint* a = reinterpret_cast<const uint*>(in) + 8 * i; const float2 uv = make_float2(asfloat(a[2]), asfloat(a[3])); float4 r;
        if (a[0] == 0u) r = k.sampleTexture(a[1], asfloat(a[4]), uv);                                                   // the material path: packed texture word, lambdaNoDims
        else if (a[0] == 1u) r = sample_bilinear(k.sc, k.sc.textures[a[1]], a[4], uv);                                   // one integer mip
        else r = sample_grad_anisotropic(k.sc, k.sc.textures[a[1]], uv, make_float2(asfloat(a[4]), asfloat(a[5])), make_float2(asfloat(a[6]), asfloat(a[7])));
        out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w; } break;
    // stochastic texture filtering (pt_stf.h; include/mi355pt_testhooks.h kind 12): twelve words in, eight out; pt_probe has checked mode, texture and filter against the scene
    case 12: { const uint* a = reinterpret_cast<const uint*>(in) + 12 * i; uint* o = reinterpret_cast<uint*>(out) + 8 * i;
        for (int q = 0; q < 8; q++) o[q] = 0u;
        if (a[0] == 0u) {      // the lookup of a context with filter a[5], at the four numbers of words 6-9: the texel, then the level and the position it was taken from
            const uint textureIndex = a[1] & 0xFFFFu, baseLOD = a[1] >> 24, mipLevels = (a[1] >> 16) & 0xFFu;
            float lambda = 0.5f * (float)baseLOD + asfloat(a[4]);      // sampleTexture's two lines (pt_path.h)
            lambda = fminf_(lambda, fmaxf_((float)mipLevels - 5.0f, 0.0f));
            const TexInfo& t = k.sc.textures[textureIndex];
            const StfPick p = stf_pick_filter((int)a[5], t, make_float2(asfloat(a[2]), asfloat(a[3])), lambda, make_float4(asfloat(a[6]), asfloat(a[7]), asfloat(a[8]), asfloat(a[9])));
            const float4 r = stf_texel(k.sc, t, p);
            o[0] = asuint(r.x); o[1] = asuint(r.y); o[2] = asuint(r.z); o[3] = asuint(r.w); o[4] = p.mip; o[5] = (uint)p.x; o[6] = (uint)p.y;
        } else { const float4 u = stf_draw(a[6], a[7], a[8]); o[0] = asuint(u.x); o[1] = asuint(u.y); o[2] = asuint(u.z); o[3] = asuint(u.w); }      // the four numbers loadSurface draws for (packed pixel, vertex, sample)
        } break;
    default: break;
    }
}
static void launch_probe(const PathKernelContext& k, int kind, const void* dIn, void* dOut, uint n, hipStream_t st) {
    hipLaunchKernelGGL(k_probe, dim3((n + 63) / 64), dim3(64), 0, st, k, kind, (const float*)dIn, (float*)dOut, n);
}
// pt_trace_route's packet route: k_extend_first_packets for rays that are STORED (pool.s0 / s1, as k_generate writes them) instead of formed from a camera — the same
// traverse8_packets, the same commit, the same leftover list; *committed counts the calls of commit. The rays the packets leave over are the caller's to trace (launch_extend
// with the list as its queue: what k_extend_first_listed is to k_extend_first).
__global__ void __launch_bounds__(T8_BLOCK, T8_EXTEND_MIN_BLOCKS) k_route_packets(DeviceScene sc, PathPool pool, const uint* __restrict__ countPtr, WaveCounters* wc, FirstPackets pk, uint* committed) {
    __shared__ uint2 stack[(T8_BLOCK / 64u) * T8_PACKET_STACK];
    __shared__ float2 mineUV[T8_BLOCK];
    traverse8_packets(sc, *countPtr, stack, mineUV, [&](uint i, float3& o, float3& d) { t8_stored_ray(pool, i, o, d); }, [&](uint p, const HitInfo& h) { t8_store_hit(pool, p, h); atomicAdd(committed, 1u); }, pk, &wc->overflow);
}
// ... and k_extend_first_packets64 for stored rays (pk.wide), with or without the interval test (pk.precull)
template <bool PRECULL>
__global__ void __launch_bounds__(T8_BLOCK, T8_PACKET64_MIN_BLOCKS) k_route_packets64(DeviceScene sc, PathPool pool, const uint* __restrict__ countPtr, WaveCounters* wc, FirstPackets pk, uint* committed) {
    __shared__ uint2 stack[(T8_BLOCK / 64u) * T8_PACKET_STACK];
    __shared__ __attribute__((aligned(16))) float interval[PRECULL ? (T8_BLOCK / 64u) * T8_PACKET_INTERVAL_WORDS : 4u];
    traverse8_packets64<PRECULL>(sc, *countPtr, stack, interval, [&](uint i, float3& o, float3& d) { t8_stored_ray(pool, i, o, d); }, [&](uint p, const HitInfo& h) { t8_store_hit(pool, p, h); atomicAdd(committed, 1u); }, pk, &wc->overflow);
}
// the `count` rays stored in pool.s0 / s1 as packets, hits to pool.hit; *committed counts the rays the packets reported themselves
static void launch_route_packets(const DeviceScene& sc, PathPool pool, const uint* countPtr, uint count, WaveCounters* wc, FirstPackets pk, uint* committed, uint maxBlocks, hipStream_t st) {
    const uint gp = t8_packet_grid(count, pk.wide != 0u, maxBlocks);
    if (pk.wide && pk.precull) hipLaunchKernelGGL(k_route_packets64<true>, dim3(gp), dim3(T8_BLOCK), 0, st, sc, pool, countPtr, wc, pk, committed);
    else if (pk.wide) hipLaunchKernelGGL(k_route_packets64<false>, dim3(gp), dim3(T8_BLOCK), 0, st, sc, pool, countPtr, wc, pk, committed);
    else hipLaunchKernelGGL(k_route_packets, dim3(gp), dim3(T8_BLOCK), 0, st, sc, pool, countPtr, wc, pk, committed);
}
} // namespace ptk

extern "C" {
int32_t pt_probe(pt_context* c, int32_t kind, const void* in, size_t inBytes, void* out, size_t outBytes, uint32_t n) {
    if (!c || !in || !out || !n) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bad argument");
    (void)hipSetDevice(c->device);
    // the surface, environment and alpha-test probes read the scene
    if (kind == 8 || kind == 9 || kind == 10 || kind == 11 || kind == 12) { int r = prepare(c); if (r != PT_OK) return r; }
    if (kind == 12) {      // the stochastic-filter probe indexes the texture table with what its rows say, and knows three filters
        if (inBytes < (size_t)n * 48u || outBytes < (size_t)n * 32u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "stochastic texture probe: 12 words in and 8 words out per row");
        const uint32_t* a = (const uint32_t*)in;
        for (uint32_t i = 0; i < n; i++, a += 12)
            if (a[0] > 1u || (a[0] == 0u && ((a[1] & 0xFFFFu) >= c->textures.size() || a[5] > PT_STF_FILTER_CUBIC))) return fail(c, PT_ERROR_INVALID_ARGUMENT, "stochastic texture probe: mode, texture or filter out of range");
    }
    if (kind == 11) {      // the texture probe indexes the texture table and a texture's mip offsets with what its rows say: hold both to the scene here, the kernel does not
        if (inBytes < (size_t)n * 32u || outBytes < (size_t)n * 16u) return fail(c, PT_ERROR_INVALID_ARGUMENT, "texture probe: 8 words in and 4 floats out per row");
        const uint32_t* a = (const uint32_t*)in;
        for (uint32_t i = 0; i < n; i++, a += 8) {
            const uint32_t tex = a[0] == 0u ? (a[1] & 0xFFFFu) : a[1];
            if (a[0] > 2u || tex >= c->textures.size() || (a[0] == 1u && a[4] >= c->textures[tex].mipLevels)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "texture probe: mode, texture or mip out of range");
        }
    }
    DevBuf<unsigned char> di, dout;
    PT_CHECK_HIP(c, di.upload((const unsigned char*)in, inBytes, c->stream)); PT_CHECK_HIP(c, dout.resize(outBytes));
    PathKernelContext k; k.sc = c->dsc; k.S = c->S; k.cam = c->cam;
    launch_probe(k, kind, di.p, dout.p, n, c->stream);
    PT_CHECK_HIP(c, hipMemcpyAsync(out, dout.p, outBytes, hipMemcpyDeviceToHost, c->stream));
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    PT_CHECK_HIP(c, hipGetLastError());
    di.free(); dout.free();
    return PT_OK;
}
int32_t pt_get_inert_terminal(pt_context* c, uint32_t* numPrims, uint32_t* words, uint32_t capacityWords, uint64_t* lastDropped) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    if (numPrims) *numPrims = c->numTris;
    if (lastDropped) *lastDropped = c->droppedTerminal;
    if (words && c->numTris) {
        if (capacityWords < inert_words(c->numTris)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "inert-terminal table: (numPrims + 15) / 16 words");
        PT_CHECK_HIP(c, hipMemcpy(words, c->dInertBits.p, 4 * (size_t)inert_words(c->numTris), hipMemcpyDeviceToHost));
    }
    return PT_OK;
}
// the wide tree as the traversal reads it: nodes8, triSorted, the scene bounds the pads were formed from and the level table the refit walks. Nothing else: after a fast refit
// (pt_build.h bvh2Stale) the BVH2 nodes, triWorld and the range tables hold an older pose
int32_t pt_get_bvh8(pt_context* c, uint32_t* numNodes, void* nodes, uint32_t capacityNodes, uint32_t* numTris, void* tris, uint32_t capacityTris, float* bounds,
                    uint32_t* collapseLevels, uint32_t* wideLevelStart, uint32_t capacityLevels) {
    if (!c) return PT_ERROR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    const uint32_t nt = c->numTris, nn = nt ? c->bvh.numNodes8 : 0u, nl = nt ? c->bvh.collapseLevels : 0u, stored = (nl < BVH_MAX_WIDE_LEVELS ? nl : BVH_MAX_WIDE_LEVELS) + 1u;
    if (numNodes) *numNodes = nn; if (numTris) *numTris = nt; if (collapseLevels) *collapseLevels = nl;
    if ((nodes && capacityNodes < nn) || (tris && capacityTris < nt) || (wideLevelStart && capacityLevels < stored)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_get_bvh8: a buffer is smaller than its count");
    PT_CHECK_HIP(c, hipStreamSynchronize(c->stream));
    if (nodes && nn) PT_CHECK_HIP(c, hipMemcpy(nodes, c->bvh.nodes8, sizeof(Bvh8Node) * (size_t)nn, hipMemcpyDeviceToHost));
    if (tris && nt) PT_CHECK_HIP(c, hipMemcpy(tris, c->bvh.triSorted, sizeof(TriRecord) * (size_t)nt, hipMemcpyDeviceToHost));
    if (bounds) {
        uint32_t enc[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        if (nt) PT_CHECK_HIP(c, hipMemcpy(enc, c->bvh.sceneBounds, sizeof(enc), hipMemcpyDeviceToHost));
        for (int k = 0; k < 6; k++) { const uint32_t b = nt ? ((enc[k] & 0x80000000u) ? (enc[k] & 0x7FFFFFFFu) : ~enc[k]) : 0u; memcpy(bounds + k, &b, 4); }      // (pt_build.hip dec_float)
    }
    if (wideLevelStart) for (uint32_t l = 0; l < stored; l++) wideLevelStart[l] = nt ? c->bvh.wideLevelStart[l] : 0u;
    return PT_OK;
}
// pt_trace_route: the caller's rays through launch_extend / launch_shadow / the packet launch, on buffers of the call's own (freed whichever way it returns)
namespace {
struct RouteBuffers {
    DevBuf<ptk::uint4> s0, s1, s2, hit; DevBuf<ptk::float4> q0, q1, q2; DevBuf<uint> queue, words, resolveList, leftover;
    DevBuf<TravTask> taskQ; DevBuf<unsigned long long> bestKey; DevBuf<WaveCounters> wc;
    ~RouteBuffers() { s0.free(); s1.free(); s2.free(); hit.free(); q0.free(); q1.free(); q2.free(); queue.free(); words.free(); resolveList.free(); leftover.free(); taskQ.free(); bestKey.free(); wc.free(); }
};
// the call's counter words: a traversal launch's TRAV_COUNTERS from word 0, the leftover count at PASS_LEFTOVER (as in a pass's block), then the launch's ray count and the packets' commits
const uint ROUTE_WORD_COUNT = PASS_COUNTERS, ROUTE_WORD_COMMITTED = PASS_COUNTERS + 1u, ROUTE_WORDS = PASS_COUNTERS + 2u;
}
int32_t pt_trace_route(pt_context* c, int32_t route, const float* rays, uint32_t n, const PtRouteOptions* options, void* out, PtRouteStats* stats) {
    if (!c || !rays || !n || !out) return fail(c, PT_ERROR_INVALID_ARGUMENT, "bad argument");
    if (route != PT_ROUTE_EXTEND && route != PT_ROUTE_EXTEND_RANGED && route != PT_ROUTE_SHADOW && route != PT_ROUTE_PACKETS) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_trace_route: unknown route " + std::to_string(route));
    const bool fixed = route == PT_ROUTE_EXTEND || route == PT_ROUTE_PACKETS;
    for (uint32_t i = 0; i < n; i++) {      // (trace_probe's rule first: the traversal orders children by the bit pattern of an entry distance >= +0)
        const float tmin = rays[8 * (size_t)i + 3], tmax = rays[8 * (size_t)i + 7];
        if (!(tmin >= 0.0f) || std::signbit(tmin)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_trace_route: ray " + std::to_string(i) + " has tmin < 0 (or -0, or NaN); tmin must be >= +0");
        if (fixed && (tmin != 0.0f || tmax != kMaxRayTravel)) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_trace_route: ray " + std::to_string(i) + " of a fixed-interval route must have tmin = 0 and tmax = 1e15f");
        if (route == PT_ROUTE_SHADOW && tmin != 0.0f) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_trace_route: ray " + std::to_string(i) + " of the shadow route must have tmin = 0 (a shadow-queue entry carries no lower bound)");
    }
    const PtRouteOptions opt = options ? *options : PtRouteOptions{0u, 0u, 0u, 0u};
    if (opt.taskCap > TASK_QUEUE_CAPACITY) return fail(c, PT_ERROR_INVALID_ARGUMENT, "pt_trace_route: taskCap above TASK_QUEUE_CAPACITY");
    (void)hipSetDevice(c->device);
    int r = prepare(c); if (r != PT_OK) return r;
    const hipStream_t st = c->stream;
    RouteBuffers B;
    std::vector<uint> words(ROUTE_WORDS, 0u); words[ROUTE_WORD_COUNT] = n;
    PT_CHECK_HIP(c, B.words.upload(words, st));
    PT_CHECK_HIP(c, B.wc.resize(1)); PT_CHECK_HIP(c, hipMemsetAsync(B.wc.p, 0, sizeof(WaveCounters), st));      // (the overflow word with it)
    TravAux aux;
    aux.taskCap = opt.taskCap ? opt.taskCap : TASK_QUEUE_CAPACITY; aux.maxBlocks = opt.maxBlocks;
    PT_CHECK_HIP(c, B.taskQ.resize(2 * (size_t)aux.taskCap)); PT_CHECK_HIP(c, B.bestKey.resize(n)); PT_CHECK_HIP(c, B.resolveList.resize(n));
    // (zeroed: an entry that no launch wrote names ray 0 and the root. The task rounds do not read such entries — t8_extend_tasks_body — and a call on a machine that
    // others share must not depend on that)
    PT_CHECK_HIP(c, hipMemsetAsync(B.taskQ.p, 0, sizeof(TravTask) * 2 * (size_t)aux.taskCap, st));
    PT_CHECK_HIP(c, hipMemsetAsync(B.bestKey.p, 0xFF, sizeof(unsigned long long) * (size_t)n, st)); PT_CHECK_HIP(c, hipMemsetAsync(B.resolveList.p, 0, 4 * (size_t)n, st));
    aux.taskQ[0] = B.taskQ.p; aux.taskQ[1] = B.taskQ.p + aux.taskCap; aux.counts = B.words.p; aux.bestKey = B.bestKey.p; aux.resolveList = B.resolveList.p; aux.primToSlot = c->bvh.primToSlot;
    const uint* countPtr = B.words.p + ROUTE_WORD_COUNT;
    std::vector<ptk::float4> hostQ2;
    if (route == PT_ROUTE_SHADOW) {
        std::vector<ptk::float4> q0(n), q1(n);
        for (uint32_t i = 0; i < n; i++) {
            const float* y = rays + 8 * (size_t)i; float tag; memcpy(&tag, &i, 4);
            q0[i] = ptk::make_float4(y[0], y[1], y[2], y[7]); q1[i] = ptk::make_float4(y[4], y[5], y[6], tag);
        }
        PT_CHECK_HIP(c, B.q0.upload(q0, st)); PT_CHECK_HIP(c, B.q1.upload(q1, st));
        PT_CHECK_HIP(c, B.q2.resize(n)); PT_CHECK_HIP(c, hipMemsetAsync(B.q2.p, 0, sizeof(ptk::float4) * (size_t)n, st));
        PT_CHECK_HIP(c, B.s2.resize(n)); PT_CHECK_HIP(c, hipMemsetAsync(B.s2.p, 0, sizeof(ptk::uint4) * (size_t)n, st));      // (entry i names path i: what k_resolve_nee folds the marks into)
        PT_CHECK_HIP(c, hipStreamSynchronize(st));      // (the uploads read host vectors of this block)
        PathPool pool{}; pool.s2 = B.s2.p;
        const ShadowQueue sq{B.q0.p, B.q1.p, B.q2.p, 1u, nullptr, nullptr, nullptr, 0u, 0u, 0u};
        launch_shadow(c->dsc, pool, sq, countPtr, n, B.wc.p, false, aux, st);
        hostQ2.resize(n);
        PT_CHECK_HIP(c, hipMemcpyAsync(hostQ2.data(), B.q2.p, sizeof(ptk::float4) * (size_t)n, hipMemcpyDeviceToHost, st));
    } else {
        std::vector<ptk::uint4> s0(n), s1(n), hit(n);
        std::vector<uint> queue(n);
        for (uint32_t i = 0; i < n; i++) {
            uint w[8]; memcpy(w, rays + 8 * (size_t)i, 32);
            s0[i] = ptk::make_uint4(w[0], w[1], w[2], i); s1[i] = ptk::make_uint4(w[4], w[5], w[6], 0u);      // origin | id, direction | scene length 0
            hit[i] = route == PT_ROUTE_EXTEND_RANGED ? ptk::make_uint4(w[3], w[7], 0u, 0u) : ptk::make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);      // (a record no launch writes stays recognisable)
            queue[i] = i;
        }
        PT_CHECK_HIP(c, B.s0.upload(s0, st)); PT_CHECK_HIP(c, B.s1.upload(s1, st)); PT_CHECK_HIP(c, B.hit.upload(hit, st)); PT_CHECK_HIP(c, B.queue.upload(queue, st));
        PT_CHECK_HIP(c, hipStreamSynchronize(st));
        PathPool pool{}; pool.s0 = B.s0.p; pool.s1 = B.s1.p; pool.hit = B.hit.p;      // (home == nullptr: every array is indexed by the queue's entries)
        if (route == PT_ROUTE_PACKETS) {
            PT_CHECK_HIP(c, B.leftover.resize(n));
            const FirstPackets pk = first_packets(c, B.leftover.p, B.words.p + PASS_LEFTOVER, n, opt.stepCap, opt.stackBound);      // (the traverser of the context's mode)
            launch_route_packets(c->dsc, pool, countPtr, n, B.wc.p, pk, B.words.p + ROUTE_WORD_COMMITTED, aux.maxBlocks, st);
            launch_extend(c->dsc, pool, pk.leftover, pk.leftoverCount, n, B.wc.p, false, aux, st);      // (n: the host's bound of the list's length, as launch_extend_first sizes k_extend_first_listed)
        } else launch_extend(c->dsc, pool, B.queue.p, countPtr, n, B.wc.p, false, aux, st, route == PT_ROUTE_EXTEND_RANGED);
        PT_CHECK_HIP(c, hipMemcpyAsync(out, B.hit.p, sizeof(ptk::uint4) * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    uint overflow = 0u;
    PT_CHECK_HIP(c, hipMemcpyAsync(words.data(), B.words.p, 4 * (size_t)ROUTE_WORDS, hipMemcpyDeviceToHost, st));
    PT_CHECK_HIP(c, hipMemcpyAsync(&overflow, &B.wc.p->overflow, 4, hipMemcpyDeviceToHost, st));
    PT_CHECK_HIP(c, hipStreamSynchronize(st));
    PT_CHECK_HIP(c, hipGetLastError());
    if (route == PT_ROUTE_SHADOW) for (uint32_t i = 0; i < n; i++) ((uint32_t*)out)[i] = hostQ2[i].w == 1.0f ? 1u : 0u;
    if (stats) {
        stats->splitRays = words[TRAV_RESOLVE]; for (int q = 0; q < 4; q++) stats->taskCounts[q] = words[q];
        stats->packetRays = words[ROUTE_WORD_COMMITTED]; stats->leftoverRays = words[PASS_LEFTOVER]; stats->overflow = overflow;
    }
    if (overflow) return fail(c, PT_ERROR_HIP, "pt_trace_route: BVH8 traversal: stack tail, straggler task queue or leftover list overflow (word " + std::to_string(overflow) + ")");
    return PT_OK;
}
} // extern "C"

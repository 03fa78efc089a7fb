// mi355pt — the packet's interval test of a BVH8 child (traverse8_packets64, pt_traverse8k.h): one conservative slab test of a child's box against ALL rays of a packet at once,
// which decides whether any ray's own test (t8_slab + T8_HIT, pt_traverse8.h) has to run for that child at all. Plain C++ without a dependency: the device includes it, and
// tests/packet_precull_check.cpp holds it on the host against a restatement of t8_slab.
//
// A ray's interval on an axis is [(pNear - o) * i, (pFar - o) * i]: i = ray_safe_rcp of the direction's component (never 0, never inf), pNear the plane the ray meets first
// (lo where i > 0, hi where i < 0). The packet knows, per axis, the interval [oMin, oMax] of its rays' origins and [iLo, iHi] of their reciprocals, and that the reciprocals have
// ONE sign on every axis (otherwise there is no test: every child is kept). fp32 subtraction and multiplication, rounded to nearest, are monotone in each operand, and over an
// interval of i that does not contain 0 the extremes of d * i lie at its endpoints. So
//   i > 0:  (pNear - o) * i >= (pNear - oMax) * i >= min((pNear - oMax) * iLo, (pNear - oMax) * iHi),   (pFar - o) * i <= max((pFar - oMin) * iLo, (pFar - oMin) * iHi)
//   i < 0:  a product with i falls as the distance grows, so the two origins swap: pNear - oMin below, pFar - oMax above.
// oN / oF are the origin to subtract from the near / far plane, chosen once per packet by the axis' sign. With L = the largest lower bound (and tmin), U = the smallest upper
// bound (and the packet's largest best t): L <= tn and tf <= U for every ray, the product with T8_HIT's factor (positive) keeps the order, and L > U * 1.0000012f means
// tn > tf * 1.0000012f for every ray: no ray's T8_HIT is true. A NaN (a plane that is not finite) compares false: the child is kept.
#pragma once
#include <math.h>
#ifdef __HIP__
#pragma clang force_cuda_host_device begin
#endif

// the packet's twelve floats, in the order the device keeps them in LDS (three 16-byte reads): x, y, z of oN, oF, iLo, iHi
struct T8PacketInterval { float oNx, oNy, oNz, oFx, oFy, oFz, iLox, iLoy, iLoz, iHix, iHiy, iHiz; };

// one axis' bounds are usable: the reciprocals have one sign, and nothing is NaN or infinite
static inline bool t8_packet_axis_definite(float oMin, float oMax, float iLo, float iHi) {
    return (iHi < 0.0f || iLo > 0.0f) && (oMax - oMin) < INFINITY && (iHi - iLo) < INFINITY;      // (inf - inf, NaN - x: NaN, which compares false)
}
// the packet's interval from the componentwise extremes over its rays; false: the reciprocals straddle zero on an axis, or a value is not finite — keep every child
static inline bool t8_packet_interval(float oMinX, float oMinY, float oMinZ, float oMaxX, float oMaxY, float oMaxZ, float iLoX, float iLoY, float iLoZ, float iHiX, float iHiY, float iHiZ,
                                      T8PacketInterval& pi) {
    const bool negX = iHiX < 0.0f, negY = iHiY < 0.0f, negZ = iHiZ < 0.0f;
    pi.oNx = negX ? oMinX : oMaxX; pi.oNy = negY ? oMinY : oMaxY; pi.oNz = negZ ? oMinZ : oMaxZ;
    pi.oFx = negX ? oMaxX : oMinX; pi.oFy = negY ? oMaxY : oMinY; pi.oFz = negZ ? oMaxZ : oMinZ;
    pi.iLox = iLoX; pi.iLoy = iLoY; pi.iLoz = iLoZ; pi.iHix = iHiX; pi.iHiy = iHiY; pi.iHiz = iHiZ;
    return t8_packet_axis_definite(oMinX, oMaxX, iLoX, iHiX) && t8_packet_axis_definite(oMinY, oMaxY, iLoY, iHiY) && t8_packet_axis_definite(oMinZ, oMaxZ, iLoZ, iHiZ);
}
// pN* / pF*: the child's near and far plane on each axis, as t8_slab decodes them with the packet's selectors; tmin / maxBest: the rays' tmin, the packet's largest best t
static inline bool t8_packet_keeps(float pNx, float pFx, float pNy, float pFy, float pNz, float pFz, const T8PacketInterval& pi, float tmin, float maxBest) {
    const float dNx = pNx - pi.oNx, dNy = pNy - pi.oNy, dNz = pNz - pi.oNz, dFx = pFx - pi.oFx, dFy = pFy - pi.oFy, dFz = pFz - pi.oFz;
    const float lx = fminf(dNx * pi.iLox, dNx * pi.iHix), ly = fminf(dNy * pi.iLoy, dNy * pi.iHiy), lz = fminf(dNz * pi.iLoz, dNz * pi.iHiz);
    const float ux = fmaxf(dFx * pi.iLox, dFx * pi.iHix), uy = fmaxf(dFy * pi.iLoy, dFy * pi.iHiy), uz = fmaxf(dFz * pi.iLoz, dFz * pi.iHiz);
    const float L = fmaxf(fmaxf(lx, ly), fmaxf(lz, tmin));
    const float U = fminf(fminf(ux, uy), fminf(uz, maxBest));
    return !(L > U * 1.0000012f);
}

#ifdef __HIP__
#pragma clang force_cuda_host_device end
#endif

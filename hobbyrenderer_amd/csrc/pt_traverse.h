// pt_traverse.h -- rays and hits, the watertight triangle test, the BVH fetch policies, inner_step, the walks over the flat and the
// two-level structure, and the fetch policy of a scene by key (GlobalBvhOf).
#pragma once

#include "pt_scene_records.h"
#include "pt_phase.h"
#include "pt_vec.h"

namespace hrt {

// ------------------------------------------------------------------ rays and hits
struct Ray { f3 o, d; float tmin, tmax; };
struct Hit { float t; uint32_t inst, prim; float u, v; uint32_t opaque; uint32_t tri; bool valid; };
struct HitKey { float t; uint32_t inst, prim; bool have; };

struct RayShear { int kx, ky, kz; float Sx, Sy, Sz; };

HRT_DEV RayShear make_shear(f3 d)
{
    RayShear s;
    int kz = 0;
    if (hrt_abs(d.y) > hrt_abs(comp(d, kz))) kz = 1;
    if (hrt_abs(d.z) > hrt_abs(comp(d, kz))) kz = 2;
    int kx = (kz + 1) % 3, ky = (kx + 1) % 3;
    if (comp(d, kz) < 0.0f) { int t = kx; kx = ky; ky = t; }
    s.kx = kx; s.ky = ky; s.kz = kz;
    float dz = comp(d, kz);
    s.Sx = comp(d, kx) / dz; s.Sy = comp(d, ky) / dz; s.Sz = 1.0f / dz;
    return s;
}
// Every component finite (x - x is 0 for a finite x and NaN for +-inf and NaN). A caller's ray that is not gives a miss: with an infinite direction
// component traversal_rcp returns 0, every plane is at distance 0 and the far-away box of an unused 4-wide slot passes the slab test -- its child
// reference is no node (hrpt_trace_rays checks its rays with this before it walks; oracle/pt_oracle.c closest_any has the same rule).
HRT_DEV bool all_finite(f3 o, f3 d)
{
    return (o.x - o.x) == 0.0f && (o.y - o.y) == 0.0f && (o.z - o.z) == 0.0f && (d.x - d.x) == 0.0f && (d.y - d.y) == 0.0f && (d.z - d.z) == 0.0f;
}
HRT_DEV bool key_less(float t, uint32_t inst, uint32_t prim, float t2, uint32_t inst2, uint32_t prim2)
{
    if (t < t2) return true;
    if (t > t2) return false;
    if (inst < inst2) return true;
    if (inst > inst2) return false;
    return prim < prim2;
}
// Watertight ray/triangle test (Woop, Benthin, Wald 2013) in fp32; no culling; (u,v) = DXR barycentrics.
HRT_DEV bool tri_test(f3 p0, f3 p1, f3 p2, const Ray& r, const RayShear& s, float& t, float& u, float& v)
{
    f3 A = p0 - r.o, B = p1 - r.o, C = p2 - r.o;
    float Akz = comp(A, s.kz), Bkz = comp(B, s.kz), Ckz = comp(C, s.kz);
    float Ax = comp(A, s.kx) - s.Sx * Akz, Ay = comp(A, s.ky) - s.Sy * Akz;
    float Bx = comp(B, s.kx) - s.Sx * Bkz, By = comp(B, s.ky) - s.Sy * Bkz;
    float Cx = comp(C, s.kx) - s.Sx * Ckz, Cy = comp(C, s.ky) - s.Sy * Ckz;
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
    float det = (U + V) + W;
    if (det == 0.0f) return false;
    float Az = s.Sz * Akz, Bz = s.Sz * Bkz, Cz = s.Sz * Ckz;
    float T = (U * Az + V * Bz) + W * Cz;
    float rcp = 1.0f / det;
    float tt = T * rcp;
    if (!(tt > r.tmin && tt < r.tmax)) return false;
    t = tt; u = V * rcp; v = W * rcp;
    return true;
}

// Node/triangle fetch policy: the BVH is read either from HBM/L2 (global) or from an LDS copy.
struct GlobalBvh {
    static constexpr int kWidth = 2; static constexpr bool kTwoLevel = false;
    const GpuNode* nodes; const GpuTri* tris;
    HRT_DEV void node(int i, float4& a, float4& b, float4& c, float4& d) const
    {
        const float4* p = reinterpret_cast<const float4*>(nodes + i);
        a = p[0]; b = p[1]; c = p[2]; d = p[3];
    }
    HRT_DEV void tri(uint32_t i, float4& a, float4& b, float4& c) const
    {
        const float4* p = reinterpret_cast<const float4*>(tris + i);
        a = p[0]; b = p[1]; c = p[2];
    }
};

struct GlobalBvh4 {
    static constexpr int kWidth = 4; static constexpr bool kTwoLevel = false; static constexpr bool kLds = false;
    const GpuNode4* nodes; const GpuTri* tris;
    // Nodes and triangles are addressed as (array base, 32-bit byte offset): the base stays in scalar registers and a lane holds one VGPR per
    // address instead of a pair (global_load saddr + voffset form; 64-bit address arithmetic is two VALU operations per add on gfx950).
    // Hence the flat structure's limits: fewer than 2^25 4-wide nodes and 2^32 / 48 triangles (bvh_build.cpp validate_scene).
    HRT_DEV void tri(uint32_t i, float4& a, float4& b, float4& c) const
    {
        const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tris) + (size_t)(i * 48u));
        a = p[0]; b = p[1]; c = p[2];
    }
    // one 16-byte row of node i: byte offset 0/16 = min/max x of the four children, 32/48 = y, 64/80 = z, 96 = child refs
    HRT_DEV uint32_t rowoff(int i, uint32_t byteOffset) const { return (uint32_t)i * 128u + byteOffset; }
    HRT_DEV float4 load(uint32_t off) const { return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(nodes) + (size_t)off); }
};

// The flat 4-wide tree through its quantised nodes (GpuNodeQ): what the wavefront kernels traverse when the tree is not LDS-resident.
struct GlobalBvhQ {
    static constexpr int kWidth = 4; static constexpr bool kTwoLevel = false; static constexpr bool kLds = false; static constexpr bool kQuantised = true;
    const GpuNodeQ* nodes; const GpuTri* tris;
    HRT_DEV void tri(uint32_t i, float4& a, float4& b, float4& c) const
    {
        const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tris) + (size_t)(i * 48u));
        a = p[0]; b = p[1]; c = p[2];
    }
    HRT_DEV float4 row(int i, uint32_t r) const { return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(nodes) + (size_t)((uint32_t)i * 64u + r * 16u)); }
};
template <class BVH, class = void> struct IsQuantised { static constexpr bool value = false; };
template <class BVH> struct IsQuantised<BVH, decltype((void)BVH::kQuantised)> { static constexpr bool value = true; };

// Conservative slab test of one child box against [t0, t1]. Culling only: it never changes which hit is
// reported (the hit definition is BVH-independent), so it may use native min/max, the hardware reciprocal and
// FMA. A NaN plane distance (zero direction component with the origin exactly on a padded slab plane) culls the
// box, which is still conservative: padded planes lie strictly outside every triangle extent inside the box.
// Plane distances are one FMA each: t = plane * inv + noi with noi = -(o * inv) computed once per ray. Its error,
// ~6e-8 * |o * inv|, is covered either by the 2e-6 relative widening (when the plane is far from the origin compared with |o|)
// or by the box padding 1e-5 * |coord| + 1e-6 (when it is not). inv is finite (traversal_rcp caps it), so no NaN arises.
HRT_DEV f3 slab_origin_term(f3 o, f3 inv) { return mk3(-(o.x * inv.x), -(o.y * inv.y), -(o.z * inv.z)); }
HRT_DEV bool slab(float4 bmin, float4 bmax, f3 noi, f3 inv, float t0, float t1, float& tnear)
{
    float tx0 = __builtin_fmaf(bmin.x, inv.x, noi.x), tx1 = __builtin_fmaf(bmax.x, inv.x, noi.x);
    float ty0 = __builtin_fmaf(bmin.y, inv.y, noi.y), ty1 = __builtin_fmaf(bmax.y, inv.y, noi.y);
    float tz0 = __builtin_fmaf(bmin.z, inv.z, noi.z), tz1 = __builtin_fmaf(bmax.z, inv.z, noi.z);
    float lo = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(tx0, tx1), __builtin_fminf(ty0, ty1)), __builtin_fmaxf(__builtin_fminf(tz0, tz1), t0));
    float hi = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(tx0, tx1), __builtin_fmaxf(ty0, ty1)), __builtin_fminf(__builtin_fmaxf(tz0, tz1), t1));
    tnear = lo;
    // widen by 2e-6 relative for the rounding of the plane distances
    return __builtin_fmaf(-__builtin_fabsf(lo), 2e-6f, lo) <= __builtin_fmaf(__builtin_fabsf(hi), 2e-6f, hi);
}

constexpr int32_t kTraversalDone = (int32_t)0x80000000;   // not a valid leaf encoding (first < 2^29)

// one box of a 4-wide node: entry distance, or +inf on a miss
HRT_DEV float slab1(float bminx, float bminy, float bminz, float bmaxx, float bmaxy, float bmaxz, f3 noi, f3 inv, float t0, float t1)
{
    float tx0 = __builtin_fmaf(bminx, inv.x, noi.x), tx1 = __builtin_fmaf(bmaxx, inv.x, noi.x);
    float ty0 = __builtin_fmaf(bminy, inv.y, noi.y), ty1 = __builtin_fmaf(bmaxy, inv.y, noi.y);
    float tz0 = __builtin_fmaf(bminz, inv.z, noi.z), tz1 = __builtin_fmaf(bmaxz, inv.z, noi.z);
    float lo = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(tx0, tx1), __builtin_fminf(ty0, ty1)), __builtin_fmaxf(__builtin_fminf(tz0, tz1), t0));
    float hi = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(tx0, tx1), __builtin_fmaxf(ty0, ty1)), __builtin_fminf(__builtin_fmaxf(tz0, tz1), t1));
    bool hit = __builtin_fmaf(-__builtin_fabsf(lo), 2e-6f, lo) <= __builtin_fmaf(__builtin_fabsf(hi), 2e-6f, hi);
    return hit ? lo : __builtin_inff();
}
// Compare-swap of two (entry distance, child) pairs: the pair with the smaller distance ends up in (ta, ra). One compare + four selects, all
// half-rate instructions on gfx950, and the five swaps of a node step are 25 of its 70 half-rate instructions -- but the integer form (mask
// (ib - ia) >> 31 of the bit patterns, masked XOR exchange: one shift + five full-rate integer / v_bitop3 operations) measured 4 % SLOWER on
// configs 2 and 4: full-rate integer and logic operations do not overlap with half-rate ones the way FMAs do.
HRT_DEV void cswap(float& ta, int32_t& ra, float& tb, int32_t& rb)
{
    bool sw = tb < ta;
    float t = sw ? tb : ta; tb = sw ? ta : tb; ta = t;
    int32_t r = sw ? rb : ra; rb = sw ? ra : rb; ra = r;
}

// One traversal step from inner node `cur`: tests its child boxes against [tmin, tlim], pushes the far hits (nearest on
// top) and returns the next node reference: the nearest hit child, else the popped stack top, else kTraversalDone.
// noi / noiF: the origin term of the near / far plane distances. They differ only inside an instance of the two-level structure, where
// every box is widened by a per-ray object-space slack (tl_enter); everywhere else the caller passes the same value twice.
template <class BVH, class STACK>
HRT_DEV int32_t inner_step(const BVH& bvh, int32_t cur, f3 noi, f3 noiF, f3 inv, float tmin, float tlim, STACK& stack, int& sp)
{
    if constexpr (BVH::kWidth == 2) {
        float4 a, b, c, d; bvh.node(cur, a, b, c, d);
        int32_t li = __float_as_int(a.w), ri = __float_as_int(b.w);
        float tl, tr;
        bool hl = slab(a, b, noi, inv, tmin, tlim, tl);
        bool hr = slab(c, d, noi, inv, tmin, tlim, tr);
        if (hl && hr) { bool leftFirst = tl <= tr; stack.push(sp++, leftFirst ? ri : li); return leftFirst ? li : ri; }
        if (hl) return li;
        if (hr) return ri;
        return (sp == 0) ? kTraversalDone : stack.pop(--sp);
    } else if constexpr (IsQuantised<BVH>::value) {
        // 64-byte quantised node: four requests. Plane distance of byte q of an axis: (o + q * s - ray.o) * inv = q * (s * inv) + (o * inv + noi);
        // the near / far plane WORDS of an axis are picked by the sign of the direction, the byte of child c by v_cvt_f32_ubyte<c>.
        const float4 r0 = bvh.row(cur, 0u), r1 = bvh.row(cur, 1u), r2 = bvh.row(cur, 2u), chf = bvh.row(cur, 3u);
        const float ax = r0.w * inv.x, ay = r2.z * inv.y, az = r2.w * inv.z;
        const float bx = __builtin_fmaf(r0.x, inv.x, noi.x), by = __builtin_fmaf(r0.y, inv.y, noi.y), bz = __builtin_fmaf(r0.z, inv.z, noi.z);
        const bool negx = inv.x < 0.0f, negy = inv.y < 0.0f, negz = inv.z < 0.0f;
        const uint32_t wnx = __float_as_uint(negx ? r1.y : r1.x), wfx = __float_as_uint(negx ? r1.x : r1.y);
        const uint32_t wny = __float_as_uint(negy ? r1.w : r1.z), wfy = __float_as_uint(negy ? r1.z : r1.w);
        const uint32_t wnz = __float_as_uint(negz ? r2.y : r2.x), wfz = __float_as_uint(negz ? r2.x : r2.y);
        auto boxq = [&](uint32_t sh) {
            const float lo = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf((float)((wnx >> sh) & 255u), ax, bx), __builtin_fmaf((float)((wny >> sh) & 255u), ay, by)),
                                                             __builtin_fmaf((float)((wnz >> sh) & 255u), az, bz)), tmin);
            const float far3 = __builtin_fminf(__builtin_fminf(__builtin_fmaf((float)((wfx >> sh) & 255u), ax, bx), __builtin_fmaf((float)((wfy >> sh) & 255u), ay, by)),
                                               __builtin_fmaf((float)((wfz >> sh) & 255u), az, bz));
            const float hi = __builtin_fminf(far3, tlim) * (1.0f + 4e-6f);       // as below: the scale after the clamp to tlim
            return lo <= hi ? lo : __builtin_inff();
        };
        float t0 = boxq(0u), t1 = boxq(8u), t2 = boxq(16u), t3 = boxq(24u);
        int32_t r0i = __float_as_int(chf.x), r1i = __float_as_int(chf.y), r2i = __float_as_int(chf.z), r3i = __float_as_int(chf.w);
        cswap(t0, r0i, t1, r1i); cswap(t2, r2i, t3, r3i); cswap(t0, r0i, t2, r2i); cswap(t1, r1i, t3, r3i); cswap(t1, r1i, t2, r2i);
        const float inf = __builtin_inff();
        if (t3 < inf) stack.push(sp++, r3i);
        if (t2 < inf) stack.push(sp++, r2i);
        if (t1 < inf) stack.push(sp++, r1i);
        if (t0 < inf) return r0i;
        return (sp == 0) ? kTraversalDone : stack.pop(--sp);
    } else {
        // The sign of the ray direction says which plane of every slab is the near one, so the near / far rows of the node are picked by
        // ADDRESS (min / max rows of an axis are 16 bytes apart: far = near ^ 16) instead of by six min/max per child box, and the 2e-6
        // relative widening of both ends is folded into one 4e-6 scale of the far end (hi > 0 whenever the test can pass: lo >= tmin >= 0).
        const uint32_t nx = inv.x < 0.0f ? 16u : 0u, ny = inv.y < 0.0f ? 48u : 32u, nz = inv.z < 0.0f ? 80u : 64u;
        // (the far address is derived from the NEAR ADDRESS, not from the offset: offsets are loop-invariant per ray and the compiler
        // would otherwise keep all six in registers -- +6 VGPRs cost the kernel a wave of occupancy; nodes are 128-byte aligned)
        const uint32_t onx = bvh.rowoff(cur, nx), ony = bvh.rowoff(cur, ny), onz = bvh.rowoff(cur, nz);
        const float4 anx = bvh.load(onx), any = bvh.load(ony), anz = bvh.load(onz);
        const float4 afx = bvh.load(onx ^ 16u), afy = bvh.load(ony ^ 16u), afz = bvh.load(onz ^ 16u);
        const float4 chf = bvh.load(bvh.rowoff(cur, 96u));
        auto box = [&](float bnx, float bny, float bnz, float bfx, float bfy, float bfz) {
            const float lo = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(bnx, inv.x, noi.x), __builtin_fmaf(bny, inv.y, noi.y)), __builtin_fmaf(bnz, inv.z, noi.z)), tmin);
            const float far3 = __builtin_fminf(__builtin_fminf(__builtin_fmaf(bfx, inv.x, noiF.x), __builtin_fmaf(bfy, inv.y, noiF.y)), __builtin_fmaf(bfz, inv.z, noiF.z));
            // the scale comes AFTER the clamp to tlim: a second triangle at exactly the distance of the best hit so far (shared edges,
            // coplanar duplicates: the tie is decided by (instance, primitive)) must survive a near distance that rounds just above tlim
            const float hi = __builtin_fminf(far3, tlim) * (1.0f + 4e-6f);
            return lo <= hi ? lo : __builtin_inff();
        };
        float t0 = box(anx.x, any.x, anz.x, afx.x, afy.x, afz.x);
        float t1 = box(anx.y, any.y, anz.y, afx.y, afy.y, afz.y);
        float t2 = box(anx.z, any.z, anz.z, afx.z, afy.z, afz.z);
        float t3 = box(anx.w, any.w, anz.w, afx.w, afy.w, afz.w);
        int32_t r0 = __float_as_int(chf.x), r1 = __float_as_int(chf.y), r2 = __float_as_int(chf.z), r3 = __float_as_int(chf.w);
        cswap(t0, r0, t1, r1); cswap(t2, r2, t3, r3); cswap(t0, r0, t2, r2); cswap(t1, r1, t3, r3); cswap(t1, r1, t2, r2);
        const float inf = __builtin_inff();
        if (t3 < inf) stack.push(sp++, r3);
        if (t2 < inf) stack.push(sp++, r2);
        if (t1 < inf) stack.push(sp++, r1);
        if (t0 < inf) return r0;
        return (sp == 0) ? kTraversalDone : stack.pop(--sp);
    }
}

template <class BVH, class STACK>
HRT_DEV int32_t inner_step(const BVH& bvh, int32_t cur, f3 noi, f3 inv, float tmin, float tlim, STACK& stack, int& sp)
{
    return inner_step(bvh, cur, noi, noi, inv, tmin, tlim, stack, sp);
}

HRT_DEV f3 traversal_rcp(f3 d)
{
    // |1/d| is capped at 1e20 (a zero component would give inf, and inf * plane - inf * origin is NaN in the FMA slab form): over
    // t <= 1e10 such a ray moves less than 1e-10 along that axis, far inside the 1e-6 box padding, so the capped interval still
    // contains every t at which the ray is inside the box.
    auto one = [](float x) { return __builtin_fminf(__builtin_fmaxf(__builtin_amdgcn_rcpf(x), -1e20f), 1e20f); };
    return mk3(one(d.x), one(d.y), one(d.z));
}

// Closest triangle (opaque or not) with key strictly above `lower` (when lower.have) in (t, inst, prim) order.
// while-while traversal: all lanes of the wave first descend inner nodes, then intersect leaves together.
// STACK: per-lane traversal stack accessor (LDS column or private array).
// nodeLoopMin: the descent loop ends once fewer lanes than this are still at inner nodes (thresholded while-while; 0 = run to a leaf)
template <class BVH, class STACK>
HRT_DEV Hit closest_any(const BVH& bvh, int32_t rootLeaf, uint32_t nodeCount, const Ray& r, HitKey lower, STACK& stack, uint32_t nodeLoopMin = 0)
{
    Hit best; best.valid = false; best.t = r.tmax; best.inst = 0; best.prim = 0; best.u = 0; best.v = 0; best.opaque = 0; best.tri = 0;
    if (!(r.d.x == r.d.x && r.d.y == r.d.y && r.d.z == r.d.z)) return best;
    RayShear sh = make_shear(r.d);
    f3 inv = traversal_rcp(r.d), noi = slab_origin_term(r.o, inv);
    int sp = 0;
    int32_t cur;                       // current node reference: >= 0 inner, < 0 leaf
    if (nodeCount == 0) { if (rootLeaf == 0) return best; cur = rootLeaf; }
    else cur = 0;
    float tlim = r.tmax;               // == best.t once a hit exists
    for (;;) {
        while (cur >= 0) {
            cur = inner_step(bvh, cur, noi, inv, r.tmin, tlim, stack, sp);
            if ((uint32_t)__popcll(__ballot(cur >= 0)) < nodeLoopMin) break;
        }
        if (cur == kTraversalDone) break;
        if (cur < 0) {
            uint32_t enc = (uint32_t)(~cur);
            uint32_t first = enc >> 2, count = (enc & 3u) + 1u;
            for (uint32_t i = 0; i < count; ++i) {
                float4 a, b, c; bvh.tri(first + i, a, b, c);
                float t, u, v;
                if (tri_test(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), r, sh, t, u, v)) {
                    uint32_t inst = __float_as_uint(a.w), prim = __float_as_uint(b.w);
                    bool ok = !lower.have || key_less(lower.t, lower.inst, lower.prim, t, inst, prim);
                    const bool take = ok && (!best.valid || key_less(t, inst, prim, best.t, best.inst, best.prim));      // selects on one flag: pt_wavefront.hip wf_extend<TL>
                    best.t = take ? t : best.t; best.u = take ? u : best.u; best.v = take ? v : best.v;
                    best.inst = take ? inst : best.inst; best.prim = take ? prim : best.prim; best.tri = take ? first + i : best.tri;
                    best.opaque = take ? (__float_as_uint(c.w) & 1u) : best.opaque;
                    best.valid = best.valid || take;
                    tlim = take ? t : tlim;
                }
            }
            if (sp == 0) break;
            cur = stack.pop(--sp);
        }
    }
    return best;
}

// Any opaque-instance triangle in (tmin, tmax)? Early exit. Non-opaque triangles are only noted.
template <class BVH, class STACK>
HRT_DEV bool any_opaque(const BVH& bvh, int32_t rootLeaf, uint32_t nodeCount, const Ray& r, STACK& stack, bool& sawNonOpaque, uint32_t nodeLoopMin = 0)
{
    sawNonOpaque = false;
    if (!(r.d.x == r.d.x && r.d.y == r.d.y && r.d.z == r.d.z)) return false;
    RayShear sh = make_shear(r.d);
    f3 inv = traversal_rcp(r.d), noi = slab_origin_term(r.o, inv);
    int sp = 0; int32_t cur;
    if (nodeCount == 0) { if (rootLeaf == 0) return false; cur = rootLeaf; }
    else cur = 0;
    for (;;) {
        while (cur >= 0) {
            cur = inner_step(bvh, cur, noi, inv, r.tmin, r.tmax, stack, sp);
            if ((uint32_t)__popcll(__ballot(cur >= 0)) < nodeLoopMin) break;
        }
        if (cur == kTraversalDone) break;
        if (cur < 0) {
            uint32_t enc = (uint32_t)(~cur);
            uint32_t first = enc >> 2, count = (enc & 3u) + 1u;
            for (uint32_t i = 0; i < count; ++i) {
                float4 a, b, c; bvh.tri(first + i, a, b, c);
                float t, u, v;
                if (tri_test(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), r, sh, t, u, v)) {
                    if (__float_as_uint(c.w) & 1u) return true;
                    sawNonOpaque = true;
                }
            }
            if (sp == 0) break;
            cur = stack.pop(--sp);
        }
    }
    return false;
}

// ------------------------------------------------------------------ two-level traversal (instanced scenes)
// The tree over the instances is walked with the world-space ray. At an instance leaf the lane pushes kExitBlas, switches its CULLING
// state (inv, noi) to the ray in the instance's object space and continues in the mesh's tree; popping kExitBlas switches back. Triangles
// are never tested in object space: a leaf transforms its three object-space vertices with m_World exactly as the flat upload does
// (bvh_build.cpp transform_point: left to right, no FMA) and runs the same watertight test on the world ray, so the hit (t, u, v) and the
// (t, instance, primitive) order are those of the flat path bit for bit. The object-space ray keeps the world parametrisation (its
// direction is d * Minv, not normalised), so tlim needs no conversion.
constexpr int32_t kExitBlas = 0x7FFFFFFE;     // stack marker; never a node index (node4 counts stay below 2^29)
struct GlobalBvhTl : GlobalBvh4 {
    static constexpr bool kTwoLevel = true;
    const GpuInstance* instances;
};
struct TlCull { f3 inv, noi, noiF; int32_t inst; };     // inst < 0: in the tree over the instances (world space, noi == noiF)
HRT_DEV void tl_world(TlCull& c, const Ray& r)
{
    c.inv = traversal_rcp(r.d); c.noi = slab_origin_term(r.o, c.inv); c.noiF = c.noi; c.inst = -1;
}
// Culling state inside instance I. Everything that separates the computed object-space ray from the exact image of the world ray, and
// the object-space triangles from the (rounded) world triangles the test runs on, is bounded by `eps` and added to both sides of every
// slab of the mesh's tree:
//   - I.boxEps: the binary32 rounding of the transformed vertices, mapped back through |Minv| (host, bvh_build.cpp)
//   - the rounding of o - T (half an ulp of the larger operand) and of the three products / two sums per component of (o - T) * Minv,
//     d * Minv, and of Minv itself (rounded from binary64): 2.4e-7 relative to the operands' magnitudes times ||Minv||
//   - the direction error acts over the parameter range in which the ray can be inside the mesh's box: t * |d'| <= objMaxAbs + |o'|
// with a factor 4 on top. Over-estimating eps only costs culling.
HRT_DEV void tl_enter(TlCull& c, const GpuInstance& I, int32_t inst, const Ray& r)
{
    const float4* w = reinterpret_cast<const float4*>(I.world);
    const float4 w2 = w[2];                                        // {M22, T.x, T.y, T.z}
    const float4* q = reinterpret_cast<const float4*>(I.inv);
    const float4 q0 = q[0], q1 = q[1]; const float q22 = I.inv[8];    // rows of Minv: {a00 a01 a02 a10} {a11 a12 a20 a21} a22
    const f3 rel = mk3(r.o.x - w2.y, r.o.y - w2.z, r.o.z - w2.w);
    const f3 oo = mk3(__builtin_fmaf(rel.z, q1.z, __builtin_fmaf(rel.y, q0.w, rel.x * q0.x)),
                      __builtin_fmaf(rel.z, q1.w, __builtin_fmaf(rel.y, q1.x, rel.x * q0.y)),
                      __builtin_fmaf(rel.z, q22, __builtin_fmaf(rel.y, q1.y, rel.x * q0.z)));
    const f3 od = mk3(__builtin_fmaf(r.d.z, q1.z, __builtin_fmaf(r.d.y, q0.w, r.d.x * q0.x)),
                      __builtin_fmaf(r.d.z, q1.w, __builtin_fmaf(r.d.y, q1.x, r.d.x * q0.y)),
                      __builtin_fmaf(r.d.z, q22, __builtin_fmaf(r.d.y, q1.y, r.d.x * q0.z)));
    auto max3abs = [](f3 v) { return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), __builtin_fabsf(v.z)); };
    const float oMax = __builtin_fmaxf(max3abs(r.o), __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(w2.y), __builtin_fabsf(w2.z)), __builtin_fabsf(w2.w)));
    const float dRatio = max3abs(r.d) * I.invNorm / __builtin_fmaxf(max3abs(od), 1e-30f);
    const float eps = I.boxEps + 4.0f * 2.4e-7f * (I.invNorm * (oMax + max3abs(rel)) + dRatio * (I.objMaxAbs + max3abs(oo)));
    c.inv = traversal_rcp(od);
    const f3 n = slab_origin_term(oo, c.inv);
    const f3 e = mk3(eps * __builtin_fabsf(c.inv.x), eps * __builtin_fabsf(c.inv.y), eps * __builtin_fabsf(c.inv.z));
    c.noi = mk3(n.x - e.x, n.y - e.y, n.z - e.z); c.noiF = mk3(n.x + e.x, n.y + e.y, n.z + e.z);
    c.inst = inst;
}
// world-space vertices of object-space triangle (a, b, c) of instance I: transform_point of bvh_build.cpp (mul(float4(p,1), M).xyz, left to right)
HRT_DEV void tl_world_triangle(const GpuInstance& I, float4 a, float4 b, float4 c, f3& p0, f3& p1, f3& p2)
{
    const float4* w = reinterpret_cast<const float4*>(I.world);
    const float4 w0 = w[0], w1 = w[1], w2 = w[2];      // {M00 M01 M02 M10} {M11 M12 M20 M21} {M22 Tx Ty Tz}
    auto xf = [&](float x, float y, float z) {
        return mk3(((x * w0.x + y * w0.w) + z * w1.z) + w2.y,
                   ((x * w0.y + y * w1.x) + z * w1.w) + w2.z,
                   ((x * w0.z + y * w1.y) + z * w2.x) + w2.w);
    };
    p0 = xf(a.x, a.y, a.z); p1 = xf(b.x, b.y, b.z); p2 = xf(c.x, c.y, c.z);
}
// One node reference of the two-level walk that is not an inner node of the current tree: the BLAS exit marker or an instance leaf.
// Returns the next reference (and updates the culling state); triangle leaves (c.inst >= 0, cur < 0) are the caller's.
template <class STACK>
HRT_DEV int32_t tl_switch(const GlobalBvhTl& bvh, int32_t cur, TlCull& c, const Ray& r, STACK& stack, int& sp)
{
    if (cur == kExitBlas) { tl_world(c, r); return sp == 0 ? kTraversalDone : stack.pop(--sp); }
    // instance leaf
    const int32_t inst = (int32_t)(((uint32_t)~cur) >> 2);
    const GpuInstance& I = bvh.instances[inst];
    const int32_t root = I.blasRoot;
    if (root == kTraversalDone) return sp == 0 ? kTraversalDone : stack.pop(--sp);      // mesh without triangles
    stack.push(sp++, kExitBlas);
    tl_enter(c, I, inst, r);
    return root;
}

// any_opaque over the two-level structure: true at the first triangle of a ForceOpaque instance; triangles of other instances are only noted
template <class STACK>
HRT_DEV bool any_hit_two_level(const GlobalBvhTl& bvh, int32_t rootLeaf, uint32_t nodeCount, const Ray& r, STACK& stack, bool& sawNonOpaque, uint32_t nodeLoopMin = 0)
{
    sawNonOpaque = false;
    if (!(r.d.x == r.d.x && r.d.y == r.d.y && r.d.z == r.d.z)) return false;
    RayShear sh = make_shear(r.d);
    TlCull c; tl_world(c, r);
    int sp = 0; int32_t cur;
    if (nodeCount == 0) { if (rootLeaf == 0) return false; cur = rootLeaf; }
    else cur = 0;
    for (;;) {
        while (cur >= 0 && cur != kExitBlas) {
            cur = inner_step(bvh, cur, c.noi, c.noiF, c.inv, r.tmin, r.tmax, stack, sp);
            if ((uint32_t)__popcll(__ballot(cur >= 0 && cur != kExitBlas)) < nodeLoopMin) break;
        }
        if (cur == kTraversalDone) break;
        if (cur == kExitBlas || (cur < 0 && c.inst < 0)) { cur = tl_switch(bvh, cur, c, r, stack, sp); continue; }
        if (cur < 0) {
            const GpuInstance& I = bvh.instances[c.inst];
            uint32_t enc = (uint32_t)(~cur);
            uint32_t first = enc >> 2, count = (enc & 3u) + 1u;
            for (uint32_t i = 0; i < count; ++i) {
                float4 ta, tb, tc; bvh.tri(first + i, ta, tb, tc);
                f3 p0, p1, p2; tl_world_triangle(I, ta, tb, tc, p0, p1, p2);
                float t, u, v;
                if (tri_test(p0, p1, p2, r, sh, t, u, v)) { if (I.flags & 1u) return true; sawNonOpaque = true; }
            }
            cur = stack.pop(--sp);          // never empty inside an instance: the exit marker is below
        }
    }
    return false;
}
// closest_any over the two-level structure: the closest triangle with key strictly above `lower` (candidate re-trace of the shadow query)
template <class STACK>
HRT_DEV Hit closest_two_level(const GlobalBvhTl& bvh, int32_t rootLeaf, uint32_t nodeCount, const Ray& r, HitKey lower, STACK& stack)
{
    Hit best; best.valid = false; best.t = r.tmax; best.inst = 0; best.prim = 0; best.u = 0; best.v = 0; best.opaque = 0; best.tri = 0;
    if (!(r.d.x == r.d.x && r.d.y == r.d.y && r.d.z == r.d.z)) return best;
    RayShear sh = make_shear(r.d);
    TlCull c; tl_world(c, r);
    int sp = 0; int32_t cur;
    if (nodeCount == 0) { if (rootLeaf == 0) return best; cur = rootLeaf; }
    else cur = 0;
    float tlim = r.tmax;
    for (;;) {
        while (cur >= 0 && cur != kExitBlas) cur = inner_step(bvh, cur, c.noi, c.noiF, c.inv, r.tmin, tlim, stack, sp);
        if (cur == kTraversalDone) break;
        if (cur == kExitBlas || (cur < 0 && c.inst < 0)) { cur = tl_switch(bvh, cur, c, r, stack, sp); continue; }
        const GpuInstance& I = bvh.instances[c.inst];
        const uint32_t enc = (uint32_t)(~cur), first = enc >> 2, count = (enc & 3u) + 1u, inst = (uint32_t)c.inst;
        for (uint32_t i = 0; i < count; ++i) {
            float4 ta, tb, tc; bvh.tri(first + i, ta, tb, tc);
            f3 p0, p1, p2; tl_world_triangle(I, ta, tb, tc, p0, p1, p2);
            float t, u, v;
            const bool hitTri = tri_test(p0, p1, p2, r, sh, t, u, v);
            const uint32_t prim = __float_as_uint(tb.w);
            const bool ok = !lower.have || key_less(lower.t, lower.inst, lower.prim, t, inst, prim);
            const bool take = hitTri && ok && (!best.valid || key_less(t, inst, prim, best.t, best.inst, best.prim));
            best.t = take ? t : best.t; best.u = take ? u : best.u; best.v = take ? v : best.v;
            best.inst = take ? inst : best.inst; best.prim = take ? prim : best.prim; best.tri = take ? first + i : best.tri;
            best.opaque = take ? (I.flags & 1u) : best.opaque;
            best.valid = best.valid || take;
            tlim = take ? t : tlim;
        }
        cur = stack.pop(--sp);
    }
    return best;
}

// ------------------------------------------------------------------ the tree views of a scene
// GlobalBvhOf<key>::make(scene): the fetch policy over the scene's arrays in global memory. Keys: the node width (2, 4), kQuantisedTree,
// kTwoLevelTree. What the wavefront kernels (pt_wf_*.h) and the thread-per-query kernels (pt_megakernel.hip) build their tree from.
template <int W> struct GlobalBvhOf;
template <> struct GlobalBvhOf<2> { using type = GlobalBvh; static HRT_DEV GlobalBvh make(const SceneView& s) { GlobalBvh g; g.nodes = s.nodes; g.tris = s.tris; return g; } };
constexpr int kTwoLevelTree = 44;     // GlobalBvhOf key of the two-level structure (4-wide nodes)
template <> struct GlobalBvhOf<kTwoLevelTree> { using type = GlobalBvhTl; static HRT_DEV GlobalBvhTl make(const SceneView& s) { GlobalBvhTl g; g.nodes = s.nodes4; g.tris = s.tris; g.instances = s.instances; return g; } };
template <> struct GlobalBvhOf<4> { using type = GlobalBvh4; static HRT_DEV GlobalBvh4 make(const SceneView& s) { GlobalBvh4 g; g.nodes = s.nodes4; g.tris = s.tris; return g; } };
constexpr int kQuantisedTree = 5;     // template width code of the 4-wide tree through its 64-byte quantised nodes (global memory only; pt_scene_records.h GpuNodeQ)
template <> struct GlobalBvhOf<kQuantisedTree> { using type = GlobalBvhQ; static HRT_DEV GlobalBvhQ make(const SceneView& s) { GlobalBvhQ g; g.nodes = s.nodesQ; g.tris = s.tris; return g; } };

} // namespace hrt

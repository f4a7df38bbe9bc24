// pt_shadow.h -- CalculateRTShadow<true> (/root/reference/src/shaders/CommonLighting.hlsli:380-496): visibility of a shadow ray through
// non-opaque geometry. Any hit on a ForceOpaque instance commits (-> 0); the triangles of the other instances are visited front to back in
// (t, instance, primitive) order, each one running the per-candidate body once (MASK alpha test, BLEND opacity, Beer-Lambert absorption
// between a front and a back face). The forms below differ in how they find the candidates, never in what they do with one:
//   shadow_query                     re-trace form: an any-hit pass over the opaque triangles, then one closest-hit query per candidate
//   shadow_query_buffered            ONE traversal that also keeps the K nearest candidates in a per-lane buffer (flat tree)
//   shadow_query_two_level_buffered  the same over the two-level structure
//   candidate_insert / shadow_resolve_candidates   the two halves of the buffered form, for a schedule that traverses elsewhere (wf_extend<ANYHIT>)
// A candidate buffer CAND (LdsCandidates / GlobalCandidates: (t, triangle); LdsCandidates3: (t, mesh triangle, instance); pt_wf_common.h)
// offers key(k, t, tri, inst), set(k, t, tri, inst) and move(dst, src); a two-column buffer leaves `inst` alone and the flat tree's triangle
// record supplies it.
// Two loops are NOT shared, because the kernels that hold them are compiled into fewer registers than they want and come out differently
// (slower on the glass config, or with more scratch) for any other spelling: the flat resolve (shadow_resolve_candidates) keeps its own
// visiting loop and its own tail where shadow_walk would do, and shadow_query_two_level_buffered keeps its own visiting loop. Both run the
// shared per-candidate body. profiles/shadow_queries_refactor.txt has the figures; tests/test_kernel_resources.py pins the resolve's.
#pragma once

#include "pt_device.h"

namespace hrt {

// (general HitKey helpers, also used by trace_standard in pt_path.h: they belong next to HitKey in pt_traverse.h)
HRT_DEV HitKey hit_key_none() { HitKey k; k.have = false; k.t = 0.0f; k.inst = 0; k.prim = 0; return k; }     // no lower bound
HRT_DEV void hit_key_advance(HitKey& k, const Hit& h) { k.have = true; k.t = h.t; k.inst = h.inst; k.prim = h.prim; }    // behind h

// State carried from candidate to candidate (:404-407)
struct ShadowState { float transmission; bool inVolume; float inVolumeStartT; f3 sigmaT; };
HRT_DEV ShadowState shadow_state()
{
    ShadowState st; st.transmission = 1.0f; st.inVolume = false; st.inVolumeStartT = 0.0f; st.sigmaT = mk3(0.0f, 0.0f, 0.0f);
    return st;
}
HRT_DEV Ray shadow_ray(f3 worldPos, f3 L, float maxDist)                           // :391-396
{
    const float kShadowBias = 0.01f;
    Ray ray; ray.o = worldPos; ray.d = L; ray.tmin = kShadowBias; ray.tmax = hrt_max(kShadowBias, maxDist - kShadowBias * 2.0f);
    return ray;
}
// Beer-Lambert over the volume segment that ends at endT, as a luminance factor (:455-461, :480-486)
HRT_DEV void shadow_absorb(ShadowState& st, float endT)
{
    float seg = hrt_max(0.0f, endT - st.inVolumeStartT);
    f3 tr = mk3(hrt_exp(-st.sigmaT.x * seg), hrt_exp(-st.sigmaT.y * seg), hrt_exp(-st.sigmaT.z * seg));
    st.transmission *= dot(tr, mk3(0.2126f, 0.7152f, 0.0722f));
}
// The per-candidate body (:409-470) for a crossed triangle of a non-opaque instance; true when the candidate commits (the query then
// returns 0). TL: the hit is one of the two-level structure. Its triangle and attribute records are per MESH, so instance and material come
// from the hit (load_hit_attr) and the world-space vertices, which only the mip-selecting alpha test asks for, from the instance's m_World.
template <bool TL>
HRT_DEV bool shadow_candidate(const SceneView& s, const Ray& ray, const Hit& h, ShadowState& st)
{
    TriVerts tv;                                   // inst.m_LODIndex is 0 on this path (validated at upload), :423
    if constexpr (TL) tv = load_hit_attr(s, h); else tv = load_tri_attr(s, h.tri);
    const HrptMaterialConstants& mat = s.materials[tv.material];
    f2 uv = interpolated_uv(tv, h.u, h.v);
    if (mat.m_AlphaMode == HRPT_ALPHA_MODE_MASK) {
        // AlphaTestGrad (RaytracingCommon.hlsli:112-130) with GetShadowRayGradients (:207-240); level 0 unless the texture has a mip chain
        auto worldTriangle = [&](f3& p0, f3& p1, f3& p2) {
            if constexpr (TL) {
                const float4* tp = reinterpret_cast<const float4*>(s.tris + h.tri);
                tl_world_triangle(s.instances[h.inst], tp[0], tp[1], tp[2], p0, p1, p2);
            } else { const GpuTri& g = s.tris[h.tri]; p0 = mk3(g.p0); p1 = mk3(g.p1); p2 = mk3(g.p2); }
        };
        return candidate_alpha_grad(s, mat, uv, tv, h.u, h.v, ray.o, worldTriangle) >= mat.m_AlphaCutoff;
    }
    if (mat.m_AlphaMode != HRPT_ALPHA_MODE_BLEND) return true;
    float alpha = candidate_alpha(s, mat, uv);
    float opacity = hrt_saturate(alpha * (1.0f - mat.m_TransmissionFactor));
    st.transmission *= (1.0f - opacity);
    if (mat.m_TransmissionFactor > 0.0f && mat.m_IsThinSurface == 0) {
        float w0 = (1.0f - h.u) - h.v;
        f3 ln = (tv.n0 * w0 + tv.n1 * h.u) + tv.n2 * h.v;
        f3 wn = normalize(transform_normal(ln, s.instShade[tv.inst]));
        bool front = dot(wn, ray.d) < 0.0f;
        if (front) { st.inVolume = true; st.inVolumeStartT = h.t; st.sigmaT = mk3(mat.m_SigmaA) + mk3(mat.m_SigmaS); }
        else if (st.inVolume) { shadow_absorb(st, h.t); st.inVolume = false; }
    }
    return st.transmission <= 1e-3f;
}
HRT_DEV float shadow_finish(const Ray& ray, ShadowState& st)                       // :477-495
{
    if (st.inVolume) shadow_absorb(st, ray.tmax);
    return hrt_saturate(st.transmission);
}

// The candidates behind `lower`, front to back, one closest-hit query each: true when one commits (the query then returns 0); any other
// becomes the exclusive lower bound of the next query. From hit_key_none() this is the whole candidate pass of the re-trace form; from the
// K-th key it is the continuation of a buffered form whose ray crossed more than K candidates.
// A hit on an opaque instance commits, as in the reference's loop. Every caller runs this after an any-hit pass that returned at the first
// opaque triangle the ray crosses (the same tri_test on the same vertices), so the test is not expected to fire; it costs one compare per
// query and keeps the walk right on its own, whatever ran before it.
template <class BVH, class STACK>
HRT_DEV bool shadow_walk(const SceneView& s, const BVH& bvh, const Ray& ray, HitKey lower, ShadowState& st, STACK& stack)
{
    for (;;) {
        Hit h;
        if constexpr (BVH::kTwoLevel) h = closest_two_level(bvh, s.rootLeaf, s.nodeCount, ray, lower, stack);
        else h = closest_any(bvh, s.rootLeaf, s.nodeCount, ray, lower, stack);
        if (!h.valid) return false;
        if (h.opaque || shadow_candidate<BVH::kTwoLevel>(s, ray, h, st)) return true;
        hit_key_advance(lower, h);
    }
}
// The candidate pass of the re-trace form: for a ray that crossed triangles of non-opaque instances and none of an opaque one.
template <class BVH, class STACK>
HRT_DEV float shadow_retrace(const SceneView& s, const BVH& bvh, const Ray& ray, STACK& stack)
{
    ShadowState st = shadow_state();
    if (shadow_walk(s, bvh, ray, hit_key_none(), st, stack)) return 0.0f;
    return shadow_finish(ray, st);
}

// Re-trace form (validation megakernel, ray queries; wf_shadow's opaque variants with ALL_OPAQUE).
// ALL_OPAQUE: the scene is known (upload-time trait) to hold ForceOpaque instances only: the candidate pass is compiled out.
template <bool ALL_OPAQUE = false, class BVH, class STACK>
HRT_DEV float shadow_query(const SceneView& s, const BVH& bvh, f3 worldPos, f3 L, float maxDist, STACK& stack, uint32_t nodeLoopMin = 0)
{
    Ray ray = shadow_ray(worldPos, L, maxDist);
    // Any hit on a ForceOpaque instance commits -> 0, whatever lies in front of it.
    bool sawNonOpaque;
    if constexpr (BVH::kTwoLevel) { if (any_hit_two_level(bvh, s.rootLeaf, s.nodeCount, ray, stack, sawNonOpaque, nodeLoopMin)) return 0.0f; }
    else if (any_opaque(bvh, s.rootLeaf, s.nodeCount, ray, stack, sawNonOpaque, nodeLoopMin)) return 0.0f;
    if (ALL_OPAQUE || !sawNonOpaque) return 1.0f;
    return shadow_retrace(s, bvh, ray, stack);
}

// ---- buffered forms: the K nearest candidates, sorted by (t, instance, primitive), in a per-lane buffer -----------------------------------
// A non-opaque hit into the buffer of the K smallest keys, kept sorted; `overflow` once a hit did not fit. The (instance, primitive) of a
// stored entry: both from the flat tree's world-space triangle record; a two-level tree's record is per mesh, so the instance is the one
// stored with the candidate. In the loop they are fetched on a tie in t only.
template <int K, class BVH, class CAND>
HRT_DEV void candidate_insert(const BVH& bvh, CAND& cand, int& count, bool& overflow, float t, uint32_t tri, uint32_t inst, uint32_t prim)
{
    int pos = count;
    if (count == K) {
        float lt; uint32_t ltri, linst; cand.key(K - 1, lt, ltri, linst);
        float4 la, lb, lc; bvh.tri(ltri, la, lb, lc);
        if constexpr (!BVH::kTwoLevel) linst = __float_as_uint(la.w);
        overflow = true;
        if (!key_less(t, inst, prim, lt, linst, __float_as_uint(lb.w))) return;
        pos = K - 1;
    } else ++count;
    while (pos > 0) {
        float pt; uint32_t ptri, pinst; cand.key(pos - 1, pt, ptri, pinst);
        bool less;
        if (t != pt) less = t < pt;
        else {
            float4 pa, pb, pc; bvh.tri(ptri, pa, pb, pc);
            if constexpr (!BVH::kTwoLevel) pinst = __float_as_uint(pa.w);
            less = key_less(t, inst, prim, pt, pinst, __float_as_uint(pb.w));
        }
        if (!less) break;
        cand.move(pos, pos - 1);
        --pos;
    }
    cand.set(pos, t, tri, inst);
}
// The shared per-candidate body for a candidate of a flat tree given by its triangle and barycentrics (what a two-column buffer holds)
HRT_DEV bool shadow_candidate_flat(const SceneView& s, const Ray& ray, float hitT, uint32_t tri, float bu, float bv, ShadowState& st)
{
    Hit h; h.valid = true; h.opaque = 0; h.inst = 0; h.prim = 0; h.t = hitT; h.tri = tri; h.u = bu; h.v = bv;
    return shadow_candidate<false>(s, ray, h, st);
}
// The buffered candidates of a flat tree front to back (`cand.key(k, ...)` yields the k-th smallest key), then -- if more than K existed --
// the re-trace loop behind the K-th, then the closing Beer-Lambert segment.
// The tail is shadow_walk's loop written out, and the visiting loop is not shared with the two-level buffered query: wf_shadow's resolve
// variant is compiled into 128 VGPRs (it wants 146-150), and only in this spelling does it come out as it did before pt_shadow.h existed;
// with shadow_walk in the tail or a Hit carried through the loop the glass config lost 0.5 to 2 %.
template <class BVH, class STACK, class CAND>
HRT_DEV float shadow_resolve_candidates(const SceneView& s, const BVH& bvh, const Ray& ray, const RayShear& sh, int count, bool overflow, const CAND& cand, STACK& stack)
{
    if (count == 0) return 1.0f;
    ShadowState st = shadow_state();
    float lastT = 0.0f; uint32_t lastTri = 0;
    for (int k = 0; k < count; ++k) {
        float t; uint32_t tri, unused; cand.key(k, t, tri, unused);
        float4 a, b, c; bvh.tri(tri, a, b, c);
        float t2, u, v;
        tri_test(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), ray, sh, t2, u, v);   // recomputes (t, u, v) bit for bit
        if (shadow_candidate_flat(s, ray, t, tri, u, v, st)) return 0.0f;
        lastT = t; lastTri = tri;
    }
    if (overflow) {   // more than K candidates: continue behind the K-th
        float4 la, lb, lc; bvh.tri(lastTri, la, lb, lc);
        HitKey lower; lower.have = true; lower.t = lastT; lower.inst = __float_as_uint(la.w); lower.prim = __float_as_uint(lb.w);
        for (;;) {
            Hit h = closest_any(bvh, s.rootLeaf, s.nodeCount, ray, lower, stack);
            if (!h.valid) break;
            if (h.opaque) return 0.0f;
            if (shadow_candidate_flat(s, ray, h.t, h.tri, h.u, h.v, st)) return 0.0f;
            lower.t = h.t; lower.inst = h.inst; lower.prim = h.prim;
        }
    }
    return shadow_finish(ray, st);
}
template <int K, class BVH, class STACK, class CAND>
HRT_DEV float shadow_query_buffered(const SceneView& s, const BVH& bvh, f3 worldPos, f3 L, float maxDist, STACK& stack, CAND& cand, uint32_t nodeLoopMin = 0)
{
    Ray ray = shadow_ray(worldPos, L, maxDist);
    if (!(ray.d.x == ray.d.x && ray.d.y == ray.d.y && ray.d.z == ray.d.z)) return 1.0f;
    RayShear sh = make_shear(ray.d);
    f3 inv = traversal_rcp(ray.d), noi = slab_origin_term(ray.o, inv);
    int sp = 0, count = 0; bool overflow = false;
    int32_t cur;
    if (s.nodeCount == 0) { if (s.rootLeaf == 0) return 1.0f; cur = s.rootLeaf; } else cur = 0;
    for (;;) {
        while (cur >= 0) {
            cur = inner_step(bvh, cur, noi, inv, ray.tmin, ray.tmax, stack, sp);
            if ((uint32_t)__popcll(__ballot(cur >= 0)) < nodeLoopMin) break;
        }
        if (cur == kTraversalDone) break;
        if (cur >= 0) continue;
        uint32_t enc = (uint32_t)(~cur);
        uint32_t first = enc >> 2, n = (enc & 3u) + 1u;
        for (uint32_t i = 0; i < n; ++i) {
            float4 a, b, c; bvh.tri(first + i, a, b, c);
            float t, u, v;
            if (!tri_test(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), ray, sh, t, u, v)) continue;
            if (__float_as_uint(c.w) & 1u) return 0.0f;                           // opaque instance: committed
            candidate_insert<K>(bvh, cand, count, overflow, t, first + i, __float_as_uint(a.w), __float_as_uint(b.w));
        }
        if (sp == 0) break;
        cur = stack.pop(--sp);
    }
    return shadow_resolve_candidates(s, bvh, ray, sh, count, overflow, cand, stack);
}
// Over the two-level structure (wf_shadow<TL = 2>): returns at the first triangle of an opaque instance and buffers the triangles of
// non-opaque instances as (t, mesh triangle, instance).
template <int K, class STACK, class CAND3>
HRT_DEV float shadow_query_two_level_buffered(const SceneView& s, const GlobalBvhTl& bvh, const Ray& ray, STACK& stack, CAND3& cand, uint32_t nodeLoopMin = 0)
{
    if (!(ray.d.x == ray.d.x && ray.d.y == ray.d.y && ray.d.z == ray.d.z)) return 1.0f;
    RayShear sh = make_shear(ray.d);
    TlCull c; tl_world(c, ray);
    int sp = 0, count = 0; bool overflow = false;
    int32_t cur;
    if (s.nodeCount == 0) { if (s.rootLeaf == 0) return 1.0f; cur = s.rootLeaf; } else cur = 0;
    for (;;) {
        while (cur >= 0 && cur != kExitBlas) {
            cur = inner_step(bvh, cur, c.noi, c.noiF, c.inv, ray.tmin, ray.tmax, stack, sp);
            if ((uint32_t)__popcll(__ballot(cur >= 0 && cur != kExitBlas)) < nodeLoopMin) break;
        }
        if (cur == kTraversalDone) break;
        if (cur == kExitBlas || (cur < 0 && c.inst < 0)) { cur = tl_switch(bvh, cur, c, ray, stack, sp); continue; }
        if (cur >= 0) continue;
        const GpuInstance& I = bvh.instances[c.inst];
        const uint32_t enc = (uint32_t)(~cur), first = enc >> 2, n = (enc & 3u) + 1u, inst = (uint32_t)c.inst;
        for (uint32_t i = 0; i < n; ++i) {
            float4 ta, tb, tc; bvh.tri(first + i, ta, tb, tc);
            f3 p0, p1, p2; tl_world_triangle(I, ta, tb, tc, p0, p1, p2);
            float t, u, v;
            if (!tri_test(p0, p1, p2, ray, sh, t, u, v)) continue;
            if (I.flags & 1u) return 0.0f;                                        // opaque instance: committed
            candidate_insert<K>(bvh, cand, count, overflow, t, first + i, inst, __float_as_uint(tb.w));
        }
        cur = stack.pop(--sp);
    }
    // The buffered candidates front to back, in a loop of this query's own: sharing one with the flat resolve, the depth-64 any-light
    // variant of wf_shadow<TL = 2> (168 VGPRs, held at 3 waves) spilled 24 B instead of 20. The per-candidate body, the sorted insert above
    // and the walk behind the K-th are the shared ones.
    if (count == 0) return 1.0f;
    ShadowState st = shadow_state();
    Hit h; h.valid = true; h.opaque = 0; h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.tri = 0; h.inst = 0; h.prim = 0;
    for (int k = 0; k < count; ++k) {
        float kt; cand.key(k, kt, h.tri, h.inst);
        float4 ta, tb, tc; bvh.tri(h.tri, ta, tb, tc);
        f3 p0, p1, p2; tl_world_triangle(bvh.instances[h.inst], ta, tb, tc, p0, p1, p2);
        tri_test(p0, p1, p2, ray, sh, h.t, h.u, h.v);                               // recomputes (t, u, v) bit for bit
        h.prim = __float_as_uint(tb.w);
        if (shadow_candidate<true>(s, ray, h, st)) return 0.0f;
    }
    if (overflow) {   // more than K candidates: continue behind the K-th
        HitKey lower; lower.have = true; lower.t = h.t; lower.inst = h.inst; lower.prim = h.prim;
        if (shadow_walk(s, bvh, ray, lower, st, stack)) return 0.0f;
    }
    return shadow_finish(ray, st);
}

} // namespace hrt

// pt_path.h -- the per-path stages of PathTracer_CSMain (/root/reference/src/shaders/PathTracer.hlsl:53-340)
// as device functions that both the validation megakernel and the wavefront kernels call:
//   primary_ray        :61-72     TraceRayStandard  RaytracingCommon.hlsli:138-198
//   shade_surface_a    :92-261    (attributes, transmission branch, emissive, NEE sample generation)
//   shade_surface_b    :264-313   (Russian roulette, BRDF lobe pick + sample, ray advance)
//   miss_sky           :315-328
// plus trace_standard / candidate_commits (the closest-hit query with its candidate branch), the three stages of one NEE light sample and
// the BRDF lobes. The visibility of an NEE shadow ray (CalculateRTShadow<true>) is pt_shadow.h, included here: every user of a path stage
// traces shadow rays too.
// NEE shadow rays draw no random numbers, so a stage may defer them: shade_surface_a hands every
// light sample to an `emit` callback (direction, distance, unshadowed diffuse/specular radiance).
#pragma once

#include "pt_device.h"
#include "pt_shadow.h"

namespace hrt {

struct PathState {
    Ray ray;
    uint32_t rng;
    f3 throughput, radiance;
    // dielectric medium the current segment travels in (PathTracer.hlsl:78-81)
    bool inVolume; float interiorIOR; f3 sigmaA, sigmaS;
};

// what shade_surface_a needs to keep for shade_surface_b
struct SurfaceCarry {
    f3 N, V, worldPos, baseColor, F0; float Fr, roughness, metallic, ior;
    uint32_t rngBeforeLights;      // RNG state at the top of the light loop (:260): lets a schedule replay the loop's draws
    uint32_t material;             // index into the material constants
};

HRT_DEV void init_path(PathState& ps, const HrptPathTracerConstants& cb, uint32_t px, uint32_t py)
{
    camera_ray(cb.m_View.m_MatClipToWorldNoOffset, cb.m_CameraPos, cb.m_Jitter[0], cb.m_Jitter[1], cb.m_View.m_ViewportSizeInv[0],
               cb.m_View.m_ViewportSizeInv[1], px, py, ps.ray.o, ps.ray.d);
    ps.ray.tmin = 0.0f; ps.ray.tmax = 1e10f;
    ps.rng = hrt_rng_seed(px, py, cb.m_AccumulationIndex);        // RNG.hlsli:21-27
    ps.throughput = mk3(1.0f, 1.0f, 1.0f); ps.radiance = mk3(0.0f, 0.0f, 0.0f);
    ps.inVolume = false; ps.interiorIOR = 1.0f; ps.sigmaA = mk3(0.0f, 0.0f, 0.0f); ps.sigmaS = mk3(0.0f, 0.0f, 0.0f);
}

// The candidate branch of TraceRayStandard (RaytracingCommon.hlsli:153-184) for a hit on a ForceNonOpaque instance:
// MASK -> AlphaTest (:91-110); BLEND -> transmissive materials always commit, others commit with probability alpha
// (one RNG draw, :181).
HRT_DEV bool candidate_commits(const SceneView& s, const Hit& h, uint32_t& rng)
{
    TriVerts tv = load_hit_attr(s, h);
    const HrptMaterialConstants& mat = s.materials[tv.material];
    uint32_t alphaMode = mat.m_AlphaMode;
    if (alphaMode == HRPT_ALPHA_MODE_MASK || (alphaMode == HRPT_ALPHA_MODE_BLEND && !(mat.m_TransmissionFactor > 0.0f))) {
        f2 uv = interpolated_uv(tv, h.u, h.v);
        float alpha = candidate_alpha(s, mat, uv);
        if (alphaMode == HRPT_ALPHA_MODE_MASK) return alpha >= mat.m_AlphaCutoff;
        return hrt_rng_next(&rng) < hrt_saturate(alpha);
    }
    return alphaMode == HRPT_ALPHA_MODE_BLEND;
}

// TraceRayStandard, RaytracingCommon.hlsli:138-198. Non-opaque candidates are visited front to back:
// a rejected candidate becomes the exclusive lower bound of the next closest-hit query.
template <class BVH, class STACK>
HRT_DEV bool trace_standard(const SceneView& s, const BVH& bvh, const Ray& ray, uint32_t& rng, STACK& stack, Hit& out)
{
    HitKey lower = hit_key_none();
    for (;;) {
        Hit h;
        if constexpr (BVH::kTwoLevel) h = closest_two_level(bvh, s.rootLeaf, s.nodeCount, ray, lower, stack);
        else h = closest_any(bvh, s.rootLeaf, s.nodeCount, ray, lower, stack);
        if (!h.valid) return false;
        if ((h.opaque & 1u) || candidate_commits(s, h, rng)) { out = h; return true; }
        hit_key_advance(lower, h);
    }
}

// One light of AccumulateDirectLighting (CommonLighting.hlsli:877-908) in three stages, so that a schedule may run the
// expensive parts where lanes are dense and skip them for occluded samples (a shadow factor of 0 contributes +0):
//   nee_draw          early-outs that precede the RNG draws (:723, :758-764, :815-833) + the two draws (:730, :776, :846)
//   nee_direction     jittered direction / distance from the draws; false when dot(N, L_s) <= 0 (no shadow ray, :731/:786/:856)
//   nee_contribution  radiance (sun: atmosphere LUT; point/spot: attenuation) + per-sample byproducts + EvaluateDirectLight
//                     without the shadow factor
// DIRONLY: the scene's light list is known to hold directional lights only (point/spot code compiled out).
// nee_draw reads no scene and lives in pt_direct.h, where the deferred stage shares its culls.
template <bool DIRONLY>
HRT_DEV bool nee_direction(const HrptGPULight& l, f3 N, f3 worldPos, f3 sunDirection, float cosSun, float ux, float uy, f3& L, float& maxDist)
{
    if (DIRONLY || l.m_Type == HRPT_LIGHT_DIRECTIONAL) {
        L = sample_cone(sunDirection, cosSun, ux, uy);
        maxDist = 1e10f;
    } else {
        float cosT = 1.0f - 2.0f * ux;
        float sinT = hrt_sqrt(hrt_max(0.0f, 1.0f - cosT * cosT));
        float phi = 2.0f * HRT_PI * uy;
        float sp, cp; hrt_sincos(phi, &sp, &cp);
        f3 sphereDir = mk3(sinT * cp, cosT, sinT * sp);
        f3 samplePos = mk3(l.m_Position) + sphereDir * l.m_Radius;
        f3 toSample = samplePos - worldPos;
        float sampleDist = length(toSample);
        L = toSample / sampleDist;
        maxDist = sampleDist;
    }
    return !(dot(N, L) <= 0.0f);
}

template <bool DIRONLY>
HRT_DEV void nee_contribution(const SceneView& s, const HrptGPULight& l, Lighting in, f3 worldPos, f3 sunDirection, float sunIntensity, f3 L,
                              f3& diffuse, f3& specular)
{
    f3 radiance;
    if (DIRONLY || l.m_Type == HRPT_LIGHT_DIRECTIONAL) {
        // inputs.sunRadiance (PathTracer.hlsl:137): a pure function of the hit position, read only by directional lights
        radiance = atm::sun_radiance(s, atm::atmosphere_pos(worldPos), sunDirection, sunIntensity);
    } else {
        // deferred::light_radiance (pt_deferred.h) is a deliberate copy of this branch: DESIGN.md section 27
        f3 toLight = mk3(l.m_Position) - worldPos;
        float distSq = dot(toLight, toLight);
        float dist = hrt_sqrt(distSq);
        float att = distance_attenuation(l, distSq, dist);
        f3 col = mk3(l.m_Color);
        if (l.m_Type == HRPT_LIGHT_SPOT) {
            f3 Lc = toLight / dist;
            f3 lightDir = normalize(mk3(l.m_Direction));
            float cosTheta = dot(-Lc, lightDir);
            float cosOuter = hrt_cos(l.m_SpotOuterConeAngle), cosInner = hrt_cos(l.m_SpotInnerConeAngle);
            float spotAtt = hrt_saturate((cosTheta - cosOuter) / (cosInner - cosOuter));
            radiance = ((col * l.m_Intensity) * spotAtt) * att;
        } else radiance = (col * l.m_Intensity) * att;
    }
    in.L = L;
    prepare_byproducts(in);
    evaluate_direct_unshadowed(in, radiance, diffuse, specular);
}

HRT_DEV HrptGPULight load_light(const SceneView& s, uint32_t i)
{
    if (i < s.lightCount) return s.lights[i];
    HrptGPULight l = HrptGPULight(); l.m_Type = 0;   // out-of-range structured-buffer read returns zeros on D3D12
    return l;
}

enum SurfaceOutcome { SURFACE_TRANSMITTED = 0, SURFACE_SCATTER = 1 };

// PathTracer.hlsl:92-261 up to the light loop. EMIT(lightIndex, ux, uy) receives the two random numbers of every light
// that passed nee_draw (carry is filled before the first call); the caller runs nee_direction, the shadow query and
// nee_contribution, and owes  radiance += throughput * (sum(diffuse_i*shadow_i) + (bounce==0 ? sum(specular_i*shadow_i) : 0)).
// Compile-time scene traits (all-true / DIRONLY=false is the general form and always correct):
//   TEX     some material samples a texture          (false: every m_TextureFlags is 0 -> sampling code compiled out)
//   TRANS   some material is transmissive or BLEND   (false: the transmission branch :149-255 is compiled out)
//   DIRONLY every light is directional               (true: point / spot code compiled out)
// TABLES: where the triangle, instance and material records are read from (pt_shade_tables.h GlobalShadeTables / LdsShadeTables)
template <bool TEX, bool TRANS, bool DIRONLY, class TABLES, class EMIT>
HRT_DEV SurfaceOutcome shade_surface_a(const SceneView& s, const TABLES& tables, const HrptPathTracerConstants& cb, PathState& ps, const Hit& hit,
                                       SurfaceCarry& carry, EMIT&& emit)
{
    TriVerts tv = tables.hit_attr(hit);                                           // inst/mesh/vertex fetch :92-94,:104 (LOD 0, :103)
    GpuInstShade is = tables.inst_shade(tv.inst);
    const HrptMaterialConstants& mat = tables.material(tv.material);
    uint32_t texFlags = TEX ? mat.m_TextureFlags : 0u;

    if (TRANS && ps.inVolume) {                                                            // Beer-Lambert :97-100
        f3 tr = mk3(hrt_exp(-(ps.sigmaA.x + ps.sigmaS.x) * hit.t), hrt_exp(-(ps.sigmaA.y + ps.sigmaS.y) * hit.t),
                    hrt_exp(-(ps.sigmaA.z + ps.sigmaS.z) * hit.t));
        ps.throughput = ps.throughput * tr;
    }
    SurfaceAttr attr = full_hit_attributes(s, hit, ps.ray, tv, is, (texFlags & HRPT_TEXFLAG_NORMAL) != 0);
    Pbr pbr = pbr_attributes(s, attr, mat, texFlags);

    f3 Ng = normalize(attr.worldNormal);
    f3 N = pbr.normal;
    f3 V = -ps.ray.d;
    bool isFrontFace = dot(Ng, ps.ray.d) < 0.0f;
    if (dot(N, V) < 0.0f) N = -N;

    f3 sunDir = mk3(cb.m_SunDirection[0], cb.m_SunDirection[1], cb.m_SunDirection[2]);

    Lighting in;
    in.N = N; in.V = V; in.L = mk3(0.0f, 0.0f, 0.0f); in.baseColor = pbr.baseColor;
    in.roughness = pbr.roughness; in.metallic = pbr.metallic; in.ior = mat.m_IOR;
    prepare_byproducts(in);                                                       // :142 (L = 0 => H = V)

    HRT_PHASE(PH_SHADE_ATTR);
    if (TRANS && (mat.m_TransmissionFactor > 0.0f || mat.m_AlphaMode == HRPT_ALPHA_MODE_BLEND)) {    // :149-255
        HRT_PHASE(PH_SHADE_TRANS);
        float effectiveAlpha = (mat.m_AlphaMode == HRPT_ALPHA_MODE_BLEND) ? pbr.alpha : 1.0f;
        float transmissionFactor = hrt_max(mat.m_TransmissionFactor, 1.0f - effectiveAlpha);
        float materialIOR = hrt_max(mat.m_IOR, 1.0001f);
        float outsideIOR = ps.inVolume ? ps.interiorIOR : 1.0f;
        float etaSurface = isFrontFace ? (outsideIOR / materialIOR) : (materialIOR / outsideIOR);
        float etaFresnel = etaSurface;
        float etaRefract = (mat.m_IsThinSurface != 0) ? 1.0f : etaFresnel;
        float cosT_geo;
        float F = fresnel_dielectric(etaFresnel, hrt_max(dot(N, V), 0.0f), cosT_geo);
        float probT = hrt_saturate((1.0f - F) * transmissionFactor);
        if (hrt_rng_next(&ps.rng) < probT) {
            f3 refractedDir, bsdfWeight;
            if (pbr.roughness <= 0.08f) {
                refractedDir = refract(ps.ray.d, N, etaRefract);
                if (dot(refractedDir, refractedDir) < 1e-8f) refractedDir = reflect(ps.ray.d, N);
                bsdfWeight = pbr.baseColor;
            } else {
                float ux = hrt_rng_next(&ps.rng), uy = hrt_rng_next(&ps.rng);
                f3 H = sample_ggx_vndf(ux, uy, N, V, pbr.roughness);
                float VdotH = hrt_saturate(dot(V, H));
                float cosT_mf; float F_mf = fresnel_dielectric(etaFresnel, VdotH, cosT_mf);
                float cosT_dir; fresnel_dielectric(etaRefract, VdotH, cosT_dir);
                refractedDir = H * (etaRefract * VdotH - cosT_dir) - V * etaRefract;
                if (dot(refractedDir, refractedDir) < 1e-8f) refractedDir = reflect(ps.ray.d, H);
                refractedDir = normalize(refractedDir);
                float alpha = pbr.roughness * pbr.roughness, alpha2 = alpha * alpha;
                float NdotL_t = hrt_abs(dot(N, refractedDir));
                float G1_t = (NdotL_t > HRT_K_EPSILON) ? 2.0f * NdotL_t / (NdotL_t + hrt_sqrt(alpha2 + (1.0f - alpha2) * NdotL_t * NdotL_t)) : 0.0f;
                bsdfWeight = ((pbr.baseColor * (1.0f - F_mf)) * G1_t) * NdotL_t;
            }
            ps.throughput = ps.throughput * bsdfWeight;
            if (mat.m_IsThinSurface == 0) {
                if (isFrontFace) { ps.inVolume = true; ps.interiorIOR = materialIOR; ps.sigmaA = mk3(mat.m_SigmaA); ps.sigmaS = mk3(mat.m_SigmaS); }
                else { ps.inVolume = false; ps.interiorIOR = 1.0f; ps.sigmaA = mk3(0.0f, 0.0f, 0.0f); ps.sigmaS = mk3(0.0f, 0.0f, 0.0f); }
            }
            ps.ray.o = attr.worldPos - N * 0.001f;
            ps.ray.d = normalize(refractedDir);
            ps.ray.tmin = 1e-4f; ps.ray.tmax = 1e10f;
            return SURFACE_TRANSMITTED;
        }
    }

    ps.radiance = ps.radiance + ps.throughput * pbr.emissive;                     // :258

    carry.N = N; carry.V = V; carry.worldPos = attr.worldPos; carry.baseColor = pbr.baseColor; carry.F0 = in.F0;
    carry.Fr = in.F.x; carry.roughness = pbr.roughness; carry.metallic = pbr.metallic; carry.ior = mat.m_IOR;
    carry.rngBeforeLights = ps.rng; carry.material = tv.material;
    HRT_PHASE(PH_SHADE_NEE);
    for (uint32_t i = 0; i < cb.m_LightCount; ++i) {                              // AccumulateDirectLighting :260
        HrptGPULight l = load_light(s, i);
        float ux, uy;
        if (nee_draw<DIRONLY>(l, N, attr.worldPos, sunDir, ps.rng, ux, uy)) emit(i, ux, uy);
    }
    return SURFACE_SCATTER;
}

// PathTracer.hlsl:264-313 in three pieces so that a wave can run the (rare, long) specular lobe for many paths at once:
//   lobe_begin     Russian roulette :264-270, lobe pick :275-280 and what both lobes share (two draws, one sincos, one sqrt)
//   lobe_diffuse   cosine-weighted sample + weight :295-304, ray advance :306-313
//   lobe_specular  GGX-VNDF sample + weight :281-294, ray advance :306-313
// shade_surface_b strings them together (validation megakernel, general wavefront variants). Values and operation order per path
// are those of the reference in every arrangement.
struct LobeDraw { float specProb, root, sp, cp; bool spec; };

HRT_DEV bool lobe_begin(PathState& ps, const SurfaceCarry& c, int bounce, LobeDraw& ld)
{
    HRT_PHASE(PH_SHADE_LOBE_BEGIN);
    if (bounce >= 2) {                                                            // Russian roulette :264-270
        float continuePr = hrt_saturate(maxcomp(ps.throughput));
        if (hrt_rng_next(&ps.rng) > continuePr) return false;
        ps.throughput = ps.throughput / continuePr;
    }
    ld.specProb = hrt_clamp(lerp(c.Fr * 0.5f + 0.5f * c.metallic, 1.0f, c.metallic), 0.1f, 0.9f);   // :275
    ld.spec = hrt_rng_next(&ps.rng) < ld.specProb;
    const float ux = hrt_rng_next(&ps.rng), uy = hrt_rng_next(&ps.rng);
    hrt_sincos(2.0f * HRT_PI * (ld.spec ? uy : ux), &ld.sp, &ld.cp);
    ld.root = hrt_sqrt(ld.spec ? ux : uy);
    return true;
}
HRT_DEV bool lobe_finish(PathState& ps, f3 worldPos, f3 N, f3 newDir, f3 numer, float denom)
{
    if (dot(N, newDir) <= 0.0f) return false;
    f3 brdfWeight = numer / denom;
    ps.throughput = ps.throughput * brdfWeight;
    if (maxcomp(ps.throughput) < 0.01f) return false;                             // :306
    ps.ray.o = worldPos; ps.ray.d = newDir; ps.ray.tmin = 1e-4f; ps.ray.tmax = 1e10f;   // :310-313
    return true;
}
HRT_DEV bool lobe_diffuse(PathState& ps, f3 worldPos, f3 N, f3 baseColor, float metallic, const LobeDraw& ld)
{
    HRT_PHASE(PH_SHADE_DIFFUSE);
    f3 T, B; tangent_frame(N, T, B);
    f3 newDir = sample_hemisphere_cosine_from(ld.root, ld.sp, ld.cp, T, B, N);
    return lobe_finish(ps, worldPos, N, newDir, baseColor * (1.0f - metallic), 1.0f - ld.specProb);
}
HRT_DEV bool lobe_specular(PathState& ps, f3 worldPos, f3 N, f3 V, f3 F0, float roughness, const LobeDraw& ld)
{
    HRT_PHASE(PH_SHADE_SPEC);
    f3 T, B; tangent_frame(N, T, B);
    f3 H = sample_ggx_vndf_from(ld.root, ld.sp, ld.cp, T, B, N, V, roughness);
    f3 newDir = reflect(-V, H);
    if (dot(N, newDir) <= 0.0f) return false;       // before the weight, as in the reference (:289)
    return lobe_finish(ps, worldPos, N, newDir, eval_ggx_vndf_weight(F0, N, V, newDir, H, roughness), ld.specProb);
}
HRT_DEV bool shade_surface_b(PathState& ps, const SurfaceCarry& c, int bounce)
{
    LobeDraw ld;
    if (!lobe_begin(ps, c, bounce, ld)) return false;
    return ld.spec ? lobe_specular(ps, c.worldPos, c.N, c.V, c.F0, c.roughness, ld) : lobe_diffuse(ps, c.worldPos, c.N, c.baseColor, c.metallic, ld);
}

// What hrpt_trace_radiance leaves in a ray's slot: (L, 1), or with `accumulate` (old.rgb + L, old.w + 1) -- the addition of
// PathTracer.hlsl:332-337 for an index above 0. A ray that was not traced (non-finite record) stores zeros, or with `accumulate` nothing.
HRT_DEV void store_ray_radiance(float4* slot, f3 L, bool traced, bool accumulate)
{
    float4 cur = traced ? make_float4(L.x, L.y, L.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (accumulate) {
        if (!traced) return;
        const float4 prev = *slot;
        cur.x += prev.x; cur.y += prev.y; cur.z += prev.z; cur.w += prev.w;
    }
    *slot = cur;
}

// PathTracer.hlsl:315-328
HRT_DEV void miss_sky(const SceneView& s, const HrptPathTracerConstants& cb, PathState& ps, int bounce)
{
    HRT_PHASE(PH_SHADE_SKY);
    f3 sunDir = mk3(cb.m_SunDirection[0], cb.m_SunDirection[1], cb.m_SunDirection[2]);
    f3 sky = atm::sky_radiance(s, ps.ray.o, ps.ray.d, sunDir, s.lights[0].m_Intensity, bounce == 0);
    ps.radiance = ps.radiance + ps.throughput * sky;
}

// A per-lane count (rays, paths) summed over the 64 lanes of the wave: the statistics of both pipelines.
HRT_DEV unsigned long long wave_sum_u32(unsigned int v)
{
    unsigned long long x = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

} // namespace hrt

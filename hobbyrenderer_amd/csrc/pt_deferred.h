// pt_deferred.h -- the arithmetic of hrpt_deferred_lighting, one __host__ __device__ source shared by the gfx950 kernels (pt_deferred.hip)
// and hrpt_deferred_rays_host / hrpt_deferred_shade_host (pt_deferred_host.cpp): the reference's DeferredLighting.hlsl with
// AccumulateDirectLighting (src/shaders/CommonLighting.hlsli:501-603) over the path tracer's own first-hit planes. It is the deterministic
// counterpart of the path tracer's bounce-0 direct light, so the primary ray (init_path), the culls, direction and radiance of a light sample
// (nee_draw / nee_direction at radius 0 / nee_contribution, pt_path.h), distance_attenuation (pt_surface.h) and prepare_byproducts +
// evaluate_direct_unshadowed (pt_lighting.h) are RESTATED here statement for statement over pt_image.h's types: those headers sit on the HIP
// runtime and cannot be built by the host-only sanitizer program, and sharing them would have meant touching files every path kernel
// includes. Arithmetic of hobbyrt/detmath.h: no FMA contraction, correctly rounded '/' and sqrt, select-form min / max, sums and dot
// products left to right; normalize(v) = v * (1 / sqrt(dot(v, v))) as pt_vec.h has it (NOT img::normalize). DESIGN.md section 27 has the
// definition in prose.
//
// What does not live here: the atmosphere (sun_radiance at X, sky_radiance along a missed ray) and the shadow query. The functions below take
// them as callables (`sun`, `vis`) and values, so the kernel computes the former from the scene's tables and reads the latter from the hit
// records of hrpt_trace_rays, while the host executors read both from images.
//
// Differences from DeferredLighting.hlsl, on purpose:
//   * X = o + d * t and V = -d come from the primary ray and the plane's t, not from a depth reconstruction at the pixel centre: with a
//     jittered G-buffer the reconstruction leaves the surface by more than the 0.01 shadow bias on slanted surfaces
//   * the sun's shadow goes through CalculateRTShadow<true>, like the path tracer's own sun sample, not the plain form (they differ only
//     behind BLEND surfaces)
//   * point lights are lit (the reference's raster loop skips type 1); m_Radius is ignored, so shadows are hard
//   * ior = 1.5f for every surface (the reference's deferred constant)
//   * not reproduced: the CSM mask of NORMAL_BASIC, IBL mode, the ReSTIR / SHARC / SSGI inputs, the debug views
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_image.h"

namespace hrt {
namespace deferred {

using img::T3;
using img::T4;
using img::t3;
using img::t4;
using img::dot3;
using img::add;
using img::sub;
using img::neg;
using img::load4;

constexpr float kIor = 1.5f;
constexpr float kInvPi = 0.31830988618f;
constexpr float kSunDistance = 1e10f;
constexpr uint32_t kAllFlags = HRPT_DEFERRED_SHADOWS | HRPT_DEFERRED_SKY | HRPT_DEFERRED_INDIRECT;
constexpr uint32_t kMaxBatch = 16;

// What the stage reads of an HrptPathTracerConstants and an HrptDeferredParams, gathered once per call.
struct Frame {
    float clipToWorld[16];      // m_View.m_MatClipToWorldNoOffset
    float cam[3];               // m_CameraPos.xyz
    float jitter[2], sizeInv[2];
    float sun[3];               // m_SunDirection
    float sunIntensity;         // I0 = lights[0].m_Intensity, 0 with an empty list (device path; the host executors get images)
    float indirectIntensity;
    uint32_t flags;
    int w, h;
};
HRT_FN Frame make_frame(const HrptPathTracerConstants& cb, const HrptDeferredParams& p, float sunIntensity, int w, int h)
{
    Frame f;
    for (int i = 0; i < 16; ++i) f.clipToWorld[i] = cb.m_View.m_MatClipToWorldNoOffset[i];
    for (int i = 0; i < 3; ++i) { f.cam[i] = cb.m_CameraPos[i]; f.sun[i] = cb.m_SunDirection[i]; }
    for (int i = 0; i < 2; ++i) { f.jitter[i] = cb.m_Jitter[i]; f.sizeInv[i] = cb.m_View.m_ViewportSizeInv[i]; }
    f.sunIntensity = sunIntensity; f.indirectIntensity = p.indirectIntensity; f.flags = p.flags;
    f.w = w; f.h = h;
    return f;
}

HRT_FN T3 scale(T3 a, float s) { return t3(a.x * s, a.y * s, a.z * s); }
HRT_FN T3 over(T3 a, float s) { return t3(a.x / s, a.y / s, a.z / s); }
HRT_FN T3 mul(T3 a, T3 b) { return t3(a.x * b.x, a.y * b.y, a.z * b.z); }
HRT_FN T3 unit(T3 a) { const float inv = 1.0f / hrt_sqrt(dot3(a, a)); return scale(a, inv); }      // pt_vec.h normalize
HRT_FN float mix(float a, float b, float t) { return a + t * (b - a); }                              // pt_vec.h lerp

// The primary ray of init_path (pt_path.h:34-48; PathTracer.hlsl:61-72): no RNG.
HRT_FN void primary_ray(const Frame& f, int px, int py, T3* o, T3* d)
{
    const float u = (((float)px + 0.5f) + f.jitter[0]) * f.sizeInv[0];
    const float v = (((float)py + 0.5f) + f.jitter[1]) * f.sizeInv[1];
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;
    const float* M = f.clipToWorld;
    const float ex = ((cx * M[0] + cy * M[4]) + 0.9f * M[8]) + 1.0f * M[12];
    const float ey = ((cx * M[1] + cy * M[5]) + 0.9f * M[9]) + 1.0f * M[13];
    const float ez = ((cx * M[2] + cy * M[6]) + 0.9f * M[10]) + 1.0f * M[14];
    const float ew = ((cx * M[3] + cy * M[7]) + 0.9f * M[11]) + 1.0f * M[15];
    const T3 end = t3(ex / ew, ey / ew, ez / ew);
    *o = t3(f.cam[0], f.cam[1], f.cam[2]);
    *d = unit(sub(end, *o));
}
HRT_FN T3 hit_position(T3 o, T3 d, float t) { return t3(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t); }

// The surface terms of a hit (nee_lighting, pt_path.h) with what prepare_byproducts derives from them alone.
struct Surface { T3 N, V, baseColor; float roughness, metallic; };
HRT_FN Surface make_surface(T4 albedo, T4 normal, float metallic, T3 d)
{
    Surface s;
    s.N = t3(normal.x, normal.y, normal.z); s.V = neg(d); s.baseColor = t3(albedo.x, albedo.y, albedo.z);
    s.roughness = normal.w; s.metallic = metallic;
    return s;
}

// ---- one light: cull + direction (nee_draw without its two draws, nee_direction at radius 0) ------------------------------------------
// false: the pair is unlit -- no shadow ray, no contribution.
HRT_FN bool light_direction(const HrptGPULight& l, T3 N, T3 X, T3 sunDir, T3* L, float* maxDist)
{
    if (l.m_Type == HRPT_LIGHT_DIRECTIONAL) {
        if (dot3(N, sunDir) <= 0.0f) return false;
        *L = sunDir; *maxDist = kSunDistance;
        return true;
    }
    if (l.m_Type != HRPT_LIGHT_POINT && l.m_Type != HRPT_LIGHT_SPOT) return false;
    if (l.m_Intensity <= 0.0f) return false;
    const T3 toLight = sub(t3(l.m_Position[0], l.m_Position[1], l.m_Position[2]), X);
    const float distSq = dot3(toLight, toLight);
    if (l.m_Range > 0.0f && distSq > l.m_Range * l.m_Range) return false;
    const float dist = hrt_sqrt(distSq);
    const T3 Lc = over(toLight, dist);
    if (l.m_Type == HRPT_LIGHT_SPOT) {
        if (dot3(N, Lc) <= 0.0f) return false;
        const T3 lightDir = unit(t3(l.m_Direction[0], l.m_Direction[1], l.m_Direction[2]));
        const float cosTheta = dot3(neg(Lc), lightDir);
        if (cosTheta < hrt_cos(l.m_SpotOuterConeAngle)) return false;
    }
    *L = Lc; *maxDist = dist;
    return !(dot3(N, Lc) <= 0.0f);
}

// ---- radiance of a point or spot light at X (nee_contribution; distance_attenuation of pt_surface.h) -----------------------------------
HRT_FN T3 light_radiance(const HrptGPULight& l, T3 X)
{
    const T3 toLight = sub(t3(l.m_Position[0], l.m_Position[1], l.m_Position[2]), X);
    const float distSq = dot3(toLight, toLight);
    const float dist = hrt_sqrt(distSq);
    float att = 1.0f / (distSq + 1.0f);
    if (l.m_Range > 0.0f) {
        const float q = dist / l.m_Range; const float q2 = q * q; const float q4 = q2 * q2;
        const float sa = hrt_saturate(1.0f - q4);
        att = att * (sa * sa);
    }
    const T3 col = t3(l.m_Color[0], l.m_Color[1], l.m_Color[2]);
    if (l.m_Type == HRPT_LIGHT_SPOT) {
        const T3 Lc = over(toLight, dist);
        const T3 lightDir = unit(t3(l.m_Direction[0], l.m_Direction[1], l.m_Direction[2]));
        const float cosTheta = dot3(neg(Lc), lightDir);
        const float cosOuter = hrt_cos(l.m_SpotOuterConeAngle), cosInner = hrt_cos(l.m_SpotInnerConeAngle);
        const float spotAtt = hrt_saturate((cosTheta - cosOuter) / (cosInner - cosOuter));
        return scale(scale(scale(col, l.m_Intensity), spotAtt), att);
    }
    return scale(scale(col, l.m_Intensity), att);
}
// A directional light without the atmosphere (the reference's useSunRadiance == false)
HRT_FN T3 light_color(const HrptGPULight& l) { return scale(t3(l.m_Color[0], l.m_Color[1], l.m_Color[2]), l.m_Intensity); }

// ---- prepare_byproducts + evaluate_direct_unshadowed (pt_lighting.h; CommonLighting.hlsli:316-375) --------------------------------------
HRT_FN float burley_diffuse(float NdotL, float NdotV, float LdotH, float rough)
{
    if (NdotL <= 0.0f || NdotV <= 0.0f) return 0.0f;
    const float rough2 = rough * rough;
    const float FL = hrt_pow5(1.0f - NdotL), FV = hrt_pow5(1.0f - NdotV);
    const float Fd90 = 0.5f + 2.0f * rough2 * LdotH * LdotH;
    const float Fd = mix(1.0f, Fd90, FL) * mix(1.0f, Fd90, FV);
    return Fd * NdotL / HRT_PI;
}
HRT_FN void direct_light(const Surface& s, T3 L, T3 radiance, T3* diffuse, T3* specular)
{
    const float NdotV = hrt_saturate(dot3(s.N, s.V));
    const float NdotL = hrt_saturate(dot3(s.N, L));
    const T3 VpL = add(s.V, L);
    const float len = dot3(VpL, VpL);
    const T3 H = (len > 1e-8f) ? scale(VpL, hrt_rsqrt(len)) : s.N;
    const float NdotH = hrt_saturate(dot3(s.N, H));
    const float VdotH = hrt_saturate(dot3(s.V, H));
    const float LdotH = hrt_saturate(dot3(L, H));
    // compute_f0 with ior = 1.5f
    const float q = (kIor - 1.0f) / (kIor + 1.0f);
    const float d0 = q * q;
    const T3 F0 = t3(mix(d0, s.baseColor.x, s.metallic), mix(d0, s.baseColor.y, s.metallic), mix(d0, s.baseColor.z, s.metallic));
    const float kD = 1.0f - s.metallic;
    // f_schlick
    const float Fc = hrt_pow5(1.0f - VdotH);
    const float fs = hrt_saturate(50.0f * F0.y) * Fc;
    const float fk = 1.0f - Fc;
    const T3 F = t3(fs + fk * F0.x, fs + fk * F0.y, fs + fk * F0.z);
    // evaluate_direct_unshadowed
    const float dt = burley_diffuse(NdotL, NdotV, LdotH, s.roughness);
    const T3 dif = mul(scale(t3(kD, kD, kD), dt), s.baseColor);
    const float alpha = s.roughness * s.roughness, alpha2 = alpha * alpha;
    const float denom = NdotH * NdotH * (alpha2 - 1.0f) + 1.0f;                       // d_ggx
    const float D = alpha2 / (HRT_PI * denom * denom);
    const float g1 = NdotV * hrt_sqrt(alpha2 + (1.0f - alpha2) * NdotL * NdotL);
    const float g2 = NdotL * hrt_sqrt(alpha2 + (1.0f - alpha2) * NdotV * NdotV);
    const float G2 = 0.5f / hrt_max(g1 + g2, 1e-6f);
    const float k = D * G2;
    const T3 spec = scale(F, k);
    *diffuse = mul(dif, radiance);
    *specular = mul(scale(spec, NdotL), radiance);
}

// ---- the shadow-ray record of one (light, pixel) pair: three 16-byte rows of an HrptRay -----------------------------------------------
HRT_FN void ray_rows(bool lit, T3 X, T3 L, float maxDist, T4 rows[3])
{
    const float nan = hrt_u2f(0x7FC00000u);
    rows[0] = lit ? t4(X.x, X.y, X.z, 0.0f) : t4(nan, nan, nan, 0.0f);
    rows[1] = lit ? t4(L.x, L.y, L.z, maxDist) : t4(0.0f, 0.0f, 0.0f, 0.0f);
    rows[2] = t4(0.0f, 0.0f, 0.0f, 0.0f);                                            // rng 0, pad 0
}
// The record of light `l` at a pixel whose depth texel is D and normal texel N4.
HRT_FN void pixel_ray(const Frame& f, const HrptGPULight& l, T4 D, T4 N4, int px, int py, T4 rows[3])
{
    T3 L = t3(0.0f, 0.0f, 0.0f), X = L;
    float maxDist = 0.0f;
    bool lit = false;
    if (!(D.x == img::kMissDepth)) {
        T3 o, d;
        primary_ray(f, px, py, &o, &d);
        X = hit_position(o, d, D.x);
        lit = light_direction(l, t3(N4.x, N4.y, N4.z), X, t3(f.sun[0], f.sun[1], f.sun[2]), &L, &maxDist);
    }
    ray_rows(lit, X, L, maxDist, rows);
}

// ---- lights [first, first + count) of a hit added into the running sums, in order ----------------------------------------------------
// sun(l): radiance of the directional light l at X; vis(j): visibility of the pair of light first + j, read for lit pairs only.
template <class SUN, class VIS>
HRT_FN void add_lights(const Surface& s, T3 X, T3 sunDir, const HrptGPULight* lights, uint32_t first, uint32_t count, SUN sun, VIS vis, T3* totalD, T3* totalS)
{
    for (uint32_t j = 0; j < count; ++j) {
        const HrptGPULight& l = lights[first + j];
        T3 L; float maxDist;
        if (!light_direction(l, s.N, X, sunDir, &L, &maxDist)) continue;
        const T3 radiance = l.m_Type == HRPT_LIGHT_DIRECTIONAL ? sun(l) : light_radiance(l, X);
        T3 dif, spec;
        direct_light(s, L, radiance, &dif, &spec);
        const float v = vis(j);
        *totalD = add(*totalD, scale(dif, v));
        *totalS = add(*totalS, scale(spec, v));
    }
}

// Steps 5-7 of a hit: emissive, the optional diffuse indirect term, alpha.
HRT_FN T4 finish_hit(const Frame& f, T4 A, T4 E, float metallic, T3 totalD, T3 totalS, T4 irr)
{
    T3 rgb = add(add(totalD, totalS), t3(E.x, E.y, E.z));
    if ((f.flags & HRPT_DEFERRED_INDIRECT) && irr.w == 1.0f) {
        const T3 ind = scale(scale(scale(mul(t3(irr.x, irr.y, irr.z), t3(A.x, A.y, A.z)), 1.0f - metallic), kInvPi), f.indirectIntensity);
        rgb = add(rgb, ind);
    }
    return t4(rgb.x, rgb.y, rgb.z, A.w);
}

HRT_FN bool params_valid(const HrptDeferredParams& p)
{
    return (p.flags & ~kAllFlags) == 0u && p.reserved[0] == 0u && p.reserved[1] == 0u && (p.indirectIntensity - p.indirectIntensity) == 0.0f;
}

} // namespace deferred
} // namespace hrt

// pt_deferred.h -- the arithmetic of hrpt_deferred_lighting, one __host__ __device__ source shared by the gfx950 kernels (pt_deferred.hip)
// and hrpt_deferred_rays_host / hrpt_deferred_shade_host (pt_deferred_host.cpp): the reference's DeferredLighting.hlsl with
// AccumulateDirectLighting (src/shaders/CommonLighting.hlsli:501-603) over the path tracer's own first-hit planes. It is the deterministic
// counterpart of the path tracer's bounce-0 direct light and CALLS the path tracer's functions: camera_ray (the primary ray of init_path),
// nee_draw (for its culls), distance_attenuation and nee_lighting of pt_direct.h, prepare_byproducts + evaluate_direct_unshadowed of
// pt_lighting.h, over pt_vec.h's f3. Stated here: the direction towards a light's centre (nee_direction at radius 0) and, still as a copy,
// the point / spot radiance of nee_contribution (light_radiance below says why). pt_image.h's T4 / load4 remain for texels. DESIGN.md
// section 27 has the definition in prose.
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
#include "pt_direct.h"
#include "pt_image.h"

namespace hrt {
namespace deferred {

using img::T4;
using img::t4;
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

HRT_FN f3 xyz(T4 a) { return mk3(a.x, a.y, a.z); }
// The primary ray of init_path (pt_path.h) for the frame's constants: no RNG.
HRT_FN void frame_ray(const Frame& f, int px, int py, f3& o, f3& d)
{
    camera_ray(f.clipToWorld, f.cam, f.jitter[0], f.jitter[1], f.sizeInv[0], f.sizeInv[1], (uint32_t)px, (uint32_t)py, o, d);
}
// The surface terms of a hit: albedo and normal texels (roughness in normal.w), the metallic of the geometric-normal plane, V = -d.
HRT_FN Lighting make_surface(T4 albedo, T4 normal, float metallic, f3 d) { return nee_lighting(xyz(normal), -d, xyz(albedo), normal.w, metallic, kIor); }

// ---- one light: cull + direction (nee_draw without its two draws, nee_direction towards the light's centre) ---------------------------
// false: the pair is unlit -- no shadow ray, no contribution.
HRT_FN bool light_direction(const HrptGPULight& l, f3 N, f3 X, f3 sunDir, f3& L, float& maxDist)
{
    // The culls are nee_draw's (pt_direct.h, which promises that they come before its draws). The stage is deterministic: the two draws go
    // to a throw-away RNG state and are not read.
    uint32_t rng = 0u; float ux, uy;
    if (l.m_Type == HRPT_LIGHT_DIRECTIONAL) {
        L = sunDir; maxDist = kSunDistance;
        return nee_draw<false>(l, N, X, sunDir, rng, ux, uy);                      // its cull is dot(N, L) <= 0
    }
    // The direction ahead of the culls: nee_draw's spot cull and light_radiance need the same toLight / dist, and computed here, where it
    // comes before both on every path, the compiler keeps one copy (a square root and three divisions per pair otherwise).
    const f3 toLight = mk3(l.m_Position) - X;
    const float dist = hrt_sqrt(dot(toLight, toLight));
    L = toLight / dist; maxDist = dist;
    if (!nee_draw<false>(l, N, X, sunDir, rng, ux, uy)) return false;
    return !(dot(N, L) <= 0.0f);
}
// Radiance of a point or spot light at X: a deliberate copy of the `else` branch of nee_contribution (pt_path.h), statement for statement and
// with its names -- the one piece of the light model this header restates (nee_contribution reads a SceneView).
HRT_FN f3 light_radiance(const HrptGPULight& l, f3 X)
{
    f3 toLight = mk3(l.m_Position) - X;
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
        return ((col * l.m_Intensity) * spotAtt) * att;
    }
    return (col * l.m_Intensity) * att;
}
// A directional light without the atmosphere (the reference's useSunRadiance == false)
HRT_FN f3 light_color(const HrptGPULight& l) { return mk3(l.m_Color) * l.m_Intensity; }

// ---- the shadow-ray record of one (light, pixel) pair: three 16-byte rows of an HrptRay -----------------------------------------------
HRT_FN void ray_rows(bool lit, f3 X, f3 L, float maxDist, T4 rows[3])
{
    const float nan = hrt_u2f(0x7FC00000u);
    rows[0] = lit ? t4(X.x, X.y, X.z, 0.0f) : t4(nan, nan, nan, 0.0f);
    rows[1] = lit ? t4(L.x, L.y, L.z, maxDist) : t4(0.0f, 0.0f, 0.0f, 0.0f);
    rows[2] = t4(0.0f, 0.0f, 0.0f, 0.0f);                                            // rng 0, pad 0
}
// The record of light `l` at a pixel whose depth texel is D and normal texel N4.
HRT_FN void pixel_ray(const Frame& f, const HrptGPULight& l, T4 D, T4 N4, int px, int py, T4 rows[3])
{
    f3 L = mk3(0.0f, 0.0f, 0.0f), X = L;
    float maxDist = 0.0f;
    bool lit = false;
    if (!(D.x == img::kMissDepth)) {
        f3 o, d;
        frame_ray(f, px, py, o, d);
        X = o + d * D.x;
        lit = light_direction(l, xyz(N4), X, mk3(f.sun), L, maxDist);
    }
    ray_rows(lit, X, L, maxDist, rows);
}

// ---- lights [first, first + count) of a hit added into the running sums, in order ----------------------------------------------------
// sun(l): radiance of the directional light l at X; vis(j): visibility of the pair of light first + j, read for lit pairs only. A lit pair
// is evaluated as nee_contribution (pt_path.h) does it: in.L = L, prepare_byproducts, evaluate_direct_unshadowed.
template <class SUN, class VIS>
HRT_FN void add_lights(Lighting in, f3 X, f3 sunDir, const HrptGPULight* lights, uint32_t first, uint32_t count, SUN sun, VIS vis, f3& totalD, f3& totalS)
{
    for (uint32_t j = 0; j < count; ++j) {
        const HrptGPULight& l = lights[first + j];
        f3 L; float maxDist;
        if (!light_direction(l, in.N, X, sunDir, L, maxDist)) continue;
        const f3 radiance = l.m_Type == HRPT_LIGHT_DIRECTIONAL ? sun(l) : light_radiance(l, X);
        f3 dif, spec;
        in.L = L;
        prepare_byproducts(in);
        evaluate_direct_unshadowed(in, radiance, dif, spec);
        const float v = vis(j);
        totalD = totalD + dif * v;
        totalS = totalS + spec * v;
    }
}

// Steps 5-7 of a hit: emissive, the optional diffuse indirect term, alpha.
HRT_FN T4 finish_hit(const Frame& f, T4 A, T4 E, float metallic, f3 totalD, f3 totalS, T4 irr)
{
    f3 rgb = (totalD + totalS) + xyz(E);
    if ((f.flags & HRPT_DEFERRED_INDIRECT) && irr.w == 1.0f) rgb = rgb + (((xyz(irr) * xyz(A)) * (1.0f - metallic)) * kInvPi) * f.indirectIntensity;
    return t4(rgb.x, rgb.y, rgb.z, A.w);
}

HRT_FN bool params_valid(const HrptDeferredParams& p)
{
    return (p.flags & ~kAllFlags) == 0u && p.reserved[0] == 0u && p.reserved[1] == 0u && (p.indirectIntensity - p.indirectIntensity) == 0.0f;
}

} // namespace deferred
} // namespace hrt

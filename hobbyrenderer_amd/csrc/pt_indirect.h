// pt_indirect.h -- the arithmetic of hrpt_indirect_lighting, one __host__ __device__ source shared by the gfx950 kernels (pt_indirect.hip)
// and hrpt_indirect_rays_host / hrpt_indirect_resolve_host / hrpt_indirect_compose_host (pt_indirect_host.cpp): the producer of the
// reference's SSGI.hlsl -- one GGX-VNDF specular ray and one cosine diffuse ray per pixel from the G-buffer, two demodulated signals out --
// with the screen-space march replaced by path-traced rays (hrpt_trace_radiance with HRPT_RADIANCE_SECONDARY). It CALLS the path tracer's
// functions and restates none: camera_ray of pt_direct.h (the primary ray of init_path), sample_hemisphere_cosine, sample_ggx_vndf,
// eval_ggx_vndf_weight and compute_f0 of pt_lighting.h, hrt_pcg_hash and hrt_rng_next of detmath, over pt_vec.h's f3. DESIGN.md section 29
// has the definition in prose.
//
// Per pixel (x, y), g = y * W + x, over the planes ALBEDO (A), NORMAL (N, roughness in w), GEO_NORMAL (metallic in w), DEPTH (.x = t):
//   (o, d) = the primary ray of the constants the G-buffer was rendered with; a miss (t == 1e10f) has two untraced records
//   X = o + d * t, V = -d, baseColor = A.rgb
//   s = hrt_pcg_hash(g + hrt_pcg_hash(frameSeed)); u0..u3 = hrt_rng_next(&s), always all four
//   diffuse:  untraced when !(1 - metallic > 0); dirD = sample_hemisphere_cosine(u0, u1, N); untraced when !(dot(N, dirD) > 0);
//             else origin X, tmin 1e-4f, direction dirD, tmax 1e10f, rng = s
//   specular: H = sample_ggx_vndf(u2, u3, N, V, roughness), dirS = reflect(-V, H); untraced when !(dot(N, dirS) > 0);
//             wS = eval_ggx_vndf_weight(compute_f0(baseColor, metallic, 1.5f), N, V, dirS, H, roughness); untraced when !(maxcomp(wS) > 0);
//             else as the diffuse record with dirS and rng = hrt_pcg_hash(s)
//   an untraced record: origin = quiet NaN x 3, everything else 0 (the rule of deferred_rays)
//   resolve: diffuse = (Ld.rgb, 1) where the record's radiance has w == 1, else zeros; specular = (Ls.rgb * wS, 1), else zeros -- wS
//            recomputed by the same function from the same planes and draws, nothing is stashed in the ray's pad
//   compose, where depth.x != 1e10f: rgb = C.rgb + ((((Dp.rgb * A.rgb) * (1 - metallic)) + Sp.rgb) * intensity); alpha kept
// The diffuse plane is demodulated (no albedo, cosine-sampling weight 1); the specular plane carries F * G1, the path tracer's lobe weight.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_direct.h"
#include "pt_image.h"

namespace hrt {
namespace indirect {

using img::T4;
using img::t4;
using img::load4;

constexpr float kIor = 1.5f;
constexpr float kTMin = 1e-4f;
constexpr float kTMax = 1e10f;
constexpr uint32_t kLobeFlags = HRPT_INDIRECT_DIFFUSE | HRPT_INDIRECT_SPECULAR;
constexpr uint32_t kAllFlags = kLobeFlags | HRPT_INDIRECT_THREAD_PER_RAY;

// What the stage reads of an HrptPathTracerConstants and an HrptIndirectParams, gathered once per call.
struct Frame {
    float clipToWorld[16];      // m_View.m_MatClipToWorldNoOffset
    float cam[3];               // m_CameraPos.xyz
    float jitter[2], sizeInv[2];
    float intensity;
    uint32_t flags;
    uint32_t seedHash;          // hrt_pcg_hash(frameSeed)
    int w, h;
};
HRT_FN Frame make_frame(const HrptPathTracerConstants& cb, const HrptIndirectParams& p, int w, int h)
{
    Frame f;
    for (int i = 0; i < 16; ++i) f.clipToWorld[i] = cb.m_View.m_MatClipToWorldNoOffset[i];
    for (int i = 0; i < 3; ++i) f.cam[i] = cb.m_CameraPos[i];
    for (int i = 0; i < 2; ++i) { f.jitter[i] = cb.m_Jitter[i]; f.sizeInv[i] = cb.m_View.m_ViewportSizeInv[i]; }
    f.intensity = p.intensity; f.flags = p.flags; f.seedHash = hrt_pcg_hash(p.frameSeed);
    f.w = w; f.h = h;
    return f;
}

HRT_FN f3 xyz(T4 a) { return mk3(a.x, a.y, a.z); }

// Steps 1-3 of a hit: the surface point, the view vector and the four draws with the state behind them.
struct Draws { f3 X, V; float u[4]; uint32_t s; };
HRT_FN Draws pixel_draws(const Frame& f, int px, int py, float t)
{
    Draws r;
    f3 o, d;
    camera_ray(f.clipToWorld, f.cam, f.jitter[0], f.jitter[1], f.sizeInv[0], f.sizeInv[1], (uint32_t)px, (uint32_t)py, o, d);
    r.X = o + d * t; r.V = -d;
    r.s = hrt_pcg_hash((uint32_t)py * (uint32_t)f.w + (uint32_t)px + f.seedHash);
    for (int k = 0; k < 4; ++k) r.u[k] = hrt_rng_next(&r.s);
    return r;
}
// Step 4. false: untraced.
HRT_FN bool diffuse_lobe(const Draws& p, f3 N, float metallic, f3& dir)
{
    dir = mk3(0.0f, 0.0f, 0.0f);
    if (!(1.0f - metallic > 0.0f)) return false;
    dir = sample_hemisphere_cosine(p.u[0], p.u[1], N);
    return dot(N, dir) > 0.0f;
}
// Step 5. false: untraced. wS is the lobe weight of a traced record.
HRT_FN bool specular_lobe(const Draws& p, f3 N, float roughness, f3 baseColor, float metallic, f3& dir, f3& wS)
{
    wS = mk3(0.0f, 0.0f, 0.0f);
    const f3 H = sample_ggx_vndf(p.u[2], p.u[3], N, p.V, roughness);
    dir = reflect(-p.V, H);
    if (!(dot(N, dir) > 0.0f)) return false;
    wS = eval_ggx_vndf_weight(compute_f0(baseColor, metallic, kIor), N, p.V, dir, H, roughness);
    return maxcomp(wS) > 0.0f;
}

// ---- the ray record of one lobe: three 16-byte rows of an HrptRay ---------------------------------------------------------------------
HRT_FN void ray_rows(bool traced, f3 X, f3 dir, uint32_t rng, T4 rows[3])
{
    const float nan = hrt_u2f(0x7FC00000u);
    rows[0] = traced ? t4(X.x, X.y, X.z, kTMin) : t4(nan, nan, nan, 0.0f);
    rows[1] = traced ? t4(dir.x, dir.y, dir.z, kTMax) : t4(0.0f, 0.0f, 0.0f, 0.0f);
    rows[2] = t4(traced ? hrt_u2f(rng) : 0.0f, 0.0f, 0.0f, 0.0f);                    // rng, pad 0
}
// Both records of a pixel from its texels; a lobe the call does not flag is not evaluated (its rows are left alone).
HRT_FN void pixel_rays(const Frame& f, T4 A, T4 N4, float metallic, T4 D, int px, int py, T4 rowsD[3], T4 rowsS[3])
{
    const bool hit = !(D.x == img::kMissDepth);
    Draws p = {};
    if (hit) p = pixel_draws(f, px, py, D.x);
    const f3 N = xyz(N4);
    if (f.flags & HRPT_INDIRECT_DIFFUSE) {
        f3 dir = mk3(0.0f, 0.0f, 0.0f);
        const bool traced = hit && diffuse_lobe(p, N, metallic, dir);
        ray_rows(traced, p.X, dir, p.s, rowsD);
    }
    if (f.flags & HRPT_INDIRECT_SPECULAR) {
        f3 dir = mk3(0.0f, 0.0f, 0.0f), wS;
        const bool traced = hit && specular_lobe(p, N, N4.w, xyz(A), metallic, dir, wS);
        ray_rows(traced, p.X, dir, hrt_pcg_hash(p.s), rowsS);
    }
}
// Where the records of a lobe start, in records: diffuse first; with one lobe flagged its records start at 0.
HRT_FN size_t specular_base(uint32_t flags, size_t WH) { return (flags & HRPT_INDIRECT_DIFFUSE) ? WH : 0; }
HRT_FN size_t record_count(uint32_t flags, size_t WH) { return (flags & kLobeFlags) == kLobeFlags ? 2 * WH : WH; }

// ---- step 8 -------------------------------------------------------------------------------------------------------------------------------
// A miss has two untraced records (step 1), so it resolves to zeros whatever the radiance slot holds.
HRT_FN T4 resolve_diffuse(T4 D, T4 Ld) { return (Ld.w == 1.0f && !(D.x == img::kMissDepth)) ? t4(Ld.x, Ld.y, Ld.z, 1.0f) : t4(0.0f, 0.0f, 0.0f, 0.0f); }
HRT_FN T4 resolve_specular(const Frame& f, T4 A, T4 N4, float metallic, T4 D, int px, int py, T4 Ls)
{
    if (!(Ls.w == 1.0f) || D.x == img::kMissDepth) return t4(0.0f, 0.0f, 0.0f, 0.0f);
    const Draws p = pixel_draws(f, px, py, D.x);
    f3 dir, wS;
    specular_lobe(p, xyz(N4), N4.w, xyz(A), metallic, dir, wS);
    return t4(Ls.x * wS.x, Ls.y * wS.y, Ls.z * wS.z, 1.0f);
}
// ---- step 9 -------------------------------------------------------------------------------------------------------------------------------
HRT_FN T4 compose(float intensity, T4 C, T4 A, float metallic, T4 D, T4 Dp, T4 Sp)
{
    if (D.x == img::kMissDepth) return C;
    const f3 rgb = xyz(C) + ((((xyz(Dp) * xyz(A)) * (1.0f - metallic)) + xyz(Sp)) * intensity);
    return t4(rgb.x, rgb.y, rgb.z, C.w);
}

HRT_FN bool params_valid(const HrptIndirectParams& p)
{
    return (p.flags & ~kAllFlags) == 0u && (p.flags & kLobeFlags) != 0u && p.reserved == 0u && (p.intensity - p.intensity) == 0.0f;
}

} // namespace indirect
} // namespace hrt

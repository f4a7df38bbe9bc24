// pt_modulation.h -- the arithmetic of hrpt_demodulate / hrpt_compose, one __host__ __device__ source shared by the gfx950 kernels
// (pt_modulation.hip) and hrpt_demodulate_host / hrpt_compose_host (pt_modulation_host.cpp): the reference's SSGI compose pass,
// src/shaders/SSGICompose.hlsl (SSGICompose_PSMain :65-110), with BuildTangentFrame (CommonLighting.hlsli:610-615), TangentToLocal /
// TangentToWorld (Common.hlsli:70-78), the local-space z-up sampleGGX_VNDF (CommonLighting.hlsli:1071-1090; NOT the path tracer's y-up
// SampleGGX_VNDF) and the float3 Schlick_Fresnel (:25-28), restated statement for statement over the path tracer's own images in the
// arithmetic of hobbyrt/detmath.h: no FMA contraction, correctly rounded '/' and sqrt, select-form min / max, sums and dot products left to
// right. DESIGN.md section 20 has the definition in prose.
//
// The reference never filters radiance: its temporal and spatial passes run on a signal with the first-hit BRDF factored out, and the
// compose pass multiplies albedo * (1 - metalness) * (1 - F) and F back in. Here the path tracer hands over radiance, so the factor
// M is divided out in front of the two filters (demodulate) and multiplied back in behind them (compose):
//   demodulate   modulation[p] = (Mf, 1),  colorOut[p] = (max(color.rgb - E, 0) / Mf, color.a)
//   compose      colorOut[p] = (color.rgb * Mf + E, color.a)        with Mf read from modulation[p], not computed again
// Images are W x H float4, row-major: `color` (Output of hrpt_render), `albedo`, `normal`, `geoNormal`, `emissive`, `depth` (the planes
// HRPT_GB_ALBEDO, HRPT_GB_NORMAL with roughness in .w, HRPT_GB_GEO_NORMAL with metallic in .w, HRPT_GB_EMISSIVE, HRPT_GB_DEPTH with the
// view depth in .y), `modulation` (rgb = Mf, a = 1 at a hit and 0 at a miss). E = emissive.rgb, 0 where no emissive image is given.
//
// What the HLSL leaves open is DEFINED here (the functions of the first four items are pt_image.h's):
//   * pixel uv (bloom::pixel_u), ReconstructWorldPos from the view depth (img::recon), lerp(a, b, t) = a + t * (b - a)
//   * normalize(v) = (v.x / len, v.y / len, v.z / len) with len = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z): one correctly rounded sqrt and
//     three correctly rounded divisions. A zero vector gives 0 / 0 = NaN in every component; the NaN ends in max(kEpsilon, dot(V, h)),
//     whose select form returns kEpsilon, so the factor of such a pixel is finite.
//   * cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x), written out in full wherever it is used (also
//     where an operand has a zero component by construction)
//   * reflect(i, n) = i - (2 * dot(n, i)) * n
//   * pow(x, 5.0f) = hrt_pow(x, 5.0f), as the HLSL writes it (not hrt_pow5); cos / sin of (2 * PI) * 0.25f through hrt_sincos
//   * max(a, b) = hrt_max(a, b) with the operands in the HLSL's order: a NaN second operand gives the first
// As written in the HLSL, sampleGGX_VNDF returns an UNNORMALISED vector (alpha * Nh.x, alpha * Nh.y, max(0, Nh.z)), and reflect is fed it as
// it is; only the reflected vector is normalised.
//
// The floor. Mf = max(M, floor) per channel, floor = HrptModulationParams::floor (finite, > 0), default 0.04. On a non-metal (metal = 0)
// f0 = lerp(0.04, albedo, 0) = 0.04, F = f0 + (1 - f0) * pow(.., 5) >= 0.04, and the albedo term (albedo * 1) * (1 - F) is >= 0 for an
// albedo >= 0 (F <= 1), so no channel of M is below 0.04 there: the default floor only ever bites on dark metals (f0 = albedo < 0.04),
// where the division would otherwise amplify noise by more than 25. Both stages use the same stored Mf, so compose undoes demodulate up
// to rounding wherever nothing was filtered: for normal numbers with x >= E >= 0, |compose(demodulate(x)) - x| <= 5 * 2^-24 * x, and
// <= 3 * 2^-24 * x when E = 0 (three, resp. two, roundings of relative size 2^-24 act on x - E, one on the sum).
//
// Differences from the reference pass, on purpose:
//   * a miss (depth.x == 1e10f) gets modulation (1, 1, 1, 0) and both stages pass its colour through bit for bit (compose knows a miss by
//     modulation.a == 0); the reference writes 0. Here Output holds the sky at a miss and keeps it (the miss rule of pt_denoise.h).
//   * one radiance image stands in for both denoisedDiffuse and denoisedSpecular (lines 105-107), the choice pt_denoise.h made.
//   * emissive is subtracted before the filters and added after them; the reference adds it in DeferredRenderer.
//   * the clamp max(color - E, 0): with several jittered samples per pixel the one-sample emissive plane can exceed Output at
//     silhouettes, and the temporal stage's log(1 + x) needs x > -1.
//   * no DecodeNormal (the plane holds unit vectors); the debug views are not restated.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_image.h"

namespace hrt {
namespace modulation {

using namespace img;

constexpr float kDefaultFloor = 0.04f;

struct Args {
    ViewArgs view;
    float floor;
};
HRT_FN Args make_args(const HrptPlanarViewConstants& view, const HrptModulationParams& p, int w, int h)
{
    Args a;
    a.view = make_view_args(view, w, h);
    a.floor = p.floor;
    return a;
}

// BuildTangentFrame (CommonLighting.hlsli:610-615)
HRT_FN void tangent_frame(T3 N, T3* T, T3* B)
{
    const T3 up = hrt_abs(N.z) < 0.999f ? t3(0.0f, 0.0f, 1.0f) : t3(1.0f, 0.0f, 0.0f);
    *T = normalize(cross(up, N));
    *B = cross(N, *T);
}
// TangentToLocal / TangentToWorld (Common.hlsli:70-78)
HRT_FN T3 to_local(T3 T, T3 B, T3 N, T3 V) { return t3(dot3(V, T), dot3(V, B), dot3(V, N)); }
HRT_FN T3 to_world(T3 T, T3 B, T3 N, T3 V)
{
    return t3((V.x * T.x + V.y * B.x) + V.z * N.x, (V.x * T.y + V.y * B.y) + V.z * N.y, (V.x * T.z + V.y * B.z) + V.z * N.z);
}

// sampleGGX_VNDF (CommonLighting.hlsli:1071-1090), local space with z up; returns the unnormalised (alpha Nh.x, alpha Nh.y, max(0, Nh.z))
HRT_FN T3 sample_ggx_vndf(T3 Ve, float roughness, float randomX, float randomY)
{
    const float alpha = roughness * roughness;
    const T3 Vh = normalize(t3(alpha * Ve.x, alpha * Ve.y, Ve.z));
    const float lensq = Vh.x * Vh.x + Vh.y * Vh.y;
    T3 T1 = t3(1.0f, 0.0f, 0.0f);
    if (lensq > 0.0f) { const float len = hrt_sqrt(lensq); T1 = t3(-Vh.y / len, Vh.x / len, 0.0f / len); }
    const T3 T2 = cross(Vh, T1);
    const float r = hrt_sqrt(randomX);
    const float phi = (2.0f * HRT_PI) * randomY;
    float sn, cs;
    hrt_sincos(phi, &sn, &cs);
    const float t1 = r * cs;
    float t2 = r * sn;
    const float s = 0.5f * (1.0f + Vh.z);
    t2 = (1.0f - s) * hrt_sqrt(hrt_max(0.0f, 1.0f - t1 * t1)) + s * t2;
    const float k = hrt_sqrt(hrt_max(0.0f, (1.0f - t1 * t1) - t2 * t2));
    const T3 Nh = t3((t1 * T1.x + t2 * T2.x) + k * Vh.x, (t1 * T1.y + t2 * T2.y) + k * Vh.y, (t1 * T1.z + t2 * T2.z) + k * Vh.z);
    return t3(alpha * Nh.x, alpha * Nh.y, hrt_max(0.0f, Nh.z));
}

// Schlick_Fresnel (CommonLighting.hlsli:25-28), one channel; p = pow(max(1 - cosTheta, 0), 5) is the same for the three
HRT_FN float schlick(float f0, float p) { return f0 + (1.0f - f0) * p; }

// SSGICompose_PSMain :85-107 from V on: the factor Mf = max(M, floor) of a hit
HRT_FN T3 factor(T3 albedo, T3 N, T3 V, float rough, float metal, float floor)
{
    T3 T, B;
    tangent_frame(N, &T, &B);
    const T3 Vlocal = to_local(T, B, N, V);
    T3 H = sample_ggx_vndf(Vlocal, rough, 0.25f, 0.25f);
    if (H.z < 0.0f) H = neg(H);
    const T3 lLocal = normalize(reflect(neg(Vlocal), H));
    const T3 l = to_world(T, B, N, lLocal);
    const T3 h = normalize(add(V, l));
    const float VoH = hrt_max(HRT_K_EPSILON, dot3(V, h));
    const float p = hrt_pow(hrt_max(1.0f - VoH, 0.0f), 5.0f);
    const float one = 1.0f - metal;
    const float a3[3] = { albedo.x, albedo.y, albedo.z };
    float m[3];
    for (int i = 0; i < 3; ++i) {
        const float F = schlick(lerp(0.04f, a3[i], metal), p);
        m[i] = hrt_max(((a3[i] * one) * (1.0f - F)) + F, floor);
    }
    return t3(m[0], m[1], m[2]);
}

// modulation[p]: (1, 1, 1, 0) at a miss, (Mf, 1) at a hit
HRT_FN T4 modulation_pixel(const Args& a, const float* albedo, const float* normal, const float* geoNormal, const float* depth, int px, int py)
{
    const int W = a.view.w, H = a.view.h;
    const T4 D = load4(depth, W, px, py);
    if (D.x == kMissDepth) return t4(1.0f, 1.0f, 1.0f, 0.0f);
    const T4 A = load4(albedo, W, px, py), N4 = load4(normal, W, px, py);
    const float metal = load4(geoNormal, W, px, py).w;
    const float u = bloom::pixel_u(px, W), v = bloom::pixel_u(py, H);
    const T3 worldPos = recon(a.view, u, v, D.y);
    const T3 V = normalize(sub(t3(a.view.cam[0], a.view.cam[1], a.view.cam[2]), worldPos));
    const T3 m = factor(t3(A.x, A.y, A.z), t3(N4.x, N4.y, N4.z), V, N4.w, metal, a.floor);
    return t4(m.x, m.y, m.z, 1.0f);
}

// C = color[p], M = modulation[p], E = emissive[p].rgb (0 without an emissive image)
HRT_FN T4 demodulate_color(T4 C, T4 M, T3 E)
{
    if (M.w == 0.0f) return C;
    return t4(hrt_max(C.x - E.x, 0.0f) / M.x, hrt_max(C.y - E.y, 0.0f) / M.y, hrt_max(C.z - E.z, 0.0f) / M.z, C.w);
}
HRT_FN T4 compose_color(T4 C, T4 M, T3 E)
{
    if (M.w == 0.0f) return C;
    return t4(C.x * M.x + E.x, C.y * M.y + E.y, C.z * M.z + E.z, C.w);
}

} // namespace modulation
} // namespace hrt

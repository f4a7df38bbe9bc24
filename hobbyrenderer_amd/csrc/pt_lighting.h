// pt_lighting.h -- the Lighting record, BRDF evaluation and sampling. __host__ __device__ like pt_vec.h, and nothing here reads a scene: the
// deferred stage's host executors evaluate the same prepare_byproducts / evaluate_direct_unshadowed as the path kernels.
#pragma once

#include "pt_vec.h"

namespace hrt {

// ------------------------------------------------------------------ BRDF (CommonLighting.hlsli)
struct Lighting {            // the part of LightingInputs the path tracer reads
    f3 N, V, L, baseColor; float roughness, metallic, ior;
    f3 F0, F; float kD;
    float NdotV, NdotL, NdotH, VdotH, LdotV, LdotH;
};
HRT_FN f3 f_schlick(f3 spec, float VdotH)                                   // :123-129
{
    float Fc = hrt_pow5(1.0f - VdotH);
    float s = hrt_saturate(50.0f * spec.y) * Fc;
    float k = 1.0f - Fc;
    return mk3(s + k * spec.x, s + k * spec.y, s + k * spec.z);
}
HRT_FN f3 compute_f0(f3 baseColor, float metallic, float ior)               // :64-68
{
    float q = (ior - 1.0f) / (ior + 1.0f);
    float d = q * q;
    return mk3(lerp(d, baseColor.x, metallic), lerp(d, baseColor.y, metallic), lerp(d, baseColor.z, metallic));
}
HRT_FN void prepare_byproducts(Lighting& in)                                // :316-334
{
    in.NdotV = hrt_saturate(dot(in.N, in.V));
    in.NdotL = hrt_saturate(dot(in.N, in.L));
    f3 VpL = in.V + in.L;
    float len = dot(VpL, VpL);
    f3 H = (len > 1e-8f) ? VpL * hrt_rsqrt(len) : in.N;
    in.NdotH = hrt_saturate(dot(in.N, H));
    in.VdotH = hrt_saturate(dot(in.V, H));
    in.LdotV = hrt_saturate(dot(in.L, in.V));
    in.LdotH = hrt_saturate(dot(in.L, H));
    in.F0 = compute_f0(in.baseColor, in.metallic, in.ior);
    in.kD = 1.0f - in.metallic;
    in.F = f_schlick(in.F0, in.VdotH);
}
HRT_FN float d_ggx(float NdotH, float roughness)                            // :80-86
{
    float alpha = roughness * roughness, alpha2 = alpha * alpha;
    float denom = NdotH * NdotH * (alpha2 - 1.0f) + 1.0f;
    return alpha2 / (HRT_PI * denom * denom);
}
HRT_FN float burley_diffuse(float NdotL, float NdotV, float LdotH, float rough)   // :148-168
{
    if (NdotL <= 0.0f || NdotV <= 0.0f) return 0.0f;
    float rough2 = rough * rough;
    float FL = hrt_pow5(1.0f - NdotL), FV = hrt_pow5(1.0f - NdotV);
    float Fd90 = 0.5f + 2.0f * rough2 * LdotH * LdotH;
    float Fd = lerp(1.0f, Fd90, FL) * lerp(1.0f, Fd90, FV);
    return Fd * NdotL / HRT_PI;
}
// EvaluateDirectLight :360-375 with ComputeSpecularBRDF :345-358, before the shadow factor:
// diffuse = (diffuseTerm*kD*baseColor)*radiance, specular = (spec*NdotL)*radiance.
HRT_FN void evaluate_direct_unshadowed(const Lighting& in, f3 radiance, f3& diffuse, f3& specular)
{
    float dt = burley_diffuse(in.NdotL, in.NdotV, in.LdotH, in.roughness);
    f3 kd = mk3(in.kD, in.kD, in.kD);
    f3 dif = (kd * dt) * in.baseColor;
    float alpha = in.roughness * in.roughness, alpha2 = alpha * alpha;
    float D = d_ggx(in.NdotH, in.roughness);
    float g1 = in.NdotV * hrt_sqrt(alpha2 + (1.0f - alpha2) * in.NdotL * in.NdotL);
    float g2 = in.NdotL * hrt_sqrt(alpha2 + (1.0f - alpha2) * in.NdotV * in.NdotV);
    float G2 = 0.5f / hrt_max(g1 + g2, 1e-6f);
    float k = D * G2;
    f3 spec = in.F * k;
    diffuse = dif * radiance;
    specular = (spec * in.NdotL) * radiance;
}
HRT_FN void tangent_frame(f3 N, f3& T, f3& B)                                // :610-615, :176-178, :702-704
{
    f3 up = hrt_abs(N.z) < 0.999f ? mk3(0.0f, 0.0f, 1.0f) : mk3(1.0f, 0.0f, 0.0f);
    T = normalize(cross(up, N));
    B = cross(N, T);
}
HRT_FN f3 frame_combine(f3 T, f3 N, f3 B, f3 l) { return (T * l.x + N * l.y) + B * l.z; }
// The two BRDF lobes share their first steps -- two random numbers, sin/cos of 2*pi*u, one square root, the tangent frame of N --
// so the callers evaluate those once (shade_surface_b) and the lobes start from them: `root` = sqrt(uy) (cosine) or sqrt(ux) (VNDF),
// (sp, cp) = sincos(2*pi*ux) (cosine) or sincos(2*pi*uy) (VNDF). Same operations on the same values as the reference order.
HRT_FN f3 sample_hemisphere_cosine_from(float root, float sp, float cp, f3 T, f3 B, f3 normal)   // :170-183
{
    float cosTheta = root;
    float sinTheta = hrt_sqrt(hrt_max(0.0f, 1.0f - cosTheta * cosTheta));
    return frame_combine(T, normal, B, mk3(sinTheta * cp, cosTheta, sinTheta * sp));
}
HRT_FN f3 sample_hemisphere_cosine(float ux, float uy, f3 normal)
{
    float sp, cp; hrt_sincos(2.0f * HRT_PI * ux, &sp, &cp);
    f3 T, B; tangent_frame(normal, T, B);
    return sample_hemisphere_cosine_from(hrt_sqrt(uy), sp, cp, T, B, normal);
}
HRT_FN f3 sample_ggx_vndf_from(float root, float sp, float cp, f3 T, f3 B, f3 N, f3 V, float roughness)   // :622-655
{
    float alpha = roughness * roughness;
    f3 Vl = mk3(dot(V, T), dot(V, N), dot(V, B));
    f3 Vh = normalize(mk3(alpha * Vl.x, Vl.y, alpha * Vl.z));
    float lensq = Vh.x * Vh.x + Vh.z * Vh.z;
    f3 T1 = lensq > 0.0f ? mk3(-Vh.z, 0.0f, Vh.x) / hrt_sqrt(lensq) : mk3(1.0f, 0.0f, 0.0f);
    f3 T2 = cross(Vh, T1);
    float r = root;
    float t1 = r * cp, t2 = r * sp;
    float s = 0.5f * (1.0f + Vh.y);
    t2 = lerp(hrt_sqrt(hrt_max(0.0f, 1.0f - t1 * t1)), t2, s);
    float nz = hrt_sqrt(hrt_max(0.0f, (1.0f - t1 * t1) - t2 * t2));
    f3 Nh = (T1 * t1 + T2 * t2) + Vh * nz;
    f3 Ne = normalize(mk3(alpha * Nh.x, hrt_max(0.0f, Nh.y), alpha * Nh.z));
    return frame_combine(T, N, B, Ne);
}
HRT_FN f3 sample_ggx_vndf(float ux, float uy, f3 N, f3 V, float roughness)
{
    float sp, cp; hrt_sincos(2.0f * HRT_PI * uy, &sp, &cp);
    f3 T, B; tangent_frame(N, T, B);
    return sample_ggx_vndf_from(hrt_sqrt(ux), sp, cp, T, B, N, V, roughness);
}
HRT_FN f3 eval_ggx_vndf_weight(f3 F0, f3 N, f3 V, f3 L, f3 H, float roughness)   // :671-688
{
    float alpha = roughness * roughness, alpha2 = alpha * alpha;
    float NdotV = hrt_saturate(dot(N, V)), NdotL = hrt_saturate(dot(N, L)), VdotH = hrt_saturate(dot(V, H));
    if (NdotV <= 0.0f || NdotL <= 0.0f) return mk3(0.0f, 0.0f, 0.0f);
    f3 F = f_schlick(F0, VdotH);
    float G1L = 2.0f * NdotL / (NdotL + hrt_sqrt(alpha2 + (1.0f - alpha2) * NdotL * NdotL));
    return F * G1L;
}
HRT_FN f3 sample_cone(f3 dir, float cosHalf, float ux, float uy)             // :693-708
{
    float cosTheta = 1.0f - ux * (1.0f - cosHalf);
    float sinTheta = hrt_sqrt(hrt_max(0.0f, 1.0f - cosTheta * cosTheta));
    float phi = 2.0f * HRT_PI * uy;
    float sp, cp; hrt_sincos(phi, &sp, &cp);
    f3 T, B; tangent_frame(dir, T, B);
    return frame_combine(T, dir, B, mk3(sinTheta * cp, cosTheta, sinTheta * sp));
}
// EvalFresnelDielectric, PathTracer.hlsl:26-43
HRT_FN float fresnel_dielectric(float eta, float cosThetaI, float& cosThetaT)
{
    if (cosThetaI < 0.0f) { eta = 1.0f / eta; cosThetaI = -cosThetaI; }
    float sinThetaTSq = eta * eta * (1.0f - cosThetaI * cosThetaI);
    if (sinThetaTSq >= 1.0f) { cosThetaT = 0.0f; return 1.0f; }
    cosThetaT = hrt_sqrt(hrt_max(0.0f, 1.0f - sinThetaTSq));
    float Rs = (eta * cosThetaI - cosThetaT) / (eta * cosThetaI + cosThetaT);
    float Rp = (eta * cosThetaT - cosThetaI) / (eta * cosThetaT + cosThetaI);
    return 0.5f * (Rs * Rs + Rp * Rp);
}

} // namespace hrt

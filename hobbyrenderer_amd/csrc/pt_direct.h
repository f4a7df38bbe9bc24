// pt_direct.h -- what a first hit needs for direct light without a SceneView: the camera ray of a pixel, the first stage of a light sample
// (nee_draw: the culls and the two draws), light distance attenuation and the Lighting record of a surface. __host__ __device__ over f3
// (pt_vec.h), so the path tracer (pt_path.h, pt_wf_raygen.h) and the deferred stage with its host executors (pt_deferred.h) run one source.
#pragma once

#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_lighting.h"

namespace hrt {

// Primary ray of pixel (px, py), PathTracer.hlsl:61-72; UVToClipXY Common.hlsli:50-53. M = m_MatClipToWorldNoOffset. No RNG: the callers seed.
// (primary_ray of pt_wf_common.h holds a deliberate copy of this body)
HRT_FN void camera_ray(const float* M, const float* cam, float jitterX, float jitterY, float invW, float invH, uint32_t px, uint32_t py, f3& o, f3& d)
{
    float u = (((float)px + 0.5f) + jitterX) * invW;
    float v = (((float)py + 0.5f) + jitterY) * invH;
    float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;
    float ex = ((cx * M[0] + cy * M[4]) + 0.9f * M[8]) + 1.0f * M[12];
    float ey = ((cx * M[1] + cy * M[5]) + 0.9f * M[9]) + 1.0f * M[13];
    float ez = ((cx * M[2] + cy * M[6]) + 0.9f * M[10]) + 1.0f * M[14];
    float ew = ((cx * M[3] + cy * M[7]) + 0.9f * M[11]) + 1.0f * M[15];
    f3 end = mk3(ex / ew, ey / ew, ez / ew);
    o = mk3(cam[0], cam[1], cam[2]);
    d = normalize(end - o);
}

// First stage of one light sample (pt_path.h has the three): the early-outs that precede the RNG draws (CommonLighting.hlsli:723, :758-764,
// :815-833), then the two draws (:730, :776, :846). false: the light is skipped for this surface point -- no draw, no shadow ray, no
// contribution. Contract: every cull comes before the first draw and none depends on rng, ux or uy, so a caller may rely on the return value
// alone -- the deferred stage (pt_deferred.h) does, on a throw-away RNG state. Keep the draws last.
template <bool DIRONLY>
HRT_FN bool nee_draw(const HrptGPULight& l, f3 N, f3 worldPos, f3 sunDirection, uint32_t& rng, float& ux, float& uy)
{
    if (DIRONLY || l.m_Type == HRPT_LIGHT_DIRECTIONAL) {                        // :716-745
        if (dot(N, sunDirection) <= 0.0f) return false;
    } else if (!DIRONLY && (l.m_Type == HRPT_LIGHT_POINT || l.m_Type == HRPT_LIGHT_SPOT)) {   // :752-804, :809-874
        if (l.m_Intensity <= 0.0f) return false;
        f3 toLight = mk3(l.m_Position) - worldPos;
        float distSq = dot(toLight, toLight);
        if (l.m_Range > 0.0f && distSq > l.m_Range * l.m_Range) return false;
        if (l.m_Type == HRPT_LIGHT_SPOT) {
            float dist = hrt_sqrt(distSq);
            f3 Lc = toLight / dist;
            if (dot(N, Lc) <= 0.0f) return false;
            f3 lightDir = normalize(mk3(l.m_Direction));
            float cosTheta = dot(-Lc, lightDir);
            if (cosTheta < hrt_cos(l.m_SpotOuterConeAngle)) return false;
        }
    } else return false;
    ux = hrt_rng_next(&rng); uy = hrt_rng_next(&rng);
    return true;
}

// Light distance attenuation, CommonLighting.hlsli:766-769 / :835-837 (pow(x,4), pow(x,2) by multiplication)
HRT_FN float distance_attenuation(const HrptGPULight& l, float distSq, float dist)
{
    float a = 1.0f / (distSq + 1.0f);
    if (l.m_Range > 0.0f) {
        float q = dist / l.m_Range; float q2 = q * q; float q4 = q2 * q2;
        float sa = hrt_saturate(1.0f - q4);
        a *= sa * sa;
    }
    return a;
}

// The surface terms a deferred NEE evaluation needs (what LightingInputs carries into AccumulateDirectLighting).
HRT_FN Lighting nee_lighting(f3 N, f3 V, f3 baseColor, float roughness, float metallic, float ior)
{
    Lighting in;
    in.N = N; in.V = V; in.L = mk3(0.0f, 0.0f, 0.0f); in.baseColor = baseColor; in.roughness = roughness; in.metallic = metallic; in.ior = ior;
    return in;
}

} // namespace hrt

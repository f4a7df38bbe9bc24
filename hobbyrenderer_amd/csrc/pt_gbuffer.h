// pt_gbuffer.h -- the first-hit G-buffer (hrpt_render_gbuffer): what path vertex 0 of one accumulation index saw, as six planes of 16 bytes per
// pixel. Contents follow GBufferOut of the reference's real-time modes (src/shaders/BasePass.hlsl:184-192, 485-493), computed
// by the path tracer's own stages: the primary ray and RNG seed of init_path, the hit of TraceRayStandard, GetFullHitAttributes +
// GetPBRAttributes and the normal flip of PathTracer.hlsl:110-117 -- the surface hrpt_render shades at bounce 0 for the same constants.
// Both paths call gbuffer_texels / gbuffer_store below: wf_gbuffer and wf_gbuffer_motion of pt_wf_gbuffer.h, and pt_gbuffer_kernel and
// pt_motion_kernel among the thread-per-query kernels of pt_megakernel.hip.
#pragma once

#include "pt_path.h"

namespace hrt {

// plane indices = HRPT_GB_* of include/hobbyrt_pt.h
constexpr uint32_t kGbAlbedo = 0, kGbNormal = 1, kGbGeoNormal = 2, kGbEmissive = 3, kGbDepth = 4, kGbIds = 5, kGbPlanes = 6;
struct GBufferPlanes { float4* plane[kGbPlanes]; };     // W x H each; only the planes of the call's mask are dereferenced

// The six texels of a pixel whose primary ray missed: zeros, depth = the ray's tmax, ids = none.
HRT_DEV void gbuffer_miss(float4 (&out)[kGbPlanes])
{
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    out[kGbAlbedo] = zero; out[kGbNormal] = zero; out[kGbGeoNormal] = zero; out[kGbEmissive] = zero;
    out[kGbDepth] = make_float4(1e10f, 1e10f, 0.0f, 0.0f);
    const float none = __uint_as_float(0xFFFFFFFFu);
    out[kGbIds] = make_float4(none, none, none, __uint_as_float(0u));
}

// ... and of a committed hit. hit.tri / hit.inst address the records as shade_surface_a does (two-level scenes: per-mesh triangle + the hit's
// instance); tangents are read only when the material samples a normal map.
HRT_DEV void gbuffer_texels(const SceneView& s, const HrptPathTracerConstants& cb, const Ray& ray, const Hit& hit, float4 (&out)[kGbPlanes])
{
    const TriVerts tv = load_hit_attr(s, hit);
    const GpuInstShade is = s.instShade[tv.inst];
    const HrptMaterialConstants& mat = s.materials[tv.material];
    const uint32_t texFlags = mat.m_TextureFlags;
    const uint32_t prim = reinterpret_cast<const uint32_t*>(s.attrs + hit.tri)[17];      // GpuTriAttr e.y
    const SurfaceAttr attr = full_hit_attributes(s, hit, ray, tv, is, (texFlags & HRPT_TEXFLAG_NORMAL) != 0);
    const Pbr pbr = pbr_attributes(s, attr, mat, texFlags);
    const f3 Ng = normalize(attr.worldNormal);                    // PathTracer.hlsl:110
    f3 N = pbr.normal;
    const f3 V = -ray.d;
    const bool isFrontFace = dot(Ng, ray.d) < 0.0f;               // :113
    if (dot(N, V) < 0.0f) N = -N;                                 // :117
    // linear view-space depth (CommonLighting.hlsli:249-250): w of float4(worldPos, 1) * m_MatWorldToClipNoOffset, summed left to right
    const float* M = cb.m_View.m_MatWorldToClipNoOffset;
    const float viewDepth = ((attr.worldPos.x * M[3] + attr.worldPos.y * M[7]) + attr.worldPos.z * M[11]) + 1.0f * M[15];
    out[kGbAlbedo] = make_float4(pbr.baseColor.x, pbr.baseColor.y, pbr.baseColor.z, pbr.alpha);
    out[kGbNormal] = make_float4(N.x, N.y, N.z, pbr.roughness);
    out[kGbGeoNormal] = make_float4(Ng.x, Ng.y, Ng.z, pbr.metallic);
    out[kGbEmissive] = make_float4(pbr.emissive.x, pbr.emissive.y, pbr.emissive.z, 1.0f);
    out[kGbDepth] = make_float4(hit.t, viewDepth, hit.u, hit.v);
    out[kGbIds] = make_float4(__uint_as_float(tv.inst), __uint_as_float(prim), __uint_as_float(tv.material), __uint_as_float(1u | (isFrontFace ? 2u : 0u)));
}

// One 16-byte store per requested plane at pixel `idx`.
HRT_DEV void gbuffer_store(const GBufferPlanes& g, uint32_t planeMask, size_t idx, const float4 (&texel)[kGbPlanes])
{
#pragma unroll
    for (uint32_t k = 0; k < kGbPlanes; ++k)
        if (planeMask & (1u << k)) g.plane[k][idx] = texel[k];
}

} // namespace hrt

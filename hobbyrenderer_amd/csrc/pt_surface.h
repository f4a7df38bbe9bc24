// pt_surface.h -- candidate alpha, hit attributes and PBR evaluation of a surface point.
#pragma once

#include "pt_shade_tables.h"
#include "pt_texture.h"

namespace hrt {

// candidate alpha = mat.m_BaseColor.w [* albedo.a] (RaytracingCommon.hlsli:97-103, :172-176)
HRT_DEV float candidate_alpha(const SceneView& s, const HrptMaterialConstants& mat, f2 uv)
{
    float alpha = mat.m_BaseColor[3];
    if (mat.m_TextureFlags & HRPT_TEXFLAG_ALBEDO) alpha *= sample_texture(s, mat.m_AlbedoTextureIndex, mat.m_AlbedoSamplerIndex, uv).w;
    return alpha;
}

// AlphaTestGrad's alpha (RaytracingCommon.hlsli:112-130) with the synthetic gradients of GetShadowRayGradients (:207-240): ddx = ddy =
// uvRange * triangleArea / max(dist, 0.1), from the world-space triangle, the hit's barycentrics and the ray origin. Only textures with a
// mip chain need them (a single-level texture is sampled at level 0 whatever the gradients are): worldTriangle(p0, p1, p2) yields the
// triangle and is called on that path alone, so every other candidate does not load it.
template <class TRI>
HRT_DEV float candidate_alpha_grad(const SceneView& s, const HrptMaterialConstants& mat, f2 uv, const TriVerts& tv, float bu, float bv, f3 rayOrigin, TRI&& worldTriangle)
{
    float alpha = mat.m_BaseColor[3];
    if (!(mat.m_TextureFlags & HRPT_TEXFLAG_ALBEDO)) return alpha;
    const uint32_t ti = mat.m_AlbedoTextureIndex;
    if (ti >= s.textureCount) return alpha * 0.0f;
    const GpuTexture& t = s.textures[ti];
    const uint8_t* texels = t.texels;
    if (!texels) return alpha * 0.0f;
    if (t.mipCount <= 1u) return alpha * sample_texture_level(texels, t.format, (int)t.w, (int)t.h, 0u, mat.m_AlbedoSamplerIndex, uv).w;
    f3 p0, p1, p2; worldTriangle(p0, p1, p2);
    const float w0 = (1.0f - bu) - bv;
    const f3 hitPos = (p0 * w0 + p1 * bu) + p2 * bv;
    const float dist = length(hitPos - rayOrigin);
    const float triangleArea = length(cross(p1 - p0, p2 - p0)) * 0.5f;
    f2 uvRange;
    uvRange.x = hrt_max(tv.uv0.x, hrt_max(tv.uv1.x, tv.uv2.x)) - hrt_min(tv.uv0.x, hrt_min(tv.uv1.x, tv.uv2.x));
    uvRange.y = hrt_max(tv.uv0.y, hrt_max(tv.uv1.y, tv.uv2.y)) - hrt_min(tv.uv0.y, hrt_min(tv.uv1.y, tv.uv2.y));
    const float gradientScale = triangleArea / hrt_max(dist, 0.1f);
    f2 grad; grad.x = uvRange.x * gradientScale; grad.y = uvRange.y * gradientScale;
    return alpha * sample_texture_grad(t, mat.m_AlbedoSamplerIndex, uv, grad, grad).w;
}

struct SurfaceAttr { f3 worldPos, worldNormal, worldTangent; float tangentSign; f2 uv; };
struct Pbr { f3 baseColor; float alpha, roughness, metallic; f3 emissive, normal; };

// GetFullHitAttributes, RaytracingCommon.hlsli:52-77 (LOD 0: PathTracer.hlsl:103)
HRT_DEV SurfaceAttr full_hit_attributes(const SceneView& s, const Hit& hit, const Ray& ray, const TriVerts& tv, const GpuInstShade& is, bool wantTangent)
{
    float bx = (1.0f - hit.u) - hit.v, by = hit.u, bz = hit.v;
    SurfaceAttr a;
    a.worldPos = ray.o + ray.d * hit.t;
    f3 ln = (tv.n0 * bx + tv.n1 * by) + tv.n2 * bz;
    a.worldNormal = transform_normal(ln, is);
    a.tangentSign = 1.0f;
    if (wantTangent && s.tangents) {
        GpuTriTangent tg = s.tangents[hit.tri];
        f3 t0 = mk3(tg.t0.x, tg.t0.y, tg.t0.z), t1 = mk3(tg.t1.x, tg.t1.y, tg.t1.z), t2 = mk3(tg.t2.x, tg.t2.y, tg.t2.z);
        f3 lt = (t0 * bx + t1 * by) + t2 * bz;
        a.worldTangent = transform_normal(lt, is);
        a.tangentSign = (tg.t0.w * bx + tg.t1.w * by) + tg.t2.w * bz;
    } else a.worldTangent = mk3(0.0f, 0.0f, 0.0f);
    a.uv.x = (tv.uv0.x * bx + tv.uv1.x * by) + tv.uv2.x * bz;
    a.uv.y = (tv.uv0.y * bx + tv.uv1.y * by) + tv.uv2.y * bz;
    return a;
}
// TransformNormalWithTBN, Common.hlsli:183-200
HRT_DEV f3 normal_with_tbn(float nx, float ny, f3 normal, f3 tangent, float tangentSign)
{
    float x = 2.0f * nx - 1.0f, y = 2.0f * ny - 1.0f;
    float z = hrt_sqrt(hrt_saturate(1.0f - (x * x + y * y)));
    f3 n_w = normalize(normal);
    f3 t_w = normalize(tangent);
    t_w = normalize(t_w - n_w * dot(t_w, n_w));
    f3 b_w = normalize(cross(n_w, t_w) * tangentSign);
    f3 o = mk3((x * t_w.x + y * b_w.x) + z * n_w.x, (x * t_w.y + y * b_w.y) + z * n_w.y, (x * t_w.z + y * b_w.z) + z * n_w.z);
    return normalize(o);
}
// GetPBRAttributes, RaytracingCommon.hlsli:252-296
// The four material textures of a hit fetched TOGETHER (GetPBRAttributes, RaytracingCommon.hlsli:252-296). Sampled one after the other, every texture
// is a chain of dependent round trips -- descriptor, then the four texels of its bilinear footprint, then (sRGB formats) the linearisation table --
// and a hit with three maps waits for nine of them in a row; wf_shade on textured scenes spends 69 % of its wave cycles waiting
// (profiles/r02_pmc_config4.txt). Here all descriptors are requested first, then all sixteen texels (unused slots read texel 0 of a valid
// texture: no divergent branch between the requests), and only then the filtering arithmetic runs, texture by texture, exactly as
// sample_texture_level does it: same operations, same order, same bits. Only for 8-bit formats (RGBA8_UNORM / RGBA8_SRGB, what stb-decoded and
// block-decoded images arrive as) at level 0; anything else takes the one-by-one path below.
#ifndef HRPT_NO_BATCHED_TEXTURES
struct TexSlot { const uint32_t* texels; uint32_t format, sampler; int w, h; bool on; };
HRT_DEV bool pbr_textures_batched(const SceneView& s, f2 uv, const HrptMaterialConstants& m, uint32_t texFlags, f4 (&out)[4])
{
    if (s.textureCount == 0u) return false;
    const uint32_t index[4] = { m.m_AlbedoTextureIndex, m.m_RoughnessMetallicTextureIndex, m.m_EmissiveTextureIndex, m.m_NormalTextureIndex };
    const uint32_t sampler[4] = { m.m_AlbedoSamplerIndex, m.m_RoughnessSamplerIndex, m.m_EmissiveSamplerIndex, m.m_NormalSamplerIndex };
    const uint32_t bit[4] = { HRPT_TEXFLAG_ALBEDO, HRPT_TEXFLAG_ROUGHNESS_METALLIC, HRPT_TEXFLAG_EMISSIVE, HRPT_TEXFLAG_NORMAL };
    TexSlot t[4];
    bool simple = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {             // round 1: the descriptors
        const bool want = (texFlags & bit[k]) != 0u && index[k] < s.textureCount;
        const GpuTexture& g = s.textures[want ? index[k] : 0u];
        t[k].texels = reinterpret_cast<const uint32_t*>(g.texels); t[k].format = g.format; t[k].w = (int)g.w; t[k].h = (int)g.h; t[k].sampler = sampler[k];
        t[k].on = want && g.texels != nullptr;
        // (a flagged texture whose index is out of range or whose texels are missing samples as zero, as sample_texture does)
        simple = simple && (!t[k].on || g.format == HRPT_TEXTURE_FORMAT_RGBA8_UNORM || g.format == HRPT_TEXTURE_FORMAT_RGBA8_SRGB);
    }
    if (!simple) return false;
    uint32_t word[4][4]; float tx[4], ty[4]; bool point[4];
    const uint32_t* safe = reinterpret_cast<const uint32_t*>(s.textures);      // readable, whatever it holds: the slot's result is discarded
#pragma unroll
    for (int k = 0; k < 4; ++k) {             // round 2: the footprints (sample_texture_level's address arithmetic) and the sixteen texel requests
        const bool wrap = (t[k].sampler <= 5u) ? ((t[k].sampler & 1u) != 0) : false;
        point[k] = (t[k].sampler == 2u || t[k].sampler == 3u);
        const int lw = t[k].on ? t[k].w : 1, lh = t[k].on ? t[k].h : 1;
        float fx = uv.x * (float)lw, fy = uv.y * (float)lh;
        if (!point[k]) { fx = fx - 0.5f; fy = fy - 0.5f; }
        const float ix = hrt_floor(fx), iy = hrt_floor(fy);
        tx[k] = point[k] ? 0.0f : fx - ix; ty[k] = point[k] ? 0.0f : fy - iy;
        const int x0 = wrap_i((int)ix, lw, wrap), x1 = wrap_i((int)ix + 1, lw, wrap), y0 = wrap_i((int)iy, lh, wrap), y1 = wrap_i((int)iy + 1, lh, wrap);
        const uint32_t* base = t[k].on ? t[k].texels : safe;
        const uint32_t r0 = (uint32_t)y0 * (uint32_t)lw, r1 = (uint32_t)y1 * (uint32_t)lw;
        word[k][0] = base[t[k].on ? r0 + (uint32_t)x0 : 0u]; word[k][1] = base[t[k].on ? r0 + (uint32_t)x1 : 0u];
        word[k][2] = base[t[k].on ? r1 + (uint32_t)x0 : 0u]; word[k][3] = base[t[k].on ? r1 + (uint32_t)x1 : 0u];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {             // round 3: decode + filter, texture by texture
        f4 c[4];
        const bool srgb = t[k].format == HRPT_TEXTURE_FORMAT_RGBA8_SRGB;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t p = word[k][j];
            if (srgb) { c[j].x = kSrgbToLinear[p & 255u]; c[j].y = kSrgbToLinear[(p >> 8) & 255u]; c[j].z = kSrgbToLinear[(p >> 16) & 255u]; }
            else { c[j].x = unorm8_to_float(p & 255u); c[j].y = unorm8_to_float((p >> 8) & 255u); c[j].z = unorm8_to_float((p >> 16) & 255u); }
            c[j].w = unorm8_to_float(p >> 24);
        }
        f4 r;
        if (point[k]) r = c[0];
        else { const f4 a = lerp4(c[0], c[1], tx[k]), b = lerp4(c[2], c[3], tx[k]); r = lerp4(a, b, ty[k]); }
        if (!t[k].on) r.x = r.y = r.z = r.w = 0.0f;
        out[k] = r;
    }
    return true;
}
#endif
HRT_DEV Pbr pbr_attributes(const SceneView& s, const SurfaceAttr& a, const HrptMaterialConstants& m, uint32_t texFlags)
{
    Pbr p;
#ifndef HRPT_NO_BATCHED_TEXTURES
    f4 tex[4];
    if (texFlags != 0u && pbr_textures_batched(s, a.uv, m, texFlags, tex)) {
        HRT_PHASE(PH_SHADE_TEX);
        p.baseColor = mk3(m.m_BaseColor); p.alpha = m.m_BaseColor[3];
        if (texFlags & HRPT_TEXFLAG_ALBEDO) { p.baseColor = p.baseColor * mk3(tex[0].x, tex[0].y, tex[0].z); p.alpha *= tex[0].w; }
        p.roughness = m.m_RoughnessMetallic[0]; p.metallic = m.m_RoughnessMetallic[1];
        if (texFlags & HRPT_TEXFLAG_ROUGHNESS_METALLIC) { p.roughness = tex[1].y; p.metallic = tex[1].z; }
        p.roughness = hrt_max(p.roughness, 0.04f);
        p.emissive = mk3(m.m_EmissiveFactor);
        if (texFlags & HRPT_TEXFLAG_EMISSIVE) p.emissive = p.emissive * mk3(tex[2].x, tex[2].y, tex[2].z);
        if (texFlags & HRPT_TEXFLAG_NORMAL) p.normal = normal_with_tbn(tex[3].x, tex[3].y, a.worldNormal, a.worldTangent, a.tangentSign);
        else p.normal = normalize(a.worldNormal);
        return p;
    }
#endif
    p.baseColor = mk3(m.m_BaseColor); p.alpha = m.m_BaseColor[3];
    if (texFlags & HRPT_TEXFLAG_ALBEDO) {
        HRT_PHASE(PH_SHADE_TEX);
        f4 t = sample_texture(s, m.m_AlbedoTextureIndex, m.m_AlbedoSamplerIndex, a.uv);
        p.baseColor = p.baseColor * mk3(t.x, t.y, t.z); p.alpha *= t.w;
    }
    p.roughness = m.m_RoughnessMetallic[0];
    p.metallic = m.m_RoughnessMetallic[1];
    if (texFlags & HRPT_TEXFLAG_ROUGHNESS_METALLIC) {
        f4 t = sample_texture(s, m.m_RoughnessMetallicTextureIndex, m.m_RoughnessSamplerIndex, a.uv);
        p.roughness = t.y; p.metallic = t.z;
    }
    p.roughness = hrt_max(p.roughness, 0.04f);
    p.emissive = mk3(m.m_EmissiveFactor);
    if (texFlags & HRPT_TEXFLAG_EMISSIVE) {
        f4 t = sample_texture(s, m.m_EmissiveTextureIndex, m.m_EmissiveSamplerIndex, a.uv);
        p.emissive = p.emissive * mk3(t.x, t.y, t.z);
    }
    if (texFlags & HRPT_TEXFLAG_NORMAL) {
        f4 t = sample_texture(s, m.m_NormalTextureIndex, m.m_NormalSamplerIndex, a.uv);
        p.normal = normal_with_tbn(t.x, t.y, a.worldNormal, a.worldTangent, a.tangentSign);
    } else p.normal = normalize(a.worldNormal);
    return p;
}

} // namespace hrt

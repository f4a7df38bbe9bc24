// pt_denoise.h -- the arithmetic of hrpt_denoise, one __host__ __device__ source shared by the gfx950 kernel (pt_denoise.hip) and
// hrpt_denoise_host (pt_denoise_host.cpp): the reference's SSGI Poisson denoise pass, src/shaders/SSGIDenoise.hlsl (SSGIDenoise_PSMain :44-191)
// with SampleBlueNoise of src/shaders/Common.hlsli:92-107 and Luminance of src/shaders/CommonLighting.hlsli:14, restated statement for
// statement over the path tracer's own images in the arithmetic of hobbyrt/detmath.h: no FMA contraction, correctly rounded '/' and sqrt,
// select-form min / max / clamp, sums and dot products left to right. DESIGN.md section 18 has the definition in prose.
//
// Images are W x H float4, row-major: `input` (rgb = radiance, a = age: the history of hrpt_temporal_accumulate), `depth`, `normal` and
// `geoNormal` (the planes HRPT_GB_DEPTH, HRPT_GB_NORMAL, HRPT_GB_GEO_NORMAL of the same frame: view depth in depth.y, roughness in
// normal.w, metallic in geoNormal.w), `output` (rgb = filtered radiance, a = the input's age, unclamped). `noise` is a 64 x 64 tile of two
// floats per texel, noise[y][x][2].
//
// What the HLSL leaves to the rasteriser and the samplers is DEFINED in pt_image.h, whose functions are used: pixel uv
// (bloom::pixel_u), the point sampler (img::point_index, clamped in fp32 before the conversion, so nothing indexes outside an image
// whatever the inputs are), ReconstructWorldPos from the view depth (img::recon), log; exp = hrt_exp, pow = hrt_pow, sincos = hrt_sincos,
// frac(x) = x - hrt_floor(x). dist == 0, NaN radiance and the like give what IEEE 754 and the select forms give.
//
// Differences from the reference pass, on purpose:
//   * a miss (depth.x == 1e10f) passes its input texel through; the reference writes 0. Here Output holds the sky at a miss and keeps it.
//   * the noise tile is an input. The reference reads a 64 x 64 blue-noise texture that its tree ships as a data file
//     (external/LDR_RG01_0.png, src/CommonResources.cpp:575); the library may not embed that file, so where the caller passes no tile (and
//     has set none with hrpt_set_denoise_noise) default_tile_texel() below is used, which is WHITE noise (the path tracer's PCG stream per
//     texel), not blue noise. The caller's own copy of the reference's tile gives the reference's behaviour.
// Not restated: the separate specular image with w2, m_SpecularPhi and specularFactor (one radiance image; it plays both signals in the
// age falloff's a + a2), and DecodeNormal (the plane already holds unit vectors).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_image.h"

namespace hrt {
namespace denoise {

using namespace img;

constexpr int kNoiseSize = 64;                                     // srrhi::CommonConsts::kBlueNoiseSize
constexpr size_t kNoiseFloats = (size_t)kNoiseSize * kNoiseSize * 2;
constexpr float kMaxEffectiveAge = 64.0f, kMinAgeFalloff = 0.15f, kPerspectiveScale = 25.0f, kMinKernelTexels = 2.0f, kYoungNormalPhi = 10.0f;

struct Args {
    ViewArgs view;
    float radius, phi, lumaPhi, depthPhi, normalPhi, roughnessPhi;
    uint32_t frame;
};
// radius and frame are those of the pass, not of the params: the context call iterates with radius * 2^i and frame * iterations + i.
HRT_FN Args make_args(const HrptPlanarViewConstants& view, const HrptDenoiseParams& p, float radius, uint32_t frame, int w, int h)
{
    Args a;
    a.view = make_view_args(view, w, h);
    a.radius = radius; a.phi = p.phi; a.lumaPhi = p.lumaPhi; a.depthPhi = p.depthPhi; a.normalPhi = p.normalPhi; a.roughnessPhi = p.roughnessPhi;
    a.frame = frame;
    return a;
}

// The tile used where the caller passes none: texel (x, y) = the first two numbers of the path tracer's stream for pixel (x, y), index 0.
HRT_FN void default_tile_texel(int x, int y, float* rg)
{
    uint32_t state = hrt_rng_seed((uint32_t)x, (uint32_t)y, 0u);
    rg[0] = hrt_rng_next(&state);
    rg[1] = hrt_rng_next(&state);
}

HRT_FN float frac(float x) { return x - hrt_floor(x); }
HRT_FN float luminance(T3 c) { return (c.x * 0.2126f + c.y * 0.7152f) + c.z * 0.0722f; }                  // CommonLighting.hlsli:14
HRT_FN T3 to_denoise_space(T4 c) { return t3(ln(c.x + 1.0f), ln(c.y + 1.0f), ln(c.z + 1.0f)); }
HRT_FN float denoise_luminance(T3 c) { return hrt_pow(luminance(c), 0.125f); }

// SampleBlueNoise (Common.hlsli:92-107): .x and .w of the four numbers, the two the pass uses.
HRT_FN T2 sample_noise(const float* noise, uint32_t px, uint32_t py, uint32_t frame)
{
    const uint32_t mask = (uint32_t)kNoiseSize - 1u;
    const uint32_t p0x = (px + frame * 9491u) & mask, p0y = (py + frame * 7459u) & mask;
    const uint32_t p1x = (px + frame * 5851u + 31u) & mask, p1y = (py + frame * 3917u + 17u) & mask;
    const float ar = noise[((size_t)p0y * kNoiseSize + p0x) * 2], bg = noise[((size_t)p1y * kNoiseSize + p1x) * 2 + 1];
    const float cycleIndex = (float)(frame & 4095u);
    return t2(frac(ar + 0.618033988749895f * cycleIndex), frac(bg + 0.167303978261419f * cycleIndex));
}

// ---- SSGIDenoise_PSMain for pixel (px, py): returns output[p]; colorOut[p] is (its rgb, color[p].a) -------------------------------------
HRT_FN T4 pixel(const Args& a, const float* input, const float* depth, const float* normal, const float* geoNormal, const float* noise, int px, int py)
{
    const float kPoissonDisk[8][2] = { { -1.0f, 0.0f }, { 0.0f, -1.0f }, { 1.0f, 0.0f }, { 0.0f, 1.0f },
                                       { -0.353553f, -0.353553f }, { 0.353553f, -0.353553f }, { 0.353553f, 0.353553f }, { -0.353553f, 0.353553f } };
    const int W = a.view.w, H = a.view.h;
    const T4 C = load4(input, W, px, py), D = load4(depth, W, px, py);
    if (D.x == kMissDepth) return C;

    const float u = bloom::pixel_u(px, W), v = bloom::pixel_u(py, H);
    const float outputAge = C.w;
    const float age = hrt_min(outputAge, kMaxEffectiveAge);
    const float w = 1.0f / hrt_sqrt(age + 1.0f);                   // the younger the pixel, the harder it is filtered

    const T3 Cd = to_denoise_space(C);
    const float centerLum = denoise_luminance(Cd);
    const T4 N4 = load4(normal, W, px, py);
    const T3 N = t3(N4.x, N4.y, N4.z);
    const float rough = N4.w, metal = load4(geoNormal, W, px, py).w;

    const T3 centerWorldPos = recon(a.view, u, v, D.y);
    const float dist = length3(sub(centerWorldPos, t3(a.view.cam[0], a.view.cam[1], a.view.cam[2])));
    const float roughnessRadius = img::lerp(hrt_sqrt(rough), 1.0f, 0.5f * (1.0f - metal));

    const T2 random = sample_noise(noise, (uint32_t)px, (uint32_t)py, a.frame);          // .x = random.r, .y = random.a

    const float ageFalloff = hrt_max(hrt_exp(-(age + age) * 0.01f), kMinAgeFalloff);
    const float r = ((hrt_sqrt(random.y) * ageFalloff) * a.radius) * roughnessRadius;
    float s, c;
    hrt_sincos((random.x * 2.0f) * HRT_PI, &s, &c);
    const float diskScale = hrt_clamp((r * kPerspectiveScale) / dist, kMinKernelTexels, a.radius * 4.0f);

    T3 sum = Cd;
    float total = 1.0f;
    for (int i = 0; i < 8; ++i) {
        const float dx = kPoissonDisk[i][0], dy = kPoissonDisk[i][1];
        const float rx = dx * c - dy * s, ry = dx * s + dy * c;
        const float nu = u + (rx * diskScale) * a.view.sizeInv[0], nv = v + (ry * diskScale) * a.view.sizeInv[1];
        const int qx = point_index(nu, W), qy = point_index(nv, H);
        const T4 nD = load4(depth, W, qx, qy);
        if (nD.x == kMissDepth) continue;

        const T3 nC = to_denoise_space(load4(input, W, qx, qy));
        const float nLum = denoise_luminance(nC);
        const T4 nN = load4(normal, W, qx, qy);
        const T3 nWorldPos = recon(a.view, nu, nv, nD.y);

        const float normalDiff = 1.0f - hrt_max(dot3(N, t3(nN.x, nN.y, nN.z)), 0.0f);
        const float depthDiff = 10.0f * hrt_abs(dot3(sub(centerWorldPos, nWorldPos), N));        // plane distance
        const float roughnessDiff = hrt_abs(rough - nN.w);
        const float lumaDiff = img::lerp(hrt_abs(centerLum - nLum), 0.0f, w);

        const float wBasic = hrt_exp(((-normalDiff * a.normalPhi) - depthDiff * a.depthPhi) - roughnessDiff * a.roughnessPhi);
        const float wBasicD = img::lerp(wBasic, hrt_exp(-normalDiff * kYoungNormalPhi), w);
        const float wDiff = hrt_min(w * hrt_pow(wBasicD * hrt_exp(-lumaDiff * a.lumaPhi), a.phi / w), 1.0f);

        sum = t3(sum.x + wDiff * nC.x, sum.y + wDiff * nC.y, sum.z + wDiff * nC.z);
        total = total + wDiff;
    }
    return t4(hrt_exp(sum.x / total) - 1.0f, hrt_exp(sum.y / total) - 1.0f, hrt_exp(sum.z / total) - 1.0f, outputAge);
}

} // namespace denoise
} // namespace hrt

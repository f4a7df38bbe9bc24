// pt_temporal.h -- the arithmetic of hrpt_temporal_accumulate, one __host__ __device__ source shared by the gfx950 kernel (pt_temporal.hip)
// and hrpt_temporal_host (pt_temporal_host.cpp): the reference's SSGI temporal pass, src/shaders/SSGITemporalReproject.hlsl
// (SSGIValidateReprojection :28-47, SSGITemporalAccumulate :50-82, SSGITemporal_PSMain :90-170) with SampleTextureCatmullRom and
// ReconstructWorldPos of src/shaders/Common.hlsli:111-172, restated statement for statement over the path tracer's own images in the
// arithmetic of hobbyrt/detmath.h: no FMA contraction, correctly rounded '/' and sqrt, select-form min / max / clamp, sums and dot products
// left to right. DESIGN.md section 17 has the definition in prose.
//
// Images are W x H float4, row-major: `color` (Output of hrpt_render), `motion` (hrpt_render_motion_vectors), `depth` and `normal` (the
// planes HRPT_GB_DEPTH and HRPT_GB_NORMAL of the same frame), `historyIn` / `historyOut` (rgb = accumulated radiance, a = age).
//
// What the HLSL leaves to the rasteriser and the samplers is DEFINED in pt_image.h, whose functions are used: pixel uv, the linear and the
// point sampler (every float -> int conversion is defined for every input), ReconstructWorldPos from the view depth, log. Here:
//   * exp = hrt_exp, pow = hrt_pow
//   * a miss (depth.x == kMissDepth) passes its colour through with age 0. A reprojection that lands on a miss texel has confidence 0; the
//     reference gets there through an infinite reconstructed position, here it is stated.
//
// Differences from the reference pass, on purpose:
//   * no history (first frame, reset, resize): acc = 0 AND confidence = 0, so temporalMix = 0, the output is the input and the age is 0.
//     The reference starts from a cleared texture with whatever confidence the validation gives, which blends in a phantom black frame.
//   * HRPT_TEMPORAL_LINEAR: the log(1 + x) / exp(x) - 1 pair around the blend becomes the identity. The reference's log-space blend is
//     biased for Monte-Carlo radiance; in linear space a static scene is the exact running mean.
//   * the specular / hit-parallax branch and the "not sampled" sentinel are not here: one radiance image, every pixel sampled.
// As in the reference, the validation reads the CURRENT frame's depth and motion at the reprojected position; no previous G-buffer is kept.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_image.h"

namespace hrt {
namespace temporal {

using namespace img;

// The view and what else the pass reads of the two HrptPlanarViewConstants and the params, gathered once per call.
struct Args {
    ViewArgs view;
    float jitterOffsetUV[2];        // (prevView->m_PixelOffset - view->m_PixelOffset) * m_ViewportSizeInv
    float blend;
    uint32_t flags;
};
HRT_FN Args make_args(const HrptPlanarViewConstants& view, const HrptPlanarViewConstants& prev, float blend, uint32_t flags, int w, int h)
{
    Args a;
    a.view = make_view_args(view, w, h);
    for (int i = 0; i < 2; ++i) a.jitterOffsetUV[i] = (prev.m_PixelOffset[i] - view.m_PixelOffset[i]) * view.m_ViewportSizeInv[i];
    a.blend = blend; a.flags = flags;
    return a;
}

// ---- SampleTextureCatmullRom (Common.hlsli:111-164) ----------------------------------------------------------------------------------
struct CrAxis { float w0, w12, w3, p0, p12, p3, p1uv, p2uv; };
HRT_FN CrAxis catmull_axis(float uv, float res)
{
    const float samplePos = uv * res;
    const float texPos1 = hrt_floor(samplePos - 0.5f) + 0.5f;
    const float f = samplePos - texPos1;
    const float w0 = f * (-0.5f + f * (1.0f - 0.5f * f));
    const float w1 = 1.0f + (f * f) * (-2.5f + 1.5f * f);
    const float w2 = f * (0.5f + f * (2.0f - 1.5f * f));
    const float w3 = (f * f) * (-0.5f + 0.5f * f);
    CrAxis r;
    r.w0 = w0; r.w12 = w1 + w2; r.w3 = w3;
    const float offset12 = w2 / (w1 + w2);
    r.p0 = (texPos1 - 1.0f) / res; r.p3 = (texPos1 + 2.0f) / res; r.p12 = (texPos1 + offset12) / res;
    r.p1uv = texPos1 / res; r.p2uv = (texPos1 + 1.0f) / res;
    return r;
}
HRT_FN T4 madd(T4 result, T4 s, float wx, float wy)                                           // result += s * wx * wy
{
    return t4(result.x + (s.x * wx) * wy, result.y + (s.y * wx) * wy, result.z + (s.z * wx) * wy, result.w + (s.w * wx) * wy);
}
HRT_FN T4 min4(T4 a, T4 b) { return t4(hrt_min(a.x, b.x), hrt_min(a.y, b.y), hrt_min(a.z, b.z), hrt_min(a.w, b.w)); }
HRT_FN T4 max4(T4 a, T4 b) { return t4(hrt_max(a.x, b.x), hrt_max(a.y, b.y), hrt_max(a.z, b.z), hrt_max(a.w, b.w)); }
HRT_FN T4 catmull_rom(const float* tex, int w, int h, float u, float v, float resX, float resY)
{
    const CrAxis X = catmull_axis(u, resX), Y = catmull_axis(v, resY);
    T4 result = t4(0.0f, 0.0f, 0.0f, 0.0f);
    result = madd(result, sample_linear(tex, w, h, X.p0, Y.p0), X.w0, Y.w0);
    result = madd(result, sample_linear(tex, w, h, X.p12, Y.p0), X.w12, Y.w0);
    result = madd(result, sample_linear(tex, w, h, X.p3, Y.p0), X.w3, Y.w0);
    result = madd(result, sample_linear(tex, w, h, X.p0, Y.p12), X.w0, Y.w12);
    result = madd(result, sample_linear(tex, w, h, X.p12, Y.p12), X.w12, Y.w12);
    result = madd(result, sample_linear(tex, w, h, X.p3, Y.p12), X.w3, Y.w12);
    result = madd(result, sample_linear(tex, w, h, X.p0, Y.p3), X.w0, Y.w3);
    result = madd(result, sample_linear(tex, w, h, X.p12, Y.p3), X.w12, Y.w3);
    result = madd(result, sample_linear(tex, w, h, X.p3, Y.p3), X.w3, Y.w3);
    // anti-ringing: clamp to the 2 x 2 neighbourhood
    const T4 c00 = sample_linear(tex, w, h, X.p1uv, Y.p1uv), c10 = sample_linear(tex, w, h, X.p2uv, Y.p1uv);
    const T4 c01 = sample_linear(tex, w, h, X.p1uv, Y.p2uv), c11 = sample_linear(tex, w, h, X.p2uv, Y.p2uv);
    const T4 lo = min4(min4(c00, c10), min4(c01, c11)), hi = max4(max4(c00, c10), max4(c01, c11));
    return t4(hrt_clamp(hrt_max(result.x, 0.0f), lo.x, hi.x), hrt_clamp(hrt_max(result.y, 0.0f), lo.y, hi.y),
              hrt_clamp(hrt_max(result.z, 0.0f), lo.z, hi.z), hrt_clamp(hrt_max(result.w, 0.0f), lo.w, hi.w));
}

// ---- SSGIValidateReprojection (:28-47); haveHistory == false is this library's "no history" rule ----------------------------------------
HRT_FN float validate(const Args& a, const float* motion, const float* depth, bool haveHistory, T2 reprojUV, T3 worldPos, T3 worldNormal, T2 velocityUV)
{
    if (!haveHistory) return 0.0f;
    if (reprojUV.x < 0.0f || reprojUV.x > 1.0f || reprojUV.y < 0.0f || reprojUV.y > 1.0f) return 0.0f;
    const int qx = point_index(reprojUV.x, a.view.w), qy = point_index(reprojUV.y, a.view.h);
    const T4 lastDepth = load4(depth, a.view.w, qx, qy);
    if (lastDepth.x == kMissDepth) return 0.0f;
    const T4 lastMotion = load4(motion, a.view.w, qx, qy);
    const T2 lastVelocityUV = t2(lastMotion.x * a.view.sizeInv[0], lastMotion.y * a.view.sizeInv[1]);
    const T3 lastWorldPos = recon(a.view, reprojUV.x, reprojUV.y, lastDepth.y);

    const float viewDist = length3(sub(worldPos, t3(a.view.cam[0], a.view.cam[1], a.view.cam[2])));
    const float distFactor = 1.0f + 1.0f / (viewDist + 1.0f);

    const T3 d = sub(worldPos, lastWorldPos);
    float disoccl = 0.0f;
    disoccl = disoccl + length2(t2(velocityUV.x - lastVelocityUV.x, velocityUV.y - lastVelocityUV.y)) / 0.005f * distFactor;   // velocity delta
    disoccl = disoccl + hrt_abs(dot3(d, worldNormal)) / 2.5f * distFactor;                                                   // plane distance
    disoccl = disoccl + length3(d) / 2.5f * distFactor;                                                                      // world distance
    disoccl = hrt_min(disoccl / 3.0f, 1.0f);
    return 1.0f - disoccl;
}

// ---- SSGITemporal_PSMain for pixel (px, py) ------------------------------------------------------------------------------------------------
HRT_FN void pixel(const Args& a, const float* color, const float* motion, const float* depth, const float* normal, const float* historyIn,
                  int px, int py, T4* historyOut, T4* colorOut)
{
    const int W = a.view.w, H = a.view.h;
    const T4 C = load4(color, W, px, py), D = load4(depth, W, px, py);
    if (D.x == kMissDepth) { *historyOut = t4(C.x, C.y, C.z, 0.0f); *colorOut = C; return; }

    const float u = bloom::pixel_u(px, W), v = bloom::pixel_u(py, H);
    const T3 worldPos = recon(a.view, u, v, D.y);
    const T4 N4 = load4(normal, W, px, py);
    const T3 worldNormal = t3(N4.x, N4.y, N4.z);

    const T4 mv = load4(motion, W, px, py);
    const T2 velocityUV = t2(mv.x * a.view.sizeInv[0], mv.y * a.view.sizeInv[1]);
    const T2 reprojUV = t2(u + velocityUV.x, v + velocityUV.y);
    const T2 reprojNoJitter = t2(reprojUV.x - a.jitterOffsetUV[0], reprojUV.y - a.jitterOffsetUV[1]);

    const bool haveHistory = historyIn != nullptr;
    float confidence = validate(a, motion, depth, haveHistory, reprojNoJitter, worldPos, worldNormal, velocityUV);

    const float moveFactor = hrt_saturate(length2(t2(velocityUV.x * a.view.size[0], velocityUV.y * a.view.size[1])) - 1.0f);

    // SSGITemporalAccumulate, bWasSampled = true
    T4 acc = haveHistory ? catmull_rom(historyIn, W, H, reprojUV.x, reprojUV.y, a.view.size[0], a.view.size[1]) : t4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool linear = (a.flags & HRPT_TEMPORAL_LINEAR) != 0;
    T3 inp = t3(C.x, C.y, C.z);
    if (!linear) {
        acc.x = ln(acc.x + 1.0f); acc.y = ln(acc.y + 1.0f); acc.z = ln(acc.z + 1.0f);
        inp = t3(ln(inp.x + 1.0f), ln(inp.y + 1.0f), ln(inp.z + 1.0f));
    }
    acc.w = acc.w + 1.0f;

    confidence = hrt_pow(confidence, 0.25f);
    float accumBlend = 1.0f - 1.0f / (acc.w + 1.0f);
    accumBlend = lerp(0.0f, accumBlend, confidence);
    const float maxValue = lerp(1.0f, a.blend, moveFactor);
    const float temporalMix = hrt_min(accumBlend, maxValue);

    T3 out = t3(lerp(inp.x, acc.x, temporalMix), lerp(inp.y, acc.y, temporalMix), lerp(inp.z, acc.z, temporalMix));
    const float outputAge = 1.0f / hrt_max(1.0f - temporalMix, HRT_K_EPSILON) - 1.0f;
    if (!linear) out = t3(hrt_exp(out.x) - 1.0f, hrt_exp(out.y) - 1.0f, hrt_exp(out.z) - 1.0f);

    *historyOut = t4(out.x, out.y, out.z, outputAge);
    *colorOut = t4(out.x, out.y, out.z, C.w);
}

} // namespace temporal
} // namespace hrt

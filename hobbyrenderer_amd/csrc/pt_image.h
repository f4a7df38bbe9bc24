// pt_image.h -- the image arithmetic the screen-space stages share (pt_temporal.h, pt_denoise.h, pt_modulation.h): the small vector types, the
// texel loads and samplers, ReconstructWorldPos of src/shaders/Common.hlsli:50-53, 167-172 with the view members it reads. The kernels'
// tile prologue is pt_image_kernel.h; the host executors' row loop is pt_host_rows.h. One __host__ __device__ source in the arithmetic of
// hobbyrt/detmath.h: no FMA contraction, correctly rounded '/' and sqrt, select-form min / max / clamp, sums and dot products left to right.
//
// What the HLSL leaves to the rasteriser and the samplers is DEFINED here, as in pt_bloom.h (whose functions are used):
//   * pixel uv: bloom::pixel_u; SampleLevel(linearClamp, uv, 0): bloom::axis / bloom::taps and the a(1 - t) + bt filter, on all four channels
//   * SampleLevel(pointClamp, r, 0): the texel ix = (int)clamp(floor(r.x * W), 0, W - 1), iy likewise -- clamped in fp32 before the
//     conversion, so the float -> int conversion is defined for every input (NaN converts as 0) and nothing indexes outside an image
//   * log(x) = hrt_log2(x) * 0.69314718f
//   * device depth: the path tracer keeps the VIEW depth vd (HRPT_GB_DEPTH.y); the reference's reversed-Z value that ReconstructWorldPos
//     takes is z = (vd * P[10] + P[14]) / vd with P = m_MatViewToClip
//   * a pixel is a miss when depth.x == kMissDepth (the sentinel of hrpt_render_gbuffer; the reference's DEPTH_FAR test)
//   * normalize, cross and reflect: as pt_modulation.h's header states them
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_bloom.h"

namespace hrt {
namespace img {

constexpr float kMissDepth = 1e10f;           // HRPT_GB_DEPTH.x of a pixel whose primary ray hit nothing
constexpr float kLn2 = 0.69314718f;

struct T2 { float x, y; };
struct T3 { float x, y, z; };
struct T4 { float x, y, z, w; };
HRT_FN T2 t2(float x, float y) { T2 r; r.x = x; r.y = y; return r; }
HRT_FN T3 t3(float x, float y, float z) { T3 r; r.x = x; r.y = y; r.z = z; return r; }
HRT_FN T4 t4(float x, float y, float z, float w) { T4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
HRT_FN T4 load4(const float* img, int w, int x, int y) { const float* p = img + ((size_t)y * (size_t)w + (size_t)x) * 4; return t4(p[0], p[1], p[2], p[3]); }
HRT_FN T3 sub(T3 a, T3 b) { return t3(a.x - b.x, a.y - b.y, a.z - b.z); }
HRT_FN T3 add(T3 a, T3 b) { return t3(a.x + b.x, a.y + b.y, a.z + b.z); }
HRT_FN T3 neg(T3 a) { return t3(-a.x, -a.y, -a.z); }
HRT_FN T3 cross(T3 a, T3 b) { return t3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
HRT_FN float dot3(T3 a, T3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
HRT_FN float length3(T3 a) { return hrt_sqrt(dot3(a, a)); }
HRT_FN float length2(T2 a) { return hrt_sqrt(a.x * a.x + a.y * a.y); }
HRT_FN T3 normalize(T3 v) { const float len = length3(v); return t3(v.x / len, v.y / len, v.z / len); }
HRT_FN T3 reflect(T3 i, T3 n) { const float k = 2.0f * dot3(n, i); return t3(i.x - k * n.x, i.y - k * n.y, i.z - k * n.z); }
HRT_FN float lerp(float a, float b, float t) { return a + t * (b - a); }                      // pt_vec.h lerp
HRT_FN float ln(float x) { return hrt_log2(x) * kLn2; }

// The members of an HrptPlanarViewConstants that recon and the stages read, gathered once per call.
struct ViewArgs {
    float clipToWorld[16];          // view->m_MatClipToWorld
    float p10, p14;                 // view->m_MatViewToClip[10], [14]
    float size[2], sizeInv[2];      // view->m_ViewportSize, m_ViewportSizeInv
    float cam[3];                   // view->m_CameraDirectionOrPosition.xyz
    int w, h;
};
HRT_FN ViewArgs make_view_args(const HrptPlanarViewConstants& view, int w, int h)
{
    ViewArgs a;
    for (int i = 0; i < 16; ++i) a.clipToWorld[i] = view.m_MatClipToWorld[i];
    a.p10 = view.m_MatViewToClip[10]; a.p14 = view.m_MatViewToClip[14];
    for (int i = 0; i < 2; ++i) { a.size[i] = view.m_ViewportSize[i]; a.sizeInv[i] = view.m_ViewportSizeInv[i]; }
    for (int i = 0; i < 3; ++i) a.cam[i] = view.m_CameraDirectionOrPosition[i];
    a.w = w; a.h = h;
    return a;
}

// ---- samplers ------------------------------------------------------------------------------------------------------------------------
HRT_FN int point_index(float r, int n) { return (int)hrt_clamp(hrt_floor(r * (float)n), 0.0f, (float)(n - 1)); }
HRT_FN T4 lerp4(T4 a, T4 b, float t)
{
    const float w = 1.0f - t;
    return t4(a.x * w + b.x * t, a.y * w + b.y * t, a.z * w + b.z * t, a.w * w + b.w * t);
}
HRT_FN T4 sample_linear(const float* img, int w, int h, float u, float v)
{
    const bloom::Taps t = bloom::taps(u, v, w, h);
    return lerp4(lerp4(load4(img, w, t.x0, t.y0), load4(img, w, t.x1, t.y0), t.fx), lerp4(load4(img, w, t.x0, t.y1), load4(img, w, t.x1, t.y1), t.fx), t.fy);
}

// ---- ReconstructWorldPos (Common.hlsli:50-53, 167-172) from a view depth ------------------------------------------------------------
HRT_FN T3 recon(const ViewArgs& a, float u, float v, float vd)
{
    const float z = (vd * a.p10 + a.p14) / vd;
    const float cx = u * 2.0f + -1.0f, cy = v * -2.0f + 1.0f;                                // UVToClipXY
    const float* M = a.clipToWorld;                                                          // float4(clipXY, z, 1) * M, left to right
    const float hx = ((cx * M[0] + cy * M[4]) + z * M[8]) + 1.0f * M[12];
    const float hy = ((cx * M[1] + cy * M[5]) + z * M[9]) + 1.0f * M[13];
    const float hz = ((cx * M[2] + cy * M[6]) + z * M[10]) + 1.0f * M[14];
    const float hw = ((cx * M[3] + cy * M[7]) + z * M[11]) + 1.0f * M[15];
    return t3(hx / hw, hy / hw, hz / hw);
}

} // namespace img
} // namespace hrt

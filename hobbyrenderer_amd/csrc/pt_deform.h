// pt_deform.h -- the arithmetic of the vertex quantiser (hrpt_quantize_vertices_host / _device, hrpt_update_vertices_device), one
// __host__ __device__ source shared by the gfx950 kernel (pt_deform.hip) and the host executor (pt_deform_host.cpp): QuantizeSnorm,
// QuantizeHalf and the body of QuantizeVertex (host/ProceduralScenes.cpp:9-49; meshopt_quantizeSnorm / meshopt_quantizeHalf) restated
// statement for statement, so that a float vertex (HrptVertexFloat, 48 B) becomes the 24-byte HrptVertexQuantized a scene file holds,
// bit for bit: hobbyrenderer_amd/scenes.py quantize_vertices states the same in NumPy. DESIGN.md section 21 has the definition in prose.
//
//   m_Pos      the three position floats, copied
//   m_Normal   snorm10(n.x) + 511 | (snorm10(n.y) + 511) << 10 | (snorm10(n.z) + 511) << 20 | (tangent[3] < 0) << 30
//   m_Uv       half(uv.x) | half(uv.y) << 16
//   m_Tangent  octahedral, 8 bits per component: with sum = (|t.x| + |t.y|) + |t.z|, 0 unless sum > 1e-6f; else (o.x, o.y) =
//              (t.x / sum, t.y / sum) for t.z >= 0 and ((1 - |t.y / sum|) * sign(t.x), (1 - |t.x / sum|) * sign(t.y)) otherwise
//              (sign(x) = x >= 0 ? 1 : -1), stored as snorm8(o.x) + 127 | (snorm8(o.y) + 127) << 8
//   snorm(v, bits) = (int)(clamp(v) * scale + (v >= 0 ? 0.5f : -0.5f)), scale = 2^(bits - 1) - 1, the clamp to [-1, 1] by two selects,
//              one rounding per operation (no FMA contraction), the cast truncating toward zero
//   half(v)    the integer conversion of meshopt_quantizeHalf: round half up on the magnitude, denormals flushed, saturation to inf, NaN 0x7e00
//
// One deviation from the C source: a NaN fed to snorm counts as 0.0f (a NaN normal component; inf / inf from an infinite tangent). The C
// source's cast of such a value is undefined, and v_cvt_i32_f32 and x86's cvttss2si disagree on it. Everything else non-finite is
// defined by the statements above: an infinite normal component clamps to +-1, uv goes through integer arithmetic alone, a NaN anywhere
// in the tangent makes the sum NaN and the tangent word 0, a NaN tangent[3] is not < 0.
// A position that is not finite is copied like any other; position_finite() is what the callers raise their flag on.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/hobbyrt_pt.h"

#if defined(__HIPCC__)
#define HRT_DEFORM_HD __host__ __device__ inline
#else
#define HRT_DEFORM_HD inline
#endif

namespace hrt {
namespace deform {

// (the copies fold to register moves on both sides)
HRT_DEFORM_HD uint32_t float_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
HRT_DEFORM_HD float fabs_bits(float v) { uint32_t u = float_bits(v) & 0x7fffffffu; float r; __builtin_memcpy(&r, &u, 4); return r; }

HRT_DEFORM_HD int quantize_snorm(float v, int bits)
{
    const float scale = (float)((1 << (bits - 1)) - 1);
    v = (v != v) ? 0.0f : v;                               // the deviation: NaN counts as 0
    const float round = (v >= 0.0f ? 0.5f : -0.5f);
    v = (v >= -1.0f) ? v : -1.0f;
    v = (v <= 1.0f) ? v : 1.0f;
    return (int)(v * scale + round);
}

HRT_DEFORM_HD uint32_t quantize_half(float v)
{
    const uint32_t ui = float_bits(v);
    const int s = (int)((ui >> 16) & 0x8000u);
    const int em = (int)(ui & 0x7fffffffu);
    int h = (int)(((uint32_t)em - (112u << 23) + (1u << 12)) >> 13);      // (unsigned: the values the selects below keep are the same)
    h = (em < (113 << 23)) ? 0 : h;
    h = (em >= (143 << 23)) ? 0x7c00 : h;
    h = (em > (255 << 23)) ? 0x7e00 : h;
    return (uint32_t)(s | h) & 0xffffu;
}

HRT_DEFORM_HD bool position_finite(const float* pos)
{
    return (float_bits(pos[0]) & 0x7f800000u) != 0x7f800000u && (float_bits(pos[1]) & 0x7f800000u) != 0x7f800000u &&
           (float_bits(pos[2]) & 0x7f800000u) != 0x7f800000u;
}

// The three packed words of a vertex (m_Normal, m_Uv, m_Tangent) from its normal, uv and tangent (xyz + handedness sign).
HRT_DEFORM_HD void quantize_attributes(const float* normal, const float* uv, const float* tangent, uint32_t& outNormal, uint32_t& outUv, uint32_t& outTangent)
{
    uint32_t n = 0;
    for (int k = 0; k < 3; ++k) n |= (uint32_t)(quantize_snorm(normal[k], 10) + 511) << (10 * k);
    if (tangent[3] < 0.0f) n |= 1u << 30;
    outNormal = n;
    outUv = quantize_half(uv[0]) | (quantize_half(uv[1]) << 16);
    uint32_t t = 0;
    const float sum = (fabs_bits(tangent[0]) + fabs_bits(tangent[1])) + fabs_bits(tangent[2]);
    if (sum > 1e-6f) {
        float ox, oy;
        if (tangent[2] >= 0.0f) { ox = tangent[0] / sum; oy = tangent[1] / sum; }
        else {
            ox = (1.0f - fabs_bits(tangent[1] / sum)) * (tangent[0] >= 0.0f ? 1.0f : -1.0f);
            oy = (1.0f - fabs_bits(tangent[0] / sum)) * (tangent[1] >= 0.0f ? 1.0f : -1.0f);
        }
        t = (uint32_t)(quantize_snorm(ox, 8) + 127) | ((uint32_t)(quantize_snorm(oy, 8) + 127) << 8);
    }
    outTangent = t;
}

HRT_DEFORM_HD HrptVertexQuantized quantize_vertex(const HrptVertexFloat& v)
{
    HrptVertexQuantized q;
    q.m_Pos[0] = v.pos[0]; q.m_Pos[1] = v.pos[1]; q.m_Pos[2] = v.pos[2];
    quantize_attributes(v.normal, v.uv, v.tangent, q.m_Normal, q.m_Uv, q.m_Tangent);
    return q;
}

} // namespace deform
} // namespace hrt

// pt_bloom.h -- the arithmetic of the bloom stage, one __host__ __device__ source shared by the gfx950 kernels (pt_bloom.hip) and
// hrpt_bloom_host: /root/reference/src/shaders/Bloom.hlsl restated statement for statement in the arithmetic of hobbyrt/detmath.h
// (no FMA contraction, correctly rounded '/', select-form min / max / clamp), expression order as written in the HLSL, as driven by
// BloomRenderer::Render (src/BloomRenderer.cpp:48-175, kBloomMipCount = 6).
//
// What the HLSL leaves to the rasteriser, the sampler and the render-target format is DEFINED here (parity with a
// D3D12 driver is unpinned for all three, like SampleGrad's level of detail):
//   * pixel uv of a full-screen pass over a w x h target: ((px + 0.5f) / w, (py + 0.5f) / h)
//   * SampleLevel(linearClamp, uv, 0): x = u * w - 0.5, x0 = floor(x), fx = x - x0, texels x0 and x0 + 1 clamped to [0, w - 1] (same in
//     y), fp32 weights, a(1 - t) + bt along x, then along y -- the filter DESIGN section 2 fixes for textures (lerp4 of pt_vec.h)
//   * the pyramids are R11G11B10_FLOAT (BloomRenderer.cpp:31): every pass's result is rounded into one 32-bit word -- R bits 0-10 and
//     G bits 11-21 with 5 exponent + 6 mantissa bits, B bits 22-31 with 5 + 5, bias 15, no sign -- and every sample reads the unpacked
//     values. From fp32: negative -> 0, NaN -> NaN, +inf -> inf, anything else ROUNDS TOWARD ZERO (so a value above the largest finite
//     one, 65024 / 64512, becomes it), denormals kept. This is the Direct3D float-to-smaller-float rule as the author recalls it; the
//     specification was not at hand when this was written.
//   * levels: level i is ((W / 2) >> i) x ((H / 2) >> i); L = number of i in 0..5 with both sides >= 1. The reference's down loop stops
//     at the first empty level while its up loop would still sample the never-written one; here the up chain is seeded from Down[L - 1]
//     and L = 0 makes the stage a no-op. For W, H >= 64 this is the reference's schedule exactly.
#pragma once

#include <stdint.h>

#include "../../include/hobbyrt/detmath.h"

namespace hrt {
namespace bloom {

constexpr int kMipCount = 6;                 // kBloomMipCount, src/BloomRenderer.cpp:9

struct B3 { float x, y, z; };
HRT_FN B3 b3(float x, float y, float z) { B3 r; r.x = x; r.y = y; r.z = z; return r; }
HRT_FN B3 add(B3 a, B3 b) { return b3(a.x + b.x, a.y + b.y, a.z + b.z); }
HRT_FN B3 mul(B3 a, float s) { return b3(a.x * s, a.y * s, a.z * s); }

HRT_FN int level_count(uint32_t W, uint32_t H)
{
    int n = 0;
    while (n < kMipCount && ((W / 2u) >> n) >= 1u && ((H / 2u) >> n) >= 1u) ++n;
    return n;
}

// ---- R11G11B10_FLOAT ----------------------------------------------------------------------------------------------------------------
// One channel with 5 exponent bits and M mantissa bits (M = 6 or 5).
template <int M> HRT_FN uint32_t to_small_float(float f)
{
    const uint32_t u = hrt_f2u(f), mask = (1u << M) - 1u;
    if ((u & 0x7fffffffu) > 0x7f800000u) return (31u << M) | (1u << (M - 1));       // NaN -> quiet NaN
    if (u & 0x80000000u) return 0u;                                                  // negative (and -0, -inf) -> 0
    if (u == 0x7f800000u) return 31u << M;                                           // +inf
    const int e = (int)(u >> 23) - 127 + 15;
    if (e >= 31) return (30u << M) | mask;                                           // above the largest finite value -> it
    if (e >= 1) return ((uint32_t)e << M) | ((u >> (23 - M)) & mask);                // normal: drop the low mantissa bits
    const int shift = (23 - M) + (1 - e);                                            // denormal: units of 2^(-14 - M)
    return shift >= 24 ? 0u : (((u & 0x007fffffu) | 0x00800000u) >> shift);
}
// `bits` = the channel's exponent and mantissa moved into the exponent / mantissa fields of an fp32 (channel << (23 - M)): that fp32 is the
// channel's value times 2^-112, a denormal fp32 where the channel is denormal, so ONE exact multiplication by 2^112 decodes normal and
// denormal channels alike (denormals are kept on both targets, detmath.h); exponent 31 is inf / NaN. Branch-free: a downsample decodes
// 156 channels per texel, and the first version of this function (three-way branch per channel) made that 12 us of dependent
// instructions per texel on the MI355X.
HRT_FN float from_small_float_bits(uint32_t bits)
{
    const float f = hrt_u2f(bits) * hrt_u2f(0x77800000u);                            // * 2^112
    return bits >= (31u << 23) ? hrt_u2f(bits | 0x7f800000u) : f;
}
template <int M> HRT_FN float from_small_float(uint32_t v) { return from_small_float_bits(v << (23 - M)); }
HRT_FN uint32_t pack(B3 c) { return to_small_float<6>(c.x) | (to_small_float<6>(c.y) << 11) | (to_small_float<5>(c.z) << 22); }
HRT_FN B3 unpack(uint32_t p)
{
    return b3(from_small_float_bits((p << 17) & 0x0ffe0000u), from_small_float_bits((p << 6) & 0x0ffe0000u), from_small_float_bits((p >> 4) & 0x0ffc0000u));
}

// ---- SampleLevel(linearClamp, uv, 0) ------------------------------------------------------------------------------------------------
struct Taps { int x0, x1, y0, y1; float fx, fy; };
HRT_FN void axis(float u, int n, int* i0, int* i1, float* f)
{
    const float x = u * (float)n - 0.5f;
    const float x0 = hrt_floor(x);
    *f = x - x0;
    const int i = (int)hrt_clamp(x0, -1.0f, (float)n);       // clamped in fp32 first: the conversion is defined for every input
    *i0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    *i1 = i + 1 < 0 ? 0 : (i + 1 > n - 1 ? n - 1 : i + 1);
}
HRT_FN Taps taps(float u, float v, int w, int h) { Taps t; axis(u, w, &t.x0, &t.x1, &t.fx); axis(v, h, &t.y0, &t.y1, &t.fy); return t; }
HRT_FN B3 lerp3(B3 a, B3 b, float t) { const float w = 1.0f - t; return b3(a.x * w + b.x * t, a.y * w + b.y * t, a.z * w + b.z * t); }
HRT_FN B3 filter(B3 t00, B3 t10, B3 t01, B3 t11, float fx, float fy) { return lerp3(lerp3(t00, t10, fx), lerp3(t01, t11, fx), fy); }

// a level of a pyramid (packed words, row-major, w x h); works on global memory, LDS and host memory alike
HRT_FN B3 sample_packed(const uint32_t* tex, int w, int h, float u, float v)
{
    const Taps t = taps(u, v, w, h);
    const uint32_t* r0 = tex + (size_t)t.y0 * (size_t)w; const uint32_t* r1 = tex + (size_t)t.y1 * (size_t)w;
    const uint32_t p00 = r0[t.x0], p10 = r0[t.x1], p01 = r1[t.x0], p11 = r1[t.x1];
    return filter(unpack(p00), unpack(p10), unpack(p01), unpack(p11), t.fx, t.fy);
}
// the HDR colour target (float4 per pixel), .rgb
HRT_FN B3 sample_hdr(const float* img, int w, int h, float u, float v)
{
    const Taps t = taps(u, v, w, h);
    const float* a = img + ((size_t)t.y0 * (size_t)w + (size_t)t.x0) * 4; const float* b = img + ((size_t)t.y0 * (size_t)w + (size_t)t.x1) * 4;
    const float* c = img + ((size_t)t.y1 * (size_t)w + (size_t)t.x0) * 4; const float* d = img + ((size_t)t.y1 * (size_t)w + (size_t)t.x1) * 4;
    return filter(b3(a[0], a[1], a[2]), b3(b[0], b[1], b[2]), b3(c[0], c[1], c[2]), b3(d[0], d[1], d[2]), t.fx, t.fy);
}
HRT_FN float pixel_u(int px, int w) { return ((float)px + 0.5f) / (float)w; }

// ---- Prefilter_PSMain (Bloom.hlsl:18-43): HDR colour (W x H) -> Down[0] (w x h) -------------------------------------------------------
HRT_FN B3 safe_hdr(B3 c) { return b3(hrt_min(c.x, 65504.0f), hrt_min(c.y, 65504.0f), hrt_min(c.z, 65504.0f)); }
HRT_FN B3 prefilter(B3 color, float knee)
{
    const float brightness = hrt_max(color.x, hrt_max(color.y, color.z));
    float soft = brightness + knee;
    soft = hrt_clamp(soft, 0.0f, 2.0f * knee);
    soft = (soft * soft) / (4.0f * knee + 1e-6f);
    float contribution = hrt_max(soft, brightness);
    contribution = contribution / hrt_max(brightness, 1e-4f);
    return mul(color, contribution);
}
HRT_FN uint32_t prefilter_texel(const float* hdr, int W, int H, int w, int h, int px, int py, float knee)
{
    const B3 color = sample_hdr(hdr, W, H, pixel_u(px, w), pixel_u(py, h));
    return pack(mul(prefilter(safe_hdr(color), knee), 1.0f));                        // m_Strength = 1 (BloomRenderer.cpp:64)
}

// ---- Downsample_PSMain (Bloom.hlsl:47-86): Jimenez 13 taps, src (sw x sh) -> target (w x h) -------------------------------------------
HRT_FN uint32_t down_texel(const uint32_t* src, int sw, int sh, int w, int h, int px, int py)
{
    const float tx = 1.0f / (float)w, ty = 1.0f / (float)h;
    const float u = pixel_u(px, w), v = pixel_u(py, h);
    const float um1 = u + -1.0f * tx, u0 = u + 0.0f * tx, up1 = u + 1.0f * tx, umh = u + -0.5f * tx, uph = u + 0.5f * tx;
    const float vm1 = v + -1.0f * ty, v0 = v + 0.0f * ty, vp1 = v + 1.0f * ty, vmh = v + -0.5f * ty, vph = v + 0.5f * ty;
    const B3 a = sample_packed(src, sw, sh, um1, vm1), b = sample_packed(src, sw, sh, u0, vm1), c = sample_packed(src, sw, sh, up1, vm1);
    const B3 d = sample_packed(src, sw, sh, umh, vmh), e = sample_packed(src, sw, sh, uph, vmh);
    const B3 f = sample_packed(src, sw, sh, um1, v0), g = sample_packed(src, sw, sh, u0, v0), hh = sample_packed(src, sw, sh, up1, v0);
    const B3 i = sample_packed(src, sw, sh, umh, vph), j = sample_packed(src, sw, sh, uph, vph);
    const B3 k = sample_packed(src, sw, sh, um1, vp1), l = sample_packed(src, sw, sh, u0, vp1), m = sample_packed(src, sw, sh, up1, vp1);
    B3 result = mul(g, 0.125f);
    result = add(result, mul(add(add(add(a, c), k), m), 0.03125f));
    result = add(result, mul(add(add(add(b, f), hh), l), 0.0625f));
    result = add(result, mul(add(add(add(d, e), i), j), 0.125f));
    return pack(result);
}

// ---- Upsample_PSMain (Bloom.hlsl:90-116): Up[i] (w x h) = sample(Down[i], uv) + tent9(Up[i + 1] (uw x uh), radius * texelSize) ---------
HRT_FN uint32_t up_texel(const uint32_t* upper, int uw, int uh, const uint32_t* down, int w, int h, int px, int py, float radius)
{
    const float tx = 1.0f / (float)w, ty = 1.0f / (float)h;
    const float d = radius;
    const float u = pixel_u(px, w), v = pixel_u(py, h);
    const float um = u + -d * tx, u0 = u + 0.0f * tx, up = u + d * tx;
    const float vm = v + -d * ty, v0 = v + 0.0f * ty, vp = v + d * ty;
    const B3 a = sample_packed(upper, uw, uh, um, vm), b = sample_packed(upper, uw, uh, u0, vm), c = sample_packed(upper, uw, uh, up, vm);
    const B3 d_ = sample_packed(upper, uw, uh, um, v0), e = sample_packed(upper, uw, uh, u0, v0), f = sample_packed(upper, uw, uh, up, v0);
    const B3 g = sample_packed(upper, uw, uh, um, vp), hh = sample_packed(upper, uw, uh, u0, vp), i = sample_packed(upper, uw, uh, up, vp);
    B3 upsample = mul(e, 0.25f);
    upsample = add(upsample, mul(add(add(add(b, d_), f), hh), 0.125f));
    upsample = add(upsample, mul(add(add(add(a, c), g), i), 0.0625f));
    const B3 bloom = sample_packed(down, w, h, u, v);
    return pack(add(bloom, upsample));
}

// ---- Composite_PSMain + the additive blend state (Bloom.hlsl:123-128, BloomRenderer.cpp:150-171): hdr.rgb += bloom * intensity ----------
HRT_FN B3 composite_texel(const uint32_t* up0, int w, int h, int W, int H, int px, int py, float intensity)
{
    return mul(sample_packed(up0, w, h, pixel_u(px, W), pixel_u(py, H)), intensity);
}

} // namespace bloom
} // namespace hrt

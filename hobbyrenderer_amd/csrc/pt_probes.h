// pt_probes.h -- the arithmetic of the irradiance probe volume (hrpt_probes_*), one __host__ __device__ source shared by the gfx950 kernels
// (pt_probes.hip) and the host executors (pt_probes_host.cpp): ray generation, the blend of traced rays into octahedral irradiance and
// distance atlases, the border rule, and the query. The stage is defined by this project after the published algorithm (Majercik et al.,
// "Dynamic Diffuse Global Illumination with Ray-Traced Irradiance Fields"); DESIGN.md section 26 has the definition in prose with the
// operation order. In the arithmetic of hobbyrt/detmath.h: no FMA contraction, correctly rounded '/' and sqrt, select-form min / max, sums
// and dot products left to right, hrt_* for every transcendental.
//
// Atlases, per probe and contiguous, linear binary32: irradiance [P][8][8] float4 (6 x 6 interior + one-texel border, texel = (M, 1));
// distance [P][16][16] float2 (14 x 14 interior + border, texel = (mean d, mean d^2)).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_image.h"

namespace hrt {
namespace probes {

using namespace img;

constexpr int kIrrInterior = 6, kIrrTile = 8, kDistInterior = 14, kDistTile = 16;
constexpr int kIrrTexels = kIrrInterior * kIrrInterior, kDistTexels = kDistInterior * kDistInterior;     // 36 and 196 blend lanes per probe
constexpr int kIrrFloats = kIrrTile * kIrrTile * 4, kDistFloats = kDistTile * kDistTile * 2;              // 256 and 512 floats per probe
constexpr uint32_t kMaxProbes = 1u << 20, kMaxRays = 1024u;
constexpr float kUntraced = -1.0f;             // the staged distance of a ray that takes no part in a sum (every traced distance is >= 0)
constexpr float kFloatMax = 3.402823466e38f;

HRT_FN bool finite(float x) { return hrt_abs(x) <= kFloatMax; }      // false for a NaN
HRT_FN float sign1(float x) { return x >= 0.0f ? 1.0f : -1.0f; }     // sign(0) = sign(-0) = +1
// v / |v|; the zero vector (and one so short that v.v underflows to 0) stays as it is
HRT_FN T3 unit0(T3 v) { const float len = length3(v); return len > 0.0f ? t3(v.x / len, v.y / len, v.z / len) : v; }

// ---- the volume ------------------------------------------------------------------------------------------------------------------------
HRT_FN uint32_t probe_count(const HrptProbeVolume& v) { return v.counts[0] * v.counts[1] * v.counts[2]; }
HRT_FN bool volume_valid(const HrptProbeVolume& v)
{
    uint64_t P = 1;
    for (int i = 0; i < 3; ++i) {
        if (v.counts[i] < 1u || v.counts[i] > kMaxProbes) return false;
        P *= v.counts[i];
        if (P > kMaxProbes) return false;
        if (!finite(v.origin[i]) || !finite(v.spacing[i]) || !(v.spacing[i] > 0.0f)) return false;
    }
    return v.raysPerProbe >= 1u && v.raysPerProbe <= kMaxRays && finite(v.maxRayDistance) && v.maxRayDistance > 0.0f &&
           v.hysteresis >= 0.0f && v.hysteresis < 1.0f && finite(v.distanceExponent) && v.distanceExponent >= 1.0f &&
           finite(v.normalBias) && v.normalBias >= 0.0f && finite(v.viewBias) && v.viewBias >= 0.0f && v.pad == 0u;
}
// position of probe (x, y, z): origin + (x, y, z) * spacing
HRT_FN T3 probe_position(const HrptProbeVolume& v, uint32_t x, uint32_t y, uint32_t z)
{
    return t3(v.origin[0] + (float)x * v.spacing[0], v.origin[1] + (float)y * v.spacing[1], v.origin[2] + (float)z * v.spacing[2]);
}
HRT_FN T3 probe_position(const HrptProbeVolume& v, uint32_t p)
{
    const uint32_t x = p % v.counts[0], yz = p / v.counts[0];
    return probe_position(v, x, yz % v.counts[1], yz / v.counts[1]);
}

// ---- octahedral mapping ----------------------------------------------------------------------------------------------------------------
// direction of the octahedral coordinate (ox, oy) in [-1, 1]^2, normalised
HRT_FN T3 oct_decode(float ox, float oy)
{
    const float ax = hrt_abs(ox), ay = hrt_abs(oy);
    const float z = (1.0f - ax) - ay;
    float x = ox, y = oy;
    if (z < 0.0f) { x = (1.0f - ay) * sign1(ox); y = (1.0f - ax) * sign1(oy); }
    return normalize(t3(x, y, z));
}
// octahedral coordinate of the unit direction d
HRT_FN T2 oct_encode(T3 d)
{
    const float s = (hrt_abs(d.x) + hrt_abs(d.y)) + hrt_abs(d.z);
    const float px = d.x / s, py = d.y / s;
    if (d.z < 0.0f) return t2((1.0f - hrt_abs(py)) * sign1(px), (1.0f - hrt_abs(px)) * sign1(py));
    return t2(px, py);
}
// direction of interior texel (i, j) of a tile with an I x I interior
HRT_FN T3 texel_direction(int i, int j, int I)
{
    return oct_decode((((float)i + 0.5f) / (float)I) * 2.0f - 1.0f, (((float)j + 0.5f) / (float)I) * 2.0f - 1.0f);
}
// the interior texel a border texel (x, y) of a T-wide tile copies; an interior texel is its own source
HRT_FN void border_source(int x, int y, int T, int* sx, int* sy)
{
    const bool ex = x == 0 || x == T - 1, ey = y == 0 || y == T - 1;
    *sx = x; *sy = y;
    if (ex && ey) { *sx = x == 0 ? T - 2 : 1; *sy = y == 0 ? T - 2 : 1; }
    else if (ey) { *sx = T - 1 - x; *sy = y == 0 ? 1 : T - 2; }
    else if (ex) { *sy = T - 1 - y; *sx = x == 0 ? 1 : T - 2; }
}

// The four taps of a lookup for the unit direction d in a tile with an I x I interior: texels (x0, y0) .. (x0 + 1, y0 + 1) of the
// (I + 2)-wide tile and the fractional weights. For a unit d both taps of an axis lie in [0, I + 1]; the clamp only keeps a direction that
// is no unit vector (a zero normal: 0 / 0) from indexing outside the tile.
struct Taps { int x0, y0; float fx, fy; };
HRT_FN Taps lookup_taps(T3 d, int I)
{
    const T2 uv = oct_encode(d);
    const float cx = (uv.x * 0.5f + 0.5f) * (float)I + 0.5f, cy = (uv.y * 0.5f + 0.5f) * (float)I + 0.5f;
    const float bx = hrt_floor(cx), by = hrt_floor(cy);
    Taps t;
    t.x0 = (int)hrt_clamp(bx, 0.0f, (float)I); t.y0 = (int)hrt_clamp(by, 0.0f, (float)I);
    t.fx = cx - bx; t.fy = cy - by;
    return t;
}
HRT_FN float bilinear(float a, float b, float c, float d, float fx, float fy)
{
    const float wx = 1.0f - fx, wy = 1.0f - fy;
    return (a * wx + b * fx) * wy + (c * wx + d * fx) * fy;
}
// rgb of the irradiance tile (8 x 8 float4) at d
HRT_FN T3 lookup_irradiance(const float* tile, T3 d)
{
    const Taps t = lookup_taps(d, kIrrInterior);
    const float* a = tile + (t.y0 * kIrrTile + t.x0) * 4;
    const float* c = a + kIrrTile * 4;
    return t3(bilinear(a[0], a[4], c[0], c[4], t.fx, t.fy), bilinear(a[1], a[5], c[1], c[5], t.fx, t.fy), bilinear(a[2], a[6], c[2], c[6], t.fx, t.fy));
}
// (mean d, mean d^2) of the distance tile (16 x 16 float2) at d
HRT_FN T2 lookup_distance(const float* tile, T3 d)
{
    const Taps t = lookup_taps(d, kDistInterior);
    const float* a = tile + (t.y0 * kDistTile + t.x0) * 2;
    const float* c = a + kDistTile * 2;
    return t2(bilinear(a[0], a[2], c[0], c[2], t.fx, t.fy), bilinear(a[1], a[3], c[1], c[3], t.fx, t.fy));
}

// ---- rays of an update -------------------------------------------------------------------------------------------------------------------
struct Rotation { float m[9]; };      // row-major
HRT_FN Rotation frame_rotation(uint32_t frameSeed)
{
    uint32_t s = hrt_pcg_hash(frameSeed ^ 0x9E3779B9u);
    const float u1 = hrt_rng_next(&s), u2 = hrt_rng_next(&s), u3 = hrt_rng_next(&s);
    const float a = hrt_sqrt(1.0f - u1), b = hrt_sqrt(u1);
    float s2, c2, s3, c3;
    hrt_sincos((2.0f * HRT_PI) * u2, &s2, &c2);
    hrt_sincos((2.0f * HRT_PI) * u3, &s3, &c3);
    const float x = a * s2, y = a * c2, z = b * s3, w = b * c3;
    Rotation R;
    R.m[0] = 1.0f - 2.0f * (y * y + z * z); R.m[1] = 2.0f * (x * y - w * z);        R.m[2] = 2.0f * (x * z + w * y);
    R.m[3] = 2.0f * (x * y + w * z);        R.m[4] = 1.0f - 2.0f * (x * x + z * z); R.m[5] = 2.0f * (y * z - w * x);
    R.m[6] = 2.0f * (x * z - w * y);        R.m[7] = 2.0f * (y * z + w * x);        R.m[8] = 1.0f - 2.0f * (x * x + y * y);
    return R;
}
// direction k of N: the spherical Fibonacci point, rotated, normalised
HRT_FN T3 ray_direction(const Rotation& R, uint32_t k, uint32_t N)
{
    const float z = 1.0f - (float)(2u * k + 1u) / (float)N;
    const float r = hrt_sqrt(hrt_max(0.0f, 1.0f - z * z));
    const float t = (float)k * 0.61803398875f;
    const float phi = (2.0f * HRT_PI) * (t - hrt_floor(t));
    float sn, cs;
    hrt_sincos(phi, &sn, &cs);
    const T3 f = t3(r * cs, r * sn, z);
    const T3 v = t3((R.m[0] * f.x + R.m[1] * f.y) + R.m[2] * f.z, (R.m[3] * f.x + R.m[4] * f.y) + R.m[5] * f.z, (R.m[6] * f.x + R.m[7] * f.y) + R.m[8] * f.z);
    const float len = hrt_sqrt(dot3(v, v));
    return t3(v.x / len, v.y / len, v.z / len);
}
HRT_FN uint32_t ray_rng(uint32_t g, uint32_t frameSeed) { return hrt_pcg_hash(g + hrt_pcg_hash(frameSeed)); }
constexpr float kRayTmax = 1e10f;

// ---- blend -----------------------------------------------------------------------------------------------------------------------------
// distance of a traced ray
HRT_FN float ray_distance(uint32_t hit, float t, float maxRayDistance) { return hit ? hrt_min(t, maxRayDistance) : maxRayDistance; }
// what a probe's ray contributes, as the blend reads it: (L.rgb, d), d = kUntraced for a ray with radiance4.w == 0
HRT_FN T4 staged_ray(const float* radiance4, uint32_t hit, float t, float maxRayDistance)
{
    return t4(radiance4[0], radiance4[1], radiance4[2], radiance4[3] == 0.0f ? kUntraced : ray_distance(hit, t, maxRayDistance));
}
// Running sums of one texel over rays in order; terms with w <= 0 and untraced rays are not added.
struct IrrSums { float r, g, b, w; };
struct DistSums { float d, d2, w; };
HRT_FN void irr_add(IrrSums* s, T3 n, const float* dir4, const float* ld4)
{
    const float w = hrt_max(0.0f, (n.x * dir4[0] + n.y * dir4[1]) + n.z * dir4[2]);
    if (ld4[3] < 0.0f || !(w > 0.0f)) return;
    s->r = s->r + w * ld4[0]; s->g = s->g + w * ld4[1]; s->b = s->b + w * ld4[2]; s->w = s->w + w;
}
HRT_FN void dist_add(DistSums* s, T3 n, const float* dir4, const float* ld4, float exponent)
{
    const float d = ld4[3];
    if (d < 0.0f) return;
    const float w = hrt_pow(hrt_max(0.0f, (n.x * dir4[0] + n.y * dir4[1]) + n.z * dir4[2]), exponent);
    if (!(w > 0.0f)) return;
    s->d = s->d + w * d; s->d2 = s->d2 + w * (d * d); s->w = s->w + w;
}
// new value against the old one: the first update stores it, later ones store new + hysteresis * (old - new)
HRT_FN float history(float fresh, float old, float hysteresis, bool hasHistory) { return hasHistory ? fresh + hysteresis * (old - fresh) : fresh; }
HRT_FN T4 irr_texel(const IrrSums& s, T4 old, float hysteresis, bool hasHistory)
{
    if (s.w == 0.0f) return old;
    return t4(history(s.r / s.w, old.x, hysteresis, hasHistory), history(s.g / s.w, old.y, hysteresis, hasHistory), history(s.b / s.w, old.z, hysteresis, hasHistory), 1.0f);
}
HRT_FN T2 dist_texel(const DistSums& s, T2 old, float hysteresis, bool hasHistory)
{
    if (s.w == 0.0f) return old;
    return t2(history(s.d / s.w, old.x, hysteresis, hasHistory), history(s.d2 / s.w, old.y, hysteresis, hasHistory));
}

// ---- query -----------------------------------------------------------------------------------------------------------------------------
// (pi * sum / sumW, inside) at point X with unit normal Nrm and unit direction to the viewer V; atlases as laid out above.
HRT_FN T4 query(const HrptProbeVolume& vol, const float* irradiance, const float* distance, T3 X, T3 Nrm, T3 V)
{
    if (!(finite(X.x) && finite(X.y) && finite(X.z) && finite(Nrm.x) && finite(Nrm.y) && finite(Nrm.z) && finite(V.x) && finite(V.y) && finite(V.z)))
        return t4(0.0f, 0.0f, 0.0f, 0.0f);
    const float xb[3] = { (X.x + Nrm.x * vol.normalBias) + V.x * vol.viewBias, (X.y + Nrm.y * vol.normalBias) + V.y * vol.viewBias,
                          (X.z + Nrm.z * vol.normalBias) + V.z * vol.viewBias };
    float alpha[3]; int base[3]; bool inside = true;
    for (int i = 0; i < 3; ++i) {
        const float rel = (xb[i] - vol.origin[i]) / vol.spacing[i];
        const float b = hrt_clamp(hrt_floor(rel), 0.0f, (float)(vol.counts[i] >= 2u ? vol.counts[i] - 2u : 0u));
        base[i] = (int)b;
        alpha[i] = hrt_saturate(rel - b);
        inside = inside && rel >= 0.0f && rel <= (float)(vol.counts[i] - 1u);
    }
    const T3 Xb = t3(xb[0], xb[1], xb[2]);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    for (int k = 0; k < 8; ++k) {
        const int off[3] = { k & 1, (k >> 1) & 1, (k >> 2) & 1 };
        uint32_t c[3];
        for (int i = 0; i < 3; ++i) { const uint32_t ci = (uint32_t)(base[i] + off[i]); c[i] = ci < vol.counts[i] - 1u ? ci : vol.counts[i] - 1u; }
        const float tri = ((off[0] ? alpha[0] : 1.0f - alpha[0]) * (off[1] ? alpha[1] : 1.0f - alpha[1])) * (off[2] ? alpha[2] : 1.0f - alpha[2]);
        const T3 pos = probe_position(vol, c[0], c[1], c[2]);
        const size_t p = (size_t)c[0] + (size_t)vol.counts[0] * ((size_t)c[1] + (size_t)vol.counts[1] * (size_t)c[2]);
        const float wrap = (dot3(unit0(sub(pos, X)), Nrm) + 1.0f) * 0.5f;
        float w = wrap * wrap + 0.2f;
        const T3 bv = sub(Xb, pos);
        const float dl = length3(bv);
        if (dl > 0.0f) {
            const T2 m = lookup_distance(distance + p * kDistFloats, t3(bv.x / dl, bv.y / dl, bv.z / dl));
            if (dl > m.x) {
                const float var = hrt_abs(m.x * m.x - m.y), diff = dl - m.x;
                const float ch = var / (var + diff * diff);
                w = w * hrt_max((ch * ch) * ch, 0.05f);
            }
        }
        w = hrt_max(1e-6f, w);
        if (w < 0.2f) w = w * ((w * w) / 0.04f);
        w = w * tri;
        const T3 e = lookup_irradiance(irradiance + p * kIrrFloats, Nrm);
        sr = sr + w * e.x; sg = sg + w * e.y; sb = sb + w * e.z; sw = sw + w;
    }
    if (sw == 0.0f) return t4(0.0f, 0.0f, 0.0f, 0.0f);
    return t4(HRT_PI * (sr / sw), HRT_PI * (sg / sw), HRT_PI * (sb / sw), inside ? 1.0f : 0.0f);
}

// hrpt_probes_shade_gbuffer: the query at the first hit of pixel (px, py), scaled; (0, 0, 0, 0) at a miss
HRT_FN T4 shade_pixel(const HrptProbeVolume& vol, const ViewArgs& view, float intensity, const float* irradiance, const float* distance,
                      const float* normal, const float* depth, int px, int py)
{
    const T4 D = load4(depth, view.w, px, py);
    if (D.x == kMissDepth) return t4(0.0f, 0.0f, 0.0f, 0.0f);
    const T4 N4 = load4(normal, view.w, px, py);
    const T3 worldPos = recon(view, bloom::pixel_u(px, view.w), bloom::pixel_u(py, view.h), D.y);
    const T3 V = normalize(sub(t3(view.cam[0], view.cam[1], view.cam[2]), worldPos));
    const T4 q = query(vol, irradiance, distance, worldPos, t3(N4.x, N4.y, N4.z), V);
    return t4(q.x * intensity, q.y * intensity, q.z * intensity, 1.0f);
}

} // namespace probes
} // namespace hrt

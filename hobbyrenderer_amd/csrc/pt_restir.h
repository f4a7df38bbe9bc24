// pt_restir.h -- the arithmetic of hrpt_restir_lighting, one __host__ __device__ source shared by the gfx950 kernels (pt_restir.hip) and the
// host executors (pt_restir_host.cpp): resampled direct light (ReSTIR DI after Bitterli et al. 2020) over the path tracer's first-hit planes.
// DESIGN.md section 30 has the definition in prose. The stage CALLS deferred lighting's functions (pt_deferred.h: frame_ray, make_surface,
// light_direction, light_radiance, light_color, ray_rows, finish_hit), the lighting functions under them and pt_denoise.h's luminance; what
// is stated here is the reservoir, its update, the three RNG states and the four passes.
//
// As in pt_deferred.h the atmosphere and the shadow query do not live here: a pass takes `sun(l, X, x, y)` (radiance of the directional
// light l at the surface point X of pixel (x, y)) and `sky(x, y, o, d)` as callables and the visibilities as an array of floats with a
// stride, so the kernels compute the former from the scene's tables and read the latter from the hit records of hrpt_trace_rays, while the
// host executors read both from images. Texels and records go through `io` (ld / st of one 16-byte row), so that the kernels' accesses are
// 16-byte ones.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_deferred.h"
#include "pt_denoise.h"

namespace hrt {
namespace restir {

using img::T4;
using img::t4;
using deferred::xyz;

constexpr uint32_t kFlags = HRPT_RESTIR_SHADOWS | HRPT_RESTIR_SKY | HRPT_RESTIR_TEMPORAL | HRPT_RESTIR_SPATIAL | HRPT_RESTIR_INITIAL_VISIBILITY | HRPT_RESTIR_RESET;
constexpr uint32_t kEmpty = HRPT_RESTIR_EMPTY;
constexpr float kTwoPi = 6.2831853f;

// What the passes read of an HrptPathTracerConstants and an HrptRestirParams, gathered once per call.
struct Args {
    deferred::Frame d;          // the primary ray, the sun and finish_hit's flags (no indirect term)
    uint32_t flags, seedHash;   // HRPT_RESTIR_*, hrt_pcg_hash(frameSeed)
    uint32_t n;                 // m_LightCount
    uint32_t candidates, spatialSamples;
    float spatialRadius, maxHistory, depthThreshold, normalThreshold;
};
HRT_FN Args make_args(const HrptPathTracerConstants& cb, const HrptRestirParams& p, float sunIntensity, int w, int h)
{
    const HrptDeferredParams dp = { (p.flags & HRPT_RESTIR_SKY) ? HRPT_DEFERRED_SKY : 0u, 0.0f, { 0u, 0u } };
    Args a;
    a.d = deferred::make_frame(cb, dp, sunIntensity, w, h);
    a.flags = p.flags; a.seedHash = hrt_pcg_hash(p.frameSeed); a.n = cb.m_LightCount;
    a.candidates = p.candidates; a.spatialSamples = p.spatialSamples;
    a.spatialRadius = p.spatialRadius; a.maxHistory = p.maxHistory; a.depthThreshold = p.depthThreshold; a.normalThreshold = p.normalThreshold;
    return a;
}
HRT_FN bool finite(float x) { return (x - x) == 0.0f; }
HRT_FN bool params_valid(const HrptRestirParams& p)
{
    return (p.flags & ~kFlags) == 0u && (p.reserved[0] | p.reserved[1] | p.reserved[2] | p.reserved[3]) == 0u && p.candidates >= 1u && p.candidates <= 32u &&
           p.spatialSamples <= 8u && finite(p.spatialRadius) && p.spatialRadius > 0.0f && p.spatialRadius <= 65535.0f && finite(p.maxHistory) && p.maxHistory > 0.0f &&
           finite(p.depthThreshold) && finite(p.normalThreshold);
}

// ---- RNG states: each derived from the initial value, never from an advanced state ----------------------------------------------------
HRT_FN uint32_t state_a(const Args& a, int px, int py) { return hrt_pcg_hash((uint32_t)py * (uint32_t)a.d.w + (uint32_t)px + a.seedHash); }
HRT_FN uint32_t state_b(const Args& a, int px, int py) { return hrt_pcg_hash(state_a(a, px, py)); }
HRT_FN uint32_t state_c(const Args& a, int px, int py) { return hrt_pcg_hash(state_b(a, px, py)); }

// ---- the reservoir ---------------------------------------------------------------------------------------------------------------------
// The stored record is an HrptRestirReservoir { light, W, M, pHat }, moved as one 16-byte row; the running one carries wSum in W's place.
struct Res { uint32_t light; float wSum, M, pHat; };
HRT_FN Res empty() { Res r; r.light = kEmpty; r.wSum = 0.0f; r.M = 0.0f; r.pHat = 0.0f; return r; }
// `<=`, not `<`: hrt_rng_next can return exactly 1.0f, and the first candidate (w == wSum) must still be taken.
HRT_FN void add(Res& r, uint32_t light, float w, float m, float pHatNew, float u)
{
    r.wSum = r.wSum + w; r.M = r.M + m;
    if (w > 0.0f && u * r.wSum <= w) { r.light = light; r.pHat = pHatNew; }
}
// W = (wSum / norm) / pHat; norm is M (initial, temporal) or the number of combined records (spatial).
HRT_FN HrptRestirReservoir finish(const Res& r, float norm)
{
    HrptRestirReservoir o;
    o.light = r.light; o.M = r.M; o.pHat = r.pHat;
    o.W = r.pHat > 0.0f ? (r.wSum / norm) / r.pHat : 0.0f;
    return o;
}
HRT_FN HrptRestirReservoir stored_empty() { HrptRestirReservoir o; o.light = kEmpty; o.W = 0.0f; o.M = 0.0f; o.pHat = 0.0f; return o; }
HRT_FN T4 as_row(const HrptRestirReservoir& r) { return t4(hrt_u2f(r.light), r.W, r.M, r.pHat); }
HRT_FN HrptRestirReservoir from_row(T4 v) { HrptRestirReservoir r; r.light = hrt_f2u(v.x); r.W = v.y; r.M = v.z; r.pHat = v.w; return r; }
template <class IO> HRT_FN HrptRestirReservoir load_res(IO io, const HrptRestirReservoir* plane, size_t idx) { return from_row(io.ld(reinterpret_cast<const float*>(plane), idx)); }
template <class IO> HRT_FN void store_res(IO io, HrptRestirReservoir* plane, size_t idx, const HrptRestirReservoir& r) { io.st(reinterpret_cast<float*>(plane), idx, as_row(r)); }

// ---- the surface of a pixel: steps 1 and 3 of deferred lighting -------------------------------------------------------------------------
struct Surface { Lighting s; f3 X; T4 N4, D; };
template <class IO> HRT_FN bool surface_at(const Args& a, const HrptRestirImages& im, IO io, int px, int py, Surface& S)
{
    const size_t idx = (size_t)py * (size_t)a.d.w + (size_t)px;
    S.D = io.ld(im.depth, idx);
    S.N4 = io.ld(im.normal, idx);
    if (S.D.x == img::kMissDepth) return false;
    f3 o, d;
    deferred::frame_ray(a.d, px, py, o, d);
    S.X = o + d * S.D.x;
    S.s = deferred::make_surface(io.ld(im.albedo, idx), S.N4, io.ld(im.geoNormal, idx).w, d);
    return true;
}

// ---- the target pHat(S, i) with the terms the shade pass needs -------------------------------------------------------------------------
// 0 when i names no light or the pair is unlit; else luminance(dif + spec) of the unshadowed light through p > 0 ? p : 0 (a NaN counts as 0).
struct Lit { f3 dif, spec, L; float maxDist; bool lit; };
template <class SUN> HRT_FN float target(const Args& a, const Surface& S, const HrptGPULight* lights, uint32_t i, SUN sun, int px, int py, Lit& e)
{
    e.dif = mk3(0.0f, 0.0f, 0.0f); e.spec = e.dif; e.L = e.dif; e.maxDist = 0.0f; e.lit = false;
    if (!(i < a.n)) return 0.0f;
    const HrptGPULight& l = lights[i];
    if (!deferred::light_direction(l, S.s.N, S.X, mk3(a.d.sun), e.L, e.maxDist)) return 0.0f;
    e.lit = true;
    const f3 radiance = l.m_Type == HRPT_LIGHT_DIRECTIONAL ? sun(l, S.X, px, py) : deferred::light_radiance(l, S.X);
    Lighting in = S.s;
    in.L = e.L;
    prepare_byproducts(in);
    evaluate_direct_unshadowed(in, radiance, e.dif, e.spec);
    const f3 c = e.dif + e.spec;
    const float p = denoise::luminance(img::t3(c.x, c.y, c.z));
    return p > 0.0f ? p : 0.0f;
}
// The shadow-ray record of reservoir r at S: the chosen light's direction again; an empty reservoir or a miss gives the NaN-origin record.
template <class IO> HRT_FN void store_ray(const Args& a, IO io, bool hit, const Surface& S, const HrptGPULight* lights, const HrptRestirReservoir& r, HrptRay* rays, size_t idx)
{
    f3 L = mk3(0.0f, 0.0f, 0.0f), X = L;
    float maxDist = 0.0f;
    bool lit = false;
    if (hit && r.light < a.n) { X = S.X; lit = deferred::light_direction(lights[r.light], S.s.N, S.X, mk3(a.d.sun), L, maxDist); }
    T4 rows[3];
    deferred::ray_rows(lit, X, L, maxDist, rows);
    float* rec = reinterpret_cast<float*>(rays);
    io.st(rec, idx * 3, rows[0]); io.st(rec, idx * 3 + 1, rows[1]); io.st(rec, idx * 3 + 2, rows[2]);
}

// ---- pass A, initial: `candidates` uniform draws of a light, resampled by the target ------------------------------------------------------
template <class IO, class SUN>
HRT_FN void initial_pixel(const Args& a, const HrptRestirImages& im, const HrptGPULight* lights, IO io, SUN sun, int px, int py, HrptRay* raysOut)
{
    const size_t idx = (size_t)py * (size_t)a.d.w + (size_t)px;
    Surface S;
    const bool hit = surface_at(a, im, io, px, py, S);
    HrptRestirReservoir out = stored_empty();
    if (hit && a.n > 0u) {
        Res r = empty();
        uint32_t s = state_a(a, px, py);
        for (uint32_t c = 0; c < a.candidates; ++c) {
            const float u0 = hrt_rng_next(&s), u1 = hrt_rng_next(&s);
            uint32_t i = (uint32_t)(u0 * (float)a.n);
            if (i > a.n - 1u) i = a.n - 1u;
            Lit e;
            const float p = target(a, S, lights, i, sun, px, py, e);
            add(r, i, p * (float)a.n, 1.0f, p, u1);
        }
        out = finish(r, r.M);
    }
    store_res(io, im.reservoirOut, idx, out);
    if (raysOut) store_ray(a, io, hit, S, lights, out, raysOut, idx);
}

// ---- pass B, temporal: the previous call's record at the reprojected pixel ----------------------------------------------------------------
// vis: the initial sample's visibility, vis[idx * visStride] (null = 1). history: reservoirIn / keyIn are read (the caller passes false
// without HRPT_RESTIR_TEMPORAL, without a history and with HRPT_RESTIR_RESET).
template <class IO, class SUN>
HRT_FN void temporal_pixel(const Args& a, const HrptRestirImages& im, const HrptGPULight* lights, IO io, SUN sun, int px, int py, const HrptRestirReservoir* initial,
                           const float* vis, size_t visStride, bool history)
{
    const size_t idx = (size_t)py * (size_t)a.d.w + (size_t)px;
    Surface S;
    HrptRestirReservoir out = stored_empty();
    if (surface_at(a, im, io, px, py, S)) {
        HrptRestirReservoir cur = load_res(io, initial, idx);
        if (vis && vis[idx * visStride] == 0.0f) cur.W = 0.0f;
        uint32_t s = state_b(a, px, py);
        const float u0 = hrt_rng_next(&s), u1 = hrt_rng_next(&s);
        Res t = empty();
        add(t, cur.light, (cur.pHat * cur.W) * cur.M, cur.M, cur.pHat, u0);
        if (history) {
            const T4 m = io.ld(im.motion, idx);
            const float qx = hrt_floor(((float)px + 0.5f) + m.x), qy = hrt_floor(((float)py + 0.5f) + m.y);
            if (m.w == 1.0f && qx >= 0.0f && qy >= 0.0f && qx < (float)a.d.w && qy < (float)a.d.h) {
                const size_t q = (size_t)(int)qy * (size_t)a.d.w + (size_t)(int)qx;
                const HrptRestirReservoir prev = load_res(io, im.reservoirIn, q);
                const T4 key = io.ld(im.keyIn, q);
                const float e = S.D.y + m.z;
                if (prev.light < a.n && dot(S.s.N, xyz(key)) >= a.normalThreshold && hrt_abs(key.w - e) <= a.depthThreshold * e) {
                    const float Mp = hrt_min(prev.M, a.maxHistory * cur.M);
                    Lit ev;
                    const float pp = target(a, S, lights, prev.light, sun, px, py, ev);
                    add(t, prev.light, (pp * prev.W) * Mp, Mp, pp, u1);
                }
            }
        }
        out = finish(t, t.M);
    }
    store_res(io, im.reservoirOut, idx, out);
}

// ---- pass C, spatial: neighbours of the temporal pass's reservoirs T, pairwise MIS -----------------------------------------------------------
// Three draws per neighbour (radius, angle, selection) and one for the own record. Two target evaluations per accepted neighbour; nothing
// per neighbour is kept. Writes the final reservoir, the key (N.xyz, view depth) and, when raysOut is not null, the chosen light's shadow ray.
template <class IO, class SUN>
HRT_FN void spatial_pixel(const Args& a, const HrptRestirImages& im, const HrptGPULight* lights, IO io, SUN sun, int px, int py, const HrptRestirReservoir* T, HrptRay* raysOut)
{
    const size_t idx = (size_t)py * (size_t)a.d.w + (size_t)px;
    Surface S;
    const bool hit = surface_at(a, im, io, px, py, S);
    HrptRestirReservoir out = stored_empty();
    if (hit) {
        const HrptRestirReservoir c = load_res(io, T, idx);
        const f3 N = S.s.N;
        const float vd = S.D.y;
        Res s = empty();
        float Sc = 0.0f;
        uint32_t accepted = 0u;
        uint32_t rng = state_c(a, px, py);
        const uint32_t k = (a.flags & HRPT_RESTIR_SPATIAL) ? a.spatialSamples : 0u;
        for (uint32_t j = 0; j < k; ++j) {
            const float ua = hrt_rng_next(&rng), ub = hrt_rng_next(&rng), us = hrt_rng_next(&rng);
            const float r = a.spatialRadius * hrt_sqrt(ua), th = kTwoPi * ub;
            const int qx = px + (int)hrt_floor(r * hrt_cos(th) + 0.5f), qy = py + (int)hrt_floor(r * hrt_sin(th) + 0.5f);
            if (qx < 0 || qy < 0 || qx >= a.d.w || qy >= a.d.h || (qx == px && qy == py)) continue;
            Surface Q;
            if (!surface_at(a, im, io, qx, qy, Q)) continue;
            if (dot(N, Q.s.N) < a.normalThreshold || hrt_abs(Q.D.y - vd) > a.depthThreshold * vd) continue;
            const HrptRestirReservoir nb = load_res(io, T, (size_t)qy * (size_t)a.d.w + (size_t)qx);
            Lit ev;
            const float ta = target(a, S, lights, nb.light, sun, px, py, ev);
            const float tb = target(a, Q, lights, c.light, sun, qx, qy, ev);
            const float ni = nb.M * nb.pHat, nc = c.M * c.pHat;
            const float mi = ni == 0.0f ? 0.0f : ni / (ni + c.M * ta);
            const float mc = nc == 0.0f ? 0.0f : nc / (nc + nb.M * tb);
            add(s, nb.light, (ta * nb.W) * mi, nb.M, ta, us);
            Sc = Sc + mc;
            ++accepted;
        }
        const float uo = hrt_rng_next(&rng);
        if (accepted == 0u) { Sc = 1.0f; accepted = 1u; }
        add(s, c.light, (c.pHat * c.W) * Sc, c.M, c.pHat, uo);
        out = finish(s, (float)accepted);
    }
    store_res(io, im.reservoirOut, idx, out);
    io.st(im.keyOut, idx, t4(S.N4.x, S.N4.y, S.N4.z, S.D.y));
    if (raysOut) store_ray(a, io, hit, S, lights, out, raysOut, idx);
}

// ---- pass D, shade: the chosen light times W times its visibility, finished as deferred lighting finishes a hit ----------------------------
template <class IO, class SUN, class SKY>
HRT_FN void shade_pixel(const Args& a, const HrptRestirImages& im, const HrptGPULight* lights, IO io, SUN sun, SKY sky, int px, int py, const HrptRestirReservoir* fin,
                        const float* vis, size_t visStride)
{
    const size_t idx = (size_t)py * (size_t)a.d.w + (size_t)px;
    Surface S;
    if (!surface_at(a, im, io, px, py, S)) { io.st(im.colorOut, idx, sky(px, py)); return; }
    const HrptRestirReservoir r = load_res(io, fin, idx);
    f3 totalD = mk3(0.0f, 0.0f, 0.0f), totalS = totalD;
    if (r.light < a.n) {
        Lit e;
        target(a, S, lights, r.light, sun, px, py, e);
        const float k = r.W * (vis ? vis[idx * visStride] : 1.0f);
        totalD = e.dif * k; totalS = e.spec * k;
    }
    io.st(im.colorOut, idx, deferred::finish_hit(a.d, io.ld(im.albedo, idx), io.ld(im.emissive, idx), io.ld(im.geoNormal, idx).w, totalD, totalS, t4(0.0f, 0.0f, 0.0f, 0.0f)));
}

} // namespace restir
} // namespace hrt

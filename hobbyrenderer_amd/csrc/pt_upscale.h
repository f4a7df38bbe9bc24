// pt_upscale.h -- the arithmetic of hrpt_upscale, one __host__ __device__ source shared by the gfx950 kernel (pt_upscale.hip) and
// hrpt_upscale_host (pt_upscale_host.cpp): temporal upscaling of a jittered render-size frame (w x h) into a display-size history (W x H).
// The stage sits where the reference schedules its TAARenderer (src/Renderer.cpp:1296,1311), whose body is a closed FSR3 call
// (src/TAARenderer.cpp:226-252): there is nothing of it to restate, so the stage is DEFINED here, as skinning was, and parity with FSR is
// out of scope. DESIGN.md section 24 has the definition in prose. It is built on pt_image.h and temporal::catmull_rom of pt_temporal.h, in the
// arithmetic of hobbyrt/detmath.h: no FMA contraction, correctly rounded '/', select-form min / max / clamp, sums left to right, hrt_exp.
//
// Images are row-major float4. At render size: `color` (rgb radiance, a), `depth` (HRPT_GB_DEPTH: miss when .x == kMissDepth, view depth in
// .y), `motion` (the plane of hrpt_render_motion_vectors: .xy in render pixels, this -> last frame). At display size: `historyIn` or null,
// `historyOut` (rgb, a = accumulated sample weight n), `colorOut` (rgb, a = alpha of the nearest render texel).
//
// Per display pixel (X, Y), with rx = (float)w / (float)W, sx = (float)W / (float)w (ry, sy likewise) and (jx, jy) the frame's sample offset
// in render pixels:
//   p  = (((float)X + 0.5f) * rx, ((float)Y + 0.5f) * ry)                    the pixel in render pixels
//   bi = (int)clamp(floor(p.x - jx), 0, w - 1), bj likewise                  the base texel
//   nine taps dj = -1..1, di = -1..1 in row-major order; tap texel ti = clamp(bi + di, 0, w - 1), tj likewise
//     q = (((float)ti + 0.5f) + jx, ((float)tj + 0.5f) + jy)                 where the tap's sample lies
//     d = ((q.x - p.x) * sx, (q.y - p.y) * sy)                               its offset in DISPLAY pixels
//     g = hrt_exp(-hrt_min(kernel * (d.x * d.x + d.y * d.y), 80.0f))         > 0 for every accepted parameter
//   lo / hi = per-channel min / max of the taps' rgb (from +inf / -inf; with HRPT_UPSCALE_NO_CLAMP they are -inf / +inf);
//   cur = clamp(sum(g * rgb) / sum(g), lo, hi) (both sums from 0, in tap order; the clamp takes back the rounding of the quotient);
//   beta = max g (from 0): how well this frame samples this pixel; alphaOut = color(bi, bj).a
//   depth key of a tap = +inf for a miss, depth.y for a hit; the chosen tap is the first with the smallest key below +inf. A hit whose view
//   depth is not below +inf (inf, NaN) counts as a miss here.
//   no tap chosen:  historyOut = (cur, 0), colorOut = (cur, alphaOut)         the temporal stage's miss rule
//   else m = motion of the chosen tap, reproj = ((U + m.x * sizeInv.x) - jitterOffsetUV.x, (V + m.y * sizeInv.y) - jitterOffsetUV.y) with
//     U = bloom::pixel_u(X, W), V likewise, sizeInv the RENDER view's m_ViewportSizeInv, jitterOffsetUV as temporal::make_args forms it
//   no history, or reproj not inside [0, 1]^2 (a NaN is not inside): out = cur exactly, n' = beta
//   else h4 = catmull_rom(historyIn, W, H, reproj, (float)W, (float)H); hc = clamp(h4.rgb, lo, hi) (the identity with HRPT_UPSCALE_NO_CLAMP);
//     n = min(h4.w, maxHistory); t = beta / (n + beta); out = lerp(hc, cur, t); n' = min(n + beta, maxHistory)
//   historyOut = (out, n'), colorOut = (out, alphaOut)
//
// Deliberately left out: sharpening (the reference's m_TAASharpness), tonemapped-space blend weights, a kept previous depth (disocclusion
// is handled by the neighbourhood clamp alone), a reactive mask, multi-GPU tiles (the stage works on whole images: run it after the
// gather), and the C++ plugin mirror.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "pt_image.h"
#include "pt_temporal.h"

namespace hrt {
namespace upscale {

using namespace img;

constexpr float kMaxExponent = 80.0f;         // exp(-80) = 1.8e-35 is a normal number: every tap weight is > 0

// What the pass reads of the sizes, the two HrptPlanarViewConstants and the params, gathered once per call.
struct Args {
    int w, h, W, H;
    float rx, ry, sx, sy;           // (float)w / (float)W, (float)h / (float)H and their counterparts
    float jx, jy;                   // params.jitter
    float sizeInv[2];               // view->m_ViewportSizeInv (render size)
    float jitterOffsetUV[2];        // (prevView->m_PixelOffset - view->m_PixelOffset) * m_ViewportSizeInv
    float kernel, maxHistory;
    uint32_t flags;
};
HRT_FN Args make_args(const HrptPlanarViewConstants& view, const HrptPlanarViewConstants& prev, const HrptUpscaleParams& p, int w, int h, int W, int H)
{
    Args a;
    a.w = w; a.h = h; a.W = W; a.H = H;
    a.rx = (float)w / (float)W; a.ry = (float)h / (float)H; a.sx = (float)W / (float)w; a.sy = (float)H / (float)h;
    a.jx = p.jitter[0]; a.jy = p.jitter[1];
    for (int i = 0; i < 2; ++i) {
        a.sizeInv[i] = view.m_ViewportSizeInv[i];
        a.jitterOffsetUV[i] = (prev.m_PixelOffset[i] - view.m_PixelOffset[i]) * view.m_ViewportSizeInv[i];
    }
    a.kernel = p.kernel; a.maxHistory = p.maxHistory; a.flags = p.flags;
    return a;
}

HRT_FN float inf() { return hrt_u2f(0x7f800000u); }
HRT_FN float depth_key(float depthX, float depthY) { return depthX == kMissDepth ? inf() : depthY; }
HRT_FN int base_texel(float p, float j, int n) { return (int)hrt_clamp(hrt_floor(p - j), 0.0f, (float)(n - 1)); }
HRT_FN int tap_texel(int b, int d, int n) { const int t = b + d; return t < 0 ? 0 : (t > n - 1 ? n - 1 : t); }

// The taps of a pixel straight from the render-size images: colour and depth key of texel (ti, tj). The kernel has a second source with the
// same two functions over its staged window (found through its argument's namespace).
struct ImageTaps { const float* color; const float* depth; int w; };
HRT_FN T4 tap_color(const ImageTaps& s, int ti, int tj) { return load4(s.color, s.w, ti, tj); }
HRT_FN float tap_key(const ImageTaps& s, int ti, int tj)
{
    const float* p = s.depth + ((size_t)tj * (size_t)s.w + (size_t)ti) * 4;
    return depth_key(p[0], p[1]);
}

// ---- display pixel (X, Y) ------------------------------------------------------------------------------------------------------------
template <class Taps>
HRT_FN void pixel(const Args& a, const Taps& taps, const float* motion, const float* historyIn, int X, int Y, T4* historyOut, T4* colorOut)
{
    const float px = ((float)X + 0.5f) * a.rx, py = ((float)Y + 0.5f) * a.ry;
    const int bi = base_texel(px, a.jx, a.w), bj = base_texel(py, a.jy, a.h);

    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, beta = 0.0f, alphaOut = 0.0f;
    // HRPT_UPSCALE_NO_CLAMP enters here, as the bounds' start: from -inf / +inf they stay there, and that clamp leaves every bit of every value
    // catmull_rom can return as it is (it never returns a NaN: its own clamp ends in select-form max / min against 0). The pixel keeps one
    // straight-line path that way; a test of the flag at the clamp cost the kernel 180 VGPRs.
    const float lo0 = (a.flags & HRPT_UPSCALE_NO_CLAMP) != 0u ? -inf() : inf();
    T3 lo = t3(lo0, lo0, lo0), hi = t3(-lo0, -lo0, -lo0);
    float best = inf(); int mi = -1, mj = -1;
    for (int dj = -1; dj <= 1; ++dj) {
        const int tj = tap_texel(bj, dj, a.h);
        const float dy = ((((float)tj + 0.5f) + a.jy) - py) * a.sy;
        for (int di = -1; di <= 1; ++di) {
            const int ti = tap_texel(bi, di, a.w);
            const float dx = ((((float)ti + 0.5f) + a.jx) - px) * a.sx;
            const float g = hrt_exp(-hrt_min(a.kernel * (dx * dx + dy * dy), kMaxExponent));
            const T4 c = tap_color(taps, ti, tj);
            sr = sr + g * c.x; sg = sg + g * c.y; sb = sb + g * c.z; sw = sw + g;
            lo = t3(hrt_min(lo.x, c.x), hrt_min(lo.y, c.y), hrt_min(lo.z, c.z));
            hi = t3(hrt_max(hi.x, c.x), hrt_max(hi.y, c.y), hrt_max(hi.z, c.z));
            beta = hrt_max(beta, g);
            if (di == 0 && dj == 0) alphaOut = c.w;
            const float z = tap_key(taps, ti, tj);
            if (z < best) { best = z; mi = ti; mj = tj; }
        }
    }
    // the quotient of the two rounded sums may leave the taps' range by an ulp or two (where one weight dominates): the clamp brings it back,
    // so that with the clamp on no output leaves [lo, hi] by more than the blend's own rounding
    const T3 cur = t3(hrt_clamp(sr / sw, lo.x, hi.x), hrt_clamp(sg / sw, lo.y, hi.y), hrt_clamp(sb / sw, lo.z, hi.z));
    if (mi < 0) { *historyOut = t4(cur.x, cur.y, cur.z, 0.0f); *colorOut = t4(cur.x, cur.y, cur.z, alphaOut); return; }

    const float* m = motion + ((size_t)mj * (size_t)a.w + (size_t)mi) * 4;
    const float ru = (bloom::pixel_u(X, a.W) + m[0] * a.sizeInv[0]) - a.jitterOffsetUV[0];
    const float rv = (bloom::pixel_u(Y, a.H) + m[1] * a.sizeInv[1]) - a.jitterOffsetUV[1];
    const bool inside = ru >= 0.0f && ru <= 1.0f && rv >= 0.0f && rv <= 1.0f;
    T3 out = cur; float n1 = beta;
    if (historyIn != nullptr && inside) {
        const T4 h4 = temporal::catmull_rom(historyIn, a.W, a.H, ru, rv, (float)a.W, (float)a.H);
        const T3 hc = t3(hrt_clamp(h4.x, lo.x, hi.x), hrt_clamp(h4.y, lo.y, hi.y), hrt_clamp(h4.z, lo.z, hi.z));
        const float n = hrt_min(h4.w, a.maxHistory);
        const float t = beta / (n + beta);
        out = t3(lerp(hc.x, cur.x, t), lerp(hc.y, cur.y, t), lerp(hc.z, cur.z, t));
        n1 = hrt_min(n + beta, a.maxHistory);
    }
    *historyOut = t4(out.x, out.y, out.z, n1);
    *colorOut = t4(out.x, out.y, out.z, alphaOut);
}

} // namespace upscale
} // namespace hrt

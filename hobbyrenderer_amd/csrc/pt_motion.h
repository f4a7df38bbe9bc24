// pt_motion.h -- screen-space motion of the first hit (hrpt_render_motion_vectors): ComputeMotionVectors of the reference
// (src/shaders/CommonLighting.hlsli:242-260) fed as its raster pass feeds it (src/shaders/BasePass.hlsl:53,492): the INTERPOLATED vertex position
// of the hit triangle under the instance's current and previous transform, each through its frame's jittered m_MatWorldToClip. The hit is the one
// hrpt_render_gbuffer commits for the same constants. Both kernels (wf_gbuffer_motion of pt_wf_gbuffer.h, pt_motion_kernel among the
// thread-per-query kernels of pt_megakernel.hip) call motion_gather / motion_texel below; DESIGN.md section 16 has the definition.
#pragma once

#include "pt_gbuffer.h"
#include "pt_motion_records.h"      // MotionInst, MotionArgs

namespace hrt {

// mul(float4(p, 1), M).xyz over rows 0..3 of a 4 x 3 matrix, left to right (bvh_build.cpp transform_point, tl_world_triangle)
HRT_DEV f3 motion_transform_point(f3 p, const float4 w0, const float4 w1, const float4 w2)
{   // {M00 M01 M02 M10} {M11 M12 M20 M21} {M22 Tx Ty Tz}
    return mk3(((p.x * w0.x + p.y * w0.w) + p.z * w1.z) + w2.y,
               ((p.x * w0.y + p.y * w1.x) + p.z * w1.w) + w2.z,
               ((p.x * w0.z + p.y * w1.y) + p.z * w2.x) + w2.w);
}

// The triangle of a committed hit now and one frame ago, in world space.
struct MotionTri { f3 cur0, cur1, cur2, prev0, prev1, prev2; };

// The gather: instance record -> three indices -> three object-space positions (a three-deep dependent chain; callers issue it before their
// texture fetches). The current vertices are those the hit was found on: the GpuTri of the flat structure, tl_world_triangle's product at a
// two-level leaf -- both are transform_point(q, m_World), the statement the previous vertices are formed with, so equal transforms give equal bits.
// The previous vertices come from prevPositions (a deforming mesh: hrpt_update_vertices); with prevPositions == positions both tables hold the
// same values and the arithmetic is the same.
HRT_DEV MotionTri motion_gather(const SceneView& s, const MotionArgs& m, const Hit& hit)
{
    const uint32_t* e = reinterpret_cast<const uint32_t*>(s.attrs + hit.tri) + 16;      // GpuTriAttr e{inst, prim, -, -}
    const uint32_t inst = s.instances ? hit.inst : e[0], prim = e[1];
    const float4* rec = reinterpret_cast<const float4*>(m.inst + inst);
    const float4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
    const uint32_t first = __float_as_uint(rec[3].x) + 3u * prim;
    const uint32_t i0 = m.indices[first], i1 = m.indices[first + 1u], i2 = m.indices[first + 2u];
    const f3 q0 = mk3(m.prevPositions + 3ull * i0), q1 = mk3(m.prevPositions + 3ull * i1), q2 = mk3(m.prevPositions + 3ull * i2);
    MotionTri t;
    if (s.instances) {
        const f3 p0 = mk3(m.positions + 3ull * i0), p1 = mk3(m.positions + 3ull * i1), p2 = mk3(m.positions + 3ull * i2);
        const float4* w = reinterpret_cast<const float4*>(s.instances[inst].world);
        const float4 c0 = w[0], c1 = w[1], c2 = w[2];
        t.cur0 = motion_transform_point(p0, c0, c1, c2); t.cur1 = motion_transform_point(p1, c0, c1, c2); t.cur2 = motion_transform_point(p2, c0, c1, c2);
    } else {
        const GpuTri& g = s.tris[hit.tri];
        t.cur0 = mk3(g.p0); t.cur1 = mk3(g.p1); t.cur2 = mk3(g.p2);
    }
    t.prev0 = motion_transform_point(q0, w0, w1, w2); t.prev1 = motion_transform_point(q1, w0, w1, w2); t.prev2 = motion_transform_point(q2, w0, w1, w2);
    return t;
}

// float4(p, 1) * M, row-vector product summed left to right
HRT_DEV void motion_clip(f3 p, const float* M, float& x, float& y, float& w)
{
    x = ((p.x * M[0] + p.y * M[4]) + p.z * M[8]) + 1.0f * M[12];
    y = ((p.x * M[1] + p.y * M[5]) + p.z * M[9]) + 1.0f * M[13];
    w = ((p.x * M[3] + p.y * M[7]) + p.z * M[11]) + 1.0f * M[15];
}

// ComputeMotionVectors for a hit with barycentrics (u, v): (prevWindow - window, prevClip.w - clip.w, 1); w is the valid flag.
HRT_DEV float4 motion_texel(const HrptPlanarViewConstants& view, const MotionArgs& m, const MotionTri& t, float u, float v)
{
    const float bx = (1.0f - u) - v, by = u, bz = v;                    // the interpolation statement of full_hit_attributes
    const f3 worldPos = (t.cur0 * bx + t.cur1 * by) + t.cur2 * bz;
    const f3 prevWorldPos = (t.prev0 * bx + t.prev1 * by) + t.prev2 * bz;
    float cx, cy, cw, px, py, pw;
    motion_clip(worldPos, view.m_MatWorldToClip, cx, cy, cw);
    motion_clip(prevWorldPos, m.prevWorldToClip, px, py, pw);
    const float wx = (cx / cw) * view.m_ClipToWindowScale[0] + view.m_ClipToWindowBias[0];
    const float wy = (cy / cw) * view.m_ClipToWindowScale[1] + view.m_ClipToWindowBias[1];
    const float pwx = (px / pw) * m.prevScale[0] + m.prevBias[0];
    const float pwy = (py / pw) * m.prevScale[1] + m.prevBias[1];
    return make_float4(pwx - wx, pwy - wy, pw - cw, 1.0f);
}

} // namespace hrt

// pt_skin.h -- the arithmetic of the vertex producer in front of the quantiser (hrpt_skin_vertices_host / _device,
// hrpt_update_vertices_skinned): morph targets, then linear-blend skinning with up to four joints, then unit normal and tangent. One
// __host__ __device__ source shared by the gfx950 kernels (pt_skin.hip) and the host executor (pt_skin_host.cpp); tests/skin_reference.py
// states the same in NumPy, and all three agree bit for bit. The reference renderer has no skinning (its loader drops morph-weight
// channels and never reads `skins`), so this stage is defined here: parity unpinned by the reference. DESIGN.md section 22 has the prose.
//
// float32 throughout, one rounding per operation (no FMA contraction), correctly rounded / and sqrt, evaluation order as written.
// Per vertex i, from the bind-pose record `base`:
//   1. morph   p = base.pos, n = base.normal, t = base.tangent[0..2]; uv and s = base.tangent[3] are copied. For k = 0 .. targetCount - 1 in
//              that order, w = morphWeights[k]: a target with w == 0 (+0 or -0) is skipped entirely (0 * inf never happens, a sparse pose
//              does not read the 36 bytes); otherwise, with d = deltas[k * count + i], per component
//              p[c] = p[c] + w * d.pos[c], n[c] = n[c] + w * d.normal[c], t[c] = t[c] + w * d.tangent[c]      (a product, then a sum)
//   2. skin    (only with joints) Mj = jointMatrices[joints[4i + j]], 12 floats, row-major 3 x 4, column-vector convention p' = M [p; 1];
//              B[r][c] = ((w0 * M0[r][c] + w1 * M1[r][c]) + w2 * M2[r][c]) + w3 * M3[r][c]       weights as given: not renormalised, none skipped
//              p'[r]   = ((B[r][0] * p[0] + B[r][1] * p[1]) + B[r][2] * p[2]) + B[r][3]
//              normal through the cofactor matrix (right under non-uniform scale, no division): with b0, b1, b2 the rows of the 3 x 3 part,
//              c0 = b1 x b2, c1 = b2 x b0, c2 = b0 x b1, every cross-product component a * b - c * d (two products, one difference),
//              det     = (b0[0] * c0[0] + b0[1] * c0[1]) + b0[2] * c0[2]
//              n'[r]   = (cr[0] * n[0] + cr[1] * n[1]) + cr[2] * n[2];   det < 0: n' = -n' and s = -s   (a mirroring joint flips handedness)
//              t'[r]   = (B[r][0] * t[0] + B[r][1] * t[1]) + B[r][2] * t[2]
//   3. unit    always, n and t separately: l2 = (v0 * v0 + v1 * v1) + v2 * v2; if l2 > 0 and l2 is finite, v = v / sqrt(l2) componentwise
//              (a division, not a reciprocal); otherwise v stays as it is (a zero or non-finite vector is not touched)
//   4. flags   a joint index >= jointCount is an error of the input; the function reads min(index, jointCount - 1), so it stays inside the
//              palette, and says so in kJointOutOfRange of its result. kPositionNotFinite: deform::position_finite of the output position.
#pragma once

#include "pt_deform.h"

namespace hrt {
namespace skin {

constexpr uint32_t kPositionNotFinite = 1u, kJointOutOfRange = 2u;      // result bits of skin_vertex = the words of the kernels' status array

HRT_DEFORM_HD void unit_or_keep(float* v)
{
    const float l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (l2 > 0.0f && (deform::float_bits(l2) & 0x7f800000u) != 0x7f800000u) {
        const float l = __builtin_sqrtf(l2);
        v[0] = v[0] / l; v[1] = v[1] / l; v[2] = v[2] / l;
    }
}

// c = a x b
HRT_DEFORM_HD void cross3(const float* a, const float* b, float* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// Steps 1 to 3 on values the caller fetched. `delta(k, d)` fills d[9] (pos, normal, tangent) with target k's record of this vertex and
// is called only for a non-zero weight; `matrix(j, m)` fills m[12] with joint matrix j < jointCount. Without `skinned`, step 2 is left out
// and joints, weights, jointCount and matrix are not used.
template <class Delta, class Matrix>
HRT_DEFORM_HD uint32_t skin_vertex(const HrptVertexFloat& base, const float* morphWeights, uint32_t targetCount, Delta delta, bool skinned, const uint16_t* joints,
                                   const float* weights, uint32_t jointCount, Matrix matrix, HrptVertexFloat& out)
{
    uint32_t status = 0;
    float p[3] = { base.pos[0], base.pos[1], base.pos[2] }, n[3] = { base.normal[0], base.normal[1], base.normal[2] };
    float t[3] = { base.tangent[0], base.tangent[1], base.tangent[2] }, s = base.tangent[3];
    for (uint32_t k = 0; k < targetCount; ++k) {
        const float w = morphWeights[k];
        if (w == 0.0f) continue;
        float d[9];
        delta(k, d);
        for (int c = 0; c < 3; ++c) { p[c] = p[c] + w * d[c]; n[c] = n[c] + w * d[3 + c]; t[c] = t[c] + w * d[6 + c]; }
    }
    if (skinned) {
        float B[12];
        for (int j = 0; j < 4; ++j) {
            uint32_t index = joints[j];
            if (index >= jointCount) { index = jointCount - 1u; status |= kJointOutOfRange; }
            float m[12];
            matrix(index, m);
            const float w = weights[j];
            for (int e = 0; e < 12; ++e) B[e] = j == 0 ? w * m[e] : B[e] + w * m[e];
        }
        const float* b0 = B; const float* b1 = B + 4; const float* b2 = B + 8;
        float q[3], c0[3], c1[3], c2[3], m[3], u[3];
        for (int r = 0; r < 3; ++r) q[r] = ((B[4 * r] * p[0] + B[4 * r + 1] * p[1]) + B[4 * r + 2] * p[2]) + B[4 * r + 3];
        cross3(b1, b2, c0); cross3(b2, b0, c1); cross3(b0, b1, c2);
        const float det = (b0[0] * c0[0] + b0[1] * c0[1]) + b0[2] * c0[2];
        m[0] = (c0[0] * n[0] + c0[1] * n[1]) + c0[2] * n[2];
        m[1] = (c1[0] * n[0] + c1[1] * n[1]) + c1[2] * n[2];
        m[2] = (c2[0] * n[0] + c2[1] * n[1]) + c2[2] * n[2];
        if (det < 0.0f) { m[0] = -m[0]; m[1] = -m[1]; m[2] = -m[2]; s = -s; }
        for (int r = 0; r < 3; ++r) u[r] = (B[4 * r] * t[0] + B[4 * r + 1] * t[1]) + B[4 * r + 2] * t[2];
        for (int c = 0; c < 3; ++c) { p[c] = q[c]; n[c] = m[c]; t[c] = u[c]; }
    }
    unit_or_keep(n);
    unit_or_keep(t);
    for (int c = 0; c < 3; ++c) { out.pos[c] = p[c]; out.normal[c] = n[c]; out.tangent[c] = t[c]; }
    out.uv[0] = base.uv[0]; out.uv[1] = base.uv[1]; out.tangent[3] = s;
    if (!deform::position_finite(p)) status |= kPositionNotFinite;
    return status;
}

// The same over the arrays of HrptSkinArgs (host memory on the host, device memory in a kernel that gathers its palette from global memory).
HRT_DEFORM_HD uint32_t skin_vertex(const HrptSkinArgs& a, uint32_t i, HrptVertexFloat& out)
{
    const HrptSkinMorphDelta* deltas = a.deltas;
    const float* matrices = a.jointMatrices;
    const uint32_t count = a.count;
    return skin_vertex(
        a.base[i], a.morphWeights, a.targetCount,
        [=](uint32_t k, float* d) {
            const HrptSkinMorphDelta& r = deltas[(size_t)k * count + i];
            for (int c = 0; c < 3; ++c) { d[c] = r.pos[c]; d[3 + c] = r.normal[c]; d[6 + c] = r.tangent[c]; }
        },
        a.joints != nullptr, a.joints ? a.joints + 4 * (size_t)i : nullptr, a.joints ? a.weights + 4 * (size_t)i : nullptr, a.jointCount,
        [=](uint32_t j, float* m) { for (int e = 0; e < 12; ++e) m[e] = matrices[12 * (size_t)j + e]; }, out);
}

} // namespace skin
} // namespace hrt

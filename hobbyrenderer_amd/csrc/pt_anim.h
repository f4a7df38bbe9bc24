// pt_anim.h -- the arithmetic of the animation stage (hrpt_animate_host, hrpt_animate): keyframe samplers, TRS composition, the node
// hierarchy, and what leaves the stage: instance matrices, the joint palette of hrpt_update_vertices_skinned and its morph weights. One
// __host__ __device__ source shared by the gfx950 kernels (pt_anim.hip) and the host executor (pt_anim_host.cpp); tests/anim_reference.py
// states the same in NumPy from the reference's Scene::Update / EvaluateAnimSampler (src/Scene.cpp:345-570), and all three agree bit for
// bit. DESIGN.md section 23 has the prose.
//
// float32 throughout, one rounding per operation (no FMA contraction), correctly rounded / and sqrt, evaluation order as written.
//   sampler   sample(): n = keyCount >= 1 keys (a sampler without keys never gets here: its channels are dead). n == 1, t <= time[0]:
//             value[0]; t >= time[n-1]: value[n-1]. Else k0 = the last i in [0, n-2] with t >= time[i] (a binary search; key times are
//             validated non-decreasing, so it is the reference's scan), k1 = k0 + 1, d = time[k1] - time[k0], a = d > 0 ? (t - time[k0]) / d : 0.
//     STEP                 v0
//     LINEAR, CUBICSPLINE  v0[c] + a * (v1[c] - v0[c])                     (the reference treats both alike; no shortest-arc flip)
//     CATMULLROM           with p0 = value[k0 > 0 ? k0 - 1 : k0], p1 = v0, p2 = v1, p3 = value[k1 < n - 1 ? k1 + 1 : k1], a2 = a * a, a3 = a * a2:
//                          w0 = ((2 * a2 - a3) - a) * 0.5      w1 = ((3 * a3 - 5 * a2) + 2) * 0.5
//                          w2 = ((4 * a2 - 3 * a3) + a) * 0.5  w3 = (a3 - a2) * 0.5
//                          result[c] = (w0 * p0[c] + w1 * p1[c]) + (w2 * p2[c] + w3 * p3[c])     (XMVectorCatmullRom's polynomial, this sum order)
//     SLERP                q0 = unit4(v0), q1 = unit4(v1), dot = ((q0x q1x + q0y q1y) + q0z q1z) + q0w q1w; dot < 0: q1 = -q1, dot = -dot.
//                          dot > kSlerpLinearAbove (0.9995): q0[c] + a * (q1[c] - q0[c]). Else s = sqrt(1 - dot * dot),
//                          omega = atan_first_quadrant(s, dot), w0 = hrt_sin((1 - a) * omega) / s, w1 = hrt_sin(a * omega) / s,
//                          result[c] = w0 * q0[c] + w1 * q1[c]. hrt_sin is detmath.h's; atan_first_quadrant is below.
//   unit4     l2 = ((x x + y y) + z z) + w w; l2 > 0 and finite: every component / sqrt(l2); otherwise the vector stays as it is.
//   channel   TRANSLATION, SCALE: xyz of the sample. ROTATION: unit4 of the sample (Scene.cpp:491). WEIGHTS: x.
//   local     x2 = x + x, y2 = y + y, z2 = z + z; xx = x * x2, yy = y * y2, zz = z * z2, xy = x * y2, xz = x * z2, yz = y * z2,
//             wx = w * x2, wy = w * y2, wz = w * z2; the rows of XMMatrixRotationQuaternion:
//               r0 = ((1 - yy) - zz, xy + wz, xz - wy)   r1 = (xy - wz, (1 - xx) - zz, yz + wx)   r2 = (xz + wy, yz - wx, (1 - xx) - yy)
//             local row i < 3 = (scale[i] * ri[0], scale[i] * ri[1], scale[i] * ri[2], 0), row 3 = (tx, ty, tz, 1): the product
//             XMMatrixScalingFromVector . XMMatrixRotationQuaternion . XMMatrixTranslationFromVector with its exact zeros and ones left out.
//   world     mul4x4: out[i][j] = ((a[i][0] b[0][j] + a[i][1] b[1][j]) + a[i][2] b[2][j]) + a[i][3] b[3][j], all 64 products.
//   palette   joint_matrix: M = inverseBind . world (mul4x4's entries, columns 0..2 only); out[r][c] = M[c][r], r < 3, c < 4.
#pragma once

#include "../../include/hobbyrt_pt.h"
#include "../../include/hobbyrt/detmath.h"

namespace hrt {
namespace anim {

constexpr float kSlerpLinearAbove = 0.9995f;
constexpr uint32_t kNoNode = 0xffffffffu;

// The tables the evaluation reads once hrpt_animation_create has resolved what is static: host memory in the executor, device memory in
// the kernels. Live channels only (their sampler has keys and at least one target survives), each with its live targets (those no later
// channel overrides), already in application order. The composed nodes come grouped by depth below the topmost composed ancestor: group g
// is order[groupFirst[g] .. groupFirst[g + 1]), and the parent of a node in group g > 0 is in group g - 1.
struct Tables {
    const HrptAnimSampler* samplers;       // as given
    const float* keyTimes;                 // as given
    const float* keyValues;                // as given, 4 floats per key, 16-byte aligned
    const HrptAnimChannel* channels;       // live channels; firstTarget / targetCount index `targets` below
    const uint32_t* targets;               // live targets: node index, or weight slot
    const uint32_t* order;                 // composed nodes by group
    const int32_t* orderParent;            // parent of order[k], -1 for a root
    const uint32_t* rangeNode;             // for instance instanceFirst + k of the closed range: the composed node it hangs under, or kNoNode
    const uint32_t* jointNode;             // node of joint j
    const float* inverseBind;              // 16 floats per joint
    uint32_t channelCount, composedCount, jointCount, animationCount, instanceFirst, instanceRange;
};

HRT_FN bool finite_bits(float x) { return (hrt_f2u(x) & 0x7f800000u) != 0x7f800000u; }

HRT_FN void unit4(float* q)
{
    const float l2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (l2 > 0.0f && finite_bits(l2)) {
        const float l = __builtin_sqrtf(l2);
        q[0] = q[0] / l; q[1] = q[1] / l; q[2] = q[2] / l; q[3] = q[3] / l;
    }
}

// atan(y / x) for y >= 0, x >= 0, not both zero: the single-precision Cephes scheme. x == 0: pi / 2. Else r = y / x;
// r > tan(3 pi / 8): base = pi / 2, r = -(1 / r); r > tan(pi / 8): base = pi / 4, r = (r - 1) / (r + 1); else base = 0. z = r * r,
// result = base + (((((8.05374449538e-2 z - 1.38776856032e-1) z + 1.99777106478e-1) z - 3.33329491539e-1) z) r + r).
HRT_FN float atan_first_quadrant(float y, float x)
{
    if (!(x > 0.0f)) return 1.57079637f;
    float r = y / x, base = 0.0f;
    if (r > 2.41421366f) { base = 1.57079637f; r = -(1.0f / r); }
    else if (r > 0.414213568f) { base = 0.785398185f; r = (r - 1.0f) / (r + 1.0f); }
    const float z = r * r;
    const float p = ((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f;
    return base + ((p * z) * r + r);
}

HRT_FN void slerp(const float* v0, const float* v1, float a, float* out)
{
    float q0[4] = { v0[0], v0[1], v0[2], v0[3] }, q1[4] = { v1[0], v1[1], v1[2], v1[3] };
    unit4(q0); unit4(q1);
    float dot = ((q0[0] * q1[0] + q0[1] * q1[1]) + q0[2] * q1[2]) + q0[3] * q1[3];
    if (dot < 0.0f) { dot = -dot; for (int c = 0; c < 4; ++c) q1[c] = -q1[c]; }
    if (dot > kSlerpLinearAbove) {
        for (int c = 0; c < 4; ++c) out[c] = q0[c] + a * (q1[c] - q0[c]);
        return;
    }
    const float s = __builtin_sqrtf(1.0f - dot * dot);
    const float omega = atan_first_quadrant(s, dot);
    const float w0 = hrt_sin((1.0f - a) * omega) / s, w1 = hrt_sin(a * omega) / s;
    for (int c = 0; c < 4; ++c) out[c] = w0 * q0[c] + w1 * q1[c];
}

// The value of sampler s (keyCount >= 1) at time t.
HRT_FN void sample(const HrptAnimSampler& s, const float* keyTimes, const float* keyValues, float t, float* out)
{
    const float* in = keyTimes + s.firstKey;
    const float* val = keyValues + 4 * (size_t)s.firstKey;
    const uint32_t n = s.keyCount;
    uint32_t whole = 0xffffffffu;
    if (n == 1 || t <= in[0]) whole = 0;
    else if (t >= in[n - 1]) whole = n - 1;
    if (whole != 0xffffffffu) { for (int c = 0; c < 4; ++c) out[c] = val[4 * (size_t)whole + c]; return; }
    uint32_t lo = 0, hi = n - 2;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (t >= in[mid]) lo = mid; else hi = mid - 1;
    }
    const uint32_t k0 = lo, k1 = lo + 1;
    const float d = in[k1] - in[k0];
    const float a = d > 0.0f ? (t - in[k0]) / d : 0.0f;
    const float* v0 = val + 4 * (size_t)k0;
    const float* v1 = val + 4 * (size_t)k1;
    if (s.interpolation == HRPT_ANIM_STEP) {
        for (int c = 0; c < 4; ++c) out[c] = v0[c];
    } else if (s.interpolation == HRPT_ANIM_SLERP) {
        slerp(v0, v1, a, out);
    } else if (s.interpolation == HRPT_ANIM_CATMULLROM) {
        const float* p0 = val + 4 * (size_t)(k0 > 0 ? k0 - 1 : k0);
        const float* p3 = val + 4 * (size_t)(k1 < n - 1 ? k1 + 1 : k1);
        const float a2 = a * a, a3 = a * a2;
        const float w0 = ((2.0f * a2 - a3) - a) * 0.5f, w1 = ((3.0f * a3 - 5.0f * a2) + 2.0f) * 0.5f;
        const float w2 = ((4.0f * a2 - 3.0f * a3) + a) * 0.5f, w3 = (a3 - a2) * 0.5f;
        for (int c = 0; c < 4; ++c) out[c] = (w0 * p0[c] + w1 * v0[c]) + (w2 * v1[c] + w3 * p3[c]);
    } else {
        for (int c = 0; c < 4; ++c) out[c] = v0[c] + a * (v1[c] - v0[c]);
    }
}

// Live channel k: samples once and writes its live targets. trs holds 12 floats per node (translation xyz, pad, rotation xyzw, scale xyz,
// pad), seeded from the base pose; every (node, path) and slot has at most one live writer, so there is no order to keep.
HRT_FN void apply_channel(const Tables& tb, uint32_t k, float t, float* trs, float* weights)
{
    const HrptAnimChannel ch = tb.channels[k];
    float v[4];
    sample(tb.samplers[ch.sampler], tb.keyTimes, tb.keyValues, t, v);
    if (ch.path == HRPT_ANIM_PATH_ROTATION) unit4(v);
    for (uint32_t i = 0; i < ch.targetCount; ++i) {
        const uint32_t target = tb.targets[ch.firstTarget + i];
        if (ch.path == HRPT_ANIM_PATH_WEIGHTS) { weights[target] = v[0]; continue; }
        float* p = trs + 12 * (size_t)target + (ch.path == HRPT_ANIM_PATH_TRANSLATION ? 0 : (ch.path == HRPT_ANIM_PATH_ROTATION ? 4 : 8));
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
        if (ch.path == HRPT_ANIM_PATH_ROTATION) p[3] = v[3];
    }
}

HRT_FN void local_matrix(const float* trs, float* m)
{
    const float x = trs[4], y = trs[5], z = trs[6], w = trs[7];
    const float x2 = x + x, y2 = y + y, z2 = z + z;
    const float xx = x * x2, yy = y * y2, zz = z * z2, xy = x * y2, xz = x * z2, yz = y * z2, wx = w * x2, wy = w * y2, wz = w * z2;
    const float r[9] = { (1.0f - yy) - zz, xy + wz, xz - wy, xy - wz, (1.0f - xx) - zz, yz + wx, xz + wy, yz - wx, (1.0f - xx) - yy };
    for (int i = 0; i < 3; ++i) {
        const float s = trs[8 + i];
        m[4 * i] = s * r[3 * i]; m[4 * i + 1] = s * r[3 * i + 1]; m[4 * i + 2] = s * r[3 * i + 2]; m[4 * i + 3] = 0.0f;
    }
    m[12] = trs[0]; m[13] = trs[1]; m[14] = trs[2]; m[15] = 1.0f;
}

HRT_FN void mul4x4(const float* a, const float* b, float* out)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            out[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j];
}

// Composed node order[k]: its world from its pose and its parent's world (which an earlier group, or the base pose, has written).
HRT_FN void compose_node(const Tables& tb, uint32_t k, const float* trs, float* worlds)
{
    const uint32_t node = tb.order[k];
    const int32_t parent = tb.orderParent[k];
    float local[16], world[16];
    local_matrix(trs + 12 * (size_t)node, local);
    if (parent >= 0) {
        float pw[16];
        for (int e = 0; e < 16; ++e) pw[e] = worlds[16 * (size_t)parent + e];
        mul4x4(local, pw, world);
    } else {
        for (int e = 0; e < 16; ++e) world[e] = local[e];
    }
    for (int e = 0; e < 16; ++e) worlds[16 * (size_t)node + e] = world[e];
}

HRT_FN void joint_matrix(const float* inverseBind, const float* world, float* out12)
{
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r)
            out12[4 * r + c] = ((inverseBind[4 * c] * world[r] + inverseBind[4 * c + 1] * world[4 + r]) + inverseBind[4 * c + 2] * world[8 + r]) + inverseBind[4 * c + 3] * world[12 + r];
}

} // namespace anim
} // namespace hrt

// ---- host side: what hrpt_animation_create keeps (pt_anim_host.cpp builds it, pt_capi.cpp uploads it) ----
#include <string>
#include <vector>

struct HrptAnimation {
    // the description, copied
    std::vector<HrptAnimSampler> samplers;
    std::vector<HrptAnimNode> nodes;
    std::vector<float> keyTimes, keyValues;
    // resolved at creation
    std::vector<HrptAnimChannel> channels;         // live channels in application order
    std::vector<uint32_t> targets;                 // their live targets
    std::vector<uint32_t> order, groupFirst;       // composed nodes by depth group; groupFirst has groups + 1 entries
    std::vector<int32_t> orderParent;
    std::vector<uint32_t> rangeNode;               // instances [instanceFirst, instanceFirst + rangeNode.size()): composed node or anim::kNoNode
    std::vector<uint32_t> jointNode;
    std::vector<float> inverseBind;
    std::vector<float> baseTrs, baseWorlds;        // 12 / 16 floats per node
    std::vector<float> durations, times;           // per animation
    uint32_t morphWeightCount = 0, instanceFirst = 0, instanceNeed = 0;   // instanceNeed: 1 + the largest instance index listed under any node (0: none)
    uint64_t serial = 0;                           // distinguishes animations that reuse an address (the per-context device copies are keyed by it)

    hrt::anim::Tables tables() const
    {
        return hrt::anim::Tables{ samplers.data(), keyTimes.data(), keyValues.data(), channels.data(), targets.data(), order.data(), orderParent.data(), rangeNode.data(),
                                  jointNode.data(), inverseBind.data(), (uint32_t)channels.size(), (uint32_t)order.size(), (uint32_t)jointNode.size(),
                                  (uint32_t)times.size(), instanceFirst, (uint32_t)rangeNode.size() };
    }
};

namespace hrt {
// Validates and resolves a description (pt_anim_host.cpp); nullptr and a message on a bad one.
HrptAnimation* animation_create(const HrptAnimationDesc& d, std::string& err);
void animation_advance(HrptAnimation& a, float dt);
// The evaluation on host threads; every output may be null. instances: the whole scene array (the caller checked its length).
void animate_host(const HrptAnimation& a, HrptPerInstanceData* instances, uint32_t instanceCount, float* palette, float* weights, float* nodeWorlds, int nthreads);
}

// pt_anim_host.cpp -- the host side of the animation stage: hrpt_animation_create's validation and everything it resolves once (durations,
// which channel targets are live, the composed nodes grouped by depth, the closed instance range), the clock, and the host-thread executor
// of pt_anim.h (hrpt_animate_host). Plain C++ with no HIP call, so that the sanitizer program (anim_asan.cpp, `make anim_asan`) builds it
// with g++ as it is.
#include "pt_anim.h"
#include "pt_host_rows.h"

#include <algorithm>
#include <atomic>
#include <cmath>

namespace hrt {

namespace {
std::atomic<uint64_t> g_serial{ 1 };

bool in_range(uint64_t first, uint64_t count, uint64_t size) { return first + count <= size; }
}

HrptAnimation* animation_create(const HrptAnimationDesc& d, std::string& err)
{
    auto bad = [&](const char* what) { err = what; return (HrptAnimation*)nullptr; };
    if (d.reserved != 0) return bad("reserved must be 0");
    if ((d.samplerCount && !d.samplers) || (d.channelCount && !d.channels) || (d.nodeCount && !d.nodes) || (d.jointCount && !d.joints) ||
        (d.keyCount && (!d.keyTimes || !d.keyValues)) || (d.targetCount && !d.targets) || (d.nodeInstanceCount && !d.nodeInstances))
        return bad("a NULL array with a non-zero count");
    for (uint32_t i = 0; i < d.samplerCount; ++i) {
        const HrptAnimSampler& s = d.samplers[i];
        if (s.interpolation > HRPT_ANIM_SLERP) return bad("unknown interpolation");
        if (s.animation >= d.animationCount) return bad("animation index out of range");
        if (!in_range(s.firstKey, s.keyCount, d.keyCount)) return bad("keyCount beyond the key arrays");
        for (uint32_t k = 0; k < s.keyCount; ++k) {
            const float t = d.keyTimes[s.firstKey + k];
            if (!anim::finite_bits(t)) return bad("a key time is not finite");
            if (k > 0 && t < d.keyTimes[s.firstKey + k - 1]) return bad("key times decrease");
        }
    }
    for (uint32_t i = 0; i < d.channelCount; ++i) {
        const HrptAnimChannel& c = d.channels[i];
        if (c.path > HRPT_ANIM_PATH_WEIGHTS) return bad("unknown path");
        if (c.sampler >= d.samplerCount) return bad("sampler index out of range");
        if (!in_range(c.firstTarget, c.targetCount, d.targetCount)) return bad("target range beyond the target array");
        const uint32_t limit = c.path == HRPT_ANIM_PATH_WEIGHTS ? d.morphWeightCount : d.nodeCount;
        for (uint32_t k = 0; k < c.targetCount; ++k)
            if (d.targets[c.firstTarget + k] >= limit) return bad(c.path == HRPT_ANIM_PATH_WEIGHTS ? "weight index out of range" : "node index out of range");
    }
    for (uint32_t i = 0; i < d.nodeCount; ++i) {
        const HrptAnimNode& n = d.nodes[i];
        if (n.parent < -1 || (n.parent >= 0 && (uint32_t)n.parent >= d.nodeCount)) return bad("parent index out of range");
        if (!in_range(n.firstInstance, n.instanceCount, d.nodeInstanceCount)) return bad("instance range beyond nodeInstances");
    }
    for (uint32_t j = 0; j < d.jointCount; ++j)
        if (d.joints[j].node >= d.nodeCount) return bad("joint node index out of range");

    // depth of every node below its root; a walk longer than the node count is a cycle
    std::vector<uint32_t> depth(d.nodeCount, 0xffffffffu);
    for (uint32_t i = 0; i < d.nodeCount; ++i) {
        if (depth[i] != 0xffffffffu) continue;
        std::vector<uint32_t> chain;
        int32_t at = (int32_t)i;
        while (at >= 0 && depth[(uint32_t)at] == 0xffffffffu) {
            if (chain.size() > d.nodeCount) return bad("parent cycle");
            chain.push_back((uint32_t)at);
            at = d.nodes[(uint32_t)at].parent;
        }
        uint32_t below = at >= 0 ? depth[(uint32_t)at] + 1u : 0u;
        for (size_t k = chain.size(); k-- > 0;) depth[chain[k]] = below++;
    }

    HrptAnimation* a = new HrptAnimation();
    a->serial = g_serial.fetch_add(1);
    a->samplers.assign(d.samplers, d.samplers + d.samplerCount);
    a->nodes.assign(d.nodes, d.nodes + d.nodeCount);
    a->keyTimes.assign(d.keyTimes, d.keyTimes + d.keyCount);
    a->keyValues.assign(d.keyValues, d.keyValues + 4 * (size_t)d.keyCount);
    a->morphWeightCount = d.morphWeightCount;
    a->durations.assign(d.animationCount, 0.0f);
    a->times.assign(d.animationCount, 0.0f);
    for (const HrptAnimSampler& s : a->samplers)
        if (s.keyCount) a->durations[s.animation] = std::max(a->durations[s.animation], a->keyTimes[s.firstKey + s.keyCount - 1]);

    // channels in (animation, channel) order; walking them backwards, the first writer met of a (node, path) or slot is the live one
    std::vector<uint32_t> byOrder;
    for (uint32_t i = 0; i < d.channelCount; ++i) if (d.samplers[d.channels[i].sampler].keyCount) byOrder.push_back(i);
    std::stable_sort(byOrder.begin(), byOrder.end(), [&](uint32_t x, uint32_t y) { return d.samplers[d.channels[x].sampler].animation < d.samplers[d.channels[y].sampler].animation; });
    std::vector<uint8_t> written(3 * (size_t)d.nodeCount + d.morphWeightCount, 0);
    std::vector<std::vector<uint32_t>> live(byOrder.size());
    for (size_t k = byOrder.size(); k-- > 0;) {
        const HrptAnimChannel& c = d.channels[byOrder[k]];
        for (uint32_t t = c.targetCount; t-- > 0;) {
            const uint32_t target = d.targets[c.firstTarget + t];
            const size_t slot = c.path == HRPT_ANIM_PATH_WEIGHTS ? 3 * (size_t)d.nodeCount + target : 3 * (size_t)target + c.path;
            if (!written[slot]) { written[slot] = 1; live[k].push_back(target); }
        }
    }
    std::vector<uint8_t> composed(d.nodeCount, 0);
    for (size_t k = 0; k < byOrder.size(); ++k) {
        if (live[k].empty()) continue;
        HrptAnimChannel c = d.channels[byOrder[k]];
        c.firstTarget = (uint32_t)a->targets.size(); c.targetCount = (uint32_t)live[k].size();
        a->targets.insert(a->targets.end(), live[k].rbegin(), live[k].rend());
        a->channels.push_back(c);
        if (c.path != HRPT_ANIM_PATH_WEIGHTS) for (uint32_t n : live[k]) composed[n] = 1;
    }

    // the composed set: targeted nodes and all their descendants; by increasing depth a parent is decided before its children
    std::vector<uint32_t> byDepth(d.nodeCount);
    for (uint32_t i = 0; i < d.nodeCount; ++i) byDepth[i] = i;
    std::stable_sort(byDepth.begin(), byDepth.end(), [&](uint32_t x, uint32_t y) { return depth[x] < depth[y]; });
    std::vector<uint32_t> group(d.nodeCount, 0);
    uint32_t groups = 0;
    for (uint32_t n : byDepth) {
        const int32_t p = d.nodes[n].parent;
        if (p >= 0 && composed[(uint32_t)p]) { composed[n] = 1; group[n] = group[(uint32_t)p] + 1u; }
        if (composed[n]) groups = std::max(groups, group[n] + 1u);
    }
    a->groupFirst.assign(groups + 1u, 0);
    for (uint32_t n = 0; n < d.nodeCount; ++n) if (composed[n]) ++a->groupFirst[group[n] + 1u];
    for (uint32_t g = 0; g < groups; ++g) a->groupFirst[g + 1u] += a->groupFirst[g];
    a->order.resize(a->groupFirst[groups]); a->orderParent.resize(a->order.size());
    std::vector<uint32_t> fill(a->groupFirst.begin(), a->groupFirst.end());
    for (uint32_t n = 0; n < d.nodeCount; ++n)
        if (composed[n]) { const uint32_t k = fill[group[n]]++; a->order[k] = n; a->orderParent[k] = d.nodes[n].parent; }

    // instances: none listed twice; the closed range of those under composed nodes
    std::vector<uint32_t> listed;
    uint32_t lo = 0xffffffffu, hi = 0;
    for (uint32_t n = 0; n < d.nodeCount; ++n)
        for (uint32_t k = 0; k < d.nodes[n].instanceCount; ++k) {
            const uint32_t inst = d.nodeInstances[d.nodes[n].firstInstance + k];
            if (inst == 0xffffffffu) { delete a; return bad("instance index out of range"); }
            listed.push_back(inst);
            a->instanceNeed = std::max(a->instanceNeed, inst + 1u);
            if (composed[n]) { lo = std::min(lo, inst); hi = std::max(hi, inst); }
        }
    std::sort(listed.begin(), listed.end());
    if (std::adjacent_find(listed.begin(), listed.end()) != listed.end()) { delete a; return bad("an instance is listed twice"); }
    if (lo <= hi) {
        a->instanceFirst = lo;
        a->rangeNode.assign((size_t)(hi - lo) + 1u, anim::kNoNode);
        for (uint32_t n = 0; n < d.nodeCount; ++n)
            if (composed[n]) for (uint32_t k = 0; k < d.nodes[n].instanceCount; ++k) a->rangeNode[d.nodeInstances[d.nodes[n].firstInstance + k] - lo] = n;
    }

    a->jointNode.resize(d.jointCount); a->inverseBind.resize(16 * (size_t)d.jointCount);
    for (uint32_t j = 0; j < d.jointCount; ++j) {
        a->jointNode[j] = d.joints[j].node;
        std::copy(d.joints[j].inverseBind, d.joints[j].inverseBind + 16, a->inverseBind.begin() + 16 * (size_t)j);
    }
    a->baseTrs.assign(12 * (size_t)d.nodeCount, 0.0f); a->baseWorlds.resize(16 * (size_t)d.nodeCount);
    for (uint32_t n = 0; n < d.nodeCount; ++n) {
        const HrptAnimNode& s = d.nodes[n];
        float* p = &a->baseTrs[12 * (size_t)n];
        for (int c = 0; c < 3; ++c) { p[c] = s.translation[c]; p[8 + c] = s.scale[c]; }
        for (int c = 0; c < 4; ++c) p[4 + c] = s.rotation[c];
        std::copy(s.baseWorld, s.baseWorld + 16, a->baseWorlds.begin() + 16 * (size_t)n);
    }
    return a;
}

void animation_advance(HrptAnimation& a, float dt)
{
    for (size_t i = 0; i < a.times.size(); ++i) {
        a.times[i] = a.times[i] + dt;
        if (a.durations[i] > 0.0f) a.times[i] = fmodf(a.times[i], a.durations[i]);
    }
}

void animate_host(const HrptAnimation& a, HrptPerInstanceData* instances, uint32_t instanceCount, float* palette, float* weights, float* nodeWorlds, int nthreads)
{
    constexpr uint32_t kChunk = 256;
    const anim::Tables tb = a.tables();
    auto chunks = [](size_t n) { return (int)(n / kChunk + (n % kChunk != 0)); };
    auto each = [&](size_t first, size_t count, auto fn) {
        over_rows(chunks(count), nthreads, [&](int c) {
            const size_t b = first + (size_t)c * kChunk, e = std::min(first + count, b + kChunk);
            for (size_t k = b; k < e; ++k) fn(k);
        });
    };
    std::vector<float> trs(a.baseTrs), worlds(a.baseWorlds), w(a.morphWeightCount, 0.0f);
    each(0, tb.channelCount, [&](size_t k) { anim::apply_channel(tb, (uint32_t)k, a.times[a.samplers[tb.channels[k].sampler].animation], trs.data(), w.data()); });
    for (size_t g = 0; g + 1 < a.groupFirst.size(); ++g)
        each(a.groupFirst[g], a.groupFirst[g + 1] - a.groupFirst[g], [&](size_t k) { anim::compose_node(tb, (uint32_t)k, trs.data(), worlds.data()); });
    if (instances) {
        each(0, instanceCount, [&](size_t i) {
            HrptPerInstanceData& r = instances[i];
            for (int e = 0; e < 16; ++e) r.m_PrevWorld[e] = r.m_World[e];
            if (i < tb.instanceFirst || i - tb.instanceFirst >= tb.instanceRange) return;
            const uint32_t node = tb.rangeNode[i - tb.instanceFirst];
            if (node != anim::kNoNode) for (int e = 0; e < 16; ++e) r.m_World[e] = worlds[16 * (size_t)node + e];
        });
    }
    if (palette) each(0, tb.jointCount, [&](size_t j) { anim::joint_matrix(tb.inverseBind + 16 * j, &worlds[16 * (size_t)tb.jointNode[j]], palette + 12 * j); });
    if (weights) std::copy(w.begin(), w.end(), weights);
    if (nodeWorlds) std::copy(worlds.begin(), worlds.end(), nodeWorlds);
}

} // namespace hrt

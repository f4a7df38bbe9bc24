// anim_asan.cpp -- driver of the sanitizer build of the animation stage's host side (`make anim_asan`: AddressSanitizer + UBSan, CPU only).
// Runs pt_anim.h through animation_create / animation_advance / animate_host (pt_anim_host.cpp) over exactly sized heap arrays: random
// forests with every interpolation and path, samplers of 0, 1, 2 and many keys, equal key times, channels with several and with repeated
// targets, instances dealt in a shuffled order, joints, weight slots; 1, 3 and 16 threads; times below, on, between and beyond the keys
// and hostile ones (NaN, infinities, huge); hostile key values. Then every kind of invalid table, each of which creation must refuse
// without reading past an array: indices one past the end and 0xffffffff, ranges that wrap, a parent cycle, decreasing and non-finite
// key times, an instance listed twice, a non-zero reserved word. Checks what can be said without a second implementation: the result does
// not depend on nthreads, m_PrevWorld is the old m_World everywhere, a node outside the composed set keeps baseWorld, an unlisted
// instance keeps its world, the clock stays inside [0, duration). Any out-of-bounds access or other report ends the program with a
// non-zero status.   usage: anim_asan [seed]
#include "asan_common.h"
#include "pt_anim.h"

#include <functional>

struct Case {
    std::vector<HrptAnimSampler> samplers;
    std::vector<HrptAnimChannel> channels;
    std::vector<HrptAnimNode> nodes;
    std::vector<HrptAnimJoint> joints;
    std::vector<float> keyTimes, keyValues;
    std::vector<uint32_t> targets, nodeInstances;
    uint32_t animationCount = 0, morphWeightCount = 0, instanceCount = 0;
    // exactly sized copies, so that one element past any array is a report
    HrptAnimationDesc desc() const
    {
        return HrptAnimationDesc{ samplers.data(), channels.data(), nodes.data(), joints.data(), keyTimes.data(), keyValues.data(), targets.data(), nodeInstances.data(),
                                  (uint32_t)samplers.size(), (uint32_t)channels.size(), (uint32_t)nodes.size(), (uint32_t)joints.size(), (uint32_t)keyTimes.size(),
                                  (uint32_t)targets.size(), (uint32_t)nodeInstances.size(), animationCount, morphWeightCount, 0 };
    }
};

static int fail(const char* what, uint32_t n) { std::fprintf(stderr, "anim_asan: %s at %u nodes\n", what, n); return -1; }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() * (float)n) % n; }

static void make_case(Case& c, uint32_t nodeCount, bool hostileValues)
{
    c = Case();
    c.animationCount = 3; c.morphWeightCount = 4;
    c.nodes.resize(nodeCount);
    std::vector<uint32_t> deal;
    for (uint32_t n = 0; n < nodeCount; ++n) {
        HrptAnimNode& node = c.nodes[n];
        node.parent = (n == 0 || rnd() < 0.2f) ? -1 : (int32_t)below(n);
        for (int k = 0; k < 3; ++k) { node.translation[k] = 2.0f * rnd() - 1.0f; node.scale[k] = 0.5f + rnd(); }
        for (int k = 0; k < 4; ++k) node.rotation[k] = 2.0f * rnd() - 1.0f;
        for (int k = 0; k < 16; ++k) node.baseWorld[k] = 2.0f * rnd() - 1.0f;
        node.instanceCount = below(3);
        node.firstInstance = (uint32_t)deal.size();
        for (uint32_t k = 0; k < node.instanceCount; ++k) deal.push_back((uint32_t)deal.size());
    }
    c.instanceCount = (uint32_t)deal.size() + 2u;                      // two records nobody lists
    for (size_t k = deal.size(); k > 1; --k) std::swap(deal[k - 1], deal[below((uint32_t)k)]);
    c.nodeInstances = deal;
    const uint32_t keyCounts[5] = { 0u, 1u, 2u, 7u, 37u };
    for (uint32_t s = 0; s < 15; ++s) {
        HrptAnimSampler sm{ s % 5u, (uint32_t)c.keyTimes.size(), keyCounts[(s / 5u + s) % 5u], s % 3u };
        float t = rnd();
        for (uint32_t k = 0; k < sm.keyCount; ++k) {
            c.keyTimes.push_back(t);
            if (k % 4u != 2u) t += rnd();                               // some equal key times
            for (int e = 0; e < 4; ++e) c.keyValues.push_back(hostileValues && (k + e) % 5u == 0u ? kBad[(s + k) % 8u] : 2.0f * rnd() - 1.0f);
        }
        c.samplers.push_back(sm);
    }
    if (nodeCount)
        for (uint32_t k = 0; k < 24; ++k) {
            HrptAnimChannel ch{ k % 4u, below(15), (uint32_t)c.targets.size(), 1u + below(3) };
            for (uint32_t t = 0; t < ch.targetCount; ++t) c.targets.push_back(ch.path == HRPT_ANIM_PATH_WEIGHTS ? below(c.morphWeightCount) : below(nodeCount));
            if (ch.targetCount > 1 && k % 5u == 0u) c.targets.back() = c.targets[ch.firstTarget];      // a repeated target
            c.channels.push_back(ch);
        }
    for (uint32_t j = 0; j < nodeCount / 2u; ++j) {
        HrptAnimJoint joint;
        joint.node = below(nodeCount);
        for (int e = 0; e < 16; ++e) joint.inverseBind[e] = 2.0f * rnd() - 1.0f;
        c.joints.push_back(joint);
    }
}

static int run(uint32_t nodeCount, bool hostile)
{
    Case c;
    make_case(c, nodeCount, hostile);
    std::string err;
    const HrptAnimationDesc d = c.desc();
    HrptAnimation* a = hrt::animation_create(d, err);
    if (!a) { std::fprintf(stderr, "anim_asan: %s\n", err.c_str()); return fail("a valid table was refused", nodeCount); }
    std::vector<uint8_t> composed(nodeCount, 0);
    for (uint32_t n : a->order) composed[n] = 1;
    int calls = 0;
    const float hostileTimes[6] = { kNan, kInf, -kInf, 3e38f, -1.0f, 0.0f };
    for (int step = 0; step < 8; ++step) {
        if (hostile) for (float& t : a->times) t = hostileTimes[(step + (int)(&t - a->times.data())) % 6];
        else hrt::animation_advance(*a, step == 3 ? 50.0f : 0.37f * (float)step);
        if (!hostile)
            for (size_t i = 0; i < a->times.size(); ++i)
                if (a->durations[i] > 0.0f && !(a->times[i] >= 0.0f && a->times[i] < a->durations[i])) { delete a; return fail("the clock left [0, duration)", nodeCount); }
        std::vector<HrptPerInstanceData> start(c.instanceCount);
        for (HrptPerInstanceData& r : start) { float* f = reinterpret_cast<float*>(&r); for (int k = 0; k < 40; ++k) f[k] = rnd(); }
        std::vector<HrptPerInstanceData> ref, out;
        std::vector<float> refPalette, refWeights, refWorlds;
        const int threads[3] = { 1, 3, 16 };
        for (int t : threads) {
            out = start;
            std::vector<float> palette(12 * c.joints.size()), weights(c.morphWeightCount), worlds(16 * (size_t)nodeCount);
            hrt::animate_host(*a, out.data(), c.instanceCount, palette.data(), weights.data(), worlds.data(), t);
            ++calls;
            if (t == 1) { ref = out; refPalette = palette; refWeights = weights; refWorlds = worlds; continue; }
            auto differs = [](const void* x, const void* y, size_t bytes) { return bytes && std::memcmp(x, y, bytes) != 0; };
            if (differs(out.data(), ref.data(), out.size() * sizeof(HrptPerInstanceData)) || differs(palette.data(), refPalette.data(), palette.size() * 4) ||
                differs(weights.data(), refWeights.data(), weights.size() * 4) || differs(worlds.data(), refWorlds.data(), worlds.size() * 4)) {
                delete a;
                return fail("result depends on nthreads", nodeCount);
            }
        }
        for (uint32_t i = 0; i < c.instanceCount; ++i)
            if (std::memcmp(ref[i].m_PrevWorld, start[i].m_World, 64) != 0 || std::memcmp(&ref[i].m_MaterialIndex, &start[i].m_MaterialIndex, 32) != 0) { delete a; return fail("the roll", nodeCount); }
        for (uint32_t n = 0; n < nodeCount; ++n) {
            if (!composed[n] && std::memcmp(&refWorlds[16 * (size_t)n], c.nodes[n].baseWorld, 64) != 0) { delete a; return fail("a static node moved", nodeCount); }
            for (uint32_t k = 0; k < c.nodes[n].instanceCount; ++k) {
                const HrptPerInstanceData& r = ref[c.nodeInstances[c.nodes[n].firstInstance + k]];
                const void* want = composed[n] ? (const void*)&refWorlds[16 * (size_t)n] : (const void*)start[c.nodeInstances[c.nodes[n].firstInstance + k]].m_World;
                if (std::memcmp(r.m_World, want, 64) != 0) { delete a; return fail("an instance world", nodeCount); }
            }
        }
        // every output may be null, and so may the instances
        hrt::animate_host(*a, nullptr, 0, nullptr, nullptr, nullptr, 3);
        ++calls;
    }
    delete a;
    return calls;
}

// Every mutation must be refused; `mutate` gets a fresh valid case.
static int refused(uint32_t nodeCount, const char* what, const std::function<void(Case&, HrptAnimationDesc&)>& mutate)
{
    Case c;
    make_case(c, nodeCount, false);
    HrptAnimationDesc d = c.desc();
    mutate(c, d);
    std::string err;
    HrptAnimation* a = hrt::animation_create(d, err);
    if (a) { delete a; return fail(what, nodeCount); }
    return 1;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    int calls = 0;
    for (uint32_t n : { 0u, 1u, 2u, 9u, 255u, 256u, 257u, 700u })
        for (int hostile = 0; hostile < 2; ++hostile) {
            const int r = run(n, hostile != 0);
            if (r < 0) return 1;
            calls += r;
        }
    using D = HrptAnimationDesc;
    const std::pair<const char*, std::function<void(Case&, D&)>> bad[] = {
        { "reserved accepted", [](Case&, D& d) { d.reserved = 1; } },
        { "parent one past the end accepted", [](Case& c, D&) { c.nodes[5].parent = (int32_t)c.nodes.size(); } },
        { "parent -2 accepted", [](Case& c, D&) { c.nodes[5].parent = -2; } },
        { "parent cycle accepted", [](Case& c, D&) { c.nodes[3].parent = 8; c.nodes[8].parent = 6; c.nodes[6].parent = 3; } },
        { "self parent accepted", [](Case& c, D&) { c.nodes[0].parent = 0; } },
        { "node target accepted", [](Case& c, D&) { c.channels[0].path = HRPT_ANIM_PATH_SCALE; c.targets[c.channels[0].firstTarget] = (uint32_t)c.nodes.size(); } },
        { "weight target accepted", [](Case& c, D&) { c.channels[0].path = HRPT_ANIM_PATH_WEIGHTS; c.targets[c.channels[0].firstTarget] = 0xffffffffu; } },
        { "sampler index accepted", [](Case& c, D&) { c.channels[1].sampler = (uint32_t)c.samplers.size(); } },
        { "animation index accepted", [](Case& c, D&) { c.samplers[2].animation = c.animationCount; } },
        { "target range accepted", [](Case& c, D&) { c.channels[2].firstTarget = (uint32_t)c.targets.size(); c.channels[2].targetCount = 1; } },
        { "wrapping target range accepted", [](Case& c, D&) { c.channels[2].firstTarget = 0xffffffffu; c.channels[2].targetCount = 2; } },
        { "key range accepted", [](Case& c, D&) { c.samplers[4].firstKey = (uint32_t)c.keyTimes.size(); c.samplers[4].keyCount = 1; } },
        { "wrapping key range accepted", [](Case& c, D&) { c.samplers[4].firstKey = 0xfffffff0u; c.samplers[4].keyCount = 0x20u; } },
        { "instance range accepted", [](Case& c, D&) { c.nodes[1].firstInstance = (uint32_t)c.nodeInstances.size(); c.nodes[1].instanceCount = 1; } },
        { "instance listed twice accepted", [](Case& c, D&) { c.nodeInstances[0] = c.nodeInstances[1]; } },
        { "instance 0xffffffff accepted", [](Case& c, D&) { c.nodeInstances[0] = 0xffffffffu; } },
        { "joint node accepted", [](Case& c, D&) { c.joints[0].node = (uint32_t)c.nodes.size(); } },
        { "unknown path accepted", [](Case& c, D&) { c.channels[0].path = 4; } },
        { "unknown interpolation accepted", [](Case& c, D&) { c.samplers[0].interpolation = 5; } },
        { "decreasing key times accepted", [](Case& c, D&) { c.keyTimes[c.samplers[3].firstKey + 1] = -5.0f; } },
        { "NaN key time accepted", [](Case& c, D&) { c.keyTimes[c.samplers[3].firstKey] = kNan; } },
        { "infinite key time accepted", [](Case& c, D&) { c.keyTimes[c.samplers[3].firstKey + c.samplers[3].keyCount - 1] = kInf; } },
        { "NULL nodes accepted", [](Case&, D& d) { d.nodes = nullptr; } },
        { "NULL key values accepted", [](Case&, D& d) { d.keyValues = nullptr; } },
    };
    for (const auto& b : bad) {
        const int r = refused(40, b.first, b.second);
        if (r < 0) return 1;
        calls += r;
    }
    (void)make_view; (void)kSizes;
    std::printf("anim_asan: %d calls, no report\n", calls);
    return 0;
}

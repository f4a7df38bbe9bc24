// skin_asan.cpp -- driver of the sanitizer build of the vertex producer's host side (`make skin_asan`: AddressSanitizer + UBSan, CPU only).
// Runs pt_skin.h through skin_vertices_host over exactly sized heap arrays: random poses (with and without joints, with and without
// targets, one target weight exactly zero), the edge rows of the definition (identity palette, a zero 3 x 3 block, a mirrored joint,
// weights that do not sum to 1, a weight of -0 on a target whose deltas hold inf, a zero-length base normal, every tangent sign), hostile
// values in every input, counts around the chunk size with unaligned tails, 1, 3 and 16 threads. Then a joint index out of range: the
// executor refuses it and writes nothing, and the shared function called directly stays inside the palette (the clamp of pt_skin.h step 4)
// and says so. Checks what can be said without a second implementation: uv is copied, tangent[3] keeps its magnitude bits, a normal that
// was normalised has unit length, the identity pose copies positions bit for bit, and the result does not depend on nthreads. Any
// out-of-bounds access or other report ends the program with a non-zero status.   usage: skin_asan [seed]
#include "asan_common.h"
#include "pt_skin.h"

namespace hrt {
uint32_t skin_vertices_host(const HrptSkinArgs& args, HrptVertexFloat* out, int nthreads);
}

struct Case {
    std::vector<HrptVertexFloat> base;
    std::vector<uint16_t> joints;
    std::vector<float> weights, palette, morphWeights;
    std::vector<HrptSkinMorphDelta> deltas;
    HrptSkinArgs args;
};

static int fail(const char* what, uint32_t count) { std::fprintf(stderr, "skin_asan: %s at count %u\n", what, count); return -1; }

// mode 0: random, 1: edge rows, 2: hostile values
static void make_case(Case& c, uint32_t count, uint32_t jointCount, uint32_t targetCount, int mode)
{
    c.base.resize(count);
    for (uint32_t i = 0; i < count; ++i) {
        float* f = reinterpret_cast<float*>(&c.base[i]);
        for (int k = 0; k < 12; ++k) f[k] = 3.0f * rnd() - 1.5f;
        const float signs[4] = { 1.0f, -1.0f, 0.0f, -0.0f };
        c.base[i].tangent[3] = signs[i % 4];
        if (mode == 1 && i % 7 == 3) c.base[i].normal[0] = c.base[i].normal[1] = c.base[i].normal[2] = 0.0f;       // zero-length base normal
        if (mode == 2) f[i % 12] = kBad[(i / 12) % 8];
    }
    c.joints.clear(); c.weights.clear(); c.palette.clear();
    if (jointCount) {
        c.joints.resize(4 * (size_t)count); c.weights.resize(4 * (size_t)count); c.palette.resize(12 * (size_t)jointCount);
        for (uint32_t j = 0; j < jointCount; ++j) {
            float* m = &c.palette[12 * (size_t)j];
            for (int e = 0; e < 12; ++e) m[e] = 2.0f * rnd() - 1.0f;
            if (mode == 1 && j % 4 == 0) for (int e = 0; e < 12; ++e) m[e] = (e % 5 == 0) ? 1.0f : 0.0f;             // identity
            if (mode == 1 && j % 4 == 1) for (int e = 0; e < 12; ++e) m[e] = (e % 4 == 3) ? m[e] : 0.0f;             // zero 3 x 3 block
            if (mode == 1 && j % 4 == 2) for (int e = 0; e < 12; ++e) m[e] = (e % 5 == 0) ? (e == 0 ? -1.0f : 1.0f) : 0.0f;     // mirror in x
            if (mode == 2 && j % 3 == 0) m[j % 12] = kBad[(j / 3) % 8];
        }
        for (size_t k = 0; k < c.joints.size(); ++k) {
            c.joints[k] = (uint16_t)((uint32_t)(rnd() * (float)jointCount) % jointCount);
            c.weights[k] = mode == 1 ? rnd() * 1.5f : rnd();                                                        // (not summing to 1)
            if (mode == 1 && (k / 4) % 5 == 0) { c.joints[k] = (uint16_t)(((k / 20) % 3) % jointCount); c.weights[k] = (k % 4 == 0) ? 1.0f : 0.0f; }   // one joint alone
            if (mode == 2 && k % 37 == 0) c.weights[k] = kBad[(k / 37) % 8];
        }
    }
    c.deltas.clear(); c.morphWeights.clear();
    if (targetCount) {
        c.deltas.resize((size_t)targetCount * count); c.morphWeights.resize(targetCount);
        for (uint32_t k = 0; k < targetCount; ++k) {
            c.morphWeights[k] = (k == 1) ? (mode == 1 ? -0.0f : 0.0f) : rnd();
            for (uint32_t i = 0; i < count; ++i) {
                float* d = reinterpret_cast<float*>(&c.deltas[(size_t)k * count + i]);
                for (int e = 0; e < 9; ++e) d[e] = (k == 1) ? kInf : 0.2f * rnd() - 0.1f;                          // the skipped target holds inf
                if (mode == 2 && k != 1 && i % 11 == 0) d[i % 9] = kBad[(i / 11) % 8];
            }
        }
    }
    c.args = HrptSkinArgs{ c.base.data(), jointCount ? c.joints.data() : nullptr, jointCount ? c.weights.data() : nullptr, jointCount ? c.palette.data() : nullptr,
                           targetCount ? c.deltas.data() : nullptr, targetCount ? c.morphWeights.data() : nullptr, count, jointCount, targetCount, 0 };
}

static int run(uint32_t count, uint32_t jointCount, uint32_t targetCount, int mode)
{
    Case c;
    make_case(c, count, jointCount, targetCount, mode);
    std::vector<HrptVertexFloat> ref(count), out(count);
    int calls = 0;
    const int threads[3] = { 1, 3, 16 };
    for (int t : threads) {
        std::vector<HrptVertexFloat>& dst = t == 1 ? ref : out;
        if (count) std::memset(dst.data(), 0xA5, dst.size() * sizeof(HrptVertexFloat));
        const uint32_t status = hrt::skin_vertices_host(c.args, dst.data(), t);
        ++calls;
        if (status & hrt::skin::kJointOutOfRange) return fail("valid joints reported out of range", count);
        if (t != 1 && count && std::memcmp(out.data(), ref.data(), (size_t)count * sizeof(HrptVertexFloat)) != 0) return fail("result depends on nthreads", count);
    }
    for (uint32_t i = 0; i < count; ++i) {
        const HrptVertexFloat& b = c.base[i]; const HrptVertexFloat& r = ref[i];
        if (std::memcmp(r.uv, b.uv, 8) != 0) return fail("uv not copied", count);
        if ((hrt::deform::float_bits(r.tangent[3]) ^ hrt::deform::float_bits(b.tangent[3])) & 0x7fffffffu) return fail("tangent[3] changed beyond its sign", count);
        if (mode != 2) {
            const double l = std::sqrt((double)r.normal[0] * r.normal[0] + (double)r.normal[1] * r.normal[1] + (double)r.normal[2] * r.normal[2]);
            if (!(l == 0.0 || std::fabs(l - 1.0) < 1e-6)) return fail("a normal is neither unit nor zero", count);
        }
        if (mode == 1 && jointCount && targetCount == 0 && i % 5 == 0 && c.joints[4 * (size_t)i] == 0 && std::memcmp(r.pos, b.pos, 12) != 0)
            return fail("the identity joint moved a position", count);
    }
    return calls;
}

// One index out of range (== jointCount, then 65535) in an exactly sized palette.
static int run_out_of_range(uint32_t count, uint32_t jointCount, uint16_t index)
{
    Case c;
    make_case(c, count, jointCount, 1, 0);
    const size_t where = 4 * (size_t)(count - 1) + 2;
    c.joints[where] = index;
    std::vector<HrptVertexFloat> out(count), untouched(count);
    std::memset(out.data(), 0xA5, out.size() * sizeof(HrptVertexFloat));
    std::memset(untouched.data(), 0xA5, untouched.size() * sizeof(HrptVertexFloat));
    int calls = 0;
    const int threads[3] = { 1, 3, 16 };
    for (int t : threads) {
        const uint32_t status = hrt::skin_vertices_host(c.args, out.data(), t);
        ++calls;
        if (status != hrt::skin::kJointOutOfRange) return fail("an index out of range was not refused", count);
        if (std::memcmp(out.data(), untouched.data(), out.size() * sizeof(HrptVertexFloat)) != 0) return fail("a refused call wrote its output", count);
    }
    // the shared function itself: reads joint jointCount - 1 instead, and reports it
    HrptVertexFloat direct, clamped;
    const uint32_t status = hrt::skin::skin_vertex(c.args, count - 1, direct);
    if (!(status & hrt::skin::kJointOutOfRange)) return fail("skin_vertex did not report the index", count);
    c.joints[where] = (uint16_t)(jointCount - 1);
    if (hrt::skin::skin_vertex(c.args, count - 1, clamped) & hrt::skin::kJointOutOfRange) return fail("skin_vertex reported a valid index", count);
    if (std::memcmp(&direct, &clamped, sizeof direct) != 0) return fail("the clamp does not read joint jointCount - 1", count);
    return calls + 2;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    const uint32_t counts[] = { 0u, 1u, 2u, 97u, 1023u, 1024u, 1025u, 4099u };
    const uint32_t jointCounts[] = { 0u, 1u, 5u, 64u };
    int calls = 0;
    for (uint32_t n : counts)
        for (uint32_t j : jointCounts)
            for (uint32_t t = 0; t <= 3; t += 3)
                for (int mode = 0; mode < 3; ++mode) {
                    const int r = run(n, j, t, mode);
                    if (r < 0) return 1;
                    calls += r;
                }
    const uint32_t sizes[][2] = { { 1u, 1u }, { 97u, 5u }, { 1025u, 64u } };
    for (const auto& s : sizes)
        for (uint16_t index : { (uint16_t)s[1], (uint16_t)65535 }) {
            const int r = run_out_of_range(s[0], s[1], index);
            if (r < 0) return 1;
            calls += r;
        }
    (void)make_view; (void)kSizes;
    std::printf("skin_asan: %d calls, no report\n", calls);
    return 0;
}

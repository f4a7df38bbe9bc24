// deform_asan.cpp -- driver of the sanitizer build of the vertex quantiser's host side (`make deform_asan`: AddressSanitizer + UBSan, CPU
// only). Runs pt_deform.h through quantize_vertices_host over exactly sized heap arrays: random vertices, then hostile ones with every
// value of the table (NaN, inf, huge, denormal ...) in every one of the twelve fields, counts 0, 1 and odd ones around the chunk size,
// nthreads below, at and far above the count. Checks what can be said without a second implementation: positions are copied bit for
// bit, the unused bits of the packed words stay clear, the finiteness answer is right, and the result does not depend on nthreads. Any
// out-of-bounds access or other report ends the program with a non-zero status.   usage: deform_asan [seed]
#include "asan_common.h"
#include "pt_deform.h"

namespace hrt {
bool quantize_vertices_host(const HrptVertexFloat* in, uint32_t count, HrptVertexQuantized* out, int nthreads);
}

static int run(uint32_t count, bool hostile)
{
    std::vector<HrptVertexFloat> in(count);
    bool finite = true;
    for (uint32_t i = 0; i < count; ++i) {
        float* f = reinterpret_cast<float*>(&in[i]);        // a record is twelve contiguous floats
        for (int k = 0; k < 12; ++k) f[k] = 3.0f * rnd() - 1.5f;
        in[i].uv[0] = 70000.0f * (rnd() - 0.5f);
        in[i].tangent[3] = rnd() < 0.5f ? 1.0f : -1.0f;
        if (hostile) f[i % 12] = kBad[(i / 12) % 8];        // every value of the table reaches every field from count 96 on
        if (hostile && rnd() < 0.1f) f[(int)(rnd() * 11.999f)] = kBad[(int)(rnd() * 7.999f)];
        for (int k = 0; k < 3; ++k) if (!std::isfinite(in[i].pos[k])) finite = false;
    }
    std::vector<HrptVertexQuantized> ref(count), out(count);
    const bool refFinite = hrt::quantize_vertices_host(in.data(), count, ref.data(), 1);
    if (refFinite != finite) { std::fprintf(stderr, "deform_asan: wrong finiteness answer at count %u\n", count); return -1; }
    for (uint32_t i = 0; i < count; ++i) {
        if (std::memcmp(ref[i].m_Pos, in[i].pos, 12) != 0) { std::fprintf(stderr, "deform_asan: position %u not copied\n", i); return -1; }
        if ((ref[i].m_Normal & 0x80000000u) || (ref[i].m_Tangent >> 16)) { std::fprintf(stderr, "deform_asan: stray bits in vertex %u\n", i); return -1; }
        for (int k = 0; k < 3; ++k)
            if (((ref[i].m_Normal >> (10 * k)) & 1023u) > 1022u) { std::fprintf(stderr, "deform_asan: normal field of vertex %u out of range\n", i); return -1; }
        if ((ref[i].m_Tangent & 255u) > 254u || ((ref[i].m_Tangent >> 8) & 255u) > 254u) { std::fprintf(stderr, "deform_asan: tangent field of vertex %u out of range\n", i); return -1; }
    }
    int calls = 1;
    const int threads[5] = { 2, 3, 7, 64, (int)count + 5 };
    for (int t : threads) {
        if (count) std::memset(out.data(), 0xA5, out.size() * sizeof(HrptVertexQuantized));
        const bool f = hrt::quantize_vertices_host(in.data(), count, out.data(), t);
        ++calls;
        if (f != finite || (count && std::memcmp(out.data(), ref.data(), (size_t)count * sizeof(HrptVertexQuantized)) != 0)) {
            std::fprintf(stderr, "deform_asan: result depends on nthreads (%d) at count %u\n", t, count);
            return -1;
        }
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    const uint32_t counts[] = { 0u, 1u, 2u, 97u, 1023u, 1024u, 1025u, 4099u };
    int calls = 0;
    for (uint32_t n : counts)
        for (int hostile = 0; hostile < 2; ++hostile) {
            const int r = run(n, hostile != 0);
            if (r < 0) return 1;
            calls += r;
        }
    (void)make_view; (void)kSizes;
    std::printf("deform_asan: %d calls, no report\n", calls);
    return 0;
}

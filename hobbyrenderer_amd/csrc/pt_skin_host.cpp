// pt_skin_host.cpp -- the host-thread executor of the vertex producer (hrpt_skin_vertices_host): pt_skin.h's skin_vertex over chunks of the
// array. Plain C++ with no HIP call, so that the sanitizer program (skin_asan.cpp, `make skin_asan`) builds it with g++ as it is.
#include "pt_skin.h"
#include "pt_host_rows.h"

namespace hrt {

// out[i] = skin_vertex(args, i) for i < args.count, every pointer of args in host memory. Joint indices are validated before anything is
// written: with one >= jointCount the answer is skin::kJointOutOfRange and `out` is untouched. Otherwise 0, or skin::kPositionNotFinite
// when some output position is not finite (out is then written like any other). A vertex writes only its own record, so the result does
// not depend on nthreads. Chunks of 1 024 vertices are dealt to the threads like rows of an image.
uint32_t skin_vertices_host(const HrptSkinArgs& a, HrptVertexFloat* out, int nthreads)
{
    constexpr uint32_t kChunk = 1024;
    const int chunks = (int)(a.count / kChunk + (a.count % kChunk != 0u));
    std::vector<uint8_t> status((size_t)chunks, 0);
    auto range = [&](int c, uint32_t& first, uint32_t& last) { first = (uint32_t)c * kChunk; last = a.count - first < kChunk ? a.count : first + kChunk; };
    if (a.joints) {
        over_rows(chunks, nthreads, [&](int c) {
            uint32_t first, last;
            range(c, first, last);
            for (size_t k = 4 * (size_t)first; k < 4 * (size_t)last; ++k)
                if (a.joints[k] >= a.jointCount) status[(size_t)c] = (uint8_t)skin::kJointOutOfRange;
        });
        for (uint8_t s : status) if (s) return skin::kJointOutOfRange;
    }
    over_rows(chunks, nthreads, [&](int c) {
        uint32_t first, last;
        range(c, first, last);
        for (uint32_t i = first; i < last; ++i) status[(size_t)c] |= (uint8_t)skin::skin_vertex(a, i, out[i]);
    });
    uint32_t all = 0;
    for (uint8_t s : status) all |= s;
    return all;
}

} // namespace hrt

// pt_deform_host.cpp -- the host-thread executor of the vertex quantiser (hrpt_quantize_vertices_host): pt_deform.h's quantize_vertex over
// chunks of the array. Plain C++ with no HIP call, so that the sanitizer program (deform_asan.cpp, `make deform_asan`) builds it with
// g++ as it is.
#include "pt_deform.h"
#include "pt_host_rows.h"

namespace hrt {

// out[i] = quantize_vertex(in[i]) for i < count; returns whether every position is finite. A vertex writes only its own record, so the
// result does not depend on nthreads. Chunks of 1 024 vertices are dealt to the threads like rows of an image.
bool quantize_vertices_host(const HrptVertexFloat* in, uint32_t count, HrptVertexQuantized* out, int nthreads)
{
    constexpr uint32_t kChunk = 1024;
    const int chunks = (int)((count + (kChunk - 1)) / kChunk);
    std::vector<uint8_t> bad((size_t)chunks, 0);
    over_rows(chunks, nthreads, [&](int c) {
        const uint32_t first = (uint32_t)c * kChunk, last = count - first < kChunk ? count : first + kChunk;
        for (uint32_t i = first; i < last; ++i) {
            if (!deform::position_finite(in[i].pos)) bad[(size_t)c] = 1;
            out[i] = deform::quantize_vertex(in[i]);
        }
    });
    for (uint8_t b : bad) if (b) return false;
    return true;
}

} // namespace hrt

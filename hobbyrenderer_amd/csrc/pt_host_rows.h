// pt_host_rows.h -- the row loop of the stages' host executors (bloom_host, temporal_host, denoise_host, demodulate_host, compose_host):
// rows interleaved over host threads, and the four-float store of a texel. Plain C++ with no HIP call, so that the sanitizer programs build
// it with g++ as it is.
#pragma once

#include <thread>
#include <vector>

#include "pt_image.h"

namespace hrt {

// row(y) for every y in [0, H): thread t takes rows t, t + nthreads, ... A row writes only its own texels, so the result does not depend on
// nthreads. std::thread may throw std::system_error, the vector std::bad_alloc; the C entry points turn both into status codes.
template <class Row> void over_rows(int H, int nthreads, Row row)
{
    if (nthreads > H) nthreads = H;
    if (nthreads <= 1) { for (int y = 0; y < H; ++y) row(y); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([=] { for (int y = t; y < H; y += nthreads) row(y); });
    for (auto& x : th) x.join();
}

inline void store4(float* p, img::T4 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }

} // namespace hrt

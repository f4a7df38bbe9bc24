// pt_temporal_host.cpp -- the host-thread executor of the temporal stage (hrpt_temporal_host): pt_temporal.h's per-pixel function over rows.
// Plain C++ with no HIP call, so that the sanitizer program (temporal_asan.cpp, `make temporal_asan`) builds it with g++ as it is.
#include <thread>
#include <vector>

#include "pt_temporal.h"

namespace hrt {

// colorOut may be color (a pixel reads only its own colour texel and reads it before writing); historyOut must not be historyIn.
void temporal_host(const HrptTemporalImages& img, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                   const HrptPlanarViewConstants& prevView, const HrptTemporalParams& params, int nthreads)
{
    const temporal::Args a = temporal::make_args(view, prevView, params.blend, params.flags, (int)width, (int)height);
    const int W = (int)width, H = (int)height;
    auto row = [&](int y) {
        for (int x = 0; x < W; ++x) {
            temporal::T4 hist, col;
            temporal::pixel(a, img.color, img.motion, img.depth, img.normal, img.historyIn, x, y, &hist, &col);
            float* h = img.historyOut + ((size_t)y * W + x) * 4; float* c = img.colorOut + ((size_t)y * W + x) * 4;
            h[0] = hist.x; h[1] = hist.y; h[2] = hist.z; h[3] = hist.w;
            c[0] = col.x; c[1] = col.y; c[2] = col.z; c[3] = col.w;
        }
    };
    if (nthreads > H) nthreads = H;
    if (nthreads <= 1) { for (int y = 0; y < H; ++y) row(y); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([=] { for (int y = t; y < H; y += nthreads) row(y); });
    for (auto& x : th) x.join();
}

} // namespace hrt

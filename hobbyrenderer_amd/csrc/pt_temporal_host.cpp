// pt_temporal_host.cpp -- the host-thread executor of the temporal stage (hrpt_temporal_host): pt_temporal.h's per-pixel function over rows,
// and the parameter rules. Plain C++ with no HIP call, so that the sanitizer program (temporal_asan.cpp, `make temporal_asan`) builds it with
// g++ as it is.
#include "pt_host_rows.h"
#include "pt_temporal.h"

namespace hrt {

bool temporal_params_valid(const HrptTemporalParams& p)
{
    return p.blend >= 0.0f && p.blend <= 1.0f && (p.flags & ~(HRPT_TEMPORAL_LINEAR | HRPT_TEMPORAL_RESET)) == 0u && p.reserved[0] == 0u && p.reserved[1] == 0u;
}

// colorOut may be color (a pixel reads only its own colour texel and reads it before writing); historyOut must not be historyIn.
void temporal_host(const HrptTemporalImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                   const HrptPlanarViewConstants& prevView, const HrptTemporalParams& params, int nthreads)
{
    const temporal::Args a = temporal::make_args(view, prevView, params.blend, params.flags, (int)width, (int)height);
    const int W = (int)width, H = (int)height;
    over_rows(H, nthreads, [&](int y) {
        for (int x = 0; x < W; ++x) {
            img::T4 hist, col;
            temporal::pixel(a, images.color, images.motion, images.depth, images.normal, images.historyIn, x, y, &hist, &col);
            const size_t i = ((size_t)y * W + x) * 4;
            store4(images.historyOut + i, hist);
            store4(images.colorOut + i, col);
        }
    });
}

} // namespace hrt

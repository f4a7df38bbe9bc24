// pt_upscale_host.cpp -- the host-thread executor of the upscale stage (hrpt_upscale_host): pt_upscale.h's per-pixel function over the rows
// of the display image, and the parameter rules. Plain C++ with no HIP call, so that the sanitizer program (upscale_asan.cpp,
// `make upscale_asan`) builds it with g++ as it is.
#include "pt_host_rows.h"
#include "pt_upscale.h"

namespace hrt {

// !(x >= lo && x <= hi) rejects a NaN as well
bool upscale_params_valid(const HrptUpscaleParams& p)
{
    for (float j : p.jitter) if (!(j >= -0.5f && j <= 0.5f)) return false;
    return p.kernel > 0.0f && p.kernel <= 16.0f && p.maxHistory >= 0.0f && p.maxHistory <= 3.402823466e38f &&
           (p.flags & ~(HRPT_UPSCALE_NO_CLAMP | HRPT_UPSCALE_RESET)) == 0u && p.reserved[0] == 0u && p.reserved[1] == 0u && p.reserved[2] == 0u;
}

// w <= W <= 4w and h <= H <= 4h (every size already known to be in 1..65535)
bool upscale_ratio_ok(uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight)
{
    return width <= displayWidth && displayWidth <= 4u * width && height <= displayHeight && displayHeight <= 4u * height;
}

// historyOut must not be historyIn, and colorOut neither of them: a pixel's history taps are other pixels' texels.
void upscale_host(const HrptUpscaleImages& images, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                  const HrptPlanarViewConstants& view, const HrptPlanarViewConstants& prevView, const HrptUpscaleParams& params, int nthreads)
{
    const upscale::Args a = upscale::make_args(view, prevView, params, (int)width, (int)height, (int)displayWidth, (int)displayHeight);
    const upscale::ImageTaps taps = { images.color, images.depth, (int)width };
    const int W = (int)displayWidth, H = (int)displayHeight;
    over_rows(H, nthreads, [&](int y) {
        for (int x = 0; x < W; ++x) {
            img::T4 hist, col;
            upscale::pixel(a, taps, images.motion, images.historyIn, x, y, &hist, &col);
            const size_t i = ((size_t)y * W + x) * 4;
            store4(images.historyOut + i, hist);
            store4(images.colorOut + i, col);
        }
    });
}

} // namespace hrt

// pt_denoise.hip -- the gfx950 kernel of the denoise stage (hrpt_denoise / hrpt_denoise_device): one pass of the edge-stopping Poisson
// filter over the temporally accumulated radiance. The arithmetic is pt_denoise.h (shared with hrpt_denoise_host); this file holds the
// kernel and its launcher.
//
// One thread per pixel in 32 x 8 tiles, like temporal_accumulate: a wave covers 32 x 2 pixels, so the four per-pixel float4 reads (input,
// depth, normal, geo-normal) and the one or two float4 writes are 512-byte row pieces. The eight taps are per-lane gathers of three float4
// each: every lane has its own disk rotation, so a wave's taps fall anywhere within +-4 * radius texels of its pixels; they are served by
// the caches. No LDS: with a per-lane rotation and a radius that doubles per iteration a tile has no fixed footprint worth staging. The
// compiler unrolls the eight taps (35 KB of code, the disk offsets as immediates). DESIGN.md section 18 has the register counts.
#include "pt_denoise.h"
#include "pt_image_kernel.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
using img::kTileX;
using img::kTileY;

// color and colorOut may be the same image (no __restrict__ on them): a thread reads its own colour texel before it writes it. Both are
// null together. output aliases no input.
__global__ __launch_bounds__(kTileX * kTileY) void denoise_poisson(denoise::Args a, const float* __restrict__ input, const float* __restrict__ depth,
                                                                   const float* __restrict__ normal, const float* __restrict__ geoNormal,
                                                                   const float* __restrict__ noise, float4* __restrict__ output,
                                                                   const float4* color, float4* colorOut)
{
    int px, py;
    if (!img::stage_pixel(a.view.w, a.view.h, &px, &py)) return;
    const img::T4 out = denoise::pixel(a, input, depth, normal, geoNormal, noise, px, py);
    const size_t idx = img::stage_index(a.view.w, px, py);
    img::st4(output, idx, out);
    if (colorOut) img::st4(colorOut, idx, img::t4(out.x, out.y, out.z, color[idx].w));
}
} // namespace

hipError_t launch_denoise(const HrptDenoiseImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                          const HrptDenoiseParams& params, float radius, uint32_t frame, hipStream_t stream)
{
    const denoise::Args a = denoise::make_args(view, params, radius, frame, (int)width, (int)height);
    hipLaunchKernelGGL(denoise_poisson, img::stage_grid(width, height), img::stage_block(), 0, stream, a, images.input, images.depth,
                       images.normal, images.geoNormal, images.noise, reinterpret_cast<float4*>(images.output),
                       reinterpret_cast<const float4*>(images.color), reinterpret_cast<float4*>(images.colorOut));
    return hipGetLastError();
}

} // namespace hrt

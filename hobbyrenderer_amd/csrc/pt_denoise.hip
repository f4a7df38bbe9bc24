// pt_denoise.hip -- the gfx950 kernel of the denoise stage (hrpt_denoise / hrpt_denoise_device): one pass of the edge-stopping Poisson
// filter over the temporally accumulated radiance. The arithmetic is pt_denoise.h (shared with hrpt_denoise_host); this file holds the
// kernel and its launcher.
//
// One thread per pixel in 32 x 8 tiles, like temporal_accumulate: a wave covers 32 x 2 pixels, so the four per-pixel float4 reads (input,
// depth, normal, geo-normal) and the one or two float4 writes are 512-byte row pieces. The eight taps are per-lane gathers of three float4
// each: every lane has its own disk rotation, so a wave's taps fall anywhere within +-4 * radius texels of its pixels; they are served by
// the caches. No LDS: with a per-lane rotation and a radius that doubles per iteration a tile has no fixed footprint worth staging. The
// compiler unrolls the eight taps (35 KB of code, the disk offsets as immediates). DESIGN.md section 18 has the register counts.
#include <hip/hip_runtime.h>

#include "pt_denoise.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
constexpr int kTileX = 32, kTileY = 8;

// color and colorOut may be the same image (no __restrict__ on them): a thread reads its own colour texel before it writes it. Both are
// null together. output aliases no input.
__global__ __launch_bounds__(kTileX * kTileY) void denoise_poisson(denoise::Args a, const float* __restrict__ input, const float* __restrict__ depth,
                                                                   const float* __restrict__ normal, const float* __restrict__ geoNormal,
                                                                   const float* __restrict__ noise, float4* __restrict__ output,
                                                                   const float4* color, float4* colorOut)
{
    const int px = blockIdx.x * kTileX + threadIdx.x, py = blockIdx.y * kTileY + threadIdx.y;
    if (px >= a.view.w || py >= a.view.h) return;
    const temporal::T4 out = denoise::pixel(a, input, depth, normal, geoNormal, noise, px, py);
    const size_t idx = (size_t)py * (size_t)a.view.w + (size_t)px;
    output[idx] = make_float4(out.x, out.y, out.z, out.w);
    if (colorOut) colorOut[idx] = make_float4(out.x, out.y, out.z, color[idx].w);
}
} // namespace

hipError_t launch_denoise(const HrptDenoiseImages& img, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                          const HrptDenoiseParams& params, float radius, uint32_t frame, hipStream_t stream)
{
    const denoise::Args a = denoise::make_args(view, params, radius, frame, (int)width, (int)height);
    const dim3 grid((width + kTileX - 1) / kTileX, (height + kTileY - 1) / kTileY), block(kTileX, kTileY);
    hipLaunchKernelGGL(denoise_poisson, grid, block, 0, stream, a, img.input, img.depth, img.normal, img.geoNormal, img.noise,
                       reinterpret_cast<float4*>(img.output), reinterpret_cast<const float4*>(img.color), reinterpret_cast<float4*>(img.colorOut));
    return hipGetLastError();
}

} // namespace hrt

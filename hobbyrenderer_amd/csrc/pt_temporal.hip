// pt_temporal.hip -- the gfx950 kernel of the temporal stage (hrpt_temporal_accumulate / hrpt_temporal_device): reprojected accumulation of
// the path tracer's radiance across frames. The arithmetic is pt_temporal.h (shared with hrpt_temporal_host); this file holds the kernel
// and its launcher.
//
// One thread per pixel in 32 x 8 tiles, like the bloom kernels: a wave covers 32 x 2 pixels, so the five per-pixel float4 reads (colour,
// depth, normal, motion, and the validation's two point samples where motion is small) and the two float4 writes are 512-byte row pieces.
// The history is read in the plain form: the 13 bilinear taps of SampleTextureCatmullRom, 52 float4 loads per pixel, all inside a
// 4 x 4 texel footprint (give or take the texel the uv round trip may move a floor by), which neighbouring lanes share -- they are served
// by the vector cache, not by HBM. No LDS: the footprint of a tile follows the motion vectors, which differ per pixel.
#include "pt_image_kernel.h"
#include "pt_kernels.h"
#include "pt_temporal.h"

namespace hrt {

namespace {
using img::kTileX;
using img::kTileY;

// color and colorOut may be the same image (no __restrict__ on them): a thread reads its own colour texel before it writes it.
__global__ __launch_bounds__(kTileX * kTileY) void temporal_accumulate(temporal::Args a, const float* color, const float* __restrict__ motion,
                                                                       const float* __restrict__ depth, const float* __restrict__ normal,
                                                                       const float* __restrict__ historyIn, float4* __restrict__ historyOut,
                                                                       float4* colorOut)
{
    int px, py;
    if (!img::stage_pixel(a.view.w, a.view.h, &px, &py)) return;
    img::T4 hist, col;
    temporal::pixel(a, color, motion, depth, normal, historyIn, px, py, &hist, &col);
    const size_t idx = img::stage_index(a.view.w, px, py);
    img::st4(historyOut, idx, hist);
    img::st4(colorOut, idx, col);
}
} // namespace

hipError_t launch_temporal(const HrptTemporalImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                           const HrptPlanarViewConstants& prevView, const HrptTemporalParams& params, hipStream_t stream)
{
    const temporal::Args a = temporal::make_args(view, prevView, params.blend, params.flags, (int)width, (int)height);
    hipLaunchKernelGGL(temporal_accumulate, img::stage_grid(width, height), img::stage_block(), 0, stream, a, images.color, images.motion,
                       images.depth, images.normal, images.historyIn, reinterpret_cast<float4*>(images.historyOut),
                       reinterpret_cast<float4*>(images.colorOut));
    return hipGetLastError();
}

} // namespace hrt

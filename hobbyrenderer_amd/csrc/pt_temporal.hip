// pt_temporal.hip -- the gfx950 kernel of the temporal stage (hrpt_temporal_accumulate / hrpt_temporal_device): reprojected accumulation of
// the path tracer's radiance across frames. The arithmetic is pt_temporal.h (shared with hrpt_temporal_host); this file holds the kernel
// and its launcher.
//
// One thread per pixel in 32 x 8 tiles, like the bloom kernels: a wave covers 32 x 2 pixels, so the five per-pixel float4 reads (colour,
// depth, normal, motion, and the validation's two point samples where motion is small) and the two float4 writes are 512-byte row pieces.
// The history is read in the plain form: the 13 bilinear taps of SampleTextureCatmullRom, 52 float4 loads per pixel, all inside a
// 4 x 4 texel footprint (give or take the texel the uv round trip may move a floor by), which neighbouring lanes share -- they are served
// by the vector cache, not by HBM. No LDS: the footprint of a tile follows the motion vectors, which differ per pixel.
#include <hip/hip_runtime.h>

#include "pt_temporal.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
constexpr int kTileX = 32, kTileY = 8;

// color and colorOut may be the same image (no __restrict__ on them): a thread reads its own colour texel before it writes it.
__global__ __launch_bounds__(kTileX * kTileY) void temporal_accumulate(temporal::Args a, const float* color, const float* __restrict__ motion,
                                                                       const float* __restrict__ depth, const float* __restrict__ normal,
                                                                       const float* __restrict__ historyIn, float4* __restrict__ historyOut,
                                                                       float4* colorOut)
{
    const int px = blockIdx.x * kTileX + threadIdx.x, py = blockIdx.y * kTileY + threadIdx.y;
    if (px >= a.w || py >= a.h) return;
    temporal::T4 hist, col;
    temporal::pixel(a, color, motion, depth, normal, historyIn, px, py, &hist, &col);
    const size_t idx = (size_t)py * (size_t)a.w + (size_t)px;
    historyOut[idx] = make_float4(hist.x, hist.y, hist.z, hist.w);
    colorOut[idx] = make_float4(col.x, col.y, col.z, col.w);
}
} // namespace

bool temporal_params_valid(const HrptTemporalParams& p)
{
    return p.blend >= 0.0f && p.blend <= 1.0f && (p.flags & ~(HRPT_TEMPORAL_LINEAR | HRPT_TEMPORAL_RESET)) == 0u && p.reserved[0] == 0u && p.reserved[1] == 0u;
}

hipError_t launch_temporal(const HrptTemporalImages& img, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                           const HrptPlanarViewConstants& prevView, const HrptTemporalParams& params, hipStream_t stream)
{
    const temporal::Args a = temporal::make_args(view, prevView, params.blend, params.flags, (int)width, (int)height);
    const dim3 grid((width + kTileX - 1) / kTileX, (height + kTileY - 1) / kTileY), block(kTileX, kTileY);
    hipLaunchKernelGGL(temporal_accumulate, grid, block, 0, stream, a, img.color, img.motion, img.depth, img.normal, img.historyIn,
                       reinterpret_cast<float4*>(img.historyOut), reinterpret_cast<float4*>(img.colorOut));
    return hipGetLastError();
}

} // namespace hrt

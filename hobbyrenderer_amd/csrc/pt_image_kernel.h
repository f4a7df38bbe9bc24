// pt_image_kernel.h -- what the one-thread-per-pixel kernels of the screen-space stages share (pt_bloom.hip, pt_temporal.hip, pt_denoise.hip,
// pt_modulation.hip): the 32 x 8 tile, so that a wave covers 32 x 2 pixels and its float4 accesses are 512-byte row pieces, the launch
// shape, the pixel-of-thread prologue and the float4 <-> T4 conversions. All forceinline: a kernel compiles to what it did with these
// lines written out in it.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_image.h"

namespace hrt {
namespace img {

constexpr int kTileX = 32, kTileY = 8;
inline dim3 stage_block() { return dim3(kTileX, kTileY); }
inline dim3 stage_grid(uint32_t width, uint32_t height) { return dim3((width + kTileX - 1) / kTileX, (height + kTileY - 1) / kTileY); }
// The pixel of this thread in a w x h image; false for the threads of a partial tile that lie outside the image.
__device__ __forceinline__ bool stage_pixel(int w, int h, int* px, int* py)
{
    *px = blockIdx.x * kTileX + threadIdx.x; *py = blockIdx.y * kTileY + threadIdx.y;
    return *px < w && *py < h;
}
// Its texel. Computed where it is used: held across a 13-tap downsample it cost bloom_downsample and bloom_upsample a register each.
__device__ __forceinline__ size_t stage_index(int w, int px, int py) { return (size_t)py * (size_t)w + (size_t)px; }
__device__ __forceinline__ T4 ld4(const float4* image, size_t idx) { const float4 v = image[idx]; return t4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void st4(float4* image, size_t idx, T4 v) { image[idx] = make_float4(v.x, v.y, v.z, v.w); }

} // namespace img
} // namespace hrt

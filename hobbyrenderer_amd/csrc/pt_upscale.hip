// pt_upscale.hip -- the gfx950 kernels of the upscale stage (hrpt_upscale / hrpt_upscale_device): temporal upscaling of a jittered render-size
// frame into a display-size history. The arithmetic is pt_upscale.h (shared with hrpt_upscale_host); this file holds the kernels and their
// launcher.
//
// One thread per DISPLAY pixel in 32 x 8 tiles, like the other image stages. The history is read as in temporal_accumulate: the 13 bilinear
// taps of SampleTextureCatmullRom through the vector cache, which is what bounds the kernel; the motion texel of the chosen tap is one
// global read per pixel. The nine current-frame taps come in two forms with the same bits:
//   * upscale_resolve (the default): plain global gathers. Neighbouring pixels share their taps -- all of them at a scale above 1 -- so the
//     vector cache serves them; measured 1.3 to 1.8 % faster than the staged form at 1x, 1.5x and 2x.
//   * upscale_resolve_staged (HRPT_UPSCALE_STAGED=1 at hrpt_create; kept for A/B measurements): unlike the history's, the current-frame
//     footprint of a tile does not follow the motion vectors -- it is the render texels under the tile plus a one-texel halo. The base texel
//     bi(X) = floor(((X + 0.5) * rx) - jx) never decreases with X, and across the 31 pixel steps of a tile it grows by at most 32 (31 * rx
//     <= 31 plus less than one texel of rounding), 8 across the 7 steps of its rows; with the halo that is a window of at most 35 x 11
//     texels whose origin is the first pixel's base texel minus one (19 x 7 at 2x). The workgroup stages that window once in LDS -- colour
//     as float4 and one float per texel holding the depth key (view depth, +inf for a miss): 36 * 12 * 20 B = 8640 B -- and serves all nine
//     taps of every pixel from it. Window texels outside the image are staged from the clamped texel and never read: a tap's texel is
//     clamped before it is looked up.
#include "pt_image_kernel.h"
#include "pt_kernels.h"
#include "pt_upscale.h"

namespace hrt {

namespace {
using img::kTileX;
using img::kTileY;

constexpr int kWinX = kTileX + 4, kWinY = kTileY + 4;      // 36 x 12 >= the 35 x 11 texels a tile can touch

// The staged window as a tap source of upscale::pixel: texel (ti, tj) of the image lies at (ti - ox, tj - oy).
struct WindowTaps { const float4* color; const float* key; int ox, oy; };
HRT_FN img::T4 tap_color(const WindowTaps& s, int ti, int tj)
{
    const float4 v = s.color[(tj - s.oy) * kWinX + (ti - s.ox)];
    return img::t4(v.x, v.y, v.z, v.w);
}
HRT_FN float tap_key(const WindowTaps& s, int ti, int tj) { return s.key[(tj - s.oy) * kWinX + (ti - s.ox)]; }

// The pixel of this thread through `taps`; threads of a partial tile outside the image do nothing.
template <class Taps>
__device__ __forceinline__ void resolve_pixel(const upscale::Args& a, const Taps& taps, const float* motion, const float* historyIn, float4* historyOut, float4* colorOut)
{
    int X, Y;
    if (!img::stage_pixel(a.W, a.H, &X, &Y)) return;
    img::T4 hist, col;
    upscale::pixel(a, taps, motion, historyIn, X, Y, &hist, &col);
    const size_t idx = img::stage_index(a.W, X, Y);
    img::st4(historyOut, idx, hist);
    img::st4(colorOut, idx, col);
}

__global__ __launch_bounds__(kTileX * kTileY) void upscale_resolve(upscale::Args a, const float* __restrict__ color, const float* __restrict__ depth,
                                                                   const float* __restrict__ motion, const float* __restrict__ historyIn,
                                                                   float4* __restrict__ historyOut, float4* __restrict__ colorOut)
{
    const upscale::ImageTaps taps = { color, depth, a.w };
    resolve_pixel(a, taps, motion, historyIn, historyOut, colorOut);
}

__global__ __launch_bounds__(kTileX * kTileY) void upscale_resolve_staged(upscale::Args a, const float* __restrict__ color, const float* __restrict__ depth,
                                                                          const float* __restrict__ motion, const float* __restrict__ historyIn,
                                                                          float4* __restrict__ historyOut, float4* __restrict__ colorOut)
{
    __shared__ float4 sColor[kWinX * kWinY];
    __shared__ float sKey[kWinX * kWinY];
    // the window's origin: the base texel of the tile's first pixel (always inside the image) minus the halo; -1 at the image's edge
    const int X0 = blockIdx.x * kTileX, Y0 = blockIdx.y * kTileY;
    const int ox = upscale::base_texel(((float)X0 + 0.5f) * a.rx, a.jx, a.w) - 1, oy = upscale::base_texel(((float)Y0 + 0.5f) * a.ry, a.jy, a.h) - 1;
    // ... and its extent: up to the base texel of the tile's last pixel inside the image plus the halo
    const int X1 = min(X0 + kTileX, a.W) - 1, Y1 = min(Y0 + kTileY, a.H) - 1;
    const int nx = upscale::base_texel(((float)X1 + 0.5f) * a.rx, a.jx, a.w) - ox + 2, ny = upscale::base_texel(((float)Y1 + 0.5f) * a.ry, a.jy, a.h) - oy + 2;
    for (int k = threadIdx.y * kTileX + threadIdx.x; k < nx * ny; k += kTileX * kTileY) {
        const int lx = k % nx, ly = k / nx;
        const int ti = upscale::tap_texel(ox, lx, a.w), tj = upscale::tap_texel(oy, ly, a.h);
        const size_t idx = img::stage_index(a.w, ti, tj);
        sColor[ly * kWinX + lx] = reinterpret_cast<const float4*>(color)[idx];
        const float2 d = reinterpret_cast<const float2*>(depth)[idx * 2];
        sKey[ly * kWinX + lx] = upscale::depth_key(d.x, d.y);
    }
    __syncthreads();
    const WindowTaps taps = { sColor, sKey, ox, oy };
    resolve_pixel(a, taps, motion, historyIn, historyOut, colorOut);
}
} // namespace

hipError_t launch_upscale(const HrptUpscaleImages& images, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                          const HrptPlanarViewConstants& view, const HrptPlanarViewConstants& prevView, const HrptUpscaleParams& params, bool staged,
                          hipStream_t stream)
{
    const upscale::Args a = upscale::make_args(view, prevView, params, (int)width, (int)height, (int)displayWidth, (int)displayHeight);
    hipLaunchKernelGGL(staged ? upscale_resolve_staged : upscale_resolve, img::stage_grid(displayWidth, displayHeight), img::stage_block(), 0, stream, a,
                       images.color, images.depth, images.motion, images.historyIn, reinterpret_cast<float4*>(images.historyOut),
                       reinterpret_cast<float4*>(images.colorOut));
    return hipGetLastError();
}

} // namespace hrt

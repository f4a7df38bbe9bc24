// pt_modulation.hip -- the gfx950 kernels of the demodulate and compose stages (hrpt_demodulate / hrpt_compose and their _device calls):
// the first-hit BRDF factor divided out of the colour image in front of the temporal and spatial filters, and multiplied back in behind
// them. The arithmetic is pt_modulation.h (shared with the host executors); this file holds the kernels and their launchers.
//
// One thread per pixel in 32 x 8 tiles, like temporal_accumulate and denoise_poisson: a wave covers 32 x 2 pixels, so every read and write
// of a wave falls in 512-byte row pieces of float4 texels (the compiler loads only the components used: dwordx3 for albedo and emissive,
// single dwords for depth.x, depth.y and the metallic). No LDS, no gathers: a pixel touches only its own texels. Bytes per pixel:
// demodulate reads six float4 (colour, albedo, normal, geo-normal, depth, emissive) and writes two (colour, modulation) = 128 B; compose
// reads three (colour, modulation, emissive) and writes one = 64 B. Storing Mf is what keeps compose at half of demodulate: it reads one
// image instead of the four planes the factor is computed from, and does none of its arithmetic. DESIGN.md section 20 has the register
// counts and the times.
#include "pt_image_kernel.h"
#include "pt_kernels.h"
#include "pt_modulation.h"

namespace hrt {

namespace {
using img::kTileX;
using img::kTileY;
using img::ld4;
using img::st4;

__device__ __forceinline__ img::T3 emissive_at(const float4* emissive, size_t idx)
{
    if (!emissive) return img::t3(0.0f, 0.0f, 0.0f);
    const float4 e = emissive[idx];
    return img::t3(e.x, e.y, e.z);
}

// color and colorOut may be the same image (no __restrict__ on them): a thread reads its own colour texel before it writes it.
// modulationOut aliases nothing. emissive may be null.
__global__ __launch_bounds__(kTileX * kTileY) void modulation_demodulate(modulation::Args a, const float4* color, const float* __restrict__ albedo,
                                                                         const float* __restrict__ normal, const float* __restrict__ geoNormal,
                                                                         const float* __restrict__ depth, const float4* __restrict__ emissive,
                                                                         float4* colorOut, float4* __restrict__ modulationOut)
{
    int px, py;
    if (!img::stage_pixel(a.view.w, a.view.h, &px, &py)) return;
    const size_t idx = img::stage_index(a.view.w, px, py);
    const img::T4 M = modulation::modulation_pixel(a, albedo, normal, geoNormal, depth, px, py);
    const img::T4 out = modulation::demodulate_color(ld4(color, idx), M, emissive_at(emissive, idx));
    st4(modulationOut, idx, M);
    st4(colorOut, idx, out);
}

__global__ __launch_bounds__(kTileX * kTileY) void modulation_compose(int w, int h, const float4* color, const float4* __restrict__ modulation,
                                                                      const float4* __restrict__ emissive, float4* colorOut)
{
    int px, py;
    if (!img::stage_pixel(w, h, &px, &py)) return;
    const size_t idx = img::stage_index(w, px, py);
    st4(colorOut, idx, modulation::compose_color(ld4(color, idx), ld4(modulation, idx), emissive_at(emissive, idx)));
}
} // namespace

hipError_t launch_demodulate(const HrptDemodulateImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                             const HrptModulationParams& params, hipStream_t stream)
{
    const modulation::Args a = modulation::make_args(view, params, (int)width, (int)height);
    hipLaunchKernelGGL(modulation_demodulate, img::stage_grid(width, height), img::stage_block(), 0, stream, a,
                       reinterpret_cast<const float4*>(images.color), images.albedo, images.normal, images.geoNormal, images.depth,
                       reinterpret_cast<const float4*>(images.emissive), reinterpret_cast<float4*>(images.colorOut),
                       reinterpret_cast<float4*>(images.modulationOut));
    return hipGetLastError();
}

hipError_t launch_compose(const HrptComposeImages& images, uint32_t width, uint32_t height, hipStream_t stream)
{
    hipLaunchKernelGGL(modulation_compose, img::stage_grid(width, height), img::stage_block(), 0, stream, (int)width, (int)height,
                       reinterpret_cast<const float4*>(images.color), reinterpret_cast<const float4*>(images.modulation),
                       reinterpret_cast<const float4*>(images.emissive), reinterpret_cast<float4*>(images.colorOut));
    return hipGetLastError();
}

} // namespace hrt

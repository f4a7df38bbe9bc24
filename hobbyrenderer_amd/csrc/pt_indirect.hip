// pt_indirect.hip -- the gfx950 kernels of traced indirect lighting (hrpt_indirect_lighting / hrpt_indirect_compose). The arithmetic is
// pt_indirect.h (shared with the host executors of pt_indirect_host.cpp). This file holds the three kernels and their launchers; the rays
// in between are traced by hrpt_trace_radiance with HRPT_RADIANCE_SECONDARY. Streaming kernels, no LDS, no scratch, no light records.
//
//   indirect_rays      32 x 8 tiles, one lane per pixel: the pixel's four texels once, then one 48-byte HrptRay per flagged lobe as three
//                      16-byte stores, diffuse at g = y * W + x, specular behind the diffuse records (a wave writes 64 consecutive records of
//                      one lobe: 3 KiB contiguous).
//   indirect_resolve   one lane per pixel: the radiance of the pixel's records, the specular weight re-evaluated from the planes and draws,
//                      one float4 store per plane; the plane of a lobe that is not flagged is zeroed.
//   indirect_compose   one lane per pixel: colour += (diffuse * albedo * (1 - metallic) + specular) * intensity at hits.
#include "pt_device.h"
#include "pt_indirect.h"
#include "pt_image_kernel.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
using namespace indirect;

__global__ __launch_bounds__(img::kTileX * img::kTileY) void indirect_rays(Frame f, const float4* __restrict__ albedo, const float4* __restrict__ normal,
                                                                         const float4* __restrict__ geoNormal, const float4* __restrict__ depth,
                                                                         float4* __restrict__ rays)
{
    int px, py;
    if (!img::stage_pixel(f.w, f.h, &px, &py)) return;
    const size_t idx = img::stage_index(f.w, px, py), WH = (size_t)f.w * (size_t)f.h;
    T4 rowsD[3], rowsS[3];
    pixel_rays(f, img::ld4(albedo, idx), img::ld4(normal, idx), geoNormal[idx].w, img::ld4(depth, idx), px, py, rowsD, rowsS);
    if (f.flags & HRPT_INDIRECT_DIFFUSE) {
        float4* rec = rays + idx * 3;
        img::st4(rec, 0, rowsD[0]); img::st4(rec, 1, rowsD[1]); img::st4(rec, 2, rowsD[2]);
    }
    if (f.flags & HRPT_INDIRECT_SPECULAR) {
        float4* rec = rays + (specular_base(f.flags, WH) + idx) * 3;
        img::st4(rec, 0, rowsS[0]); img::st4(rec, 1, rowsS[1]); img::st4(rec, 2, rowsS[2]);
    }
}

__global__ __launch_bounds__(img::kTileX * img::kTileY) void indirect_resolve(Frame f, const float4* __restrict__ albedo, const float4* __restrict__ normal,
                                                                            const float4* __restrict__ geoNormal, const float4* __restrict__ depth,
                                                                            const float4* __restrict__ radiance, float4* __restrict__ diffuseOut,
                                                                            float4* __restrict__ specularOut)
{
    int px, py;
    if (!img::stage_pixel(f.w, f.h, &px, &py)) return;
    const size_t idx = img::stage_index(f.w, px, py), WH = (size_t)f.w * (size_t)f.h;
    const T4 zero = t4(0.0f, 0.0f, 0.0f, 0.0f);
    const T4 D = img::ld4(depth, idx);
    if (diffuseOut) img::st4(diffuseOut, idx, (f.flags & HRPT_INDIRECT_DIFFUSE) ? resolve_diffuse(D, img::ld4(radiance, idx)) : zero);
    if (specularOut) {
        T4 out = zero;
        if (f.flags & HRPT_INDIRECT_SPECULAR)
            out = resolve_specular(f, img::ld4(albedo, idx), img::ld4(normal, idx), geoNormal[idx].w, D, px, py, img::ld4(radiance, specular_base(f.flags, WH) + idx));
        img::st4(specularOut, idx, out);
    }
}

__global__ __launch_bounds__(img::kTileX * img::kTileY) void indirect_compose(int w, int h, float intensity, const float4* __restrict__ albedo,
                                                                            const float4* __restrict__ geoNormal, const float4* __restrict__ depth,
                                                                            const float4* __restrict__ diffuse, const float4* __restrict__ specular,
                                                                            float4* __restrict__ color)
{
    int px, py;
    if (!img::stage_pixel(w, h, &px, &py)) return;
    const size_t idx = img::stage_index(w, px, py);
    const T4 D = img::ld4(depth, idx);
    if (D.x == img::kMissDepth) return;                                    // a miss passes through
    img::st4(color, idx, compose(intensity, img::ld4(color, idx), img::ld4(albedo, idx), geoNormal[idx].w, D, img::ld4(diffuse, idx), img::ld4(specular, idx)));
}
} // namespace

static const float4* c4(const float* p) { return reinterpret_cast<const float4*>(p); }

hipError_t launch_indirect_rays(const indirect::Frame& frame, const HrptIndirectImages& images, HrptRay* rays, hipStream_t stream)
{
    hipLaunchKernelGGL(indirect_rays, img::stage_grid((uint32_t)frame.w, (uint32_t)frame.h), img::stage_block(), 0, stream, frame, c4(images.albedo), c4(images.normal),
                       c4(images.geoNormal), c4(images.depth), reinterpret_cast<float4*>(rays));
    return hipGetLastError();
}

hipError_t launch_indirect_resolve(const indirect::Frame& frame, const HrptIndirectImages& images, const float4* radiance, hipStream_t stream)
{
    hipLaunchKernelGGL(indirect_resolve, img::stage_grid((uint32_t)frame.w, (uint32_t)frame.h), img::stage_block(), 0, stream, frame, c4(images.albedo), c4(images.normal),
                       c4(images.geoNormal), c4(images.depth), radiance, reinterpret_cast<float4*>(images.diffuse), reinterpret_cast<float4*>(images.specular));
    return hipGetLastError();
}

hipError_t launch_indirect_compose(const HrptIndirectImages& images, uint32_t width, uint32_t height, float intensity, hipStream_t stream)
{
    hipLaunchKernelGGL(indirect_compose, img::stage_grid(width, height), img::stage_block(), 0, stream, (int)width, (int)height, intensity, c4(images.albedo),
                       c4(images.geoNormal), c4(images.depth), c4(images.diffuse), c4(images.specular), reinterpret_cast<float4*>(images.colorInOut));
    return hipGetLastError();
}

} // namespace hrt

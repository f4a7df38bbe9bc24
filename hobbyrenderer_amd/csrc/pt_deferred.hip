// pt_deferred.hip -- the gfx950 kernels of deferred lighting (hrpt_deferred_lighting). The arithmetic is pt_deferred.h (shared with the host
// executors of pt_deferred_host.cpp); the atmosphere terms are pt_atmosphere.h's, as the path tracer calls them. This file holds the two
// kernels and their launchers; the shadow rays in between are traced by hrpt_trace_rays.
//
//   deferred_rays    32 x 8 tiles, one lane per pixel: the pixel's depth and normal texels are loaded once, then one 48-byte HrptRay per
//                    light of the batch as three 16-byte stores at g = j * W * H + y * W + x (a wave writes 64 consecutive records of one
//                    light: 3 KiB contiguous). Light records are read at a wave-uniform index. Streaming, no LDS.
//   deferred_shade   32 x 8 tiles, one lane per pixel: the planes once, the batch's lights re-evaluated, vis = hits[g].t (4 of the 32 bytes
//                    of a hit record), the running sums carried between batches in two float4 images (no carry traffic when one batch
//                    holds every light); the last batch finishes the pixel into colorOut. Misses are written by the last batch only.
#include "pt_device.h"
#include "pt_deferred.h"
#include "pt_image_kernel.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
using namespace deferred;

__global__ __launch_bounds__(img::kTileX * img::kTileY) void deferred_rays(Frame f, const HrptGPULight* __restrict__ lights, uint32_t first, uint32_t count,
                                                                         const float4* __restrict__ depth, const float4* __restrict__ normal,
                                                                         float4* __restrict__ rays)
{
    int px, py;
    if (!img::stage_pixel(f.w, f.h, &px, &py)) return;
    const size_t idx = img::stage_index(f.w, px, py), WH = (size_t)f.w * (size_t)f.h;
    const T4 D = img::ld4(depth, idx), N4 = img::ld4(normal, idx);
    for (uint32_t j = 0; j < count; ++j) {
        T4 rows[3];
        pixel_ray(f, lights[first + j], D, N4, px, py, rows);
        float4* rec = rays + ((size_t)j * WH + idx) * 3;
        img::st4(rec, 0, rows[0]); img::st4(rec, 1, rows[1]); img::st4(rec, 2, rows[2]);
    }
}

__global__ __launch_bounds__(img::kTileX * img::kTileY) void deferred_shade(SceneView scene, Frame f, const HrptGPULight* __restrict__ lights, uint32_t first,
                                                                          uint32_t count, uint32_t isFirst, uint32_t isLast,
                                                                          const float4* __restrict__ albedo, const float4* __restrict__ normal,
                                                                          const float4* __restrict__ geoNormal, const float4* __restrict__ emissive,
                                                                          const float4* __restrict__ depth, const float4* __restrict__ indirect,
                                                                          const HrptRayHit* __restrict__ hits, float4* __restrict__ carryD,
                                                                          float4* __restrict__ carryS, float4* __restrict__ out)
{
    int px, py;
    if (!img::stage_pixel(f.w, f.h, &px, &py)) return;
    const size_t idx = img::stage_index(f.w, px, py), WH = (size_t)f.w * (size_t)f.h;
    const T4 D = img::ld4(depth, idx);
    f3 o, d;
    frame_ray(f, px, py, o, d);
    const f3 sunDir = mk3(f.sun);
    if (D.x == img::kMissDepth) {
        if (!isLast) return;
        T4 sky = t4(0.0f, 0.0f, 0.0f, 0.0f);
        if (f.flags & HRPT_DEFERRED_SKY) {
            const f3 r = atm::sky_radiance(scene, o, d, sunDir, f.sunIntensity, true);
            sky = t4(r.x, r.y, r.z, 1.0f);
        }
        img::st4(out, idx, sky);
        return;
    }
    const T4 A = img::ld4(albedo, idx);
    const float metallic = geoNormal[idx].w;
    const f3 X = o + d * D.x;
    const Lighting s = make_surface(A, img::ld4(normal, idx), metallic, d);
    f3 totalD = mk3(0.0f, 0.0f, 0.0f), totalS = totalD;
    if (!isFirst) { totalD = xyz(img::ld4(carryD, idx)); totalS = xyz(img::ld4(carryS, idx)); }
    add_lights(s, X, sunDir, lights, first, count,
               [&](const HrptGPULight& l) {
                   return (f.flags & HRPT_DEFERRED_SKY) ? atm::sun_radiance(scene, atm::atmosphere_pos(X), sunDir, f.sunIntensity) : light_color(l);
               },
               [&](uint32_t j) { return hits ? hits[(size_t)j * WH + idx].t : 1.0f; }, totalD, totalS);
    if (!isLast) {
        img::st4(carryD, idx, t4(totalD.x, totalD.y, totalD.z, 0.0f));
        img::st4(carryS, idx, t4(totalS.x, totalS.y, totalS.z, 0.0f));
        return;
    }
    const T4 irr = (f.flags & HRPT_DEFERRED_INDIRECT) ? img::ld4(indirect, idx) : t4(0.0f, 0.0f, 0.0f, 0.0f);
    img::st4(out, idx, finish_hit(f, A, img::ld4(emissive, idx), metallic, totalD, totalS, irr));
}
} // namespace

hipError_t launch_deferred_rays(const deferred::Frame& frame, const HrptGPULight* lights, uint32_t first, uint32_t count, const float* depth, const float* normal,
                                HrptRay* rays, hipStream_t stream)
{
    hipLaunchKernelGGL(deferred_rays, img::stage_grid((uint32_t)frame.w, (uint32_t)frame.h), img::stage_block(), 0, stream, frame, lights, first, count,
                       reinterpret_cast<const float4*>(depth), reinterpret_cast<const float4*>(normal), reinterpret_cast<float4*>(rays));
    return hipGetLastError();
}

hipError_t launch_deferred_shade(const SceneView& scene, const deferred::Frame& frame, const HrptGPULight* lights, uint32_t first, uint32_t count, bool isFirst,
                                 bool isLast, const HrptDeferredImages& images, const HrptRayHit* hits, float4* carryD, float4* carryS, hipStream_t stream)
{
    hipLaunchKernelGGL(deferred_shade, img::stage_grid((uint32_t)frame.w, (uint32_t)frame.h), img::stage_block(), 0, stream, scene, frame, lights, first, count,
                       isFirst ? 1u : 0u, isLast ? 1u : 0u, reinterpret_cast<const float4*>(images.albedo), reinterpret_cast<const float4*>(images.normal),
                       reinterpret_cast<const float4*>(images.geoNormal), reinterpret_cast<const float4*>(images.emissive),
                       reinterpret_cast<const float4*>(images.depth), reinterpret_cast<const float4*>(images.indirect), hits, carryD, carryS,
                       reinterpret_cast<float4*>(images.colorOut));
    return hipGetLastError();
}

} // namespace hrt

// pt_restir.hip -- the gfx950 kernels of resampled direct lighting (hrpt_restir_lighting). The arithmetic is pt_restir.h (shared with the
// host executors of pt_restir_host.cpp); the atmosphere terms are pt_atmosphere.h's, as deferred_shade calls them. This file holds the four
// kernels and their launchers; the shadow rays in between are traced by hrpt_trace_rays.
//
// All four: 32 x 8 tiles, one lane per pixel, the planes as 16-byte loads, reservoirs and keys as one 16-byte store per pixel, a shadow-ray
// record as three.
//   restir_initial<LDS>   a lane's candidate indices are random, so a candidate is a 64-byte gather of a light record. LDS = true
//                         (m_LightCount <= HRPT_RESTIR_LDS_MAX_LIGHTS): the block stages the list with 16-byte loads behind one barrier
//                         (64 x HRPT_RESTIR_LDS_MAX_LIGHTS bytes, the kernel's only LDS) and gathers from there; LDS = false: the same
//                         reads go to global memory. Same bits either way.
//   restir_temporal       one record of the history at the reprojected pixel, one target evaluation when it is accepted
//   restir_spatial        per accepted neighbour its planes, its record and two target evaluations; no per-neighbour array
//   restir_shade          the chosen light again, vis = hits[g].t, finish_hit; the sky at misses
#include "pt_device.h"
#include "pt_restir.h"
#include "pt_image_kernel.h"
#include "pt_kernels.h"

namespace hrt {

namespace {
using namespace restir;

struct DeviceIO {
    __host__ __device__ T4 ld(const float* image, size_t idx) const { const float4 v = reinterpret_cast<const float4*>(image)[idx]; return t4(v.x, v.y, v.z, v.w); }
    __host__ __device__ void st(float* image, size_t idx, T4 v) const { reinterpret_cast<float4*>(image)[idx] = make_float4(v.x, v.y, v.z, v.w); }
};
// Radiance of the directional light l at X: the atmosphere's with HRPT_RESTIR_SKY, else colour x intensity.
struct DeviceSun {
    const SceneView& scene; const Args& a;
    __device__ f3 operator()(const HrptGPULight& l, f3 X, int, int) const
    {
        return (a.flags & HRPT_RESTIR_SKY) ? atm::sun_radiance(scene, atm::atmosphere_pos(X), mk3(a.d.sun), a.d.sunIntensity) : deferred::light_color(l);
    }
};
constexpr size_t kHitStride = sizeof(HrptRayHit) / sizeof(float);       // vis = hits[g].t, the first float of a 32-byte record
inline const float* hit_t(const HrptRayHit* hits) { return reinterpret_cast<const float*>(hits); }

template <bool LDS>
__global__ __launch_bounds__(img::kTileX * img::kTileY) void restir_initial(SceneView scene, Args a, const HrptGPULight* __restrict__ lights, HrptRestirImages im,
                                                                          HrptRay* __restrict__ raysOut)
{
    const HrptGPULight* table = lights;
    if constexpr (LDS) {
        __shared__ float4 staged[4 * HRPT_RESTIR_LDS_MAX_LIGHTS];
        const float4* rows = reinterpret_cast<const float4*>(lights);
        for (uint32_t k = threadIdx.y * img::kTileX + threadIdx.x; k < 4u * a.n; k += img::kTileX * img::kTileY) staged[k] = rows[k];
        __syncthreads();                                                 // before the partial tile's lanes leave
        table = reinterpret_cast<const HrptGPULight*>(staged);
    }
    int px, py;
    if (!img::stage_pixel(a.d.w, a.d.h, &px, &py)) return;
    initial_pixel(a, im, table, DeviceIO{}, DeviceSun{ scene, a }, px, py, raysOut);
}

__global__ __launch_bounds__(img::kTileX * img::kTileY) void restir_temporal(SceneView scene, Args a, const HrptGPULight* __restrict__ lights, HrptRestirImages im,
                                                                           const HrptRestirReservoir* __restrict__ initial, const float* __restrict__ vis, uint32_t history)
{
    int px, py;
    if (!img::stage_pixel(a.d.w, a.d.h, &px, &py)) return;
    temporal_pixel(a, im, lights, DeviceIO{}, DeviceSun{ scene, a }, px, py, initial, vis, kHitStride, history != 0u);
}

__global__ __launch_bounds__(img::kTileX * img::kTileY) void restir_spatial(SceneView scene, Args a, const HrptGPULight* __restrict__ lights, HrptRestirImages im,
                                                                          const HrptRestirReservoir* __restrict__ temporal, HrptRay* __restrict__ raysOut)
{
    int px, py;
    if (!img::stage_pixel(a.d.w, a.d.h, &px, &py)) return;
    spatial_pixel(a, im, lights, DeviceIO{}, DeviceSun{ scene, a }, px, py, temporal, raysOut);
}

__global__ __launch_bounds__(img::kTileX * img::kTileY) void restir_shade(SceneView scene, Args a, const HrptGPULight* __restrict__ lights, HrptRestirImages im,
                                                                        const HrptRestirReservoir* __restrict__ fin, const float* __restrict__ vis)
{
    int px, py;
    if (!img::stage_pixel(a.d.w, a.d.h, &px, &py)) return;
    shade_pixel(a, im, lights, DeviceIO{}, DeviceSun{ scene, a },
                [&](int x, int y) {
                    if (!(a.flags & HRPT_RESTIR_SKY)) return t4(0.0f, 0.0f, 0.0f, 0.0f);
                    f3 o, d;
                    deferred::frame_ray(a.d, x, y, o, d);
                    const f3 r = atm::sky_radiance(scene, o, d, mk3(a.d.sun), a.d.sunIntensity, true);
                    return t4(r.x, r.y, r.z, 1.0f);
                },
                px, py, fin, vis, kHitStride);
}

inline dim3 grid(const Args& a) { return img::stage_grid((uint32_t)a.d.w, (uint32_t)a.d.h); }
} // namespace

hipError_t launch_restir_initial(const SceneView& scene, const restir::Args& a, const HrptGPULight* lights, const HrptRestirImages& im, HrptRay* raysOut, bool lds,
                                 hipStream_t stream)
{
    if (lds && a.n <= (uint32_t)HRPT_RESTIR_LDS_MAX_LIGHTS) hipLaunchKernelGGL(restir_initial<true>, grid(a), img::stage_block(), 0, stream, scene, a, lights, im, raysOut);
    else hipLaunchKernelGGL(restir_initial<false>, grid(a), img::stage_block(), 0, stream, scene, a, lights, im, raysOut);
    return hipGetLastError();
}

hipError_t launch_restir_temporal(const SceneView& scene, const restir::Args& a, const HrptGPULight* lights, const HrptRestirImages& im, const HrptRestirReservoir* initial,
                                  const HrptRayHit* initialHits, bool history, hipStream_t stream)
{
    hipLaunchKernelGGL(restir_temporal, grid(a), img::stage_block(), 0, stream, scene, a, lights, im, initial, hit_t(initialHits), history ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_restir_spatial(const SceneView& scene, const restir::Args& a, const HrptGPULight* lights, const HrptRestirImages& im, const HrptRestirReservoir* temporal,
                                 HrptRay* raysOut, hipStream_t stream)
{
    hipLaunchKernelGGL(restir_spatial, grid(a), img::stage_block(), 0, stream, scene, a, lights, im, temporal, raysOut);
    return hipGetLastError();
}

hipError_t launch_restir_shade(const SceneView& scene, const restir::Args& a, const HrptGPULight* lights, const HrptRestirImages& im, const HrptRestirReservoir* fin,
                               const HrptRayHit* hits, hipStream_t stream)
{
    hipLaunchKernelGGL(restir_shade, grid(a), img::stage_block(), 0, stream, scene, a, lights, im, fin, hit_t(hits));
    return hipGetLastError();
}

} // namespace hrt

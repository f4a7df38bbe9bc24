// pt_probes.hip -- the gfx950 kernels of the irradiance probe volume (hrpt_probes_*). The arithmetic is pt_probes.h (shared with the host
// executors of pt_probes_host.cpp); this file holds the kernels and their launchers.
//
//   probes_raygen         one lane per ray record g = p * N + k: 48 bytes as three 16-byte stores; the lanes of probe 0 also write the N
//                         shared directions. Streaming, no LDS.
//   probes_blend          the hot path. One workgroup of 256 lanes per probe: lanes 0..195 own the 14 x 14 distance texels, lanes 196..231
//                         the 6 x 6 irradiance texels. All 232 texels walk the same N rays, so the rays are staged in LDS in chunks of 256
//                         (one ray per lane: its shared direction and the probe's (L, d), 16-byte loads of radiance4 and hits as the trace
//                         calls left them, 32 bytes per ray) and every lane reads the same LDS address per step -- a broadcast, free of bank
//                         conflicts. Each lane keeps its own running sums in ray order, so neither the chunking nor the lane assignment
//                         changes a sum. The finished texels go through LDS for the border copy, and the tiles leave as whole rows of
//                         16-byte stores: 1 KiB + 2 KiB contiguous per probe.
//   probes_query          one lane per point; the eight corner lookups are gathers of 2 x 2 texels.
//   probes_shade_gbuffer  the query at every first hit, 32 x 8 tiles like the other image stages.
#include "pt_image_kernel.h"
#include "pt_kernels.h"
#include "pt_probes.h"

namespace hrt {

namespace {
using namespace probes;

constexpr int kBlendLanes = 256;       // = rays per staged chunk
constexpr int kRaygenLanes = 256, kQueryLanes = 256;

__global__ __launch_bounds__(kRaygenLanes) void probes_raygen(HrptProbeVolume vol, Rotation R, uint32_t frameSeed, uint32_t total, float4* __restrict__ rays,
                                                             float4* __restrict__ directions)
{
    const uint32_t g = blockIdx.x * kRaygenLanes + threadIdx.x;
    if (g >= total) return;
    const uint32_t N = vol.raysPerProbe, p = g / N, k = g - p * N;
    const T3 o = probe_position(vol, p), d = ray_direction(R, k, N);
    float4* rec = rays + (size_t)g * 3;
    rec[0] = make_float4(o.x, o.y, o.z, 0.0f);
    rec[1] = make_float4(d.x, d.y, d.z, kRayTmax);
    rec[2] = make_float4(hrt_u2f(ray_rng(g, frameSeed)), 0.0f, 0.0f, 0.0f);
    if (p == 0u) directions[k] = make_float4(d.x, d.y, d.z, 0.0f);
}

__global__ __launch_bounds__(kBlendLanes) void probes_blend(HrptProbeVolume vol, const float4* __restrict__ directions, const float4* __restrict__ radiance,
                                                           const uint4* __restrict__ hits, float4* __restrict__ irradiance, float2* __restrict__ distance,
                                                           uint32_t hasHistory)
{
    __shared__ float4 sDir[kBlendLanes];
    __shared__ float4 sRay[kBlendLanes];
    __shared__ float4 sIrr[kIrrTile * kIrrTile];
    __shared__ float2 sDist[kDistTile * kDistTile];
    const uint32_t p = blockIdx.x, N = vol.raysPerProbe;
    const int lane = threadIdx.x;
    const bool isDist = lane < kDistTexels, isIrr = !isDist && lane < kDistTexels + kIrrTexels;
    // this lane's texel and its direction
    const int q = isDist ? lane : lane - kDistTexels, I = isDist ? kDistInterior : kIrrInterior;
    const int ti = q % I, tj = q / I;
    const T3 n = texel_direction(ti, tj, I);
    IrrSums si = { 0.0f, 0.0f, 0.0f, 0.0f };
    DistSums sd = { 0.0f, 0.0f, 0.0f };
    for (uint32_t k0 = 0; k0 < N; k0 += kBlendLanes) {
        const uint32_t k = k0 + lane, count = min((uint32_t)kBlendLanes, N - k0);
        if (k < N) {
            const size_t g = (size_t)p * N + k;
            const float4 L = radiance[g];
            const uint4 h0 = hits[g * 2], h1 = hits[g * 2 + 1];       // the 32-byte HrptRayHit: h0.x = t, h1.y = hit
            const float l4[4] = { L.x, L.y, L.z, L.w };
            const T4 s = staged_ray(l4, h1.y, hrt_u2f(h0.x), vol.maxRayDistance);
            sDir[lane] = directions[k];
            sRay[lane] = make_float4(s.x, s.y, s.z, s.w);
        }
        __syncthreads();
        if (isDist) {
            for (uint32_t j = 0; j < count; ++j) dist_add(&sd, n, reinterpret_cast<const float*>(&sDir[j]), reinterpret_cast<const float*>(&sRay[j]), vol.distanceExponent);
        } else if (isIrr) {
            for (uint32_t j = 0; j < count; ++j) irr_add(&si, n, reinterpret_cast<const float*>(&sDir[j]), reinterpret_cast<const float*>(&sRay[j]));
        }
        __syncthreads();
    }
    // the interior texels, blended with what the atlas holds
    float4* irrTile = irradiance + (size_t)p * (kIrrTile * kIrrTile);
    float2* distTile = distance + (size_t)p * (kDistTile * kDistTile);
    if (isDist) {
        const int t = (tj + 1) * kDistTile + (ti + 1);
        const float2 old = distTile[t];
        const T2 v = dist_texel(sd, t2(old.x, old.y), vol.hysteresis, hasHistory != 0u);
        sDist[t] = make_float2(v.x, v.y);
    } else if (isIrr) {
        const int t = (tj + 1) * kIrrTile + (ti + 1);
        const float4 old = irrTile[t];
        const T4 v = irr_texel(si, t4(old.x, old.y, old.z, old.w), vol.hysteresis, hasHistory != 0u);
        sIrr[t] = make_float4(v.x, v.y, v.z, v.w);
    }
    __syncthreads();
    // borders from their interior sources; whole rows as 16-byte stores
    if (lane < kDistTile * kDistTile / 2) {
        const int x = (lane * 2) % kDistTile, y = (lane * 2) / kDistTile;
        int ax, ay, bx, by;
        border_source(x, y, kDistTile, &ax, &ay);
        border_source(x + 1, y, kDistTile, &bx, &by);
        const float2 a = sDist[ay * kDistTile + ax], b = sDist[by * kDistTile + bx];
        reinterpret_cast<float4*>(distTile)[lane] = make_float4(a.x, a.y, b.x, b.y);
    } else if (lane < kDistTile * kDistTile / 2 + kIrrTile * kIrrTile) {
        const int t = lane - kDistTile * kDistTile / 2;
        int sx, sy;
        border_source(t % kIrrTile, t / kIrrTile, kIrrTile, &sx, &sy);
        irrTile[t] = sIrr[sy * kIrrTile + sx];
    }
}

__global__ __launch_bounds__(kQueryLanes) void probes_query(HrptProbeVolume vol, const float* __restrict__ irradiance, const float* __restrict__ distance,
                                                           const float4* __restrict__ points, float4* __restrict__ out, uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * kQueryLanes + threadIdx.x;
    if (i >= count) return;
    const float4 X = points[i * 3], Nn = points[i * 3 + 1], V = points[i * 3 + 2];
    const T4 r = query(vol, irradiance, distance, t3(X.x, X.y, X.z), t3(Nn.x, Nn.y, Nn.z), t3(V.x, V.y, V.z));
    out[i] = make_float4(r.x, r.y, r.z, r.w);
}

__global__ __launch_bounds__(img::kTileX * img::kTileY) void probes_shade_gbuffer(HrptProbeVolume vol, img::ViewArgs view, float intensity,
                                                                                const float* __restrict__ irradiance, const float* __restrict__ distance,
                                                                                const float* __restrict__ normal, const float* __restrict__ depth,
                                                                                float4* __restrict__ out)
{
    int px, py;
    if (!img::stage_pixel(view.w, view.h, &px, &py)) return;
    img::st4(out, img::stage_index(view.w, px, py), shade_pixel(vol, view, intensity, irradiance, distance, normal, depth, px, py));
}
} // namespace

hipError_t launch_probes_raygen(const HrptProbeVolume& vol, uint32_t frameSeed, HrptRay* rays, float* directions4, hipStream_t stream)
{
    const uint32_t total = probe_count(vol) * vol.raysPerProbe;
    hipLaunchKernelGGL(probes_raygen, dim3((total + kRaygenLanes - 1) / kRaygenLanes), dim3(kRaygenLanes), 0, stream, vol, frame_rotation(frameSeed), frameSeed, total,
                       reinterpret_cast<float4*>(rays), reinterpret_cast<float4*>(directions4));
    return hipGetLastError();
}

hipError_t launch_probes_blend(const HrptProbeVolume& vol, const float* directions4, const float* radiance4, const HrptRayHit* hits, float* irradiance,
                               float* distance, bool hasHistory, hipStream_t stream)
{
    hipLaunchKernelGGL(probes_blend, dim3(probe_count(vol)), dim3(kBlendLanes), 0, stream, vol, reinterpret_cast<const float4*>(directions4),
                       reinterpret_cast<const float4*>(radiance4), reinterpret_cast<const uint4*>(hits), reinterpret_cast<float4*>(irradiance),
                       reinterpret_cast<float2*>(distance), hasHistory ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_probes_query(const HrptProbeVolume& vol, const float* irradiance, const float* distance, const HrptProbePoint* points, float* out4,
                               uint64_t count, hipStream_t stream)
{
    hipLaunchKernelGGL(probes_query, dim3((uint32_t)((count + kQueryLanes - 1) / kQueryLanes)), dim3(kQueryLanes), 0, stream, vol, irradiance, distance,
                       reinterpret_cast<const float4*>(points), reinterpret_cast<float4*>(out4), count);
    return hipGetLastError();
}

hipError_t launch_probes_shade_gbuffer(const HrptProbeVolume& vol, const HrptPlanarViewConstants& view, uint32_t width, uint32_t height, float intensity,
                                       const float* irradiance, const float* distance, const float* normal, const float* depth, float4* out,
                                       hipStream_t stream)
{
    hipLaunchKernelGGL(probes_shade_gbuffer, img::stage_grid(width, height), img::stage_block(), 0, stream, vol, img::make_view_args(view, (int)width, (int)height),
                       intensity, irradiance, distance, normal, depth, out);
    return hipGetLastError();
}

} // namespace hrt

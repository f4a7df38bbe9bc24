// pt_megakernel.hip -- the thread-per-query kernels: one thread walks the tree with a private stack for one pixel or one ray. pt_megakernel
// runs the whole of PathTracer_CSMain (/root/reference/src/shaders/PathTracer.hlsl:53-340) for one accumulation index, exactly like one
// dispatch of the reference (8x8 groups -> here 64-lane waves over 8x8 pixel tiles); pt_radiance_kernel runs its bounce loop from a caller's
// ray, pt_gbuffer_kernel and pt_motion_kernel stop at the first hit, pt_trace_rays_kernel answers stand-alone ray queries and pt_surface_rays_kernel
// adds position and geometric normal to them (the radiance cache's surface query). They exist to
// prove struct layouts, RNG streams, LUT sampling, the BVH and the shading stages bit-for-bit against the CPU
// oracle; the wavefront pipeline (pt_wavefront.hip) is the production path and reuses the same stages.
#include <type_traits>

#include "bvh_build.h"
#include "pt_gbuffer.h"
#include "pt_motion.h"
#include "pt_kernels.h"
#include "pt_path.h"

namespace hrt {

// ---- what the kernels share; a new one adds a body and a launcher
struct PrivateStack {       // index wrapped: a two-level structure that needs more entries is refused by the C API (exceeds_private_stack)
    static constexpr int kMask = (int)kPrivateStackDepth - 1;      // bvh_build.h
    int32_t e[kPrivateStackDepth];
    HRT_DEV void push(int sp, int32_t v) { e[sp & kMask] = v; }
    HRT_DEV int32_t pop(int sp) { return e[sp & kMask]; }
};
// TL, the template argument of every kernel: the scene holds the two-level structure (SceneView::instances): the same code over
// closest_two_level / any_hit_two_level (pt_traverse.h, pt_shadow.h), so that the wavefront pipeline's two-level kernels keep the
// wavefront == megakernel cross-check. In a kernel GlobalBvhOf<tree_key<TL>>::make(s) is the tree; on the host with_tree_of picks TL.
template <bool TL> constexpr int tree_key = TL ? kTwoLevelTree : 2;
template <class F> static void with_tree_of(const SceneView& scene, F f) { if (scene.instances) f(std::true_type()); else f(std::false_type()); }
// Pixel of this lane in the block's 8x8 tile (the footprint of [numthreads(8,8,1)], PathTracer.hlsl:52); false: outside the rectangle.
HRT_DEV bool tile_pixel(const TileRect& rect, uint32_t& px, uint32_t& py)
{
    const uint32_t lx = threadIdx.x & 7u, ly = threadIdx.x >> 3;
    px = rect.column_x(blockIdx.x) + lx; py = rect.y0 + blockIdx.y * 8u + ly;
    return px < rect.x1 && py < rect.y1;
}
// ... and the grid of 64-lane blocks for it; false: the rectangle (or this stripe of it) is empty, nothing to launch.
static bool tile_grid(const TileRect& rect, dim3& grid)
{
    grid = dim3(rect.columns(), (rect.y1 - rect.y0 + 7) / 8, 1);
    return !(rect.x1 <= rect.x0 || rect.y1 <= rect.y0 || rect.columns() == 0);
}
// Origin, direction as given and tmin of a caller's ray record; tmax is the kernel's to set.
HRT_DEV void load_ray(const HrptRay& r, Ray& ray)
{
    ray.o = mk3(r.origin[0], r.origin[1], r.origin[2]); ray.d = mk3(r.direction[0], r.direction[1], r.direction[2]); ray.tmin = r.tmin;
}

// The bounce loop of PathTracer_CSMain (PathTracer.hlsl:90-330) for one path from the state `ps` holds (init_path, or a caller's ray record):
// what pt_megakernel and the radiance kernels run. `firstBounce`: the path segment `ps` holds (0; 1 for HRPT_RADIANCE_SECONDARY). Leaves the
// path's radiance in ps.radiance; nClosest / nShadow count its queries.
template <class BVH>
HRT_DEV void trace_path(const SceneView& s, const BVH& bvh, const HrptPathTracerConstants& cb, PathState& ps, PrivateStack& stack,
                        unsigned int& nClosest, unsigned int& nShadow, int firstBounce)
{
    int maxBounces = (int)cb.m_MaxBounces;
    for (int bounce = firstBounce; bounce < maxBounces; ++bounce) {
        Hit hit;
        ++nClosest;
        if (trace_standard(s, bvh, ps.ray, ps.rng, stack, hit)) {
            SurfaceCarry carry;
            f3 totalDiffuse = mk3(0.0f, 0.0f, 0.0f), totalSpecular = mk3(0.0f, 0.0f, 0.0f);
            f3 neeThroughput;
            const f3 sunDir = mk3(cb.m_SunDirection[0], cb.m_SunDirection[1], cb.m_SunDirection[2]);
            const float sunIntensity = s.lights[0].m_Intensity;                  // g_Lights[0], PathTracer.hlsl:137 (quirk kept)
            SurfaceOutcome oc = shade_surface_a<true, true, false>(s, GlobalShadeTables{ s }, cb, ps, hit, carry, [&](uint32_t li, float ux, float uy) {
                HrptGPULight l = load_light(s, li);
                f3 L; float maxDist;
                if (!nee_direction<false>(l, carry.N, carry.worldPos, sunDir, cb.m_CosSunAngularRadius, ux, uy, L, maxDist)) return;
                ++nShadow;
                float shadow = shadow_query(s, bvh, carry.worldPos, L, maxDist, stack);
                if (shadow != 0.0f) {                                              // an occluded sample contributes +0
                    f3 dif, spec;
                    nee_contribution<false>(s, l, nee_lighting(carry.N, carry.V, carry.baseColor, carry.roughness, carry.metallic, carry.ior),
                                            carry.worldPos, sunDir, sunIntensity, L, dif, spec);
                    totalDiffuse = totalDiffuse + dif * shadow;
                    totalSpecular = totalSpecular + spec * shadow;
                }
            });
            if (oc == SURFACE_TRANSMITTED) continue;
            neeThroughput = ps.throughput;
            f3 dsum = totalDiffuse + (bounce == 0 ? totalSpecular : mk3(0.0f, 0.0f, 0.0f));
            ps.radiance = ps.radiance + neeThroughput * dsum;                   // PathTracer.hlsl:261
            if (!shade_surface_b(ps, carry, bounce)) break;
        } else {
            miss_sky(s, cb, ps, bounce);
            break;
        }
    }
}

// One dispatch of the reference shader: one path per pixel of `rect` for cb.m_AccumulationIndex, accumulated and resolved.
template <bool TL>
__global__ __launch_bounds__(64) void pt_megakernel(SceneView s, HrptPathTracerConstants cb, float4* __restrict__ accumulation,
                                                    float4* __restrict__ output, uint32_t imageWidth, TileRect rect,
                                                    DeviceCounters* counters)
{
    uint32_t px, py; bool active = tile_pixel(rect, px, py);
    unsigned int nClosest = 0, nShadow = 0;

    if (active) {
        const auto bvh = GlobalBvhOf<tree_key<TL>>::make(s);
        PrivateStack stack;
        PathState ps; init_path(ps, cb, px, py);
        trace_path(s, bvh, cb, ps, stack, nClosest, nShadow, 0);
        // accumulate + resolve, PathTracer.hlsl:332-339
        size_t idx = (size_t)py * imageWidth + px;
        float4 accum = make_float4(ps.radiance.x, ps.radiance.y, ps.radiance.z, 1.0f);
        if (cb.m_AccumulationIndex > 0) {
            float4 prev = accumulation[idx];
            accum.x += prev.x; accum.y += prev.y; accum.z += prev.z; accum.w += prev.w;
        }
        accumulation[idx] = accum;
        output[idx] = make_float4(accum.x / accum.w, accum.y / accum.w, accum.z / accum.w, 1.0f);
    }
    unsigned long long c = wave_sum_u32(nClosest), sh = wave_sum_u32(nShadow), pa = wave_sum_u32(active ? 1u : 0u);
    if (threadIdx.x == 0) {
        DeviceCounters* shard = counters + (blockIdx.x + blockIdx.y * gridDim.x) % kCounterShards;   // spread the tail atomics
        atomicAdd(&shard->closestRays, c);
        atomicAdd(&shard->shadowRays, sh);
        atomicAdd(&shard->paths, pa);
    }
}
hipError_t launch_megakernel(const SceneView& scene, const HrptPathTracerConstants& constants, float4* accumulation, float4* output,
                             uint32_t imageWidth, TileRect rect, DeviceCounters* counters, hipStream_t stream)
{
    dim3 grid; if (!tile_grid(rect, grid)) return hipSuccess;
    with_tree_of(scene, [&](auto tl) { hipLaunchKernelGGL(pt_megakernel<decltype(tl)::value>, grid, dim3(64, 1, 1), 0, stream, scene, constants, accumulation, output, imageWidth, rect, counters); });
    return hipGetLastError();
}

// hrpt_trace_radiance, validation path (HRPT_RADIANCE_THREAD_PER_RAY, and scenes the wavefront pipeline does not take): one thread per ray runs
// trace_path from the caller's record -- origin, direction as given, tmin, RNG state; unbounded, throughput 1, outside any medium -- and
// leaves the radiance by store_ray_radiance. No counters: HrptStats describes renders. Two kernels of one text: pt_radiance_kernel starts at
// path segment 0, pt_radiance_secondary_kernel at segment 1 (HRPT_RADIANCE_SECONDARY). The text is a macro and not a function both call: through
// a function, however it was spelled, the segment-0 kernel came out with its instructions in another order than before the second one existed.
#define HRT_RADIANCE_KERNEL(NAME, FIRST)                                                                                                   \
    template <bool TL>                                                                                                                     \
    __global__ __launch_bounds__(64) void NAME(SceneView s, HrptPathTracerConstants cb, const HrptRay* __restrict__ rays,                  \
                                               float4* __restrict__ radiance, uint64_t count, uint32_t accumulate)                         \
    {                                                                                                                                      \
        const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;                                                                \
        if (i >= count) return;                                                                                                            \
        const HrptRay r = rays[i];                                                                                                         \
        PathState ps;                                                                                                                      \
        load_ray(r, ps.ray); ps.ray.tmax = 1e10f;                                                                                          \
        ps.rng = r.rng;                                                                                                                    \
        ps.throughput = mk3(1.0f, 1.0f, 1.0f); ps.radiance = mk3(0.0f, 0.0f, 0.0f);                                                        \
        ps.inVolume = false; ps.interiorIOR = 1.0f; ps.sigmaA = mk3(0.0f, 0.0f, 0.0f); ps.sigmaS = mk3(0.0f, 0.0f, 0.0f);                  \
        const bool traced = all_finite(ps.ray.o, ps.ray.d) && (r.tmin - r.tmin) == 0.0f;                                                   \
        if (traced) {                                                                                                                      \
            const auto bvh = GlobalBvhOf<tree_key<TL>>::make(s);                                                                           \
            PrivateStack stack;                                                                                                            \
            unsigned int nClosest = 0, nShadow = 0;                                                                                        \
            trace_path(s, bvh, cb, ps, stack, nClosest, nShadow, FIRST);                                                                   \
        }                                                                                                                                  \
        store_ray_radiance(radiance + i, ps.radiance, traced, accumulate != 0u);                                                           \
    }
HRT_RADIANCE_KERNEL(pt_radiance_kernel, 0)
HRT_RADIANCE_KERNEL(pt_radiance_secondary_kernel, 1)
#undef HRT_RADIANCE_KERNEL
hipError_t launch_radiance_rays(const SceneView& scene, const HrptPathTracerConstants& constants, const HrptRay* rays, float4* radiance, uint64_t count,
                                bool accumulate, bool secondary, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    const dim3 grid((unsigned)((count + 63) / 64));
    with_tree_of(scene, [&](auto tl) {
        if (secondary) hipLaunchKernelGGL(pt_radiance_secondary_kernel<decltype(tl)::value>, grid, dim3(64), 0, stream, scene, constants, rays, radiance, count, accumulate ? 1u : 0u);
        else hipLaunchKernelGGL(pt_radiance_kernel<decltype(tl)::value>, grid, dim3(64), 0, stream, scene, constants, rays, radiance, count, accumulate ? 1u : 0u);
    });
    return hipGetLastError();
}

// First-hit G-buffer, validation path (hrpt_render_gbuffer with HRPT_FRAME_MEGAKERNEL): one thread per pixel, 8x8 pixel tile per wave like
// pt_megakernel: init_path -> trace_standard -> gbuffer_texels (pt_gbuffer.h) -> one 16-byte store per requested plane. No counters: HrptStats
// describes renders.
template <bool TL>
__global__ __launch_bounds__(64) void pt_gbuffer_kernel(SceneView s, HrptPathTracerConstants cb, GBufferPlanes planes, uint32_t planeMask,
                                                        uint32_t imageWidth, TileRect rect)
{
    uint32_t px, py; if (!tile_pixel(rect, px, py)) return;
    const auto bvh = GlobalBvhOf<tree_key<TL>>::make(s);
    PrivateStack stack;
    PathState ps; init_path(ps, cb, px, py);
    float4 texel[kGbPlanes];
    Hit hit;
    if (trace_standard(s, bvh, ps.ray, ps.rng, stack, hit)) gbuffer_texels(s, cb, ps.ray, hit, texel);
    else gbuffer_miss(texel);
    gbuffer_store(planes, planeMask, (size_t)py * imageWidth + px, texel);
}
hipError_t launch_gbuffer_megakernel(const SceneView& scene, const HrptPathTracerConstants& constants, float4* const* planes, uint32_t planeMask,
                                     uint32_t imageWidth, TileRect rect, hipStream_t stream)
{
    dim3 grid; if (!tile_grid(rect, grid)) return hipSuccess;
    GBufferPlanes g; for (uint32_t k = 0; k < kGbPlanes; ++k) g.plane[k] = planes[k];
    with_tree_of(scene, [&](auto tl) { hipLaunchKernelGGL(pt_gbuffer_kernel<decltype(tl)::value>, grid, dim3(64, 1, 1), 0, stream, scene, constants, g, planeMask, imageWidth, rect); });
    return hipGetLastError();
}

// First-hit motion vectors, validation path (hrpt_render_motion_vectors with HRPT_FRAME_MEGAKERNEL): pt_gbuffer_kernel plus the motion texel of
// pt_motion.h; the G-buffer texels are evaluated and stored only when the call names G-buffer planes (planeMask != 0).
template <bool TL>
__global__ __launch_bounds__(64) void pt_motion_kernel(SceneView s, HrptPathTracerConstants cb, GBufferPlanes planes, uint32_t planeMask,
                                                       MotionArgs m, uint32_t imageWidth, TileRect rect)
{
    uint32_t px, py; if (!tile_pixel(rect, px, py)) return;
    const auto bvh = GlobalBvhOf<tree_key<TL>>::make(s);
    PrivateStack stack;
    PathState ps; init_path(ps, cb, px, py);
    float4 texel[kGbPlanes];
    float4 motion = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const size_t idx = (size_t)py * imageWidth + px;
    Hit hit;
    if (trace_standard(s, bvh, ps.ray, ps.rng, stack, hit)) {
        const MotionTri mt = motion_gather(s, m, hit);
        if (planeMask != 0u) gbuffer_texels(s, cb, ps.ray, hit, texel);
        motion = motion_texel(cb.m_View, m, mt, hit.u, hit.v);
    } else if (planeMask != 0u) gbuffer_miss(texel);
    if (planeMask != 0u) gbuffer_store(planes, planeMask, idx, texel);
    m.plane[idx] = motion;
}
hipError_t launch_motion_megakernel(const SceneView& scene, const HrptPathTracerConstants& constants, float4* const* planes, uint32_t planeMask,
                                    const MotionArgs& motion, uint32_t imageWidth, TileRect rect, hipStream_t stream)
{
    dim3 grid; if (!tile_grid(rect, grid)) return hipSuccess;
    GBufferPlanes g; for (uint32_t k = 0; k < kGbPlanes; ++k) g.plane[k] = planes[k];
    with_tree_of(scene, [&](auto tl) { hipLaunchKernelGGL(pt_motion_kernel<decltype(tl)::value>, grid, dim3(64, 1, 1), 0, stream, scene, constants, g, planeMask, motion, imageWidth, rect); });
    return hipGetLastError();
}

// Stand-alone ray queries over the scene's acceleration structure: TraceRayStandard (RaytracingCommon.hlsli:138-198) and
// CalculateRTShadow<true> (CommonLighting.hlsli:380-496) for callers other than the path tracer (the reference's DDGI probe trace,
// ray-traced shadows and BRDF ray tracing share exactly these two includes). One thread per ray, 2-wide tree, private stack.
template <bool SHADOW, bool TL>
__global__ __launch_bounds__(256) void pt_trace_rays_kernel(SceneView s, const HrptRay* __restrict__ rays, HrptRayHit* __restrict__ hits, uint64_t count)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    HrptRay r = rays[i];
    HrptRayHit out; out.t = 0.0f; out.u = 0.0f; out.v = 0.0f; out.instance = 0; out.primitive = 0; out.hit = 0; out.rng = r.rng; out.pad = 0;
    const auto bvh = GlobalBvhOf<tree_key<TL>>::make(s);
    PrivateStack stack;
    Ray ray; load_ray(r, ray); ray.tmax = r.tmax;
    const bool finite = all_finite(ray.o, ray.d);
    if (SHADOW) {
        out.t = finite ? shadow_query(s, bvh, ray.o, ray.d, r.tmax, stack) : 1.0f;     // visibility in [0, 1]
        out.hit = out.t < 1.0f ? 1u : 0u;
    } else if (finite) {
        uint32_t rng = r.rng; Hit h;
        if (trace_standard(s, bvh, ray, rng, stack, h)) { out.t = h.t; out.u = h.u; out.v = h.v; out.instance = h.inst; out.primitive = h.prim; out.hit = 1; }
        out.rng = rng;
    }
    hits[i] = out;
}
hipError_t launch_trace_rays(const SceneView& scene, const HrptRay* rays, HrptRayHit* hits, uint64_t count, bool shadow, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    dim3 grid((unsigned)((count + 255) / 256));
    with_tree_of(scene, [&](auto tl) {
        if (shadow) hipLaunchKernelGGL((pt_trace_rays_kernel<true, decltype(tl)::value>), grid, dim3(256), 0, stream, scene, rays, hits, count);
        else hipLaunchKernelGGL((pt_trace_rays_kernel<false, decltype(tl)::value>), grid, dim3(256), 0, stream, scene, rays, hits, count);
    });
    return hipGetLastError();
}

// Where rays land, for the radiance cache (hrpt_rcache_surfaces_device): pt_trace_rays_kernel's closest-hit query, then the terms gbuffer_texels
// forms of the hit (pt_gbuffer.h:36-38): position o + d * t and Ng = normalize(worldNormal), here turned to face the ray. One thread per ray.
template <bool TL>
__global__ __launch_bounds__(256) void pt_surface_rays_kernel(SceneView s, const HrptRay* __restrict__ rays, float4* __restrict__ surfaces, uint64_t count)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    HrptRay r = rays[i];
    float4 row0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), row1 = row0;
    uint32_t rng = r.rng;
    Ray ray; load_ray(r, ray); ray.tmax = r.tmax;
    if (all_finite(ray.o, ray.d)) {
        const auto bvh = GlobalBvhOf<tree_key<TL>>::make(s);
        PrivateStack stack;
        Hit hit;
        if (trace_standard(s, bvh, ray, rng, stack, hit)) {
            const TriVerts tv = load_hit_attr(s, hit);
            const SurfaceAttr attr = full_hit_attributes(s, hit, ray, tv, s.instShade[tv.inst], false);
            f3 Ng = normalize(attr.worldNormal);
            if (dot(Ng, ray.d) > 0.0f) Ng = -Ng;
            const f3 X = ray.o + ray.d * hit.t;
            row0 = make_float4(X.x, X.y, X.z, hit.t);
            row1 = make_float4(Ng.x, Ng.y, Ng.z, __uint_as_float(1u));
        }
    }
    surfaces[i * 3] = row0; surfaces[i * 3 + 1] = row1;
    surfaces[i * 3 + 2] = make_float4(__uint_as_float(rng), 0.0f, 0.0f, 0.0f);
}
hipError_t launch_surface_rays(const SceneView& scene, const HrptRay* rays, HrptRcacheSurface* surfaces, uint64_t count, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    dim3 grid((unsigned)((count + 255) / 256));
    with_tree_of(scene, [&](auto tl) {
        hipLaunchKernelGGL(pt_surface_rays_kernel<decltype(tl)::value>, grid, dim3(256), 0, stream, scene, rays, reinterpret_cast<float4*>(surfaces), count);
    });
    return hipGetLastError();
}

} // namespace hrt

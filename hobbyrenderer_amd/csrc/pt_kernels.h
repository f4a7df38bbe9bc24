// pt_kernels.h -- host-callable launchers of the gfx950 path-tracer kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"

namespace hrt {

struct SceneView;   // pt_scene_records.h
struct MotionArgs;  // pt_motion_records.h
struct GpuNode4; struct GpuNodeQ;   // pt_scene_records.h

constexpr int kCounterShards = 32;   // DeviceCounters[kCounterShards] per context; a block adds to shard blockIdx % kCounterShards
struct DeviceCounters {         // 80 B; summed over the shards by hrpt_get_stats. The wavefront kernels address the fields by word index.
    unsigned long long closestRays;       // 0
    unsigned long long shadowRays;        // 1
    unsigned long long paths;             // 2
    unsigned long long neeEntries;        // 3: shadow-queue entries wf_shade wrote (path vertices with at least one light sample)
    unsigned long long neeSamples;        // 4: light-sample records wf_shadow read
    unsigned long long radianceShade;     // 5: sampleRadiance read-modify-writes of wf_shade (emissive / sky terms)
    unsigned long long radianceShadow;    // 6: sampleRadiance read-modify-writes of wf_shadow (NEE terms)
    unsigned long long skipped16;         // 7: 16-byte path-record reads wf_shadow's slim mode did not make at bounce 0 of a batch without raygen pass
    unsigned long long fusedPaths;        // 8: primary paths wf_bounce0 traced and shaded (no hit record, no {direction, seed} record for all of them)
    unsigned long long fusedEntries;      // 9: ... and the shadow-queue entries it emitted (a {direction, seed} record written for each)
};

struct TileRect {
    uint32_t x0, y0, x1, y1;
    uint32_t stripeCount = 1, stripeIndex = 0;     // of the rectangle's 8-pixel columns, those with column % stripeCount == stripeIndex
    // number of 8-pixel columns this call covers / pixel column of its k-th one
    __host__ __device__ uint32_t columns() const { uint32_t all = (x1 - x0 + 7u) / 8u; return all > stripeIndex ? (all - stripeIndex + stripeCount - 1u) / stripeCount : 0u; }
    __host__ __device__ uint32_t column_x(uint32_t k) const { return x0 + (k * stripeCount + stripeIndex) * 8u; }
};

// ---- thread-per-query kernels (pt_megakernel.hip): the validation paths, one thread per pixel or ray with a private traversal stack
// One dispatch of the reference shader: one path per pixel of `rect` for constants.m_AccumulationIndex.
hipError_t launch_megakernel(const SceneView& scene, const HrptPathTracerConstants& constants, float4* accumulation,
                             float4* output, uint32_t imageWidth, TileRect rect, DeviceCounters* counters, hipStream_t stream);

// First-hit G-buffer (pt_gbuffer.h): planes[HRPT_GB_PLANES] device images of imageWidth x H float4, of which those in
// planeMask are written inside `rect`; constants.m_Jitter / m_AccumulationIndex are used as given.
hipError_t launch_gbuffer_megakernel(const SceneView& scene, const HrptPathTracerConstants& constants, float4* const* planes, uint32_t planeMask,
                                     uint32_t imageWidth, TileRect rect, hipStream_t stream);

// First-hit motion vectors (pt_motion.h): launch_gbuffer_megakernel's pass plus motion.plane; planeMask may be 0.
hipError_t launch_motion_megakernel(const SceneView& scene, const HrptPathTracerConstants& constants, float4* const* planes, uint32_t planeMask,
                                    const MotionArgs& motion, uint32_t imageWidth, TileRect rect, hipStream_t stream);

// Batch ray queries (hrpt_trace_rays): closest hit with the candidate rules of TraceRayStandard, or NEE-style visibility.
hipError_t launch_trace_rays(const SceneView& scene, const HrptRay* rays, HrptRayHit* hits, uint64_t count, bool shadow, hipStream_t stream);

// Path-traced radiance along a caller's rays (hrpt_trace_radiance): the megakernel's bounce loop from the ray's record;
// radiance[i] = (L, 1), or with `accumulate` (old.rgb + L, old.w + 1). Device arrays.
hipError_t launch_radiance_rays(const SceneView& scene, const HrptPathTracerConstants& constants, const HrptRay* rays, float4* radiance, uint64_t count,
                                bool accumulate, bool secondary, hipStream_t stream);

// ---- accumulation to output (pt_resolve.hip)
// Output[xy] = accum.rgb / accum.a (PathTracer.hlsl:339) over the whole image; launch_resolve_columns: the same from the rank-major column
// shards of an all-gather, with the assembled accumulation image when `accumulation` is not null.
hipError_t launch_resolve(const float4* accumulation, float4* output, uint32_t pixelCount, hipStream_t stream);
hipError_t launch_resolve_columns(const float4* shards, float4* accumulation, float4* output, uint32_t width, uint32_t height, uint32_t ranks, hipStream_t stream);

// ---- the GpuNodeQ encoding (pt_bvh_nodes.hip)
// The flat 4-wide tree in its 64-byte quantised form (pt_scene_records.h GpuNodeQ): out[i] from nodes4[i]. leafArea (two zeroed doubles, or null)
// receives the summed surface area of the leaf boxes before / after the rounding: what the looser boxes will cost in triangle tests.
hipError_t launch_quantise_nodes(const GpuNode4* nodes4, uint32_t count, GpuNodeQ* out, double* leafArea, hipStream_t stream);
// Self-test: counts child boxes of the 2-wide and 4-wide trees that do not contain their subtree's boxes / triangle vertices (0 = sound).
hipError_t launch_bvh_check(const SceneView& scene, unsigned long long* violations, hipStream_t stream);

// ---- decode and lookup self-tests (pt_selftest.hip)
// out[i] = device decode of the binary16 pattern i, i in [0, 65536); out512 = the unorm8 decode of every byte, then the division it replaces.
hipError_t launch_unorm8_table(float* out512, hipStream_t stream);
hipError_t launch_f16_table(float* out, hipStream_t stream);
// results[i] = the shader's texture sampling functions on probes[i] (hrpt_selftest_sample_textures); device arrays.
hipError_t launch_sample_textures(const SceneView& scene, uint32_t materialCount, const HrptTextureProbe* probes, HrptTextureProbeResult* results,
                                  uint32_t count, hipStream_t stream);
// results[i] = the run-time atmosphere lookups (sky radiance, sun radiance, transmittance) on probes[i] (hrpt_selftest_atmosphere); device arrays.
hipError_t launch_atmosphere_probes(const SceneView& scene, const HrptAtmosphereProbe* probes, HrptAtmosphereProbeResult* results, uint32_t count, hipStream_t stream);

// HDR post chain over `hdr` (W*H float4): histogram[256] + exposure[1] are context-owned device buffers.
hipError_t launch_post_chain(const float4* hdr, float4* display, uint32_t pixelCount, const HrptPostParams& params, uint32_t* histogram,
                             float* exposure, hipStream_t stream);

// Bloom (pt_bloom.hip; arithmetic in pt_bloom.h): composites into `hdr` (W x H float4) in place. downPyramid / upPyramid hold
// bloom_pyramid_words(W, H) packed R11G11B10_FLOAT words each. tailTexels: 0 = one kernel per pass, otherwise the levels from the first one
// with at most that many texels on run in one workgroup's LDS (same bits). bloom_host: the same arithmetic on host threads.
size_t bloom_pyramid_words(uint32_t width, uint32_t height);
bool bloom_params_valid(const HrptBloomParams& params);
hipError_t launch_bloom(float4* hdr, uint32_t width, uint32_t height, const HrptBloomParams& params, uint32_t* downPyramid, uint32_t* upPyramid,
                        uint32_t tailTexels, hipStream_t stream);
void bloom_pack_probe(const float* rgb, uint32_t count, uint32_t* packed, float* unpacked);   // test hook: the format conversion alone
void bloom_host(const float* hdrIn, float* hdrOut, uint32_t width, uint32_t height, const HrptBloomParams& params, int nthreads);

// Temporal accumulation (pt_temporal.hip; arithmetic in pt_temporal.h): one kernel over width x height device images. temporal_host
// (pt_temporal_host.cpp): the same arithmetic on host threads. colorOut may be color; historyOut must not be historyIn.
bool temporal_params_valid(const HrptTemporalParams& params);
hipError_t launch_temporal(const HrptTemporalImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                           const HrptPlanarViewConstants& prevView, const HrptTemporalParams& params, hipStream_t stream);
void temporal_host(const HrptTemporalImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                   const HrptPlanarViewConstants& prevView, const HrptTemporalParams& params, int nthreads);

// Temporal upscaling (pt_upscale.hip; arithmetic in pt_upscale.h): one kernel from width x height colour, depth and motion images into
// displayWidth x displayHeight history and colour images. staged: false = the nine current-frame taps are global gathers (the measured-faster
// default), true = they are served from an LDS-staged window (same bits). upscale_host (pt_upscale_host.cpp): the same arithmetic on host
// threads. historyOut must not be historyIn, and colorOut neither of them.
bool upscale_params_valid(const HrptUpscaleParams& params);
bool upscale_ratio_ok(uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight);
hipError_t launch_upscale(const HrptUpscaleImages& images, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                          const HrptPlanarViewConstants& view, const HrptPlanarViewConstants& prevView, const HrptUpscaleParams& params, bool staged,
                          hipStream_t stream);
void upscale_host(const HrptUpscaleImages& images, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                  const HrptPlanarViewConstants& view, const HrptPlanarViewConstants& prevView, const HrptUpscaleParams& params, int nthreads);

// Denoise (pt_denoise.hip; arithmetic in pt_denoise.h): ONE pass of the Poisson filter with the given radius and frame over width x height
// device images; images.noise must be set (a device tile of denoise_noise_floats() floats). denoise_host (pt_denoise_host.cpp): the same
// arithmetic on host threads; a NULL images.noise means the default tile there. colorOut may be color; output must not be input.
bool denoise_params_valid(const HrptDenoiseParams& params);
size_t denoise_noise_floats();
void denoise_default_tile(float* tile);
hipError_t launch_denoise(const HrptDenoiseImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                          const HrptDenoiseParams& params, float radius, uint32_t frame, hipStream_t stream);
void denoise_host(const HrptDenoiseImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                  const HrptDenoiseParams& params, int nthreads);

// Demodulate / compose (pt_modulation.hip; arithmetic in pt_modulation.h): one kernel each over width x height device images; emissive may be
// null. demodulate_host / compose_host (pt_modulation_host.cpp): the same arithmetic on host threads. colorOut may be color; modulationOut
// aliases nothing. modulation_probe: the factor of one hit with the view vector given (test hook).
bool modulation_params_valid(const HrptModulationParams& params);
hipError_t launch_demodulate(const HrptDemodulateImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                             const HrptModulationParams& params, hipStream_t stream);
hipError_t launch_compose(const HrptComposeImages& images, uint32_t width, uint32_t height, hipStream_t stream);
void demodulate_host(const HrptDemodulateImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                     const HrptModulationParams& params, int nthreads);
void compose_host(const HrptComposeImages& images, uint32_t width, uint32_t height, int nthreads);
void modulation_probe(const float* albedo3, const float* N3, const float* V3, float rough, float metal, float floor, float* outM3);

// Irradiance probe volume (pt_probes.hip; arithmetic in pt_probes.h): ray records and shared directions of an update, the blend of traced
// rays into the atlases (in place), the query at points and at the first hits of the G-buffer; every pointer in device memory, 16-byte
// aligned. probes_*_host (pt_probes_host.cpp): the same arithmetic on host threads; raysOut / directions4Out may be null there.
bool probes_volume_valid(const HrptProbeVolume& volume);
hipError_t launch_probes_raygen(const HrptProbeVolume& volume, uint32_t frameSeed, HrptRay* rays, float* directions4, hipStream_t stream);
hipError_t launch_probes_blend(const HrptProbeVolume& volume, const float* directions4, const float* radiance4, const HrptRayHit* hits, float* irradiance,
                               float* distance, bool hasHistory, hipStream_t stream);
hipError_t launch_probes_query(const HrptProbeVolume& volume, const float* irradiance, const float* distance, const HrptProbePoint* points, float* out4,
                               uint64_t count, hipStream_t stream);
hipError_t launch_probes_shade_gbuffer(const HrptProbeVolume& volume, const HrptPlanarViewConstants& view, uint32_t width, uint32_t height, float intensity,
                                       const float* irradiance, const float* distance, const float* normal, const float* depth, float4* out,
                                       hipStream_t stream);
void probes_rays_host(const HrptProbeVolume& volume, uint32_t frameSeed, HrptRay* raysOut, float* directions4Out);
void probes_blend_host(const HrptProbeVolume& volume, const float* directions4, const float* radiance4, const HrptRayHit* hits, float* irradiance,
                       float* distance, bool hasHistory, int nthreads);
void probes_query_host(const HrptProbeVolume& volume, const float* irradiance, const float* distance, const HrptProbePoint* points, float* out4,
                       uint64_t count, int nthreads);

// Deferred lighting (pt_deferred.hip; arithmetic in pt_deferred.h): the shadow-ray records of lights [first, first + count) at every pixel
// (rays: count * W * H records), and the shade pass of the same lights over the hit records hrpt_trace_rays left (hits null = visibility 1),
// which carries the running sums in carryD / carryS between batches (read unless isFirst, written unless isLast; may be null for a single
// batch) and finishes images.colorOut on the last one. Every pointer in device memory, 16-byte aligned. deferred_*_host
// (pt_deferred_host.cpp): the same arithmetic on host threads, the atmosphere terms and visibilities as images.
namespace deferred { struct Frame; }
bool deferred_params_valid(const HrptDeferredParams& params);
hipError_t launch_deferred_rays(const deferred::Frame& frame, const HrptGPULight* lights, uint32_t first, uint32_t count, const float* depth, const float* normal,
                                HrptRay* rays, hipStream_t stream);
hipError_t launch_deferred_shade(const SceneView& scene, const deferred::Frame& frame, const HrptGPULight* lights, uint32_t first, uint32_t count, bool isFirst,
                                 bool isLast, const HrptDeferredImages& images, const HrptRayHit* hits, float4* carryD, float4* carryS, hipStream_t stream);
void deferred_rays_host(const HrptDeferredImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                        uint32_t firstLight, uint32_t lightCount, HrptRay* raysOut);
void deferred_shade_host(const HrptDeferredImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                         uint32_t lightCount, const float* visibility, const float* sunRadiance, const float* sky, const HrptDeferredParams& params,
                         int nthreads);

// Traced indirect lighting (pt_indirect.hip; arithmetic in pt_indirect.h): the diffuse and specular ray records of every pixel (rays: W * H
// records per flagged lobe, diffuse first), the resolve of the radiance hrpt_trace_radiance left for them into images.diffuse /
// images.specular (either may be null), and the compose into images.colorInOut. Every pointer in device memory, 16-byte aligned.
// indirect_*_host (pt_indirect_host.cpp): the same arithmetic on host threads.
namespace indirect { struct Frame; }
bool indirect_params_valid(const HrptIndirectParams& params);
hipError_t launch_indirect_rays(const indirect::Frame& frame, const HrptIndirectImages& images, HrptRay* rays, hipStream_t stream);
hipError_t launch_indirect_resolve(const indirect::Frame& frame, const HrptIndirectImages& images, const float4* radiance, hipStream_t stream);
hipError_t launch_indirect_compose(const HrptIndirectImages& images, uint32_t width, uint32_t height, float intensity, hipStream_t stream);
void indirect_rays_host(const HrptIndirectImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptIndirectParams& params,
                        HrptRay* raysOut, int nthreads);
void indirect_resolve_host(const HrptIndirectImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptIndirectParams& params,
                           const float* radiance4, int nthreads);
void indirect_compose_host(const HrptIndirectImages& images, uint32_t width, uint32_t height, const HrptIndirectParams& params, int nthreads);

// Resampled direct lighting (pt_restir.hip; arithmetic in pt_restir.h): the four passes, each over the planes of `images` and the device
// arrays named after what they hold. initial writes images.reservoirOut (raysOut null = no record); temporal reads `initial`, its hit
// records (null = visibility 1) and, with `history`, images.reservoirIn / keyIn / motion, and writes images.reservoirOut; spatial reads
// `temporal` and writes images.reservoirOut, images.keyOut and the final ray records (raysOut null = none); shade reads `final` and its hit
// records (null = visibility 1) and writes images.colorOut. `lds`: initial stages the light list in LDS when it fits. No output may alias an
// input of the same pass. restir_*_host (pt_restir_host.cpp): the same arithmetic on host threads, atmosphere terms and visibilities as images.
namespace restir { struct Args; }
bool restir_params_valid(const HrptRestirParams& params);
hipError_t launch_restir_initial(const SceneView& scene, const restir::Args& args, const HrptGPULight* lights, const HrptRestirImages& images, HrptRay* raysOut, bool lds,
                                 hipStream_t stream);
hipError_t launch_restir_temporal(const SceneView& scene, const restir::Args& args, const HrptGPULight* lights, const HrptRestirImages& images,
                                  const HrptRestirReservoir* initial, const HrptRayHit* initialHits, bool history, hipStream_t stream);
hipError_t launch_restir_spatial(const SceneView& scene, const restir::Args& args, const HrptGPULight* lights, const HrptRestirImages& images,
                                 const HrptRestirReservoir* temporal, HrptRay* raysOut, hipStream_t stream);
hipError_t launch_restir_shade(const SceneView& scene, const restir::Args& args, const HrptGPULight* lights, const HrptRestirImages& images,
                               const HrptRestirReservoir* final, const HrptRayHit* hits, hipStream_t stream);
void restir_initial_host(const HrptRestirImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                         const HrptRestirParams& params, const float* sunRadiance, HrptRay* raysOut, int nthreads);
void restir_temporal_host(const HrptRestirImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                          const HrptRestirParams& params, const float* sunRadiance, const HrptRestirReservoir* initial, const float* initialVisibility, int nthreads);
void restir_spatial_host(const HrptRestirImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                         const HrptRestirParams& params, const float* sunRadiance, const HrptRestirReservoir* temporal, HrptRay* raysOut, int nthreads);
void restir_shade_host(const HrptRestirImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                       const HrptRestirParams& params, const float* sunRadiance, const float* sky, const HrptRestirReservoir* final, const float* visibility, int nthreads);

// Hash-grid radiance cache (pt_rcache.hip; arithmetic in pt_rcache.h): the four table kernels over three device arrays of 2^capacityLog2
// entries and the drop counter, and the glue of the two frame calls. query reads `count` records of recordBytes (32: HrptRcachePoint, 48:
// HrptRcacheSurface; position in floats 0..2, normal in floats 4..6). update_rays writes one diffuse record per sparse block, row-major over
// the blocks; serve writes the served plane and overwrites the records of served pixels; apply copies served texels over the diffuse plane.
// Every pointer in device memory, 16-byte aligned. rcache_*_host (pt_rcache_host.cpp): the table stages on host threads.
// launch_surface_rays (pt_megakernel.hip): position, facing geometric normal, t and RNG state at the closest hit of each ray.
bool rcache_desc_valid(const HrptRcacheDesc& desc);
hipError_t launch_surface_rays(const SceneView& scene, const HrptRay* rays, HrptRcacheSurface* surfaces, uint64_t count, hipStream_t stream);
hipError_t launch_rcache_insert(const HrptRcacheDesc& desc, const float* cameraPos, uint64_t* keys, HrptRcacheAccum* accum, uint64_t* drops,
                                const HrptRcacheSample* samples, uint64_t count, bool waveCombine, hipStream_t stream);
hipError_t launch_rcache_resolve(const HrptRcacheDesc& desc, uint64_t* keys, HrptRcacheAccum* accum, HrptRcacheEntry* resolved, hipStream_t stream);
hipError_t launch_rcache_query(const HrptRcacheDesc& desc, const float* cameraPos, const uint64_t* keys, const HrptRcacheEntry* resolved, const void* records,
                               uint32_t recordBytes, float* out4, float* voxelOut, uint64_t count, hipStream_t stream);
hipError_t launch_rcache_clear(const HrptRcacheDesc& desc, uint64_t* keys, HrptRcacheAccum* accum, HrptRcacheEntry* resolved, uint64_t* drops, hipStream_t stream);
hipError_t launch_rcache_update_rays(const indirect::Frame& frame, const HrptRcacheDesc& desc, uint32_t frameIndex, const float* normal, const float* geoNormal,
                                     const float* depth, HrptRay* rays, hipStream_t stream);
hipError_t launch_rcache_gather_samples(const HrptRcacheSurface* surfaces, const float4* radiance, HrptRcacheSample* samples, uint64_t count, hipStream_t stream);
hipError_t launch_rcache_serve(const HrptRcacheSurface* surfaces, const float4* cached, const float* voxel, float4* servedOut, HrptRay* rays, uint64_t count,
                               hipStream_t stream);
hipError_t launch_rcache_apply(const float4* servedPlane, float4* diffuse, uint64_t count, hipStream_t stream);
void rcache_insert_host(const HrptRcacheDesc& desc, const float* cameraPos, uint64_t* keys, HrptRcacheAccum* accum, uint64_t* drops, const HrptRcacheSample* samples,
                        uint64_t count, int nthreads);
void rcache_resolve_host(const HrptRcacheDesc& desc, uint64_t* keys, HrptRcacheAccum* accum, HrptRcacheEntry* resolved, int nthreads);
void rcache_query_host(const HrptRcacheDesc& desc, const float* cameraPos, const uint64_t* keys, const HrptRcacheEntry* resolved, const HrptRcachePoint* points,
                       float* out4, float* voxelOut, uint64_t count, int nthreads);
// nullptr when the table keeps the invariant of pt_rcache.h, else what breaks it
const char* rcache_table_fault(const HrptRcacheDesc& desc, const uint64_t* keys, const HrptRcacheAccum* accum, const HrptRcacheEntry* resolved);

// Vertex quantiser (pt_deform.hip; arithmetic in pt_deform.h): out[i] = the 24-byte scene-format record of the float vertex in[i], both in
// device memory (in 16-byte aligned); *flag (device, may be null) is set to 1 when a position is not finite. quantize_vertices_host
// (pt_deform_host.cpp): the same arithmetic on host threads; returns whether every position is finite.
hipError_t launch_quantise_vertices(const HrptVertexFloat* in, uint32_t count, HrptVertexQuantized* out, uint32_t* flag, hipStream_t stream);
bool quantize_vertices_host(const HrptVertexFloat* in, uint32_t count, HrptVertexQuantized* out, int nthreads);

// Vertex producer (pt_skin.hip; arithmetic in pt_skin.h): morph targets + four-joint skinning of args.base, every pointer of args in device
// memory, into float records (out 16-byte aligned). status2 (device; may be null): word 0 is set to 1 when an output position is not
// finite, word 1 when a joint index is >= args.jointCount. palette: 0 = LDS up to HRPT_SKIN_LDS_MAX_JOINTS joints and a global gather beyond, 1 = always the
// gather (for A/B measurements). skin_vertices_host (pt_skin_host.cpp): the same arithmetic on host threads, args in host memory; returns
// the skin::k* bits, and writes nothing when a joint index is out of range.
hipError_t launch_skin_vertices(const HrptSkinArgs& args, HrptVertexFloat* out, uint32_t* status2, int palette, hipStream_t stream);
uint32_t skin_vertices_host(const HrptSkinArgs& args, HrptVertexFloat* out, int nthreads);

// Animation stage (pt_anim.hip; arithmetic in pt_anim.h): the three kernels of hrpt_animate on `stream`, every pointer in device memory.
// tables: anim::Tables with device arrays; times: one per animation; groupFirst: groups + 1 offsets into tables.order (device) and the same
// on the host; trs (12 floats per node, seeded with the base pose), worlds (16 per node, seeded with baseWorld), weights and palette are
// the state the kernels write. records: the instance records [tables.instanceFirst, + tables.instanceRange), 160 bytes each, or null to
// leave instances alone.
namespace anim { struct Tables; }
hipError_t launch_animate(const anim::Tables& tables, const float* times, const uint32_t* groupFirst, const uint32_t* groupFirstHost, uint32_t groups,
                          float* trs, float* worlds, float* weights, float* palette, void* records, hipStream_t stream);

} // namespace hrt

// pt_wavefront.h -- host interface of the persistent wavefront pipeline (pt_wavefront.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/hobbyrt_pt.h"
#include "pt_device_buffer.h"
#include "pt_kernels.h"
#include "pt_wavefront_plan.h"

namespace hrt {

struct SceneView;
struct MotionArgs;     // pt_motion.h

// Kernel classes of the per-launch timing; the values index WavefrontState::kernelMs / kernelLaunches and name HrptStats fields in this order.
enum KernelClass : int { kKernelExtend = 0, kKernelShade = 1, kKernelShadow = 2, kKernelRaygen = 3, kKernelResolve = 4, kKernelClasses = 5 };

struct WavefrontState {
    DeviceBuffer<void> pool;           // one device allocation carved into the SoA queues
    DeviceBuffer<void> spill;          // traversal-stack overflow columns (only for trees deeper than the LDS stack)
    DeviceBuffer<void> traceSpill;     // the same for hrpt_trace_rays batches
    DeviceBuffer<void> gbPool;         // queue pool of hrpt_render_gbuffer calls the render's pool is too small for (never rendered, or a smaller tile)
    DeviceBuffer<void> radPool;        // the same for hrpt_trace_radiance batches
    // start/stop event pairs around every timed launch; kind[i] = its KernelClass
    std::vector<hipEvent_t> events;
    std::vector<uint8_t> kind;
    uint32_t eventsUsed = 0;
    float kernelMs[kKernelClasses] = {};            // summed device time per kernel class since the last reset
    uint32_t kernelLaunches[kKernelClasses] = {};
    // queue-byte accounting (HrptStats::*QueueBytes): what the host knows per render is summed here, the rest follows from the device
    // counters and the record layout of the last render (its plan)
    uint64_t raygenBytes = 0, resolveBytes = 0;
    RenderPlan plan;
    uint32_t shadeInstances = 0, shadeMaterials = 0;   // records of SceneView::instShade / materials (set by the owner of the scene; 0 = unknown: no LDS tables)
    WavefrontKnobs knobs;
    uint32_t cus = 0;                  // compute units of the context's device (0: not asked yet)
    bool profile = false;              // record HIP events around every extend / shade / shadow launch (HRPT_FRAME_PROFILE)
    // second stream + fork/join events: wf_shadow(b) overlaps wf_extend(b+1) (they share no buffer)
    hipStream_t auxStream = nullptr;
    std::vector<hipEvent_t> forkEvents, joinEvents;
};

bool wavefront_supports(const SceneView& scene, const HrptPathTracerConstants& constants);
hipError_t wavefront_render(WavefrontState& st, const SceneView& scene, const SceneTraits& traits, const HrptPathTracerConstants& constants,
                            uint32_t accumCount, float4* accumulation, float4* output, uint32_t width, uint32_t height, TileRect rect,
                            DeviceCounters* counters, hipStream_t stream, std::string& error);
// hrpt_trace_rays over device arrays (where wavefront_trace_rays_supported, pt_wavefront_plan.h)
hipError_t wavefront_trace_rays(WavefrontState& st, const SceneView& scene, const SceneTraits& traits, const HrptRay* rays, HrptRayHit* hits, uint64_t count,
                                bool shadow, hipStream_t stream, std::string& error);
// hrpt_render_gbuffer: the render's bounce-0 front end over one sample per pixel of `rect`, then wf_gbuffer into the planes of planeMask
// (planes[HRPT_GB_PLANES], width x H float4 each). Leaves the statistics, the plan and the timing state of renders alone.
// hrpt_render_motion_vectors is the same call with `motion` (pt_motion.h): wf_gbuffer_motion then writes motion->plane as well, and planeMask may be 0.
hipError_t wavefront_gbuffer(WavefrontState& st, const SceneView& scene, const SceneTraits& traits, const HrptPathTracerConstants& constants,
                             float4* const* planes, uint32_t planeMask, uint32_t width, TileRect rect, hipStream_t stream, std::string& error,
                             const MotionArgs* motion = nullptr);
// hrpt_trace_radiance: radiance[i] = (L, 1) -- or, accumulate, (old.rgb + L, old.w + 1) -- of the path that starts as rays[i], by the render's
// kernels between wf_raygen_rays and wf_store_radiance (device arrays). Leaves the statistics, the plan and the timing state of renders alone.
hipError_t wavefront_radiance(WavefrontState& st, const SceneView& scene, const SceneTraits& traits, const HrptPathTracerConstants& constants,
                              const HrptRay* rays, float4* radiance, uint64_t count, bool accumulate, bool secondary, hipStream_t stream, std::string& error);
void wavefront_release(WavefrontState& st);
void wavefront_collect_timing(WavefrontState& st);   // call after the stream is synchronised; folds pending events into kernelMs
void wavefront_reset_timing(WavefrontState& st);
// Queue bytes per kernel class from the device counters (summed over the shards) and the record layout of the last render.
void wavefront_queue_bytes(const WavefrontState& st, const DeviceCounters& total, uint64_t& trace, uint64_t& shade, uint64_t& shadow);

} // namespace hrt

// pt_capi_internal.h -- what the pt_capi*.cpp files share: the context, the status / error plumbing, the exception guard and the way from
// the context's images to a stage's image struct.
// Host code of the C boundary only: no .hip file and no header a kernel includes may include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/hobbyrt_pt.h"
#include "bvh_build.h"
#include "bvh_build_gpu.h"
#include "pt_anim.h"
#include "pt_device_buffer.h"
#include "pt_kernels.h"
#include "pt_motion_records.h"
#include "pt_scene_records.h"
#include "pt_wavefront.h"

namespace hrt::capi {

using hrt::DeviceBuffer;                     // pt_device_buffer.h: the owner of one device allocation
using DeviceAllocations = std::vector<DeviceBuffer<void>>;

// The device copy of one animation on one context (hrpt_animate): the resolved tables, and the state its kernels write.
struct AnimDeviceCopy {
    AnimDeviceCopy() = default; AnimDeviceCopy(AnimDeviceCopy&&) = default; AnimDeviceCopy& operator=(AnimDeviceCopy&&) = default;   // move-only: it owns `allocations`
    const HrptAnimation* anim = nullptr; uint64_t serial = 0;
    DeviceAllocations allocations;
    anim::Tables tables{};
    uint32_t* groupFirst = nullptr; float* times = nullptr;
    float* trs = nullptr; float* worlds = nullptr; float* weights = nullptr; float* palette = nullptr;
    HrptPerInstanceData* records = nullptr;      // the closed instance range; equal to the context's host copy of it while recordsEpoch == instanceEpoch
    uint64_t recordsEpoch = 0;
};

// Buffers that live as long as the uploaded scene: free_scene drops them with one assignment.
struct PerSceneBuffers {
    // the device tables the first motion call (hrpt_render_motion_vectors) builds from the kept copies
    DeviceBuffer<MotionInst> dMotionInst;                                      // one record per instance: m_PrevWorld + the mesh's LOD-0 index offset
    DeviceBuffer<float> dMotionPositions; DeviceBuffer<uint32_t> dMotionIndices;   // object-space positions (12 B per vertex) and the index buffer
    bool motionInstStale = true, motionGeometryStale = true;                   // set by uploads / instance updates / rebuilds, cleared by the next motion call
    // deforming meshes (hrpt_update_vertices): the object-space positions of the previous frame, 3 floats per vertex; EMPTY = previous == current
    // (a context that never deforms pays nothing). The device copy is made by the next motion call (motionPositionsStale), like dMotionPositions.
    std::vector<float> keptPrevPositions; DeviceBuffer<float> dMotionPrevPositions; bool motionPositionsStale = true;
    DeviceBuffer<HrptVertexFloat> dSkinFloats;                                 // hrpt_update_vertices_skinned: the skinned float vertices between its two kernels, sized for the whole vertex buffer at first use
    DeviceBuffer<void> dDeformStaging;                                         // hrpt_update_vertices_device / _skinned: quantised records + the two status words, sized for the whole vertex buffer at first use
};

// What a stage allocates at first use, grows on demand and finds gone after a resize: hrpt_resize drops all of it with one assignment, and
// the stage's next call makes its part again at the new size. A stage with images of this kind adds them here and nowhere else.
struct StageImages {
    DeviceBuffer<float4> dDisplay;                   // hrpt_post_process
    DeviceBuffer<float4> dDenoiseScratch[2];         // the scratch pair of HRPT_DENOISE_OUTPUT_ONLY
    DeviceBuffer<float4> dModulation;                // demodulate / compose: the stored factor, written by hrpt_demodulate
    // temporal upscaling (hrpt_upscale): ping-pong history pair and the colour image, all of upscaleWidth x upscaleHeight (the DISPLAY size of
    // the last call, not the context's), re-allocated when the display size changes; [upscaleCur] is the history the last call wrote
    DeviceBuffer<float4> dUpscaleHistory[2], dUpscaled;
    uint32_t upscaleWidth = 0, upscaleHeight = 0; int upscaleCur = 0; bool upscaleValid = false;
    DeviceBuffer<float4> dProbeIrradiance;           // hrpt_probes_shade_gbuffer: the probe volume's irradiance at the first hits
    // deferred lighting (hrpt_deferred_lighting): shadow-ray and hit records of one light batch, and the two running-sum images of a multi-batch call
    DeviceBuffer<HrptRay> dDeferredRays; DeviceBuffer<HrptRayHit> dDeferredHits;
    DeviceBuffer<float4> dDeferredCarry[2];
    // traced indirect lighting (hrpt_indirect_lighting): the two resolved planes ([0] diffuse, [1] specular) and the ray and radiance records of one call
    DeviceBuffer<float4> dIndirect[2];
    DeviceBuffer<HrptRay> dIndirectRays; DeviceBuffer<float4> dIndirectRadiance;
    // resampled direct lighting (hrpt_restir_lighting): the ping-pong history (final reservoirs and their keys; [restirCur] is what the last
    // call wrote, read only while restirValid), the plane between the temporal and the spatial pass, and the ray and hit records of one trace
    DeviceBuffer<HrptRestirReservoir> dRestirReservoirs[2], dRestirScratch;
    DeviceBuffer<float4> dRestirKeys[2];
    DeviceBuffer<HrptRay> dRestirRays; DeviceBuffer<HrptRayHit> dRestirHits;
    int restirCur = 0; bool restirValid = false;
    // radiance cache (hrpt_rcache_indirect): the served plane, and the surface, cached-radiance and voxel-size records of one call (its ray and
    // radiance records are dIndirectRays / dIndirectRadiance)
    DeviceBuffer<float4> dRcacheServed, dRcacheCached;
    DeviceBuffer<HrptRcacheSurface> dRcacheSurfaces; DeviceBuffer<float> dRcacheVoxel;
};

// Images of width * height float4. The members named here are the ones hrpt_resize makes again at the new size, zeroed and without
// history (the G-buffer planes, the motion plane and the temporal pair only where a call has requested them); `stage` it drops.
struct PerSizeImages {
    DeviceBuffer<float4> dAccum, dOutput;
    DeviceBuffer<float4> dGBuffer[HRPT_GB_PLANES];   // first-hit G-buffer planes (hrpt_render_gbuffer): allocated by the first call that requests one
    DeviceBuffer<float4> dMotion;                    // first-hit motion vectors (hrpt_render_motion_vectors)
    DeviceBuffer<float4> dTemporal[2];               // temporal accumulation (hrpt_temporal_accumulate): ping-pong history pair, allocated by the first call
    int temporalCur = 0; bool temporalValid = false; // [temporalCur] is the history image the last hrpt_temporal_accumulate wrote
    StageImages stage;
};

// Buffers that live as long as the context.
struct PerContextBuffers {
    DeviceBuffer<uint32_t> dHistogram; DeviceBuffer<float> dExposure;   // persistent exposure buffer (HDRRenderer m_RG_ExposureBuffer)
    DeviceBuffer<uint32_t> dBloomDown, dBloomUp;                        // bloom pyramids (packed R11G11B10_FLOAT), sized by the last bloom call
    DeviceBuffer<float> dDenoiseTile;                // the default noise tile, uploaded by the first denoise call of the context
    DeviceBuffer<DeviceCounters> dCounters;
};

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t ownStream = nullptr;         // created by hrpt_create; `stream` may be redirected by hrpt_set_stream
    std::string err;
    // scene
    DeviceAllocations allocations;           // scene-lifetime device allocations
    DeviceAllocations bvhAllocations;        // acceleration structure of the host builder + per-instance records: replaced by hrpt_update_instances
    DeviceBuffer<GpuNodeQ> nodesQ;           // quantised copy of the flat 4-wide tree (pt_scene_records.h GpuNodeQ), kept across rebuilds
    uint32_t nodes4Capacity = 0;             // records behind view.nodes4 when it is the GPU builder's buffer (0: allocated to size), for hrpt_selftest_read_bvh
    std::unique_ptr<GpuBvhBuilder> gpuBuilder;   // GPU builders: geometry + build buffers stay on the device for rebuilds
    std::unique_ptr<GpuBvhBuilder> tlasBuilder; uint32_t tlasBuilderInstances = 0;   // two-level structure: the tree over the instances, built on the GPU (build_two_level)
    // host copy of what a rebuild needs (the reference's Scene keeps the same vectors: m_InstanceData, m_Vertices, m_Indices, m_MeshData)
    std::vector<HrptVertexQuantized> keptVertices; std::vector<uint32_t> keptIndices; std::vector<HrptMeshData> keptMeshData;
    std::vector<HrptPerInstanceData> keptInstances; std::vector<HrptMaterialConstants> keptMaterials; std::vector<HrptGPULight> keptLights;
    size_t lightCapacity = 0;                // entries the device light buffer can hold (hrpt_update_lights may grow it)
    SceneView view{};
    bool haveScene = false;
    uint32_t bvhNodes = 0, bvhTris = 0;
    PerSceneBuffers perScene;
    // images
    uint32_t width = 0, height = 0;
    PerSizeImages perSize;
    PerContextBuffers perContext;
    uint32_t bloomTailTexels = 0;            // HRPT_BLOOM_FUSED_TAIL: levels of at most this many texels run in one workgroup's LDS (0 = one kernel per pass, the measured-faster default)
    uint32_t deferredLightBatch = 0;         // HRPT_DEFERRED_LIGHT_BATCH: lights per pass of hrpt_deferred_lighting, 1..16 (0 = min(m_LightCount, 4))
    bool restirGlobalLights = false;        // HRPT_RESTIR_GLOBAL_LIGHTS: restir_initial gathers its candidates' light records from global memory whatever the count (false = from LDS up to HRPT_RESTIR_LDS_MAX_LIGHTS; same bits)
    bool upscaleStaged = false;            // HRPT_UPSCALE_STAGED: the upscale kernel serves its current-frame taps from an LDS-staged window (false = global gathers, the measured-faster default)
    hipEvent_t evStart = nullptr, evStop = nullptr;
    bool timed = false;
    WavefrontState wf;
    SceneTraits traits;
    int bvhBuilder = HRPT_BVH_BUILDER_AUTO;       // hrpt_set_bvh_builder
    int accelStructure = HRPT_ACCEL_AUTO;         // hrpt_set_acceleration_structure
    BuiltTwoLevel* twoLevel = nullptr;            // two-level scenes: host copy (hrpt_update_instances rebuilds the instance tree from it)
    DeviceAllocations meshAllocations;            // ... and the device copies of the per-mesh arrays, which survive instance updates
    uint32_t megakernelFallbacks = 0;             // renders that wanted the wavefront pipeline but could not use it (HrptStats)
    HrptBuildInfo buildInfo{};
    std::vector<AnimDeviceCopy> animations;       // hrpt_animate: one device copy per animation seen, until hrpt_animation_release / hrpt_destroy
    uint64_t instanceEpoch = 1;                   // bumped whenever keptInstances changes
};

} // namespace hrt::capi

struct HrptContext : hrt::capi::Context {};

namespace hrt::capi {

// Records the message (on the context, or for hrpt_last_error(NULL) without one) and passes the code through.
int fail(HrptContext* ctx, int code, const std::string& msg);
inline int hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? HRPT_ERR_OUT_OF_MEMORY : HRPT_ERR_HIP; }
#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(ctx, hip_status(e_), std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define HRPT_TRY(expr) do { int r_ = (expr); if (r_ != HRPT_OK) return r_; } while (0)      // pass a failed status on (fail() has set the message)

// No C++ exception crosses the C boundary: host-side allocation failures (std::bad_alloc on very large scenes) become status codes. Every
// exported function that can allocate on the host (a std::vector, a std::string for fail()) is a function-try-block that ends in
// `catch (...) { return caught(c, "hrpt_x"); }`: caught() rethrows the exception in flight and is the one place that maps it.
inline int caught(HrptContext* c, const char* name)
{
    try { throw; }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, std::string(name) + ": host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(name) + ": " + e.what()); }
}

// The host executors (the *_host entry points, which take no context) keep a mapping of their own: what they may throw is their buffers
// and their threads.
template <class Fn> int run_host(const char* what, Fn fn)
{
    try { fn(); }
    catch (const std::bad_alloc&) { return fail(nullptr, HRPT_ERR_OUT_OF_MEMORY, std::string(what) + ": out of memory"); }
    catch (const std::system_error& e) { return fail(nullptr, HRPT_ERR_UNSUPPORTED, std::string(what) + ": " + e.what()); }
    return HRPT_OK;
}
// Threads of a host executor: 0 or less = one per hardware thread up to 16; at most 256.
inline int host_threads(int nthreads)
{
    if (nthreads <= 0) { nthreads = (int)std::thread::hardware_concurrency(); if (nthreads > 16) nthreads = 16; }
    if (nthreads < 1) nthreads = 1;
    return nthreads > 256 ? 256 : nthreads;
}

// The scene's two-level structure needs more stack than the thread-per-query kernels have (bvh_build.h kPrivateStackDepth): the calls that
// would run one of them refuse.
static_assert(kPrivateStackDepth == 64u, "the refusal messages say \"64-entry stack\"; tests match on them");
inline bool exceeds_private_stack(const SceneTraits& traits) { return traits.twoLevelStackNeed > kPrivateStackDepth; }

inline bool size_ok(uint32_t width, uint32_t height) { return !(width == 0 || height == 0 || width > 65535u || height > 65535u); }
int realloc_image(HrptContext* c, DeviceBuffer<float4>& image, size_t bytes);      // a fresh image, zeroed on the context stream
int read_image(HrptContext* c, const float4* src, float* dst, size_t bytes, const char* what);

// ---- from the context's images to a stage's image struct ----
// An image as the stages' image structs take it, a plain array of floats: the one place that recasts.
inline const float* floats(const DeviceBuffer<float4>& image) { return reinterpret_cast<const float*>(image.get()); }
inline float* floats(DeviceBuffer<float4>& image) { return reinterpret_cast<float*>(image.get()); }
// The G-buffer planes of `gbMask` (bits 1 << HRPT_GB_*), and the motion plane if `motion`, must have been requested from a G-buffer or
// motion call: the message names `what`, the first plane that is missing and the planeMask that would fill them all.
int planes_requested(HrptContext* c, const char* what, uint32_t gbMask, bool motion);
// c->stream redirected for a scope: the public trace calls a stage is composed of then run on the stage's stream.
class ScopedStream {
public:
    ScopedStream(HrptContext* c, hipStream_t stream) : c_(c), saved_(c->stream) { c->stream = stream; }
    ~ScopedStream() { c_->stream = saved_; }
    ScopedStream(const ScopedStream&) = delete; ScopedStream& operator=(const ScopedStream&) = delete;
private:
    HrptContext* c_; hipStream_t saved_;
};

// Device room for `count` records owned by `owner` (default: the scene's allocation list), with host[skip .. count) copied into place:
// the records in front of `skip` are the caller's to write on the device.
template <class T>
int upload_writable(HrptContext* c, const T* host, size_t count, T** dev, DeviceAllocations* owner = nullptr, size_t skip = 0)
{
    *dev = nullptr;
    size_t bytes = count * sizeof(T);
    DeviceBuffer<void> p;
    HIP_TRY(c, p.alloc(bytes ? bytes : 16));
    T* d = static_cast<T*>(p.get());
    (owner ? *owner : c->allocations).push_back(std::move(p));
    if (count > skip) HIP_TRY(c, hipMemcpyAsync(d + skip, host + skip, (count - skip) * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *dev = d;
    return HRPT_OK;
}
// A device copy of host[0 .. count).
template <class T>
int upload(HrptContext* c, const T* host, size_t count, const T** dev, DeviceAllocations* owner = nullptr)
{
    T* d = nullptr;
    const int r = upload_writable(c, host, count, &d, owner);
    *dev = d;
    return r;
}

// pt_capi_scene.cpp
int build_acceleration(HrptContext* c, const HrptSceneDesc& s, uint64_t sceneTris, SceneView& v, bool firstBuild, bool refit = false);
HrptSceneDesc kept_scene_desc(HrptContext* c);
uint64_t kept_triangle_count(const HrptContext* c);
int update_instances_impl(HrptContext* c, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count, bool refit);
void free_scene(HrptContext* c);
void refresh_traits(HrptContext* c);

} // namespace hrt::capi

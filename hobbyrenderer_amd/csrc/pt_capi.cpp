// pt_capi.cpp -- implementation of the C ABI declared in include/hobbyrt_pt.h. Host code only:
// context/stream ownership, scene upload (copies), BVH build, per-dispatch constants exactly as
// PathTracerRenderer::Render fills them (/root/reference/src/PathTracerRenderer.cpp:58-75), launches.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <stdexcept>
#include <limits>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/hobbyrt_pt.h"
#include "bvh_build.h"
#include "bvh_build_gpu.h"
#include "pt_deform.h"
#include "pt_skin.h"
#include "pt_anim.h"
#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_motion.h"
#include "pt_wavefront.h"

using namespace hrt;

// The device copy of one animation on one context (hrpt_animate): the resolved tables, and the state its kernels write.
struct AnimDeviceCopy {
    const HrptAnimation* anim = nullptr; uint64_t serial = 0;
    std::vector<void*> allocations;
    anim::Tables tables{};
    uint32_t* groupFirst = nullptr; float* times = nullptr;
    float* trs = nullptr; float* worlds = nullptr; float* weights = nullptr; float* palette = nullptr;
    HrptPerInstanceData* records = nullptr;      // the closed instance range; equal to the context's host copy of it while recordsEpoch == instanceEpoch
    uint64_t recordsEpoch = 0;
};

struct HrptContext {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t ownStream = nullptr;         // created by hrpt_create; `stream` may be redirected by hrpt_set_stream
    std::string err;
    // scene
    std::vector<void*> allocations;          // scene-lifetime device allocations
    std::vector<void*> bvhAllocations;       // acceleration structure of the host builder + per-instance records: replaced by hrpt_update_instances
    GpuNodeQ* nodesQ = nullptr; size_t nodesQCapacity = 0;    // quantised copy of the flat 4-wide tree (pt_device.h GpuNodeQ), kept across rebuilds
    uint32_t nodes4Capacity = 0;             // records behind view.nodes4 when it is the GPU builder's buffer (0: allocated to size), for hrpt_selftest_read_bvh
    GpuBvhBuilder* gpuBuilder = nullptr;     // GPU builders: geometry + build buffers stay on the device for rebuilds
    GpuBvhBuilder* tlasBuilder = nullptr; uint32_t tlasBuilderInstances = 0;   // two-level structure: the tree over the instances, built on the GPU (build_two_level)
    // host copy of what a rebuild needs (the reference's Scene keeps the same vectors: m_InstanceData, m_Vertices, m_Indices, m_MeshData)
    std::vector<HrptVertexQuantized> keptVertices; std::vector<uint32_t> keptIndices; std::vector<HrptMeshData> keptMeshData;
    std::vector<HrptPerInstanceData> keptInstances; std::vector<HrptMaterialConstants> keptMaterials; std::vector<HrptGPULight> keptLights;
    size_t lightCapacity = 0;                // entries the device light buffer can hold (hrpt_update_lights may grow it)
    SceneView view{};
    bool haveScene = false;
    uint32_t bvhNodes = 0, bvhTris = 0;
    // images
    uint32_t width = 0, height = 0;
    float4* dAccum = nullptr; float4* dOutput = nullptr; float4* dDisplay = nullptr;
    uint32_t* dHistogram = nullptr; float* dExposure = nullptr;   // persistent exposure buffer (HDRRenderer m_RG_ExposureBuffer)
    uint32_t* dBloomDown = nullptr; uint32_t* dBloomUp = nullptr; size_t bloomWords = 0;   // bloom pyramids (packed R11G11B10_FLOAT), sized by the last bloom call
    uint32_t bloomTailTexels = 0;            // HRPT_BLOOM_FUSED_TAIL: levels of at most this many texels run in one workgroup's LDS (0 = one kernel per pass, the measured-faster default)
    float4* dGBuffer[HRPT_GB_PLANES] = {};   // first-hit G-buffer planes (hrpt_render_gbuffer): allocated by the first call that requests one, re-allocated by hrpt_resize
    // first-hit motion vectors (hrpt_render_motion_vectors): the plane, and the device tables the first motion call builds from the kept copies
    float4* dMotion = nullptr;
    MotionInst* dMotionInst = nullptr; size_t motionInstCapacity = 0;          // one record per instance: m_PrevWorld + the mesh's LOD-0 index offset
    float* dMotionPositions = nullptr; uint32_t* dMotionIndices = nullptr;     // object-space positions (12 B per vertex) and the index buffer
    bool motionInstStale = true, motionGeometryStale = true;                   // set by uploads / instance updates / rebuilds, cleared by the next motion call
    // deforming meshes (hrpt_update_vertices): the object-space positions of the previous frame, 3 floats per vertex; EMPTY = previous == current
    // (a context that never deforms pays nothing). The device copy is made by the next motion call (motionPositionsStale), like dMotionPositions.
    std::vector<float> keptPrevPositions; float* dMotionPrevPositions = nullptr; bool motionPositionsStale = true;
    HrptVertexFloat* dSkinFloats = nullptr;                                    // hrpt_update_vertices_skinned: the skinned float vertices between its two kernels, sized for the whole vertex buffer at first use
    void* dDeformStaging = nullptr; size_t deformStagingBytes = 0;             // hrpt_update_vertices_device / _skinned: quantised records + the two status words, sized for the whole vertex buffer at first use
    // temporal accumulation (hrpt_temporal_accumulate): ping-pong history pair, allocated by the first call; [temporalCur] is the image the last call wrote
    float4* dTemporal[2] = {}; int temporalCur = 0; bool temporalValid = false;
    // denoise (hrpt_denoise): the default noise tile (uploaded by the first denoise call of the context) and the scratch pair of HRPT_DENOISE_OUTPUT_ONLY
    float* dDenoiseTile = nullptr; float4* dDenoiseScratch[2] = {};
    // demodulate / compose (hrpt_demodulate): the stored factor, allocated by the first hrpt_demodulate, dropped by hrpt_resize
    float4* dModulation = nullptr;
    DeviceCounters* dCounters = nullptr;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    bool timed = false;
    WavefrontState wf;
    SceneTraits traits;
    int bvhBuilder = HRPT_BVH_BUILDER_AUTO;       // hrpt_set_bvh_builder
    int accelStructure = HRPT_ACCEL_AUTO;         // hrpt_set_acceleration_structure
    BuiltTwoLevel* twoLevel = nullptr;            // two-level scenes: host copy (hrpt_update_instances rebuilds the instance tree from it)
    std::vector<void*> meshAllocations;           // ... and the device copies of the per-mesh arrays, which survive instance updates
    uint32_t megakernelFallbacks = 0;             // renders that wanted the wavefront pipeline but could not use it (HrptStats)
    HrptBuildInfo buildInfo{};
    std::vector<AnimDeviceCopy> animations;       // hrpt_animate: one device copy per animation seen, until hrpt_animation_release / hrpt_destroy
    uint64_t instanceEpoch = 1;                   // bumped whenever keptInstances changes
};

static std::mutex g_errMutex;
static std::string g_createError;

static int fail(HrptContext* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    else { std::lock_guard<std::mutex> l(g_errMutex); g_createError = msg; }
    return code;
}
#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(ctx, e_ == hipErrorOutOfMemory ? HRPT_ERR_OUT_OF_MEMORY : HRPT_ERR_HIP, \
                                          std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)
#define HRPT_TRY(expr) do { int r_ = (expr); if (r_ != HRPT_OK) return r_; } while (0)      // pass a failed status on (fail() has set the message)

static bool size_ok(uint32_t width, uint32_t height) { return !(width == 0 || height == 0 || width > 65535u || height > 65535u); }

// Per-context images of width * height float4. hipFree waits for work in flight.
static void free_image(float4*& image) { if (image) { (void)hipFree(image); image = nullptr; } }
static int realloc_image(HrptContext* c, float4*& image, size_t bytes)      // a fresh image, zeroed on the context stream
{
    free_image(image);
    HIP_TRY(c, hipMalloc((void**)&image, bytes));
    HIP_TRY(c, hipMemsetAsync(image, 0, bytes, c->stream));
    return HRPT_OK;
}

// DirectX::PackedVector::XMConvertFloatToHalf (round to nearest even), src/CommonResources.cpp:553
static uint16_t float_to_half(float f)
{
    uint32_t x; memcpy(&x, &f, 4);
    uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u | ((x > 0x7f800000u) ? (0x200u | ((x >> 13) & 0x3ffu)) : 0u));
    if (x < 0x38800000u) {
        if (x < 0x33000000u) return (uint16_t)sign;
        uint32_t shift = 126u - (x >> 23);
        uint32_t m = (x & 0x7fffffu) | 0x800000u;
        uint32_t h = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
        if (rem > halfway || (rem == halfway && (h & 1u))) ++h;
        return (uint16_t)(sign | h);
    }
    uint32_t r = x + 0xfffu + ((x >> 13) & 1u);
    return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}

static void free_acceleration(HrptContext* c, bool keepGpuBuilder)
{
    for (void* p : c->bvhAllocations) (void)hipFree(p);
    c->bvhAllocations.clear();
    if (!keepGpuBuilder) {
        delete c->gpuBuilder; c->gpuBuilder = nullptr;
        delete c->tlasBuilder; c->tlasBuilder = nullptr; c->tlasBuilderInstances = 0;
        for (void* p : c->meshAllocations) (void)hipFree(p);
        c->meshAllocations.clear();
        delete c->twoLevel; c->twoLevel = nullptr;
    }
}

static void free_motion_tables(HrptContext* c)
{
    if (c->dMotionInst) (void)hipFree(c->dMotionInst);
    if (c->dMotionPositions) (void)hipFree(c->dMotionPositions);
    if (c->dMotionIndices) (void)hipFree(c->dMotionIndices);
    if (c->dMotionPrevPositions) (void)hipFree(c->dMotionPrevPositions);
    if (c->dDeformStaging) (void)hipFree(c->dDeformStaging);
    if (c->dSkinFloats) (void)hipFree(c->dSkinFloats);
    c->dMotionInst = nullptr; c->motionInstCapacity = 0; c->dMotionPositions = nullptr; c->dMotionIndices = nullptr;
    c->dMotionPrevPositions = nullptr; c->dDeformStaging = nullptr; c->dSkinFloats = nullptr; c->deformStagingBytes = 0; c->keptPrevPositions.clear();
    c->motionInstStale = c->motionGeometryStale = c->motionPositionsStale = true;
}

static void free_scene(HrptContext* c)
{
    free_acceleration(c, false);
    free_motion_tables(c);
    for (void* p : c->allocations) (void)hipFree(p);
    c->allocations.clear();
    if (c->nodesQ) { (void)hipFree(c->nodesQ); c->nodesQ = nullptr; c->nodesQCapacity = 0; }
    c->keptVertices.clear(); c->keptIndices.clear(); c->keptMeshData.clear(); c->keptInstances.clear(); c->keptMaterials.clear(); c->keptLights.clear(); c->lightCapacity = 0;
    c->haveScene = false;
    ++c->instanceEpoch;
    memset(&c->view, 0, sizeof c->view);
}

static void free_animation_copy(AnimDeviceCopy& a)
{
    for (void* p : a.allocations) (void)hipFree(p);
    a = AnimDeviceCopy{};
}

template <class T>
static int upload(HrptContext* c, const T* host, size_t count, const T** dev, std::vector<void*>* owner = nullptr)
{
    *dev = nullptr;
    size_t bytes = count * sizeof(T);
    void* p = nullptr;
    HIP_TRY(c, hipMalloc(&p, bytes ? bytes : 16));
    (owner ? *owner : c->allocations).push_back(p);
    if (bytes) HIP_TRY(c, hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, c->stream));
    *dev = static_cast<const T*>(p);
    return HRPT_OK;
}

extern "C" {

int hrpt_create(const HrptDeviceDesc* desc, HrptContext** out)
{
    if (!desc || !out) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_create: null argument");
    *out = nullptr;
    if (desc->abiVersion != HRPT_ABI_VERSION) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_create: ABI version mismatch");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, HRPT_ERR_NO_DEVICE, "hrpt_create: no HIP device available (the gfx950 kernels are the only backend)");
    if (desc->deviceOrdinal < 0 || desc->deviceOrdinal >= n) return fail(nullptr, HRPT_ERR_NO_DEVICE, "hrpt_create: device ordinal out of range");
    HrptContext* c = new HrptContext();
    c->device = desc->deviceOrdinal;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->evStart) != hipSuccess || hipEventCreate(&c->evStop) != hipSuccess ||
        hipMalloc((void**)&c->dCounters, sizeof(DeviceCounters) * kCounterShards) != hipSuccess ||
        hipMemset(c->dCounters, 0, sizeof(DeviceCounters) * kCounterShards) != hipSuccess) {
        int r = fail(nullptr, HRPT_ERR_HIP, "hrpt_create: stream/event/counter creation failed");
        delete c;
        return r;
    }
    c->ownStream = c->stream;
    if (const char* e = getenv("HRPT_WF_SEGMENT_SHIFT")) c->wf.knobs.segmentShift = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_WF_SEGMENT_SIZE")) c->wf.knobs.segmentSize = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_WF_BLOCKS_PER_CU")) c->wf.knobs.blocksPerCu = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_WF_EXTEND_BLOCKS_PER_CU")) c->wf.knobs.extendBlocksPerCu = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_WF_REFILL_MIN")) c->wf.knobs.refillMin = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_WF_BVH_WIDTH")) c->wf.knobs.bvhWidth = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_BVH_BUILDER")) c->bvhBuilder = (strcmp(e, "ploc") == 0 || strcmp(e, "2") == 0) ? HRPT_BVH_BUILDER_GPU_PLOC : ((strcmp(e, "gpu") == 0 || strcmp(e, "lbvh") == 0 || strcmp(e, "1") == 0) ? HRPT_BVH_BUILDER_GPU_LBVH : ((strcmp(e, "auto") == 0 || strcmp(e, "3") == 0) ? HRPT_BVH_BUILDER_AUTO : HRPT_BVH_BUILDER_HOST_SAH));
    if (const char* e = getenv("HRPT_WF_PAD_LDS")) c->wf.knobs.padLdsBytes = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_WF_DRAIN_SEGMENTS")) c->wf.knobs.drainSegments = atoi(e) != 0;
    if (const char* e = getenv("HRPT_WF_SERIAL_SHADOW")) c->wf.knobs.serialShadow = atoi(e) != 0;
    if (const char* e = getenv("HRPT_WF_SHADOW_PATH")) c->wf.knobs.shadowPath = atoi(e);
    if (const char* e = getenv("HRPT_WF_SHADE_SORT")) c->wf.knobs.shadeSort = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("HRPT_WF_SLIM_SHADOW")) c->wf.knobs.noSlimShadow = atoi(e) == 0;
    if (const char* e = getenv("HRPT_WF_FUSED_PRIMARY")) c->wf.knobs.noFusedPrimary = atoi(e) == 0;
    if (const char* e = getenv("HRPT_WF_FUSED_BOUNCE0")) c->wf.knobs.noFusedBounce0 = atoi(e) == 0;
    if (const char* e = getenv("HRPT_WF_SHADE_LDS_TABLES")) c->wf.knobs.noShadeLdsTables = atoi(e) == 0;
    if (const char* e = getenv("HRPT_WF_NODE_LOOP_MIN")) c->wf.knobs.nodeLoopMin = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_BLOOM_FUSED_TAIL")) { const int v = atoi(e); c->bloomTailTexels = v == 1 ? 8192u : (v > 0 ? (uint32_t)v : 0u); }
    *out = c;
    return HRPT_OK;
}

void hrpt_destroy(HrptContext* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_scene(c);
    for (AnimDeviceCopy& a : c->animations) free_animation_copy(a);
    wavefront_release(c->wf);
    if (c->dAccum) (void)hipFree(c->dAccum);
    if (c->dOutput) (void)hipFree(c->dOutput);
    if (c->dDisplay) (void)hipFree(c->dDisplay);
    for (float4* plane : c->dGBuffer) if (plane) (void)hipFree(plane);
    if (c->dMotion) (void)hipFree(c->dMotion);
    for (float4* image : c->dTemporal) if (image) (void)hipFree(image);
    for (float4* image : c->dDenoiseScratch) if (image) (void)hipFree(image);
    if (c->dDenoiseTile) (void)hipFree(c->dDenoiseTile);
    if (c->dModulation) (void)hipFree(c->dModulation);
    if (c->dHistogram) (void)hipFree(c->dHistogram);
    if (c->dExposure) (void)hipFree(c->dExposure);
    if (c->dBloomDown) (void)hipFree(c->dBloomDown);
    if (c->dBloomUp) (void)hipFree(c->dBloomUp);
    if (c->dCounters) (void)hipFree(c->dCounters);
    if (c->evStart) (void)hipEventDestroy(c->evStart);
    if (c->evStop) (void)hipEventDestroy(c->evStop);
    if (c->ownStream) (void)hipStreamDestroy(c->ownStream);
    delete c;
}

const char* hrpt_last_error(const HrptContext* c)
{
    if (c) return c->err.c_str();
    std::lock_guard<std::mutex> l(g_errMutex);
    static thread_local std::string copy;
    copy = g_createError;
    return copy.c_str();
}

// The acceleration structure + the records derived from instance transforms (Scene::BuildAccelerationStructures, src/Scene.cpp:67-214),
// written into `v`. First build of a scene or a rebuild after hrpt_update_instances (the GPU builder then keeps its device-resident
// geometry and buffers).
// Two-level structure: asked for, or (AUTO) large and heavily instanced
static bool two_level_wanted(const HrptContext* c, const HrptSceneDesc& s, uint64_t sceneTris)
{
    int want = c->accelStructure;
    if (const char* e = getenv("HRPT_ACCEL_STRUCTURE")) { const int v = atoi(e); if (v >= HRPT_ACCEL_AUTO && v <= HRPT_ACCEL_TWO_LEVEL) want = v; }
    if (want == HRPT_ACCEL_FLAT || s.instanceCount == 0) return false;
    if (want == HRPT_ACCEL_TWO_LEVEL) return true;
    std::vector<uint8_t> used(s.meshDataCount, 0); uint32_t distinct = 0;
    for (uint32_t i = 0; i < s.instanceCount; ++i) if (!used[s.instances[i].m_MeshDataIndex]) { used[s.instances[i].m_MeshDataIndex] = 1; ++distinct; }
    // scenes with non-opaque instances: measured cross-over against the flat structure at ~16 M world triangles (instanced alpha-tested + glass
    // meshes: 7.6 M triangles 35.5 vs 32.3 ms, 30 M 38 vs 46 ms; the two-level candidate buffer holds 4 entries with the instance next to the triangle)
    bool nonOpaque = false;
    for (uint32_t i = 0; i < s.instanceCount && !nonOpaque; ++i) nonOpaque = s.materials[s.instances[i].m_MaterialIndex].m_AlphaMode != HRPT_ALPHA_MODE_OPAQUE;
    return sceneTris >= (nonOpaque ? (16ull << 20) : (2ull << 20)) && (uint64_t)s.instanceCount >= 8ull * distinct;
}

// instancesOnly: the mesh trees of c->twoLevel are kept (hrpt_update_instances)
// kTwoLevelDoesNotFit: the scene cannot be held in this form (an instance with a singular world matrix -- a mesh flattened to a plane --, trees
// too deep): the caller builds the flat structure instead, which has no such limits
constexpr int kTwoLevelDoesNotFit = 1;
// The tree over the instances on the GPU (the reference rebuilds its TLAS on the GPU every frame, src/CommonRenderers.cpp:234-246): the
// builder's box mode over the instances' padded world boxes, then launch_tlas_fixup writes the nodes, leaves turned into instance references,
// to the front of the scene's node array. The builder and its buffers stay on the device: a rebuild (hrpt_update_instances) uploads 24 bytes
// per instance and runs the kernels. false: not built (a device error, a tree too deep): the caller builds the tree on the host instead.
static bool build_instance_tree_on_gpu(HrptContext* c, uint32_t instanceCount, const std::vector<float>& boxes, bool rebuild, bool refit, GpuNode4* dstNodes, uint32_t& depth4Levels)
{
    std::string gerr;
    if (!c->tlasBuilder || c->tlasBuilderInstances != instanceCount) {
        delete c->tlasBuilder; c->tlasBuilder = new GpuBvhBuilder(); c->tlasBuilderInstances = 0;
        if (c->tlasBuilder->prepare_boxes(instanceCount, c->stream, gerr) != hipSuccess) { delete c->tlasBuilder; c->tlasBuilder = nullptr; return false; }
        c->tlasBuilderInstances = instanceCount;
    }
    GpuBuiltBvh g;
    // Hierarchy: PLOC at upload, the Morton radix tree for rebuilds (hrpt_update_instances) unless a GPU builder was asked for by name. Measured on
    // 16 384 / 65 536 instances: the radix tree is built in 0.45 ms of device time against 1.9 / 2.1 ms and traverses 0 / 2 % slower, so a host that
    // moves instances every frame comes out ahead with it (update 1.8 / 4.0 ms against 3.0 / 5.5 ms), a static scene with PLOC.
    bool ploc = c->bvhBuilder == HRPT_BVH_BUILDER_GPU_PLOC || (c->bvhBuilder != HRPT_BVH_BUILDER_GPU_LBVH && !rebuild);
    if (const char* e = getenv("HRPT_TLAS_LBVH")) ploc = atoi(e) == 0;
    const hipError_t ge = (rebuild && refit && c->tlasBuilder->can_refit()) ? c->tlasBuilder->refit_boxes(boxes.data(), c->stream, g, gerr)      // hrpt_refit_instances
                                                                              : c->tlasBuilder->build_boxes(boxes.data(), ploc, kTraversalStackDepth, c->stream, g, gerr);
    if (ge != hipSuccess || g.maxDepth + 2 > kTraversalStackDepth || g.node4Count == 0 || g.node4Count > instanceCount) return false;
    if (launch_tlas_fixup(g.nodes4, g.node4Count, g.leafOrder, dstNodes, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return false;
    depth4Levels = g.maxDepth4 + 1;
    c->buildInfo.deviceBuildMs = g.deviceMs; c->buildInfo.usedBuilder = (g.ploc ? HRPT_BVH_BUILDER_GPU_PLOC : HRPT_BVH_BUILDER_GPU_LBVH) | (g.refitted ? HRPT_BVH_BUILDER_REFITTED : 0u);
    return true;
}

static int build_two_level(HrptContext* c, const HrptSceneDesc& s, SceneView& v, bool instancesOnly, bool refit)
{
    std::string berr; int r;
    const bool timing = getenv("HRPT_BUILD_TIMING") != nullptr; auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!timing) return; (void)hipStreamSynchronize(c->stream); auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[two-level] %-22s %7.3f ms\n", what, std::chrono::duration<float, std::milli>(t - tp).count()); tp = t; };
    // who builds the tree over the instances: the GPU from 1024 instances on (host SAH: 2 / 6 / 16 ms for 4 096 / 16 384 / 65 536 instances, the GPU
    // ~1 ms), unless the host builder was asked for (hrpt_set_bvh_builder) or HRPT_TLAS_BUILDER says otherwise
    bool gpuTree = s.instanceCount >= 1024 && c->bvhBuilder != HRPT_BVH_BUILDER_HOST_SAH;
    if (const char* e = getenv("HRPT_TLAS_BUILDER")) gpuTree = s.instanceCount >= 8 && (strcmp(e, "gpu") == 0 || strcmp(e, "1") == 0);
    lap("(entry)");
    std::vector<float> boxes;
    std::vector<float>* wantBoxes = gpuTree ? &boxes : nullptr;      // set: the node range of the instance tree is reserved and left empty
    if (!instancesOnly) { delete c->twoLevel; c->twoLevel = new BuiltTwoLevel(); }
    if (!(instancesOnly ? rebuild_two_level_instances(s, *c->twoLevel, berr, wantBoxes) : build_scene_two_level(s, *c->twoLevel, berr, wantBoxes))) {
        if (berr.find("singular") != std::string::npos) return kTwoLevelDoesNotFit;
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
    }
    lap("host records");
    BuiltTwoLevel& b = *c->twoLevel;
    if (two_level_stack_need(b) > 128u) return kTwoLevelDoesNotFit;
    if (!instancesOnly) {
        const HostTri* dt; const HostTriAttr* da; const HostTriTangent* dtg;
        if ((r = upload(c, b.tris.data(), b.tris.size(), &dt, &c->meshAllocations)) != HRPT_OK) return r;
        if ((r = upload(c, b.attrs.data(), b.attrs.size(), &da, &c->meshAllocations)) != HRPT_OK) return r;
        v.tris = reinterpret_cast<const GpuTri*>(dt); v.triCount = (uint32_t)b.tris.size(); v.attrs = reinterpret_cast<const GpuTriAttr*>(da);
        v.tangents = nullptr;
        if (!b.tangents.empty()) {
            if ((r = upload(c, b.tangents.data(), b.tangents.size(), &dtg, &c->meshAllocations)) != HRPT_OK) return r;
            v.tangents = reinterpret_cast<const GpuTriTangent*>(dtg);
        }
    }
    const HostNode4* dn4; const HostInstance* di; const HostInstShade* dis;
    if (b.nodes4.size() >= kMaxStructureNodes) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: more than 2^25 nodes (32-bit node offsets in the traversal kernels)");
    if (gpuTree) {      // the reserved range at the front is written on the device (launch_tlas_fixup): only the mesh trees behind it cross PCIe
        void* p = nullptr;
        HIP_TRY(c, hipMalloc(&p, b.nodes4.size() * sizeof(HostNode4)));
        c->bvhAllocations.push_back(p);
        dn4 = static_cast<const HostNode4*>(p);
        HIP_TRY(c, hipMemcpyAsync(static_cast<HostNode4*>(p) + b.tlasNodeCount, b.nodes4.data() + b.tlasNodeCount, (b.nodes4.size() - b.tlasNodeCount) * sizeof(HostNode4), hipMemcpyHostToDevice, c->stream));
    } else if ((r = upload(c, b.nodes4.data(), b.nodes4.size(), &dn4, &c->bvhAllocations)) != HRPT_OK) return r;
    if ((r = upload(c, b.instances.data(), b.instances.size(), &di, &c->bvhAllocations)) != HRPT_OK) return r;
    if ((r = upload(c, b.instShade.data(), b.instShade.size(), &dis, &c->bvhAllocations)) != HRPT_OK) return r;
    lap("uploads");
    if (gpuTree) {
        uint32_t levels = 0;
        if (build_instance_tree_on_gpu(c, s.instanceCount, boxes, instancesOnly, refit, const_cast<GpuNode4*>(reinterpret_cast<const GpuNode4*>(dn4)), levels)) {
            b.maxDepth4Tlas = levels;
        } else {
            // the host builds it after all: same layout rules as ever (the reserved node range shrinks to the tree's size)
            for (void* p : c->bvhAllocations) (void)hipFree(p);
            c->bvhAllocations.clear();
            if (!rebuild_two_level_instances(s, b, berr)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
            if ((r = upload(c, b.nodes4.data(), b.nodes4.size(), &dn4, &c->bvhAllocations)) != HRPT_OK) return r;
            if ((r = upload(c, b.instances.data(), b.instances.size(), &di, &c->bvhAllocations)) != HRPT_OK) return r;
            if ((r = upload(c, b.instShade.data(), b.instShade.size(), &dis, &c->bvhAllocations)) != HRPT_OK) return r;
            gpuTree = false;
        }
    }
    lap("instance tree (GPU)");
    if (two_level_stack_need(b) > 128u) return kTwoLevelDoesNotFit;
    v.nodes = nullptr; v.nodeCount = b.tlasNodeCount; v.rootLeaf = b.tlasRootLeaf;      // nodeCount != 0: the walk starts at node4 0 (the instance tree)
    v.nodes4 = reinterpret_cast<const GpuNode4*>(dn4); v.node4Count = (uint32_t)b.nodes4.size(); v.nodesQ = nullptr;
    v.instances = reinterpret_cast<const GpuInstance*>(di); v.instanceCount = (uint32_t)b.instances.size();
    v.instShade = reinterpret_cast<const GpuInstShade*>(dis);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!gpuTree) c->buildInfo.usedBuilder = HRPT_BVH_BUILDER_HOST_SAH;      // (the mesh trees are the host's either way; usedBuilder names who built the tree over the instances)
    c->buildInfo.structure = HRPT_ACCEL_TWO_LEVEL;
    c->buildInfo.instanceNodeCount = b.tlasNodeCount; c->buildInfo.distinctMeshes = b.distinctMeshes;
    c->buildInfo.triangleCount = v.triCount; c->buildInfo.nodeCount = 0; c->buildInfo.node4Count = v.node4Count;
    c->buildInfo.maxDepth = 0; c->buildInfo.maxDepth4 = b.maxDepth4Tlas + b.maxDepth4Blas;
    c->bvhNodes = v.node4Count; c->bvhTris = v.triCount;
    c->traits.bvhMaxDepth = 0; c->traits.bvh4MaxDepth = b.maxDepth4Tlas + b.maxDepth4Blas; c->traits.twoLevelStackNeed = two_level_stack_need(b); c->traits.quantisedNodes = false;
    return HRPT_OK;
}

// refit (hrpt_refit_instances): where a GPU builder holds the hierarchy of the previous build, its boxes are recomputed instead of the tree rebuilt
static int build_acceleration(HrptContext* c, const HrptSceneDesc& s, uint64_t sceneTris, SceneView& v, bool firstBuild, bool refit = false)
{
    const auto t0 = std::chrono::steady_clock::now();
    std::string berr;
    int r;
    c->buildInfo = HrptBuildInfo{};
    c->buildInfo.requestedBuilder = (uint32_t)c->bvhBuilder;
    c->buildInfo.structure = HRPT_ACCEL_FLAT; c->nodes4Capacity = 0;
    const bool keepMeshTrees = !firstBuild && c->twoLevel != nullptr;       // hrpt_update_instances on a two-level scene
    free_acceleration(c, !firstBuild);
    if (keepMeshTrees || (firstBuild && two_level_wanted(c, s, sceneTris))) {
        r = build_two_level(c, s, v, keepMeshTrees, refit);
        if (r != kTwoLevelDoesNotFit) {
            c->buildInfo.buildMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            return r;
        }
        // flat after all: drop everything of the two-level form (a moved instance may have become singular: hrpt_update_instances ends up here too)
        free_acceleration(c, false);
        c->buildInfo.structure = HRPT_ACCEL_FLAT;
        firstBuild = true;
    }
    v.instances = nullptr; v.instanceCount = 0; c->traits.twoLevelStackNeed = 0;
    if (sceneTris >= kMaxStructureTriangles) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: too many triangles for the flat structure (2^32 / 48 = 89 M world-space triangles; instanced scenes can use HRPT_ACCEL_TWO_LEVEL)");
    uint32_t maxDepth = 0, maxDepth4 = 0;
    bool built = false;
    const int builder = c->bvhBuilder == HRPT_BVH_BUILDER_AUTO ? (sceneTris >= 65536 ? HRPT_BVH_BUILDER_GPU_PLOC : HRPT_BVH_BUILDER_HOST_SAH) : c->bvhBuilder;
    if (builder != HRPT_BVH_BUILDER_GPU_LBVH && builder != HRPT_BVH_BUILDER_GPU_PLOC) { delete c->gpuBuilder; c->gpuBuilder = nullptr; }
    if ((builder == HRPT_BVH_BUILDER_GPU_LBVH || builder == HRPT_BVH_BUILDER_GPU_PLOC) && sceneTris >= 8) {
        // the whole build runs on the device; only the per-instance adjugate rows (O(instances)) are prepared on the host
        GpuBuiltBvh g; std::string gerr;
        hipError_t ge = hipSuccess;
        if (!c->gpuBuilder) {
            c->gpuBuilder = new GpuBvhBuilder();
            ge = c->gpuBuilder->prepare(s, scene_needs_tangents(s), c->stream, gerr);
        }
        if (ge == hipSuccess) ge = (refit && !firstBuild && c->gpuBuilder->can_refit()) ? c->gpuBuilder->refit(s.instances, c->stream, g, gerr)
                                                                                          : c->gpuBuilder->build(s.instances, builder == HRPT_BVH_BUILDER_GPU_PLOC, kTraversalStackDepth, c->stream, g, gerr);
        if (ge == hipSuccess && g.maxDepth + 2 <= kTraversalStackDepth) {
            v.nodes = g.nodes; v.nodeCount = g.nodeCount; v.nodes4 = g.nodes4; v.node4Count = g.node4Count; v.tris = g.tris; v.triCount = g.triCount;
            v.rootLeaf = 0; v.attrs = g.attrs; v.tangents = g.tangents;
            maxDepth = g.maxDepth; maxDepth4 = g.maxDepth4; built = true; c->nodes4Capacity = g.nodes4Capacity;
            if (getenv("HRPT_GPU_BVH_HOST_COLLAPSE")) {     // experiment: the GPU-built 2-wide tree with the host's area-greedy, depth-first 4-wide collapse
                std::vector<HostNode> n2(g.nodeCount); std::vector<HostNode4> n4; uint32_t d4 = 0;
                HIP_TRY(c, hipMemcpy(n2.data(), g.nodes, n2.size() * sizeof(HostNode), hipMemcpyDeviceToHost));
                collapse_bvh2_on_host(n2, n4, d4);
                const HostNode4* dn4;
                if ((r = upload(c, n4.data(), n4.size(), &dn4, &c->bvhAllocations)) != HRPT_OK) return r;
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                v.nodes4 = reinterpret_cast<const GpuNode4*>(dn4); v.node4Count = (uint32_t)n4.size(); maxDepth4 = d4; c->nodes4Capacity = 0;
            }
            c->buildInfo.usedBuilder = g.ploc ? HRPT_BVH_BUILDER_GPU_PLOC : HRPT_BVH_BUILDER_GPU_LBVH; c->buildInfo.deviceBuildMs = g.deviceMs; c->buildInfo.mortonBits = g.mortonBits; c->buildInfo.sahCost = g.sahCost;
            if (g.refitted) c->buildInfo.usedBuilder |= HRPT_BVH_BUILDER_REFITTED;
        } else {
            // too deep for the traversal stacks (or a device error): drop the device-side builder and build on the host instead
            delete c->gpuBuilder; c->gpuBuilder = nullptr;
            if (ge == hipErrorInvalidValue && gerr == "non-finite vertex position") return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + gerr);
            if (ge == hipErrorOutOfMemory) return fail(c, HRPT_ERR_OUT_OF_MEMORY, "acceleration structure: " + gerr);
        }
        if (built) {
            std::vector<HostInstShade> shade; build_instance_shade(s, shade);
            const HostInstShade* dis;
            if ((r = upload(c, shade.data(), shade.size(), &dis, &c->bvhAllocations)) != HRPT_OK) return r;
            v.instShade = reinterpret_cast<const GpuInstShade*>(dis);
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    if (!built) {
        BuiltBvh bvh;
        if (!build_scene_bvh(s, bvh, berr)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
        std::vector<void*>* own = &c->bvhAllocations;
        const HostNode* dn; const HostTri* dt;
        if ((r = upload(c, bvh.nodes.data(), bvh.nodes.size(), &dn, own)) != HRPT_OK) return r;
        if ((r = upload(c, bvh.tris.data(), bvh.tris.size(), &dt, own)) != HRPT_OK) return r;
        v.nodes = reinterpret_cast<const GpuNode*>(dn); v.nodeCount = (uint32_t)bvh.nodes.size();
        v.tris = reinterpret_cast<const GpuTri*>(dt); v.triCount = (uint32_t)bvh.tris.size();
        v.rootLeaf = bvh.rootLeaf;
        const HostNode4* dn4;
        if ((r = upload(c, bvh.nodes4.data(), bvh.nodes4.size(), &dn4, own)) != HRPT_OK) return r;
        v.nodes4 = reinterpret_cast<const GpuNode4*>(dn4); v.node4Count = (uint32_t)bvh.nodes4.size();
        // The quantised vertex / index / mesh / instance buffers are consumed here: per-triangle attribute records and
        // per-instance adjugate rows replace the per-hit GetTriangleVertices + UnpackVertex + MakeAdjugateMatrix work.
        const HostTriAttr* da; const HostTriTangent* dtg; const HostInstShade* dis;
        if ((r = upload(c, bvh.attrs.data(), bvh.attrs.size(), &da, own)) != HRPT_OK) return r;
        if ((r = upload(c, bvh.instShade.data(), bvh.instShade.size(), &dis, own)) != HRPT_OK) return r;
        v.attrs = reinterpret_cast<const GpuTriAttr*>(da); v.instShade = reinterpret_cast<const GpuInstShade*>(dis);
        v.tangents = nullptr;
        if (!bvh.tangents.empty()) {
            if ((r = upload(c, bvh.tangents.data(), bvh.tangents.size(), &dtg, own)) != HRPT_OK) return r;
            v.tangents = reinterpret_cast<const GpuTriTangent*>(dtg);
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // the BuiltBvh staging vectors die at scope exit
        maxDepth = bvh.maxDepth; maxDepth4 = bvh.maxDepth4;
        c->buildInfo.usedBuilder = HRPT_BVH_BUILDER_HOST_SAH; c->buildInfo.sahCost = bvh.sahCost;
    }
    if (v.node4Count >= kMaxStructureNodes) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: more than 2^25 nodes (32-bit node offsets in the traversal kernels)");
    // the 64-byte quantised form of the 4-wide tree, whichever builder made it (what the wavefront kernels may read when the tree is not in LDS)
    v.nodesQ = nullptr; bool quantisedNodes = false;
    if (v.node4Count) {
        if (c->nodesQCapacity <= v.node4Count) {                   // (<=: record nodesQCapacity - 1 is the accumulator below, never a node)
            if (c->nodesQ) (void)hipFree(c->nodesQ);
            c->nodesQ = nullptr; c->nodesQCapacity = 0;
            const size_t cap = (size_t)v.node4Count + v.node4Count / 8 + 64;
            if (hipMalloc((void**)&c->nodesQ, cap * sizeof(GpuNodeQ)) != hipSuccess) return fail(c, HRPT_ERR_OUT_OF_MEMORY, "acceleration structure: quantised nodes");
            c->nodesQCapacity = cap;
        }
        double* dArea = reinterpret_cast<double*>(c->nodesQ + (c->nodesQCapacity - 1));       // the last (spare) record of the buffer: two doubles
        HIP_TRY(c, hipMemsetAsync(dArea, 0, 4 * sizeof(double), c->stream));
        HIP_TRY(c, launch_quantise_nodes(v.nodes4, v.node4Count, c->nodesQ, dArea, c->stream));
        double area[4] = { 0.0, 0.0, 0.0, 0.0 };
        HIP_TRY(c, hipMemcpyAsync(area, dArea, sizeof area, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        v.nodesQ = c->nodesQ;
        // Which nodes the kernels walk when the tree is in global memory. The quantised form saves three of seven 16-byte requests per lane and
        // step and pays in decode arithmetic and in looser boxes; what the looser LEAF boxes cost is triangle tests (three requests + a
        // watertight test each). Measured (MI355X, 1080p): Sponza-class scene: wf_extend 6.66 -> 6.18 ms, frame 13.8 -> 13.3 ms; glass scene
        // (18 k triangles of tessellated glass bodies): shadow-ray triangle tests x 2.4, closest-hit leaf visits + 43 %, frame +2 %.
        const float inflation = area[0] > 0.0 ? (float)(area[1] / area[0]) : 1.0f;
        if (getenv("HRPT_BVH_NODE_FORMAT_DEBUG")) fprintf(stderr, "quantised nodes: leaf area ratio %.4f (area-weighted), %.4f (mean over %.0f leaves)\n", inflation, area[3] > 0 ? area[2] / area[3] : 1.0, area[3]);
        int format = 0;
        if (const char* e = getenv("HRPT_BVH_NODE_FORMAT")) format = atoi(e);          // 1: fp32 nodes, 2: quantised nodes, else by the leaf-area ratio
        // (the leaf-area ratio is ~1.01 on BOTH scenes, so it does not tell them apart: on the glass scene it is the paths that bounce inside and between
        // the finely tessellated glass bodies that visit 40 % more leaves through the rounded boxes. Until that is understood the rule is empirical:
        // quantised nodes unless some instance is transmissive or BLEND.)
        bool glassy = false;
        for (uint32_t i = 0; i < s.instanceCount && !glassy; ++i) {
            const HrptMaterialConstants& m = s.materials[s.instances[i].m_MaterialIndex];
            glassy = m.m_TransmissionFactor > 0.0f || m.m_AlphaMode == HRPT_ALPHA_MODE_BLEND;
        }
        quantisedNodes = format == 2 || (format != 1 && inflation <= 1.10f && !glassy);
        c->buildInfo.leafAreaPermille = (uint32_t)(inflation * 1000.0f + 0.5f); c->buildInfo.nodeFormat = quantisedNodes ? 2u : 1u;
    }
    c->buildInfo.buildMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->buildInfo.triangleCount = v.triCount; c->buildInfo.nodeCount = v.nodeCount; c->buildInfo.node4Count = v.node4Count;
    c->buildInfo.maxDepth = maxDepth; c->buildInfo.maxDepth4 = maxDepth4;
    c->bvhNodes = v.nodeCount; c->bvhTris = v.triCount;
    c->traits.bvhMaxDepth = maxDepth; c->traits.bvh4MaxDepth = maxDepth4; c->traits.quantisedNodes = quantisedNodes;
    return HRPT_OK;
}

// What the kernels specialise on (SceneTraits), from the library's copy of instances / materials / lights; the tree depths are kept.
static void refresh_traits(HrptContext* c)
{
    SceneTraits t; t.bvhMaxDepth = c->traits.bvhMaxDepth; t.bvh4MaxDepth = c->traits.bvh4MaxDepth; t.twoLevelStackNeed = c->traits.twoLevelStackNeed; t.quantisedNodes = c->traits.quantisedNodes;
    for (const HrptPerInstanceData& in : c->keptInstances) {
        const HrptMaterialConstants& m = c->keptMaterials[in.m_MaterialIndex];
        // the transmission branch (PathTracer.hlsl:149-255) is entered for transmissive AND for BLEND materials (effective transmission
        // 1 - alpha), and a thick one switches the path's medium state there: that state then has to travel with the path
        if ((m.m_TransmissionFactor > 0.0f || m.m_AlphaMode == HRPT_ALPHA_MODE_BLEND) && m.m_IsThinSurface == 0) t.hasMedium = true;
        if (m.m_AlphaMode == HRPT_ALPHA_MODE_BLEND && !(m.m_TransmissionFactor > 0.0f)) t.hasStochasticAlpha = true;
        if (m.m_TextureFlags != 0) t.hasTextures = true;
        if (m.m_AlphaMode != HRPT_ALPHA_MODE_OPAQUE) t.hasNonOpaque = true;
        if (m.m_TransmissionFactor > 0.0f || m.m_AlphaMode == HRPT_ALPHA_MODE_BLEND) t.hasTransmissiveOrBlend = true;
    }
    for (const HrptGPULight& l : c->keptLights) if (l.m_Type != HRPT_LIGHT_DIRECTIONAL) t.directionalLightsOnly = false;
    c->traits = t;
}

static int upload_scene_impl(HrptContext* c, const HrptSceneDesc* s)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!s) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: null scene");
    if (!s->brunetonTransmittance || !s->brunetonScattering) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: Bruneton LUTs missing");
    if (s->textureCount && !s->textures) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: null texture table");
    HIP_TRY(c, hipSetDevice(c->device));
    std::string berr;
    uint64_t sceneTris = 0;
    if (!validate_scene(*s, sceneTris, berr, false)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: " + berr);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_scene(c);
    c->traits = SceneTraits();
    SceneView v{};
    int r;
    const bool timing = getenv("HRPT_BUILD_TIMING") != nullptr; auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!timing) return; (void)hipStreamSynchronize(c->stream); auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[upload]    %-22s %7.3f ms\n", what, std::chrono::duration<float, std::milli>(t - tp).count()); tp = t; };
    if ((r = build_acceleration(c, *s, sceneTris, v, true)) != HRPT_OK) return r;
    lap("acceleration structure");
    if ((r = upload(c, s->materials, s->materialCount, &v.materials)) != HRPT_OK) return r;
    if ((r = upload(c, s->lights, s->lightCount, &v.lights)) != HRPT_OK) return r;
    v.lightCount = s->lightCount; c->lightCapacity = s->lightCount;

    std::vector<GpuTexture> table(s->textureCount);
    for (uint32_t i = 0; i < s->textureCount; ++i) {
        const HrptTextureDesc& td = s->textures[i];
        GpuTexture& g = table[i];
        memset(&g, 0, sizeof g);
        g.w = td.width; g.h = td.height; g.format = td.format; g.mipCount = td.mipCount ? td.mipCount : 1u;
        if (!td.texels) continue;
        if (td.width == 0 || td.height == 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: zero-sized texture");
        if (td.format > HRPT_TEXTURE_FORMAT_RGBA32_FLOAT) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: unknown texture format");
        if (g.mipCount > HRPT_TEXTURE_MAX_MIPS) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: more than HRPT_TEXTURE_MAX_MIPS mip levels");
        uint64_t texels = 0;
        for (uint32_t l = 0; l < g.mipCount; ++l) {
            if (l > 0 && (td.width >> l) == 0 && (td.height >> l) == 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: more mip levels than the texture size allows");
            g.mipOffset[l] = (uint32_t)texels;
            texels += (uint64_t)((td.width >> l) ? (td.width >> l) : 1u) * ((td.height >> l) ? (td.height >> l) : 1u);
        }
        if (texels > 0xFFFFFFFFull) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upload_scene: texture too large");
        const size_t bpt = td.format <= HRPT_TEXTURE_FORMAT_RGBA8_SRGB ? 4 : (td.format == HRPT_TEXTURE_FORMAT_RGBA16_FLOAT ? 8 : 16);
        const uint8_t* d;
        if ((r = upload(c, static_cast<const uint8_t*>(td.texels), (size_t)texels * bpt, &d)) != HRPT_OK) return r;
        g.texels = d;
    }
    if ((r = upload(c, table.data(), table.size(), &v.textures)) != HRPT_OK) return r;
    v.textureCount = s->textureCount;
    lap("materials, textures");

    // Bruneton LUTs: float32 file layout -> RGBA16F (src/CommonResources.cpp:534-558)
    const size_t nT = 256u * 64u * 4u, nS = 256u * 128u * 32u * 4u;
    std::vector<uint16_t> hT(nT), hS(nS);
    for (size_t i = 0; i < nT; ++i) hT[i] = float_to_half(s->brunetonTransmittance[i]);
    {   // 4 M conversions: 9 ms of every upload on one thread
        const float* src = s->brunetonScattering; uint16_t* dst = hS.data();
        const unsigned threads = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
        const size_t chunk = (nS + threads - 1) / threads;
        auto part = [src, dst, nS, chunk](size_t t) { for (size_t i = t * chunk, e = std::min(nS, i + chunk); i < e; ++i) dst[i] = float_to_half(src[i]); };
        std::vector<std::thread> pool;
        size_t started = 1;
        try { for (; started < threads; ++started) pool.emplace_back(part, started); } catch (const std::system_error&) {}
        part(0);
        for (std::thread& th : pool) th.join();
        for (size_t t = started; t < threads; ++t) part(t);       // (threads that could not be started)
    }
    if ((r = upload(c, hT.data(), nT, &v.lutTransmittance)) != HRPT_OK) return r;
    if ((r = upload(c, hS.data(), nS, &v.lutScattering)) != HRPT_OK) return r;
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // host staging vectors die at scope exit
    lap("atmosphere tables");

    c->view = v; c->haveScene = true;
    c->keptVertices.assign(s->vertices, s->vertices + s->vertexCount); c->keptIndices.assign(s->indices, s->indices + s->indexCount);
    c->keptMeshData.assign(s->meshData, s->meshData + s->meshDataCount); c->keptInstances.assign(s->instances, s->instances + s->instanceCount);
    c->keptMaterials.assign(s->materials, s->materials + s->materialCount);
    c->keptLights.assign(s->lights, s->lights + s->lightCount);
    refresh_traits(c);
    lap("kept copies, traits");
    return HRPT_OK;
}

// The scene description the rebuild paths hand to the builders, over the library's copies.
static HrptSceneDesc kept_scene_desc(HrptContext* c)
{
    HrptSceneDesc s{};
    s.vertices = c->keptVertices.data(); s.vertexCount = (uint32_t)c->keptVertices.size();
    s.indices = c->keptIndices.data(); s.indexCount = (uint32_t)c->keptIndices.size();
    s.meshData = c->keptMeshData.data(); s.meshDataCount = (uint32_t)c->keptMeshData.size();
    s.instances = c->keptInstances.data(); s.instanceCount = (uint32_t)c->keptInstances.size();
    s.materials = c->keptMaterials.data(); s.materialCount = (uint32_t)c->keptMaterials.size();
    static const HrptGPULight noLight{};                 // lights play no part in the build; validate_scene only wants the array to exist
    s.lights = &noLight; s.lightCount = 1;
    return s;
}
static uint64_t kept_triangle_count(const HrptContext* c)
{
    uint64_t n = 0;
    for (const HrptPerInstanceData& in : c->keptInstances) n += c->keptMeshData[in.m_MeshDataIndex].m_IndexCounts[0] / 3;
    return n;
}

static int update_lights_impl(HrptContext* c, const HrptGPULight* lights, uint32_t count)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_lights: no scene uploaded");
    if (!lights || count == 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_lights: a scene needs at least one light (the reference guarantees a directional light, src/Scene.cpp:635-666)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // frames in flight still read the old buffer
    if (count > c->lightCapacity) {
        const HrptGPULight* d; int r;
        if ((r = upload(c, lights, count, &d)) != HRPT_OK) return r;      // the old, smaller buffer stays in the scene's allocation list
        c->view.lights = d; c->lightCapacity = count;
    } else {
        HIP_TRY(c, hipMemcpyAsync(const_cast<HrptGPULight*>(c->view.lights), lights, (size_t)count * sizeof(HrptGPULight), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->view.lightCount = count;
    c->keptLights.assign(lights, lights + count);
    refresh_traits(c);
    return HRPT_OK;
}

static int update_materials_impl(HrptContext* c, const HrptMaterialConstants* materials, uint32_t firstMaterial, uint32_t count)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_materials: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!materials) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_materials: null material array");
    if ((uint64_t)firstMaterial + count > c->keptMaterials.size()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_materials: range exceeds the scene's material count");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // The acceleration structure caches two things of a material: whether its triangles are opaque (any-hit / candidate handling) and
    // whether any material needs tangent frames. A change of either needs a rebuild; everything else is a plain buffer write.
    HrptSceneDesc before = kept_scene_desc(c);
    const bool tangentsBefore = scene_needs_tangents(before);
    bool structural = false;
    for (uint32_t i = 0; i < count; ++i)
        if (triangle_flags_for_material(materials[i]) != triangle_flags_for_material(c->keptMaterials[firstMaterial + i])) structural = true;   // opacity or shading class
    std::memcpy(c->keptMaterials.data() + firstMaterial, materials, (size_t)count * sizeof(HrptMaterialConstants));
    HIP_TRY(c, hipMemcpyAsync(const_cast<HrptMaterialConstants*>(c->view.materials) + firstMaterial, materials, (size_t)count * sizeof(HrptMaterialConstants), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HrptSceneDesc s = kept_scene_desc(c);
    if (scene_needs_tangents(s) != tangentsBefore) structural = true;
    if (structural) {
        SceneView v = c->view;
        int r = build_acceleration(c, s, kept_triangle_count(c), v, true);     // from scratch: the GPU builder's resident instance table holds the opacity flags
        if (r != HRPT_OK) { c->haveScene = false; return r; }
        c->view = v;
        c->motionInstStale = true;
    }
    refresh_traits(c);
    return HRPT_OK;
}

static int update_instances_impl(HrptContext* c, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count, bool refit)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_instances: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!instances) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_instances: null instance array");
    if ((uint64_t)firstInstance + count > c->keptInstances.size()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_instances: range exceeds the scene's instance count");
    for (uint32_t i = 0; i < count; ++i) {
        const HrptPerInstanceData& now = instances[i]; const HrptPerInstanceData& was = c->keptInstances[firstInstance + i];
        if (now.m_MeshDataIndex != was.m_MeshDataIndex || now.m_MaterialIndex != was.m_MaterialIndex || now.m_LODIndex != was.m_LODIndex)
            return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_instances: mesh, material and LOD of an instance cannot change (upload the scene again)");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // frames in flight still traverse the old tree
    std::memcpy(c->keptInstances.data() + firstInstance, instances, (size_t)count * sizeof(HrptPerInstanceData));
    ++c->instanceEpoch;
    c->motionInstStale = true;                          // m_PrevWorld travels in these records (hrpt_render_motion_vectors)
    HrptSceneDesc s = kept_scene_desc(c);
    const uint64_t sceneTris = kept_triangle_count(c);
    SceneView v = c->view;
    int r = build_acceleration(c, s, sceneTris, v, false, refit);
    if (r != HRPT_OK) { c->haveScene = false; return r; }   // the old tree is gone: the scene has to be uploaded again
    c->view = v;
    return HRPT_OK;
}

// ---- keyframe animation on the device: hrpt_animate and its companions (csrc/pt_anim.h has the definition) ----
static AnimDeviceCopy* find_animation_copy(HrptContext* c, const HrptAnimation* anim)
{
    for (AnimDeviceCopy& a : c->animations) if (a.anim == anim && a.serial == anim->serial) return &a;
    return nullptr;
}

// Uploads the resolved tables and seeds the state: once per (context, animation).
static int upload_animation(HrptContext* c, const HrptAnimation* anim, AnimDeviceCopy*& out)
{
    for (size_t i = 0; i < c->animations.size(); ++i)          // an address reused by a newer animation: the old copy is dead
        if (c->animations[i].anim == anim) { free_animation_copy(c->animations[i]); c->animations.erase(c->animations.begin() + (long)i); break; }
    AnimDeviceCopy a;
    a.anim = anim; a.serial = anim->serial;
    int r = HRPT_OK;
    auto put = [&](const auto& v, auto*& dev) {
        using T = typename std::remove_reference<decltype(v)>::type::value_type;
        const T* d = nullptr;
        if (r == HRPT_OK) r = upload(c, v.data(), v.size(), &d, &a.allocations);
        dev = const_cast<T*>(d);
    };
    HrptAnimSampler* samplers; float* keyTimes; float* keyValues; HrptAnimChannel* channels; uint32_t* targets; uint32_t* order; int32_t* orderParent;
    uint32_t* rangeNode; uint32_t* jointNode; float* inverseBind;
    put(anim->samplers, samplers); put(anim->keyTimes, keyTimes); put(anim->keyValues, keyValues); put(anim->channels, channels); put(anim->targets, targets);
    put(anim->order, order); put(anim->orderParent, orderParent); put(anim->rangeNode, rangeNode); put(anim->jointNode, jointNode); put(anim->inverseBind, inverseBind);
    put(anim->groupFirst, a.groupFirst); put(anim->times, a.times); put(anim->baseTrs, a.trs); put(anim->baseWorlds, a.worlds);
    const std::vector<float> zeroWeights(anim->morphWeightCount, 0.0f), zeroPalette(12 * anim->jointNode.size(), 0.0f);
    put(zeroWeights, a.weights); put(zeroPalette, a.palette);
    const std::vector<HrptPerInstanceData> zeroRecords(anim->rangeNode.size());
    put(zeroRecords, a.records);
    if (r == HRPT_OK && hipStreamSynchronize(c->stream) != hipSuccess) r = fail(c, HRPT_ERR_HIP, "hrpt_animate: table upload failed");   // the staging vectors above die here
    if (r != HRPT_OK) { free_animation_copy(a); return r; }
    a.tables = anim->tables();
    a.tables.samplers = samplers; a.tables.keyTimes = keyTimes; a.tables.keyValues = keyValues; a.tables.channels = channels; a.tables.targets = targets;
    a.tables.order = order; a.tables.orderParent = orderParent; a.tables.rangeNode = rangeNode; a.tables.jointNode = jointNode; a.tables.inverseBind = inverseBind;
    c->animations.push_back(a);
    out = &c->animations.back();
    return HRPT_OK;
}

static int animate_impl(HrptContext* c, const HrptAnimation* anim, uint32_t flags)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!anim) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate: null animation");
    if (flags & ~(uint32_t)(HRPT_ANIMATE_REFIT | HRPT_ANIMATE_NO_COMMIT)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate: unknown flag bits");
    const bool evaluateInstances = (flags & HRPT_ANIMATE_NO_COMMIT) == 0;
    if (evaluateInstances) {
        if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate: no scene uploaded");
        if (anim->instanceNeed > c->keptInstances.size()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate: an instance index of the animation exceeds the scene's instance count");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    AnimDeviceCopy* a = find_animation_copy(c, anim);
    if (!a) HRPT_TRY(upload_animation(c, anim, a));
    const uint32_t range = (uint32_t)anim->rangeNode.size();
    const bool commit = evaluateInstances && range > 0;
    if (!anim->times.empty()) HIP_TRY(c, hipMemcpyAsync(a->times, anim->times.data(), anim->times.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (commit && a->recordsEpoch != c->instanceEpoch) {       // something else wrote the instances since this copy was made
        HIP_TRY(c, hipMemcpyAsync(a->records, c->keptInstances.data() + anim->instanceFirst, (size_t)range * sizeof(HrptPerInstanceData), hipMemcpyHostToDevice, c->stream));
        a->recordsEpoch = 0;
    }
    // HRPT_ANIM_TIMING (scripts/anim_bench.py): device time of the kernels between events, host time of the read-back and of the commit, on stderr
    const bool timing = getenv("HRPT_ANIM_TIMING") != nullptr;
    if (timing) HIP_TRY(c, hipEventRecord(c->evStart, c->stream));
    HIP_TRY(c, launch_animate(a->tables, a->times, a->groupFirst, anim->groupFirst.data(), (uint32_t)anim->groupFirst.size() - 1u, a->trs, a->worlds, a->weights, a->palette,
                              commit ? a->records : nullptr, c->stream));
    float kernelMs = 0.0f;
    if (timing) {
        HIP_TRY(c, hipEventRecord(c->evStop, c->stream));
        HIP_TRY(c, hipEventSynchronize(c->evStop));
        HIP_TRY(c, hipEventElapsedTime(&kernelMs, c->evStart, c->evStop));
        if (!commit) fprintf(stderr, "[animate] kernels %.4f ms\n", kernelMs);
    }
    if (!commit) return HRPT_OK;                                // evaluation only, or no instance hangs under a composed node: nothing to commit, nothing to build
    const auto t0 = std::chrono::steady_clock::now();
    // the commit of hrpt_update_instances: the evaluated range comes back into the host copy, the rest of the roll is host work
    std::vector<HrptPerInstanceData> evaluated(range);
    HIP_TRY(c, hipMemcpyAsync(evaluated.data(), a->records, (size_t)range * sizeof(HrptPerInstanceData), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->keptInstances.size(); ++i)
        if (i < anim->instanceFirst || i - anim->instanceFirst >= range) std::memcpy(c->keptInstances[i].m_PrevWorld, c->keptInstances[i].m_World, sizeof(float) * 16);
    const auto t1 = std::chrono::steady_clock::now();
    const int r = update_instances_impl(c, evaluated.data(), anim->instanceFirst, range, (flags & HRPT_ANIMATE_REFIT) != 0);
    if (timing) fprintf(stderr, "[animate] kernels %.4f ms read-back and roll %.4f ms commit %.4f ms\n", kernelMs, std::chrono::duration<float, std::milli>(t1 - t0).count(),
                        std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count());
    a = find_animation_copy(c, anim);
    if (a) a->recordsEpoch = r == HRPT_OK ? c->instanceEpoch : 0;
    return r;
}

static int animation_pointers(HrptContext* c, const char* what, const HrptAnimation* anim, AnimDeviceCopy*& a)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!anim) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null animation");
    a = find_animation_copy(c, anim);
    if (!a) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": hrpt_animate has not run for this animation on this context");
    return HRPT_OK;
}

// ---- deforming meshes: hrpt_update_vertices / hrpt_update_vertices_device (include/hobbyrt_pt.h has the contract) ----
constexpr uint32_t kVertexUpdateFlags = HRPT_VERTICES_REFIT | HRPT_VERTICES_SAME_FRAME;

// The argument checks both variants share (the answer without a scene is hrpt_update_instances').
static int check_vertex_update(HrptContext* c, const char* what, const void* vertices, uint32_t firstVertex, uint32_t count, uint32_t flags)
{
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": no scene uploaded");
    if (flags & ~kVertexUpdateFlags) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown flag bits");
    if (!vertices && count > 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null vertex array");
    if ((uint64_t)firstVertex + count > c->keptVertices.size()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": range exceeds the scene's vertex count");
    return HRPT_OK;
}

// The previous-position protocol: a call without HRPT_VERTICES_SAME_FRAME starts a frame (previous = current everywhere), every call records
// the positions it is about to replace. While no call has recorded anything the table stays empty, which stands for previous == current.
static void roll_previous_positions(HrptContext* c, uint32_t firstVertex, uint32_t count, uint32_t flags)
{
    const bool newFrame = (flags & HRPT_VERTICES_SAME_FRAME) == 0;
    if (count == 0) {
        if (newFrame && !c->keptPrevPositions.empty()) { c->keptPrevPositions.clear(); c->motionPositionsStale = true; }
        return;
    }
    if (newFrame || c->keptPrevPositions.empty()) {
        c->keptPrevPositions.resize(c->keptVertices.size() * 3);
        for (size_t i = 0; i < c->keptVertices.size(); ++i) std::memcpy(&c->keptPrevPositions[3 * i], c->keptVertices[i].m_Pos, 12);
    } else {
        for (size_t i = firstVertex; i < (size_t)firstVertex + count; ++i) std::memcpy(&c->keptPrevPositions[3 * i], c->keptVertices[i].m_Pos, 12);
    }
    c->motionPositionsStale = true;
}

// Installs validated vertices: `quantised` (host, count records) goes into the kept copy; a flat structure's GPU builder gets its device
// buffer patched from `deviceQuantised` when the records are already on the device, from the host array otherwise; then the structure follows.
static int commit_vertices(HrptContext* c, const char* what, const HrptVertexQuantized* quantised, const HrptVertexQuantized* deviceQuantised,
                           uint32_t firstVertex, uint32_t count, uint32_t flags)
{
    roll_previous_positions(c, firstVertex, count, flags);
    std::memcpy(c->keptVertices.data() + firstVertex, quantised, (size_t)count * sizeof(HrptVertexQuantized));
    const bool twoLevel = c->twoLevel != nullptr;
    if (!twoLevel && c->gpuBuilder) {
        std::string gerr;
        const hipError_t e = c->gpuBuilder->update_vertices(deviceQuantised ? deviceQuantised : quantised, deviceQuantised != nullptr, firstVertex, count, c->stream, gerr);
        if (e != hipSuccess) { c->haveScene = false; return fail(c, HRPT_ERR_HIP, std::string(what) + ": " + gerr + ": " + hipGetErrorString(e)); }
    }
    HrptSceneDesc s = kept_scene_desc(c);
    SceneView v = c->view;
    // flat: a rebuild like hrpt_update_instances' (the GPU builder keeps its buffers; the host builder starts from the kept copy). Two-level: the
    // mesh trees hold the old vertices, so the whole structure is built again along the first-build path.
    const int r = build_acceleration(c, s, kept_triangle_count(c), v, twoLevel, (flags & HRPT_VERTICES_REFIT) != 0);
    if (r != HRPT_OK) { c->haveScene = false; return r; }   // the old tree is gone: the scene has to be uploaded again
    c->view = v;
    return HRPT_OK;
}

static int update_vertices_impl(HrptContext* c, const HrptVertexQuantized* vertices, uint32_t firstVertex, uint32_t count, uint32_t flags)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(check_vertex_update(c, "hrpt_update_vertices", vertices, firstVertex, count, flags));
    for (uint32_t i = 0; i < count; ++i)
        if (!deform::position_finite(vertices[i].m_Pos)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_vertices: non-finite vertex position");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // frames in flight still traverse the old tree and read the old motion tables
    if (count == 0) { roll_previous_positions(c, 0, 0, flags); return HRPT_OK; }
    return commit_vertices(c, "hrpt_update_vertices", vertices, nullptr, firstVertex, count, flags);
}

// What hrpt_update_vertices_device and hrpt_update_vertices_skinned share once their arguments are checked: `launch(staged, dStatus2)` puts
// a kernel on the context's stream that writes `count` quantised records into the staging buffer and raises the two status words behind
// them (word 0: a position that is not finite; word 1: a joint index out of range); nothing is committed before both are known to be clear.
extern "C++" template <class Launch>
static int update_vertices_staged(HrptContext* c, const std::string& what, uint32_t firstVertex, uint32_t count, uint32_t flags, hipStream_t stream, Launch launch)
{
    constexpr size_t kStatusBytes = 2 * sizeof(uint32_t);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (count == 0) { roll_previous_positions(c, 0, 0, flags); return HRPT_OK; }
    HIP_TRY(c, hipStreamSynchronize(stream));           // whatever writes the caller's arrays has to be done before the kernel below reads them
    const size_t recordBytes = (size_t)count * sizeof(HrptVertexQuantized);
    if (!c->dDeformStaging) {                           // once per scene: room for the whole vertex buffer + the status words
        const size_t bytes = c->keptVertices.size() * sizeof(HrptVertexQuantized) + kStatusBytes;
        HIP_TRY(c, hipMalloc(&c->dDeformStaging, bytes));
        c->deformStagingBytes = bytes;
    }
    if (recordBytes + kStatusBytes > c->deformStagingBytes) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": range exceeds the staging buffer");
    HrptVertexQuantized* staged = static_cast<HrptVertexQuantized*>(c->dDeformStaging);
    uint32_t* dStatus = reinterpret_cast<uint32_t*>(static_cast<char*>(c->dDeformStaging) + recordBytes);
    HIP_TRY(c, hipMemsetAsync(dStatus, 0, kStatusBytes, c->stream));
    HIP_TRY(c, launch(staged, dStatus));
    // the copy-back that keeps the host copy current also brings the status words
    std::vector<HrptVertexQuantized> host((recordBytes + kStatusBytes + sizeof(HrptVertexQuantized) - 1) / sizeof(HrptVertexQuantized));
    HIP_TRY(c, hipMemcpyAsync(host.data(), staged, recordBytes + kStatusBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t status[2] = { 0, 0 };
    std::memcpy(status, reinterpret_cast<const char*>(host.data()) + recordBytes, sizeof status);
    if (status[1]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": joint index out of range");
    if (status[0]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": non-finite vertex position");
    return commit_vertices(c, what.c_str(), host.data(), staged, firstVertex, count, flags);
}

static int update_vertices_device_impl(HrptContext* c, const HrptVertexFloat* deviceVertices, uint32_t firstVertex, uint32_t count, uint32_t flags, hipStream_t stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(check_vertex_update(c, "hrpt_update_vertices_device", deviceVertices, firstVertex, count, flags));
    if (reinterpret_cast<uintptr_t>(deviceVertices) & 15u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_update_vertices_device: deviceVertices must be 16-byte aligned");
    return update_vertices_staged(c, "hrpt_update_vertices_device", firstVertex, count, flags, stream, [&](HrptVertexQuantized* staged, uint32_t* dStatus) {
        return launch_quantise_vertices(deviceVertices, count, staged, dStatus, c->stream);
    });
}

// ---- the producer in front: hrpt_skin_vertices_host / _device, hrpt_update_vertices_skinned (csrc/pt_skin.h has the definition) ----
// The argument checks all three share.
static int skin_args_check(HrptContext* c, const char* what, const HrptSkinArgs* a)
{
    const std::string w(what);
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (!a) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null args");
    if (a->reserved != 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": reserved must be 0");
    if (misaligned(a->base, 15) || misaligned(a->joints, 7) || misaligned(a->weights, 15) || misaligned(a->jointMatrices, 15) || misaligned(a->deltas, 3) ||
        misaligned(a->morphWeights, 3))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": base, weights and jointMatrices must be 16-byte aligned, joints 8-byte, deltas and morphWeights 4-byte");
    if (a->joints && (!a->weights || !a->jointMatrices || a->jointCount == 0)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": joints need weights, jointMatrices and a jointCount > 0");
    if (a->targetCount > 0 && (!a->deltas || !a->morphWeights)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": targetCount > 0 needs deltas and morphWeights");
    if (!a->base && a->count > 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null base");
    return HRPT_OK;
}

// HRPT_SKIN_PALETTE=1: gather every palette from global memory (the A/B of scripts/skin_bench.py); anything else: by joint count
static int skin_palette_mode() { const char* e = getenv("HRPT_SKIN_PALETTE"); return e ? atoi(e) : 0; }

static int update_vertices_skinned_impl(HrptContext* c, const HrptSkinArgs* args, uint32_t firstVertex, uint32_t flags, hipStream_t stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(skin_args_check(c, "hrpt_update_vertices_skinned", args));
    HRPT_TRY(check_vertex_update(c, "hrpt_update_vertices_skinned", args->base, firstVertex, args->count, flags));
    // Two kernels on the context's stream, the skinned floats in a buffer of the context between them. A kernel that quantised in
    // registers instead was measured no faster than this and is not kept.
    return update_vertices_staged(c, "hrpt_update_vertices_skinned", firstVertex, args->count, flags, stream, [&](HrptVertexQuantized* staged, uint32_t* dStatus) {
        if (!c->dSkinFloats) {                          // once per scene: room for the whole vertex buffer
            const hipError_t e = hipMalloc((void**)&c->dSkinFloats, c->keptVertices.size() * sizeof(HrptVertexFloat));
            if (e != hipSuccess) { c->dSkinFloats = nullptr; return e; }
        }
        const hipError_t e = launch_skin_vertices(*args, c->dSkinFloats, dStatus, skin_palette_mode(), c->stream);
        return e != hipSuccess ? e : launch_quantise_vertices(c->dSkinFloats, args->count, staged, dStatus, c->stream);
    });
}

int hrpt_resize(HrptContext* c, uint32_t width, uint32_t height)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!size_ok(width, height))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resize: size must be 1..65535 (RNG seed packs y*65536+x, RNG.hlsli:24)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_image(c->dAccum); free_image(c->dOutput); free_image(c->dDisplay);      // all three go before anything is allocated
    const size_t bytes = (size_t)width * height * sizeof(float4);
    HRPT_TRY(realloc_image(c, c->dAccum, bytes));
    HRPT_TRY(realloc_image(c, c->dOutput, bytes));
    for (float4*& plane : c->dGBuffer)         // the G-buffer planes a caller has asked for follow the image size (zeroed, like a first request)
        if (plane) HRPT_TRY(realloc_image(c, plane, bytes));
    if (c->dMotion) HRPT_TRY(realloc_image(c, c->dMotion, bytes));       // ... and so does the motion plane
    c->temporalValid = false; c->temporalCur = 0;     // the temporal history does not survive a resize
    for (float4*& image : c->dTemporal)
        if (image) HRPT_TRY(realloc_image(c, image, bytes));
    for (float4*& image : c->dDenoiseScratch) free_image(image);        // allocated again by the call that needs it
    free_image(c->dModulation);                                         // written again by the next hrpt_demodulate
    c->width = width; c->height = height;
    return HRPT_OK;
}

float hrpt_halton(uint32_t index, uint32_t base)   // src/Utilities.cpp:67-79
{
    float result = 0.0f;
    float f = 1.0f / (float)base;
    uint32_t i = index;
    while (i > 0) {
        result += f * (float)(i % base);
        i /= base;
        f /= (float)base;
    }
    return result;
}

static int render_impl(HrptContext* c, const HrptFrameParams* p)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: null params");
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_render: no scene uploaded");
    if (!c->dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: hrpt_resize not called");
    if (p->accumCount == 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: accumCount == 0");
    if (p->constants.m_MaxBounces > 64u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: m_MaxBounces above 64 (the reference's UI stops at 12, src/ImGuiLayer.cpp:760; one kernel sequence is launched per bounce)");
    if (p->constants.m_LightCount > c->view.lightCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: m_LightCount exceeds the scene's light buffer");
    uint32_t vw = (uint32_t)p->constants.m_View.m_ViewportSize[0], vh = (uint32_t)p->constants.m_View.m_ViewportSize[1];
    if (vw != c->width || vh != c->height) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: m_ViewportSize does not match hrpt_resize");
    TileRect rect; rect.x0 = p->tileX0; rect.y0 = p->tileY0; rect.x1 = p->tileX1; rect.y1 = p->tileY1;
    rect.stripeCount = p->stripeCount ? p->stripeCount : 1u; rect.stripeIndex = p->stripeIndex;
    if (rect.stripeIndex >= rect.stripeCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: stripeIndex must be below stripeCount");
    if (rect.x0 == 0 && rect.y0 == 0 && rect.x1 == 0 && rect.y1 == 0) { rect.x1 = c->width; rect.y1 = c->height; }
    if (rect.x1 > c->width || rect.y1 > c->height || rect.x0 > rect.x1 || rect.y0 > rect.y1)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: tile rectangle outside the image");
    HIP_TRY(c, hipSetDevice(c->device));

    bool wavefront = (p->flags & HRPT_FRAME_MEGAKERNEL) == 0 && wavefront_supports(c->view, p->constants);
    if (!wavefront && c->view.instances && c->traits.twoLevelStackNeed > 64u)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_render: this two-level structure is deeper than the validation megakernel's 64-entry stack");
    if (!wavefront && (p->flags & HRPT_FRAME_MEGAKERNEL) == 0) c->megakernelFallbacks++;
    HIP_TRY(c, hipEventRecord(c->evStart, c->stream));
    if (wavefront) {
        std::string werr;
        c->wf.profile = (p->flags & HRPT_FRAME_PROFILE) != 0;
        c->wf.shadeInstances = (uint32_t)c->keptInstances.size(); c->wf.shadeMaterials = (uint32_t)c->keptMaterials.size();    // as uploaded / last updated
        hipError_t e = wavefront_render(c->wf, c->view, c->traits, p->constants, p->accumCount, c->dAccum, c->dOutput, c->width, c->height, rect,
                                        c->dCounters, c->stream, werr);
        if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? HRPT_ERR_OUT_OF_MEMORY : HRPT_ERR_HIP, "wavefront_render: " + werr + ": " + hipGetErrorString(e));
    } else {
        for (uint32_t k = 0; k < p->accumCount; ++k) {
            HrptPathTracerConstants cb = p->constants;
            cb.m_AccumulationIndex = p->constants.m_AccumulationIndex + k;                 // PathTracerRenderer.cpp:62,:105
            cb.m_Jitter[0] = hrpt_halton(cb.m_AccumulationIndex + 1, 2) - 0.5f;            // :65
            cb.m_Jitter[1] = hrpt_halton(cb.m_AccumulationIndex + 1, 3) - 0.5f;
            HIP_TRY(c, launch_megakernel(c->view, cb, c->dAccum, c->dOutput, c->width, rect, c->dCounters, c->stream));
        }
    }
    HIP_TRY(c, hipEventRecord(c->evStop, c->stream));
    c->timed = true;
    return HRPT_OK;
}

// No C++ exception crosses the C boundary: host-side allocation failures (std::bad_alloc on very large scenes) become status codes.
int hrpt_upload_scene(HrptContext* c, const HrptSceneDesc* s)
{
    try { return upload_scene_impl(c, s); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_upload_scene: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_upload_scene: ") + e.what()); }
}
int hrpt_refit_instances(HrptContext* c, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count)
{
    try { return update_instances_impl(c, instances, firstInstance, count, true); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_refit_instances: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_refit_instances: ") + e.what()); }
}
int hrpt_update_instances(HrptContext* c, const HrptPerInstanceData* instances, uint32_t firstInstance, uint32_t count)
{
    try { return update_instances_impl(c, instances, firstInstance, count, false); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_update_instances: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_update_instances: ") + e.what()); }
}
int hrpt_update_lights(HrptContext* c, const HrptGPULight* lights, uint32_t count)
{
    try { return update_lights_impl(c, lights, count); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_update_lights: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_update_lights: ") + e.what()); }
}
int hrpt_update_materials(HrptContext* c, const HrptMaterialConstants* materials, uint32_t firstMaterial, uint32_t count)
{
    try { return update_materials_impl(c, materials, firstMaterial, count); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_update_materials: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_update_materials: ") + e.what()); }
}
int hrpt_update_vertices(HrptContext* c, const HrptVertexQuantized* vertices, uint32_t firstVertex, uint32_t count, uint32_t flags)
{
    try { return update_vertices_impl(c, vertices, firstVertex, count, flags); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_update_vertices: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_update_vertices: ") + e.what()); }
}
int hrpt_update_vertices_device(HrptContext* c, const HrptVertexFloat* deviceVertices, uint32_t firstVertex, uint32_t count, uint32_t flags, void* stream)
{
    try { return update_vertices_device_impl(c, deviceVertices, firstVertex, count, flags, static_cast<hipStream_t>(stream)); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_update_vertices_device: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_update_vertices_device: ") + e.what()); }
}
int hrpt_update_vertices_skinned(HrptContext* c, const HrptSkinArgs* args, uint32_t firstVertex, uint32_t flags, void* stream)
{
    try { return update_vertices_skinned_impl(c, args, firstVertex, flags, static_cast<hipStream_t>(stream)); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_update_vertices_skinned: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_update_vertices_skinned: ") + e.what()); }
}
int hrpt_animate(HrptContext* c, const HrptAnimation* anim, uint32_t flags)
{
    try { return animate_impl(c, anim, flags); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_animate: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_animate: ") + e.what()); }
}
int hrpt_get_animation_device(HrptContext* c, const HrptAnimation* anim, void** palette, void** weights, void** nodeWorlds)
{
    AnimDeviceCopy* a = nullptr;
    HRPT_TRY(animation_pointers(c, "hrpt_get_animation_device", anim, a));
    if (palette) *palette = anim->jointNode.empty() ? nullptr : a->palette;
    if (weights) *weights = anim->morphWeightCount ? a->weights : nullptr;
    if (nodeWorlds) *nodeWorlds = anim->nodes.empty() ? nullptr : a->worlds;
    return HRPT_OK;
}
int hrpt_read_animation(HrptContext* c, const HrptAnimation* anim, float* palette, float* weights, float* nodeWorlds)
{
    AnimDeviceCopy* a = nullptr;
    HRPT_TRY(animation_pointers(c, "hrpt_read_animation", anim, a));
    HIP_TRY(c, hipSetDevice(c->device));
    if (palette && !anim->jointNode.empty()) HIP_TRY(c, hipMemcpyAsync(palette, a->palette, anim->jointNode.size() * 12 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (weights && anim->morphWeightCount) HIP_TRY(c, hipMemcpyAsync(weights, a->weights, anim->morphWeightCount * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (nodeWorlds && !anim->nodes.empty()) HIP_TRY(c, hipMemcpyAsync(nodeWorlds, a->worlds, anim->nodes.size() * 16 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
}
int hrpt_animation_release(HrptContext* c, const HrptAnimation* anim)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!anim) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_release: null animation");
    HIP_TRY(c, hipSetDevice(c->device));
    for (size_t i = 0; i < c->animations.size(); ++i)
        if (c->animations[i].anim == anim) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            free_animation_copy(c->animations[i]);
            c->animations.erase(c->animations.begin() + (long)i);
            break;
        }
    return HRPT_OK;
}
int hrpt_skin_vertices_device(HrptContext* c, const HrptSkinArgs* args, HrptVertexFloat* deviceOut, uint32_t* deviceStatus2, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(skin_args_check(c, "hrpt_skin_vertices_device", args));
    if (args->count == 0) return HRPT_OK;
    if (!deviceOut || (reinterpret_cast<uintptr_t>(deviceOut) & 15u) || (reinterpret_cast<uintptr_t>(deviceStatus2) & 3u))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_skin_vertices_device: deviceOut must be 16-byte aligned and not NULL, deviceStatus2 4-byte aligned");
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(args->base), out0 = reinterpret_cast<uintptr_t>(deviceOut), bytes = (uintptr_t)args->count * sizeof(HrptVertexFloat);
    if (in0 < out0 + bytes && out0 < in0 + bytes) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_skin_vertices_device: deviceOut overlaps base");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_skin_vertices(*args, deviceOut, deviceStatus2, skin_palette_mode(), static_cast<hipStream_t>(stream)));
    return HRPT_OK;
}
int hrpt_quantize_vertices_device(HrptContext* c, const HrptVertexFloat* deviceIn, uint32_t count, HrptVertexQuantized* deviceOut, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (count == 0) return HRPT_OK;
    if (!deviceIn || !deviceOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_quantize_vertices_device: null array");
    if ((reinterpret_cast<uintptr_t>(deviceIn) & 15u) || (reinterpret_cast<uintptr_t>(deviceOut) & 3u))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_quantize_vertices_device: deviceIn must be 16-byte aligned, deviceOut 4-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_quantise_vertices(deviceIn, count, deviceOut, nullptr, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
}
int hrpt_render(HrptContext* c, const HrptFrameParams* p)
{
    try { return render_impl(c, p); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_render: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_render: ") + e.what()); }
}

int hrpt_set_stream(HrptContext* c, void* hipStream, int useCallerStream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = useCallerStream ? static_cast<hipStream_t>(hipStream) : c->ownStream;   // a NULL caller stream is the legacy default stream
    return HRPT_OK;
}

int hrpt_synchronize(HrptContext* c)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
}

int hrpt_get_device_images(HrptContext* c, void** accumulation, void** output)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_device_images: hrpt_resize not called");
    if (accumulation) *accumulation = c->dAccum;
    if (output) *output = c->dOutput;
    return HRPT_OK;
}

static int read_image(HrptContext* c, const float4* src, float* dst, size_t bytes, const char* what)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!dst || !src || bytes != (size_t)c->width * c->height * 16) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": bad buffer size");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
}
int hrpt_read_accumulation(HrptContext* c, float* rgba, size_t bytes) { return read_image(c, c ? c->dAccum : nullptr, rgba, bytes, "hrpt_read_accumulation"); }
int hrpt_read_output(HrptContext* c, float* rgba, size_t bytes) { return read_image(c, c ? c->dOutput : nullptr, rgba, bytes, "hrpt_read_output"); }

// The device tables of hrpt_render_motion_vectors, (re)built from the kept copies where a flag says they are stale: the instance records after
// every upload / instance update / rebuild, indices after an upload only, positions after an upload and after hrpt_update_vertices (12 bytes
// per vertex from the kept copy, and as much again for the previous positions while a deformation lasts). A context that never asks for
// motion never gets here.
static int refresh_motion_tables(HrptContext* c)
{
    if (!c->motionInstStale && !c->motionGeometryStale && !c->motionPositionsStale) return HRPT_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // motion calls in flight still read the old tables
    std::vector<float> positions;
    const size_t pb = c->keptVertices.size() * 3 * sizeof(float);
    if (c->motionGeometryStale) {
        if (c->dMotionPositions) { (void)hipFree(c->dMotionPositions); c->dMotionPositions = nullptr; }
        if (c->dMotionPrevPositions) { (void)hipFree(c->dMotionPrevPositions); c->dMotionPrevPositions = nullptr; }
        if (c->dMotionIndices) { (void)hipFree(c->dMotionIndices); c->dMotionIndices = nullptr; }
        const size_t ib = c->keptIndices.size() * sizeof(uint32_t);
        HIP_TRY(c, hipMalloc((void**)&c->dMotionPositions, pb ? pb : 16));
        HIP_TRY(c, hipMalloc((void**)&c->dMotionIndices, ib ? ib : 16));
        if (ib) HIP_TRY(c, hipMemcpyAsync(c->dMotionIndices, c->keptIndices.data(), ib, hipMemcpyHostToDevice, c->stream));
        c->motionPositionsStale = true;
    }
    if (c->motionPositionsStale) {
        positions.resize(c->keptVertices.size() * 3);
        for (size_t i = 0; i < c->keptVertices.size(); ++i) std::memcpy(&positions[3 * i], c->keptVertices[i].m_Pos, 12);
        if (pb) HIP_TRY(c, hipMemcpyAsync(c->dMotionPositions, positions.data(), pb, hipMemcpyHostToDevice, c->stream));
        if (!c->keptPrevPositions.empty()) {            // (same size as `positions`: hrpt_update_vertices fills it for all vertices)
            if (!c->dMotionPrevPositions) HIP_TRY(c, hipMalloc((void**)&c->dMotionPrevPositions, pb ? pb : 16));
            if (pb) HIP_TRY(c, hipMemcpyAsync(c->dMotionPrevPositions, c->keptPrevPositions.data(), pb, hipMemcpyHostToDevice, c->stream));
        }
    }
    std::vector<MotionInst> records(c->keptInstances.size());
    for (size_t i = 0; i < records.size(); ++i) {
        const HrptPerInstanceData& in = c->keptInstances[i];
        MotionInst& r = records[i];
        for (int row = 0; row < 4; ++row) for (int k = 0; k < 3; ++k) r.prevWorld[row * 3 + k] = in.m_PrevWorld[row * 4 + k];
        r.firstIndex = c->keptMeshData[in.m_MeshDataIndex].m_IndexOffsets[0];         // LOD 0 (PathTracer.hlsl:102-103)
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
    }
    if (records.size() > c->motionInstCapacity || !c->dMotionInst) {
        if (c->dMotionInst) { (void)hipFree(c->dMotionInst); c->dMotionInst = nullptr; c->motionInstCapacity = 0; }
        HIP_TRY(c, hipMalloc((void**)&c->dMotionInst, records.empty() ? 64 : records.size() * sizeof(MotionInst)));
        c->motionInstCapacity = records.size();
    }
    if (!records.empty()) HIP_TRY(c, hipMemcpyAsync(c->dMotionInst, records.data(), records.size() * sizeof(MotionInst), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // the staging vectors die at scope exit
    c->motionInstStale = c->motionGeometryStale = c->motionPositionsStale = false;
    return HRPT_OK;
}

// First-hit G-buffer: the checks of render_impl that apply (no bounces, no lights), then one of the two kernel paths. No events, no counters, no
// fallback count: HrptStats keeps describing renders. hrpt_render_motion_vectors (`motion`) is the same pass with the motion plane written too
// and a planeMask that may be 0.
static int render_gbuffer_impl(HrptContext* c, const HrptFrameParams* p, uint32_t planeMask, bool motion, const HrptPlanarViewConstants* prevView)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const std::string what = motion ? "hrpt_render_motion_vectors" : "hrpt_render_gbuffer";
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": null params");
    if (motion && !prevView) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": null prevView (pass the current view for a camera that did not move)");
    if ((planeMask == 0 && !motion) || (planeMask >> HRPT_GB_PLANES) != 0)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + (motion ? ": planeMask names G-buffer planes (bits 0..5) only" : ": planeMask must name at least one of the HRPT_GB_PLANES planes and no other bit"));
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, what + ": no scene uploaded");
    if (!c->dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": hrpt_resize not called");
    if (p->accumCount != 1) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": accumCount must be 1 (the planes describe path vertex 0 of ONE accumulation index)");
    uint32_t vw = (uint32_t)p->constants.m_View.m_ViewportSize[0], vh = (uint32_t)p->constants.m_View.m_ViewportSize[1];
    if (vw != c->width || vh != c->height) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": m_ViewportSize does not match hrpt_resize");
    TileRect rect; rect.x0 = p->tileX0; rect.y0 = p->tileY0; rect.x1 = p->tileX1; rect.y1 = p->tileY1;
    rect.stripeCount = p->stripeCount ? p->stripeCount : 1u; rect.stripeIndex = p->stripeIndex;
    if (rect.stripeIndex >= rect.stripeCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": stripeIndex must be below stripeCount");
    if (rect.x0 == 0 && rect.y0 == 0 && rect.x1 == 0 && rect.y1 == 0) { rect.x1 = c->width; rect.y1 = c->height; }
    if (rect.x1 > c->width || rect.y1 > c->height || rect.x0 > rect.x1 || rect.y0 > rect.y1)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": tile rectangle outside the image");
    HIP_TRY(c, hipSetDevice(c->device));
    const bool wavefront = (p->flags & HRPT_FRAME_MEGAKERNEL) == 0;
    if (!wavefront && c->view.instances && c->traits.twoLevelStackNeed > 64u)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, what + ": this two-level structure is deeper than the validation kernel's 64-entry stack");
    const size_t bytes = (size_t)c->width * c->height * sizeof(float4);
    for (uint32_t k = 0; k < HRPT_GB_PLANES; ++k) {
        if ((planeMask & (1u << k)) && !c->dGBuffer[k]) HRPT_TRY(realloc_image(c, c->dGBuffer[k], bytes));
    }
    MotionArgs m{};
    if (motion) {
        if (!c->dMotion) HRPT_TRY(realloc_image(c, c->dMotion, bytes));
        int r = refresh_motion_tables(c);
        if (r != HRPT_OK) return r;
        m.inst = c->dMotionInst; m.positions = c->dMotionPositions; m.prevPositions = c->keptPrevPositions.empty() ? c->dMotionPositions : c->dMotionPrevPositions; m.indices = c->dMotionIndices; m.plane = c->dMotion;
        std::memcpy(m.prevWorldToClip, prevView->m_MatWorldToClip, sizeof m.prevWorldToClip);
        m.prevScale[0] = prevView->m_ClipToWindowScale[0]; m.prevScale[1] = prevView->m_ClipToWindowScale[1];
        m.prevBias[0] = prevView->m_ClipToWindowBias[0]; m.prevBias[1] = prevView->m_ClipToWindowBias[1];
    }
    if (wavefront) {
        std::string werr;
        hipError_t e = wavefront_gbuffer(c->wf, c->view, c->traits, p->constants, c->dGBuffer, planeMask, c->width, rect, c->stream, werr, motion ? &m : nullptr);
        if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? HRPT_ERR_OUT_OF_MEMORY : HRPT_ERR_HIP, "wavefront_gbuffer: " + werr + ": " + hipGetErrorString(e));
    } else if (motion) HIP_TRY(c, launch_motion_megakernel(c->view, p->constants, c->dGBuffer, planeMask, m, c->width, rect, c->stream));
    else HIP_TRY(c, launch_gbuffer_megakernel(c->view, p->constants, c->dGBuffer, planeMask, c->width, rect, c->stream));
    return HRPT_OK;
}
int hrpt_render_gbuffer(HrptContext* c, const HrptFrameParams* p, uint32_t planeMask)
{
    try { return render_gbuffer_impl(c, p, planeMask, false, nullptr); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_render_gbuffer: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_render_gbuffer: ") + e.what()); }
}
int hrpt_render_motion_vectors(HrptContext* c, const HrptFrameParams* p, const HrptPlanarViewConstants* prevView, uint32_t planeMask)
{
    try { return render_gbuffer_impl(c, p, planeMask, true, prevView); }
    catch (const std::bad_alloc&) { return fail(c, HRPT_ERR_OUT_OF_MEMORY, "hrpt_render_motion_vectors: host allocation failed"); }
    catch (const std::exception& e) { return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_render_motion_vectors: ") + e.what()); }
}
int hrpt_read_motion_vectors(HrptContext* c, float* dst, size_t bytes)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->dMotion) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_motion_vectors: the motion plane was never requested from hrpt_render_motion_vectors");
    return read_image(c, c->dMotion, dst, bytes, "hrpt_read_motion_vectors");
}
int hrpt_get_motion_vectors_device(HrptContext* c, void** devicePtr)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_motion_vectors_device: null out");
    *devicePtr = c->dMotion;
    return HRPT_OK;
}
int hrpt_read_gbuffer(HrptContext* c, uint32_t plane, void* dst, size_t bytes)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (plane >= HRPT_GB_PLANES) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_gbuffer: unknown plane");
    if (!c->dGBuffer[plane]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_gbuffer: plane " + std::to_string(plane) + " was never requested from hrpt_render_gbuffer");
    return read_image(c, c->dGBuffer[plane], static_cast<float*>(dst), bytes, "hrpt_read_gbuffer");
}
int hrpt_get_gbuffer_device(HrptContext* c, uint32_t plane, void** devicePtr)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (plane >= HRPT_GB_PLANES || !devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_gbuffer_device: unknown plane or null out");
    *devicePtr = c->dGBuffer[plane];
    return HRPT_OK;
}

int hrpt_write_accumulation(HrptContext* c, const float* rgba, size_t bytes)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!rgba || !c->dAccum || bytes != (size_t)c->width * c->height * 16) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_write_accumulation: bad buffer size");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->dAccum, rgba, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
}

int hrpt_resolve_output(HrptContext* c)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_output: hrpt_resize not called");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_resolve(c->dAccum, c->dOutput, c->width * c->height, c->stream));
    return HRPT_OK;
}

int hrpt_resolve_device(HrptContext* c, const float* accumulationDevice, float* outputDevice, uint64_t pixelCount, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!accumulationDevice || !outputDevice) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_device: null image");
    if (pixelCount == 0) return HRPT_OK;
    if (pixelCount > 0xFFFFFFFFull) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_device: image too large");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_resolve(reinterpret_cast<const float4*>(accumulationDevice), reinterpret_cast<float4*>(outputDevice), (uint32_t)pixelCount,
                              static_cast<hipStream_t>(stream)));
    return HRPT_OK;
}

int hrpt_allgather(HrptContext* const* ranks, int n)
{
    if (!ranks || n <= 0) return HRPT_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; ++i) if (!ranks[i]) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c0 = ranks[0];
    const uint32_t W = c0->width, H = c0->height;
    if (!c0->dAccum || W == 0 || H == 0) return fail(c0, HRPT_ERR_INVALID_ARGUMENT, "hrpt_allgather: hrpt_resize not called");
    if (H % (uint32_t)n != 0) return fail(c0, HRPT_ERR_INVALID_ARGUMENT, "hrpt_allgather: image height must be a multiple of the number of ranks");
    for (int i = 0; i < n; ++i) {
        if (ranks[i]->width != W || ranks[i]->height != H || !ranks[i]->dAccum) return fail(c0, HRPT_ERR_INVALID_ARGUMENT, "hrpt_allgather: contexts differ in image size");
        for (int j = 0; j < i; ++j) if (ranks[j] == ranks[i]) return fail(c0, HRPT_ERR_INVALID_ARGUMENT, "hrpt_allgather: the same context appears twice");
    }
    const size_t rows = H / (uint32_t)n, bandBytes = rows * (size_t)W * sizeof(float4);
    std::vector<hipEvent_t> sent((size_t)n, nullptr);
    auto cleanup = [&]() { for (hipEvent_t e : sent) if (e) (void)hipEventDestroy(e); };
    // every rank pushes its band to all the others on its own stream, then marks the point where its sends are enqueued
    for (int i = 0; i < n; ++i) {
        HrptContext* src = ranks[i];
        hipError_t e = hipSetDevice(src->device);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sent[(size_t)i], hipEventDisableTiming);
        const size_t off = (size_t)i * rows * W;
        for (int j = 0; j < n && e == hipSuccess; ++j) {
            if (j == i) continue;
            HrptContext* dst = ranks[j];
            // the destination band must not be in use by the destination's earlier work (e.g. its previous resolve): order behind it
            hipEvent_t ready = nullptr;
            e = hipSetDevice(dst->device);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(ready, dst->stream);
            if (e == hipSuccess) e = hipSetDevice(src->device);
            if (e == hipSuccess) e = hipStreamWaitEvent(src->stream, ready, 0);
            if (e == hipSuccess) e = hipMemcpyPeerAsync(dst->dAccum + off, dst->device, src->dAccum + off, src->device, bandBytes, src->stream);
            if (ready) (void)hipEventDestroy(ready);
        }
        if (e == hipSuccess) e = hipEventRecord(sent[(size_t)i], src->stream);
        if (e != hipSuccess) { cleanup(); return fail(c0, HRPT_ERR_HIP, std::string("hrpt_allgather (send): ") + hipGetErrorString(e)); }
    }
    // every rank waits for all senders, then resolves its now complete image
    for (int j = 0; j < n; ++j) {
        HrptContext* dst = ranks[j];
        hipError_t e = hipSetDevice(dst->device);
        for (int i = 0; i < n && e == hipSuccess; ++i) if (i != j) e = hipStreamWaitEvent(dst->stream, sent[(size_t)i], 0);
        if (e == hipSuccess) e = launch_resolve(dst->dAccum, dst->dOutput, W * H, dst->stream);
        if (e != hipSuccess) { cleanup(); return fail(c0, HRPT_ERR_HIP, std::string("hrpt_allgather (receive): ") + hipGetErrorString(e)); }
    }
    cleanup();      // destroying a recorded event is deferred by the runtime until the waits that reference it have run
    return HRPT_OK;
}

int hrpt_trace_rays(HrptContext* c, const HrptRay* rays, HrptRayHit* hits, uint64_t count, uint32_t flags)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!rays || !hits) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: null array");
    if ((flags & 0xFFu) > HRPT_RAYS_SHADOW || (flags & ~(0xFFu | HRPT_RAYS_DEVICE_POINTERS | HRPT_RAYS_THREAD_PER_RAY))) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: unknown flags");
    if (count > (1ull << 31)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: too many rays in one call");
    if (c->view.instances && ((flags & HRPT_RAYS_THREAD_PER_RAY) || !wavefront_trace_rays_supported(c->traits)) && c->traits.twoLevelStackNeed > 64u)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_trace_rays: this two-level structure is deeper than the thread-per-ray kernel's 64-entry stack");
    HIP_TRY(c, hipSetDevice(c->device));
    const bool shadow = (flags & 0xFFu) == HRPT_RAYS_SHADOW;
    // the persistent refilling traversal kernel (pt_wavefront.hip wf_trace_rays); the thread-per-ray kernel stays as the fallback for trees
    // deeper than its stacks allow and as the cross-check (HRPT_RAYS_THREAD_PER_RAY)
    const bool persistent = !(flags & HRPT_RAYS_THREAD_PER_RAY) && wavefront_trace_rays_supported(c->traits) && c->view.node4Count > 0;
    auto trace = [&](const HrptRay* dr, HrptRayHit* dh) -> hipError_t {
        if (!persistent) return launch_trace_rays(c->view, dr, dh, count, shadow, c->stream);
        std::string werr;
        hipError_t te = wavefront_trace_rays(c->wf, c->view, c->traits, dr, dh, count, shadow, c->stream, werr);
        if (te != hipSuccess) c->err = "hrpt_trace_rays: " + werr;
        return te;
    };
    if (flags & HRPT_RAYS_DEVICE_POINTERS) {
        HIP_TRY(c, trace(rays, hits));
        return HRPT_OK;
    }
    HrptRay* dRays = nullptr; HrptRayHit* dHits = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dRays), count * sizeof(HrptRay));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dHits), count * sizeof(HrptRayHit));
    if (e == hipSuccess) e = hipMemcpyAsync(dRays, rays, count * sizeof(HrptRay), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = trace(dRays, dHits);
    if (e == hipSuccess) e = hipMemcpyAsync(hits, dHits, count * sizeof(HrptRayHit), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (dRays) (void)hipFree(dRays);
    if (dHits) (void)hipFree(dHits);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? HRPT_ERR_OUT_OF_MEMORY : HRPT_ERR_HIP, std::string("hrpt_trace_rays: ") + hipGetErrorString(e));
    return HRPT_OK;
}

int hrpt_resolve_columns_device(HrptContext* c, const float* shardsDevice, float* accumulationDevice, float* outputDevice, uint32_t width, uint32_t height, uint32_t ranks, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!shardsDevice || !outputDevice) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_columns_device: null image");
    if (ranks == 0 || width == 0 || height == 0 || width % (8u * ranks) != 0) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_columns_device: width must be a positive multiple of 8 * ranks");
    if ((uint64_t)width * height > 0xFFFFFFFFull) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resolve_columns_device: image too large");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_resolve_columns(reinterpret_cast<const float4*>(shardsDevice), reinterpret_cast<float4*>(accumulationDevice), reinterpret_cast<float4*>(outputDevice),
                                      width, height, ranks, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
}

int hrpt_set_shadow_overlap(HrptContext* c, int enabled)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    c->wf.knobs.serialShadow = enabled == 0;
    return HRPT_OK;
}

int hrpt_set_acceleration_structure(HrptContext* c, int structure)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (structure < HRPT_ACCEL_AUTO || structure > HRPT_ACCEL_TWO_LEVEL) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_set_acceleration_structure: unknown structure");
    c->accelStructure = structure;
    return HRPT_OK;
}

int hrpt_set_bvh_builder(HrptContext* c, int builder)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (builder != HRPT_BVH_BUILDER_HOST_SAH && builder != HRPT_BVH_BUILDER_GPU_LBVH && builder != HRPT_BVH_BUILDER_GPU_PLOC && builder != HRPT_BVH_BUILDER_AUTO) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_set_bvh_builder: unknown builder");
    c->bvhBuilder = builder;
    return HRPT_OK;
}

int hrpt_get_build_info(HrptContext* c, HrptBuildInfo* out)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_build_info: null out");
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_build_info: no scene uploaded");
    *out = c->buildInfo;
    return HRPT_OK;
}

int hrpt_get_stats(HrptContext* c, HrptStats* out)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_stats: null out");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    DeviceCounters h[kCounterShards];
    HIP_TRY(c, hipMemcpy(h, c->dCounters, sizeof h, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    DeviceCounters total{};
    for (int i = 0; i < kCounterShards; ++i) {
        total.closestRays += h[i].closestRays; total.shadowRays += h[i].shadowRays; total.paths += h[i].paths; total.neeEntries += h[i].neeEntries;
        total.neeSamples += h[i].neeSamples; total.radianceShade += h[i].radianceShade; total.radianceShadow += h[i].radianceShadow; total.skipped16 += h[i].skipped16;
        total.fusedPaths += h[i].fusedPaths; total.fusedEntries += h[i].fusedEntries;
    }
    out->closestRays = total.closestRays; out->shadowRays = total.shadowRays; out->paths = total.paths;
    out->neeEntries = total.neeEntries; out->neeSamples = total.neeSamples;
    out->megakernelFallbacks = c->megakernelFallbacks; out->queuePoolBytes = c->wf.poolBytes;
    if (total.neeEntries || c->wf.raygenBytes || c->wf.resolveBytes) {     // the wavefront pipeline ran since the last reset
        wavefront_queue_bytes(c->wf, total, out->traceQueueBytes, out->shadeQueueBytes, out->shadowQueueBytes);
        out->raygenQueueBytes = c->wf.raygenBytes; out->resolveQueueBytes = c->wf.resolveBytes;
    }
    if (c->timed) { float ms = 0.0f; if (hipEventElapsedTime(&ms, c->evStart, c->evStop) == hipSuccess) out->lastRenderMs = ms; }
    wavefront_collect_timing(c->wf);
    out->traceKernelMs = c->wf.kernelMs[0]; out->traceKernelLaunches = c->wf.kernelLaunches[0];
    out->shadeKernelMs = c->wf.kernelMs[1]; out->shadeKernelLaunches = c->wf.kernelLaunches[1];
    out->shadowKernelMs = c->wf.kernelMs[2]; out->shadowKernelLaunches = c->wf.kernelLaunches[2];
    out->raygenKernelMs = c->wf.kernelMs[3]; out->raygenKernelLaunches = c->wf.kernelLaunches[3];
    out->resolveKernelMs = c->wf.kernelMs[4]; out->resolveKernelLaunches = c->wf.kernelLaunches[4];
    out->bvhNodeCount = c->bvhNodes; out->bvhTriangleCount = c->bvhTris; out->bvhMaxDepth = c->traits.bvhMaxDepth;
    return HRPT_OK;
}

int hrpt_post_process(HrptContext* c, const HrptPostParams* p)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_post_process: null params");
    if (!c->dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_post_process: hrpt_resize not called");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->dExposure) {
        HIP_TRY(c, hipMalloc((void**)&c->dExposure, 16));
        HIP_TRY(c, hipMalloc((void**)&c->dHistogram, 256 * sizeof(uint32_t)));
        const float one[4] = { 1.0f, 0.0f, 0.0f, 0.0f };
        HIP_TRY(c, hipMemcpy(c->dExposure, one, 16, hipMemcpyHostToDevice));
    }
    if (!c->dDisplay) HIP_TRY(c, hipMalloc((void**)&c->dDisplay, (size_t)c->width * c->height * sizeof(float4)));
    HIP_TRY(c, launch_post_chain(c->dOutput, c->dDisplay, c->width * c->height, *p, c->dHistogram, c->dExposure, c->stream));
    return HRPT_OK;
}

// ---- screen-space stages: bloom, temporal accumulation, denoise, demodulate / compose ----
// What the _host, _device and context entry points of a stage with a view check alike, in this order, after their null checks and, for
// caller-owned images, the image checks: the size, then the view against it. The stage's parameter rule follows.
static bool view_matches(const HrptPlanarViewConstants& view, uint32_t width, uint32_t height)
{
    return view.m_ViewportSize[0] == (float)width && view.m_ViewportSize[1] == (float)height;
}
static int size_and_view_check(HrptContext* c, const std::string& w, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view)
{
    if (!size_ok(width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": size must be 1..65535");
    if (!view_matches(view, width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": view->m_ViewportSize does not match the image size");
    return HRPT_OK;
}

// Threads of a host executor: 0 or less = one per hardware thread up to 16; at most 256.
static int host_threads(int nthreads)
{
    if (nthreads <= 0) { nthreads = (int)std::thread::hardware_concurrency(); if (nthreads > 16) nthreads = 16; }
    if (nthreads < 1) nthreads = 1;
    return nthreads > 256 ? 256 : nthreads;
}

// No C++ exception crosses the C boundary: what a host executor may throw (its buffers, its threads) becomes a status code. A template, so
// that the call itself allocates nothing; templates need C++ linkage.
extern "C++" template <class Fn> static int run_host(const char* what, Fn fn)
{
    try { fn(); }
    catch (const std::bad_alloc&) { return fail(nullptr, HRPT_ERR_OUT_OF_MEMORY, std::string(what) + ": out of memory"); }
    catch (const std::system_error& e) { return fail(nullptr, HRPT_ERR_UNSUPPORTED, std::string(what) + ": " + e.what()); }
    return HRPT_OK;
}

// Pyramids for a width x height image: kept while the size stays, re-allocated when it changes (hipFree waits for work in flight).
static int bloom_run(HrptContext* c, float4* image, uint32_t width, uint32_t height, const HrptBloomParams& p, hipStream_t stream)
{
    const size_t words = bloom_pyramid_words(width, height);
    if (words == 0) return HRPT_OK;
    if (words != c->bloomWords) {
        if (c->dBloomDown) { (void)hipFree(c->dBloomDown); c->dBloomDown = nullptr; }
        if (c->dBloomUp) { (void)hipFree(c->dBloomUp); c->dBloomUp = nullptr; }
        c->bloomWords = 0;
        HIP_TRY(c, hipMalloc((void**)&c->dBloomDown, words * sizeof(uint32_t)));
        HIP_TRY(c, hipMalloc((void**)&c->dBloomUp, words * sizeof(uint32_t)));
        c->bloomWords = words;
    }
    HIP_TRY(c, launch_bloom(image, width, height, p, c->dBloomDown, c->dBloomUp, c->bloomTailTexels, stream));
    return HRPT_OK;
}

int hrpt_bloom(HrptContext* c, const HrptBloomParams* p)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom: null params");
    if (!bloom_params_valid(*p)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom: knee, intensity and upsampleRadius must be finite and >= 0");
    if (!c->dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom: hrpt_resize not called");
    HIP_TRY(c, hipSetDevice(c->device));
    return bloom_run(c, c->dOutput, c->width, c->height, *p, c->stream);
}

int hrpt_bloom_device(HrptContext* c, float* hdrDevice, uint32_t width, uint32_t height, const HrptBloomParams* p, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_device: null params");
    if (!hdrDevice) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_device: null image");
    if (!size_ok(width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_device: size must be 1..65535");
    if (!bloom_params_valid(*p)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_device: knee, intensity and upsampleRadius must be finite and >= 0");
    HIP_TRY(c, hipSetDevice(c->device));
    return bloom_run(c, reinterpret_cast<float4*>(hdrDevice), width, height, *p, static_cast<hipStream_t>(stream));
}

int hrpt_bloom_host(const float* hdrIn, float* hdrOut, uint32_t width, uint32_t height, const HrptBloomParams* p, int nthreads)
{
    if (!p) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_host: null params");
    if (!hdrIn || !hdrOut) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_host: null image");
    if (!size_ok(width, height)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_host: size must be 1..65535");
    if (!bloom_params_valid(*p)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_host: knee, intensity and upsampleRadius must be finite and >= 0");
    return run_host("hrpt_bloom_host", [&] { bloom_host(hdrIn, hdrOut, width, height, *p, host_threads(nthreads)); });
}

int hrpt_bloom_pack_probe(const float* rgb, uint32_t count, uint32_t* packed, float* unpackedRgb)
{
    if (!rgb && count) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_pack_probe: null input");
    bloom_pack_probe(rgb, count, packed, unpackedRgb);
    return HRPT_OK;
}

// ---- temporal accumulation (pt_temporal.h / pt_temporal.hip) ----
// Size, view and parameters: all a context call has left to check once its arguments are not null (its images are the context's own).
static int temporal_args_check(HrptContext* c, const std::string& w, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view, const HrptTemporalParams& p)
{
    HRPT_TRY(size_and_view_check(c, w, width, height, view));
    if (!temporal_params_valid(p)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": blend must be finite and in [0, 1], flags HRPT_TEMPORAL_* only, reserved 0");
    return HRPT_OK;
}
// Caller-owned images: the null checks and the aliasing rule first, then the above.
static int temporal_check(HrptContext* c, const char* what, const HrptTemporalImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                          const HrptPlanarViewConstants* prevView, const HrptTemporalParams* p)
{
    const std::string w(what);
    if (!img || !view || !prevView || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null argument");
    if (!img->color || !img->motion || !img->depth || !img->normal || !img->historyOut || !img->colorOut)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null image (only historyIn may be NULL)");
    if (img->historyOut == img->historyIn) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": historyOut must differ from historyIn");
    return temporal_args_check(c, w, width, height, *view, *p);
}

int hrpt_temporal_host(const HrptTemporalImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                       const HrptPlanarViewConstants* prevView, const HrptTemporalParams* p, int nthreads)
{
    HRPT_TRY(temporal_check(nullptr, "hrpt_temporal_host", img, width, height, view, prevView, p));
    return run_host("hrpt_temporal_host", [&] { temporal_host(*img, width, height, *view, *prevView, *p, host_threads(nthreads)); });
}

int hrpt_temporal_device(HrptContext* c, const HrptTemporalImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                         const HrptPlanarViewConstants* prevView, const HrptTemporalParams* p, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(temporal_check(c, "hrpt_temporal_device", img, width, height, view, prevView, p));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_temporal(*img, width, height, *view, *prevView, *p, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
}

int hrpt_temporal_accumulate(HrptContext* c, const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView, const HrptTemporalParams* p)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!view || !prevView || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_temporal_accumulate: null argument");
    if (!c->dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_temporal_accumulate: hrpt_resize not called");
    if (!c->dMotion || !c->dGBuffer[HRPT_GB_DEPTH] || !c->dGBuffer[HRPT_GB_NORMAL])
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_temporal_accumulate: the motion, depth or normal plane was never requested (hrpt_render_motion_vectors with planeMask = DEPTH | NORMAL fills them)");
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(temporal_args_check(c, "hrpt_temporal_accumulate", c->width, c->height, *view, *p));      // before anything is allocated
    const bool fresh = !c->dTemporal[0];
    const int next = fresh ? 0 : 1 - c->temporalCur;
    if (fresh) {
        for (float4*& image : c->dTemporal) HRPT_TRY(realloc_image(c, image, (size_t)c->width * c->height * sizeof(float4)));
        c->temporalValid = false;
    }
    HrptTemporalImages img{};
    img.color = reinterpret_cast<const float*>(c->dOutput); img.colorOut = reinterpret_cast<float*>(c->dOutput);
    img.motion = reinterpret_cast<const float*>(c->dMotion);
    img.depth = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_DEPTH]); img.normal = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_NORMAL]);
    const bool useHistory = c->temporalValid && (p->flags & HRPT_TEMPORAL_RESET) == 0;
    img.historyIn = useHistory ? reinterpret_cast<const float*>(c->dTemporal[1 - next]) : nullptr;
    img.historyOut = reinterpret_cast<float*>(c->dTemporal[next]);
    HIP_TRY(c, launch_temporal(img, c->width, c->height, *view, *prevView, *p, c->stream));
    c->temporalCur = next; c->temporalValid = true;
    return HRPT_OK;
}

int hrpt_read_temporal_history(HrptContext* c, float* dst, size_t bytes)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->dTemporal[0]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_temporal_history: the history was never requested from hrpt_temporal_accumulate");
    return read_image(c, c->dTemporal[c->temporalCur], dst, bytes, "hrpt_read_temporal_history");
}

int hrpt_get_temporal_history_device(HrptContext* c, void** devicePtr)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_temporal_history_device: null out");
    *devicePtr = c->dTemporal[0] ? c->dTemporal[c->temporalCur] : nullptr;
    return HRPT_OK;
}

// ---- denoise (pt_denoise.h / pt_denoise.hip) ----
// Size, view and parameters: all a context call has left to check once its arguments are not null (its images are the context's own).
static int denoise_args_check(HrptContext* c, const std::string& w, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view, const HrptDenoiseParams& p,
                              bool singlePass)
{
    HRPT_TRY(size_and_view_check(c, w, width, height, view));
    if (!denoise_params_valid(p))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": radius and phi must be finite and > 0, the other phis finite and >= 0, iterations 1..5 with radius * 2^(iterations - 1) finite, flags HRPT_DENOISE_* only, reserved 0");
    if (singlePass && p.iterations != 1u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": one pass per call, iterations must be 1 (hrpt_denoise iterates)");
    return HRPT_OK;
}
// Caller-owned images, one pass: the null checks and the aliasing rules first, then the above.
static int denoise_check(HrptContext* c, const char* what, const HrptDenoiseImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                         const HrptDenoiseParams* p)
{
    const std::string w(what);
    if (!img || !view || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null argument");
    if (!img->input || !img->depth || !img->normal || !img->geoNormal || !img->output)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null image (only noise, and color with colorOut, may be NULL)");
    if ((img->color == nullptr) != (img->colorOut == nullptr)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": color and colorOut must both be NULL or both be set");
    if (img->output == img->input) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": output must differ from input");
    if (img->color && (img->color == img->input || img->colorOut == img->input)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": color and colorOut must differ from input");
    return denoise_args_check(c, w, width, height, *view, *p, true);
}

static int denoise_tile(HrptContext* c)
{
    if (c->dDenoiseTile) return HRPT_OK;
    std::vector<float> tile(denoise_noise_floats());
    denoise_default_tile(tile.data());
    float* d = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d, tile.size() * sizeof(float)));
    hipError_t e = hipMemcpy(d, tile.data(), tile.size() * sizeof(float), hipMemcpyHostToDevice);     // complete on return: ordered before every later launch
    if (e != hipSuccess) { (void)hipFree(d); HIP_TRY(c, e); }
    c->dDenoiseTile = d;
    return HRPT_OK;
}

int hrpt_set_denoise_noise(HrptContext* c, const float* hostTile)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const size_t count = denoise_noise_floats();
    std::vector<float> tile(count);
    if (hostTile) {
        for (size_t i = 0; i < count; ++i) {
            if (!std::isfinite(hostTile[i])) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_set_denoise_noise: the tile holds a value that is not finite");
            tile[i] = hostTile[i];
        }
    } else denoise_default_tile(tile.data());
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(denoise_tile(c));
    // on the context stream: passes enqueued before this call still read the old tile. The source is pageable and local, so wait for the copy.
    HIP_TRY(c, hipMemcpyAsync(c->dDenoiseTile, tile.data(), count * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
}

int hrpt_denoise_host(const HrptDenoiseImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view, const HrptDenoiseParams* p, int nthreads)
{
    HRPT_TRY(denoise_check(nullptr, "hrpt_denoise_host", img, width, height, view, p));
    return run_host("hrpt_denoise_host", [&] { denoise_host(*img, width, height, *view, *p, host_threads(nthreads)); });
}

int hrpt_denoise_device(HrptContext* c, const HrptDenoiseImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                        const HrptDenoiseParams* p, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(denoise_check(c, "hrpt_denoise_device", img, width, height, view, p));
    HIP_TRY(c, hipSetDevice(c->device));
    HrptDenoiseImages im = *img;
    if (!im.noise) { HRPT_TRY(denoise_tile(c)); im.noise = c->dDenoiseTile; }
    HIP_TRY(c, launch_denoise(im, width, height, *view, *p, p->radius, p->frame, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
}

int hrpt_denoise(HrptContext* c, const HrptPlanarViewConstants* view, const HrptDenoiseParams* p)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!view || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_denoise: null argument");
    if (!c->dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_denoise: hrpt_resize not called");
    if (!c->dTemporal[0] || !c->temporalValid)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_denoise: no temporal history at the current size (hrpt_temporal_accumulate writes the image this stage filters)");
    if (!c->dGBuffer[HRPT_GB_DEPTH] || !c->dGBuffer[HRPT_GB_NORMAL] || !c->dGBuffer[HRPT_GB_GEO_NORMAL])
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_denoise: the depth, normal or geo-normal plane was never requested (hrpt_render_motion_vectors with planeMask = DEPTH | NORMAL | GEO_NORMAL fills them)");
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(denoise_args_check(c, "hrpt_denoise", c->width, c->height, *view, *p, false));
    HRPT_TRY(denoise_tile(c));
    HrptDenoiseImages img{};
    img.input = reinterpret_cast<const float*>(c->dTemporal[c->temporalCur]);
    img.depth = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_DEPTH]); img.normal = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_NORMAL]);
    img.geoNormal = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_GEO_NORMAL]);
    img.noise = c->dDenoiseTile;
    const bool outputOnly = (p->flags & HRPT_DENOISE_OUTPUT_ONLY) != 0;
    if (outputOnly) {
        const size_t bytes = (size_t)c->width * c->height * sizeof(float4);
        for (uint32_t k = 0; k < (p->iterations > 1u ? 2u : 1u); ++k)
            if (!c->dDenoiseScratch[k]) HIP_TRY(c, hipMalloc((void**)&c->dDenoiseScratch[k], bytes));
    }
    int cur = c->temporalCur;
    for (uint32_t i = 0; i < p->iterations; ++i) {
        // default: the two history images are the ping-pong pair (the stale one is free after the temporal call); the image a pass wrote is the history
        float4* dst = outputOnly ? c->dDenoiseScratch[i & 1u] : c->dTemporal[1 - cur];
        img.output = reinterpret_cast<float*>(dst);
        const bool last = i + 1u == p->iterations;
        img.color = last ? reinterpret_cast<const float*>(c->dOutput) : nullptr;
        img.colorOut = last ? reinterpret_cast<float*>(c->dOutput) : nullptr;
        HIP_TRY(c, launch_denoise(img, c->width, c->height, *view, *p, p->radius * (float)(1u << i), p->frame * p->iterations + i, c->stream));
        img.input = reinterpret_cast<const float*>(dst);
        if (!outputOnly) { cur = 1 - cur; c->temporalCur = cur; }
    }
    return HRPT_OK;
}

// ---- demodulate / compose (pt_modulation.h / pt_modulation.hip) ----
// Size, view and parameters: all a context call has left to check once its arguments are not null (its images are the context's own).
static int demodulate_args_check(HrptContext* c, const std::string& w, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view, const HrptModulationParams& p)
{
    HRPT_TRY(size_and_view_check(c, w, width, height, view));
    if (!modulation_params_valid(p)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": floor must be finite and > 0, flags 0, reserved 0");
    return HRPT_OK;
}
// Caller-owned images: the null checks and the aliasing rules first, then the above.
static int demodulate_check(HrptContext* c, const char* what, const HrptDemodulateImages* img, uint32_t width, uint32_t height,
                            const HrptPlanarViewConstants* view, const HrptModulationParams* p)
{
    const std::string w(what);
    if (!img || !view || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null argument");
    if (!img->color || !img->albedo || !img->normal || !img->geoNormal || !img->depth || !img->colorOut || !img->modulationOut)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null image (only emissive may be NULL)");
    const float* inputs[6] = { img->color, img->albedo, img->normal, img->geoNormal, img->depth, img->emissive };
    for (const float* in : inputs)
        if (in && img->modulationOut == in) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": modulationOut must differ from every input");
    if (img->modulationOut == img->colorOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": modulationOut must differ from colorOut");
    for (int i = 1; i < 6; ++i)
        if (inputs[i] && img->colorOut == inputs[i]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": colorOut may equal color, but no other input");
    return demodulate_args_check(c, w, width, height, *view, *p);
}

static int compose_check(HrptContext* c, const char* what, const HrptComposeImages* img, uint32_t width, uint32_t height)
{
    const std::string w(what);
    if (!img) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null argument");
    if (!img->color || !img->modulation || !img->colorOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null image (only emissive may be NULL)");
    if (img->colorOut == img->modulation || (img->emissive && img->colorOut == img->emissive))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": colorOut may equal color, but not modulation or emissive");
    if (!size_ok(width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": size must be 1..65535");
    return HRPT_OK;
}

int hrpt_demodulate_host(const HrptDemodulateImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                         const HrptModulationParams* p, int nthreads)
{
    HRPT_TRY(demodulate_check(nullptr, "hrpt_demodulate_host", img, width, height, view, p));
    return run_host("hrpt_demodulate_host", [&] { demodulate_host(*img, width, height, *view, *p, host_threads(nthreads)); });
}

int hrpt_quantize_vertices_host(const HrptVertexFloat* in, uint32_t count, HrptVertexQuantized* out, int nthreads)
{
    if (count == 0) return HRPT_OK;
    if (!in || !out) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_quantize_vertices_host: null array");
    return run_host("hrpt_quantize_vertices_host", [&] { (void)quantize_vertices_host(in, count, out, host_threads(nthreads)); });
}
// ---- keyframe animation without a context: the tables, the clock and the host executor (csrc/pt_anim_host.cpp) ----
int hrpt_animation_create(const HrptAnimationDesc* desc, HrptAnimation** out)
{
    if (!out) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_create: null out");
    *out = nullptr;
    if (!desc) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_create: null desc");
    std::string err;
    HRPT_TRY(run_host("hrpt_animation_create", [&] { *out = animation_create(*desc, err); }));
    return *out ? HRPT_OK : fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_create: " + err);
}
void hrpt_animation_destroy(HrptAnimation* anim) { delete anim; }
int hrpt_animation_advance(HrptAnimation* anim, float dt)
{
    if (!anim) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_advance: null animation");
    animation_advance(*anim, dt);
    return HRPT_OK;
}
int hrpt_animation_set_times(HrptAnimation* anim, const float* times, uint32_t count)
{
    if (!anim || count != anim->times.size() || (count && !times)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_set_times: null argument, or count is not the animation count");
    for (uint32_t i = 0; i < count; ++i) anim->times[i] = times[i];
    return HRPT_OK;
}
int hrpt_animation_get_times(const HrptAnimation* anim, float* times, float* durations, uint32_t count)
{
    if (!anim || count != anim->times.size()) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animation_get_times: null animation, or count is not the animation count");
    for (uint32_t i = 0; i < count; ++i) { if (times) times[i] = anim->times[i]; if (durations) durations[i] = anim->durations[i]; }
    return HRPT_OK;
}
int hrpt_animate_host(const HrptAnimation* anim, const HrptPerInstanceData* prevInstances, HrptPerInstanceData* instancesInOut, uint32_t instanceCount,
                      float* paletteOut, float* weightsOut, float* nodeWorldsOut, int nthreads)
{
    if (!anim) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate_host: null animation");
    if (instancesInOut && anim->instanceNeed > instanceCount) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_animate_host: an instance index of the animation exceeds instanceCount");
    return run_host("hrpt_animate_host", [&] {
        if (instancesInOut && prevInstances && prevInstances != instancesInOut) std::memmove(instancesInOut, prevInstances, (size_t)instanceCount * sizeof(HrptPerInstanceData));
        animate_host(*anim, instancesInOut, instancesInOut ? instanceCount : 0u, paletteOut, weightsOut, nodeWorldsOut, host_threads(nthreads));
    });
}

int hrpt_skin_vertices_host(const HrptSkinArgs* args, HrptVertexFloat* out, int nthreads)
{
    HRPT_TRY(skin_args_check(nullptr, "hrpt_skin_vertices_host", args));
    if (args->count == 0) return HRPT_OK;
    if (!out) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_skin_vertices_host: null out");
    uint32_t status = 0;
    HRPT_TRY(run_host("hrpt_skin_vertices_host", [&] { status = skin_vertices_host(*args, out, host_threads(nthreads)); }));
    if (status & skin::kJointOutOfRange) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_skin_vertices_host: joint index out of range");
    return HRPT_OK;
}
int hrpt_compose_host(const HrptComposeImages* img, uint32_t width, uint32_t height, int nthreads)
{
    HRPT_TRY(compose_check(nullptr, "hrpt_compose_host", img, width, height));
    return run_host("hrpt_compose_host", [&] { compose_host(*img, width, height, host_threads(nthreads)); });
}

int hrpt_demodulate_device(HrptContext* c, const HrptDemodulateImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                           const HrptModulationParams* p, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(demodulate_check(c, "hrpt_demodulate_device", img, width, height, view, p));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_demodulate(*img, width, height, *view, *p, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
}

int hrpt_compose_device(HrptContext* c, const HrptComposeImages* img, uint32_t width, uint32_t height, void* stream)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(compose_check(c, "hrpt_compose_device", img, width, height));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_compose(*img, width, height, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
}

int hrpt_demodulate(HrptContext* c, const HrptPlanarViewConstants* view, const HrptModulationParams* p)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!view || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_demodulate: null argument");
    if (!c->dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_demodulate: hrpt_resize not called");
    static const struct { int plane; const char* name; } needed[5] = { { HRPT_GB_ALBEDO, "HRPT_GB_ALBEDO" }, { HRPT_GB_NORMAL, "HRPT_GB_NORMAL" },
        { HRPT_GB_GEO_NORMAL, "HRPT_GB_GEO_NORMAL" }, { HRPT_GB_EMISSIVE, "HRPT_GB_EMISSIVE" }, { HRPT_GB_DEPTH, "HRPT_GB_DEPTH" } };
    for (const auto& n : needed)
        if (!c->dGBuffer[n.plane])
            return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_demodulate: the plane ") + n.name + " was never requested (hrpt_render_motion_vectors or hrpt_render_gbuffer with planeMask = ALBEDO | NORMAL | GEO_NORMAL | EMISSIVE | DEPTH fills them)");
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(demodulate_args_check(c, "hrpt_demodulate", c->width, c->height, *view, *p));      // before anything is allocated
    if (!c->dModulation) HIP_TRY(c, hipMalloc((void**)&c->dModulation, (size_t)c->width * c->height * sizeof(float4)));
    HrptDemodulateImages img{};
    img.color = reinterpret_cast<const float*>(c->dOutput); img.colorOut = reinterpret_cast<float*>(c->dOutput);
    img.albedo = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_ALBEDO]); img.normal = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_NORMAL]);
    img.geoNormal = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_GEO_NORMAL]); img.depth = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_DEPTH]);
    img.emissive = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_EMISSIVE]);
    img.modulationOut = reinterpret_cast<float*>(c->dModulation);
    HIP_TRY(c, launch_demodulate(img, c->width, c->height, *view, *p, c->stream));
    return HRPT_OK;
}

int hrpt_compose(HrptContext* c)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_compose: hrpt_resize not called");
    if (!c->dModulation)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_compose: no modulation image at the current size (hrpt_demodulate writes the factor this stage multiplies back in)");
    HIP_TRY(c, hipSetDevice(c->device));
    HrptComposeImages img{};
    img.color = reinterpret_cast<const float*>(c->dOutput); img.colorOut = reinterpret_cast<float*>(c->dOutput);
    img.modulation = reinterpret_cast<const float*>(c->dModulation);
    img.emissive = reinterpret_cast<const float*>(c->dGBuffer[HRPT_GB_EMISSIVE]);      // set: hrpt_demodulate required it, and a resize drops the modulation image
    HIP_TRY(c, launch_compose(img, c->width, c->height, c->stream));
    return HRPT_OK;
}

int hrpt_read_modulation(HrptContext* c, float* dst, size_t bytes)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->dModulation) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_modulation: no modulation image at the current size (hrpt_demodulate writes it)");
    return read_image(c, c->dModulation, dst, bytes, "hrpt_read_modulation");
}

int hrpt_get_modulation_device(HrptContext* c, void** devicePtr)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_modulation_device: null out");
    *devicePtr = c->dModulation;
    return HRPT_OK;
}

int hrpt_modulation_probe(const float* albedo3, const float* N3, const float* V3, float rough, float metal, float floor, float* outM3)
{
    if (!albedo3 || !N3 || !V3 || !outM3) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_modulation_probe: null argument");
    modulation_probe(albedo3, N3, V3, rough, metal, floor, outM3);
    return HRPT_OK;
}

int hrpt_clear_accumulation(HrptContext* c)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_clear_accumulation: hrpt_resize not called");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->dAccum, 0, (size_t)c->width * c->height * sizeof(float4), c->stream));
    return HRPT_OK;
}

int hrpt_read_display(HrptContext* c, float* rgba, size_t bytes) { return read_image(c, c ? c->dDisplay : nullptr, rgba, bytes, "hrpt_read_display"); }

int hrpt_get_exposure(HrptContext* c, float* exposure, uint32_t histogram256[256])
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!exposure || !c->dExposure) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_exposure: no post pass has run");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(exposure, c->dExposure, sizeof(float), hipMemcpyDeviceToHost));
    if (histogram256) HIP_TRY(c, hipMemcpy(histogram256, c->dHistogram, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HRPT_OK;
}

int hrpt_set_exposure(HrptContext* c, float exposure)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->dExposure) {
        HIP_TRY(c, hipMalloc((void**)&c->dExposure, 16));
        HIP_TRY(c, hipMalloc((void**)&c->dHistogram, 256 * sizeof(uint32_t)));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(c->dExposure, &exposure, sizeof(float), hipMemcpyHostToDevice));
    return HRPT_OK;
}

int hrpt_selftest_f16_decode(HrptContext* c, float* out65536)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out65536) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_f16_decode: null out");
    HIP_TRY(c, hipSetDevice(c->device));
    float* d = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d, 65536 * sizeof(float)));
    hipError_t e = launch_f16_table(d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out65536, d, 65536 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, HRPT_ERR_HIP, std::string("hrpt_selftest_f16_decode: ") + hipGetErrorString(e));
    return HRPT_OK;
}

int hrpt_selftest_bvh(HrptContext* c, uint64_t* violations)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!violations) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_bvh: null out");
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_selftest_bvh: no scene uploaded");
    if (c->view.instances) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_bvh: not available on the two-level structure (hrpt_set_acceleration_structure)");
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = launch_bvh_check(c->view, d, c->stream);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, HRPT_ERR_HIP, std::string("hrpt_selftest_bvh: ") + hipGetErrorString(e));
    *violations = h;
    return HRPT_OK;
}

int hrpt_selftest_read_bvh(HrptContext* c, HrptBvhDump* d)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!d) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_read_bvh: null dump");
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_selftest_read_bvh: no scene uploaded");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const SceneView& v = c->view;
    const bool twoLevel = v.instances != nullptr;
    d->structure = twoLevel ? HRPT_ACCEL_TWO_LEVEL : HRPT_ACCEL_FLAT;
    d->nodeCount = twoLevel ? 0u : v.nodeCount; d->node4Count = v.node4Count; d->triangleCount = v.triCount;
    d->instanceCount = twoLevel ? v.instanceCount : 0u; d->instanceNodeCount = twoLevel ? v.nodeCount : 0u;
    d->rootLeaf = v.rootLeaf; d->hasNodesQ = v.nodesQ ? 1u : 0u; d->hasTangents = v.tangents ? 1u : 0u;
    d->maxDepth = c->buildInfo.maxDepth; d->maxDepth4 = c->buildInfo.maxDepth4;
    d->maxDepth4Tlas = twoLevel && c->twoLevel ? c->twoLevel->maxDepth4Tlas : 0u; d->maxDepth4Blas = twoLevel && c->twoLevel ? c->twoLevel->maxDepth4Blas : 0u;
    d->sahCost = c->buildInfo.sahCost;
    d->nodes4Capacity = twoLevel ? 0u : c->nodes4Capacity; d->nodesQCapacity = v.nodesQ ? (uint32_t)c->nodesQCapacity : 0u;
    auto fetch = [&](void* dst, const void* src, size_t bytes) { return (dst && src && bytes) ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
    HIP_TRY(c, fetch(d->nodes, twoLevel ? nullptr : v.nodes, (size_t)d->nodeCount * sizeof(GpuNode)));
    HIP_TRY(c, fetch(d->nodes4, v.nodes4, (size_t)v.node4Count * sizeof(GpuNode4)));
    HIP_TRY(c, fetch(d->nodesQ, v.nodesQ, (size_t)v.node4Count * sizeof(GpuNodeQ)));
    HIP_TRY(c, fetch(d->triangles, v.tris, (size_t)v.triCount * sizeof(GpuTri)));
    HIP_TRY(c, fetch(d->attributes, v.attrs, (size_t)v.triCount * sizeof(GpuTriAttr)));
    HIP_TRY(c, fetch(d->tangents, v.tangents, (size_t)v.triCount * sizeof(GpuTriTangent)));
    HIP_TRY(c, fetch(d->instances, v.instances, (size_t)d->instanceCount * sizeof(GpuInstance)));
    return HRPT_OK;
}

int hrpt_selftest_host_build(const HrptSceneDesc* scene, uint32_t structure, uint32_t flags, HrptBvhDump* d)
{
    if (!scene || !d) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_host_build: null argument");
    if ((structure != HRPT_ACCEL_FLAT && structure != HRPT_ACCEL_TWO_LEVEL) || (flags & ~HRPT_HOST_BUILD_SEPARATE_COLLAPSE) ||
        (flags && structure != HRPT_ACCEL_FLAT)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_host_build: structure / flags");
    std::string berr;
    auto put = [](void* dst, const void* src, size_t bytes) { if (dst && bytes) memcpy(dst, src, bytes); };
    d->structure = structure; d->hasNodesQ = 0; d->nodes4Capacity = 0; d->nodesQCapacity = 0;
    if (structure == HRPT_ACCEL_FLAT) {
        BuiltBvh b;
        if (!build_scene_bvh(*scene, b, berr)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
        if ((flags & HRPT_HOST_BUILD_SEPARATE_COLLAPSE) && !b.nodes.empty()) collapse_bvh2_on_host(b.nodes, b.nodes4, b.maxDepth4);
        d->nodeCount = (uint32_t)b.nodes.size(); d->node4Count = (uint32_t)b.nodes4.size(); d->triangleCount = (uint32_t)b.tris.size();
        d->instanceCount = 0; d->instanceNodeCount = 0; d->rootLeaf = b.rootLeaf; d->hasTangents = b.tangents.empty() ? 0u : 1u;
        d->maxDepth = b.maxDepth; d->maxDepth4 = b.maxDepth4; d->maxDepth4Tlas = 0; d->maxDepth4Blas = 0; d->sahCost = b.sahCost;
        put(d->nodes, b.nodes.data(), b.nodes.size() * sizeof(HostNode)); put(d->nodes4, b.nodes4.data(), b.nodes4.size() * sizeof(HostNode4));
        put(d->triangles, b.tris.data(), b.tris.size() * sizeof(HostTri)); put(d->attributes, b.attrs.data(), b.attrs.size() * sizeof(HostTriAttr));
        put(d->tangents, b.tangents.data(), b.tangents.size() * sizeof(HostTriTangent));
        return HRPT_OK;
    }
    BuiltTwoLevel b;
    if (!build_scene_two_level(*scene, b, berr)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "acceleration structure: " + berr);
    d->nodeCount = 0; d->node4Count = (uint32_t)b.nodes4.size(); d->triangleCount = (uint32_t)b.tris.size();
    d->instanceCount = (uint32_t)b.instances.size(); d->instanceNodeCount = b.tlasNodeCount; d->rootLeaf = b.tlasRootLeaf; d->hasTangents = b.tangents.empty() ? 0u : 1u;
    d->maxDepth = 0; d->maxDepth4 = b.maxDepth4Tlas + b.maxDepth4Blas; d->maxDepth4Tlas = b.maxDepth4Tlas; d->maxDepth4Blas = b.maxDepth4Blas; d->sahCost = 0.0f;
    put(d->nodes4, b.nodes4.data(), b.nodes4.size() * sizeof(HostNode4));
    put(d->triangles, b.tris.data(), b.tris.size() * sizeof(HostTri)); put(d->attributes, b.attrs.data(), b.attrs.size() * sizeof(HostTriAttr));
    put(d->tangents, b.tangents.data(), b.tangents.size() * sizeof(HostTriTangent)); put(d->instances, b.instances.data(), b.instances.size() * sizeof(HostInstance));
    return HRPT_OK;
}

int hrpt_selftest_unorm8(HrptContext* c, float* out512)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out512) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_unorm8: null out");
    HIP_TRY(c, hipSetDevice(c->device));
    float* d = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d, 512 * sizeof(float)));
    hipError_t e = launch_unorm8_table(d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out512, d, 512 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, HRPT_ERR_HIP, std::string("hrpt_selftest_unorm8: ") + hipGetErrorString(e));
    return HRPT_OK;
}

int hrpt_selftest_sample_textures(HrptContext* c, const HrptTextureProbe* probes, HrptTextureProbeResult* results, uint64_t count)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_selftest_sample_textures: no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!probes || !results) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_sample_textures: null array");
    if (count > (1ull << 24)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_sample_textures: too many probes in one call");
    const uint32_t materialCount = (uint32_t)c->keptMaterials.size();
    for (uint64_t i = 0; i < count; ++i)
        if (probes[i].material >= materialCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_selftest_sample_textures: material index out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    HrptTextureProbe* dProbes = nullptr; HrptTextureProbeResult* dResults = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dProbes), count * sizeof(HrptTextureProbe));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dResults), count * sizeof(HrptTextureProbeResult));
    if (e == hipSuccess) e = hipMemcpyAsync(dProbes, probes, count * sizeof(HrptTextureProbe), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_sample_textures(c->view, materialCount, dProbes, dResults, (uint32_t)count, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(results, dResults, count * sizeof(HrptTextureProbeResult), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (dProbes) (void)hipFree(dProbes);
    if (dResults) (void)hipFree(dResults);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? HRPT_ERR_OUT_OF_MEMORY : HRPT_ERR_HIP, std::string("hrpt_selftest_sample_textures: ") + hipGetErrorString(e));
    return HRPT_OK;
}

int hrpt_reset_stats(HrptContext* c)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemsetAsync(c->dCounters, 0, sizeof(DeviceCounters) * kCounterShards, c->stream));
    wavefront_reset_timing(c->wf);
    c->megakernelFallbacks = 0;
    return HRPT_OK;
}

} // extern "C"

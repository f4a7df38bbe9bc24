// pt_capi.cpp -- implementation of the C ABI declared in include/hobbyrt_pt.h. Host code only. This file holds the context itself: create /
// destroy, errors, resize, stream, setters, statistics, image read / write. Its neighbours, by subject: pt_capi_scene.cpp (upload, acceleration
// structure, updates of lights / materials / instances), pt_capi_geometry.cpp (deform, skin, animate), pt_capi_render.cpp (render, G-buffer,
// motion, rays, resolves), pt_capi_post.cpp (screen-space stages), pt_capi_selftest.cpp. pt_capi_internal.h is what they share.
#include <mutex>

#include "pt_capi_internal.h"

using namespace hrt;
using namespace hrt::capi;

static std::mutex g_errMutex;
static std::string g_createError;

int capi::fail(HrptContext* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    else { std::lock_guard<std::mutex> l(g_errMutex); g_createError = msg; }
    return code;
}

int capi::realloc_image(HrptContext* c, DeviceBuffer<float4>& image, size_t bytes)
{
    HIP_TRY(c, image.alloc(bytes));
    HIP_TRY(c, hipMemsetAsync(image, 0, bytes, c->stream));
    return HRPT_OK;
}

int capi::planes_requested(HrptContext* c, const char* what, uint32_t gbMask, bool motion)
{
    static const char* const kNames[HRPT_GB_PLANES] = { "ALBEDO", "NORMAL", "GEO_NORMAL", "EMISSIVE", "DEPTH", "IDS" };
    uint32_t first = HRPT_GB_PLANES;             // the first G-buffer plane of the mask that is missing
    for (uint32_t k = HRPT_GB_PLANES; k-- > 0;)
        if ((gbMask & (1u << k)) && !c->perSize.dGBuffer[k]) first = k;
    const bool noMotion = motion && !c->perSize.dMotion;
    if (!noMotion && first == HRPT_GB_PLANES) return HRPT_OK;        // the text is built for a failure only
    std::string mask;
    for (uint32_t k = 0; k < HRPT_GB_PLANES; ++k)
        if (gbMask & (1u << k)) mask += std::string(mask.empty() ? "" : " | ") + kNames[k];
    return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": " + (noMotion ? std::string("the motion plane") : std::string("the plane HRPT_GB_") + kNames[first]) +
                                              " was never requested (" + (motion ? "" : "hrpt_render_gbuffer or ") + "hrpt_render_motion_vectors with planeMask = " + mask + " fills them)");
}

int hrpt_create(const HrptDeviceDesc* desc, HrptContext** out)
try {
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
        c->perContext.dCounters.alloc(sizeof(DeviceCounters) * kCounterShards) != hipSuccess ||
        hipMemset(c->perContext.dCounters, 0, sizeof(DeviceCounters) * kCounterShards) != hipSuccess) {
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
    if (const char* e = getenv("HRPT_RADIANCE_BATCH")) c->wf.knobs.radianceBatch = (uint32_t)atoi(e);
    if (const char* e = getenv("HRPT_BLOOM_FUSED_TAIL")) { const int v = atoi(e); c->bloomTailTexels = v == 1 ? 8192u : (v > 0 ? (uint32_t)v : 0u); }
    if (const char* e = getenv("HRPT_UPSCALE_STAGED")) c->upscaleStaged = atoi(e) != 0;
    if (const char* e = getenv("HRPT_RESTIR_GLOBAL_LIGHTS")) c->restirGlobalLights = atoi(e) != 0;
    if (const char* e = getenv("HRPT_DEFERRED_LIGHT_BATCH")) { const int v = atoi(e); c->deferredLightBatch = (v >= 1 && v <= 16) ? (uint32_t)v : 0u; }
    *out = c;
    return HRPT_OK;
} catch (...) { return caught(nullptr, "hrpt_create"); }

void hrpt_destroy(HrptContext* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_scene(c);
    c->animations.clear();
    wavefront_release(c->wf);
    c->perSize = PerSizeImages{}; c->perContext = PerContextBuffers{};      // every buffer goes before the events and the stream do
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

int hrpt_resize(HrptContext* c, uint32_t width, uint32_t height)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!size_ok(width, height))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_resize: size must be 1..65535 (RNG seed packs y*65536+x, RNG.hlsli:24)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PerSizeImages& ps = c->perSize;
    ps.dAccum.reset(); ps.dOutput.reset(); ps.stage = StageImages{};      // Accumulation, Output, Display and whatever else a stage allocated go before anything is allocated
    const size_t bytes = (size_t)width * height * sizeof(float4);
    HRPT_TRY(realloc_image(c, ps.dAccum, bytes));
    HRPT_TRY(realloc_image(c, ps.dOutput, bytes));
    for (DeviceBuffer<float4>& plane : ps.dGBuffer)         // the G-buffer planes a caller has asked for follow the image size (zeroed, like a first request)
        if (plane) HRPT_TRY(realloc_image(c, plane, bytes));
    if (ps.dMotion) HRPT_TRY(realloc_image(c, ps.dMotion, bytes));       // ... and so does the motion plane
    ps.temporalValid = false; ps.temporalCur = 0;     // the temporal history does not survive a resize
    for (DeviceBuffer<float4>& image : ps.dTemporal)
        if (image) HRPT_TRY(realloc_image(c, image, bytes));
    c->width = width; c->height = height;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_resize"); }

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

int hrpt_set_stream(HrptContext* c, void* hipStream, int useCallerStream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = useCallerStream ? static_cast<hipStream_t>(hipStream) : c->ownStream;   // a NULL caller stream is the legacy default stream
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_set_stream"); }

int hrpt_synchronize(HrptContext* c)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_synchronize"); }

int hrpt_get_device_images(HrptContext* c, void** accumulation, void** output)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_device_images: hrpt_resize not called");
    if (accumulation) *accumulation = c->perSize.dAccum;
    if (output) *output = c->perSize.dOutput;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_device_images"); }

int capi::read_image(HrptContext* c, const float4* src, float* dst, size_t bytes, const char* what)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!dst || !src || bytes != (size_t)c->width * c->height * 16) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": bad buffer size");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, what); }
int hrpt_read_accumulation(HrptContext* c, float* rgba, size_t bytes) { return read_image(c, c ? c->perSize.dAccum : nullptr, rgba, bytes, "hrpt_read_accumulation"); }
int hrpt_read_output(HrptContext* c, float* rgba, size_t bytes) { return read_image(c, c ? c->perSize.dOutput : nullptr, rgba, bytes, "hrpt_read_output"); }
int hrpt_read_display(HrptContext* c, float* rgba, size_t bytes) { return read_image(c, c ? c->perSize.stage.dDisplay : nullptr, rgba, bytes, "hrpt_read_display"); }

int hrpt_write_accumulation(HrptContext* c, const float* rgba, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!rgba || !c->perSize.dAccum || bytes != (size_t)c->width * c->height * 16) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_write_accumulation: bad buffer size");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(c->perSize.dAccum, rgba, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_write_accumulation"); }

int hrpt_clear_accumulation(HrptContext* c)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.dAccum) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_clear_accumulation: hrpt_resize not called");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->perSize.dAccum, 0, (size_t)c->width * c->height * sizeof(float4), c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_clear_accumulation"); }

int hrpt_set_shadow_overlap(HrptContext* c, int enabled)
{
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    c->wf.knobs.serialShadow = enabled == 0;
    return HRPT_OK;
}

int hrpt_set_acceleration_structure(HrptContext* c, int structure)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (structure < HRPT_ACCEL_AUTO || structure > HRPT_ACCEL_TWO_LEVEL) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_set_acceleration_structure: unknown structure");
    c->accelStructure = structure;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_set_acceleration_structure"); }

int hrpt_set_bvh_builder(HrptContext* c, int builder)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (builder != HRPT_BVH_BUILDER_HOST_SAH && builder != HRPT_BVH_BUILDER_GPU_LBVH && builder != HRPT_BVH_BUILDER_GPU_PLOC && builder != HRPT_BVH_BUILDER_AUTO) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_set_bvh_builder: unknown builder");
    c->bvhBuilder = builder;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_set_bvh_builder"); }

int hrpt_get_build_info(HrptContext* c, HrptBuildInfo* out)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_build_info: null out");
    if (!c->haveScene) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_build_info: no scene uploaded");
    *out = c->buildInfo;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_build_info"); }

int hrpt_get_stats(HrptContext* c, HrptStats* out)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_stats: null out");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    DeviceCounters h[kCounterShards];
    HIP_TRY(c, hipMemcpy(h, c->perContext.dCounters, sizeof h, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    DeviceCounters total{};
    for (int i = 0; i < kCounterShards; ++i) {
        total.closestRays += h[i].closestRays; total.shadowRays += h[i].shadowRays; total.paths += h[i].paths; total.neeEntries += h[i].neeEntries;
        total.neeSamples += h[i].neeSamples; total.radianceShade += h[i].radianceShade; total.radianceShadow += h[i].radianceShadow; total.skipped16 += h[i].skipped16;
        total.fusedPaths += h[i].fusedPaths; total.fusedEntries += h[i].fusedEntries;
    }
    out->closestRays = total.closestRays; out->shadowRays = total.shadowRays; out->paths = total.paths;
    out->neeEntries = total.neeEntries; out->neeSamples = total.neeSamples;
    out->megakernelFallbacks = c->megakernelFallbacks; out->queuePoolBytes = c->wf.pool.bytes();
    if (total.neeEntries || c->wf.raygenBytes || c->wf.resolveBytes) {     // the wavefront pipeline ran since the last reset
        wavefront_queue_bytes(c->wf, total, out->traceQueueBytes, out->shadeQueueBytes, out->shadowQueueBytes);
        out->raygenQueueBytes = c->wf.raygenBytes; out->resolveQueueBytes = c->wf.resolveBytes;
    }
    if (c->timed) { float ms = 0.0f; if (hipEventElapsedTime(&ms, c->evStart, c->evStop) == hipSuccess) out->lastRenderMs = ms; }
    wavefront_collect_timing(c->wf);
    out->traceKernelMs = c->wf.kernelMs[kKernelExtend]; out->traceKernelLaunches = c->wf.kernelLaunches[kKernelExtend];
    out->shadeKernelMs = c->wf.kernelMs[kKernelShade]; out->shadeKernelLaunches = c->wf.kernelLaunches[kKernelShade];
    out->shadowKernelMs = c->wf.kernelMs[kKernelShadow]; out->shadowKernelLaunches = c->wf.kernelLaunches[kKernelShadow];
    out->raygenKernelMs = c->wf.kernelMs[kKernelRaygen]; out->raygenKernelLaunches = c->wf.kernelLaunches[kKernelRaygen];
    out->resolveKernelMs = c->wf.kernelMs[kKernelResolve]; out->resolveKernelLaunches = c->wf.kernelLaunches[kKernelResolve];
    out->bvhNodeCount = c->bvhNodes; out->bvhTriangleCount = c->bvhTris; out->bvhMaxDepth = c->traits.bvhMaxDepth;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_stats"); }

int hrpt_reset_stats(HrptContext* c)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemsetAsync(c->perContext.dCounters, 0, sizeof(DeviceCounters) * kCounterShards, c->stream));
    wavefront_reset_timing(c->wf);
    c->megakernelFallbacks = 0;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_reset_stats"); }

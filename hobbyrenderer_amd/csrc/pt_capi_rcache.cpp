// pt_capi_rcache.cpp -- the hash-grid radiance cache (pt_rcache.h / pt_rcache.hip / pt_rcache_host.cpp): the HrptRcache object with its
// table and the buffers of one update, the two frame calls, the read-backs, the surface query and the table stages alone (_host, _device).
// The frame calls are compositions: launch_rcache_update_rays / launch_indirect_rays, launch_surface_rays, the public hrpt_trace_radiance
// (HRPT_RADIANCE_SECONDARY), the table kernels and launch_indirect_resolve.
#include <cmath>

#include "pt_capi_internal.h"
#include "pt_indirect.h"
#include "pt_rcache.h"

using namespace hrt;
using namespace hrt::capi;

// The table, the drop counter and the records of one update (one per sparse block, grown on demand).
struct HrptRcache {
    HrptContext* ctx = nullptr;
    int device = 0;                          // the context's, kept so that destruction does not read the context
    HrptRcacheDesc desc{};
    DeviceBuffer<uint64_t> dKeys, dDrops;
    DeviceBuffer<HrptRcacheAccum> dAccum;
    DeviceBuffer<HrptRcacheEntry> dResolved;
    DeviceBuffer<HrptRay> dRays;
    DeviceBuffer<float4> dRadiance;
    DeviceBuffer<HrptRcacheSurface> dSurfaces;
    DeviceBuffer<HrptRcacheSample> dSamples;
    uint64_t entries() const { return rcache::capacity(desc); }
};

static const char* const kDescRule = ": capacityLog2 10..26, sceneScale and radianceScale finite and > 0, levelBias in [-64, 64], maxSamples 1..65535, "
                                     "staleFramesMax <= 65534, sparseBlock 1..16, roughnessThreshold finite";

static int desc_check(HrptContext* c, const char* what, const HrptRcacheDesc* desc)
{
    if (!desc) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null desc");
    if (!rcache_desc_valid(*desc)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + kDescRule);
    return HRPT_OK;
}
static int camera_check(HrptContext* c, const char* what, const float* cam)
{
    if (!cam) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null cameraPos");
    if (!rcache::finite3(cam)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": the camera position is not finite");
    return HRPT_OK;
}
// What the surface query and hrpt_trace_radiance would refuse, asked before anything is written.
static int frame_check(HrptContext* c, const char* what, const HrptPathTracerConstants* constants)
{
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, std::string(what) + ": no scene uploaded");
    if (!constants) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (constants->m_MaxBounces > 64u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": m_MaxBounces above 64");
    if (constants->m_LightCount > c->view.lightCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": m_LightCount exceeds the scene's light buffer");
    if (c->view.instances && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": this two-level structure is deeper than the thread-per-ray kernel's 64-entry stack");
    HRPT_TRY(camera_check(c, what, constants->m_CameraPos));
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": hrpt_resize not called");
    return planes_requested(c, what, 1u << HRPT_GB_ALBEDO | 1u << HRPT_GB_NORMAL | 1u << HRPT_GB_GEO_NORMAL | 1u << HRPT_GB_DEPTH, false);
}
static HrptIndirectImages gbuffer_images(HrptContext* c)
{
    PerSizeImages& ps = c->perSize;
    HrptIndirectImages im = {};
    im.albedo = floats(ps.dGBuffer[HRPT_GB_ALBEDO]); im.normal = floats(ps.dGBuffer[HRPT_GB_NORMAL]); im.geoNormal = floats(ps.dGBuffer[HRPT_GB_GEO_NORMAL]);
    im.depth = floats(ps.dGBuffer[HRPT_GB_DEPTH]);
    return im;
}
static indirect::Frame diffuse_frame(HrptContext* c, const HrptPathTracerConstants& cb, uint32_t frameSeed)
{
    HrptIndirectParams p = {};
    p.flags = HRPT_INDIRECT_DIFFUSE; p.frameSeed = frameSeed;
    return indirect::make_frame(cb, p, (int)c->width, (int)c->height);
}

int hrpt_rcache_create(HrptContext* c, const HrptRcacheDesc* desc, HrptRcache** out)
try {
    if (out) *out = nullptr;
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!out) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_rcache_create: null argument");
    HRPT_TRY(desc_check(c, "hrpt_rcache_create", desc));
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<HrptRcache> p(new HrptRcache);
    p->ctx = c; p->device = c->device; p->desc = *desc;
    const uint64_t n = p->entries();
    HIP_TRY(c, p->dKeys.alloc(n * sizeof(uint64_t)));
    HIP_TRY(c, p->dAccum.alloc(n * sizeof(HrptRcacheAccum)));
    HIP_TRY(c, p->dResolved.alloc(n * sizeof(HrptRcacheEntry)));
    HIP_TRY(c, p->dDrops.alloc(16));
    HIP_TRY(c, launch_rcache_clear(p->desc, p->dKeys, p->dAccum, p->dResolved, p->dDrops, c->stream));
    *out = p.release();
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_rcache_create"); }

void hrpt_rcache_destroy(HrptRcache* p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;                                // hipFree waits for work in flight
}

int hrpt_rcache_clear(HrptRcache* p)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_rcache_clear(p->desc, p->dKeys, p->dAccum, p->dResolved, p->dDrops, c->stream));
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_rcache_clear"); }

int hrpt_rcache_update(HrptRcache* p, const HrptPathTracerConstants* constants, uint32_t frameIndex, uint32_t flags)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    const char* what = "hrpt_rcache_update";
    if (flags & ~rcache::kUpdateFlags) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown flags");
    HRPT_TRY(frame_check(c, what, constants));
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t B = p->desc.sparseBlock;
    const uint64_t n = (uint64_t)((c->width + B - 1u) / B) * ((c->height + B - 1u) / B);
    HIP_TRY(c, p->dRays.reserve(n * sizeof(HrptRay)));
    HIP_TRY(c, p->dRadiance.reserve(n * sizeof(float4)));
    HIP_TRY(c, p->dSurfaces.reserve(n * sizeof(HrptRcacheSurface)));
    HIP_TRY(c, p->dSamples.reserve(n * sizeof(HrptRcacheSample)));
    const HrptIndirectImages im = gbuffer_images(c);
    // So far only the cache's own record buffers were written: a failed argument check of the trace leaves the table as it was.
    HIP_TRY(c, launch_rcache_update_rays(diffuse_frame(c, *constants, frameIndex), p->desc, frameIndex, im.normal, im.geoNormal, im.depth, p->dRays, c->stream));
    HRPT_TRY(hrpt_rcache_surfaces_device(c, p->dRays, p->dSurfaces, n, c->stream));
    HRPT_TRY(hrpt_trace_radiance(c, p->dRays, reinterpret_cast<float*>(p->dRadiance.get()), n, constants, HRPT_RADIANCE_DEVICE_POINTERS | HRPT_RADIANCE_SECONDARY));
    if (flags & HRPT_RCACHE_RESET) HIP_TRY(c, launch_rcache_clear(p->desc, p->dKeys, p->dAccum, p->dResolved, p->dDrops, c->stream));
    HIP_TRY(c, launch_rcache_gather_samples(p->dSurfaces, p->dRadiance, p->dSamples, n, c->stream));
    HIP_TRY(c, launch_rcache_insert(p->desc, constants->m_CameraPos, p->dKeys, p->dAccum, p->dDrops, p->dSamples, n, !(flags & HRPT_RCACHE_NO_WAVE_COMBINE), c->stream));
    HIP_TRY(c, launch_rcache_resolve(p->desc, p->dKeys, p->dAccum, p->dResolved, c->stream));
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_rcache_update"); }

int hrpt_rcache_indirect(HrptRcache* p, const HrptPathTracerConstants* constants, const HrptRcacheParams* params)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    const char* what = "hrpt_rcache_indirect";
    if (!params) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if ((params->flags & ~HRPT_RCACHE_NO_FALLBACK) || params->reserved[0] || params->reserved[1])
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown flag bits or non-zero reserved");
    HRPT_TRY(frame_check(c, what, constants));
    HIP_TRY(c, hipSetDevice(c->device));
    StageImages& st = c->perSize.stage;
    const size_t WH = (size_t)c->width * c->height;
    for (DeviceBuffer<float4>& image : st.dIndirect)
        if (!image) HRPT_TRY(realloc_image(c, image, WH * sizeof(float4)));
    if (!st.dRcacheServed) HRPT_TRY(realloc_image(c, st.dRcacheServed, WH * sizeof(float4)));
    HIP_TRY(c, st.dIndirectRays.reserve(WH * sizeof(HrptRay)));
    HIP_TRY(c, st.dIndirectRadiance.reserve(WH * sizeof(float4)));
    HIP_TRY(c, st.dRcacheSurfaces.reserve(WH * sizeof(HrptRcacheSurface)));
    HIP_TRY(c, st.dRcacheCached.reserve(WH * sizeof(float4)));
    HIP_TRY(c, st.dRcacheVoxel.reserve(WH * sizeof(float)));
    HrptIndirectImages im = gbuffer_images(c);
    im.diffuse = floats(st.dIndirect[0]);                  // specular stays NULL: the resolve leaves that plane alone
    const indirect::Frame f = diffuse_frame(c, *constants, params->frameSeed);
    HIP_TRY(c, launch_indirect_rays(f, im, st.dIndirectRays, c->stream));
    HRPT_TRY(hrpt_rcache_surfaces_device(c, st.dIndirectRays, st.dRcacheSurfaces, WH, c->stream));
    HIP_TRY(c, launch_rcache_query(p->desc, constants->m_CameraPos, p->dKeys, p->dResolved, st.dRcacheSurfaces.get(), (uint32_t)sizeof(HrptRcacheSurface),
                                   floats(st.dRcacheCached), st.dRcacheVoxel, WH, c->stream));
    HIP_TRY(c, launch_rcache_serve(st.dRcacheSurfaces, st.dRcacheCached, st.dRcacheVoxel, st.dRcacheServed, st.dIndirectRays, WH, c->stream));
    if (params->flags & HRPT_RCACHE_NO_FALLBACK) HIP_TRY(c, hipMemsetAsync(st.dIndirectRadiance, 0, WH * sizeof(float4), c->stream));
    else HRPT_TRY(hrpt_trace_radiance(c, st.dIndirectRays, floats(st.dIndirectRadiance), WH, constants, HRPT_RADIANCE_DEVICE_POINTERS | HRPT_RADIANCE_SECONDARY));
    HIP_TRY(c, launch_indirect_resolve(f, im, st.dIndirectRadiance, c->stream));
    HIP_TRY(c, launch_rcache_apply(st.dRcacheServed, st.dIndirect[0], WH, c->stream));
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_rcache_indirect"); }

int hrpt_read_rcache_served(HrptContext* c, float* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.stage.dRcacheServed) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_rcache_served: no served plane at the current size (hrpt_rcache_indirect writes it)");
    return read_image(c, c->perSize.stage.dRcacheServed, dst, bytes, "hrpt_read_rcache_served");
} catch (...) { return caught(c, "hrpt_read_rcache_served"); }

int hrpt_rcache_read(HrptRcache* p, uint64_t* keys, HrptRcacheAccum* accumulation, HrptRcacheEntry* resolved, uint64_t entries, uint64_t* dropsOut)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    if ((keys || accumulation || resolved) && entries != p->entries()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_rcache_read: entries must equal the capacity");
    HIP_TRY(c, hipSetDevice(c->device));
    if (keys) HIP_TRY(c, hipMemcpyAsync(keys, p->dKeys, entries * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (accumulation) HIP_TRY(c, hipMemcpyAsync(accumulation, p->dAccum, entries * sizeof(HrptRcacheAccum), hipMemcpyDeviceToHost, c->stream));
    if (resolved) HIP_TRY(c, hipMemcpyAsync(resolved, p->dResolved, entries * sizeof(HrptRcacheEntry), hipMemcpyDeviceToHost, c->stream));
    if (dropsOut) HIP_TRY(c, hipMemcpyAsync(dropsOut, p->dDrops, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_rcache_read"); }

int hrpt_rcache_write(HrptRcache* p, const uint64_t* keys, const HrptRcacheAccum* accumulation, const HrptRcacheEntry* resolved, uint64_t entries)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    if (!keys || !accumulation || !resolved) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_rcache_write: null array");
    if (entries != p->entries()) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_rcache_write: entries must equal the capacity");
    if (const char* fault = rcache_table_fault(p->desc, keys, accumulation, resolved)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_rcache_write: ") + fault);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(p->dKeys, keys, entries * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(p->dAccum, accumulation, entries * sizeof(HrptRcacheAccum), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(p->dResolved, resolved, entries * sizeof(HrptRcacheEntry), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_rcache_write"); }

int hrpt_rcache_get_device(HrptRcache* p, void** keys, void** accumulation, void** resolved, void** drops)
{
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    if (keys) *keys = p->dKeys;
    if (accumulation) *accumulation = p->dAccum;
    if (resolved) *resolved = p->dResolved;
    if (drops) *drops = p->dDrops;
    return HRPT_OK;
}

int hrpt_rcache_surfaces_device(HrptContext* c, const HrptRay* rays, HrptRcacheSurface* surfacesOut, uint64_t count, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_rcache_surfaces_device";
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, std::string(what) + ": no scene uploaded");
    if (count == 0) return HRPT_OK;
    if (!rays || !surfacesOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
    if (count > (1ull << 31)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": too many rays in one call");
    if (c->view.instances && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": this two-level structure is deeper than the thread-per-ray kernel's 64-entry stack");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_surface_rays(c->view, rays, surfacesOut, count, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_rcache_surfaces_device"); }

// ---- the table stages alone ----
static int insert_check(HrptContext* c, const char* what, const HrptRcacheDesc* desc, const float* cam, const void* keys, const void* accum, const void* drops,
                        const void* samples, uint64_t count)
{
    HRPT_TRY(desc_check(c, what, desc));
    HRPT_TRY(camera_check(c, what, cam));
    if (!keys || !accum || !drops || (count && !samples)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
    if (count > (1ull << 31)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": too many samples in one call");
    return HRPT_OK;
}
static int resolve_check(HrptContext* c, const char* what, const HrptRcacheDesc* desc, const void* keys, const void* accum, const void* resolved, uint32_t flags)
{
    HRPT_TRY(desc_check(c, what, desc));
    if (!keys || !accum || !resolved) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
    if (flags & ~HRPT_RCACHE_RESET) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown flags");
    return HRPT_OK;
}
static int query_check(HrptContext* c, const char* what, const HrptRcacheDesc* desc, const float* cam, const void* keys, const void* resolved, const void* points,
                       const void* out4, uint64_t count)
{
    HRPT_TRY(desc_check(c, what, desc));
    HRPT_TRY(camera_check(c, what, cam));
    if (!keys || !resolved || (count && (!points || !out4))) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
    if (count > (1ull << 31)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": too many points in one call");
    return HRPT_OK;
}

int hrpt_rcache_insert_host(const HrptRcacheDesc* desc, const float* cameraPos, uint64_t* keys, HrptRcacheAccum* accumulation, uint64_t* drops,
                            const HrptRcacheSample* samples, uint64_t count, int nthreads)
{
    HRPT_TRY(insert_check(nullptr, "hrpt_rcache_insert_host", desc, cameraPos, keys, accumulation, drops, samples, count));
    return run_host("hrpt_rcache_insert_host", [&] { rcache_insert_host(*desc, cameraPos, keys, accumulation, drops, samples, count, host_threads(nthreads)); });
}

int hrpt_rcache_insert_device(HrptContext* c, const HrptRcacheDesc* desc, const float* cameraPos, uint64_t* keys, HrptRcacheAccum* accumulation, uint64_t* drops,
                              const HrptRcacheSample* samples, uint64_t count, uint32_t flags, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(insert_check(c, "hrpt_rcache_insert_device", desc, cameraPos, keys, accumulation, drops, samples, count));
    if (flags & ~HRPT_RCACHE_NO_WAVE_COMBINE) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_rcache_insert_device: unknown flags");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_rcache_insert(*desc, cameraPos, keys, accumulation, drops, samples, count, !(flags & HRPT_RCACHE_NO_WAVE_COMBINE), static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_rcache_insert_device"); }

int hrpt_rcache_resolve_host(const HrptRcacheDesc* desc, uint64_t* keys, HrptRcacheAccum* accumulation, HrptRcacheEntry* resolved, uint32_t flags, int nthreads)
{
    HRPT_TRY(resolve_check(nullptr, "hrpt_rcache_resolve_host", desc, keys, accumulation, resolved, flags));
    if (flags & HRPT_RCACHE_RESET) {
        const uint64_t n = rcache::capacity(*desc);
        std::memset(keys, 0, n * sizeof(uint64_t)); std::memset(accumulation, 0, n * sizeof(HrptRcacheAccum)); std::memset(resolved, 0, n * sizeof(HrptRcacheEntry));
        return HRPT_OK;
    }
    return run_host("hrpt_rcache_resolve_host", [&] { rcache_resolve_host(*desc, keys, accumulation, resolved, host_threads(nthreads)); });
}

int hrpt_rcache_resolve_device(HrptContext* c, const HrptRcacheDesc* desc, uint64_t* keys, HrptRcacheAccum* accumulation, HrptRcacheEntry* resolved, uint32_t flags,
                               void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(resolve_check(c, "hrpt_rcache_resolve_device", desc, keys, accumulation, resolved, flags));
    HIP_TRY(c, hipSetDevice(c->device));
    if (flags & HRPT_RCACHE_RESET) HIP_TRY(c, launch_rcache_clear(*desc, keys, accumulation, resolved, nullptr, static_cast<hipStream_t>(stream)));
    else HIP_TRY(c, launch_rcache_resolve(*desc, keys, accumulation, resolved, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_rcache_resolve_device"); }

int hrpt_rcache_query_host(const HrptRcacheDesc* desc, const float* cameraPos, const uint64_t* keys, const HrptRcacheEntry* resolved, const HrptRcachePoint* points,
                           float* out4, float* voxelOut, uint64_t count, int nthreads)
{
    HRPT_TRY(query_check(nullptr, "hrpt_rcache_query_host", desc, cameraPos, keys, resolved, points, out4, count));
    return run_host("hrpt_rcache_query_host", [&] { rcache_query_host(*desc, cameraPos, keys, resolved, points, out4, voxelOut, count, host_threads(nthreads)); });
}

int hrpt_rcache_query_device(HrptContext* c, const HrptRcacheDesc* desc, const float* cameraPos, const uint64_t* keys, const HrptRcacheEntry* resolved,
                             const HrptRcachePoint* points, float* out4, float* voxelOut, uint64_t count, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(query_check(c, "hrpt_rcache_query_device", desc, cameraPos, keys, resolved, points, out4, count));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_rcache_query(*desc, cameraPos, keys, resolved, points, (uint32_t)sizeof(HrptRcachePoint), out4, voxelOut, count, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_rcache_query_device"); }

// pt_capi_probes.cpp -- the irradiance probe volume (pt_probes.h / pt_probes.hip / pt_probes_host.cpp): the HrptProbes object with its
// atlases and ray buffers, update, query at points and at the G-buffer, the read-backs, and the stages alone (_host, _device).
#include <cmath>

#include "pt_capi_internal.h"

using namespace hrt;
using namespace hrt::capi;

// The atlases and the buffers of one update: P * N ray records, radiance and hits, N shared directions; all sized at creation.
struct HrptProbes {
    HrptContext* ctx = nullptr;
    int device = 0;                          // the context's, kept so that destruction does not read the context
    HrptProbeVolume volume{};
    uint32_t probeCount = 0;
    bool hasHistory = false;                 // an update since creation / a write: the next update blends with hysteresis
    DeviceBuffer<float> dIrradiance, dDistance, dDirections, dRadiance;
    DeviceBuffer<HrptRay> dRays;
    DeviceBuffer<HrptRayHit> dHits;
    size_t irradianceBytes() const { return (size_t)probeCount * 256 * sizeof(float); }
    size_t distanceBytes() const { return (size_t)probeCount * 512 * sizeof(float); }
};

static const char* const kVolumeRule = ": counts >= 1 with at most 2^20 probes, raysPerProbe 1..1024, spacing and maxRayDistance finite and > 0, hysteresis in [0, 1), "
                                       "distanceExponent finite and >= 1, normalBias and viewBias finite and >= 0, pad 0";

int hrpt_probes_create(HrptContext* c, const HrptProbeVolume* volume, HrptProbes** out)
try {
    if (out) *out = nullptr;
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!volume || !out) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_create: null argument");
    if (!probes_volume_valid(*volume)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string("hrpt_probes_create") + kVolumeRule);
    HIP_TRY(c, hipSetDevice(c->device));
    std::unique_ptr<HrptProbes> p(new HrptProbes);
    p->ctx = c; p->device = c->device; p->volume = *volume;
    p->probeCount = volume->counts[0] * volume->counts[1] * volume->counts[2];
    const size_t rays = (size_t)p->probeCount * volume->raysPerProbe;
    HIP_TRY(c, p->dIrradiance.alloc(p->irradianceBytes()));
    HIP_TRY(c, p->dDistance.alloc(p->distanceBytes()));
    HIP_TRY(c, p->dDirections.alloc((size_t)volume->raysPerProbe * 16));
    HIP_TRY(c, p->dRadiance.alloc(rays * 16));
    HIP_TRY(c, p->dRays.alloc(rays * sizeof(HrptRay)));
    HIP_TRY(c, p->dHits.alloc(rays * sizeof(HrptRayHit)));
    HIP_TRY(c, hipMemsetAsync(p->dIrradiance, 0, p->irradianceBytes(), c->stream));
    HIP_TRY(c, hipMemsetAsync(p->dDistance, 0, p->distanceBytes(), c->stream));
    *out = p.release();
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_probes_create"); }

void hrpt_probes_destroy(HrptProbes* p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;                                // hipFree waits for work in flight
}

int hrpt_probes_update(HrptProbes* p, const HrptPathTracerConstants* constants, uint32_t frameSeed, uint32_t flags)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, "hrpt_probes_update: no scene uploaded");
    if (!constants) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_update: null constants");
    if (flags & ~HRPT_PROBES_RESET) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_update: unknown flags");
    HIP_TRY(c, hipSetDevice(c->device));
    // The records, then the two public trace calls on them: a failed argument check of either leaves the atlases as they were (so far only
    // the volume's own ray buffers were written).
    const uint64_t rays = (uint64_t)p->probeCount * p->volume.raysPerProbe;
    HIP_TRY(c, launch_probes_raygen(p->volume, frameSeed, p->dRays, p->dDirections, c->stream));
    HRPT_TRY(hrpt_trace_radiance(c, p->dRays, p->dRadiance, rays, constants, HRPT_RADIANCE_DEVICE_POINTERS));
    HRPT_TRY(hrpt_trace_rays(c, p->dRays, p->dHits, rays, HRPT_RAYS_CLOSEST | HRPT_RAYS_DEVICE_POINTERS));
    const bool useHistory = p->hasHistory && (flags & HRPT_PROBES_RESET) == 0;
    HIP_TRY(c, launch_probes_blend(p->volume, p->dDirections, p->dRadiance, p->dHits, p->dIrradiance, p->dDistance, useHistory, c->stream));
    p->hasHistory = true;
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_probes_update"); }

int hrpt_probes_query(HrptProbes* p, const HrptProbePoint* points, float* irradiance4, uint64_t count, uint32_t flags)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    if (flags & ~HRPT_PROBES_DEVICE_POINTERS) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_query: unknown flags");
    if (count == 0) return HRPT_OK;
    if (!points || !irradiance4) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_query: null array");
    if (count > (1ull << 31)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_query: too many points in one call");
    HIP_TRY(c, hipSetDevice(c->device));
    if (flags & HRPT_PROBES_DEVICE_POINTERS) {
        HIP_TRY(c, launch_probes_query(p->volume, p->dIrradiance, p->dDistance, points, irradiance4, count, c->stream));
        return HRPT_OK;
    }
    DeviceBuffer<HrptProbePoint> dPoints; DeviceBuffer<float> dOut;
    hipError_t e = dPoints.alloc(count * sizeof(HrptProbePoint));
    if (e == hipSuccess) e = dOut.alloc(count * 16);
    if (e == hipSuccess) e = hipMemcpyAsync(dPoints, points, count * sizeof(HrptProbePoint), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_probes_query(p->volume, p->dIrradiance, p->dDistance, dPoints, dOut, count, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(irradiance4, dOut, count * 16, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, hip_status(e), std::string("hrpt_probes_query: ") + hipGetErrorString(e));
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_probes_query"); }

int hrpt_probes_shade_gbuffer(HrptProbes* p, const HrptPlanarViewConstants* view, float intensity)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    if (!view) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_shade_gbuffer: null view");
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_shade_gbuffer: hrpt_resize not called");
    HRPT_TRY(planes_requested(c, "hrpt_probes_shade_gbuffer", 1u << HRPT_GB_NORMAL | 1u << HRPT_GB_DEPTH, false));
    if (view->m_ViewportSize[0] != (float)c->width || view->m_ViewportSize[1] != (float)c->height)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_shade_gbuffer: view->m_ViewportSize does not match the image size");
    if (!(intensity >= 0.0f && intensity <= 3.402823466e38f)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_shade_gbuffer: intensity must be finite and >= 0");
    HIP_TRY(c, hipSetDevice(c->device));
    PerSizeImages& ps = c->perSize;
    if (!ps.stage.dProbeIrradiance) HRPT_TRY(realloc_image(c, ps.stage.dProbeIrradiance, (size_t)c->width * c->height * sizeof(float4)));
    HIP_TRY(c, launch_probes_shade_gbuffer(p->volume, *view, c->width, c->height, intensity, p->dIrradiance, p->dDistance, floats(ps.dGBuffer[HRPT_GB_NORMAL]),
                                           floats(ps.dGBuffer[HRPT_GB_DEPTH]), ps.stage.dProbeIrradiance, c->stream));
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_probes_shade_gbuffer"); }

int hrpt_read_probe_irradiance(HrptContext* c, float* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.stage.dProbeIrradiance) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_probe_irradiance: no probe irradiance plane at the current size (hrpt_probes_shade_gbuffer writes it)");
    return read_image(c, c->perSize.stage.dProbeIrradiance, dst, bytes, "hrpt_read_probe_irradiance");
} catch (...) { return caught(c, "hrpt_read_probe_irradiance"); }

int hrpt_get_probe_irradiance_device(HrptContext* c, void** devicePtr)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_probe_irradiance_device: null out");
    *devicePtr = c->perSize.stage.dProbeIrradiance;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_probe_irradiance_device"); }

// The byte counts of hrpt_probes_read / _write: a given pointer comes with exactly its atlas's size.
static int atlas_sizes_check(HrptProbes* p, const char* what, const void* irradiance, size_t irradianceBytes, const void* distance, size_t distanceBytes)
{
    if ((irradiance && irradianceBytes != p->irradianceBytes()) || (distance && distanceBytes != p->distanceBytes()))
        return fail(p->ctx, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": bad buffer size (irradiance: probes * 1024 bytes, distance: probes * 2048 bytes)");
    return HRPT_OK;
}

int hrpt_probes_read(HrptProbes* p, float* irradiance, size_t irradianceBytes, float* distance, size_t distanceBytes)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    HRPT_TRY(atlas_sizes_check(p, "hrpt_probes_read", irradiance, irradianceBytes, distance, distanceBytes));
    HIP_TRY(c, hipSetDevice(c->device));
    if (irradiance) HIP_TRY(c, hipMemcpyAsync(irradiance, p->dIrradiance, irradianceBytes, hipMemcpyDeviceToHost, c->stream));
    if (distance) HIP_TRY(c, hipMemcpyAsync(distance, p->dDistance, distanceBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_probes_read"); }

int hrpt_probes_write(HrptProbes* p, const float* irradiance, size_t irradianceBytes, const float* distance, size_t distanceBytes)
try {
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    HrptContext* c = p->ctx;
    HRPT_TRY(atlas_sizes_check(p, "hrpt_probes_write", irradiance, irradianceBytes, distance, distanceBytes));
    HIP_TRY(c, hipSetDevice(c->device));
    if (irradiance) HIP_TRY(c, hipMemcpyAsync(p->dIrradiance, irradiance, irradianceBytes, hipMemcpyHostToDevice, c->stream));
    if (distance) HIP_TRY(c, hipMemcpyAsync(p->dDistance, distance, distanceBytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (irradiance || distance) p->hasHistory = true;
    return HRPT_OK;
} catch (...) { return caught(p ? p->ctx : nullptr, "hrpt_probes_write"); }

int hrpt_probes_get_device(HrptProbes* p, void** irradiance, void** distance)
{
    if (!p) return HRPT_ERR_INVALID_ARGUMENT;
    if (irradiance) *irradiance = p->dIrradiance;
    if (distance) *distance = p->dDistance;
    return HRPT_OK;
}

// ---- the stages alone ----
static int volume_check(HrptContext* c, const char* what, const HrptProbeVolume* volume)
{
    if (!volume) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null volume");
    if (!probes_volume_valid(*volume)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + kVolumeRule);
    return HRPT_OK;
}
static int blend_check(HrptContext* c, const char* what, const HrptProbeVolume* volume, const float* directions4, const float* radiance4, const HrptRayHit* hits,
                       float* irradiance, float* distance, uint32_t hasHistory)
{
    HRPT_TRY(volume_check(c, what, volume));
    if (!directions4 || !radiance4 || !hits || !irradiance || !distance) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
    if (hasHistory > 1u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": hasHistory must be 0 or 1");
    return HRPT_OK;
}

int hrpt_probes_rays_host(const HrptProbeVolume* volume, uint32_t frameSeed, HrptRay* raysOut, float* directions4Out)
{
    HRPT_TRY(volume_check(nullptr, "hrpt_probes_rays_host", volume));
    return run_host("hrpt_probes_rays_host", [&] { probes_rays_host(*volume, frameSeed, raysOut, directions4Out); });
}

int hrpt_probes_blend_host(const HrptProbeVolume* volume, const float* directions4, const float* radiance4, const HrptRayHit* hits, float* irradiance,
                           float* distance, uint32_t hasHistory, int nthreads)
{
    HRPT_TRY(blend_check(nullptr, "hrpt_probes_blend_host", volume, directions4, radiance4, hits, irradiance, distance, hasHistory));
    return run_host("hrpt_probes_blend_host", [&] { probes_blend_host(*volume, directions4, radiance4, hits, irradiance, distance, hasHistory != 0u, host_threads(nthreads)); });
}

int hrpt_probes_blend_device(HrptContext* c, const HrptProbeVolume* volume, const float* directions4, const float* radiance4, const HrptRayHit* hits,
                             float* irradiance, float* distance, uint32_t hasHistory, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(blend_check(c, "hrpt_probes_blend_device", volume, directions4, radiance4, hits, irradiance, distance, hasHistory));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_probes_blend(*volume, directions4, radiance4, hits, irradiance, distance, hasHistory != 0u, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_probes_blend_device"); }

int hrpt_probes_query_host(const HrptProbeVolume* volume, const float* irradiance, const float* distance, const HrptProbePoint* points, float* out4,
                           uint64_t count, int nthreads)
{
    HRPT_TRY(volume_check(nullptr, "hrpt_probes_query_host", volume));
    if (count == 0) return HRPT_OK;
    if (!irradiance || !distance || !points || !out4) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_probes_query_host: null array");
    return run_host("hrpt_probes_query_host", [&] { probes_query_host(*volume, irradiance, distance, points, out4, count, host_threads(nthreads)); });
}

// pt_capi_deferred.cpp -- deferred lighting (pt_deferred.h / pt_deferred.hip / pt_deferred_host.cpp): the context call over the G-buffer
// planes into Output, the same over caller-owned device images, and the two host executors. The context call is the composition of
// launch_deferred_rays, the public hrpt_trace_rays and launch_deferred_shade, per batch of lights.
#include <cmath>

#include "pt_capi_internal.h"
#include "pt_deferred.h"

using namespace hrt;
using namespace hrt::capi;

static const char* const kParamsRule = ": unknown flag bits, non-zero reserved or an indirectIntensity that is not finite";

static int images_check(HrptContext* c, const char* what, const HrptDeferredImages* im, uint32_t width, uint32_t height, bool indirect)
{
    if (!im) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null images");
    if (!size_ok(width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": size must be 1..65535");
    if (!im->albedo || !im->normal || !im->geoNormal || !im->emissive || !im->depth || !im->colorOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null image");
    if (indirect && !im->indirect) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": HRPT_DEFERRED_INDIRECT without an indirect image");
    const float* inputs[6] = { im->albedo, im->normal, im->geoNormal, im->emissive, im->depth, im->indirect };
    for (const float* p : inputs)
        if (p == im->colorOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": colorOut must differ from every other image");
    return HRPT_OK;
}

// The batches of one call on `stream`, which also carries the trace calls: the context stream is redirected for their duration.
static int deferred_run(HrptContext* c, const HrptDeferredImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb,
                        const HrptDeferredParams& p, hipStream_t stream)
{
    const uint32_t n = cb.m_LightCount;
    const size_t WH = (size_t)width * height;
    uint32_t B = c->deferredLightBatch ? c->deferredLightBatch : 4u;
    if (B > n) B = n;
    if (B < 1u) B = 1u;
    while (B > 1u && WH * B > (1ull << 31)) --B;                  // one hrpt_trace_rays call takes at most 2^31 rays
    const bool shadows = (p.flags & HRPT_DEFERRED_SHADOWS) != 0u && n > 0u;
    StageImages& ps = c->perSize.stage;
    if (shadows) {
        HIP_TRY(c, ps.dDeferredRays.reserve(WH * B * sizeof(HrptRay)));
        HIP_TRY(c, ps.dDeferredHits.reserve(WH * B * sizeof(HrptRayHit)));
    }
    if (n > B)
        for (DeviceBuffer<float4>& image : ps.dDeferredCarry) HIP_TRY(c, image.reserve(WH * sizeof(float4)));
    const float sunIntensity = c->keptLights.empty() ? 0.0f : c->keptLights[0].m_Intensity;
    const deferred::Frame f = deferred::make_frame(cb, p, sunIntensity, (int)width, (int)height);
    const ScopedStream redirect(c, stream);
    uint32_t first = 0;
    do {
        const uint32_t count = n - first < B ? n - first : B;
        if (shadows) {
            HIP_TRY(c, launch_deferred_rays(f, c->view.lights, first, count, im.depth, im.normal, ps.dDeferredRays, stream));
            HRPT_TRY(hrpt_trace_rays(c, ps.dDeferredRays, ps.dDeferredHits, (uint64_t)WH * count, HRPT_RAYS_SHADOW | HRPT_RAYS_DEVICE_POINTERS));
        }
        HIP_TRY(c, launch_deferred_shade(c->view, f, c->view.lights, first, count, first == 0u, first + count >= n, im, shadows ? ps.dDeferredHits.get() : nullptr,
                                         ps.dDeferredCarry[0], ps.dDeferredCarry[1], stream));
        first += count;
    } while (first < n);
    return HRPT_OK;
}

static int common_check(HrptContext* c, const char* what, const HrptPathTracerConstants* constants, const HrptDeferredParams* params)
{
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, std::string(what) + ": no scene uploaded");
    if (!constants || !params) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (!deferred_params_valid(*params)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + kParamsRule);
    if (constants->m_LightCount > c->view.lightCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": m_LightCount exceeds the scene's light buffer");
    if ((params->flags & HRPT_DEFERRED_SHADOWS) && c->view.instances && !wavefront_trace_rays_supported(c->traits) && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": this two-level structure is deeper than the thread-per-ray kernel's 64-entry stack");
    return HRPT_OK;
}

int hrpt_deferred_lighting(HrptContext* c, const HrptPathTracerConstants* constants, const HrptDeferredParams* params)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(common_check(c, "hrpt_deferred_lighting", constants, params));
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_deferred_lighting: hrpt_resize not called");
    PerSizeImages& ps = c->perSize;
    HRPT_TRY(planes_requested(c, "hrpt_deferred_lighting", 1u << HRPT_GB_ALBEDO | 1u << HRPT_GB_NORMAL | 1u << HRPT_GB_GEO_NORMAL | 1u << HRPT_GB_EMISSIVE | 1u << HRPT_GB_DEPTH, false));
    if ((params->flags & HRPT_DEFERRED_INDIRECT) && !ps.stage.dProbeIrradiance)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_deferred_lighting: HRPT_DEFERRED_INDIRECT with no probe irradiance plane at the current size (hrpt_probes_shade_gbuffer writes it)");
    HIP_TRY(c, hipSetDevice(c->device));
    HrptDeferredImages im = {};
    im.albedo = floats(ps.dGBuffer[HRPT_GB_ALBEDO]); im.normal = floats(ps.dGBuffer[HRPT_GB_NORMAL]); im.geoNormal = floats(ps.dGBuffer[HRPT_GB_GEO_NORMAL]);
    im.emissive = floats(ps.dGBuffer[HRPT_GB_EMISSIVE]); im.depth = floats(ps.dGBuffer[HRPT_GB_DEPTH]); im.indirect = floats(ps.stage.dProbeIrradiance);
    im.colorOut = floats(ps.dOutput);
    return deferred_run(c, im, c->width, c->height, *constants, *params, c->stream);
} catch (...) { return caught(c, "hrpt_deferred_lighting"); }

int hrpt_deferred_lighting_device(HrptContext* c, const HrptDeferredImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                                  const HrptDeferredParams* params, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(common_check(c, "hrpt_deferred_lighting_device", constants, params));
    HRPT_TRY(images_check(c, "hrpt_deferred_lighting_device", images, width, height, (params->flags & HRPT_DEFERRED_INDIRECT) != 0u));
    HIP_TRY(c, hipSetDevice(c->device));
    return deferred_run(c, *images, width, height, *constants, *params, static_cast<hipStream_t>(stream));
} catch (...) { return caught(c, "hrpt_deferred_lighting_device"); }

// ---- the stages on the host ----
int hrpt_deferred_rays_host(const HrptDeferredImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptGPULight* lights,
                            uint32_t firstLight, uint32_t lightCount, HrptRay* raysOut)
{
    const char* what = "hrpt_deferred_rays_host";
    if (!images || !constants) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (!size_ok(width, height)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": size must be 1..65535");
    if (!images->depth || !images->normal) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": the depth and normal images are required");
    if (lightCount == 0) return HRPT_OK;
    if (!lights || !raysOut) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null array");
    if ((uint64_t)firstLight + lightCount > 0xFFFFFFFFull) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": light range out of range");
    return run_host(what, [&] { deferred_rays_host(*images, width, height, *constants, lights, firstLight, lightCount, raysOut); });
}

int hrpt_deferred_shade_host(const HrptDeferredImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptGPULight* lights,
                             uint32_t lightCount, const float* visibility, const float* sunRadiance, const float* sky, const HrptDeferredParams* params, int nthreads)
{
    const char* what = "hrpt_deferred_shade_host";
    if (!constants || !params) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (!deferred_params_valid(*params)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + kParamsRule);
    HRPT_TRY(images_check(nullptr, what, images, width, height, (params->flags & HRPT_DEFERRED_INDIRECT) != 0u));
    if (lightCount > 0 && !lights) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null lights");
    if ((sunRadiance && sunRadiance == images->colorOut) || (sky && sky == images->colorOut) || (visibility && visibility == images->colorOut))
        return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": colorOut must differ from every other image");
    return run_host(what, [&] { deferred_shade_host(*images, width, height, *constants, lights, lightCount, visibility, sunRadiance, sky, *params, host_threads(nthreads)); });
}

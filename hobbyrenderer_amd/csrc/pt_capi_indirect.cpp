// pt_capi_indirect.cpp -- traced indirect lighting (pt_indirect.h / pt_indirect.hip / pt_indirect_host.cpp): the context calls over the
// G-buffer planes into two library-owned planes and from them into Output, the same over caller-owned device images, and the three host
// executors. The lighting call is the composition of launch_indirect_rays, the public hrpt_trace_radiance (HRPT_RADIANCE_SECONDARY) and
// launch_indirect_resolve.
#include <cmath>

#include "pt_capi_internal.h"
#include "pt_indirect.h"

using namespace hrt;
using namespace hrt::capi;

static const char* const kParamsRule = ": no lobe flag (HRPT_INDIRECT_DIFFUSE | HRPT_INDIRECT_SPECULAR), unknown flag bits, non-zero reserved or an intensity that is not finite";

static int params_check(HrptContext* c, const char* what, const HrptIndirectParams* params)
{
    if (!params) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (!indirect_params_valid(*params)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + kParamsRule);
    return HRPT_OK;
}

// Images of a lighting / resolve call (`compose` false) or of a compose call: present, and no written image among the others.
static int images_check(HrptContext* c, const char* what, const HrptIndirectImages* im, uint32_t width, uint32_t height, uint32_t flags, bool compose)
{
    if (!im) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null images");
    if (!size_ok(width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": size must be 1..65535");
    if (!im->albedo || !im->geoNormal || !im->depth || (!compose && !im->normal)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null image");
    const float* inputs[4] = { im->albedo, im->normal, im->geoNormal, im->depth };
    if (compose) {
        if (!im->diffuse || !im->specular || !im->colorInOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null image");
        for (const float* p : inputs)
            if (p == im->colorInOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": colorInOut must differ from every other image");
        if (im->diffuse == im->colorInOut || im->specular == im->colorInOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": colorInOut must differ from every other image");
        return HRPT_OK;
    }
    if (((flags & HRPT_INDIRECT_DIFFUSE) && !im->diffuse) || ((flags & HRPT_INDIRECT_SPECULAR) && !im->specular))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null image for a flagged lobe");
    for (const float* p : inputs)
        if (p == im->diffuse || p == im->specular) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": an output image must differ from every other image");
    if (im->diffuse && im->diffuse == im->specular) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": an output image must differ from every other image");
    return HRPT_OK;
}

// What hrpt_trace_radiance would refuse, asked before anything is written.
static int lighting_check(HrptContext* c, const char* what, const HrptPathTracerConstants* constants, const HrptIndirectParams* params)
{
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, std::string(what) + ": no scene uploaded");
    if (!constants) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    HRPT_TRY(params_check(c, what, params));
    if (constants->m_MaxBounces > 64u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": m_MaxBounces above 64");
    if (constants->m_LightCount > c->view.lightCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": m_LightCount exceeds the scene's light buffer");
    const bool wavefront = !(params->flags & HRPT_INDIRECT_THREAD_PER_RAY) && wavefront_supports(c->view, *constants);
    if (!wavefront && c->view.instances && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": this two-level structure is deeper than the thread-per-ray kernel's 64-entry stack");
    return HRPT_OK;
}

// Rays, trace and resolve of one call on `stream`, which also carries the trace: the context stream is redirected for its duration.
static int lighting_run(HrptContext* c, const HrptIndirectImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb,
                        const HrptIndirectParams& p, hipStream_t stream)
{
    const size_t WH = (size_t)width * height, n = indirect::record_count(p.flags, WH);
    if (n > (1ull << 31)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_indirect_lighting: more than 2^31 ray records (one hrpt_trace_radiance call)");
    StageImages& ps = c->perSize.stage;
    HIP_TRY(c, ps.dIndirectRays.reserve(n * sizeof(HrptRay)));
    HIP_TRY(c, ps.dIndirectRadiance.reserve(n * sizeof(float4)));
    const indirect::Frame f = indirect::make_frame(cb, p, (int)width, (int)height);
    const ScopedStream redirect(c, stream);
    HIP_TRY(c, launch_indirect_rays(f, im, ps.dIndirectRays, stream));
    const uint32_t traceFlags = HRPT_RADIANCE_DEVICE_POINTERS | HRPT_RADIANCE_SECONDARY | ((p.flags & HRPT_INDIRECT_THREAD_PER_RAY) ? HRPT_RADIANCE_THREAD_PER_RAY : 0u);
    HRPT_TRY(hrpt_trace_radiance(c, ps.dIndirectRays, floats(ps.dIndirectRadiance), (uint64_t)n, &cb, traceFlags));
    HIP_TRY(c, launch_indirect_resolve(f, im, ps.dIndirectRadiance, stream));
    return HRPT_OK;
}

int hrpt_indirect_lighting(HrptContext* c, const HrptPathTracerConstants* constants, const HrptIndirectParams* params)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(lighting_check(c, "hrpt_indirect_lighting", constants, params));
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_indirect_lighting: hrpt_resize not called");
    PerSizeImages& ps = c->perSize;
    HRPT_TRY(planes_requested(c, "hrpt_indirect_lighting", 1u << HRPT_GB_ALBEDO | 1u << HRPT_GB_NORMAL | 1u << HRPT_GB_GEO_NORMAL | 1u << HRPT_GB_DEPTH, false));
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->width * c->height * sizeof(float4);
    for (DeviceBuffer<float4>& image : ps.stage.dIndirect)
        if (!image) HRPT_TRY(realloc_image(c, image, bytes));
    HrptIndirectImages im = {};
    im.albedo = floats(ps.dGBuffer[HRPT_GB_ALBEDO]); im.normal = floats(ps.dGBuffer[HRPT_GB_NORMAL]); im.geoNormal = floats(ps.dGBuffer[HRPT_GB_GEO_NORMAL]);
    im.depth = floats(ps.dGBuffer[HRPT_GB_DEPTH]); im.diffuse = floats(ps.stage.dIndirect[0]); im.specular = floats(ps.stage.dIndirect[1]);
    return lighting_run(c, im, c->width, c->height, *constants, *params, c->stream);
} catch (...) { return caught(c, "hrpt_indirect_lighting"); }

int hrpt_indirect_lighting_device(HrptContext* c, const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                                  const HrptIndirectParams* params, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(lighting_check(c, "hrpt_indirect_lighting_device", constants, params));
    HRPT_TRY(images_check(c, "hrpt_indirect_lighting_device", images, width, height, params->flags, false));
    HIP_TRY(c, hipSetDevice(c->device));
    return lighting_run(c, *images, width, height, *constants, *params, static_cast<hipStream_t>(stream));
} catch (...) { return caught(c, "hrpt_indirect_lighting_device"); }

int hrpt_indirect_compose(HrptContext* c, const HrptIndirectParams* params)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(params_check(c, "hrpt_indirect_compose", params));
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_indirect_compose: hrpt_resize not called");
    PerSizeImages& ps = c->perSize;
    if (!ps.stage.dIndirect[0] || !ps.stage.dIndirect[1])
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_indirect_compose: no indirect planes at the current size (hrpt_indirect_lighting writes them)");
    HIP_TRY(c, hipSetDevice(c->device));
    HrptIndirectImages im = {};
    im.albedo = floats(ps.dGBuffer[HRPT_GB_ALBEDO]); im.geoNormal = floats(ps.dGBuffer[HRPT_GB_GEO_NORMAL]); im.depth = floats(ps.dGBuffer[HRPT_GB_DEPTH]);
    im.diffuse = floats(ps.stage.dIndirect[0]); im.specular = floats(ps.stage.dIndirect[1]); im.colorInOut = floats(ps.dOutput);
    HIP_TRY(c, launch_indirect_compose(im, c->width, c->height, params->intensity, c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_indirect_compose"); }

int hrpt_indirect_compose_device(HrptContext* c, const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptIndirectParams* params, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(params_check(c, "hrpt_indirect_compose_device", params));
    HRPT_TRY(images_check(c, "hrpt_indirect_compose_device", images, width, height, params->flags, true));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_indirect_compose(*images, width, height, params->intensity, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_indirect_compose_device"); }

int hrpt_indirect_rays_device(HrptContext* c, const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                              const HrptIndirectParams* params, HrptRay* raysOut, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_indirect_rays_device";
    if (!constants) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    HRPT_TRY(params_check(c, what, params));
    if (!images) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null images");
    if (!size_ok(width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": size must be 1..65535");
    if (!images->albedo || !images->normal || !images->geoNormal || !images->depth || !raysOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null image");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_indirect_rays(indirect::make_frame(*constants, *params, (int)width, (int)height), *images, raysOut, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_indirect_rays_device"); }

int hrpt_indirect_resolve_device(HrptContext* c, const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                                 const HrptIndirectParams* params, const float* radiance4, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_indirect_resolve_device";
    if (!constants) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    HRPT_TRY(params_check(c, what, params));
    HRPT_TRY(images_check(c, what, images, width, height, params->flags, false));
    if (!radiance4 || radiance4 == images->diffuse || radiance4 == images->specular) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null or aliased radiance");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_indirect_resolve(indirect::make_frame(*constants, *params, (int)width, (int)height), *images, reinterpret_cast<const float4*>(radiance4),
                                       static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_indirect_resolve_device"); }

int hrpt_read_indirect(HrptContext* c, uint32_t which, float* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (which > 1u) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_indirect: which must be 0 (diffuse) or 1 (specular)");
    if (!c->perSize.stage.dIndirect[which]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_indirect: no indirect planes at the current size (hrpt_indirect_lighting writes them)");
    return read_image(c, c->perSize.stage.dIndirect[which], dst, bytes, "hrpt_read_indirect");
} catch (...) { return caught(c, "hrpt_read_indirect"); }

int hrpt_get_indirect_device(HrptContext* c, uint32_t which, void** devicePtr)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (which > 1u || !devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_indirect_device: which must be 0 or 1, and out not null");
    *devicePtr = c->perSize.stage.dIndirect[which];
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_indirect_device"); }

// ---- the stages on the host ----
int hrpt_indirect_rays_host(const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptIndirectParams* params,
                            HrptRay* raysOut, int nthreads)
{
    const char* what = "hrpt_indirect_rays_host";
    if (!constants) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    HRPT_TRY(params_check(nullptr, what, params));
    if (!images) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null images");
    if (!size_ok(width, height)) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": size must be 1..65535");
    if (!images->albedo || !images->normal || !images->geoNormal || !images->depth || !raysOut) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null image");
    return run_host(what, [&] { indirect_rays_host(*images, width, height, *constants, *params, raysOut, host_threads(nthreads)); });
}

int hrpt_indirect_resolve_host(const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptIndirectParams* params,
                               const float* radiance4, int nthreads)
{
    const char* what = "hrpt_indirect_resolve_host";
    if (!constants) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    HRPT_TRY(params_check(nullptr, what, params));
    HRPT_TRY(images_check(nullptr, what, images, width, height, params->flags, false));
    if (!radiance4 || radiance4 == images->diffuse || radiance4 == images->specular) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null or aliased radiance");
    return run_host(what, [&] { indirect_resolve_host(*images, width, height, *constants, *params, radiance4, host_threads(nthreads)); });
}

int hrpt_indirect_compose_host(const HrptIndirectImages* images, uint32_t width, uint32_t height, const HrptIndirectParams* params, int nthreads)
{
    const char* what = "hrpt_indirect_compose_host";
    HRPT_TRY(params_check(nullptr, what, params));
    HRPT_TRY(images_check(nullptr, what, images, width, height, params->flags, true));
    return run_host(what, [&] { indirect_compose_host(*images, width, height, *params, host_threads(nthreads)); });
}

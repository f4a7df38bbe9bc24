// pt_capi_restir.cpp -- resampled direct lighting (pt_restir.h / pt_restir.hip / pt_restir_host.cpp): the context call over the G-buffer
// planes into Output, the same over caller-owned device images, the four passes alone on the device and on the host, and the read-back of
// the reservoirs. The context call is the composition of the four launchers and the public hrpt_trace_rays.
#include <cmath>

#include "pt_capi_internal.h"
#include "pt_restir.h"

using namespace hrt;
using namespace hrt::capi;

static const char* const kParamsRule = ": unknown flag bits, non-zero reserved, candidates outside 1..32, spatialSamples above 8, a spatialRadius outside (0, 65535], "
                                       "a maxHistory that is not finite and positive, or a threshold that is not finite";

enum Pass { kInitial, kTemporal, kSpatial, kShade, kAll };

static int params_check(HrptContext* c, const char* what, const HrptPathTracerConstants* constants, const HrptRestirParams* params)
{
    if (!constants || !params) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null argument");
    if (!restir_params_valid(*params)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + kParamsRule);
    return HRPT_OK;
}

// The images a pass reads and writes: present, and nothing written among what is read. `extraIn` / `extraOut`: the arrays the pass takes
// beside the struct.
static int images_check(HrptContext* c, const char* what, const HrptRestirImages* im, uint32_t width, uint32_t height, uint32_t flags, Pass pass,
                        std::initializer_list<const void*> extraIn = {}, std::initializer_list<const void*> extraOut = {})
{
    if (!im) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null images");
    if (!size_ok(width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": size must be 1..65535");
    if (!im->albedo || !im->normal || !im->geoNormal || !im->depth) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null image");
    const bool temporal = (pass == kTemporal || pass == kAll) && (flags & HRPT_RESTIR_TEMPORAL);
    if (temporal && !im->motion) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": HRPT_RESTIR_TEMPORAL without a motion image");
    if ((im->reservoirIn == nullptr) != (im->keyIn == nullptr)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": reservoirIn and keyIn go together");
    const void* in[16] = { im->albedo, im->normal, im->geoNormal, im->depth, im->emissive };
    const void* out[8] = {};
    size_t nIn = 5, nOut = 0;
    if (temporal) { in[nIn++] = im->motion; in[nIn++] = im->reservoirIn; in[nIn++] = im->keyIn; }
    if (pass != kShade) out[nOut++] = im->reservoirOut;
    if (pass == kSpatial || pass == kAll) out[nOut++] = im->keyOut;
    if (pass == kShade || pass == kAll) {
        if (!im->emissive) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null image");
        out[nOut++] = im->colorOut;
    }
    for (const void* p : extraIn) in[nIn++] = p;
    for (const void* p : extraOut) out[nOut++] = p;
    for (size_t i = 0; i < nOut; ++i) {
        if (!out[i]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null output");
        for (size_t j = 0; j < nIn; ++j)
            if (in[j] == out[i]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": an output must differ from every other image");
        for (size_t j = 0; j < i; ++j)
            if (out[j] == out[i]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": an output must differ from every other image");
    }
    return HRPT_OK;
}

static int device_check(HrptContext* c, const char* what, const HrptPathTracerConstants* constants, const HrptRestirParams* params, bool traces)
{
    if (!c->haveScene) return fail(c, HRPT_ERR_NO_SCENE, std::string(what) + ": no scene uploaded");
    HRPT_TRY(params_check(c, what, constants, params));
    if (constants->m_LightCount > c->view.lightCount) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": m_LightCount exceeds the scene's light buffer");
    const bool rays = (params->flags & (HRPT_RESTIR_SHADOWS | HRPT_RESTIR_INITIAL_VISIBILITY)) != 0u;
    if (traces && rays && c->view.instances && !wavefront_trace_rays_supported(c->traits) && exceeds_private_stack(c->traits))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": this two-level structure is deeper than the thread-per-ray kernel's 64-entry stack");
    return HRPT_OK;
}

static restir::Args device_args(HrptContext* c, const HrptPathTracerConstants& cb, const HrptRestirParams& p, uint32_t width, uint32_t height)
{
    return restir::make_args(cb, p, c->keptLights.empty() ? 0.0f : c->keptLights[0].m_Intensity, (int)width, (int)height);
}

// The passes of one call on `stream`, which also carries the trace calls: the context stream is redirected for their duration. The initial
// pass writes into im.reservoirOut, the temporal pass from there into the library's scratch plane, the spatial pass from there into
// im.reservoirOut again.
static int restir_run(HrptContext* c, const HrptRestirImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptRestirParams& p,
                      hipStream_t stream)
{
    const size_t WH = (size_t)width * height;
    StageImages& ps = c->perSize.stage;
    const bool initialVis = (p.flags & HRPT_RESTIR_INITIAL_VISIBILITY) != 0u, shadows = (p.flags & HRPT_RESTIR_SHADOWS) != 0u;
    HIP_TRY(c, ps.dRestirScratch.reserve(WH * sizeof(HrptRestirReservoir)));
    if (initialVis || shadows) {
        HIP_TRY(c, ps.dRestirRays.reserve(WH * sizeof(HrptRay)));
        HIP_TRY(c, ps.dRestirHits.reserve(WH * sizeof(HrptRayHit)));
    }
    const restir::Args a = device_args(c, cb, p, width, height);
    const bool history = (p.flags & HRPT_RESTIR_TEMPORAL) && !(p.flags & HRPT_RESTIR_RESET) && im.reservoirIn && im.keyIn;
    const uint32_t traceFlags = HRPT_RAYS_SHADOW | HRPT_RAYS_DEVICE_POINTERS;
    const ScopedStream redirect(c, stream);
    HIP_TRY(c, launch_restir_initial(c->view, a, c->view.lights, im, initialVis ? ps.dRestirRays.get() : nullptr, !c->restirGlobalLights, stream));
    if (initialVis) HRPT_TRY(hrpt_trace_rays(c, ps.dRestirRays, ps.dRestirHits, (uint64_t)WH, traceFlags));
    HrptRestirImages temporal = im;
    temporal.reservoirOut = ps.dRestirScratch;
    HIP_TRY(c, launch_restir_temporal(c->view, a, c->view.lights, temporal, im.reservoirOut, initialVis ? ps.dRestirHits.get() : nullptr, history, stream));
    HIP_TRY(c, launch_restir_spatial(c->view, a, c->view.lights, im, ps.dRestirScratch, shadows ? ps.dRestirRays.get() : nullptr, stream));
    if (shadows) HRPT_TRY(hrpt_trace_rays(c, ps.dRestirRays, ps.dRestirHits, (uint64_t)WH, traceFlags));
    HIP_TRY(c, launch_restir_shade(c->view, a, c->view.lights, im, im.reservoirOut, shadows ? ps.dRestirHits.get() : nullptr, stream));
    return HRPT_OK;
}

int hrpt_restir_lighting(HrptContext* c, const HrptPathTracerConstants* constants, const HrptRestirParams* params)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_restir_lighting";
    HRPT_TRY(device_check(c, what, constants, params, true));
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": hrpt_resize not called");
    PerSizeImages& ps = c->perSize;
    StageImages& st = ps.stage;
    HRPT_TRY(planes_requested(c, what, 1u << HRPT_GB_ALBEDO | 1u << HRPT_GB_NORMAL | 1u << HRPT_GB_GEO_NORMAL | 1u << HRPT_GB_EMISSIVE | 1u << HRPT_GB_DEPTH,
                              (params->flags & HRPT_RESTIR_TEMPORAL) != 0u));
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t WH = (size_t)c->width * c->height;
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(c, st.dRestirReservoirs[k].reserve(WH * sizeof(HrptRestirReservoir)));
        HIP_TRY(c, st.dRestirKeys[k].reserve(WH * sizeof(float4)));
    }
    const int prev = st.restirCur, next = 1 - prev;
    const bool history = st.restirValid && !(params->flags & HRPT_RESTIR_RESET);
    HrptRestirImages im = {};
    im.albedo = floats(ps.dGBuffer[HRPT_GB_ALBEDO]); im.normal = floats(ps.dGBuffer[HRPT_GB_NORMAL]); im.geoNormal = floats(ps.dGBuffer[HRPT_GB_GEO_NORMAL]);
    im.emissive = floats(ps.dGBuffer[HRPT_GB_EMISSIVE]); im.depth = floats(ps.dGBuffer[HRPT_GB_DEPTH]);
    im.motion = (params->flags & HRPT_RESTIR_TEMPORAL) ? floats(ps.dMotion) : nullptr;
    im.reservoirIn = history ? st.dRestirReservoirs[prev].get() : nullptr; im.keyIn = history ? floats(st.dRestirKeys[prev]) : nullptr;
    im.reservoirOut = st.dRestirReservoirs[next]; im.keyOut = floats(st.dRestirKeys[next]);
    im.colorOut = floats(ps.dOutput);
    st.restirValid = false;                                          // a call that fails half-way leaves no history
    HRPT_TRY(restir_run(c, im, c->width, c->height, *constants, *params, c->stream));
    st.restirCur = next; st.restirValid = true;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_restir_lighting"); }

int hrpt_restir_lighting_device(HrptContext* c, const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                                const HrptRestirParams* params, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_restir_lighting_device";
    HRPT_TRY(device_check(c, what, constants, params, true));
    HRPT_TRY(images_check(c, what, images, width, height, params->flags, kAll));
    HIP_TRY(c, hipSetDevice(c->device));
    return restir_run(c, *images, width, height, *constants, *params, static_cast<hipStream_t>(stream));
} catch (...) { return caught(c, "hrpt_restir_lighting_device"); }

int hrpt_read_restir_reservoirs(HrptContext* c, HrptRestirReservoir* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const StageImages& st = c->perSize.stage;
    if (!st.restirValid) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_restir_reservoirs: no reservoirs at the current size (hrpt_restir_lighting writes them)");
    return read_image(c, reinterpret_cast<const float4*>(st.dRestirReservoirs[st.restirCur].get()), reinterpret_cast<float*>(dst), bytes, "hrpt_read_restir_reservoirs");
} catch (...) { return caught(c, "hrpt_read_restir_reservoirs"); }

int hrpt_get_restir_device(HrptContext* c, void** reservoirs, void** keys)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!reservoirs || !keys) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_restir_device: null argument");
    const StageImages& st = c->perSize.stage;
    *reservoirs = st.restirValid ? st.dRestirReservoirs[st.restirCur].get() : nullptr;
    *keys = st.restirValid ? st.dRestirKeys[st.restirCur].get() : nullptr;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_restir_device"); }

// ---- the four kernels alone ----
int hrpt_restir_initial_device(HrptContext* c, const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                               const HrptRestirParams* params, HrptRay* raysOut, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_restir_initial_device";
    HRPT_TRY(device_check(c, what, constants, params, false));
    HRPT_TRY(images_check(c, what, images, width, height, params->flags, kInitial));
    if ((params->flags & HRPT_RESTIR_INITIAL_VISIBILITY) && !raysOut) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": HRPT_RESTIR_INITIAL_VISIBILITY without raysOut");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_restir_initial(c->view, device_args(c, *constants, *params, width, height), c->view.lights, *images,
                                     (params->flags & HRPT_RESTIR_INITIAL_VISIBILITY) ? raysOut : nullptr, !c->restirGlobalLights, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_restir_initial_device"); }

int hrpt_restir_temporal_device(HrptContext* c, const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                                const HrptRestirParams* params, const HrptRestirReservoir* initial, const HrptRayHit* initialHits, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_restir_temporal_device";
    HRPT_TRY(device_check(c, what, constants, params, false));
    HRPT_TRY(images_check(c, what, images, width, height, params->flags, kTemporal, { initial, initialHits }));
    if (!initial) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null reservoirs");
    const bool history = (params->flags & HRPT_RESTIR_TEMPORAL) && !(params->flags & HRPT_RESTIR_RESET) && images->reservoirIn && images->keyIn;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_restir_temporal(c->view, device_args(c, *constants, *params, width, height), c->view.lights, *images, initial, initialHits, history,
                                      static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_restir_temporal_device"); }

int hrpt_restir_spatial_device(HrptContext* c, const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                               const HrptRestirParams* params, const HrptRestirReservoir* temporal, HrptRay* raysOut, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_restir_spatial_device";
    HRPT_TRY(device_check(c, what, constants, params, false));
    HRPT_TRY(images_check(c, what, images, width, height, params->flags, kSpatial, { temporal }));
    if (!temporal) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null reservoirs");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_restir_spatial(c->view, device_args(c, *constants, *params, width, height), c->view.lights, *images, temporal, raysOut, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_restir_spatial_device"); }

int hrpt_restir_shade_device(HrptContext* c, const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants,
                             const HrptRestirParams* params, const HrptRestirReservoir* final, const HrptRayHit* hits, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    const char* what = "hrpt_restir_shade_device";
    HRPT_TRY(device_check(c, what, constants, params, false));
    HRPT_TRY(images_check(c, what, images, width, height, params->flags, kShade, { final, hits }));
    if (!final) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null reservoirs");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_restir_shade(c->view, device_args(c, *constants, *params, width, height), c->view.lights, *images, final, hits, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_restir_shade_device"); }

// ---- the four passes on the host ----
static int host_check(const char* what, const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptGPULight* lights,
                      const HrptRestirParams* params, Pass pass, std::initializer_list<const void*> extraIn, std::initializer_list<const void*> extraOut = {})
{
    HRPT_TRY(params_check(nullptr, what, constants, params));
    HRPT_TRY(images_check(nullptr, what, images, width, height, params->flags, pass, extraIn, extraOut));
    if (constants->m_LightCount > 0u && !lights) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null lights");
    return HRPT_OK;
}

int hrpt_restir_initial_host(const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptGPULight* lights,
                             const HrptRestirParams* params, const float* sunRadiance, HrptRay* raysOut, int nthreads)
{
    const char* what = "hrpt_restir_initial_host";
    HRPT_TRY(host_check(what, images, width, height, constants, lights, params, kInitial, { sunRadiance }));
    const bool vis = (params->flags & HRPT_RESTIR_INITIAL_VISIBILITY) != 0u;
    if (vis && !raysOut) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": HRPT_RESTIR_INITIAL_VISIBILITY without raysOut");
    return run_host(what, [&] { restir_initial_host(*images, width, height, *constants, lights, *params, sunRadiance, vis ? raysOut : nullptr, host_threads(nthreads)); });
}

int hrpt_restir_temporal_host(const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptGPULight* lights,
                              const HrptRestirParams* params, const float* sunRadiance, const HrptRestirReservoir* initial, const float* initialVisibility, int nthreads)
{
    const char* what = "hrpt_restir_temporal_host";
    HRPT_TRY(host_check(what, images, width, height, constants, lights, params, kTemporal, { sunRadiance, initial, initialVisibility }));
    if (!initial) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null reservoirs");
    return run_host(what, [&] { restir_temporal_host(*images, width, height, *constants, lights, *params, sunRadiance, initial, initialVisibility, host_threads(nthreads)); });
}

int hrpt_restir_spatial_host(const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptGPULight* lights,
                             const HrptRestirParams* params, const float* sunRadiance, const HrptRestirReservoir* temporal, HrptRay* raysOut, int nthreads)
{
    const char* what = "hrpt_restir_spatial_host";
    HRPT_TRY(host_check(what, images, width, height, constants, lights, params, kSpatial, { sunRadiance, temporal }));
    if (!temporal) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null reservoirs");
    return run_host(what, [&] { restir_spatial_host(*images, width, height, *constants, lights, *params, sunRadiance, temporal, raysOut, host_threads(nthreads)); });
}

int hrpt_restir_shade_host(const HrptRestirImages* images, uint32_t width, uint32_t height, const HrptPathTracerConstants* constants, const HrptGPULight* lights,
                           const HrptRestirParams* params, const float* sunRadiance, const float* sky, const HrptRestirReservoir* final, const float* visibility, int nthreads)
{
    const char* what = "hrpt_restir_shade_host";
    HRPT_TRY(host_check(what, images, width, height, constants, lights, params, kShade, { sunRadiance, sky, final, visibility }));
    if (!final) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": null reservoirs");
    return run_host(what, [&] { restir_shade_host(*images, width, height, *constants, lights, *params, sunRadiance, sky, final, visibility, host_threads(nthreads)); });
}

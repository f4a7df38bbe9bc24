// pt_capi_post.cpp -- what works on finished images: hrpt_post_process and the exposure, then the screen-space stages (bloom, temporal
// accumulation, temporal upscaling, denoise, demodulate / compose) with their _host, _device and probe entry points.
#include <cmath>

#include "pt_capi_internal.h"

using namespace hrt;
using namespace hrt::capi;

// The context's histogram (initially all zero) and exposure (initially 1), allocated by the first post pass or hrpt_set_exposure: the one
// place that allocates and initialises them.
static int post_buffers(HrptContext* c)
{
    if (c->perContext.dExposure) return HRPT_OK;
    DeviceBuffer<float> exposure;
    DeviceBuffer<uint32_t> histogram;
    HIP_TRY(c, exposure.alloc(16));
    HIP_TRY(c, histogram.alloc(256 * sizeof(uint32_t)));
    const float one[4] = { 1.0f, 0.0f, 0.0f, 0.0f };
    const uint32_t zero[256] = {};
    HIP_TRY(c, hipMemcpy(exposure, one, 16, hipMemcpyHostToDevice));      // both complete on return: ordered before every later launch
    HIP_TRY(c, hipMemcpy(histogram, zero, sizeof zero, hipMemcpyHostToDevice));
    c->perContext.dExposure = std::move(exposure); c->perContext.dHistogram = std::move(histogram);
    return HRPT_OK;
}

int hrpt_post_process_device(HrptContext* c, const float* hdrDevice, float* displayDevice, uint64_t pixelCount, const HrptPostParams* p, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_post_process_device: null params");
    if (!hdrDevice || !displayDevice) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_post_process_device: null image");
    if (displayDevice == hdrDevice) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_post_process_device: displayDevice must differ from hdrDevice");
    if (pixelCount == 0 || pixelCount > 0xffffffffull) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_post_process_device: pixelCount must be 1..2^32-1");
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(post_buffers(c));
    HIP_TRY(c, launch_post_chain(reinterpret_cast<const float4*>(hdrDevice), reinterpret_cast<float4*>(displayDevice), (uint32_t)pixelCount, *p,
                                 c->perContext.dHistogram, c->perContext.dExposure, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_post_process_device"); }

int hrpt_post_process(HrptContext* c, const HrptPostParams* p)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_post_process: null params");
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_post_process: hrpt_resize not called");
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(post_buffers(c));
    HIP_TRY(c, c->perSize.stage.dDisplay.reserve((size_t)c->width * c->height * sizeof(float4)));
    HIP_TRY(c, launch_post_chain(c->perSize.dOutput, c->perSize.stage.dDisplay, c->width * c->height, *p, c->perContext.dHistogram, c->perContext.dExposure, c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_post_process"); }

// ---- screen-space stages: bloom, temporal accumulation, temporal upscaling, denoise, demodulate / compose ----
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

// Pyramids for a width x height image: kept while the size stays, re-allocated when it changes (hipFree waits for work in flight).
static int bloom_run(HrptContext* c, float4* image, uint32_t width, uint32_t height, const HrptBloomParams& p, hipStream_t stream)
{
    const size_t bytes = bloom_pyramid_words(width, height) * sizeof(uint32_t);
    if (bytes == 0) return HRPT_OK;
    if (bytes != c->perContext.dBloomDown.bytes() || bytes != c->perContext.dBloomUp.bytes()) {
        c->perContext.dBloomDown.reset(); c->perContext.dBloomUp.reset();     // both go before anything is allocated
        HIP_TRY(c, c->perContext.dBloomDown.alloc(bytes));
        HIP_TRY(c, c->perContext.dBloomUp.alloc(bytes));
    }
    HIP_TRY(c, launch_bloom(image, width, height, p, c->perContext.dBloomDown, c->perContext.dBloomUp, c->bloomTailTexels, stream));
    return HRPT_OK;
}

int hrpt_bloom(HrptContext* c, const HrptBloomParams* p)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom: null params");
    if (!bloom_params_valid(*p)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom: knee, intensity and upsampleRadius must be finite and >= 0");
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom: hrpt_resize not called");
    HIP_TRY(c, hipSetDevice(c->device));
    return bloom_run(c, c->perSize.dOutput, c->width, c->height, *p, c->stream);
} catch (...) { return caught(c, "hrpt_bloom"); }

int hrpt_bloom_device(HrptContext* c, float* hdrDevice, uint32_t width, uint32_t height, const HrptBloomParams* p, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_device: null params");
    if (!hdrDevice) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_device: null image");
    if (!size_ok(width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_device: size must be 1..65535");
    if (!bloom_params_valid(*p)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_bloom_device: knee, intensity and upsampleRadius must be finite and >= 0");
    HIP_TRY(c, hipSetDevice(c->device));
    return bloom_run(c, reinterpret_cast<float4*>(hdrDevice), width, height, *p, static_cast<hipStream_t>(stream));
} catch (...) { return caught(c, "hrpt_bloom_device"); }

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
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(temporal_check(c, "hrpt_temporal_device", img, width, height, view, prevView, p));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_temporal(*img, width, height, *view, *prevView, *p, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_temporal_device"); }

int hrpt_temporal_accumulate(HrptContext* c, const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView, const HrptTemporalParams* p)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!view || !prevView || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_temporal_accumulate: null argument");
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_temporal_accumulate: hrpt_resize not called");
    HRPT_TRY(planes_requested(c, "hrpt_temporal_accumulate", 1u << HRPT_GB_DEPTH | 1u << HRPT_GB_NORMAL, true));
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(temporal_args_check(c, "hrpt_temporal_accumulate", c->width, c->height, *view, *p));      // before anything is allocated
    PerSizeImages& ps = c->perSize;
    const bool fresh = !ps.dTemporal[0];
    const int next = fresh ? 0 : 1 - ps.temporalCur;
    if (fresh) {
        for (DeviceBuffer<float4>& image : ps.dTemporal) HRPT_TRY(realloc_image(c, image, (size_t)c->width * c->height * sizeof(float4)));
        ps.temporalValid = false;
    }
    HrptTemporalImages img{};
    img.color = floats(ps.dOutput); img.colorOut = floats(ps.dOutput); img.motion = floats(ps.dMotion);
    img.depth = floats(ps.dGBuffer[HRPT_GB_DEPTH]); img.normal = floats(ps.dGBuffer[HRPT_GB_NORMAL]);
    const bool useHistory = ps.temporalValid && (p->flags & HRPT_TEMPORAL_RESET) == 0;
    img.historyIn = useHistory ? floats(ps.dTemporal[1 - next]) : nullptr;
    img.historyOut = floats(ps.dTemporal[next]);
    HIP_TRY(c, launch_temporal(img, c->width, c->height, *view, *prevView, *p, c->stream));
    ps.temporalCur = next; ps.temporalValid = true;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_temporal_accumulate"); }

int hrpt_read_temporal_history(HrptContext* c, float* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.dTemporal[0]) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_temporal_history: the history was never requested from hrpt_temporal_accumulate");
    return read_image(c, c->perSize.dTemporal[c->perSize.temporalCur], dst, bytes, "hrpt_read_temporal_history");
} catch (...) { return caught(c, "hrpt_read_temporal_history"); }

int hrpt_get_temporal_history_device(HrptContext* c, void** devicePtr)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_temporal_history_device: null out");
    *devicePtr = c->perSize.dTemporal[0] ? c->perSize.dTemporal[c->perSize.temporalCur] : nullptr;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_temporal_history_device"); }

// ---- temporal upscaling (pt_upscale.h / pt_upscale.hip) ----
// Sizes, view and parameters: all a context call has left to check once its arguments are not null (its images are the context's own).
static int upscale_args_check(HrptContext* c, const std::string& w, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                              const HrptPlanarViewConstants& view, const HrptUpscaleParams& p)
{
    if (!size_ok(width, height) || !size_ok(displayWidth, displayHeight)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": size must be 1..65535");
    if (!upscale_ratio_ok(width, height, displayWidth, displayHeight))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": the display size must lie between the render size and four times it, per axis");
    if (!view_matches(view, width, height)) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": view->m_ViewportSize does not match the image size");
    if (!upscale_params_valid(p))
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": jitter must be finite and in [-0.5, 0.5], kernel finite and in (0, 16], maxHistory finite and >= 0, flags HRPT_UPSCALE_* only, reserved 0");
    return HRPT_OK;
}
// Caller-owned images: the null checks and the aliasing rules first, then the above.
static int upscale_check(HrptContext* c, const char* what, const HrptUpscaleImages* img, uint32_t width, uint32_t height, uint32_t displayWidth,
                         uint32_t displayHeight, const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView, const HrptUpscaleParams* p)
{
    const std::string w(what);
    if (!img || !view || !prevView || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null argument");
    if (!img->color || !img->depth || !img->motion || !img->historyOut || !img->colorOut)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": null image (only historyIn may be NULL)");
    if (img->historyOut == img->historyIn) return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": historyOut must differ from historyIn");
    if (img->colorOut == img->historyIn || img->colorOut == img->historyOut)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, w + ": colorOut must differ from historyIn and historyOut");
    return upscale_args_check(c, w, width, height, displayWidth, displayHeight, *view, *p);
}

int hrpt_upscale_host(const HrptUpscaleImages* img, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                      const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView, const HrptUpscaleParams* p, int nthreads)
{
    HRPT_TRY(upscale_check(nullptr, "hrpt_upscale_host", img, width, height, displayWidth, displayHeight, view, prevView, p));
    return run_host("hrpt_upscale_host", [&] { upscale_host(*img, width, height, displayWidth, displayHeight, *view, *prevView, *p, host_threads(nthreads)); });
}

int hrpt_upscale_device(HrptContext* c, const HrptUpscaleImages* img, uint32_t width, uint32_t height, uint32_t displayWidth, uint32_t displayHeight,
                        const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView, const HrptUpscaleParams* p, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(upscale_check(c, "hrpt_upscale_device", img, width, height, displayWidth, displayHeight, view, prevView, p));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_upscale(*img, width, height, displayWidth, displayHeight, *view, *prevView, *p, c->upscaleStaged, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_upscale_device"); }

int hrpt_upscale(HrptContext* c, uint32_t displayWidth, uint32_t displayHeight, const HrptPlanarViewConstants* view, const HrptPlanarViewConstants* prevView,
                 const HrptUpscaleParams* p)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!view || !prevView || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upscale: null argument");
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_upscale: hrpt_resize not called");
    HRPT_TRY(planes_requested(c, "hrpt_upscale", 1u << HRPT_GB_DEPTH, true));
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(upscale_args_check(c, "hrpt_upscale", c->width, c->height, displayWidth, displayHeight, *view, *p));      // before anything is allocated
    StageImages& st = c->perSize.stage;
    if (!st.dUpscaled || displayWidth != st.upscaleWidth || displayHeight != st.upscaleHeight) {
        for (DeviceBuffer<float4>& image : st.dUpscaleHistory) image.reset();           // all three go before anything is allocated
        st.dUpscaled.reset(); st.upscaleValid = false; st.upscaleCur = 0; st.upscaleWidth = st.upscaleHeight = 0;
        const size_t bytes = (size_t)displayWidth * displayHeight * sizeof(float4);
        for (DeviceBuffer<float4>& image : st.dUpscaleHistory) HRPT_TRY(realloc_image(c, image, bytes));
        HRPT_TRY(realloc_image(c, st.dUpscaled, bytes));
        st.upscaleWidth = displayWidth; st.upscaleHeight = displayHeight;
    }
    const int next = st.upscaleValid ? 1 - st.upscaleCur : 0;
    HrptUpscaleImages img{};
    img.color = floats(c->perSize.dOutput); img.depth = floats(c->perSize.dGBuffer[HRPT_GB_DEPTH]); img.motion = floats(c->perSize.dMotion);
    const bool useHistory = st.upscaleValid && (p->flags & HRPT_UPSCALE_RESET) == 0;
    img.historyIn = useHistory ? floats(st.dUpscaleHistory[1 - next]) : nullptr;
    img.historyOut = floats(st.dUpscaleHistory[next]);
    img.colorOut = floats(st.dUpscaled);
    HIP_TRY(c, launch_upscale(img, c->width, c->height, displayWidth, displayHeight, *view, *prevView, *p, c->upscaleStaged, c->stream));
    st.upscaleCur = next; st.upscaleValid = true;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_upscale"); }

// A display-size image of the upscale stage to the host: read_image's protocol with the size of the last hrpt_upscale.
static int read_upscale_image(HrptContext* c, const float4* src, float* dst, size_t bytes, const char* what)
{
    if (!src) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": no upscaled image (hrpt_upscale writes it; hrpt_resize drops it)");
    if (!dst || bytes != (size_t)c->perSize.stage.upscaleWidth * c->perSize.stage.upscaleHeight * 16) return fail(c, HRPT_ERR_INVALID_ARGUMENT, std::string(what) + ": bad buffer size");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
}

int hrpt_read_upscaled(HrptContext* c, float* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    return read_upscale_image(c, c->perSize.stage.dUpscaled, dst, bytes, "hrpt_read_upscaled");
} catch (...) { return caught(c, "hrpt_read_upscaled"); }

int hrpt_read_upscale_history(HrptContext* c, float* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    return read_upscale_image(c, c->perSize.stage.dUpscaled ? c->perSize.stage.dUpscaleHistory[c->perSize.stage.upscaleCur].get() : nullptr, dst, bytes, "hrpt_read_upscale_history");
} catch (...) { return caught(c, "hrpt_read_upscale_history"); }

int hrpt_get_upscaled_device(HrptContext* c, void** devicePtr)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_upscaled_device: null out");
    *devicePtr = c->perSize.stage.dUpscaled;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_upscaled_device"); }

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
    if (c->perContext.dDenoiseTile) return HRPT_OK;
    std::vector<float> tile(denoise_noise_floats());
    denoise_default_tile(tile.data());
    DeviceBuffer<float> d;
    HIP_TRY(c, d.alloc(tile.size() * sizeof(float)));
    HIP_TRY(c, hipMemcpy(d, tile.data(), tile.size() * sizeof(float), hipMemcpyHostToDevice));     // complete on return: ordered before every later launch
    c->perContext.dDenoiseTile = std::move(d);
    return HRPT_OK;
}

int hrpt_set_denoise_noise(HrptContext* c, const float* hostTile)
try {
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
    HIP_TRY(c, hipMemcpyAsync(c->perContext.dDenoiseTile, tile.data(), count * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_set_denoise_noise"); }

int hrpt_denoise_host(const HrptDenoiseImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view, const HrptDenoiseParams* p, int nthreads)
{
    HRPT_TRY(denoise_check(nullptr, "hrpt_denoise_host", img, width, height, view, p));
    return run_host("hrpt_denoise_host", [&] { denoise_host(*img, width, height, *view, *p, host_threads(nthreads)); });
}

int hrpt_denoise_device(HrptContext* c, const HrptDenoiseImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                        const HrptDenoiseParams* p, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(denoise_check(c, "hrpt_denoise_device", img, width, height, view, p));
    HIP_TRY(c, hipSetDevice(c->device));
    HrptDenoiseImages im = *img;
    if (!im.noise) { HRPT_TRY(denoise_tile(c)); im.noise = c->perContext.dDenoiseTile; }
    HIP_TRY(c, launch_denoise(im, width, height, *view, *p, p->radius, p->frame, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_denoise_device"); }

int hrpt_denoise(HrptContext* c, const HrptPlanarViewConstants* view, const HrptDenoiseParams* p)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!view || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_denoise: null argument");
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_denoise: hrpt_resize not called");
    PerSizeImages& ps = c->perSize;
    if (!ps.dTemporal[0] || !ps.temporalValid)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_denoise: no temporal history at the current size (hrpt_temporal_accumulate writes the image this stage filters)");
    HRPT_TRY(planes_requested(c, "hrpt_denoise", 1u << HRPT_GB_DEPTH | 1u << HRPT_GB_NORMAL | 1u << HRPT_GB_GEO_NORMAL, false));
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(denoise_args_check(c, "hrpt_denoise", c->width, c->height, *view, *p, false));
    HRPT_TRY(denoise_tile(c));
    HrptDenoiseImages img{};
    img.input = floats(ps.dTemporal[ps.temporalCur]);
    img.depth = floats(ps.dGBuffer[HRPT_GB_DEPTH]); img.normal = floats(ps.dGBuffer[HRPT_GB_NORMAL]); img.geoNormal = floats(ps.dGBuffer[HRPT_GB_GEO_NORMAL]);
    img.noise = c->perContext.dDenoiseTile;
    const bool outputOnly = (p->flags & HRPT_DENOISE_OUTPUT_ONLY) != 0;
    if (outputOnly) {
        for (uint32_t k = 0; k < (p->iterations > 1u ? 2u : 1u); ++k) HIP_TRY(c, ps.stage.dDenoiseScratch[k].reserve((size_t)c->width * c->height * sizeof(float4)));
    }
    int cur = ps.temporalCur;
    for (uint32_t i = 0; i < p->iterations; ++i) {
        // default: the two history images are the ping-pong pair (the stale one is free after the temporal call); the image a pass wrote is the history
        DeviceBuffer<float4>& dst = outputOnly ? ps.stage.dDenoiseScratch[i & 1u] : ps.dTemporal[1 - cur];
        img.output = floats(dst);
        const bool last = i + 1u == p->iterations;
        img.color = last ? floats(ps.dOutput) : nullptr;
        img.colorOut = last ? floats(ps.dOutput) : nullptr;
        HIP_TRY(c, launch_denoise(img, c->width, c->height, *view, *p, p->radius * (float)(1u << i), p->frame * p->iterations + i, c->stream));
        img.input = floats(dst);
        if (!outputOnly) { cur = 1 - cur; ps.temporalCur = cur; }
    }
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_denoise"); }

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

int hrpt_compose_host(const HrptComposeImages* img, uint32_t width, uint32_t height, int nthreads)
{
    HRPT_TRY(compose_check(nullptr, "hrpt_compose_host", img, width, height));
    return run_host("hrpt_compose_host", [&] { compose_host(*img, width, height, host_threads(nthreads)); });
}

int hrpt_demodulate_device(HrptContext* c, const HrptDemodulateImages* img, uint32_t width, uint32_t height, const HrptPlanarViewConstants* view,
                           const HrptModulationParams* p, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(demodulate_check(c, "hrpt_demodulate_device", img, width, height, view, p));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_demodulate(*img, width, height, *view, *p, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_demodulate_device"); }

int hrpt_compose_device(HrptContext* c, const HrptComposeImages* img, uint32_t width, uint32_t height, void* stream)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HRPT_TRY(compose_check(c, "hrpt_compose_device", img, width, height));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_compose(*img, width, height, static_cast<hipStream_t>(stream)));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_compose_device"); }

int hrpt_demodulate(HrptContext* c, const HrptPlanarViewConstants* view, const HrptModulationParams* p)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!view || !p) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_demodulate: null argument");
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_demodulate: hrpt_resize not called");
    HRPT_TRY(planes_requested(c, "hrpt_demodulate", 1u << HRPT_GB_ALBEDO | 1u << HRPT_GB_NORMAL | 1u << HRPT_GB_GEO_NORMAL | 1u << HRPT_GB_EMISSIVE | 1u << HRPT_GB_DEPTH, false));
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(demodulate_args_check(c, "hrpt_demodulate", c->width, c->height, *view, *p));      // before anything is allocated
    PerSizeImages& ps = c->perSize;
    HIP_TRY(c, ps.stage.dModulation.reserve((size_t)c->width * c->height * sizeof(float4)));
    HrptDemodulateImages img{};
    img.color = floats(ps.dOutput); img.colorOut = floats(ps.dOutput);
    img.albedo = floats(ps.dGBuffer[HRPT_GB_ALBEDO]); img.normal = floats(ps.dGBuffer[HRPT_GB_NORMAL]); img.geoNormal = floats(ps.dGBuffer[HRPT_GB_GEO_NORMAL]);
    img.depth = floats(ps.dGBuffer[HRPT_GB_DEPTH]); img.emissive = floats(ps.dGBuffer[HRPT_GB_EMISSIVE]);
    img.modulationOut = floats(ps.stage.dModulation);
    HIP_TRY(c, launch_demodulate(img, c->width, c->height, *view, *p, c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_demodulate"); }

int hrpt_compose(HrptContext* c)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.dOutput) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_compose: hrpt_resize not called");
    if (!c->perSize.stage.dModulation)
        return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_compose: no modulation image at the current size (hrpt_demodulate writes the factor this stage multiplies back in)");
    HIP_TRY(c, hipSetDevice(c->device));
    HrptComposeImages img{};
    img.color = floats(c->perSize.dOutput); img.colorOut = floats(c->perSize.dOutput);
    img.modulation = floats(c->perSize.stage.dModulation);
    img.emissive = floats(c->perSize.dGBuffer[HRPT_GB_EMISSIVE]);      // set: hrpt_demodulate required it, and a resize drops the modulation image
    HIP_TRY(c, launch_compose(img, c->width, c->height, c->stream));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_compose"); }

int hrpt_read_modulation(HrptContext* c, float* dst, size_t bytes)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!c->perSize.stage.dModulation) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_read_modulation: no modulation image at the current size (hrpt_demodulate writes it)");
    return read_image(c, c->perSize.stage.dModulation, dst, bytes, "hrpt_read_modulation");
} catch (...) { return caught(c, "hrpt_read_modulation"); }

int hrpt_get_modulation_device(HrptContext* c, void** devicePtr)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!devicePtr) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_modulation_device: null out");
    *devicePtr = c->perSize.stage.dModulation;
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_modulation_device"); }

int hrpt_modulation_probe(const float* albedo3, const float* N3, const float* V3, float rough, float metal, float floor, float* outM3)
{
    if (!albedo3 || !N3 || !V3 || !outM3) return fail(nullptr, HRPT_ERR_INVALID_ARGUMENT, "hrpt_modulation_probe: null argument");
    modulation_probe(albedo3, N3, V3, rough, metal, floor, outM3);
    return HRPT_OK;
}

int hrpt_get_exposure(HrptContext* c, float* exposure, uint32_t histogram256[256])
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    if (!exposure || !c->perContext.dExposure) return fail(c, HRPT_ERR_INVALID_ARGUMENT, "hrpt_get_exposure: no post pass has run");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(exposure, c->perContext.dExposure, sizeof(float), hipMemcpyDeviceToHost));
    if (histogram256) HIP_TRY(c, hipMemcpy(histogram256, c->perContext.dHistogram, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_get_exposure"); }

int hrpt_set_exposure(HrptContext* c, float exposure)
try {
    if (!c) return HRPT_ERR_INVALID_ARGUMENT;
    HIP_TRY(c, hipSetDevice(c->device));
    HRPT_TRY(post_buffers(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(c->perContext.dExposure, &exposure, sizeof(float), hipMemcpyHostToDevice));
    return HRPT_OK;
} catch (...) { return caught(c, "hrpt_set_exposure"); }

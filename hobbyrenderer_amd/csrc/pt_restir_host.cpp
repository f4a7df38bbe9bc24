// pt_restir_host.cpp -- the host-thread executors of resampled direct lighting (hrpt_restir_initial_host, _temporal_host, _spatial_host,
// _shade_host): pt_restir.h's passes over the pixels of host images. Plain C++ with no HIP call, so that the sanitizer program
// (restir_asan.cpp, `make restir_asan`) builds it with g++ as it is.
#include <cstring>

#include "pt_restir.h"
#include "pt_host_rows.h"

namespace hrt {

using namespace restir;

namespace {
struct HostIO {
    T4 ld(const float* image, size_t idx) const { const float* p = image + idx * 4; return t4(p[0], p[1], p[2], p[3]); }
    void st(float* image, size_t idx, T4 v) const { store4(image + idx * 4, v); }
};
// Radiance of the directional light l at the surface point of pixel (x, y): the image's texel, or colour x intensity without one.
struct HostSun {
    const float* image; int w;
    f3 operator()(const HrptGPULight& l, f3, int x, int y) const { return image ? deferred::xyz(img::load4(image, w, x, y)) : deferred::light_color(l); }
};
// A pixel writes only its own records and texels, so the result does not depend on nthreads.
template <class Pixel> void over_pixels(const Args& a, int nthreads, Pixel pixel)
{
    over_rows(a.d.h, nthreads, [&](int py) { for (int px = 0; px < a.d.w; ++px) pixel(px, py); });
}
} // namespace

bool restir_params_valid(const HrptRestirParams& params) { return params_valid(params); }

void restir_initial_host(const HrptRestirImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptGPULight* lights,
                         const HrptRestirParams& params, const float* sunRadiance, HrptRay* raysOut, int nthreads)
{
    const Args a = make_args(cb, params, 0.0f, (int)width, (int)height);
    const HostSun sun = { sunRadiance, a.d.w };
    over_pixels(a, nthreads, [&](int px, int py) { initial_pixel(a, im, lights, HostIO{}, sun, px, py, raysOut); });
}

void restir_temporal_host(const HrptRestirImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptGPULight* lights,
                          const HrptRestirParams& params, const float* sunRadiance, const HrptRestirReservoir* initial, const float* initialVisibility, int nthreads)
{
    const Args a = make_args(cb, params, 0.0f, (int)width, (int)height);
    const HostSun sun = { sunRadiance, a.d.w };
    const bool history = (params.flags & HRPT_RESTIR_TEMPORAL) && !(params.flags & HRPT_RESTIR_RESET) && im.reservoirIn && im.keyIn;
    over_pixels(a, nthreads, [&](int px, int py) { temporal_pixel(a, im, lights, HostIO{}, sun, px, py, initial, initialVisibility, 1, history); });
}

void restir_spatial_host(const HrptRestirImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptGPULight* lights,
                         const HrptRestirParams& params, const float* sunRadiance, const HrptRestirReservoir* temporal, HrptRay* raysOut, int nthreads)
{
    const Args a = make_args(cb, params, 0.0f, (int)width, (int)height);
    const HostSun sun = { sunRadiance, a.d.w };
    over_pixels(a, nthreads, [&](int px, int py) { spatial_pixel(a, im, lights, HostIO{}, sun, px, py, temporal, raysOut); });
}

void restir_shade_host(const HrptRestirImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptGPULight* lights,
                       const HrptRestirParams& params, const float* sunRadiance, const float* sky, const HrptRestirReservoir* fin, const float* visibility, int nthreads)
{
    const Args a = make_args(cb, params, 0.0f, (int)width, (int)height);
    const HostSun sun = { sunRadiance, a.d.w };
    over_pixels(a, nthreads, [&](int px, int py) {
        shade_pixel(a, im, lights, HostIO{}, sun, [&](int x, int y) { return sky ? img::load4(sky, a.d.w, x, y) : t4(0.0f, 0.0f, 0.0f, 0.0f); }, px, py, fin, visibility, 1);
    });
}

} // namespace hrt

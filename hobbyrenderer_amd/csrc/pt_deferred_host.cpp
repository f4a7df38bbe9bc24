// pt_deferred_host.cpp -- the host-thread executors of deferred lighting (hrpt_deferred_rays_host / hrpt_deferred_shade_host):
// pt_deferred.h's functions over the pixels of host images. Plain C++ with no HIP call, so that the sanitizer program (deferred_asan.cpp,
// `make deferred_asan`) builds it with g++ as it is.
#include <cstring>

#include "pt_deferred.h"
#include "pt_host_rows.h"

namespace hrt {

using namespace deferred;

bool deferred_params_valid(const HrptDeferredParams& params) { return params_valid(params); }

void deferred_rays_host(const HrptDeferredImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptGPULight* lights,
                        uint32_t firstLight, uint32_t lightCount, HrptRay* raysOut)
{
    const HrptDeferredParams none = { 0u, 0.0f, { 0u, 0u } };
    const Frame f = make_frame(cb, none, 0.0f, (int)width, (int)height);
    const size_t WH = (size_t)width * height;
    for (uint32_t j = 0; j < lightCount; ++j)
        for (int py = 0; py < f.h; ++py)
            for (int px = 0; px < f.w; ++px) {
                T4 rows[3];
                pixel_ray(f, lights[firstLight + j], load4(im.depth, f.w, px, py), load4(im.normal, f.w, px, py), px, py, rows);
                float* rec = reinterpret_cast<float*>(raysOut + ((size_t)j * WH + (size_t)py * width + px));
                for (int r = 0; r < 3; ++r) store4(rec + r * 4, rows[r]);
            }
}

// One image row per "row": a pixel writes only its own texel, so the result does not depend on nthreads.
void deferred_shade_host(const HrptDeferredImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptGPULight* lights,
                         uint32_t lightCount, const float* visibility, const float* sunRadiance, const float* sky, const HrptDeferredParams& params,
                         int nthreads)
{
    const Frame f = make_frame(cb, params, 0.0f, (int)width, (int)height);
    const size_t WH = (size_t)width * height;
    const f3 sunDir = mk3(f.sun);
    over_rows(f.h, nthreads, [&](int py) {
        for (int px = 0; px < f.w; ++px) {
            const size_t idx = (size_t)py * width + px;
            float* out = im.colorOut + idx * 4;
            const T4 D = load4(im.depth, f.w, px, py);
            if (D.x == img::kMissDepth) {
                store4(out, sky ? load4(sky, f.w, px, py) : t4(0.0f, 0.0f, 0.0f, 0.0f));
                continue;
            }
            const T4 A = load4(im.albedo, f.w, px, py), E = load4(im.emissive, f.w, px, py);
            const float metallic = load4(im.geoNormal, f.w, px, py).w;
            f3 o, d;
            frame_ray(f, px, py, o, d);
            const f3 X = o + d * D.x;
            const Lighting s = make_surface(A, load4(im.normal, f.w, px, py), metallic, d);
            f3 totalD = mk3(0.0f, 0.0f, 0.0f), totalS = totalD;
            add_lights(s, X, sunDir, lights, 0u, lightCount,
                       [&](const HrptGPULight& l) { return sunRadiance ? xyz(load4(sunRadiance, f.w, px, py)) : light_color(l); },
                       [&](uint32_t j) { return visibility ? visibility[(size_t)j * WH + idx] : 1.0f; }, totalD, totalS);
            const T4 irr = (f.flags & HRPT_DEFERRED_INDIRECT) ? load4(im.indirect, f.w, px, py) : t4(0.0f, 0.0f, 0.0f, 0.0f);
            store4(out, finish_hit(f, A, E, metallic, totalD, totalS, irr));
        }
    });
}

} // namespace hrt

// pt_indirect_host.cpp -- the host-thread executors of traced indirect lighting (hrpt_indirect_rays_host / hrpt_indirect_resolve_host /
// hrpt_indirect_compose_host): pt_indirect.h's functions over the pixels of host images. Plain C++ with no HIP call, so that the sanitizer
// program (indirect_asan.cpp, `make indirect_asan`) builds it with g++ as it is.
#include <cstring>

#include "pt_indirect.h"
#include "pt_host_rows.h"

namespace hrt {

using namespace indirect;

bool indirect_params_valid(const HrptIndirectParams& params) { return params_valid(params); }

// One image row per "row": a pixel writes only its own records and texels, so the result does not depend on nthreads.
void indirect_rays_host(const HrptIndirectImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptIndirectParams& params,
                        HrptRay* raysOut, int nthreads)
{
    const Frame f = make_frame(cb, params, (int)width, (int)height);
    const size_t WH = (size_t)width * height;
    auto put = [](HrptRay* rec, const T4 rows[3]) {
        float* p = reinterpret_cast<float*>(rec);
        for (int r = 0; r < 3; ++r) store4(p + r * 4, rows[r]);
    };
    over_rows(f.h, nthreads, [&](int py) {
        for (int px = 0; px < f.w; ++px) {
            const size_t idx = (size_t)py * width + px;
            T4 rowsD[3], rowsS[3];
            pixel_rays(f, load4(im.albedo, f.w, px, py), load4(im.normal, f.w, px, py), load4(im.geoNormal, f.w, px, py).w, load4(im.depth, f.w, px, py), px, py,
                       rowsD, rowsS);
            if (f.flags & HRPT_INDIRECT_DIFFUSE) put(raysOut + idx, rowsD);
            if (f.flags & HRPT_INDIRECT_SPECULAR) put(raysOut + specular_base(f.flags, WH) + idx, rowsS);
        }
    });
}

void indirect_resolve_host(const HrptIndirectImages& im, uint32_t width, uint32_t height, const HrptPathTracerConstants& cb, const HrptIndirectParams& params,
                           const float* radiance4, int nthreads)
{
    const Frame f = make_frame(cb, params, (int)width, (int)height);
    const size_t WH = (size_t)width * height;
    const T4 zero = t4(0.0f, 0.0f, 0.0f, 0.0f);
    over_rows(f.h, nthreads, [&](int py) {
        for (int px = 0; px < f.w; ++px) {
            const size_t idx = (size_t)py * width + px;
            const T4 D = load4(im.depth, f.w, px, py);
            if (im.diffuse) store4(im.diffuse + idx * 4, (f.flags & HRPT_INDIRECT_DIFFUSE) ? resolve_diffuse(D, load4(radiance4, f.w, px, py)) : zero);
            if (im.specular) {
                T4 out = zero;
                if (f.flags & HRPT_INDIRECT_SPECULAR)
                    out = resolve_specular(f, load4(im.albedo, f.w, px, py), load4(im.normal, f.w, px, py), load4(im.geoNormal, f.w, px, py).w, D, px, py,
                                           load4(radiance4 + specular_base(f.flags, WH) * 4, f.w, px, py));
                store4(im.specular + idx * 4, out);
            }
        }
    });
}

void indirect_compose_host(const HrptIndirectImages& im, uint32_t width, uint32_t height, const HrptIndirectParams& params, int nthreads)
{
    const int w = (int)width;
    over_rows((int)height, nthreads, [&](int py) {
        for (int px = 0; px < w; ++px) {
            float* c = im.colorInOut + ((size_t)py * width + px) * 4;
            store4(c, compose(params.intensity, load4(im.colorInOut, w, px, py), load4(im.albedo, w, px, py), load4(im.geoNormal, w, px, py).w, load4(im.depth, w, px, py),
                              load4(im.diffuse, w, px, py), load4(im.specular, w, px, py)));
        }
    });
}

} // namespace hrt

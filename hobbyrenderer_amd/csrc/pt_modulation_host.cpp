// pt_modulation_host.cpp -- the host-thread executors of the demodulate and compose stages (hrpt_demodulate_host / hrpt_compose_host):
// pt_modulation.h's per-pixel functions over rows, the parameter rules and the probe of the factor. Plain C++ with no HIP call, so that the
// sanitizer program (modulation_asan.cpp, `make modulation_asan`) builds it with g++ as it is.
#include <cmath>

#include "pt_host_rows.h"
#include "pt_modulation.h"

namespace hrt {

bool modulation_params_valid(const HrptModulationParams& p)
{
    return std::isfinite(p.floor) && p.floor > 0.0f && p.flags == 0u && p.reserved[0] == 0u && p.reserved[1] == 0u;
}

namespace {
img::T3 emissive_at(const float* emissive, size_t i)
{
    return emissive ? img::t3(emissive[i], emissive[i + 1], emissive[i + 2]) : img::t3(0.0f, 0.0f, 0.0f);
}
} // namespace

// colorOut may be color (a pixel reads only its own colour texel and reads it before writing); modulationOut aliases nothing.
void demodulate_host(const HrptDemodulateImages& images, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                     const HrptModulationParams& params, int nthreads)
{
    const modulation::Args a = modulation::make_args(view, params, (int)width, (int)height);
    const int W = (int)width, H = (int)height;
    over_rows(H, nthreads, [&](int y) {
        for (int x = 0; x < W; ++x) {
            const size_t i = ((size_t)y * W + x) * 4;
            const img::T4 M = modulation::modulation_pixel(a, images.albedo, images.normal, images.geoNormal, images.depth, x, y);
            const img::T4 out = modulation::demodulate_color(img::load4(images.color, W, x, y), M, emissive_at(images.emissive, i));
            store4(images.modulationOut + i, M);
            store4(images.colorOut + i, out);
        }
    });
}

void compose_host(const HrptComposeImages& images, uint32_t width, uint32_t height, int nthreads)
{
    const int W = (int)width, H = (int)height;
    over_rows(H, nthreads, [&](int y) {
        for (int x = 0; x < W; ++x) {
            const size_t i = ((size_t)y * W + x) * 4;
            store4(images.colorOut + i, modulation::compose_color(img::load4(images.color, W, x, y), img::load4(images.modulation, W, x, y),
                                                                  emissive_at(images.emissive, i)));
        }
    });
}

void modulation_probe(const float* albedo3, const float* N3, const float* V3, float rough, float metal, float floor, float* outM3)
{
    const img::T3 m = modulation::factor(img::t3(albedo3[0], albedo3[1], albedo3[2]), img::t3(N3[0], N3[1], N3[2]),
                                         img::t3(V3[0], V3[1], V3[2]), rough, metal, floor);
    outM3[0] = m.x; outM3[1] = m.y; outM3[2] = m.z;
}

} // namespace hrt

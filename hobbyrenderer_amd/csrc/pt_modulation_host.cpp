// pt_modulation_host.cpp -- the host-thread executors of the demodulate and compose stages (hrpt_demodulate_host / hrpt_compose_host):
// pt_modulation.h's per-pixel functions over rows, the parameter rules and the probe of the factor. Plain C++ with no HIP call, so that the
// sanitizer program (modulation_asan.cpp, `make modulation_asan`) builds it with g++ as it is.
#include <cmath>
#include <thread>
#include <vector>

#include "pt_modulation.h"

namespace hrt {

bool modulation_params_valid(const HrptModulationParams& p)
{
    return std::isfinite(p.floor) && p.floor > 0.0f && p.flags == 0u && p.reserved[0] == 0u && p.reserved[1] == 0u;
}

namespace {
template <class Row> void over_rows(int H, int nthreads, Row row)
{
    if (nthreads > H) nthreads = H;
    if (nthreads <= 1) { for (int y = 0; y < H; ++y) row(y); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([=] { for (int y = t; y < H; y += nthreads) row(y); });
    for (auto& x : th) x.join();
}
temporal::T3 emissive_at(const float* emissive, size_t i)
{
    return emissive ? temporal::t3(emissive[i], emissive[i + 1], emissive[i + 2]) : temporal::t3(0.0f, 0.0f, 0.0f);
}
void store4(float* p, temporal::T4 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
} // namespace

// colorOut may be color (a pixel reads only its own colour texel and reads it before writing); modulationOut aliases nothing.
void demodulate_host(const HrptDemodulateImages& img, uint32_t width, uint32_t height, const HrptPlanarViewConstants& view,
                     const HrptModulationParams& params, int nthreads)
{
    const modulation::Args a = modulation::make_args(view, params, (int)width, (int)height);
    const int W = (int)width, H = (int)height;
    over_rows(H, nthreads, [&](int y) {
        for (int x = 0; x < W; ++x) {
            const size_t i = ((size_t)y * W + x) * 4;
            const temporal::T4 M = modulation::modulation_pixel(a, img.albedo, img.normal, img.geoNormal, img.depth, x, y);
            const temporal::T4 out = modulation::demodulate_color(temporal::load4(img.color, W, x, y), M, emissive_at(img.emissive, i));
            store4(img.modulationOut + i, M);
            store4(img.colorOut + i, out);
        }
    });
}

void compose_host(const HrptComposeImages& img, uint32_t width, uint32_t height, int nthreads)
{
    const int W = (int)width, H = (int)height;
    over_rows(H, nthreads, [&](int y) {
        for (int x = 0; x < W; ++x) {
            const size_t i = ((size_t)y * W + x) * 4;
            store4(img.colorOut + i, modulation::compose_color(temporal::load4(img.color, W, x, y), temporal::load4(img.modulation, W, x, y),
                                                               emissive_at(img.emissive, i)));
        }
    });
}

void modulation_probe(const float* albedo3, const float* N3, const float* V3, float rough, float metal, float floor, float* outM3)
{
    const temporal::T3 m = modulation::factor(temporal::t3(albedo3[0], albedo3[1], albedo3[2]), temporal::t3(N3[0], N3[1], N3[2]),
                                              temporal::t3(V3[0], V3[1], V3[2]), rough, metal, floor);
    outM3[0] = m.x; outM3[1] = m.y; outM3[2] = m.z;
}

} // namespace hrt

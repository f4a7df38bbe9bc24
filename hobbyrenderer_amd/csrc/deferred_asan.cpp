// deferred_asan.cpp -- driver of the sanitizer build of deferred lighting's host side (`make deferred_asan`: AddressSanitizer + UBSan, CPU
// only). Runs pt_deferred.h through deferred_rays_host and deferred_shade_host over exactly sized heap arrays: 1 x 1 to 64 x 36 images, 0 to 9
// lights of every type and of unknown types, ranges 0 and finite, lights on a surface point, misses, with and without the visibility,
// sun-radiance, sky and indirect images, light sub-ranges for the ray records, and hostile values (NaN, infinities, huge, denormal) in the
// planes, the lights and the constants. Any out-of-bounds access or other report ends the program with a non-zero status.
// usage: deferred_asan [seed]
#include "asan_common.h"
#include "pt_deferred.h"

namespace hrt {
void deferred_rays_host(const HrptDeferredImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                        uint32_t firstLight, uint32_t lightCount, HrptRay* raysOut);
void deferred_shade_host(const HrptDeferredImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                         uint32_t lightCount, const float* visibility, const float* sunRadiance, const float* sky, const HrptDeferredParams& params,
                         int nthreads);
bool deferred_params_valid(const HrptDeferredParams& params);
}

static int run(int w, int h, uint32_t lightCount, bool hostile)
{
    const size_t WH = (size_t)w * h;
    HrptPathTracerConstants cb;
    std::memset(&cb, 0, sizeof cb);
    cb.m_View = make_view(w, h);
    std::memcpy(cb.m_View.m_MatClipToWorldNoOffset, cb.m_View.m_MatClipToWorld, sizeof cb.m_View.m_MatClipToWorld);
    cb.m_Jitter[0] = 0.25f; cb.m_Jitter[1] = -0.125f;
    cb.m_SunDirection[0] = 0.3f; cb.m_SunDirection[1] = 0.8f; cb.m_SunDirection[2] = -0.52f;
    cb.m_LightCount = lightCount;
    std::vector<float> planes[9];          // albedo, normal, geoNormal, emissive, depth, indirect, sunRadiance, sky, out
    for (auto& p : planes) p.resize(WH * 4);
    for (size_t i = 0; i < WH; ++i) {
        float n[3] = { 2.0f * rnd() - 1.0f, 2.0f * rnd() - 1.0f, -rnd() - 0.1f };
        const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int c = 0; c < 3; ++c) {
            planes[0][i * 4 + c] = rnd(); planes[1][i * 4 + c] = n[c] / len; planes[2][i * 4 + c] = n[c] / len; planes[3][i * 4 + c] = rnd() < 0.1f ? 3.0f * rnd() : 0.0f;
            planes[5][i * 4 + c] = rnd(); planes[6][i * 4 + c] = 5.0f * rnd(); planes[7][i * 4 + c] = rnd();
        }
        planes[0][i * 4 + 3] = rnd(); planes[1][i * 4 + 3] = 0.04f + 0.96f * rnd(); planes[2][i * 4 + 3] = rnd() < 0.5f ? rnd() : 0.0f; planes[3][i * 4 + 3] = 1.0f;
        const bool miss = rnd() < 0.2f;
        planes[4][i * 4 + 0] = miss ? 1e10f : 1.0f + 4.0f * rnd(); planes[4][i * 4 + 1] = planes[4][i * 4 + 0];
        planes[5][i * 4 + 3] = rnd() < 0.8f ? 1.0f : 0.0f; planes[7][i * 4 + 3] = 1.0f;
        if (hostile && rnd() < 0.1f) planes[(int)(rnd() * 7.999f)][i * 4 + (int)(rnd() * 3.999f)] = kBad[(int)(rnd() * 7.999f)];
    }
    std::vector<HrptGPULight> lights(lightCount);
    for (uint32_t i = 0; i < lightCount; ++i) {
        HrptGPULight& l = lights[i];
        std::memset(&l, 0, sizeof l);
        l.m_Type = i % 5 == 4 ? 7u : i % 3;
        for (int c = 0; c < 3; ++c) { l.m_Position[c] = 4.0f * rnd() - 2.0f; l.m_Direction[c] = 2.0f * rnd() - 1.0f; l.m_Color[c] = rnd(); }
        l.m_Position[2] += 3.0f;
        l.m_Intensity = i % 7 == 6 ? 0.0f : 10.0f * rnd(); l.m_Range = i % 2 ? 6.0f : 0.0f;
        l.m_SpotInnerConeAngle = 0.3f; l.m_SpotOuterConeAngle = 0.9f; l.m_Radius = 0.1f;
        if (hostile && rnd() < 0.3f) reinterpret_cast<float*>(&l)[(int)(rnd() * 6.999f)] = kBad[(int)(rnd() * 7.999f)];
    }
    if (hostile) cb.m_Jitter[0] = kBad[(int)(rnd() * 7.999f)];
    std::vector<float> vis(WH * lightCount);
    for (float& v : vis) v = rnd() < 0.3f ? 0.0f : (rnd() < 0.5f ? 1.0f : rnd());
    HrptDeferredImages im;
    im.albedo = planes[0].data(); im.normal = planes[1].data(); im.geoNormal = planes[2].data(); im.emissive = planes[3].data(); im.depth = planes[4].data();
    im.indirect = planes[5].data(); im.colorOut = planes[8].data();
    int calls = 0;
    for (uint32_t first = 0; first <= lightCount; first += 4) {
        const uint32_t count = lightCount - first < 4u ? lightCount - first : 4u;
        std::vector<HrptRay> rays(WH * count);
        hrt::deferred_rays_host(im, (uint32_t)w, (uint32_t)h, cb, lights.data(), first, count, rays.data());
        ++calls;
    }
    for (int mode = 0; mode < 4; ++mode) {
        HrptDeferredParams p = { (mode & 1) ? HRPT_DEFERRED_INDIRECT : 0u, 0.7f, { 0u, 0u } };
        if (!hrt::deferred_params_valid(p)) { std::printf("deferred_asan: params refused\n"); std::exit(2); }
        HrptDeferredImages use = im;
        if (!(mode & 1)) use.indirect = nullptr;
        hrt::deferred_shade_host(use, (uint32_t)w, (uint32_t)h, cb, lights.data(), lightCount, (mode & 2) ? vis.data() : nullptr, (mode & 2) ? planes[6].data() : nullptr,
                                 (mode & 2) ? planes[7].data() : nullptr, p, 1 + mode);
        ++calls;
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    static const uint32_t kLights[4] = { 0, 1, 3, 9 };
    int calls = 0;
    for (const auto& s : kSizes)
        for (uint32_t n : kLights)
            for (int hostile = 0; hostile < 2; ++hostile) calls += run(s[0], s[1], n, hostile != 0);
    std::printf("deferred_asan: %d calls, no report\n", calls);
    return 0;
}

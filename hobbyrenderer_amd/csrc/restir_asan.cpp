// restir_asan.cpp -- driver of the sanitizer build of resampled direct lighting's host side (`make restir_asan`: AddressSanitizer + UBSan,
// CPU only). Runs pt_restir.h through the four host executors, chained as the context call chains them, over exactly sized heap arrays:
// 1 x 1 to 64 x 36 images, 0 to 70 lights of every type and of unknown types, misses, every flag, 1 and 32 candidates, 0 to 8 neighbours with
// radii from below one pixel to far beyond the image, with and without a history, and hostile values (NaN, infinities, huge, denormal; light
// indices outside the list) in the planes, the motion plane, the history, the lights and the constants. Any out-of-bounds access or other
// report ends the program with a non-zero status.
// usage: restir_asan [seed]
#include "asan_common.h"
#include "pt_restir.h"

namespace hrt {
bool restir_params_valid(const HrptRestirParams& params);
void restir_initial_host(const HrptRestirImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                         const HrptRestirParams& params, const float* sunRadiance, HrptRay* raysOut, int nthreads);
void restir_temporal_host(const HrptRestirImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                          const HrptRestirParams& params, const float* sunRadiance, const HrptRestirReservoir* initial, const float* initialVisibility, int nthreads);
void restir_spatial_host(const HrptRestirImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                         const HrptRestirParams& params, const float* sunRadiance, const HrptRestirReservoir* temporal, HrptRay* raysOut, int nthreads);
void restir_shade_host(const HrptRestirImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptGPULight* lights,
                       const HrptRestirParams& params, const float* sunRadiance, const float* sky, const HrptRestirReservoir* final, const float* visibility, int nthreads);
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
    std::vector<float> planes[11];          // albedo, normal, geoNormal, emissive, depth, motion, sunRadiance, sky, key in, key out, colour out
    for (auto& p : planes) p.resize(WH * 4);
    std::vector<HrptRestirReservoir> res[4];    // history, initial, temporal, final
    for (auto& r : res) r.resize(WH);
    for (size_t i = 0; i < WH; ++i) {
        float n[3] = { 2.0f * rnd() - 1.0f, 2.0f * rnd() - 1.0f, -rnd() - 0.1f };
        const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (int c = 0; c < 3; ++c) {
            planes[0][i * 4 + c] = rnd(); planes[1][i * 4 + c] = n[c] / len; planes[2][i * 4 + c] = n[c] / len; planes[3][i * 4 + c] = rnd() < 0.1f ? 3.0f * rnd() : 0.0f;
            planes[6][i * 4 + c] = 5.0f * rnd(); planes[7][i * 4 + c] = rnd(); planes[8][i * 4 + c] = rnd() < 0.7f ? n[c] / len : -n[c] / len;
        }
        planes[0][i * 4 + 3] = rnd(); planes[1][i * 4 + 3] = 0.04f + 0.96f * rnd(); planes[2][i * 4 + 3] = rnd() < 0.5f ? rnd() : 0.0f; planes[3][i * 4 + 3] = 1.0f;
        const bool miss = rnd() < 0.2f;
        planes[4][i * 4 + 0] = miss ? 1e10f : 1.0f + 4.0f * rnd(); planes[4][i * 4 + 1] = planes[4][i * 4 + 0];
        planes[5][i * 4 + 0] = rnd() < 0.5f ? 0.0f : 6.0f * rnd() - 3.0f; planes[5][i * 4 + 1] = rnd() < 0.5f ? 0.0f : 6.0f * rnd() - 3.0f;
        planes[5][i * 4 + 2] = 0.2f * rnd() - 0.1f; planes[5][i * 4 + 3] = rnd() < 0.9f ? 1.0f : 0.0f;
        planes[8][i * 4 + 3] = planes[4][i * 4 + 1];
        HrptRestirReservoir& r = res[0][i];
        r.light = rnd() < 0.1f ? HRPT_RESTIR_EMPTY : (uint32_t)(rnd() * (float)(lightCount + 2u));       // up to two past the list
        r.W = 2.0f * rnd(); r.M = 1.0f + 30.0f * rnd(); r.pHat = rnd();
        if (hostile && rnd() < 0.1f) planes[(int)(rnd() * 8.999f)][i * 4 + (int)(rnd() * 3.999f)] = kBad[(int)(rnd() * 7.999f)];
        if (hostile && rnd() < 0.1f) { r.light = hrt_f2u(kBad[(int)(rnd() * 7.999f)]); r.W = kBad[(int)(rnd() * 7.999f)]; r.M = kBad[(int)(rnd() * 7.999f)]; r.pHat = kBad[(int)(rnd() * 7.999f)]; }
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
    std::vector<float> vis(WH * 2);
    for (float& v : vis) v = rnd() < 0.3f ? 0.0f : (rnd() < 0.5f ? 1.0f : rnd());
    std::vector<HrptRay> rays(WH);
    static const float kRadii[4] = { 0.4f, 3.0f, 32.0f, 65535.0f };
    int calls = 0;
    for (int mode = 0; mode < 8; ++mode) {
        HrptRestirParams p;
        std::memset(&p, 0, sizeof p);
        p.flags = (mode & 1 ? HRPT_RESTIR_TEMPORAL | HRPT_RESTIR_INITIAL_VISIBILITY : 0u) | (mode & 2 ? HRPT_RESTIR_SPATIAL | HRPT_RESTIR_SHADOWS : 0u) | (mode & 4 ? HRPT_RESTIR_SKY : 0u) |
                  (mode == 7 ? HRPT_RESTIR_RESET : 0u);
        p.frameSeed = (uint32_t)(rnd() * 65536.0f); p.candidates = mode & 1 ? 32u : 1u; p.spatialSamples = (uint32_t)(mode & 2 ? 1 + (mode * 3) % 8 : 0);
        p.spatialRadius = kRadii[mode % 4]; p.maxHistory = 20.0f; p.depthThreshold = 0.1f; p.normalThreshold = mode & 4 ? -1.0f : 0.5f;
        if (!hrt::restir_params_valid(p)) { std::printf("restir_asan: params refused\n"); std::exit(2); }
        const float* sun = (mode & 4) ? planes[6].data() : nullptr;
        const bool history = (mode & 1) && mode != 5;
        HrptRestirImages im;
        std::memset(&im, 0, sizeof im);
        im.albedo = planes[0].data(); im.normal = planes[1].data(); im.geoNormal = planes[2].data(); im.emissive = planes[3].data(); im.depth = planes[4].data();
        im.motion = (mode & 1) ? planes[5].data() : nullptr;
        im.reservoirIn = history ? res[0].data() : nullptr; im.keyIn = history ? planes[8].data() : nullptr;
        im.keyOut = planes[9].data(); im.colorOut = planes[10].data();
        const int nthreads = 1 + mode;
        im.reservoirOut = res[1].data();
        hrt::restir_initial_host(im, (uint32_t)w, (uint32_t)h, cb, lights.data(), p, sun, (mode & 1) ? rays.data() : nullptr, nthreads);
        im.reservoirOut = res[2].data();
        hrt::restir_temporal_host(im, (uint32_t)w, (uint32_t)h, cb, lights.data(), p, sun, hostile && mode == 3 ? res[0].data() : res[1].data(), (mode & 1) ? vis.data() : nullptr, nthreads);
        im.reservoirOut = res[3].data();
        hrt::restir_spatial_host(im, (uint32_t)w, (uint32_t)h, cb, lights.data(), p, sun, hostile && mode == 6 ? res[0].data() : res[2].data(), (mode & 2) ? rays.data() : nullptr, nthreads);
        hrt::restir_shade_host(im, (uint32_t)w, (uint32_t)h, cb, lights.data(), p, sun, (mode & 4) ? planes[7].data() : nullptr, hostile && mode == 2 ? res[0].data() : res[3].data(),
                               (mode & 2) ? vis.data() + WH : nullptr, nthreads);
        calls += 4;
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    static const uint32_t kLights[4] = { 0, 1, 9, 70 };
    int calls = 0;
    for (const auto& s : kSizes)
        for (uint32_t n : kLights)
            for (int hostile = 0; hostile < 2; ++hostile) calls += run(s[0], s[1], n, hostile != 0);
    std::printf("restir_asan: %d calls, no report\n", calls);
    return 0;
}

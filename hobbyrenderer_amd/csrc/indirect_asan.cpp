// indirect_asan.cpp -- driver of the sanitizer build of traced indirect lighting's host side (`make indirect_asan`: AddressSanitizer +
// UBSan, CPU only). Runs pt_indirect.h through indirect_rays_host, indirect_resolve_host and indirect_compose_host over exactly sized heap
// arrays: 1 x 1 to 64 x 36 images, each lobe flag alone and both (so that the record arrays hold W * H or 2 * W * H entries), with and
// without the output plane of a lobe that is not flagged, misses, metallic 0 and 1, and hostile values (NaN, infinities, huge, denormal) in
// the planes, the radiance and the constants. Any out-of-bounds access or other report ends the program with a non-zero status.
// usage: indirect_asan [seed]
#include "asan_common.h"
#include "pt_indirect.h"

namespace hrt {
void indirect_rays_host(const HrptIndirectImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptIndirectParams& params,
                        HrptRay* raysOut, int nthreads);
void indirect_resolve_host(const HrptIndirectImages& images, uint32_t width, uint32_t height, const HrptPathTracerConstants& constants, const HrptIndirectParams& params,
                           const float* radiance4, int nthreads);
void indirect_compose_host(const HrptIndirectImages& images, uint32_t width, uint32_t height, const HrptIndirectParams& params, int nthreads);
bool indirect_params_valid(const HrptIndirectParams& params);
}

static int run(int w, int h, uint32_t flags, bool hostile)
{
    const size_t WH = (size_t)w * h;
    HrptPathTracerConstants cb;
    std::memset(&cb, 0, sizeof cb);
    cb.m_View = make_view(w, h);
    std::memcpy(cb.m_View.m_MatClipToWorldNoOffset, cb.m_View.m_MatClipToWorld, sizeof cb.m_View.m_MatClipToWorld);
    cb.m_Jitter[0] = 0.25f; cb.m_Jitter[1] = -0.125f;
    std::vector<float> planes[7];          // albedo, normal, geoNormal, depth, diffuse, specular, colour
    for (auto& p : planes) p.resize(WH * 4);
    for (size_t i = 0; i < WH; ++i) {
        float n[3] = { 2.0f * rnd() - 1.0f, 2.0f * rnd() - 1.0f, 2.0f * rnd() - 1.0f };
        const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) + 1e-6f;
        for (int c = 0; c < 3; ++c) { planes[0][i * 4 + c] = rnd(); planes[1][i * 4 + c] = n[c] / len; planes[2][i * 4 + c] = n[c] / len; planes[6][i * 4 + c] = 2.0f * rnd(); }
        const float m = rnd();
        planes[0][i * 4 + 3] = rnd(); planes[1][i * 4 + 3] = 0.04f + 0.96f * rnd(); planes[2][i * 4 + 3] = m < 0.3f ? 0.0f : (m < 0.6f ? 1.0f : rnd()); planes[6][i * 4 + 3] = 1.0f;
        const bool miss = rnd() < 0.2f;
        planes[3][i * 4 + 0] = miss ? 1e10f : 1.0f + 4.0f * rnd(); planes[3][i * 4 + 1] = planes[3][i * 4 + 0];
        if (hostile && rnd() < 0.1f) planes[(int)(rnd() * 3.999f)][i * 4 + (int)(rnd() * 3.999f)] = kBad[(int)(rnd() * 7.999f)];
    }
    if (hostile) cb.m_Jitter[0] = kBad[(int)(rnd() * 7.999f)];
    const HrptIndirectParams p = { flags, (uint32_t)(rnd() * 65535.0f), 0.7f, 0u };
    if (!hrt::indirect_params_valid(p)) { std::printf("indirect_asan: params refused\n"); std::exit(2); }
    const size_t records = hrt::indirect::record_count(flags, WH);
    std::vector<HrptRay> rays(records);
    std::vector<float> radiance(records * 4);
    for (size_t i = 0; i < records; ++i) {
        for (int c = 0; c < 3; ++c) radiance[i * 4 + c] = 3.0f * rnd();
        radiance[i * 4 + 3] = rnd() < 0.7f ? 1.0f : 0.0f;
        if (hostile && rnd() < 0.1f) radiance[i * 4 + (int)(rnd() * 3.999f)] = kBad[(int)(rnd() * 7.999f)];
    }
    HrptIndirectImages im;
    std::memset(&im, 0, sizeof im);
    im.albedo = planes[0].data(); im.normal = planes[1].data(); im.geoNormal = planes[2].data(); im.depth = planes[3].data();
    im.diffuse = planes[4].data(); im.specular = planes[5].data(); im.colorInOut = planes[6].data();
    int calls = 0;
    for (int threads = 1; threads <= 3; threads += 2) {
        hrt::indirect_rays_host(im, (uint32_t)w, (uint32_t)h, cb, p, rays.data(), threads);
        hrt::indirect_resolve_host(im, (uint32_t)w, (uint32_t)h, cb, p, radiance.data(), threads);
        HrptIndirectImages flagged = im;          // only the planes of the flagged lobes
        if (!(flags & HRPT_INDIRECT_DIFFUSE)) flagged.diffuse = nullptr;
        if (!(flags & HRPT_INDIRECT_SPECULAR)) flagged.specular = nullptr;
        hrt::indirect_resolve_host(flagged, (uint32_t)w, (uint32_t)h, cb, p, radiance.data(), threads);
        hrt::indirect_compose_host(im, (uint32_t)w, (uint32_t)h, p, threads);
        calls += 4;
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    int calls = 0;
    for (const auto& s : kSizes)
        for (uint32_t flags = 1; flags <= 3; ++flags)
            for (int hostile = 0; hostile < 2; ++hostile) calls += run(s[0], s[1], flags, hostile != 0);
    std::printf("indirect_asan: %d calls, no report\n", calls);
    return 0;
}

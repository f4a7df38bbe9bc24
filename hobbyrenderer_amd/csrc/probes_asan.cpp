// probes_asan.cpp -- driver of the sanitizer build of the probe volume's host side (`make probes_asan`: AddressSanitizer + UBSan, CPU only).
// Runs pt_probes.h through probes_rays_host, probes_blend_host and probes_query_host over exactly sized heap arrays: grids with one probe
// per axis and more, 1 to 1024 rays, misses, untraced rays, probes without a traced ray, hostile radiance and hit distances, with and without
// history; then queries on probes, between them, far outside the grid, with zero normals and hostile coordinates, against the blended
// atlases and against atlases filled with hostile values. Any out-of-bounds access, undefined float -> int conversion or other report ends
// the program with a non-zero status.
// usage: probes_asan [seed]
#include "asan_common.h"
#include "pt_probes.h"

namespace hrt {
void probes_rays_host(const HrptProbeVolume& volume, uint32_t frameSeed, HrptRay* raysOut, float* directions4Out);
void probes_blend_host(const HrptProbeVolume& volume, const float* directions4, const float* radiance4, const HrptRayHit* hits, float* irradiance,
                       float* distance, bool hasHistory, int nthreads);
void probes_query_host(const HrptProbeVolume& volume, const float* irradiance, const float* distance, const HrptProbePoint* points, float* out4,
                       uint64_t count, int nthreads);
bool probes_volume_valid(const HrptProbeVolume& volume);
}

static int run(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t N, float exponent, bool hostile)
{
    HrptProbeVolume v;
    std::memset(&v, 0, sizeof v);
    v.origin[0] = -1.0f; v.origin[1] = 0.5f; v.origin[2] = -2.0f; v.hysteresis = 0.9f;
    v.spacing[0] = 1.0f; v.spacing[1] = 0.75f; v.spacing[2] = 1.5f; v.maxRayDistance = 3.0f;
    v.counts[0] = cx; v.counts[1] = cy; v.counts[2] = cz; v.raysPerProbe = N;
    v.distanceExponent = exponent; v.normalBias = 0.1f; v.viewBias = 0.05f;
    if (!hrt::probes_volume_valid(v)) { std::printf("probes_asan: volume refused\n"); std::exit(2); }
    const size_t P = (size_t)cx * cy * cz, R = P * N;
    std::vector<HrptRay> rays(R);
    std::vector<float> dirs((size_t)N * 4), radiance(R * 4), irr(P * hrt::probes::kIrrFloats), dist(P * hrt::probes::kDistFloats);
    std::vector<HrptRayHit> hits(R);
    int calls = 0;
    for (uint32_t frame = 0; frame < 3; ++frame) {
        hrt::probes_rays_host(v, 17u + frame, rays.data(), dirs.data());
        for (size_t g = 0; g < R; ++g) {
            std::memset(&hits[g], 0, sizeof hits[g]);
            const bool untraced = g / N == 1 || rnd() < 0.05f;       // probe 1: no traced ray at all
            for (int c = 0; c < 3; ++c) radiance[g * 4 + c] = 4.0f * rnd();
            radiance[g * 4 + 3] = untraced ? 0.0f : 1.0f;
            hits[g].hit = rnd() < 0.8f; hits[g].t = 6.0f * rnd();
            if (hostile && rnd() < 0.1f) {
                if (rnd() < 0.5f) radiance[g * 4 + (int)(rnd() * 2.999f)] = kBad[(int)(rnd() * 7.999f)];
                else hits[g].t = kBad[(int)(rnd() * 7.999f)];
            }
        }
        hrt::probes_blend_host(v, dirs.data(), radiance.data(), hits.data(), irr.data(), dist.data(), frame > 0, 1 + (int)(frame % 3));
        ++calls;
        const size_t Q = 257;
        std::vector<HrptProbePoint> pts(Q);
        std::vector<float> out(Q * 4);
        for (int pass = 0; pass < (hostile ? 2 : 1); ++pass) {
            for (size_t i = 0; i < Q; ++i) {
                HrptProbePoint& q = pts[i];
                std::memset(&q, 0, sizeof q);
                const float reach = i % 5 == 0 ? 1e6f : 4.0f;
                for (int c = 0; c < 3; ++c) {
                    q.position[c] = i % 7 == 0 ? v.origin[c] + (float)(i % (c == 0 ? cx : (c == 1 ? cy : cz))) * v.spacing[c] : (2.0f * rnd() - 1.0f) * reach;
                    q.normal[c] = i % 11 == 0 ? 0.0f : 2.0f * rnd() - 1.0f;
                    q.view[c] = 2.0f * rnd() - 1.0f;
                }
                if (i % 11 != 0) {
                    const float len = std::sqrt(q.normal[0] * q.normal[0] + q.normal[1] * q.normal[1] + q.normal[2] * q.normal[2]);
                    if (len > 0.0f) for (int c = 0; c < 3; ++c) q.normal[c] /= len;
                }
                if (hostile && rnd() < 0.2f) reinterpret_cast<float*>(&q)[(int)(rnd() * 11.999f)] = kBad[(int)(rnd() * 7.999f)];
            }
            hrt::probes_query_host(v, irr.data(), dist.data(), pts.data(), out.data(), Q, 1 + pass);
            ++calls;
            if (pass == 0 && hostile)       // second pass, and the next frame's blend: atlases with hostile texels
                for (size_t i = 0; i < dist.size(); i += 13) if (rnd() < 0.3f) dist[i] = kBad[(int)(rnd() * 7.999f)];
        }
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    static const uint32_t kGrids[4][3] = { { 1, 1, 1 }, { 3, 2, 2 }, { 2, 1, 5 }, { 1, 4, 1 } };
    static const uint32_t kRays[5] = { 1, 32, 100, 257, 1024 };
    int calls = 0;
    for (const auto& g : kGrids)
        for (uint32_t n : kRays)
            for (int hostile = 0; hostile < 2; ++hostile)
                calls += run(g[0], g[1], g[2], n, n == 100 ? 50.0f : 1.0f, hostile != 0);
    std::printf("probes_asan: %d calls, no report\n", calls);
    return 0;
}

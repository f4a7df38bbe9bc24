// pt_probes_host.cpp -- the host-thread executors of the irradiance probe volume (hrpt_probes_rays_host / _blend_host / _query_host):
// pt_probes.h's functions over the records, the probes and the points, and the volume rule. Plain C++ with no HIP call, so that the
// sanitizer program (probes_asan.cpp, `make probes_asan`) builds it with g++ as it is.
#include <cstring>

#include "pt_host_rows.h"
#include "pt_probes.h"

namespace hrt {

using namespace probes;

bool probes_volume_valid(const HrptProbeVolume& volume) { return volume_valid(volume); }

void probes_rays_host(const HrptProbeVolume& vol, uint32_t frameSeed, HrptRay* raysOut, float* directions4Out)
{
    const uint32_t P = probe_count(vol), N = vol.raysPerProbe;
    const Rotation R = frame_rotation(frameSeed);
    std::vector<T3> dirs(N);
    for (uint32_t k = 0; k < N; ++k) {
        dirs[k] = ray_direction(R, k, N);
        if (directions4Out) { float* d = directions4Out + (size_t)k * 4; d[0] = dirs[k].x; d[1] = dirs[k].y; d[2] = dirs[k].z; d[3] = 0.0f; }
    }
    if (!raysOut) return;
    for (uint32_t p = 0; p < P; ++p) {
        const T3 o = probe_position(vol, p);
        for (uint32_t k = 0; k < N; ++k) {
            const uint32_t g = p * N + k;
            HrptRay& r = raysOut[g];
            std::memset(&r, 0, sizeof r);
            r.origin[0] = o.x; r.origin[1] = o.y; r.origin[2] = o.z; r.tmin = 0.0f;
            r.direction[0] = dirs[k].x; r.direction[1] = dirs[k].y; r.direction[2] = dirs[k].z; r.tmax = kRayTmax;
            r.rng = ray_rng(g, frameSeed);
        }
    }
}

// One probe per "row": a probe writes only its own two tiles, so the result does not depend on nthreads. The order inside a probe is the
// kernel's: every interior texel is blended against the old interior texel first, the borders are copied afterwards.
void probes_blend_host(const HrptProbeVolume& vol, const float* directions4, const float* radiance4, const HrptRayHit* hits, float* irradiance,
                       float* distance, bool hasHistory, int nthreads)
{
    const uint32_t N = vol.raysPerProbe;
    over_rows((int)probe_count(vol), nthreads, [&](int p) {
        std::vector<float> staged((size_t)N * 4);
        for (uint32_t k = 0; k < N; ++k) {
            const size_t g = (size_t)p * N + k;
            const T4 s = staged_ray(radiance4 + g * 4, hits[g].hit, hits[g].t, vol.maxRayDistance);
            store4(&staged[(size_t)k * 4], s);
        }
        float* irrTile = irradiance + (size_t)p * kIrrFloats;
        float* distTile = distance + (size_t)p * kDistFloats;
        for (int tj = 0; tj < kDistInterior; ++tj)
            for (int ti = 0; ti < kDistInterior; ++ti) {
                const T3 n = texel_direction(ti, tj, kDistInterior);
                DistSums s = { 0.0f, 0.0f, 0.0f };
                for (uint32_t k = 0; k < N; ++k) dist_add(&s, n, directions4 + (size_t)k * 4, &staged[(size_t)k * 4], vol.distanceExponent);
                float* t = distTile + ((tj + 1) * kDistTile + (ti + 1)) * 2;
                const T2 v = dist_texel(s, t2(t[0], t[1]), vol.hysteresis, hasHistory);
                t[0] = v.x; t[1] = v.y;
            }
        for (int tj = 0; tj < kIrrInterior; ++tj)
            for (int ti = 0; ti < kIrrInterior; ++ti) {
                const T3 n = texel_direction(ti, tj, kIrrInterior);
                IrrSums s = { 0.0f, 0.0f, 0.0f, 0.0f };
                for (uint32_t k = 0; k < N; ++k) irr_add(&s, n, directions4 + (size_t)k * 4, &staged[(size_t)k * 4]);
                float* t = irrTile + ((tj + 1) * kIrrTile + (ti + 1)) * 4;
                store4(t, irr_texel(s, t4(t[0], t[1], t[2], t[3]), vol.hysteresis, hasHistory));
            }
        for (int y = 0; y < kDistTile; ++y)
            for (int x = 0; x < kDistTile; ++x) {
                int sx, sy;
                border_source(x, y, kDistTile, &sx, &sy);
                if (sx != x || sy != y) std::memcpy(distTile + (y * kDistTile + x) * 2, distTile + (sy * kDistTile + sx) * 2, 8);
            }
        for (int y = 0; y < kIrrTile; ++y)
            for (int x = 0; x < kIrrTile; ++x) {
                int sx, sy;
                border_source(x, y, kIrrTile, &sx, &sy);
                if (sx != x || sy != y) std::memcpy(irrTile + (y * kIrrTile + x) * 4, irrTile + (sy * kIrrTile + sx) * 4, 16);
            }
    });
}

void probes_query_host(const HrptProbeVolume& vol, const float* irradiance, const float* distance, const HrptProbePoint* points, float* out4,
                       uint64_t count, int nthreads)
{
    constexpr uint64_t kChunk = 1024;
    over_rows((int)((count + kChunk - 1) / kChunk), nthreads, [&](int c) {
        const uint64_t end = ((uint64_t)c + 1) * kChunk < count ? ((uint64_t)c + 1) * kChunk : count;
        for (uint64_t i = (uint64_t)c * kChunk; i < end; ++i) {
            const HrptProbePoint& q = points[i];
            store4(out4 + i * 4, query(vol, irradiance, distance, t3(q.position[0], q.position[1], q.position[2]), t3(q.normal[0], q.normal[1], q.normal[2]),
                                       t3(q.view[0], q.view[1], q.view[2])));
        }
    });
}

} // namespace hrt

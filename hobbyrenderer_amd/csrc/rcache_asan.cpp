// rcache_asan.cpp -- driver of the sanitizer build of the radiance cache's host side (`make rcache_asan`: AddressSanitizer + UBSan, CPU only).
// Runs pt_rcache.h through rcache_insert_host, rcache_resolve_host, rcache_query_host and rcache_table_fault over exactly sized heap arrays,
// chained as hrpt_rcache_update chains them for several frames: tables of 2^10 and 2^12 entries, 0 to 4096 samples from 1 to 16 threads, few
// keys (every sample in one voxel) and many (full buckets, drops), short ageing so that entries are evicted and buckets compacted, hostile
// positions, normals, radiance and camera distances, and queries against tables whose resolved records were overwritten with hostile
// values. Any out-of-bounds access, undefined float -> int conversion or shift, or other report ends the program with a non-zero status.
// usage: rcache_asan [seed]
#include "asan_common.h"
#include "pt_rcache.h"

namespace hrt {
bool rcache_desc_valid(const HrptRcacheDesc& desc);
void rcache_insert_host(const HrptRcacheDesc& desc, const float* cameraPos, uint64_t* keys, HrptRcacheAccum* accum, uint64_t* drops, const HrptRcacheSample* samples,
                        uint64_t count, int nthreads);
void rcache_resolve_host(const HrptRcacheDesc& desc, uint64_t* keys, HrptRcacheAccum* accum, HrptRcacheEntry* resolved, int nthreads);
void rcache_query_host(const HrptRcacheDesc& desc, const float* cameraPos, const uint64_t* keys, const HrptRcacheEntry* resolved, const HrptRcachePoint* points,
                       float* out4, float* voxelOut, uint64_t count, int nthreads);
const char* rcache_table_fault(const HrptRcacheDesc& desc, const uint64_t* keys, const HrptRcacheAccum* accum, const HrptRcacheEntry* resolved);
}

static int run(uint32_t capacityLog2, size_t count, float spread, float levelBias, bool hostile)
{
    HrptRcacheDesc d;
    std::memset(&d, 0, sizeof d);
    d.capacityLog2 = capacityLog2; d.sceneScale = 50.0f; d.levelBias = levelBias; d.radianceScale = 1e3f;
    d.maxSamples = 4; d.staleFramesMax = 1; d.sparseBlock = 5; d.roughnessThreshold = 0.1f;
    if (!hrt::rcache_desc_valid(d)) { std::printf("rcache_asan: desc refused\n"); std::exit(2); }
    const size_t n = (size_t)1 << capacityLog2;
    std::vector<uint64_t> keys(n, 0);
    std::vector<HrptRcacheAccum> accum(n);
    std::vector<HrptRcacheEntry> resolved(n);
    std::memset(accum.data(), 0, n * sizeof(HrptRcacheAccum));
    std::memset(resolved.data(), 0, n * sizeof(HrptRcacheEntry));
    const float cam[3] = { 0.5f, -1.0f, 2.0f };
    uint64_t drops = 0;
    int calls = 0;
    for (int frame = 0; frame < 5; ++frame) {
        const size_t m = frame == 3 ? 0 : count;                      // one frame without samples: ageing alone
        std::vector<HrptRcacheSample> samples(m);
        for (size_t i = 0; i < m; ++i) {
            HrptRcacheSample& s = samples[i];
            std::memset(&s, 0, sizeof s);
            s.valid = rnd() < 0.9f ? 1.0f : 0.0f;
            for (int c = 0; c < 3; ++c) {
                s.position[c] = cam[c] + (2.0f * rnd() - 1.0f) * spread * (float)(1 + frame % 2);
                s.normal[c] = 2.0f * rnd() - 1.0f;
                s.radiance[c] = 8.0f * rnd();
            }
            if (hostile && rnd() < 0.2f) reinterpret_cast<float*>(&s)[(int)(rnd() * 11.999f)] = rnd() < 0.5f ? kBad[(int)(rnd() * 7.999f)] : 1e30f * (rnd() - 0.5f);
        }
        hrt::rcache_insert_host(d, cam, keys.data(), accum.data(), &drops, samples.data(), m, 1 + frame * 5);
        hrt::rcache_resolve_host(d, keys.data(), accum.data(), resolved.data(), 1 + frame);
        if (const char* fault = hrt::rcache_table_fault(d, keys.data(), accum.data(), resolved.data())) { std::printf("rcache_asan: %s\n", fault); std::exit(3); }
        const size_t Q = 257;
        std::vector<HrptRcachePoint> pts(Q);
        std::vector<float> out(Q * 4), voxel(Q);
        for (int pass = 0; pass < (hostile ? 2 : 1); ++pass) {
            for (size_t i = 0; i < Q; ++i) {
                HrptRcachePoint& q = pts[i];
                std::memset(&q, 0, sizeof q);
                const bool known = m > 0 && i % 2 == 0;
                for (int c = 0; c < 3; ++c) {
                    q.position[c] = known ? samples[i % m].position[c] : cam[c] + (2.0f * rnd() - 1.0f) * (i % 5 == 0 ? 1e6f : spread);
                    q.normal[c] = known ? samples[i % m].normal[c] : 2.0f * rnd() - 1.0f;
                }
                if (hostile && rnd() < 0.2f) reinterpret_cast<float*>(&q)[(int)(rnd() * 7.999f)] = kBad[(int)(rnd() * 7.999f)];
            }
            hrt::rcache_query_host(d, cam, keys.data(), resolved.data(), pts.data(), out.data(), pass ? nullptr : voxel.data(), Q, 1 + pass * 3);
            if (pass == 0 && hostile) {                                // second pass, and the next frame's resolve: hostile resolved records
                std::vector<HrptRcacheEntry> saved = resolved;
                for (size_t i = 0; i < n; i += 7) if (keys[i] != 0 && rnd() < 0.5f) { resolved[i].r = kBad[(int)(rnd() * 7.999f)]; resolved[i].meta = 0xFFFFFFFFu; }
                hrt::rcache_query_host(d, cam, keys.data(), resolved.data(), pts.data(), out.data(), voxel.data(), Q, 2);
                if (frame % 2) resolved = saved;
                ++calls;
            }
            ++calls;
        }
        calls += 2;
    }
    return calls;
}

int main(int argc, char** argv)
{
    seed_from(argc, argv);
    static const size_t kCounts[6] = { 0, 1, 63, 64, 65, 4096 };
    int calls = 0;
    for (uint32_t capacityLog2 : { 10u, 12u })
        for (size_t count : kCounts)
            for (int hostile = 0; hostile < 2; ++hostile) {
                calls += run(capacityLog2, count, 0.01f, 0.0f, hostile != 0);       // one voxel: every sample on a few keys
                calls += run(capacityLog2, count, 40.0f, 3.0f, hostile != 0);       // many keys: full buckets at 2^10
            }
    std::printf("rcache_asan: %d calls, no report\n", calls);
    return 0;
}

// pt_rcache_host.cpp -- the host-thread executors of the hash-grid radiance cache (hrpt_rcache_insert_host / _resolve_host / _query_host),
// the desc rule and the invariant check of hrpt_rcache_write: pt_rcache.h's functions over the samples, the buckets and the points. Plain
// C++ with no HIP call, so that the sanitizer program (rcache_asan.cpp, `make rcache_asan`) builds it with g++ as it is.
#include <cstring>

#include "pt_host_rows.h"
#include "pt_rcache.h"

namespace hrt {

using namespace rcache;

bool rcache_desc_valid(const HrptRcacheDesc& desc) { return desc_valid(desc); }

namespace {
struct HostAtomics {
    uint64_t load(uint64_t* p) const { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    uint64_t cas(uint64_t* p, uint64_t expected, uint64_t desired) const
    {
        __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expected;                         // the value found: `expected` is rewritten on failure and was it on success
    }
};
constexpr uint64_t kChunk = 1024;
template <class F> void over_chunks(uint64_t count, int nthreads, F f)
{
    over_rows((int)((count + kChunk - 1) / kChunk), nthreads, [&](int c) {
        const uint64_t end = ((uint64_t)c + 1) * kChunk < count ? ((uint64_t)c + 1) * kChunk : count;
        for (uint64_t i = (uint64_t)c * kChunk; i < end; ++i) f(i);
    });
}
} // namespace

// The per-sample form of the kernel: the same walk and the same integer adds, from as many threads as asked for. Which slot a key lands in
// depends on the threads' order; the sums do not.
void rcache_insert_host(const HrptRcacheDesc& d, const float* cam, uint64_t* keys, HrptRcacheAccum* accum, uint64_t* drops, const HrptRcacheSample* samples,
                        uint64_t count, int nthreads)
{
    over_chunks(count, nthreads, [&](uint64_t i) {
        const HrptRcacheSample& s = samples[i];
        if (!sample_used(s)) return;
        const uint64_t key = key_of(d, s.position, s.normal, cam, nullptr);
        const uint64_t base = bucket_base(key, d.capacityLog2);
        const int slot = claim_slot(HostAtomics(), keys, base, key);
        if (slot < 0) { __atomic_fetch_add(drops, 1ull, __ATOMIC_RELAXED); return; }
        HrptRcacheAccum& a = accum[base + (uint64_t)slot];
        __atomic_fetch_add(&a.r, quantise(s.radiance[0], d.radianceScale), __ATOMIC_RELAXED);
        __atomic_fetch_add(&a.g, quantise(s.radiance[1], d.radianceScale), __ATOMIC_RELAXED);
        __atomic_fetch_add(&a.b, quantise(s.radiance[2], d.radianceScale), __ATOMIC_RELAXED);
        __atomic_fetch_add(&a.count, 1u, __ATOMIC_RELAXED);
    });
}

// One bucket per "row": a bucket writes only its own 32 entries, so the result does not depend on nthreads.
void rcache_resolve_host(const HrptRcacheDesc& d, uint64_t* keys, HrptRcacheAccum* accum, HrptRcacheEntry* resolved, int nthreads)
{
    over_rows((int)(capacity(d) / kBucket), nthreads, [&](int bucket) {
        const uint64_t base = (uint64_t)bucket * kBucket;
        uint32_t out = 0;
        for (uint32_t l = 0; l < kBucket; ++l) {
            const uint64_t key = keys[base + l];
            HrptRcacheEntry e = resolved[base + l];
            const bool survive = key != 0ull && resolve_entry(d, accum[base + l], e);
            std::memset(&accum[base + l], 0, sizeof(HrptRcacheAccum));
            if (survive) { keys[base + out] = key; resolved[base + out] = e; ++out; }      // out <= l: nothing unread is overwritten
        }
        for (uint32_t l = out; l < kBucket; ++l) { keys[base + l] = 0ull; std::memset(&resolved[base + l], 0, sizeof(HrptRcacheEntry)); }
    });
}

void rcache_query_host(const HrptRcacheDesc& d, const float* cam, const uint64_t* keys, const HrptRcacheEntry* resolved, const HrptRcachePoint* points, float* out4,
                       float* voxelOut, uint64_t count, int nthreads)
{
    over_chunks(count, nthreads, [&](uint64_t i) { query(d, cam, keys, resolved, points[i], out4 + i * 4, voxelOut ? voxelOut + i : nullptr); });
}

const char* rcache_table_fault(const HrptRcacheDesc& d, const uint64_t* keys, const HrptRcacheAccum* accum, const HrptRcacheEntry* resolved)
{
    static const HrptRcacheAccum zeroA = {};
    static const HrptRcacheEntry zeroE = {};
    for (uint64_t base = 0; base < capacity(d); base += kBucket) {
        bool empty = false;
        for (uint32_t l = 0; l < kBucket; ++l) {
            const uint64_t key = keys[base + l];
            if (key == 0ull) {
                empty = true;
                if (std::memcmp(&accum[base + l], &zeroA, sizeof zeroA) != 0 || std::memcmp(&resolved[base + l], &zeroE, sizeof zeroE) != 0)
                    return "an empty slot's records are not zero";
                continue;
            }
            if (empty) return "an empty slot precedes an occupied one";
            if (bucket_base(key, d.capacityLog2) != base) return "a key sits outside its bucket";
            for (uint32_t k = 0; k < l; ++k)
                if (keys[base + k] == key) return "a key appears twice";
        }
    }
    return nullptr;
}

} // namespace hrt

// pt_rcache.h -- the arithmetic of the world-space hash-grid radiance cache (hrpt_rcache_*), one __host__ __device__ source shared by the
// gfx950 kernels (pt_rcache.hip) and the host executors (pt_rcache_host.cpp): the counterpart of the reference's SHARCUpdate.hlsl,
// SharcResolve.hlsl and SHARCQuery.hlsl. The SDK headers behind those shaders (SharcCommon.h, HashGridCommon.h) are not in the reference tree,
// so the stage is DEFINED here after the published description; DESIGN.md section 32 has every operation in order. In the arithmetic of
// hobbyrt/detmath.h: no FMA contraction, correctly rounded '/', select-form min / max, sums left to right.
//
// Unlike the reference there is no four-vertex back-propagation stack and no cache resampling: the value stored for a voxel is the path
// tracer's full estimate along the ray that landed in it (hrpt_trace_radiance), so the cache has no feedback from its own last state and
// needs no energy clamp.
//
// The table: `capacity` = 2^capacityLog2 entries in three arrays -- keys (uint64, 0 = empty), accumulation (HrptRcacheAccum, 32 B: integer
// sums of one frame) and resolved (HrptRcacheEntry, 16 B: the running mean, samples in the low and stale frames in the high 16 bits of meta).
//   level = clamp(floor(0.5 * log2(max(|p - camera|^2, FLT_MIN)) + levelBias), 1, 1023)
//   voxel = exp2(level) / (sceneScale * exp2(levelBias))
//   grid  = floor(p / voxel) per component, clamped to the int32 range, the low 17 bits kept (two's complement, wrapped)
//   key   = gx | gy << 17 | gz << 34 | level << 51 | octant << 61, octant bit c = (n.c >= 0)            (never 0: level >= 1)
//   bucket = 32 consecutive entries at (pcg(lo(key) + pcg(hi(key))) mod (capacity / 32)) * 32
// INVARIANT: the occupied slots of a bucket are a prefix of it. insert relies on it, resolve restores it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/hobbyrt_pt.h"
#include "../../include/hobbyrt/detmath.h"

namespace hrt {
namespace rcache {

constexpr uint32_t kBucket = 32u;
constexpr float kTiny = 1.17549435e-38f;            // FLT_MIN
constexpr float kChannelMax = 4294967040.0f;        // the largest binary32 below 2^32
constexpr uint32_t kUpdateFlags = HRPT_RCACHE_RESET | HRPT_RCACHE_NO_WAVE_COMBINE;

HRT_FN bool finite1(float x) { return (x - x) == 0.0f; }
HRT_FN bool finite3(const float* v) { return finite1(v[0]) && finite1(v[1]) && finite1(v[2]); }

HRT_FN bool desc_valid(const HrptRcacheDesc& d)
{
    return d.capacityLog2 >= 10u && d.capacityLog2 <= 26u && finite1(d.sceneScale) && d.sceneScale > 0.0f && finite1(d.levelBias) && d.levelBias >= -64.0f &&
           d.levelBias <= 64.0f && finite1(d.radianceScale) && d.radianceScale > 0.0f && d.maxSamples >= 1u && d.maxSamples <= 65535u &&
           d.staleFramesMax <= 65534u && d.sparseBlock >= 1u && d.sparseBlock <= 16u && finite1(d.roughnessThreshold);
}
HRT_FN uint64_t capacity(const HrptRcacheDesc& d) { return 1ull << d.capacityLog2; }

// ---- the key ------------------------------------------------------------------------------------------------------------------------------
HRT_FN uint32_t level_of(const HrptRcacheDesc& d, const float* p, const float* cam)
{
    const float dx = p[0] - cam[0], dy = p[1] - cam[1], dz = p[2] - cam[2];
    const float d2 = hrt_max((dx * dx + dy * dy) + dz * dz, kTiny);
    return (uint32_t)hrt_clamp(hrt_floor(0.5f * hrt_log2(d2) + d.levelBias), 1.0f, 1023.0f);
}
HRT_FN float voxel_of(const HrptRcacheDesc& d, uint32_t level) { return hrt_exp2((float)level) / (d.sceneScale * hrt_exp2(d.levelBias)); }
HRT_FN uint64_t grid17(float p, float voxel)
{
    const float g = hrt_clamp(hrt_floor(p / voxel), -2147483648.0f, 2147483520.0f);      // NaN (0 / 0, inf / inf) converts as -2^31
    return (uint64_t)((uint32_t)(int32_t)g & 0x1FFFFu);
}
// Key and voxel size of a finite point and normal.
HRT_FN uint64_t key_of(const HrptRcacheDesc& d, const float* p, const float* n, const float* cam, float* voxelOut)
{
    const uint32_t level = level_of(d, p, cam);
    const float voxel = voxel_of(d, level);
    if (voxelOut) *voxelOut = voxel;
    const uint64_t octant = (n[0] >= 0.0f ? 1u : 0u) | (n[1] >= 0.0f ? 2u : 0u) | (n[2] >= 0.0f ? 4u : 0u);
    return grid17(p[0], voxel) | grid17(p[1], voxel) << 17 | grid17(p[2], voxel) << 34 | (uint64_t)level << 51 | octant << 61;
}
HRT_FN uint64_t bucket_base(uint64_t key, uint32_t capacityLog2)
{
    const uint32_t h = hrt_pcg_hash((uint32_t)key + hrt_pcg_hash((uint32_t)(key >> 32)));
    return (uint64_t)(h & ((1u << (capacityLog2 - 5u)) - 1u)) * kBucket;
}

// ---- insert -------------------------------------------------------------------------------------------------------------------------------
// What one sample adds to a channel: a NaN adds 0, a negative value 0, anything above the clamp the clamp.
HRT_FN uint64_t quantise(float L, float radianceScale) { return (uint64_t)hrt_min(hrt_max(L, 0.0f) * radianceScale, kChannelMax); }
// false: the sample takes no part (not valid, or a position or normal that is not finite) and is not counted anywhere.
HRT_FN bool sample_used(const HrptRcacheSample& s) { return s.valid == 1.0f && finite3(s.position) && finite3(s.normal); }
// The walk of a bucket from slot 0: the first slot that was empty (claimed by the CAS) or already holds the key; -1: the bucket is full.
// A is the atomics of the side that runs it: load(p) and cas(p, expected, desired) -> the value found.
template <class A>
HRT_FN int claim_slot(A a, uint64_t* keys, uint64_t base, uint64_t key)
{
    for (uint32_t slot = 0; slot < kBucket; ++slot) {
        uint64_t k = a.load(keys + base + slot);
        if (k == 0ull) k = a.cas(keys + base + slot, 0ull, key);
        if (k == 0ull || k == key) return (int)slot;
    }
    return -1;
}
// ... and of a query: it ends at the first empty slot.
HRT_FN int find_slot(const uint64_t* keys, uint64_t base, uint64_t key)
{
    for (uint32_t slot = 0; slot < kBucket; ++slot) {
        const uint64_t k = keys[base + slot];
        if (k == 0ull) return -1;
        if (k == key) return (int)slot;
    }
    return -1;
}

// ---- resolve ------------------------------------------------------------------------------------------------------------------------------
// One occupied entry after a frame: false = evicted. `e` is updated in place.
HRT_FN bool resolve_entry(const HrptRcacheDesc& d, const HrptRcacheAccum& a, HrptRcacheEntry& e)
{
    uint32_t samples = e.meta & 0xFFFFu, stale = e.meta >> 16;
    if (a.count > 0u) {
        const uint32_t No = samples < d.maxSamples ? samples : d.maxSamples;
        const float fo = (float)No, fn = (float)a.count, den = fo + fn;
        e.r = (e.r * fo + (float)a.r / d.radianceScale) / den;
        e.g = (e.g * fo + (float)a.g / d.radianceScale) / den;
        e.b = (e.b * fo + (float)a.b / d.radianceScale) / den;
        const uint64_t sum = (uint64_t)No + a.count;
        samples = sum < d.maxSamples ? (uint32_t)sum : d.maxSamples;
        stale = 0u;
    } else {
        stale += 1u;
        if (stale > d.staleFramesMax) return false;
    }
    e.meta = samples | stale << 16;
    return true;
}

// ---- query --------------------------------------------------------------------------------------------------------------------------------
// out4 = (resolved.rgb, 1) when the key is present with samples > 0, else zeros; *voxelOut = the voxel size at the point (0 when the point or
// the normal is not finite).
HRT_FN void query(const HrptRcacheDesc& d, const float* cam, const uint64_t* keys, const HrptRcacheEntry* resolved, const HrptRcachePoint& q, float* out4,
                  float* voxelOut)
{
    out4[0] = 0.0f; out4[1] = 0.0f; out4[2] = 0.0f; out4[3] = 0.0f;
    if (voxelOut) *voxelOut = 0.0f;
    if (!finite3(q.position) || !finite3(q.normal)) return;
    const uint64_t key = key_of(d, q.position, q.normal, cam, voxelOut);
    const uint64_t base = bucket_base(key, d.capacityLog2);
    const int slot = find_slot(keys, base, key);
    if (slot < 0) return;
    const HrptRcacheEntry e = resolved[base + (uint64_t)slot];
    if ((e.meta & 0xFFFFu) == 0u) return;
    out4[0] = e.r; out4[1] = e.g; out4[2] = e.b; out4[3] = 1.0f;
}

// ---- the frame calls ----------------------------------------------------------------------------------------------------------------------
// The pixel a sparseBlock x sparseBlock block feeds the cache with this frame: the two PCGHash draws of SHARCUpdate.hlsl:108-121.
HRT_FN void block_pixel(uint32_t bx, uint32_t by, uint32_t block, uint32_t frameIndex, uint32_t* px, uint32_t* py)
{
    *px = bx * block + hrt_pcg_hash(bx ^ (by << 16) ^ frameIndex) % block;
    *py = by * block + hrt_pcg_hash(by ^ (bx << 16) ^ (frameIndex + 1u)) % block;
}
// A pixel of hrpt_rcache_indirect is served when its ray hit, the key was found and the segment spans the voxel (SHARCQuery.hlsl:118-121).
HRT_FN bool served(const HrptRcacheSurface& s, const float* cached4, float voxel) { return s.hit != 0u && cached4[3] == 1.0f && s.t >= voxel; }

} // namespace rcache
} // namespace hrt

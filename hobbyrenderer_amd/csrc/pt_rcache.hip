// pt_rcache.hip -- the gfx950 kernels of the hash-grid radiance cache (hrpt_rcache_*). The arithmetic is pt_rcache.h (shared with the host
// executors of pt_rcache_host.cpp); the diffuse records of the frame calls come from pt_indirect.h. The table is a concurrent hash table in
// HBM: the hot path is atomics, not arithmetic. No scratch; no LDS (the resolve keeps its bucket in the registers of half a wave).
//
//   rcache_insert<COMBINE>   one lane per sample. COMBINE: lanes of a wave with the same key first add their sums into the lowest of them
//                            (one ballot per distinct key; a key only one lane holds costs no reduction), so that neighbouring pixels, which
//                            fall into the same voxel, issue one set of atomics per (wave, key) instead of serialising on one address. Then
//                            the walk of pt_rcache.h claim_slot (64-bit CAS) and up to three 64-bit and one 32-bit atomic add; a zero
//                            channel adds nothing. Integer sums: the table does not depend on COMBINE.
//   rcache_resolve           half a wave per bucket, one lane per slot: key, accumulation and resolved record are read once (56 B), the
//                            survivors are counted by ballot and scattered to their prefix position; a slot is written only where it changes.
//   rcache_query             one lane per point: the key, a walk that ends at the first empty slot, one 16-byte gather.
//   rcache_clear             zeroes the three arrays and the drop counter.
//   rcache_update_rays       one lane per sparse block: the block's pixel and its diffuse record (pt_indirect.h).
//   rcache_gather_samples    (surface, radiance) -> sample record.
//   rcache_serve             one lane per pixel: the served test, the served plane, the untraced record over a served pixel's ray.
//   rcache_apply             one lane per pixel: (cached.rgb, 1) over the diffuse plane where the pixel is served.
#include "pt_device.h"
#include "pt_indirect.h"
#include "pt_kernels.h"
#include "pt_rcache.h"

namespace hrt {

namespace {
using namespace rcache;

struct Cam { float v[3]; };
static Cam cam_of(const float* p) { Cam c; c.v[0] = p[0]; c.v[1] = p[1]; c.v[2] = p[2]; return c; }

struct DeviceAtomics {
    HRT_DEV uint64_t load(uint64_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    HRT_DEV uint64_t cas(uint64_t* p, uint64_t expected, uint64_t desired) const
    {
        return atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expected, (unsigned long long)desired);
    }
};

HRT_DEV unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <bool COMBINE>
__global__ __launch_bounds__(256) void rcache_insert(HrptRcacheDesc d, Cam cam, uint64_t* __restrict__ keys, HrptRcacheAccum* __restrict__ accum,
                                                     unsigned long long* __restrict__ drops, const float4* __restrict__ samples, uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint64_t key = 0ull;
    unsigned long long r = 0ull, g = 0ull, b = 0ull, n = 0ull;
    if (i < count) {                                                   // no early return: the wave's ballots need every lane
        const float4 r0 = samples[i * 3], r1 = samples[i * 3 + 1], r2 = samples[i * 3 + 2];
        HrptRcacheSample s;
        s.position[0] = r0.x; s.position[1] = r0.y; s.position[2] = r0.z; s.valid = r0.w;
        s.normal[0] = r1.x; s.normal[1] = r1.y; s.normal[2] = r1.z; s.pad0 = 0.0f;
        if (sample_used(s)) {
            key = key_of(d, s.position, s.normal, cam.v, nullptr);
            r = quantise(r2.x, d.radianceScale); g = quantise(r2.y, d.radianceScale); b = quantise(r2.z, d.radianceScale); n = 1ull;
        }
    }
    bool writer = key != 0ull;
    if (COMBINE) {
        const int lane = (int)(threadIdx.x & 63u);
        unsigned long long pending = __ballot(key != 0ull);
        while (pending != 0ull) {                                      // wave-uniform: one turn per distinct key of the wave
            const int leader = __ffsll((long long)pending) - 1;
            const uint64_t leaderKey = (uint64_t)__shfl((unsigned long long)key, leader, 64);
            const bool mine = key == leaderKey;
            const unsigned long long match = __ballot(mine);
            if (__popcll(match) > 1) {
                const unsigned long long sr = wave_sum_u64(mine ? r : 0ull), sg = wave_sum_u64(mine ? g : 0ull), sb = wave_sum_u64(mine ? b : 0ull);
                const unsigned long long sn = wave_sum_u64(mine ? n : 0ull);
                if (lane == leader) { r = sr; g = sg; b = sb; n = sn; }
                else if (mine) writer = false;
            }
            pending &= ~match;
        }
    }
    if (!writer) return;
    const uint64_t base = bucket_base(key, d.capacityLog2);
    const int slot = claim_slot(DeviceAtomics(), keys, base, key);
    if (slot < 0) { atomicAdd(drops, n); return; }
    HrptRcacheAccum* a = accum + base + (uint64_t)slot;
    if (r != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(&a->r), r);
    if (g != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(&a->g), g);
    if (b != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(&a->b), b);
    atomicAdd(&a->count, (unsigned int)n);
}

// 256 lanes = 8 buckets of a table whose capacity is a multiple of 1024: every lane has an entry.
__global__ __launch_bounds__(256) void rcache_resolve(HrptRcacheDesc d, uint64_t* __restrict__ keys, uint4* __restrict__ accum, uint4* __restrict__ resolved)
{
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t l = threadIdx.x & 31u;
    const uint64_t key = keys[e];
    const uint4 a0 = accum[e * 2], a1 = accum[e * 2 + 1];
    HrptRcacheAccum a;
    a.r = (uint64_t)a0.x | (uint64_t)a0.y << 32; a.g = (uint64_t)a0.z | (uint64_t)a0.w << 32; a.b = (uint64_t)a1.x | (uint64_t)a1.y << 32; a.count = a1.z; a.pad = a1.w;
    HrptRcacheEntry ent; ent.r = 0.0f; ent.g = 0.0f; ent.b = 0.0f; ent.meta = 0u;
    bool survive = false;
    if (key != 0ull) {
        const uint4 v = resolved[e];
        ent.r = __uint_as_float(v.x); ent.g = __uint_as_float(v.y); ent.b = __uint_as_float(v.z); ent.meta = v.w;
        survive = resolve_entry(d, a, ent);
    }
    // every load above feeds the ballot or a store of this lane, so the wave has read its two buckets before any lane writes
    const unsigned long long ballot = __ballot(survive);
    const uint32_t mask = (uint32_t)(ballot >> (threadIdx.x & 32u));
    const uint32_t dest = (uint32_t)__popc(mask & ((1u << l) - 1u)), survivors = (uint32_t)__popc(mask);
    const uint64_t base = e - l;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if ((a0.x | a0.y | a0.z | a0.w | a1.x | a1.y | a1.z | a1.w) != 0u) { accum[e * 2] = zero; accum[e * 2 + 1] = zero; }
    if (survive) {
        if (dest != l) keys[base + dest] = key;
        resolved[base + dest] = make_uint4(__float_as_uint(ent.r), __float_as_uint(ent.g), __float_as_uint(ent.b), ent.meta);
    }
    if (l >= survivors && key != 0ull) { keys[e] = 0ull; resolved[e] = zero; }
}

// `in`: records with the position in floats 0..2 and the normal in floats 4..6, `stride4` float4 rows apart (HrptRcachePoint: 2, HrptRcacheSurface: 3).
__global__ __launch_bounds__(256) void rcache_query(HrptRcacheDesc d, Cam cam, const uint64_t* __restrict__ keys, const HrptRcacheEntry* __restrict__ resolved,
                                                    const float4* __restrict__ in, uint32_t stride4, float4* __restrict__ out, float* __restrict__ voxelOut,
                                                    uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const float4 r0 = in[i * stride4], r1 = in[i * stride4 + 1];
    HrptRcachePoint q;
    q.position[0] = r0.x; q.position[1] = r0.y; q.position[2] = r0.z; q.pad0 = 0.0f;
    q.normal[0] = r1.x; q.normal[1] = r1.y; q.normal[2] = r1.z; q.pad1 = 0.0f;
    float o[4], voxel;
    query(d, cam.v, keys, resolved, q, o, &voxel);
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
    if (voxelOut) voxelOut[i] = voxel;
}

__global__ __launch_bounds__(256) void rcache_clear(uint4* __restrict__ keys2, uint4* __restrict__ accum, uint4* __restrict__ resolved,
                                                    unsigned long long* __restrict__ drops, uint64_t entries)
{
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < entries; e += (uint64_t)gridDim.x * 256u) {
        if ((e & 1u) == 0u) keys2[e >> 1] = zero;
        accum[e * 2] = zero; accum[e * 2 + 1] = zero;
        resolved[e] = zero;
    }
    if (drops && blockIdx.x == 0 && threadIdx.x == 0) *drops = 0ull;
}

__global__ __launch_bounds__(256) void rcache_update_rays(indirect::Frame f, uint32_t block, uint32_t blocksX, uint32_t blocksY, uint32_t frameIndex,
                                                          float roughnessThreshold, const float4* __restrict__ normal, const float4* __restrict__ geoNormal,
                                                          const float4* __restrict__ depth, float4* __restrict__ rays)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= blocksX * blocksY) return;
    uint32_t px, py;
    block_pixel(i % blocksX, i / blocksX, block, frameIndex, &px, &py);
    bool traced = false;
    indirect::Draws p = {};
    f3 dir = mk3(0.0f, 0.0f, 0.0f);
    if (px < (uint32_t)f.w && py < (uint32_t)f.h) {
        const size_t idx = (size_t)py * (size_t)f.w + px;
        const float4 D = depth[idx], N4 = normal[idx];
        if (!(D.x == img::kMissDepth) && !(N4.w < roughnessThreshold)) {
            p = indirect::pixel_draws(f, (int)px, (int)py, D.x);
            traced = indirect::diffuse_lobe(p, mk3(N4.x, N4.y, N4.z), geoNormal[idx].w, dir);
        }
    }
    img::T4 rows[3];
    indirect::ray_rows(traced, p.X, dir, p.s, rows);
    for (int k = 0; k < 3; ++k) rays[(size_t)i * 3 + k] = make_float4(rows[k].x, rows[k].y, rows[k].z, rows[k].w);
}

__global__ __launch_bounds__(256) void rcache_gather_samples(const HrptRcacheSurface* __restrict__ surfaces, const float4* __restrict__ radiance,
                                                             float4* __restrict__ samples, uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const HrptRcacheSurface s = surfaces[i];
    const float4 L = radiance[i];
    samples[i * 3] = make_float4(s.position[0], s.position[1], s.position[2], (s.hit != 0u && L.w == 1.0f) ? 1.0f : 0.0f);
    samples[i * 3 + 1] = make_float4(s.normal[0], s.normal[1], s.normal[2], 0.0f);
    samples[i * 3 + 2] = make_float4(L.x, L.y, L.z, 0.0f);
}

__global__ __launch_bounds__(256) void rcache_serve(const HrptRcacheSurface* __restrict__ surfaces, const float4* __restrict__ cached, const float* __restrict__ voxel,
                                                    float4* __restrict__ servedOut, float4* __restrict__ rays, uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const HrptRcacheSurface s = surfaces[i];
    const float4 c = cached[i];
    const float c4[4] = { c.x, c.y, c.z, c.w };
    const bool sv = served(s, c4, voxel[i]);
    servedOut[i] = sv ? make_float4(c.x, c.y, c.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (sv) {
        img::T4 rows[3];
        indirect::ray_rows(false, mk3(0.0f, 0.0f, 0.0f), mk3(0.0f, 0.0f, 0.0f), 0u, rows);
        for (int k = 0; k < 3; ++k) rays[i * 3 + k] = make_float4(rows[k].x, rows[k].y, rows[k].z, rows[k].w);
    }
}

__global__ __launch_bounds__(256) void rcache_apply(const float4* __restrict__ servedPlane, float4* __restrict__ diffuse, uint64_t count)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const float4 s = servedPlane[i];
    if (s.w == 1.0f) diffuse[i] = s;
}

unsigned blocks_of(uint64_t count) { return (unsigned)((count + 255u) / 256u); }
} // namespace

hipError_t launch_rcache_insert(const HrptRcacheDesc& desc, const float* cameraPos, uint64_t* keys, HrptRcacheAccum* accum, uint64_t* drops,
                                const HrptRcacheSample* samples, uint64_t count, bool waveCombine, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    auto* dr = reinterpret_cast<unsigned long long*>(drops);
    auto* sm = reinterpret_cast<const float4*>(samples);
    if (waveCombine) hipLaunchKernelGGL(rcache_insert<true>, dim3(blocks_of(count)), dim3(256), 0, stream, desc, cam_of(cameraPos), keys, accum, dr, sm, count);
    else hipLaunchKernelGGL(rcache_insert<false>, dim3(blocks_of(count)), dim3(256), 0, stream, desc, cam_of(cameraPos), keys, accum, dr, sm, count);
    return hipGetLastError();
}

hipError_t launch_rcache_resolve(const HrptRcacheDesc& desc, uint64_t* keys, HrptRcacheAccum* accum, HrptRcacheEntry* resolved, hipStream_t stream)
{
    hipLaunchKernelGGL(rcache_resolve, dim3((unsigned)(rcache::capacity(desc) / 256u)), dim3(256), 0, stream, desc, keys, reinterpret_cast<uint4*>(accum),
                       reinterpret_cast<uint4*>(resolved));
    return hipGetLastError();
}

hipError_t launch_rcache_query(const HrptRcacheDesc& desc, const float* cameraPos, const uint64_t* keys, const HrptRcacheEntry* resolved, const void* records,
                               uint32_t recordBytes, float* out4, float* voxelOut, uint64_t count, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rcache_query, dim3(blocks_of(count)), dim3(256), 0, stream, desc, cam_of(cameraPos), keys, resolved, static_cast<const float4*>(records),
                       recordBytes / 16u, reinterpret_cast<float4*>(out4), voxelOut, count);
    return hipGetLastError();
}

hipError_t launch_rcache_clear(const HrptRcacheDesc& desc, uint64_t* keys, HrptRcacheAccum* accum, HrptRcacheEntry* resolved, uint64_t* drops, hipStream_t stream)
{
    const uint64_t entries = rcache::capacity(desc);
    const unsigned blocks = entries / 256u > 4096u ? 4096u : (unsigned)(entries / 256u);
    hipLaunchKernelGGL(rcache_clear, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<uint4*>(keys), reinterpret_cast<uint4*>(accum),
                       reinterpret_cast<uint4*>(resolved), reinterpret_cast<unsigned long long*>(drops), entries);
    return hipGetLastError();
}

hipError_t launch_rcache_update_rays(const indirect::Frame& frame, const HrptRcacheDesc& desc, uint32_t frameIndex, const float* normal, const float* geoNormal,
                                     const float* depth, HrptRay* rays, hipStream_t stream)
{
    const uint32_t B = desc.sparseBlock, bx = ((uint32_t)frame.w + B - 1u) / B, by = ((uint32_t)frame.h + B - 1u) / B;
    hipLaunchKernelGGL(rcache_update_rays, dim3(blocks_of((uint64_t)bx * by)), dim3(256), 0, stream, frame, B, bx, by, frameIndex, desc.roughnessThreshold,
                       reinterpret_cast<const float4*>(normal), reinterpret_cast<const float4*>(geoNormal), reinterpret_cast<const float4*>(depth),
                       reinterpret_cast<float4*>(rays));
    return hipGetLastError();
}

hipError_t launch_rcache_gather_samples(const HrptRcacheSurface* surfaces, const float4* radiance, HrptRcacheSample* samples, uint64_t count, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(rcache_gather_samples, dim3(blocks_of(count)), dim3(256), 0, stream, surfaces, radiance, reinterpret_cast<float4*>(samples), count);
    return hipGetLastError();
}

hipError_t launch_rcache_serve(const HrptRcacheSurface* surfaces, const float4* cached, const float* voxel, float4* servedOut, HrptRay* rays, uint64_t count,
                               hipStream_t stream)
{
    hipLaunchKernelGGL(rcache_serve, dim3(blocks_of(count)), dim3(256), 0, stream, surfaces, cached, voxel, servedOut, reinterpret_cast<float4*>(rays), count);
    return hipGetLastError();
}

hipError_t launch_rcache_apply(const float4* servedPlane, float4* diffuse, uint64_t count, hipStream_t stream)
{
    hipLaunchKernelGGL(rcache_apply, dim3(blocks_of(count)), dim3(256), 0, stream, servedPlane, diffuse, count);
    return hipGetLastError();
}

} // namespace hrt

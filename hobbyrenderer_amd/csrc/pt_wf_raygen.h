// pt_wf_raygen.h -- the two ends of a batch: wf_store_primary (PrimaryArgs into the queue pool for batches without a raygen pass), wf_raygen
// (one path record per pixel of the rectangle and accumulation index, sampleRadiance zeroed) and wf_resolve (folds the indices of a pixel in
// order into Accumulation and Output); for hrpt_trace_radiance wf_raygen_rays (one path record per ray of the caller) and wf_store_radiance
// (sampleRadiance into the caller's array). A piece of pt_wavefront.hip, included there after pt_wf_common.h: no stand-alone header.

// PrimaryArgs into the queue pool (the kernels index its jitter table per lane: a by-value kernel argument would be copied to scratch for that)
__global__ void wf_store_primary(PrimaryArgs pr, PrimaryArgs* dst)
{
    if (threadIdx.x < 16) dst->clipToWorld[threadIdx.x] = pr.clipToWorld[threadIdx.x];
    if (threadIdx.x < 3) dst->cam[threadIdx.x] = pr.cam[threadIdx.x];
    if (threadIdx.x == 0) { dst->invW = pr.invW; dst->invH = pr.invH; dst->accumIndex = pr.accumIndex; }
    if (threadIdx.x < kMaxSppPerBatch) dst->j[threadIdx.x] = pr.j[threadIdx.x];
}

// ------------------------------------------------------------------ raygen
__global__ __launch_bounds__(kBlock) void wf_raygen(WfArgs a, HrptPathTracerConstants cb, JitterTable jt)
{
    const uint32_t wavesPerBlock = kBlock / 64, lane = lane_id();
    const uint32_t gw = uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), totalWaves = gridDim.x * wavesPerBlock;
    unsigned int nPaths = 0;
    for (uint32_t seg = gw; seg < a.numSegments; seg += totalWaves) {
        uint32_t segBase = seg * a.segSize, outCount = 0;
        for (uint32_t base = 0; base < a.segSize; base += 64) {
            uint32_t smp = segBase + base + lane;
            const bool mine = base + lane < a.segSize && smp < a.numSamples;      // (a segment need not be a multiple of 64 samples)
            bool active = mine;
            uint32_t k = 0, px = 0, py = 0;
            if (active) {
                k = smp / a.pixelsPadded;
                uint32_t p = smp - k * a.pixelsPadded;
                uint32_t tile = p >> 6, within = p & 63u;
                uint32_t tcol, trow; tile_position(a, tile, tcol, trow);
                px = a.rect.column_x(tcol) + (within & 7u);
                py = a.rect.y0 + trow * 8u + (within >> 3);
                active = px < a.rect.x1 && py < a.rect.y1;
            }
            if (mine) a.b.radiance[smp] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            unsigned long long m = __ballot(active);
            if (active) {
                PathState ps;
                // camera_ray (pt_direct.h) with the jitter / RNG stream of accumulation index first+k (PathTracerRenderer.cpp:62,:65)
                camera_ray(cb.m_View.m_MatClipToWorldNoOffset, cb.m_CameraPos, jt.j[k].x, jt.j[k].y, cb.m_View.m_ViewportSizeInv[0],
                           cb.m_View.m_ViewportSizeInv[1], px, py, ps.ray.o, ps.ray.d);
                ps.rng = hrt_rng_seed(px, py, cb.m_AccumulationIndex + k);
                uint32_t o = segBase + outCount + prefix_rank(m);
                a.b.rayO[0][o] = make_float4(ps.ray.o.x, ps.ray.o.y, ps.ray.o.z, 0.0f);
                a.b.rayD[0][o] = make_float4(ps.ray.d.x, ps.ray.d.y, ps.ray.d.z, __uint_as_float(ps.rng));
                a.b.thr[0][o] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(smp));
                if (a.hasMedium) {
                    a.b.med0[0][o] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
                    a.b.med1[0][o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
                ++nPaths;
            }
            outCount += (uint32_t)__popcll(m);
        }
        if (lane == 0) a.b.pathCnt[0][seg] = outCount;
    }
    block_count_add(&a.counters->closestRays, 2, nPaths);
}

// ------------------------------------------------------------------ the caller's rays (hrpt_trace_radiance)
// wf_raygen over a batch of HrptRay records instead of the pixel grid: sample smp is path segment 0 of rays[smp] (origin, direction as given,
// tmin, RNG state; tmax is not read: the first segment is unbounded like a camera ray's). A record with a non-finite origin, direction or tmin
// gets no path; its radiance slot carries a set sign bit in w (nothing downstream touches w), which is all wf_store_radiance needs to tell it
// from a traced sample. `rays` is the batch's first record, read as three 16-byte words. Paths are not counted: HrptStats describes renders.
__global__ __launch_bounds__(kBlock) void wf_raygen_rays(WfArgs a, const float4* __restrict__ rays)
{
    const uint32_t wavesPerBlock = kBlock / 64, lane = lane_id();
    const uint32_t gw = uniform(blockIdx.x * wavesPerBlock + (threadIdx.x >> 6)), totalWaves = gridDim.x * wavesPerBlock;
    for (uint32_t seg = gw; seg < a.numSegments; seg += totalWaves) {
        uint32_t segBase = seg * a.segSize, outCount = 0;
        for (uint32_t base = 0; base < a.segSize; base += 64) {
            const uint32_t smp = segBase + base + lane;
            const bool mine = base + lane < a.segSize && smp < a.numSamples;
            bool active = false;
            float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
            if (mine) {
                const float4* rec = rays + (size_t)smp * 3;
                r0 = rec[0]; r1 = rec[1]; r2 = rec[2];
                active = all_finite(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z)) && (r0.w - r0.w) == 0.0f;
                a.b.radiance[smp] = make_float4(0.0f, 0.0f, 0.0f, active ? 0.0f : -0.0f);
            }
            const unsigned long long m = __ballot(active);
            if (active) {
                const uint32_t o = segBase + outCount + prefix_rank(m);
                a.b.rayO[0][o] = r0;                                              // {origin, tmin}
                a.b.rayD[0][o] = make_float4(r1.x, r1.y, r1.z, r2.x);             // {direction, RNG state}
                a.b.thr[0][o] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(smp));
                if (a.hasMedium) {
                    a.b.med0[0][o] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
                    a.b.med1[0][o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
            outCount += (uint32_t)__popcll(m);
        }
        if (lane == 0) a.b.pathCnt[0][seg] = outCount;
    }
}

// The back end of hrpt_trace_radiance: sampleRadiance of the batch to the caller's array by store_ray_radiance (pt_path.h), `out` being the
// batch's first slot.
__global__ __launch_bounds__(kBlock) void wf_store_radiance(WfArgs a, float4* __restrict__ out, uint32_t accumulate)
{
    uint32_t smp = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (; smp < a.numSamples; smp += stride) {
        const float4 r = a.b.radiance[smp];
        store_ray_radiance(out + smp, mk3(r.x, r.y, r.z), (__float_as_uint(r.w) >> 31) == 0u, accumulate != 0u);
    }
}

// ------------------------------------------------------------------ resolve: fold the indices in order (:332-339)
__global__ __launch_bounds__(kBlock) void wf_resolve(WfArgs a, float4* __restrict__ accumulation, float4* __restrict__ output, uint32_t firstIndex)
{
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t stride = gridDim.x * blockDim.x;
    for (; p < a.pixelsPadded; p += stride) {
        uint32_t tile = p >> 6, within = p & 63u;
        uint32_t tcol, trow; tile_position(a, tile, tcol, trow);
        uint32_t px = a.rect.column_x(tcol) + (within & 7u), py = a.rect.y0 + trow * 8u + (within >> 3);
        if (px >= a.rect.x1 || py >= a.rect.y1) continue;
        size_t idx = (size_t)py * a.imageWidth + px;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (uint32_t k = 0; k < a.spp; ++k) {
            float4 r = a.b.radiance[(size_t)k * a.pixelsPadded + p];
            float4 cur = make_float4(r.x, r.y, r.z, 1.0f);
            if (firstIndex + k > 0) {
                float4 prev = (k == 0) ? accumulation[idx] : acc;
                cur.x += prev.x; cur.y += prev.y; cur.z += prev.z; cur.w += prev.w;
            }
            acc = cur;
        }
        accumulation[idx] = acc;
        output[idx] = make_float4(acc.x / acc.w, acc.y / acc.w, acc.z / acc.w, 1.0f);
    }
}
